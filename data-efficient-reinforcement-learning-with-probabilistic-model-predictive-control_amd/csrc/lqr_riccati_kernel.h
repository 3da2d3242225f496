// lqr_riccati_kernel.h -- the two kernels gpmpc_lqr_gains (lqr_gains.hip) and the backward sweep of gpmpc_ilqr_* (ilqr.hip) share:
//   lqr_inputs_kernel            one thread per (candidate, model input): the model inputs of step t (t = 0: from mu0; else mu += M),
//                                and, where asked for, the stored nominal trajectory (index t; t = H: the last state alone).
//   lqr_riccati_kernel<AFFINE>   one wavefront per candidate, lanes over matrix elements, every matrix in LDS with an odd row pitch:
//                                the backward Riccati sweep
//                                  F = P_{t+1} A_t,  Huu = R + B_t^T P_{t+1} B_t + reg I,  Hux = N^T + B_t^T F,  K_t = -Huu^-1 Hux,
//                                  P_t = Q + A_t^T F + Hux^T K_t
//                                with the A x A Cholesky factorisation on the wavefront (A <= 8 dependent pivots) and the two
//                                triangular solves one column of Hux per lane.  The next step's V rides in registers under the
//                                algebra.  AFFINE (the iLQR): `reg` is read per candidate, and the affine half of the sweep rides
//                                along on D- and A-vectors in LDS
//                                  p_H = P_H e_H,  q = W_s e_t,  g_x = q_x + A_t^T p_{t+1},  g_u = q_u + B_t^T p_{t+1},
//                                  k_t = -Huu^-1 g_u (one more right-hand side of the two solves, on lane D),  p_t = g_x + Hux^T k_t,
//                                  dV = sum_t g_u^T k_t / (H + 1),  step = max |clip(ubar_t + k_t, 0, 1) - ubar_t|.
//                                The AFFINE form adds statements and changes none: K_t and P_t take the same operations in the
//                                same order in both forms.
// Every sum runs in an order fixed by E, D, A and H alone.
#pragma once
#include "device_common.h"
#include "lqr_gains_plan.h"

namespace gpmpc_hip {

namespace {

constexpr int kPD = kMaxD + 1;           // LDS row pitch (doubles) of a matrix with up to D columns: odd, so that a walk down a
constexpr int kPA = kLqrMaxA + 1;        // column and a walk along a row both spread over the banks
constexpr int kVRegs = (kMaxD + kLqrMaxA) * kMaxD / kWave;      // V values a lane carries from one step to the next
static_assert(kVRegs * kWave >= (kMaxD + kLqrMaxA) * kMaxD, "lqr_riccati_kernel: V values per lane");

struct LqrInputArgs {
    const double* actions;   // (rows, H, A) of this chunk
    const double* M;         // (rows, D) of the step before
    double* Xq;              // (rows, E)
    double* mu;              // (rows, H + 1, D) of this chunk: the nominal trajectory, or NULL
    int rows, E, D, A, H, t, include_time;
    double time0;
    double mu0[kMaxD];
};

struct LqrRiccatiArgs {
    const double* V;         // (H, rows, E, D) of this chunk
    const double* cost;      // target (D + A) | W (D + A)^2 | W_T D^2 | ...
    double* gains;           // (rows, H, A, D) of this chunk
    double* P;               // (rows, H + 1, D, D) of this chunk, or NULL
    int* flags;              // (rows) of this chunk, or NULL
    int rows, E, D, A, H;
    double reg;
    // AFFINE only
    const double* reg_dev;   // (rows)
    const double* status;    // (rows), or NULL: a candidate whose status != 0 is left alone
    const double* mu;        // (rows, H + 1, D) the nominal trajectory
    const double* actions;   // (rows, H, A)
    double* ff;              // (rows, H, A)
    double* dV;              // each: element b at [b * info_stride]
    double* step;
    double* fflags;          // the lost pivots, as a double
    double* reserved;        // set to 0, or NULL
    int info_stride;
};

// The model inputs of step t: the state entries advance by the mean of the step before (the operation of
// rollout_linear_step_kernel, moments_linear_kernels.h: the same bits), the action and time entries are set.  t = H (only with
// `mu`): the last state of the stored trajectory, no model input.
__global__ __launch_bounds__(256) void lqr_inputs_kernel(LqrInputArgs p) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)p.rows * p.E) return;
    const int b = (int)(idx / p.E), e = (int)(idx - (long long)b * p.E);
    double* xq = p.Xq + (size_t)b * p.E;
    if (e < p.D) {
        xq[e] = p.t == 0 ? p.mu0[e] : xq[e] + p.M[(size_t)b * p.D + e];
        if (p.mu) p.mu[((size_t)b * (p.H + 1) + p.t) * p.D + e] = xq[e];
    } else if (p.t == p.H) {
        return;
    } else if (e < p.D + p.A) xq[e] = p.actions[((size_t)b * p.H + p.t) * p.A + (e - p.D)];
    else xq[e] = p.time0 + (double)p.t;              // (only with include_time: E = D + A + 1)
}

// One wavefront per candidate: the backward Riccati sweep.
template <bool AFFINE>
__global__ __launch_bounds__(64) void lqr_riccati_kernel(LqrRiccatiArgs p) {
    __shared__ double s_Q[kMaxD][kPD];               // W_s, state block
    __shared__ double s_N[kMaxD][kPA];               // W_s, state x action block
    __shared__ double s_R[kLqrMaxA][kPA];            // W_s, action block
    __shared__ double s_A[kMaxD][kPD];               // A_t = I + V_s^T
    __shared__ double s_B[kMaxD][kPA];               // B_t = V_u^T
    __shared__ double s_P[kMaxD][kPD];               // P_{t+1}, then P_t
    __shared__ double s_F[kMaxD][kPD];               // P_{t+1} A_t
    __shared__ double s_G[kMaxD][kPA];               // P_{t+1} B_t
    __shared__ double s_Hux[kLqrMaxA][kPD];
    __shared__ double s_Huu[kLqrMaxA][kPA];          // Huu, then its Cholesky factor below the diagonal
    __shared__ double s_K[kLqrMaxA][kPD];            // K_t [action][state]
    __shared__ double s_diag[kLqrMaxA];              // the factor's diagonal
    [[maybe_unused]] __shared__ double s_e[AFFINE ? kMaxD + kLqrMaxA : 1];       // AFFINE: e_t = [x_t | u_t] - target
    [[maybe_unused]] __shared__ double s_p[AFFINE ? kMaxD : 1];                  // p_{t+1}, then p_t
    [[maybe_unused]] __shared__ double s_gx[AFFINE ? kMaxD : 1];
    [[maybe_unused]] __shared__ double s_gu[AFFINE ? kLqrMaxA : 1];
    [[maybe_unused]] __shared__ double s_k[AFFINE ? kLqrMaxA : 1];               // k_t
    const int b = blockIdx.x, tid = threadIdx.x;
    const int D = p.D, A = p.A, E = p.E, H = p.H, DA = D + A;
    if constexpr (AFFINE) {
        if (p.status && p.status[b] != 0.0) return;                  // (uniform) a finished candidate: its state no longer changes
    }
    const double* W = p.cost + DA;
    const double* WT = W + DA * DA;
    double* Pb = p.P ? p.P + (size_t)b * (H + 1) * D * D : nullptr;
    double* Kb = p.gains + (size_t)b * H * A * D;
    double reg = p.reg;
    if constexpr (AFFINE) reg = p.reg_dev[b];

    for (int idx = tid; idx < DA * DA; idx += 64) {                  // W_s = (W + W^T) / 2 by blocks
        const int i = idx / DA, j = idx - i * DA;
        const double w = 0.5 * (W[i * DA + j] + W[j * DA + i]);
        if (i < D && j < D) s_Q[i][j] = w;
        else if (i < D) s_N[i][j - D] = w;
        else if (j >= D) s_R[i - D][j - D] = w;
    }
    for (int idx = tid; idx < D * D; idx += 64) {                    // P_H = (W_T + W_T^T) / 2
        const int i = idx / D, j = idx - i * D;
        const double w = 0.5 * (WT[i * D + j] + WT[j * D + i]);
        s_P[i][j] = w;
        if (Pb) Pb[(size_t)H * D * D + idx] = w;
    }
    [[maybe_unused]] const double* mub = nullptr;
    [[maybe_unused]] const double* ub = nullptr;
    [[maybe_unused]] double dV = 0.0, stepmax = 0.0;
    if constexpr (AFFINE) {                                          // p_H = P_H e_H
        mub = p.mu + (size_t)b * (H + 1) * D;
        ub = p.actions + (size_t)b * H * A;
        if (tid < D) s_e[tid] = mub[(size_t)H * D + tid] - p.cost[tid];
        wave_lds_sync();
        if (tid < D) {
            double v = 0.0;
            for (int j = 0; j < D; ++j) v = fma(s_P[tid][j], s_e[j], v);
            s_p[tid] = v;
        }
    }
    double vreg[kVRegs];
    auto load_v = [&](int t) {                                       // the D + A kept rows of step t's V: (e, a) = idx / D, idx % D
        const double* Vt = p.V + ((size_t)t * p.rows + b) * E * D;
#pragma unroll
        for (int q = 0; q < kVRegs; ++q) {
            const int idx = tid + 64 * q;
            vreg[q] = idx < DA * D ? Vt[idx] : 0.0;
        }
    };
    load_v(H - 1);
    int failed = 0;
    for (int t = H - 1; t >= 0; --t) {
        wave_lds_sync();                                             // the step before has read s_A / s_B; s_P is written
#pragma unroll
        for (int q = 0; q < kVRegs; ++q) {
            const int idx = tid + 64 * q;
            if (idx < DA * D) {
                const int e = idx / D, a = idx - e * D;              // V[e][a] = dM_a / dm_e
                if (e < D) s_A[a][e] = (a == e) ? 1.0 + vreg[q] : vreg[q];
                else s_B[a][e - D] = vreg[q];
            }
        }
        if constexpr (AFFINE) {
            if (tid < D) s_e[tid] = mub[(size_t)t * D + tid] - p.cost[tid];
            else if (tid < DA) s_e[tid] = ub[(size_t)t * A + (tid - D)] - p.cost[tid];
        }
        wave_lds_sync();
        if (t > 0) load_v(t - 1);                                    // in flight under this step's algebra
        for (int idx = tid; idx < D * D; idx += 64) {                // F = P A
            const int i = idx / D, j = idx - i * D;
            double f = 0.0;
            for (int k = 0; k < D; ++k) f = fma(s_P[i][k], s_A[k][j], f);
            s_F[i][j] = f;
        }
        for (int idx = tid; idx < D * A; idx += 64) {                // G = P B
            const int i = idx / A, u = idx - i * A;
            double g = 0.0;
            for (int k = 0; k < D; ++k) g = fma(s_P[i][k], s_B[k][u], g);
            s_G[i][u] = g;
        }
        if constexpr (AFFINE) {
            if (tid < D) {                                           // g_x = Q e_x + N e_u + A^T p
                double g = 0.0;
                for (int j = 0; j < D; ++j) g = fma(s_Q[tid][j], s_e[j], g);
                for (int u = 0; u < A; ++u) g = fma(s_N[tid][u], s_e[D + u], g);
                for (int k = 0; k < D; ++k) g = fma(s_A[k][tid], s_p[k], g);
                s_gx[tid] = g;
            } else if (tid < DA) {                                   // g_u = N^T e_x + R e_u + B^T p
                const int u = tid - D;
                double g = 0.0;
                for (int j = 0; j < D; ++j) g = fma(s_N[j][u], s_e[j], g);
                for (int v = 0; v < A; ++v) g = fma(s_R[u][v], s_e[D + v], g);
                for (int k = 0; k < D; ++k) g = fma(s_B[k][u], s_p[k], g);
                s_gu[u] = g;
            }
        }
        wave_lds_sync();
        for (int idx = tid; idx < A * A; idx += 64) {                // Huu = R + B^T G + reg I for i <= j, mirrored
            const int i = idx / A, j = idx - i * A;
            if (i > j) continue;
            double h = s_R[i][j];
            for (int k = 0; k < D; ++k) h = fma(s_B[k][i], s_G[k][j], h);
            if (i == j) h += reg;
            s_Huu[i][j] = h;
            s_Huu[j][i] = h;
        }
        for (int idx = tid; idx < A * D; idx += 64) {                // Hux = N^T + B^T F
            const int u = idx / D, j = idx - u * D;
            double h = s_N[j][u];
            for (int k = 0; k < D; ++k) h = fma(s_B[k][u], s_F[k][j], h);
            s_Hux[u][j] = h;
        }
        wave_lds_sync();
        // Huu = L L^T, right-looking; the pivot is read by every lane (a broadcast), so the branch is uniform
        bool ok = true;
        for (int k = 0; k < A; ++k) {
            const double d = s_Huu[k][k];
            if (!(d > 0.0) || !(d <= 1.79769313486231570815e308)) { ok = false; break; }
            const double l = sqrt(d);
            wave_lds_sync();                                         // every lane holds the pivot before column k is scaled
            if (tid == 0) s_diag[k] = l;
            if (tid > k && tid < A) s_Huu[tid][k] = s_Huu[tid][k] / l;
            wave_lds_sync();
            for (int idx = tid; idx < A * A; idx += 64) {
                const int i = idx / A, j = idx - i * A;
                if (j > k && i >= j) s_Huu[i][j] = fma(-s_Huu[i][k], s_Huu[j][k], s_Huu[i][j]);
            }
            wave_lds_sync();
        }
        if (ok) {
            const bool rhs_ff = AFFINE && tid == D;                  // AFFINE: lane D solves for k_t
            if (tid < D || rhs_ff) {                                 // one column of Hux per lane: L y = Hux, L^T x = y, K = -x
                double y[kLqrMaxA];
#pragma unroll
                for (int i = 0; i < kLqrMaxA; ++i) {
                    y[i] = 0.0;
                    if (i < A) {
                        double s = rhs_ff ? s_gu[AFFINE ? i : 0] : s_Hux[i][tid];
#pragma unroll
                        for (int k = 0; k < i; ++k) s = fma(-s_Huu[i][k], y[k], s);
                        y[i] = s / s_diag[i];
                    }
                }
#pragma unroll
                for (int i = kLqrMaxA - 1; i >= 0; --i) {
                    if (i < A) {
                        double s = y[i];
#pragma unroll
                        for (int k = i + 1; k < kLqrMaxA; ++k)
                            if (k < A) s = fma(-s_Huu[k][i], y[k], s);
                        y[i] = s / s_diag[i];
                    }
                }
#pragma unroll
                for (int i = 0; i < kLqrMaxA; ++i)
                    if (i < A) {
                        if (rhs_ff) s_k[AFFINE ? i : 0] = 0.0 - y[i];
                        else s_K[i][tid] = 0.0 - y[i];
                    }
            }
        } else {
            ++failed;                                                // a lost pivot: K_t = 0, P_t = sym(Q + A^T F)
            for (int idx = tid; idx < A * D; idx += 64) s_K[idx / D][idx % D] = 0.0;
            if constexpr (AFFINE) {
                if (tid < A) s_k[tid] = 0.0;                         // ... k_t = 0, p_t = g_x
            }
        }
        wave_lds_sync();
        for (int idx = tid; idx < A * D; idx += 64) Kb[(size_t)t * A * D + idx] = s_K[idx / D][idx % D];
        for (int idx = tid; idx < D * D; idx += 64) {                // P_t = Q + A^T F + Hux^T K for i <= j, mirrored
            const int i = idx / D, j = idx - i * D;
            if (i > j) continue;
            double v = s_Q[i][j];
            for (int k = 0; k < D; ++k) v = fma(s_A[k][i], s_F[k][j], v);
            if (ok)
                for (int u = 0; u < A; ++u) v = fma(s_Hux[u][i], s_K[u][j], v);
            s_P[i][j] = v;
            s_P[j][i] = v;
            if (Pb) {
                Pb[((size_t)t * D + i) * D + j] = v;
                Pb[((size_t)t * D + j) * D + i] = v;
            }
        }
        if constexpr (AFFINE) {
            if (tid < D) {                                           // p_t = g_x + Hux^T k_t
                double v = s_gx[tid];
                if (ok)
                    for (int u = 0; u < A; ++u) v = fma(s_Hux[u][tid], s_k[u], v);
                s_p[tid] = v;
            }
            if (tid < A) {
                const double kv = s_k[tid], uv = ub[(size_t)t * A + tid], un = uv + kv;
                p.ff[((size_t)b * H + t) * A + tid] = kv;
                const double uc = un < 0.0 ? 0.0 : (un > 1.0 ? 1.0 : un);
                stepmax = fmax(stepmax, fabs(uc - uv));
            }
            for (int u = 0; u < A; ++u) dV = fma(s_gu[u], s_k[u], dV);       // every lane the same sum, the actions in order
        }
    }
    if (p.flags && tid == 0) p.flags[b] = failed;
    if constexpr (AFFINE) {
        for (int off = 32; off >= 1; off >>= 1) stepmax = fmax(stepmax, __shfl_xor(stepmax, off, 64));
        if (tid == 0) {
            const size_t o = (size_t)b * p.info_stride;
            p.dV[o] = dV / (double)(H + 1);
            p.step[o] = stepmax;
            p.fflags[o] = (double)failed;
            if (p.reserved) p.reserved[o] = 0.0;
        }
    }
}

}  // namespace

}  // namespace gpmpc_hip
