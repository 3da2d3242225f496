// lqr_gains.hip -- the LQR feedback gains of the linearisation along every candidate's nominal trajectory (gpmpc_lqr_gains): the
// gains K_t that gpmpc_rollout_linear_feedback takes as given.  Per candidate and step t the model input is
// [mu_t | ubar_t | time0 + t], mu_0 = mu0, mu_{t+1} = mu_t + M, with M and the mean Jacobian V (E x D) of gpmpc_moments_linear at
// that input; no covariance enters and no K* iK product runs.  With V_s / V_u the state / action rows of V,
//   A_t = I + V_s^T (D x D),   B_t = V_u^T (D x A)
// and, on the symmetric part W_s of the loaded stage weight (Q | N ; N^T | R) and P_H = sym(W_T), for t = H-1 .. 0
//   F = P_{t+1} A_t,  Huu = R + B_t^T P_{t+1} B_t + reg I,  Hux = N^T + B_t^T F,  K_t = -Huu^-1 Hux,  P_t = Q + A_t^T F + Hux^T K_t.
//
// Structure ("LQR gains"):
//   lqr_inputs_kernel     one thread per (candidate, model input): the model inputs of step t (t = 0: from mu0; else mu += M).
//   run_moments_linear    per step, on the chunk's model inputs, S NULL: its no-matrix-product form; the existing tile and finish
//                         kernels, unchanged.  M goes to the chunk's M array, V to slot t of the chunk's V array.
//   lqr_riccati_kernel    after the H steps: one wavefront per candidate, lanes over matrix elements, every matrix in LDS with an
//                         odd row pitch; the A x A Cholesky factorisation runs on the wavefront (A <= 8 dependent pivots), the two
//                         triangular solves one column of Hux per lane.  The next step's V rides in registers under the algebra.
// Every sum runs in an order fixed by N, E, D and A alone: a candidate's gains, cost-to-go and flag do not depend on the batch, on
// its place in it or on the chunks.  Plain kernels: no atomics, no waits between workgroups.  The workspace (Handle::lqrws) is this
// file's own, sized by plan_lqr_gains (lqr_gains_plan.h); run_moments_linear keeps using its own (Handle::linws).
#include "device_common.h"
#include "lqr_gains_plan.h"

namespace gpmpc_hip {

namespace {

constexpr int kPD = kMaxD + 1;           // LDS row pitch (doubles) of a matrix with up to D columns: odd, so that a walk down a
constexpr int kPA = kLqrMaxA + 1;        // column and a walk along a row both spread over the banks
constexpr int kVRegs = (kMaxD + kLqrMaxA) * kMaxD / kWave;      // V values a lane carries from one step to the next

struct LqrInputArgs {
    const double* actions;   // (rows, H, A) of this chunk
    const double* M;         // (rows, D) of the step before
    double* Xq;              // (rows, E)
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
};

// The model inputs of step t: the state entries advance by the mean of the step before (the operation of
// rollout_linear_step_kernel, moments_linear_kernels.h: the same bits), the action and time entries are set.
__global__ __launch_bounds__(256) void lqr_inputs_kernel(LqrInputArgs p) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)p.rows * p.E) return;
    const int b = (int)(idx / p.E), e = (int)(idx - (long long)b * p.E);
    double* xq = p.Xq + (size_t)b * p.E;
    if (e < p.D) xq[e] = p.t == 0 ? p.mu0[e] : xq[e] + p.M[(size_t)b * p.D + e];
    else if (e < p.D + p.A) xq[e] = p.actions[((size_t)b * p.H + p.t) * p.A + (e - p.D)];
    else xq[e] = p.time0 + (double)p.t;              // (only with include_time: E = D + A + 1)
}

// One wavefront per candidate: the backward Riccati sweep.
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
    const int b = blockIdx.x, tid = threadIdx.x;
    const int D = p.D, A = p.A, E = p.E, H = p.H, DA = D + A;
    const double* W = p.cost + DA;
    const double* WT = W + DA * DA;
    double* Pb = p.P ? p.P + (size_t)b * (H + 1) * D * D : nullptr;
    double* Kb = p.gains + (size_t)b * H * A * D;

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
        wave_lds_sync();
        for (int idx = tid; idx < A * A; idx += 64) {                // Huu = R + B^T G + reg I for i <= j, mirrored
            const int i = idx / A, j = idx - i * A;
            if (i > j) continue;
            double h = s_R[i][j];
            for (int k = 0; k < D; ++k) h = fma(s_B[k][i], s_G[k][j], h);
            if (i == j) h += p.reg;
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
            if (tid < D) {                                           // one column of Hux per lane: L y = Hux, L^T x = y, K = -x
                double y[kLqrMaxA];
#pragma unroll
                for (int i = 0; i < kLqrMaxA; ++i) {
                    y[i] = 0.0;
                    if (i < A) {
                        double s = s_Hux[i][tid];
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
                    if (i < A) s_K[i][tid] = 0.0 - y[i];
            }
        } else {
            ++failed;                                                // a lost pivot: K_t = 0, P_t = sym(Q + A^T F)
            for (int idx = tid; idx < A * D; idx += 64) s_K[idx / D][idx % D] = 0.0;
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
    }
    if (p.flags && tid == 0) p.flags[b] = failed;
}

}  // namespace

int run_lqr_gains(Handle* h, const double* actions, const double* mu0_host, int B, int H, int A, int include_time, double time0,
                  double reg, double* gains_out, double* P_out, int* flags_out, hipStream_t s) {
    const int D = h->D, E = h->E;
    static_assert(kVRegs * kWave >= (kMaxD + kLqrMaxA) * kMaxD, "lqr_riccati_kernel: V values per lane");
    LqrGainsPlan pl;
    plan_lqr_gains(D, E, H, B, h->opt_lqr_gains_chunk, pl);
    int rc = grow(h, h->lqrws, pl.total);
    if (rc) return rc;
    double* ws = h->lqrws.p;
    LqrInputArgs in{};
    in.Xq = ws + pl.xq; in.M = ws + pl.M;
    in.E = E; in.D = D; in.A = A; in.H = H; in.include_time = include_time; in.time0 = time0;
    for (int d = 0; d < D; ++d) in.mu0[d] = mu0_host[d];
    LqrRiccatiArgs r{};
    r.V = ws + pl.V; r.cost = h->cost.p;
    r.E = E; r.D = D; r.A = A; r.H = H; r.reg = reg;
    for (long long b0 = 0; b0 < B; b0 += pl.chunk) {
        const int rows = (int)((B - b0) < pl.chunk ? (B - b0) : pl.chunk);
        in.rows = rows;
        in.actions = actions + (size_t)b0 * H * A;
        const unsigned blocks = (unsigned)(((long long)rows * E + 255) / 256);
        for (int t = 0; t < H; ++t) {
            in.t = t;
            hipLaunchKernelGGL(lqr_inputs_kernel, dim3(blocks), dim3(256), 0, s, in);
            rc = run_moments_linear(h, ws + pl.xq, nullptr, rows, ws + pl.M, nullptr, ws + pl.V + (size_t)t * rows * E * D, s);
            if (rc) return rc;
        }
        r.rows = rows;
        r.gains = gains_out + (size_t)b0 * H * A * D;
        r.P = P_out ? P_out + (size_t)b0 * (H + 1) * D * D : nullptr;
        r.flags = flags_out ? flags_out + b0 : nullptr;
        hipLaunchKernelGGL(lqr_riccati_kernel, dim3(rows), dim3(64), 0, s, r);
        GPMPC_HIP_CHECK(h, hipGetLastError());
    }
    return GPMPC_OK;
}

}  // namespace gpmpc_hip
