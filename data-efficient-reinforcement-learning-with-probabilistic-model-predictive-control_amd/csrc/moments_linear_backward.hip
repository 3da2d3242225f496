// moments_linear_backward.hip -- reverse-mode products of the linearised propagation: gpmpc_moments_linear_backward (one step),
// gpmpc_rollout_linear_backward (a trajectory with its costs) and gpmpc_rollout_linear_feedback_backward (the same in closed loop).  Per point, with d_je = x_je - m_e (formed per element, as the
// forward does), r_aje = d_je / l_ae^2, k_aj as in the forward and q_a = iK_a k_a (a row of K* iK; iK taken as symmetric):
//   var_bar = sym(V S_bar V^T)
//   W = V_bar + Sigma V (S_bar + S_bar^T)                      (E x D)
//   s_a = S_bar[a,a],   u_aj = sum_e W[e,a] r_aje,   c_aj = beta_aj (M_bar_a + u_aj) - 2 s_a q_aj
//   mu_bar_g = sum_a [ sum_j c_aj k_aj r_ajg  -  W[g,a] M_a / l_ag^2 ]
// from dM_a/dm_g = V[g,a], dV[e,a]/dm_g = sum_j beta k r_e r_g - delta_eg M_a / l_ae^2, dv_a/dm_g = -2 sum_j q_aj k_aj r_ajg.
//
// Structure ("Gradients of the linearised propagation"):
//   lin_tile_kernel           (moments_linear_kernels.h, shared with the forward) one workgroup per (64 rows, 256-column block of
//                             iK_a, output a), the k loop P = K*_a iK_a on v_mfma_f64_16x16x4_f64, compiled out where no variance
//                             term is needed.  Forward form: the block's partial sums  sum_j P k | sum_j k beta | E sums
//                             beta k (x_j - m).  Reverse form: every lane forms k and c for its 16 rows x 1 column from the row's
//                             coefficients M_bar_a | s_a | W[e,a] / l_ae^2 (staged in LDS) and P, stages c k in LDS, and the
//                             contraction of the forward leaves the E sums  sum_j c k (x_jg - m_g).
//   lin_bwd_point_kernel      one wavefront per point, between the two tile launches: adds the forward sums in block order, forms
//                             V, var_bar, W, the coefficients and  sum_a W[g,a] M_a / l_ag^2.
//   lin_bwd_finish_kernel     one wavefront per point: adds the reverse sums in block order, scales, subtracts.
//   rollout_linear_bwd_*      the trajectory: per chunk of candidates the forward is recomputed batch-major by the forward's own
//                             kernels (rollout_linear_init_kernel, then one tile launch + rollout_linear_step_kernel per step,
//                             moments_linear_kernels.h), which KEEP every step's M and the state rows of V (keepM / keepV)
//                             beside the trajectory; the cost variances come from the trajectory cost kernel.  Reverse
//                             sweep t = H-1 .. 0 with A_t = I + V_s (Sigma_{t+1} = A_t^T Sigma_t A_t + diag v): one wavefront per
//                             candidate closes step t + 1 (x_bar from the tile sums -> lambda, actions_bar) and opens step t (cost
//                             partials by cost_adjoint_wave, W = 2 Sigma_t A_t Lambda on the state rows, the coefficients,
//                             Lambda_t = sym(seeds) + A_t Lambda A_t^T, the model inputs), then one reverse tile launch over the
//                             chunk: H + 1 small launches and H tile launches.
//   closed loop (FB)          u = ubar_t + K_t (x - mu_t): C_t = V_s + K_t^T V_u takes the place of V_s (A_t = I + C_t).  The forward
//                             is recomputed by rollout_linear_step_kernel<true>, the closed-loop forward's own step, and keeps
//                             the D + A state and action rows of V; the cost
//                             variances come from the closed-loop cost kernel (launch_traj_cost_feedback).  The reverse kernel's
//                             FB instantiation loads K_t, takes the cost partials from cost_adjoint_feedback_wave, fills the
//                             action rows of W with K_t C_bar (C_bar = 2 Sigma_t A_t Lambda) and writes gains_bar_t = (cost
//                             partial) + V_u C_bar^T when it opens step t.  The tile kernels and their launches are shared.
// Every sum runs in an order fixed by N, E, D and A alone; a point's or candidate's bits do not depend on the batch, on its place in
// it or on the chunks.  Plain kernels: no atomics, no waits between workgroups.  The workspace (Handle::linbws) is this file's
// own, laid out by plan_moments_linear_backward (moments_linear_backward_plan.h).
#include "cost_adjoint_feedback.h"
#include "moments_linear_backward_plan.h"
#include "moments_linear_kernels.h"

namespace gpmpc_hip {

namespace {

struct LbPointArgs {
    const double* part;
    const double* ils2;      // (D, E)
    const double* Sig;       // (rows, E, E) of this chunk, or NULL (= 0)
    const double* Mb;        // (rows, D) or NULL
    const double* Sb;        // (rows, D, D) or NULL
    const double* Vb;        // (rows, E, D) or NULL
    double* coef;            // written when mu_bar is asked for (with base)
    double* base;            // (rows, E)
    double* var_bar;         // (rows, E, E) of this chunk, or NULL
    double* mu_bar;          // (rows, E) of this chunk, or NULL (finish kernel)
    int E, D, nCB, NW;
    long long Mc;
};

// The reverse kernel's block: the recomputed forward's (mu / Sig: the recomputed trajectory; keepM / keepV set) and the sweep's own.
struct LbRollArgs : LinStepArgs {
    const double* cost;      // target | W | W_T | smin | smax
    const double* cv;        // (rows, H + 1) cost variances (read with an objective seed only)
    double* adj;             // (rows, 2 D + D D + A): lambda | Lambda | cost partials of the open step wrt mu and the action
    double* coef;            // (D, NW, Mc)
    double* base;            // (rows, E)
    SweepSeeds sd;           // this chunk's cotangents (each NULL = 0) and initial-state outputs (each NULL = not written)
    double* actions_bar;     // (rows, H, A) of this chunk
    double* gains_bar;       // closed loop: (rows, H, A, D) of this chunk, or NULL (not written)
    int use_constraints;
    double kappa;
};

// One wavefront per point, after the forward-form tile launch (no k loop: M and the Jacobian sums only).
__global__ __launch_bounds__(64) void lin_bwd_point_kernel(LbPointArgs p) {
    __shared__ double s_sum[kMaxD][kMaxE + 2];
    __shared__ double s_V[kMaxE][kMaxD];
    __shared__ double s_S2[kMaxD][kMaxD];            // S_bar + S_bar^T
    __shared__ double s_T[kMaxE][kMaxD];             // V (S_bar + S_bar^T)
    __shared__ double s_W[kMaxE][kMaxD];
    const int m = blockIdx.x, tid = threadIdx.x;
    const int D = p.D, E = p.E, NW = p.NW;
    const size_t Mc = (size_t)p.Mc;
    for (int idx = tid; idx < D * NW; idx += 64) {
        const int a = idx / NW, which = idx - a * NW;
        s_sum[a][which] = which == 0 ? 0.0 : block_sum(p.part, a, which, (size_t)m, p.nCB, NW, Mc);
    }
    const double* Sb = p.Sb ? p.Sb + (size_t)m * D * D : nullptr;
    for (int idx = tid; idx < D * D; idx += 64) {
        const int a = idx / D, b = idx - a * D;
        s_S2[a][b] = Sb ? Sb[a * D + b] + Sb[b * D + a] : 0.0;
    }
    __syncthreads();
    for (int idx = tid; idx < E * D; idx += 64) {
        const int e = idx / D, a = idx - e * D;
        s_V[e][a] = p.ils2[a * E + e] * s_sum[a][2 + e];
    }
    __syncthreads();
    for (int idx = tid; idx < E * D; idx += 64) {
        const int e = idx / D, b = idx - e * D;
        double t = 0.0;
        for (int a = 0; a < D; ++a) t = fma(s_V[e][a], s_S2[a][b], t);
        s_T[e][b] = t;
    }
    __syncthreads();
    if (p.var_bar) {                                 // sym(V S_bar V^T) = 1/2 T V^T: e <= f, mirrored -- exactly symmetric
        double* vb = p.var_bar + (size_t)m * E * E;
        for (int idx = tid; idx < E * E; idx += 64) {
            const int e = idx / E, f = idx - e * E;
            if (e > f) continue;
            double q = 0.0;
            for (int b = 0; b < D; ++b) q = fma(s_T[e][b], s_V[f][b], q);
            q *= 0.5;
            vb[e * E + f] = q;
            vb[f * E + e] = q;
        }
    }
    if (!p.mu_bar) return;
    const double* Sg = p.Sig ? p.Sig + (size_t)m * E * E : nullptr;
    const double* Vb = p.Vb ? p.Vb + (size_t)m * E * D : nullptr;
    for (int idx = tid; idx < E * D; idx += 64) {    // W = V_bar + Sigma T
        const int e = idx / D, b = idx - e * D;
        double t = 0.0;
        if (Sg)
            for (int f = 0; f < E; ++f) t = fma(Sg[e * E + f], s_T[f][b], t);
        s_W[e][b] = (Vb ? Vb[idx] : 0.0) + t;
    }
    __syncthreads();
    for (int idx = tid; idx < D * NW; idx += 64) {
        const int a = idx / NW, which = idx - a * NW;
        double v;
        if (which == 0) v = p.Mb ? p.Mb[(size_t)m * D + a] : 0.0;
        else if (which == 1) v = Sb ? Sb[a * D + a] : 0.0;
        else v = s_W[which - 2][a] * p.ils2[a * E + which - 2];
        p.coef[((size_t)a * NW + which) * Mc + m] = v;
    }
    for (int g = tid; g < E; g += 64) {
        double t = 0.0;
        for (int a = 0; a < D; ++a) t = fma(s_W[g][a] * p.ils2[a * E + g], s_sum[a][1], t);
        p.base[(size_t)m * E + g] = t;
    }
}

// x_bar_g = sum_a (1 / l_ag^2) sum_j c k (x_jg - m_g)  -  sum_a W[g,a] M_a / l_ag^2   (outputs in order, column blocks in order)
__device__ inline double input_adjoint(const double* part, const double* ils2, const double* base_row, int g, size_t row, int D,
                                       int E, int nCB, int NW, size_t Mc) {
    double t = 0.0;
    for (int a = 0; a < D; ++a) t = fma(ils2[a * E + g], block_sum(part, a, 2 + g, row, nCB, NW, Mc), t);
    return t - base_row[g];
}

// One wavefront per point, after the reverse-form tile launch.
__global__ __launch_bounds__(64) void lin_bwd_finish_kernel(LbPointArgs p) {
    const int m = blockIdx.x, E = p.E;
    for (int g = threadIdx.x; g < E; g += 64)
        p.mu_bar[(size_t)m * E + g] = input_adjoint(p.part, p.ils2, p.base + (size_t)m * E, g, (size_t)m, p.D, E, p.nCB, p.NW,
                                                   (size_t)p.Mc);
}

// ---- the trajectory ------------------------------------------------------------------------------------------------------------
// One wavefront per candidate of the reverse sweep.  t_post >= 0: the reverse tile launch of step t_post is done -- x_bar from its
// sums, lambda_t = lambda_{t+1} + x_bar[:D] + (cost partial + seed), actions_bar_t = (cost partial) + x_bar[D:D+A]; t_post < 0
// (first launch): the adjoints start at the terminal index H.  t_pre >= 0: step t_pre is opened -- its cost partials and seeds,
// A = I + V_s, W = 2 Sigma_t A Lambda, the coefficients and model inputs of its tile launch, Lambda_t = sym(.) + A Lambda A^T;
// t_pre < 0 (last launch): lambda_0 / Lambda_0 go to mu0_bar / S0_bar.
// FB (compile time): the closed loop -- K_t is loaded, the stage's cost partials
// come from cost_adjoint_feedback_wave (with the one wrt K_t), A = I + C with C = V_s + K_t^T V_u, the action rows of W are
// K_t C_bar (C_bar = the state rows, 2 Sigma_t A Lambda), and opening step t writes gains_bar_t = (cost partial) + V_u C_bar^T.
// Static LDS of the FB instantiation at kMaxD = 16, kMaxE = 24: 5520 doubles = 44160 bytes (open loop: 3760 = 30080).
template <bool FB>
__global__ __launch_bounds__(64) void rollout_linear_bwd_reverse_kernel(LbRollArgs p, int t_post, int t_pre) {
    constexpr int kN = kMaxE;                        // D + A <= E <= kMaxE
    constexpr int kTmp = FB ? cost_adjoint_feedback_tmp(kMaxD, kN - kMaxD) : 2 * kN * kN + 3 * kN;
    constexpr int kWR = FB ? kMaxE : kMaxD;          // rows of W that may be non-zero
    constexpr int kAD = (kMaxE / 2) * (kMaxE - kMaxE / 2);      // A D <= this for D + A <= kMaxE
    static_assert(kMaxE / 2 <= kMaxD, "bound of A D");
    __shared__ double s_cost[kN + kN * kN + kMaxD * kMaxD + 2 * kMaxD];
    __shared__ double s_tmp[kTmp];
    __shared__ double s_lam[kMaxD], s_Lam[kMaxD * kMaxD];
    __shared__ double s_gmu[kMaxD], s_gSig[kMaxD * kMaxD], s_gu[kN];
    __shared__ double s_mu[kMaxD], s_Sg[kMaxD * kMaxD], s_act[kN], s_M[kMaxD];
    __shared__ double s_A[kMaxD][kMaxD], s_AL[kMaxD][kMaxD], s_W[kWR][kMaxD];
    [[maybe_unused]] __shared__ double s_V[FB ? kMaxE : 1][kMaxD];      // FB: the kept rows of V [state or action input][output]
    [[maybe_unused]] __shared__ double s_K[FB ? kAD : 1];               // FB: K_t (A, D) row-major
    [[maybe_unused]] __shared__ double s_gK[FB ? kAD : 1];              // FB: the cost partial wrt K_t (A, D)
    const int b = blockIdx.x, lane = threadIdx.x;
    const int D = p.D, E = p.E, A = p.A, H = p.H, DD = D * D, n = D + A, NW = p.NW;
    const size_t Mc = (size_t)p.Mc;
    const SweepSeeds& sd = p.sd;
    const bool has_cm = sd.cm != nullptr, has_cv = sd.cv != nullptr, has_J = sd.J != nullptr;
    const bool cost_on = has_cm || has_cv || has_J;
    const double inv_n = 1.0 / (double)(H + 1);
    double* adj = p.adj + (size_t)b * (2 * D + DD + A);
    double* g_lam = adj;
    double* g_Lam = adj + D;
    double* g_gmu = g_Lam + DD;
    double* g_gu = g_gmu + D;
    if (cost_on)
        for (int i = lane; i < n + n * n + DD + 2 * D; i += 64) s_cost[i] = p.cost[i];
    const double* target = s_cost;
    const double* Wst = s_cost + n;
    const double* WT = Wst + n * n;
    const double* smin = WT + DD;
    const double* smax = smin + D;
    const double jb = has_J ? sd.J[b] : 0.0;

    // cost partials (weighted by the seeds) and trajectory seeds of time index t -> s_gmu, s_gSig, s_gu; reads s_mu / s_Sg / s_act
    auto stage_adjoint = [&](int t) {
        const bool terminal = (t == H);
        const size_t bt = (size_t)b * (H + 1) + t;
        for (int i = lane; i < D; i += 64) s_mu[i] = p.mu[bt * D + i];
        for (int i = lane; i < DD; i += 64) s_Sg[i] = p.Sig[bt * DD + i];
        if (!terminal)
            for (int i = lane; i < A; i += 64) s_act[i] = p.actions[((size_t)b * H + t) * A + i];
        if constexpr (FB) {
            if (!terminal) {
                const double* K = p.gains + (size_t)b * (size_t)p.gain_stride + (size_t)t * A * D;
                for (int i = lane; i < A * D; i += 64) s_K[i] = K[i];
            }
        }
        wave_lds_sync();
        if (cost_on) {
            double wm, wv;
            seeded_cost_weights(has_cm, has_cm ? sd.cm[bt] : 0.0, has_cv, has_cv ? sd.cv[bt] : 0.0, has_J, jb, p.kappa,
                                has_J ? p.cv[bt] : 1.0, inv_n, wm, wv);
            bool done = false;
            if constexpr (FB) {
                if (!terminal) {
                    cost_adjoint_feedback_wave(lane, D, A, s_mu, s_Sg, s_act, s_K, target, Wst, smin, smax, p.use_constraints != 0,
                                               wm, wv, s_tmp, s_gmu, s_gSig, s_gu, s_gK);
                    done = true;
                }
            }
            if (!done)
                cost_adjoint_wave(lane, D, A, terminal, s_mu, s_Sg, s_act, target, terminal ? WT : Wst, smin, smax,
                                  p.use_constraints != 0, wm, wv, s_tmp, s_gmu, s_gSig, s_gu);
            wave_lds_sync();
        }
        for (int i = lane; i < D; i += 64) {
            double v = cost_on ? s_gmu[i] : 0.0;
            if (sd.mu) v += sd.mu[bt * D + i];
            s_gmu[i] = v;
        }
        for (int i = lane; i < DD; i += 64) {
            double v = cost_on ? s_gSig[i] : 0.0;
            if (sd.Sig) v += sd.Sig[bt * DD + i];
            s_gSig[i] = v;
        }
        if (!cost_on || terminal)
            for (int i = lane; i < A; i += 64) s_gu[i] = 0.0;
        if constexpr (FB) {
            if (!cost_on)
                for (int i = lane; i < A * D; i += 64) s_gK[i] = 0.0;
        }
        wave_lds_sync();
    };

    wave_lds_sync();
    if (t_post >= 0) {
        double x = 0.0;
        if (lane < D + A) x = input_adjoint(p.part, p.ils2, p.base + (size_t)b * E, lane, (size_t)b, D, E, p.nCB, NW, Mc);
        if (lane < D) s_lam[lane] = (g_lam[lane] + x) + g_gmu[lane];
        else if (lane < D + A) p.actions_bar[((size_t)b * H + t_post) * A + lane - D] = g_gu[lane - D] + x;      // (time: no gradient)
        for (int i = lane; i < DD; i += 64) s_Lam[i] = g_Lam[i];
    } else {
        stage_adjoint(H);
        for (int i = lane; i < D; i += 64) s_lam[i] = s_gmu[i];
        for (int i = lane; i < DD; i += 64) {
            const int r = i / D, q = i - r * D;
            s_Lam[i] = 0.5 * (s_gSig[i] + s_gSig[q * D + r]);
        }
    }
    wave_lds_sync();
    if (t_pre < 0) {
        if (sd.mu0_bar)
            for (int i = lane; i < D; i += 64) sd.mu0_bar[(size_t)b * D + i] = s_lam[i];
        if (sd.S0_bar)
            for (int i = lane; i < DD; i += 64) sd.S0_bar[(size_t)b * DD + i] = s_Lam[i];
        return;
    }
    const int t = t_pre;
    stage_adjoint(t);
    const double* keepM = p.keepM + ((size_t)b * H + t) * D;
    const double* keepV = p.keepV + ((size_t)b * H + t) * (FB ? n * D : DD);
    for (int i = lane; i < D; i += 64) s_M[i] = keepM[i];
    if constexpr (FB) {
        for (int idx = lane; idx < n * D; idx += 64) s_V[idx / D][idx % D] = keepV[idx];
        wave_lds_sync();
        for (int idx = lane; idx < DD; idx += 64) {              // A = I + C, C = V_s + K^T V_u as the forward forms it
            const int i = idx / D, a = idx - i * D;
            double v = 0.0;
            for (int u = 0; u < A; ++u) v = fma(s_K[u * D + i], s_V[D + u][a], v);
            s_A[i][a] = (s_V[i][a] + v) + (i == a ? 1.0 : 0.0);
        }
    } else {
        for (int idx = lane; idx < DD; idx += 64) {
            const int i = idx / D, a = idx - i * D;
            s_A[i][a] = keepV[idx] + (i == a ? 1.0 : 0.0);
        }
    }
    wave_lds_sync();
    for (int idx = lane; idx < DD; idx += 64) {                  // A Lambda
        const int i = idx / D, a = idx - i * D;
        double v = 0.0;
        for (int c = 0; c < D; ++c) v = fma(s_A[i][c], s_Lam[c * D + a], v);
        s_AL[i][a] = v;
    }
    wave_lds_sync();
    for (int idx = lane; idx < DD; idx += 64) {                  // W = 2 Sigma_t A Lambda
        const int i = idx / D, a = idx - i * D;
        double v = 0.0;
        for (int k = 0; k < D; ++k) v = fma(s_Sg[i * D + k], s_AL[k][a], v);
        s_W[i][a] = 2.0 * v;
    }
    for (int idx = lane; idx < DD; idx += 64) {                  // Lambda_t: i <= j, mirrored -- exactly symmetric
        const int i = idx / D, j = idx - i * D;
        if (i > j) continue;
        double v = 0.0;
        for (int a = 0; a < D; ++a) v = fma(s_AL[i][a], s_A[j][a], v);
        v += 0.5 * (s_gSig[i * D + j] + s_gSig[j * D + i]);
        g_Lam[i * D + j] = v;
        g_Lam[j * D + i] = v;
    }
    if constexpr (FB) {
        wave_lds_sync();                                         // the state rows of W are C_bar
        for (int idx = lane; idx < A * D; idx += 64) {           // the action rows: K C_bar
            const int u = idx / D, a = idx - u * D;
            double v = 0.0;
            for (int i = 0; i < D; ++i) v = fma(s_K[u * D + i], s_W[i][a], v);
            s_W[D + u][a] = v;
        }
        if (p.gains_bar) {                                       // gains_bar_t = (cost partial) + V_u C_bar^T
            double* gb = p.gains_bar + ((size_t)b * H + t) * A * D;
            for (int idx = lane; idx < A * D; idx += 64) {
                const int u = idx / D, i = idx - u * D;
                double v = 0.0;
                for (int a = 0; a < D; ++a) v = fma(s_V[D + u][a], s_W[i][a], v);
                gb[idx] = s_gK[idx] + v;
            }
        }
    }
    wave_lds_sync();
    const int nW = FB ? n : D;                                   // rows of W that are not zero by construction
    for (int idx = lane; idx < D * NW; idx += 64) {
        const int a = idx / NW, which = idx - a * NW;
        double v;
        if (which == 0) v = s_lam[a];
        else if (which == 1) v = s_Lam[a * D + a];
        else v = (which - 2 < nW) ? s_W[which - 2][a] * p.ils2[a * E + which - 2] : 0.0;
        p.coef[((size_t)a * NW + which) * Mc + b] = v;
    }
    for (int g = lane; g < E; g += 64) {
        double v = 0.0;
        if (g < nW)
            for (int a = 0; a < D; ++a) v = fma(s_W[g][a] * p.ils2[a * E + g], s_M[a], v);
        p.base[(size_t)b * E + g] = v;
    }
    double* xq = p.Xq + (size_t)b * E;
    for (int i = lane; i < D; i += 64) {
        g_lam[i] = s_lam[i];
        g_gmu[i] = s_gmu[i];
        xq[i] = s_mu[i];
    }
    for (int i = lane; i < A; i += 64) {
        g_gu[i] = s_gu[i];
        xq[D + i] = s_act[i];
    }
    if (p.include_time && lane == 0) xq[E - 1] = p.time0 + (double)t;
}

}  // namespace

int run_moments_linear_backward(Handle* h, const double* mu, const double* Sig, int P, const double* Mb, const double* Sb,
                                const double* Vb, double* mb_out, double* vb_out, hipStream_t s) {
    const int N = h->N, D = h->D, E = h->E;
    if (P == 0 || (!mb_out && !vb_out)) return GPMPC_OK;
    if (vb_out && !Sb) {                             // var_bar = sym(V S_bar V^T) = 0
        GPMPC_HIP_CHECK(h, hipMemsetAsync(vb_out, 0, (size_t)P * E * E * sizeof(double), s));
        vb_out = nullptr;
    }
    if (mb_out && !Mb && !Sb && !Vb) {
        GPMPC_HIP_CHECK(h, hipMemsetAsync(mb_out, 0, (size_t)P * E * sizeof(double), s));
        mb_out = nullptr;
    }
    if (!mb_out && !vb_out) return GPMPC_OK;
    LinearBwdPlan pl;
    plan_moments_linear_backward(N, D, E, 0, P, 0, h->opt_moments_linear_bwd_chunk, 0, pl);
    int rc = grow(h, h->linbws, pl.total);
    if (rc) return rc;
    double* ws = h->linbws.p;
    LinTileArgs p{};
    p.Xt = h->Xt.p; p.ils2 = h->ils2.p; p.var = h->var.p; p.beta = h->beta.p; p.iK = h->iK.p;
    p.part = ws + pl.part; p.coef = ws + pl.coef;
    p.N = N; p.E = E; p.D = D; p.nCB = pl.nCB; p.NW = pl.NW; p.Mc = pl.Mc;
    LbPointArgs f{};
    f.part = p.part; f.ils2 = p.ils2; f.coef = ws + pl.coef; f.base = ws + pl.base;
    f.E = E; f.D = D; f.nCB = pl.nCB; f.NW = pl.NW; f.Mc = pl.Mc;
    for (long long m0 = 0; m0 < P; m0 += pl.chunk) {
        const int rows = (int)((P - m0) < pl.chunk ? (P - m0) : pl.chunk);
        p.rows = rows;
        p.Xq = mu + (size_t)m0 * E;
        launch_lin_tiles<false>(p, false, s);        // M and the Jacobian sums: no matrix product
        f.Sig = Sig ? Sig + (size_t)m0 * E * E : nullptr;
        f.Mb = Mb ? Mb + (size_t)m0 * D : nullptr;
        f.Sb = Sb ? Sb + (size_t)m0 * D * D : nullptr;
        f.Vb = Vb ? Vb + (size_t)m0 * E * D : nullptr;
        f.var_bar = vb_out ? vb_out + (size_t)m0 * E * E : nullptr;
        f.mu_bar = mb_out ? mb_out + (size_t)m0 * E : nullptr;
        hipLaunchKernelGGL(lin_bwd_point_kernel, dim3(rows), dim3(64), 0, s, f);
        if (mb_out) {
            launch_lin_tiles<true>(p, Sb != nullptr, s);
            hipLaunchKernelGGL(lin_bwd_finish_kernel, dim3(rows), dim3(64), 0, s, f);
        }
    }
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

namespace {

// a: filled by the entry point (model, cost settings, actions, shape, initial state); sd: the cotangents and initial-state outputs.
// gains != NULL: the closed loop (gains (B, H, A, D) when per_candidate, else (H, A, D) shared; gains_bar (B, H, A, D) or NULL) --
// the same plan with the action rows of V kept, the same init kernel and tile launches, with the FB forms of the step and reverse
// kernels and the closed-loop cost kernel; a chunk of candidates offsets the gain pointer only when the gains are per candidate.
int rollout_linear_backward_chunks(Handle* h, const RolloutArgs& a, const RolloutSeeds& sd, const double* gains, bool per_candidate,
                                   double* actions_bar, double* gains_bar, hipStream_t s) {
    const int N = a.N, D = a.D, E = a.E, A = a.A, H = a.H, B = a.B;
    const bool fb = gains != nullptr;
    LinearBwdPlan pl;
    plan_moments_linear_backward(N, D, E, A, B, H, h->opt_moments_linear_bwd_chunk, fb ? A : 0, pl);
    int rc = grow(h, h->linbws, pl.total);
    if (rc) return rc;
    double* ws = h->linbws.p;
    LinTileArgs p{};
    p.Xt = h->Xt.p; p.ils2 = h->ils2.p; p.var = h->var.p; p.beta = h->beta.p; p.iK = h->iK.p;
    p.part = ws + pl.part; p.coef = ws + pl.coef; p.Xq = ws + pl.xq;
    p.N = N; p.E = E; p.D = D; p.nCB = pl.nCB; p.NW = pl.NW; p.Mc = pl.Mc;
    LbRollArgs q{};
    const LinStepArgs& fq = q;                        // the forward's kernels take its LinStepArgs part
    q.gain_stride = per_candidate ? (long long)H * A * D : 0;
    q.part = p.part; q.ils2 = p.ils2; q.var = p.var; q.cost = a.cost;
    q.mu = ws + pl.mu; q.Sig = ws + pl.Sig; q.keepM = ws + pl.stepM; q.keepV = ws + pl.stepV; q.cv = ws + pl.cv;
    q.adj = ws + pl.adj; q.coef = ws + pl.coef; q.base = ws + pl.base; q.Xq = ws + pl.xq;
    q.E = E; q.D = D; q.A = A; q.H = H; q.nCB = pl.nCB; q.NW = pl.NW; q.Mc = pl.Mc;
    q.include_time = a.include_time; q.time0 = a.time0; q.kappa = a.kappa; q.use_constraints = a.use_constraints;
    for (int d = 0; d < D; ++d) q.mu0[d] = a.mu0[d];
    for (int d = 0; d < D * D; ++d) q.S0[d] = a.S0[d];
    const size_t T1 = (size_t)(H + 1);
    for (long long b0 = 0; b0 < B; b0 += pl.chunk) {
        const int rows = (int)((B - b0) < pl.chunk ? (B - b0) : pl.chunk);
        const size_t o = (size_t)b0;
        p.rows = rows;
        q.gains = fb ? gains + o * (size_t)q.gain_stride : nullptr;
        q.gains_bar = gains_bar ? gains_bar + o * H * A * D : nullptr;
        auto launch_reverse = [&](int t_post, int t_pre) {
            if (fb) hipLaunchKernelGGL(rollout_linear_bwd_reverse_kernel<true>, dim3(rows), dim3(64), 0, s, q, t_post, t_pre);
            else hipLaunchKernelGGL(rollout_linear_bwd_reverse_kernel<false>, dim3(rows), dim3(64), 0, s, q, t_post, t_pre);
        };
        q.actions = a.actions + o * H * A;
        q.actions_bar = actions_bar + o * H * A;
        q.sd.mu = sd.mu ? sd.mu + o * T1 * D : nullptr;
        q.sd.Sig = sd.Sig ? sd.Sig + o * T1 * D * D : nullptr;
        q.sd.cm = sd.cm ? sd.cm + o * T1 : nullptr;
        q.sd.cv = sd.cv ? sd.cv + o * T1 : nullptr;
        q.sd.J = sd.J ? sd.J + o : nullptr;
        q.sd.mu0_bar = sd.mu0_bar ? sd.mu0_bar + o * D : nullptr;
        q.sd.S0_bar = sd.S0_bar ? sd.S0_bar + o * D * D : nullptr;
        // the forward, recomputed
        q.t = 0;
        hipLaunchKernelGGL(rollout_linear_init_kernel, dim3(rows), dim3(64), 0, s, fq);
        for (int t = 0; t < H; ++t) {
            launch_lin_tiles<false>(p, true, s);
            q.t = t;
            if (fb) hipLaunchKernelGGL(rollout_linear_step_kernel<true>, dim3(rows), dim3(64), 0, s, fq);
            else hipLaunchKernelGGL(rollout_linear_step_kernel<false>, dim3(rows), dim3(64), 0, s, fq);
        }
        GPMPC_HIP_CHECK(h, hipGetLastError());
        if (sd.J && fb) {                             // the objective's weights need the (closed-loop) cost variances
            rc = launch_traj_cost_feedback(h, a, rows, q.mu, q.Sig, q.actions, q.gains, q.gain_stride, nullptr, ws + pl.cv, nullptr,
                                           s);
            if (rc) return rc;
        } else if (sd.J) {                            // the objective's weights need the cost variances
            RolloutArgs c = a;
            c.B = rows;
            c.actions = q.actions;
            c.mu_out = q.mu; c.Sig_out = q.Sig;
            rc = launch_traj_cost(h, c, nullptr, ws + pl.cv, nullptr, s);
            if (rc) return rc;
        }
        // the reverse sweep
        launch_reverse(-1, H - 1);
        for (int t = H - 1; t >= 0; --t) {
            launch_lin_tiles<true>(p, true, s);
            launch_reverse(t, t - 1);
        }
        GPMPC_HIP_CHECK(h, hipGetLastError());
    }
    return GPMPC_OK;
}

}  // namespace

int run_rollout_linear_backward(Handle* h, const RolloutArgs& a, const RolloutSeeds& sd, double* actions_bar, hipStream_t s) {
    return rollout_linear_backward_chunks(h, a, sd, nullptr, false, actions_bar, nullptr, s);
}

int run_rollout_linear_feedback_backward(Handle* h, const RolloutArgs& a, const RolloutSeeds& sd, const double* gains,
                                         bool per_candidate, double* actions_bar, double* gains_bar, hipStream_t s) {
    return rollout_linear_backward_chunks(h, a, sd, gains, per_candidate, actions_bar, gains_bar, s);
}

}  // namespace gpmpc_hip
