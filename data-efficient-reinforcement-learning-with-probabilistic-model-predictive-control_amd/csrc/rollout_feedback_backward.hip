// rollout_feedback_backward.hip -- the reverse-mode product of the closed-loop moment-matched rollout
// (gpmpc_rollout_feedback_backward).  Forward, per candidate and step t, with x_t = [mu_t | ubar_t | time0 + t] and
// G_t = [I_D ; K_t ; 0] (rollout_feedback.hip):
//   Sigma_in = G_t Sigma_t G_t^T,  (M, S, V) = moments(x_t, Sigma_in),  R = Sigma_in[:D, :] (D x E),  C = R V,
//   mu_{t+1} = mu_t + M,  Sigma_{t+1} = Sigma_t + S + C + C^T
// Reverse sweep t = H-1 .. 0 with the adjoints lambda_{t+1} (D) and Lambda_{t+1} (D x D, symmetric):
//   M_bar = lambda_{t+1},  S_bar = Lambda_{t+1},  C_bar = 2 Lambda_{t+1}
//   V_bar = R^T C_bar (E x D, time row zero),  R_bar = C_bar V^T (D x E)
//   (x_bar, P) = the step formula of gpmpc_moments_backward at (x_t, Sigma_in) with (M_bar, S_bar, V_bar)      [P: symmetric part]
//   Z = P + sym([R_bar ; 0])                                                                                    (E x E)
//   actions_bar_t = x_bar[D:D+A] + (cost partial wrt ubar_t)
//   gains_bar_t   = action rows of 2 Z G_t Sigma_t + (cost partial wrt K_t)
//   lambda_t = lambda_{t+1} + x_bar[:D] + mu_bar_t + (cost partial wrt mu_t)
//   Lambda_t = Lambda_{t+1} + G_t^T Z G_t + sym(Sig_bar_t + cost partial wrt Sigma_t)                           (i <= j, mirrored)
// and mu0_bar = lambda_0, S0_bar = Lambda_0.  Stage and terminal cost partials are gpmpc_rollout_linear_feedback_backward's
// (cost_adjoint_feedback.h, grad_kernels.h).
//
// Structure ("Gradients of closed-loop moment-matched rollouts"): batch-major, per chunk of candidates
//   forward, recomputed           the forward's own rollout_feedback_init_kernel, run_moments and rollout_feedback_step_kernel
//                                 (rollout_feedback_kernels.h): the trajectory has gpmpc_rollout_feedback's bits.  Every step's V is
//                                 written by the moment kernels straight into the step-major keepV array.
//   traj_cost_feedback_kernel     with an objective seed: the closed-loop cost variances its weights need.
//   rollout_feedback_bwd_reverse_kernel(t_post, t_pre)
//                                 one wavefront per candidate.  t_post >= 0 closes step t_post from (x_bar, P): the stage's cost
//                                 partials and seeds, R_bar, Z, actions_bar, gains_bar, lambda_t, Lambda_t; t_post < 0 (first
//                                 launch) starts the adjoints at the terminal index H.  t_pre >= 0 opens step t_pre: the model
//                                 input of that step by write_model_input (the forward's bits), M_bar, S_bar, V_bar; t_pre < 0
//                                 (last launch) writes mu0_bar / S0_bar.
//   run_moments_backward          per reverse step, on the chunk's model inputs: its setup, point, pair and finish launches,
//                                 unchanged.  All three cotangents are always handed over, so its launches do not depend on which
//                                 of the caller's cotangents are NULL.
// H + 1 small launches, H forward and H reverse moment passes per chunk.  A call without gains runs the same kernels on a zeroed
// shared gain sequence in the workspace.  Every sum runs in an order fixed by D, A and E alone, the moment kernels' by N, E and the
// pair: a candidate's bits do not depend on the batch, on its place in it, on any chunk option or on the gain layout.  Plain
// kernels: no atomics, no waits between workgroups.  The workspace (Handle::fbbws) is this file's own, laid out by
// plan_rollout_feedback_backward (rollout_feedback_backward_plan.h); run_moments uses Handle::momws, run_moments_backward
// Handle::mombws.
#include "cost_adjoint_feedback.h"
#include "rollout_feedback_backward_plan.h"
#include "rollout_feedback_kernels.h"

namespace gpmpc_hip {

namespace {

// The reverse kernel's block: the recomputed forward's (f.mu / f.Sig: the recomputed trajectory, f.xin / f.sin: the model input of
// the step that is opened) and the sweep's own.
struct FbBwdArgs {
    FbArgs f;
    const double* cost;      // target | W | W_T | smin | smax
    const double* cv;        // (rows, H + 1) cost variances (read with an objective seed only)
    const double* keepV;     // (H, rows_stride, E, D) every step's V
    long long rows_stride;   // candidates per step of keepV (the plan's chunk)
    double* adj;             // (rows, D + D D): lambda | Lambda
    double* Mb;              // (rows, D)     cotangents of the open step for run_moments_backward ...
    double* Sb;              // (rows, D, D)
    double* Vb;              // (rows, E, D)
    const double* xb;        // (rows, E)     ... and its results for the step that is closed
    const double* Pb;        // (rows, E, E)
    SweepSeeds sd;           // this chunk's cotangents (each NULL = 0) and initial-state outputs (each NULL = not written)
    double* actions_bar;     // (rows, H, A) of this chunk
    double* gains_bar;       // (rows, H, A, D) of this chunk, or NULL (not written)
    int use_constraints;
    double kappa;
};

// Static LDS at kMaxD = 16, kMaxE = 24: 6232 doubles = 49856 bytes.
__global__ __launch_bounds__(64) void rollout_feedback_bwd_reverse_kernel(FbBwdArgs p, int t_post, int t_pre) {
    constexpr int kN = kMaxE;                        // D + A <= E <= kMaxE
    constexpr int kTmp = cost_adjoint_feedback_tmp(kMaxD, kN - kMaxD);
    constexpr int kAD = (kMaxE / 2) * (kMaxE - kMaxE / 2);      // A D <= this for D + A <= kMaxE
    static_assert(kMaxE / 2 <= kMaxD, "bound of A D");
    static_assert(kTmp >= 2 * kN * kMaxD + kMaxD * kN + kN * kN, "the closing algebra's scratch lies over the cost adjoint's");
    __shared__ double s_cost[kN + kN * kN + kMaxD * kMaxD + 2 * kMaxD];
    __shared__ double s_tmp[kTmp];
    __shared__ double s_P[kN * kN];                  // P of the closed step (n x n, the state and action rows and columns)
    __shared__ double s_lam[kMaxD], s_Lam[kMaxD * kMaxD];
    __shared__ double s_gmu[kMaxD], s_gSig[kMaxD * kMaxD], s_gu[kN], s_gK[kAD];
    __shared__ double s_mu[kMaxD], s_Sg[kMaxD * kMaxD], s_act[kN], s_Kf[kAD], s_x[kN];
    __shared__ double s_V[kMaxE][kMaxD];             // V of the closed step [input][output]
    __shared__ double s_S[kMaxD][kMaxD];             // Sigma_t of the opened step, for write_model_input
    __shared__ double s_K[kMaxE][kMaxD];
    __shared__ double s_KS[kMaxE][kMaxD];
    const int b = blockIdx.x, lane = threadIdx.x;
    const FbArgs& f = p.f;
    const int D = f.D, E = f.E, A = f.A, H = f.H, DD = D * D, n = D + A;
    const SweepSeeds& sd = p.sd;
    const bool has_cm = sd.cm != nullptr, has_cv = sd.cv != nullptr, has_J = sd.J != nullptr;
    const bool cost_on = has_cm || has_cv || has_J;
    const double inv_n = 1.0 / (double)(H + 1);
    double* g_lam = p.adj + (size_t)b * (D + DD);
    double* g_Lam = g_lam + D;
    if (cost_on)
        for (int i = lane; i < n + n * n + DD + 2 * D; i += 64) s_cost[i] = p.cost[i];
    const double* target = s_cost;
    const double* Wst = s_cost + n;
    const double* WT = Wst + n * n;
    const double* smin = WT + DD;
    const double* smax = smin + D;
    const double jb = has_J ? sd.J[b] : 0.0;

    // cost partials (weighted by the seeds) and trajectory seeds of time index t -> s_gmu, s_gSig, s_gu, s_gK; leaves mu_t, Sigma_t,
    // ubar_t and K_t in s_mu / s_Sg / s_act / s_Kf
    auto stage_adjoint = [&](int t) {
        const bool terminal = (t == H);
        const size_t bt = (size_t)b * (H + 1) + t;
        for (int i = lane; i < D; i += 64) s_mu[i] = f.mu[bt * D + i];
        for (int i = lane; i < DD; i += 64) s_Sg[i] = f.Sig[bt * DD + i];
        if (!terminal) {
            for (int i = lane; i < A; i += 64) s_act[i] = f.actions[((size_t)b * H + t) * A + i];
            const double* K = f.gains + (size_t)b * (size_t)f.gain_stride + (size_t)t * A * D;
            for (int i = lane; i < A * D; i += 64) s_Kf[i] = K[i];
        }
        wave_lds_sync();
        if (cost_on) {
            double wm, wv;
            seeded_cost_weights(has_cm, has_cm ? sd.cm[bt] : 0.0, has_cv, has_cv ? sd.cv[bt] : 0.0, has_J, jb, p.kappa,
                                has_J ? p.cv[bt] : 1.0, inv_n, wm, wv);
            if (!terminal)
                cost_adjoint_feedback_wave(lane, D, A, s_mu, s_Sg, s_act, s_Kf, target, Wst, smin, smax, p.use_constraints != 0, wm,
                                           wv, s_tmp, s_gmu, s_gSig, s_gu, s_gK);
            else
                cost_adjoint_wave(lane, D, A, true, s_mu, s_Sg, s_act, target, WT, smin, smax, p.use_constraints != 0, wm, wv, s_tmp,
                                  s_gmu, s_gSig, s_gu);
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
        if (!cost_on || terminal) {
            for (int i = lane; i < A; i += 64) s_gu[i] = 0.0;
            for (int i = lane; i < A * D; i += 64) s_gK[i] = 0.0;
        }
        wave_lds_sync();
    };

    wave_lds_sync();
    if (t_post >= 0) {
        const int t = t_post;
        stage_adjoint(t);
        const double* Vt = p.keepV + ((size_t)t * (size_t)p.rows_stride + b) * E * D;
        const double* Pt = p.Pb + (size_t)b * E * E;
        for (int i = lane; i < D; i += 64) s_lam[i] = g_lam[i];
        for (int i = lane; i < DD; i += 64) s_Lam[i] = g_Lam[i];
        for (int idx = lane; idx < n * D; idx += 64) s_V[idx / D][idx % D] = Vt[idx];
        for (int i = lane; i < n; i += 64) s_x[i] = p.xb[(size_t)b * E + i];
        for (int idx = lane; idx < n * n; idx += 64) s_P[idx] = Pt[(idx / n) * E + idx % n];
        wave_lds_sync();
        double* GS = s_tmp;                          // G Sigma_t  (n x D)
        double* Rb = GS + n * D;                     // R_bar  (D x n, the zero time column left out)
        double* Z = Rb + D * n;                      // Z  (n x n)
        double* ZG = Z + n * n;                      // Z G  (n x D)
        for (int idx = lane; idx < n * D; idx += 64) {           // Sigma_t as the forward reads it: the upper triangle
            const int i = idx / D, j = idx - i * D;
            double v;
            if (i < D) {
                v = i <= j ? s_Sg[i * D + j] : s_Sg[j * D + i];
            } else {
                v = 0.0;
                for (int k = 0; k < D; ++k) v = fma(s_Kf[(i - D) * D + k], k <= j ? s_Sg[k * D + j] : s_Sg[j * D + k], v);
            }
            GS[idx] = v;
        }
        for (int idx = lane; idx < D * n; idx += 64) {           // R_bar = 2 Lambda V^T, the outputs in order
            const int a = idx / n, e = idx - a * n;
            double v = 0.0;
            for (int c = 0; c < D; ++c) v = fma(s_Lam[a * D + c], s_V[e][c], v);
            Rb[idx] = 2.0 * v;
        }
        wave_lds_sync();
        for (int idx = lane; idx < n * n; idx += 64) {           // Z = P + sym([R_bar ; 0]): i <= j, mirrored
            const int i = idx / n, j = idx - i * n;
            if (i > j) continue;
            const double r = (i < D ? Rb[i * n + j] : 0.0) + (j < D ? Rb[j * n + i] : 0.0);
            const double v = s_P[i * n + j] + 0.5 * r;
            Z[i * n + j] = v;
            Z[j * n + i] = v;
        }
        wave_lds_sync();
        for (int idx = lane; idx < n * D; idx += 64) {           // Z G, the actions in order
            const int k = idx / D, j = idx - k * D;
            double v = 0.0;
            for (int u = 0; u < A; ++u) v = fma(Z[k * n + D + u], s_Kf[u * D + j], v);
            ZG[idx] = Z[k * n + j] + v;
        }
        if (p.gains_bar) {                                       // gains_bar_t = (cost partial) + action rows of 2 Z (G Sigma_t)
            double* gb = p.gains_bar + ((size_t)b * H + t) * A * D;
            for (int idx = lane; idx < A * D; idx += 64) {
                const int u = idx / D, j = idx - u * D;
                double v = 0.0;
                for (int k = 0; k < n; ++k) v = fma(Z[(D + u) * n + k], GS[k * D + j], v);
                gb[idx] = s_gK[idx] + 2.0 * v;
            }
        }
        for (int u = lane; u < A; u += 64)                       // (time: no gradient)
            p.actions_bar[((size_t)b * H + t) * A + u] = s_gu[u] + s_x[D + u];
        wave_lds_sync();
        for (int idx = lane; idx < DD; idx += 64) {              // Lambda_t: i <= j, mirrored -- exactly symmetric
            const int i = idx / D, j = idx - i * D;
            if (i > j) continue;
            double v = 0.0;
            for (int u = 0; u < A; ++u) v = fma(s_Kf[u * D + i], ZG[(D + u) * D + j], v);
            v = ZG[i * D + j] + v;
            v = (s_Lam[i * D + j] + v) + 0.5 * (s_gSig[i * D + j] + s_gSig[j * D + i]);
            s_Lam[i * D + j] = v;
            s_Lam[j * D + i] = v;
        }
        for (int i = lane; i < D; i += 64) s_lam[i] = (s_lam[i] + s_x[i]) + s_gmu[i];
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
    // open step t: its model input with the forward's bits, and the cotangents of its moments
    const int t = t_pre;
    const size_t bt = (size_t)b * (H + 1) + t;
    for (int i = lane; i < D; i += 64) {
        s_mu[i] = f.mu[bt * D + i];
        g_lam[i] = s_lam[i];
        p.Mb[(size_t)b * D + i] = s_lam[i];
    }
    for (int i = lane; i < DD; i += 64) {
        s_S[i / D][i % D] = f.Sig[bt * DD + i];
        g_Lam[i] = s_Lam[i];
        p.Sb[(size_t)b * DD + i] = s_Lam[i];
    }
    __syncthreads();
    write_model_input(f, b, t, s_mu, s_S, s_K, s_KS);
    __syncthreads();
    double* Vb = p.Vb + (size_t)b * E * D;
    for (int idx = lane; idx < E * D; idx += 64) {               // V_bar = 2 R^T Lambda, the states in order; the time row zero
        const int e = idx / D, c = idx - e * D;
        double v = 0.0;
        if (e < n) {
            for (int a = 0; a < D; ++a) {
                const double r = e < D ? (a <= e ? s_S[a][e] : s_S[e][a]) : s_KS[e - D][a];
                v = fma(r, s_Lam[a * D + c], v);
            }
            v *= 2.0;
        }
        Vb[idx] = v;
    }
}

}  // namespace

// a: filled by the entry point (model, cost settings, actions, shape, initial state); sd: the cotangents and initial-state outputs.
// gains (B, H, A, D) when per_candidate, else (H, A, D) shared by all candidates, or NULL: the all-zero shared sequence (gains_bar
// is then NULL).  gains_bar (B, H, A, D) or NULL.
int run_rollout_feedback_backward(Handle* h, const RolloutArgs& a, const RolloutSeeds& sd, const double* gains, bool per_candidate,
                                  double* actions_bar, double* gains_bar, hipStream_t s) {
    const int D = a.D, E = a.E, A = a.A, H = a.H, B = a.B;
    FeedbackBwdPlan pl;
    plan_rollout_feedback_backward(D, E, A, B, H, gains == nullptr, h->opt_rollout_feedback_bwd_chunk, pl);
    int rc = grow(h, h->fbbws, pl.total);
    if (rc) return rc;
    double* ws = h->fbbws.p;
    if (!gains) {
        if (pl.total > pl.zero_gains)
            GPMPC_HIP_CHECK(h, hipMemsetAsync(ws + pl.zero_gains, 0, (pl.total - pl.zero_gains) * sizeof(double), s));
        gains = ws + pl.zero_gains;
        per_candidate = false;
    }
    FbBwdArgs q{};
    FbArgs& f = q.f;
    f.xin = ws + pl.xin; f.sin = ws + pl.sin;
    f.M = ws + pl.M; f.S = ws + pl.S;
    f.mu = ws + pl.mu; f.Sig = ws + pl.Sig;
    f.E = E; f.D = D; f.A = A; f.H = H;
    f.include_time = a.include_time; f.time0 = a.time0;
    for (int d = 0; d < D; ++d) f.mu0[d] = a.mu0[d];
    for (int d = 0; d < D * D; ++d) f.S0[d] = a.S0[d];
    f.gain_stride = per_candidate ? (long long)H * A * D : 0;
    q.cost = a.cost; q.cv = ws + pl.cv; q.keepV = ws + pl.keepV; q.rows_stride = pl.chunk;
    q.adj = ws + pl.adj; q.Mb = ws + pl.Mb; q.Sb = ws + pl.Sb; q.Vb = ws + pl.Vb; q.xb = ws + pl.xb; q.Pb = ws + pl.Pb;
    q.kappa = a.kappa; q.use_constraints = a.use_constraints;
    const size_t T1 = (size_t)(H + 1);
    const size_t stepV = (size_t)pl.chunk * E * D;
    for (long long b0 = 0; b0 < B; b0 += pl.chunk) {
        const int rows = (int)((B - b0) < pl.chunk ? (B - b0) : pl.chunk);
        const size_t o = (size_t)b0;
        f.actions = a.actions + o * H * A;
        f.gains = gains + o * (size_t)f.gain_stride;
        q.actions_bar = actions_bar + o * H * A;
        q.gains_bar = gains_bar ? gains_bar + o * H * A * D : nullptr;
        q.sd.mu = sd.mu ? sd.mu + o * T1 * D : nullptr;
        q.sd.Sig = sd.Sig ? sd.Sig + o * T1 * D * D : nullptr;
        q.sd.cm = sd.cm ? sd.cm + o * T1 : nullptr;
        q.sd.cv = sd.cv ? sd.cv + o * T1 : nullptr;
        q.sd.J = sd.J ? sd.J + o : nullptr;
        q.sd.mu0_bar = sd.mu0_bar ? sd.mu0_bar + o * D : nullptr;
        q.sd.S0_bar = sd.S0_bar ? sd.S0_bar + o * D * D : nullptr;
        // the forward, recomputed: every step's V goes straight into keepV
        f.t = 0;
        hipLaunchKernelGGL(rollout_feedback_init_kernel, dim3(rows), dim3(64), 0, s, f);
        for (int t = 0; t < H; ++t) {
            double* Vt = ws + pl.keepV + (size_t)t * stepV;
            rc = run_moments(h, f.xin, f.sin, rows, ws + pl.M, ws + pl.S, Vt, s);
            if (rc) return rc;
            f.t = t;
            f.V = Vt;
            hipLaunchKernelGGL(rollout_feedback_step_kernel, dim3(rows), dim3(64), 0, s, f);
        }
        GPMPC_HIP_CHECK(h, hipGetLastError());
        if (sd.J) {                                   // the objective's weights need the closed-loop cost variances
            rc = launch_traj_cost_feedback(h, a, rows, f.mu, f.Sig, f.actions, f.gains, f.gain_stride, nullptr, ws + pl.cv, nullptr,
                                           s);
            if (rc) return rc;
        }
        // the reverse sweep
        hipLaunchKernelGGL(rollout_feedback_bwd_reverse_kernel, dim3(rows), dim3(64), 0, s, q, -1, H - 1);
        for (int t = H - 1; t >= 0; --t) {
            rc = run_moments_backward(h, f.xin, f.sin, rows, q.Mb, q.Sb, q.Vb, ws + pl.xb, ws + pl.Pb, s);
            if (rc) return rc;
            hipLaunchKernelGGL(rollout_feedback_bwd_reverse_kernel, dim3(rows), dim3(64), 0, s, q, t, t - 1);
        }
        GPMPC_HIP_CHECK(h, hipGetLastError());
    }
    return GPMPC_OK;
}

}  // namespace gpmpc_hip
