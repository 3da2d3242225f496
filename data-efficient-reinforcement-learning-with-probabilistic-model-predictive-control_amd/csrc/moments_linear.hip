// moments_linear.hip -- first-order (linearised) propagation of a Gaussian input through the GP posterior (gpmpc_moments_linear)
// and the horizon rollout built on it (gpmpc_rollout_linear).  Per point with input mean m (E), covariance Sigma (E x E), output a:
//   k_aj = sigma2_a exp(-1/2 sum_e (m_e - x_je)^2 / l_ae^2)
//   M_a = sum_j k_aj beta_aj                              posterior mean at m
//   V[e,a] = (1 / l_ae^2) sum_j beta_aj k_aj (x_je - m_e)   its Jacobian dM_a / dm_e
//   v_a = sigma2_a - k_a^T iK_a k_a                       posterior variance at m (not clamped, no noise)
//   S = V^T Sigma V + diag(v)
// from the cached Xt / ils2 / var / beta / iK.  The differences x_je - m_e are formed per element: the factored form
// sum_j c x_j - m sum_j c cancels digits with a time input.
//
// Structure ("Linearised propagation"):
//   lin_tile_kernel<EP, KLOOP, false>   (moments_linear_kernels.h, shared with the gradients) one workgroup per (64 rows, 256-column
//                                 block of iK_a, output a): per row it leaves the block's partial sums
//                                 sum_j P_mj k_mj | sum_j k_mj beta_j | E sums beta_j k_mj (x_je - m_e),  P = K*_a iK_a.  Without S
//                                 the k loop that forms P is compiled out.
//   moments_linear_finish_kernel  one wavefront per point: adds the column blocks in block order, scales the Jacobian, forms
//                                 Sigma V and V^T (Sigma V) for a <= b and mirrors.
//   rollout_linear_init_kernel /  (moments_linear_kernels.h) the rollout is batch-major: per horizon step one tile launch over all
//   rollout_linear_step_kernel<FB>   candidates of the chunk, then one wavefront per candidate adds the blocks, advances (mu, Sigma)
//                                 in the stored trajectory
//                                   mu' = mu + M,  T = Sigma V_s,  Sigma' = Sigma + (V_s^T Sigma V_s + diag v) + T + T^T
//                                 (V_s: the state rows of V) and writes the next step's model inputs [mu' | action | time0 + t + 1].
//   closed loop (FB) /            gpmpc_rollout_linear_feedback: the same init kernel and tile launches; the step's FB instantiation
//   traj_cost_feedback_kernel     uses C = V_s + K_t^T V_u in place of V_s, the cost kernel the state-action covariance
//                                 [I ; K_t] Sigma_t [I ; K_t]^T in place of block_diag(Sigma_t, 0).
// Every sum runs in an order fixed by N, E and D alone (k steps, lanes, waves, slices, column blocks): a point's bits do not depend
// on the batch size, on its place in the batch, on its neighbours or on the chunks.  Plain kernels: no atomics, no waits between
// workgroups.  The workspace (Handle::linws) is this file's own, sized by plan_moments_linear (moments_linear_plan.h); a chunk of
// candidates runs its whole horizon.  There is no fused-horizon form: with few candidates a 64-row tile is mostly padding and
// every step costs two launches.
#include "moments_linear_kernels.h"

namespace gpmpc_hip {

namespace {

struct LinFinishArgs {
    const double* part;
    const double* ils2;      // (D, E)
    const double* var;       // (D)
    const double* Sig;       // (rows, E, E) of this chunk, or NULL (= 0)
    double* M_out;           // (rows, D) of this chunk, or NULL
    double* S_out;           // (rows, D, D) of this chunk, or NULL
    double* V_out;           // (rows, E, D) of this chunk, or NULL
    int rows, E, D, nCB, NW;
    long long Mc;
};

// One wavefront per point.
__global__ __launch_bounds__(64) void moments_linear_finish_kernel(LinFinishArgs p) {
    __shared__ double s_sum[kMaxD][kMaxE + 2];
    __shared__ double s_V[kMaxE][kMaxD];
    __shared__ double s_T[kMaxE][kMaxD];
    const int m = blockIdx.x, tid = threadIdx.x;
    const int D = p.D, E = p.E, NW = p.NW;
    const bool with_S = p.S_out != nullptr;
    for (int idx = tid; idx < D * NW; idx += 64) {
        const int a = idx / NW, which = idx - a * NW;
        s_sum[a][which] = (which == 0 && !with_S) ? 0.0 : block_sum(p.part, a, which, (size_t)m, p.nCB, NW, (size_t)p.Mc);
    }
    __syncthreads();
    for (int idx = tid; idx < E * D; idx += 64) {
        const int e = idx / D, a = idx - e * D;
        const double v = p.ils2[a * E + e] * s_sum[a][2 + e];
        s_V[e][a] = v;
        if (p.V_out) p.V_out[(size_t)m * E * D + idx] = v;
    }
    if (p.M_out && tid < D) p.M_out[(size_t)m * D + tid] = s_sum[tid][1];
    if (!with_S) return;
    __syncthreads();
    if (p.Sig) {
        const double* Sg = p.Sig + (size_t)m * E * E;
        for (int idx = tid; idx < E * D; idx += 64) {            // T = Sigma V
            const int e = idx / D, b = idx - e * D;
            double t = 0.0;
            for (int f = 0; f < E; ++f) t = fma(Sg[e * E + f], s_V[f][b], t);
            s_T[e][b] = t;
        }
        __syncthreads();
    }
    double* S = p.S_out + (size_t)m * D * D;
    for (int idx = tid; idx < D * D; idx += 64) {                // a <= b, mirrored: exactly symmetric
        const int a = idx / D, b = idx - a * D;
        if (a > b) continue;
        double q = 0.0;
        if (p.Sig)
            for (int e = 0; e < E; ++e) q = fma(s_V[e][a], s_T[e][b], q);
        if (a == b) q += p.var[a] - s_sum[a][0];                 // not clamped
        S[a * D + b] = q;
        S[b * D + a] = q;
    }
}

// Stage / terminal costs and the objective of the closed-loop trajectory: traj_cost_body (one wavefront per candidate, lanes over
// the H + 1 steps, wave_xor_sum for J) with the state-action covariance Sigma_z = G Sigma_t G^T, G = [I ; K_t], in place of
// block_diag(Sigma_t, 0).  Sigma_z enters the quadratic cost only through
//   tr(Sigma_z W) = tr(Sigma_t Wg),  tr(2 (W Sigma_z)^2) = tr(2 (Wg Sigma_t)^2),  e^T W Sigma_z W e = (G^T W^T e)^T Sigma_t (G^T W e)
// with Wg = G^T W G, so a lane keeps D^2 + 2 D values (DP: the array bound) instead of (D + A)^2.  Terminal step: G = I, W = W_T.
template <int DP>
__global__ __launch_bounds__(64) void traj_cost_feedback_kernel(const double* __restrict__ mu, const double* __restrict__ Sig,
                                                                const double* __restrict__ actions,
                                                                const double* __restrict__ gains, long long gain_stride,
                                                                const double* __restrict__ cost, int D, int A, int H,
                                                                double kappa, int clip, int use_constraints,
                                                                double* __restrict__ cm_out, double* __restrict__ cv_out,
                                                                double* __restrict__ J_out) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int DA = D + A;
    const double* target = cost;
    const double* W = cost + DA;
    const double* WT = W + DA * DA;
    const double* smin = WT + D * D;
    const double* smax = smin + D;
    double jsum = 0.0;
    for (int t = lane; t <= H; t += 64) {
        const bool terminal = (t == H);
        const int n = terminal ? D : DA, Au = terminal ? 0 : A;
        const double* Wm = terminal ? WT : W;
        const double* m = mu + ((size_t)c * (H + 1) + t) * D;
        const double* S = Sig + ((size_t)c * (H + 1) + t) * D * D;
        const double* a = actions + ((size_t)c * H + (terminal ? 0 : t)) * A;
        const double* K = gains + (size_t)c * (size_t)gain_stride + (size_t)(terminal ? 0 : t) * A * D;      // [action][state]
        auto err = [&](int i) { return (i < D ? m[i] : a[i - D]) - target[i]; };
        double Wg[DP * DP], p1[DP], p2[DP];
        for (int i = 0; i < D; ++i) {
            for (int j = 0; j < D; ++j) {
                double w = Wm[i * n + j];
                for (int u = 0; u < Au; ++u) {
                    w = fma(Wm[i * n + D + u], K[u * D + j], w);
                    w = fma(K[u * D + i], Wm[(D + u) * n + j], w);
                    double kw = 0.0;
                    for (int v = 0; v < Au; ++v) kw = fma(Wm[(D + u) * n + D + v], K[v * D + j], kw);
                    w = fma(K[u * D + i], kw, w);
                }
                Wg[i * DP + j] = w;
            }
            double v1 = 0.0, v2 = 0.0;                           // (G^T W^T e)_i, (G^T W e)_i
            for (int k = 0; k < n; ++k) {
                v1 = fma(err(k), Wm[k * n + i], v1);
                v2 = fma(Wm[i * n + k], err(k), v2);
            }
            for (int u = 0; u < Au; ++u) {
                double r1 = 0.0, r2 = 0.0;
                for (int k = 0; k < n; ++k) {
                    r1 = fma(err(k), Wm[k * n + D + u], r1);
                    r2 = fma(Wm[(D + u) * n + k], err(k), r2);
                }
                v1 = fma(K[u * D + i], r1, v1);
                v2 = fma(K[u * D + i], r2, v2);
            }
            p1[i] = v1;
            p2[i] = v2;
        }
        double cm = 0.0, cv = 0.0;
        // tr(Sigma Wg) and e^T W e
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) cm = fma(S[i * D + j], Wg[j * DP + i], cm);
        for (int i = 0; i < n; ++i) {
            const double ei = err(i);
            for (int j = 0; j < n; ++j) cm = fma(ei * Wm[i * n + j], err(j), cm);
        }
        // tr(2 TS TS) with TS = Wg Sigma, 4 p1^T Sigma p2
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) {
                double tij = 0.0, tji = 0.0;
                for (int k = 0; k < D; ++k) {
                    tij = fma(Wg[i * DP + k], S[k * D + j], tij);
                    tji = fma(Wg[j * DP + k], S[k * D + i], tji);
                }
                cv = fma(2.0 * tij, tji, cv);
                cv = fma(4.0 * p1[i] * S[i * D + j], p2[j], cv);
            }
        if (use_constraints && !terminal) {                      // state marginals only, as traj_cost_body
            for (int d = 0; d < D; ++d) {
                const double sg = S[d * D + d];
                cm += 0.5 * (1.0 + erf((smin[d] - m[d]) / (sg * 1.4142135623730951)))
                    + (1.0 - 0.5 * (1.0 + erf((smax[d] - m[d]) / (sg * 1.4142135623730951))));
            }
        }
        double ucb = -cm + kappa * sqrt(cv);
        if (clip) ucb = fmin(ucb, 0.0);
        jsum -= ucb;
        if (cm_out) cm_out[(size_t)c * (H + 1) + t] = cm;
        if (cv_out) cv_out[(size_t)c * (H + 1) + t] = cv;
    }
    jsum = wave_xor_sum(jsum);
    if (lane == 0 && J_out) J_out[c] = jsum / (double)(H + 1);
}

}  // namespace

int launch_traj_cost_feedback(Handle* h, const RolloutArgs& a, int rows, const double* mu, const double* Sig, const double* actions,
                              const double* gains, long long gain_stride, double* cm, double* cv, double* J, hipStream_t s) {
    const int D = a.D, A = a.A, H = a.H;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(rows), dim3(64), 0, s, mu, Sig, actions, gains, gain_stride, a.cost, D, A, H, a.kappa,
                           a.clip, a.use_constraints, cm, cv, J);
    };
    static_assert(kMaxD <= 16, "traj_cost_feedback_kernel: per-lane arrays");
    if (D <= 4) launch(traj_cost_feedback_kernel<4>);
    else if (D <= 8) launch(traj_cost_feedback_kernel<8>);
    else launch(traj_cost_feedback_kernel<16>);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

int run_moments_linear(Handle* h, const double* mu, const double* Sig, int P, double* M_out, double* S_out, double* V_out,
                       hipStream_t s) {
    const int N = h->N, D = h->D, E = h->E;
    if (P == 0 || (!M_out && !S_out && !V_out)) return GPMPC_OK;
    LinearPlan pl;
    plan_moments_linear(N, D, E, P, 0, false, h->opt_moments_linear_chunk, pl);
    int rc = grow(h, h->linws, pl.total);
    if (rc) return rc;
    LinTileArgs p{};
    p.Xt = h->Xt.p; p.ils2 = h->ils2.p; p.var = h->var.p; p.beta = h->beta.p; p.iK = h->iK.p;
    p.part = h->linws.p;
    p.N = N; p.E = E; p.D = D; p.nCB = pl.nCB; p.NW = pl.NW; p.Mc = pl.Mc;
    LinFinishArgs f{};
    f.part = p.part; f.ils2 = p.ils2; f.var = p.var;
    f.E = E; f.D = D; f.nCB = pl.nCB; f.NW = pl.NW; f.Mc = pl.Mc;
    for (long long m0 = 0; m0 < P; m0 += pl.chunk) {
        const int rows = (int)((P - m0) < pl.chunk ? (P - m0) : pl.chunk);
        p.rows = rows;
        p.Xq = mu + (size_t)m0 * E;
        launch_lin_tiles<false>(p, S_out != nullptr, s);
        f.rows = rows;
        f.Sig = Sig ? Sig + (size_t)m0 * E * E : nullptr;
        f.M_out = M_out ? M_out + (size_t)m0 * D : nullptr;
        f.S_out = S_out ? S_out + (size_t)m0 * D * D : nullptr;
        f.V_out = V_out ? V_out + (size_t)m0 * E * D : nullptr;
        hipLaunchKernelGGL(moments_linear_finish_kernel, dim3(rows), dim3(64), 0, s, f);
    }
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

// a: filled by the entry point (model, cost settings, actions, shape, initial state, outputs -- each output may be NULL).
// gains != NULL: the closed-loop rollout under u = ubar_t + K_t (x - mu_t), gains (B, H, A, D) when per_candidate, else (H, A, D)
// shared by all candidates -- the same plan, workspace, init kernel and tile launches with the step kernel's FB form and the
// closed-loop cost kernel; a chunk of candidates offsets the gain pointer only when the gains are per candidate.
int run_rollout_linear(Handle* h, const RolloutArgs& a, hipStream_t s, const double* gains, bool per_candidate) {
    const int N = a.N, D = a.D, E = a.E, A = a.A, H = a.H, B = a.B;
    const bool own_traj = !a.mu_out || !a.Sig_out;
    const bool costs = a.cm_out || a.cv_out || a.J_out;
    LinearPlan pl;
    plan_moments_linear(N, D, E, B, H, own_traj, h->opt_moments_linear_chunk, pl);
    int rc = grow(h, h->linws, pl.total);
    if (rc) return rc;
    LinTileArgs p{};
    p.Xt = h->Xt.p; p.ils2 = h->ils2.p; p.var = h->var.p; p.beta = h->beta.p; p.iK = h->iK.p;
    p.part = h->linws.p;
    p.Xq = h->linws.p + pl.part;
    p.N = N; p.E = E; p.D = D; p.nCB = pl.nCB; p.NW = pl.NW; p.Mc = pl.Mc;
    double* own_mu = h->linws.p + pl.part + pl.xq;
    double* own_Sig = own_mu + (size_t)pl.chunk * (H + 1) * D;
    LinStepArgs q{};
    q.part = p.part; q.ils2 = p.ils2; q.var = p.var;
    q.Xq = h->linws.p + pl.part;
    q.E = E; q.D = D; q.A = A; q.H = H; q.nCB = pl.nCB; q.NW = pl.NW; q.Mc = pl.Mc;
    q.include_time = a.include_time; q.time0 = a.time0;
    for (int d = 0; d < D; ++d) q.mu0[d] = a.mu0[d];
    for (int d = 0; d < D * D; ++d) q.S0[d] = a.S0[d];
    q.gain_stride = per_candidate ? (long long)H * A * D : 0;
    for (long long b0 = 0; b0 < B; b0 += pl.chunk) {
        const int rows = (int)((B - b0) < pl.chunk ? (B - b0) : pl.chunk);
        p.rows = rows;
        q.actions = a.actions + (size_t)b0 * H * A;
        q.gains = gains ? gains + (size_t)b0 * (size_t)q.gain_stride : nullptr;
        q.mu = a.mu_out ? a.mu_out + (size_t)b0 * (H + 1) * D : own_mu;
        q.Sig = a.Sig_out ? a.Sig_out + (size_t)b0 * (H + 1) * D * D : own_Sig;
        q.t = 0;
        hipLaunchKernelGGL(rollout_linear_init_kernel, dim3(rows), dim3(64), 0, s, q);
        for (int t = 0; t < H; ++t) {
            launch_lin_tiles<false>(p, true, s);
            q.t = t;
            if (gains) hipLaunchKernelGGL(rollout_linear_step_kernel<true>, dim3(rows), dim3(64), 0, s, q);
            else hipLaunchKernelGGL(rollout_linear_step_kernel<false>, dim3(rows), dim3(64), 0, s, q);
        }
        GPMPC_HIP_CHECK(h, hipGetLastError());
        if (costs && gains) {                         // closed-loop stage costs + objective of the chunk's stored trajectory
            double* cm = a.cm_out ? a.cm_out + (size_t)b0 * (H + 1) : nullptr;
            double* cv = a.cv_out ? a.cv_out + (size_t)b0 * (H + 1) : nullptr;
            double* J = a.J_out ? a.J_out + b0 : nullptr;
            rc = launch_traj_cost_feedback(h, a, rows, q.mu, q.Sig, q.actions, q.gains, q.gain_stride, cm, cv, J, s);
            if (rc) return rc;
        } else if (costs) {                           // stage costs + objective of the chunk's stored trajectory
            RolloutArgs c = a;
            c.B = rows;
            c.actions = q.actions;
            c.mu_out = q.mu; c.Sig_out = q.Sig;
            rc = launch_traj_cost(h, c, a.cm_out ? a.cm_out + (size_t)b0 * (H + 1) : nullptr,
                                  a.cv_out ? a.cv_out + (size_t)b0 * (H + 1) : nullptr, a.J_out ? a.J_out + b0 : nullptr, s);
            if (rc) return rc;
        }
    }
    return GPMPC_OK;
}

}  // namespace gpmpc_hip
