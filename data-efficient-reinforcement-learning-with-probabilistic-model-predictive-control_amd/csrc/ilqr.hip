// ilqr.hip -- device-resident clamped iLQR on the mean dynamics of the linearised propagation (include/gpmpc.h: gpmpc_ilqr_backward /
// _forward / _init / _step / _search).  Per candidate (B of them in lockstep) with ubar (H, A) in [0, 1]:
//   dynamics  x_{t+1} = x_t + M([x_t | u_t | time0 + t]), x_0 = mu0 (the posterior mean of gpmpc_moments_linear);
//   cost      c = (sum_{t<H} e_t^T W_s e_t + e_H^T P_H e_H) / (H + 1) on the block loaded by gpmpc_set_cost.
// CERTAINTY-EQUIVALENT: kappa, the variance terms, clipping of the cost and the state constraints do not enter.  CLAMPED: the box is
// honoured by clipping the realised action of the forward pass, not by a box QP in the sweep.
//
// Structure ("iLQR"):
//   backward   per horizon step lqr_inputs_kernel + run_moments_linear (S NULL, V wanted) exactly as gpmpc_lqr_gains, with the
//              nominal trajectory stored; then ilqr_cost_kernel (nominal cost) and lqr_riccati_kernel<true> (lqr_riccati_kernel.h:
//              the Riccati recurrence of gpmpc_lqr_gains plus the affine terms, one wavefront per candidate).
//   forward    rows = chunk x L (candidate, step size): per horizon step ilqr_forward_kernel, one thread per (row, model input) --
//              u_t = clip(ubar_t + alpha k_t + K_t (x_t - xbar_t)), x += M (the operation of rollout_linear_step_kernel), the next
//              model input -- then run_moments_linear (S NULL, V NULL: M only); then ilqr_cost_kernel on the trial trajectories.
//   ilqr_cost_kernel   one wavefront per trajectory, lanes over the H + 1 steps, wave_xor_sum.  The one cost kernel of the nominal
//              and of every trial trajectory: equal trajectories get equal bits.
//   ilqr_accept_kernel one wavefront per candidate: status, the walk over the L trial costs in index order, accept / reject, reg.
// The launch sequence depends on the arguments alone; nothing is read back.  Plain kernels: no atomics, no waits between workgroups;
// every sum runs in an order fixed by N, E, D, A, H and L alone, so a candidate's bits depend neither on the batch nor on its place
// nor on the chunks.  The workspace (Handle::ilqrws) is this file's own, sized by plan_ilqr (ilqr_plan.h); run_moments_linear and
// run_rollout_linear keep using theirs (Handle::linws).
#include "lqr_riccati_kernel.h"
#include "ilqr_plan.h"
#include "ilqr_state.h"

namespace gpmpc_hip {

namespace {

// NaN stays NaN (fmin / fmax would turn it into a bound): a non-finite start must reach the cost
__device__ inline double ilqr_clip01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }

struct IlqrForwardArgs {
    const double* actions;   // (cands, H, A) nominal, of this chunk
    const double* gains;     // (cands, H, A, D)
    const double* ff;        // (cands, H, A)
    const double* mu_nom;    // (cands, H + 1, D)
    const double* M;         // (rows, D) of the step before
    double* Xq;              // (rows, E)
    double* tmu;             // (rows, H + 1, D) trial trajectories
    double* tact;            // (rows, H, A) trial actions
    int rows, L, E, D, A, H, t;
    double time0;
    double alphas[kIlqrMaxL];
    double mu0[kMaxD];
};

// Step t of the forward pass for row r = (candidate, step size): the state of step t (t = 0: mu0; else the stored state of the step
// before + M, read from the stored trajectory so that no thread depends on another's store of this launch), the realised action, the
// model input.  t = H: the last state alone.
__global__ __launch_bounds__(256) void ilqr_forward_kernel(IlqrForwardArgs p) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)p.rows * p.E) return;
    const int r = (int)(idx / p.E), e = (int)(idx - (long long)r * p.E);
    const int D = p.D, A = p.A, H = p.H, t = p.t;
    const int b = r / p.L, l = r - b * p.L;
    double* tm = p.tmu + (size_t)r * (H + 1) * D;
    const double* Mr = p.M + (size_t)r * D;
    auto state = [&](int d) { return t == 0 ? p.mu0[d] : tm[(size_t)(t - 1) * D + d] + Mr[d]; };
    double* xq = p.Xq + (size_t)r * p.E;
    if (e < D) {
        const double x = state(e);
        tm[(size_t)t * D + e] = x;
        xq[e] = x;
    } else if (t == H) {
        return;
    } else if (e < D + A) {
        const int a = e - D;
        const double* K = p.gains + (((size_t)b * H + t) * A + a) * D;
        const double* xn = p.mu_nom + ((size_t)b * (H + 1) + t) * D;
        double fb = 0.0;
        for (int d = 0; d < D; ++d) fb = fma(K[d], state(d) - xn[d], fb);
        const size_t ia = ((size_t)b * H + t) * A + a;
        const double u = ilqr_clip01(fma(p.alphas[l], p.ff[ia], p.actions[ia]) + fb);
        p.tact[((size_t)r * H + t) * A + a] = u;
        xq[e] = u;
    } else xq[e] = p.time0 + (double)t;
}

// One wavefront per trajectory: c = (sum_{t<H} e_t^T W_s e_t + e_H^T P_H e_H) / (H + 1), e_t = [x_t | u_t] - target.
__global__ __launch_bounds__(64) void ilqr_cost_kernel(const double* __restrict__ mu, const double* __restrict__ actions,
                                                       const double* __restrict__ cost, int D, int A, int H,
                                                       double* __restrict__ out, int out_stride) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int DA = D + A;
    const double* target = cost;
    const double* W = cost + DA;
    const double* WT = W + DA * DA;
    double sum = 0.0;
    for (int t = lane; t <= H; t += 64) {
        const bool terminal = (t == H);
        const int n = terminal ? D : DA;
        const double* Wm = terminal ? WT : W;
        const double* m = mu + ((size_t)c * (H + 1) + t) * D;
        const double* a = actions + ((size_t)c * H + (terminal ? 0 : t)) * A;
        auto err = [&](int i) { return (i < D ? m[i] : a[i - D]) - target[i]; };
        double ct = 0.0;
        for (int i = 0; i < n; ++i) {
            double row = 0.0;                                        // (W_s e)_i
            for (int j = 0; j < n; ++j) row = fma(0.5 * (Wm[i * n + j] + Wm[j * n + i]), err(j), row);
            ct = fma(err(i), row, ct);
        }
        sum += ct;
    }
    sum = wave_xor_sum(sum);
    if (lane == 0) out[(size_t)c * out_stride] = sum / (double)(H + 1);
}

struct IlqrAcceptArgs {
    double* state;
    int B, H, A, D, L;
    double reg0, reg_factor, reg_max, tol;
};

// One wavefront per candidate; every lane takes the same decisions, the lanes share the copy of the accepted actions.
__global__ __launch_bounds__(64) void ilqr_accept_kernel(const IlqrAcceptArgs p) {
    const int b = blockIdx.x, lane = threadIdx.x, n = p.H * p.A;
    const IlqrLayout Y = make_ilqr_layout(p.B, p.H, p.A, p.D, p.L);
    double* st = p.state;
    if (st[Y.status + b] != 0.0) return;              // (uniform) a finished candidate: its state no longer changes
    const double cost = st[Y.cost + b];
    if (!finite_d(cost)) {
        if (lane == 0) { st[Y.status + b] = 3.0; st[Y.chosen + b] = -1.0; }
        return;
    }
    if (st[Y.step + b] <= p.tol) {
        if (lane == 0) { st[Y.status + b] = 1.0; st[Y.chosen + b] = -1.0; }
        return;
    }
    const double* tc = st + Y.trial_cost + (size_t)b * p.L;
    int best = -1;
    double bestc = 0.0;
    for (int l = 0; l < p.L; ++l) {                   // the finite trial of lowest cost, ties to the smallest l
        const double c = tc[l];
        if (finite_d(c) && (best < 0 || c < bestc)) { best = l; bestc = c; }
    }
    const double reg = st[Y.reg + b];
    if (best >= 0 && bestc < cost) {
        const double* src = st + Y.trial_actions + ((size_t)b * p.L + best) * n;
        double* dst = st + Y.actions + (size_t)b * n;
        for (int i = lane; i < n; i += kWave) dst[i] = src[i];
        if (lane == 0) {
            st[Y.cost + b] = bestc;
            st[Y.reg + b] = fmax(reg / p.reg_factor, p.reg0);
            st[Y.accepts + b] += 1.0;
            st[Y.chosen + b] = (double)best;
        }
    } else if (lane == 0) {
        const double r = reg * p.reg_factor;
        st[Y.chosen + b] = -1.0;
        st[Y.reg + b] = r;
        if (r > p.reg_max) st[Y.status + b] = 2.0;
    }
}

struct IlqrInitArgs {
    const double* x0;
    double* state;
    int B, H, A, D, L;
    double reg0;
};

// actions = clip(x0), reg = reg0, chosen = -1, everything else 0
__global__ __launch_bounds__(256) void ilqr_init_kernel(const IlqrInitArgs p) {
    const IlqrLayout Y = make_ilqr_layout(p.B, p.H, p.A, p.D, p.L);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= Y.total) return;
    double v = 0.0;
    if (i < Y.cost) v = ilqr_clip01(p.x0[i]);
    else if (i >= Y.reg && i < Y.status) v = p.reg0;
    else if (i >= Y.chosen && i < Y.dV) v = -1.0;
    p.state[i] = v;
}

// where the backward pass leaves a candidate's scalars: element b of each at [b * stride]
struct IlqrInfo {
    double* cost;
    double* dV;
    double* step;
    double* flags;
    double* reserved;        // or NULL
    int stride;
};

int backward(Handle* h, const double* actions, const double* mu0_host, int B, int H, int A, int include_time, double time0,
             const double* reg_dev, const double* status, double* gains, double* ff, double* mu, const IlqrInfo& info, int L_plan,
             hipStream_t s) {
    const int D = h->D, E = h->E;
    IlqrPlan pl;
    plan_ilqr(D, E, H, L_plan, B, h->opt_ilqr_chunk, pl);
    int rc = grow(h, h->ilqrws, pl.total);
    if (rc) return rc;
    double* ws = h->ilqrws.p;
    LqrInputArgs in{};
    in.Xq = ws + pl.xq; in.M = ws + pl.M;
    in.E = E; in.D = D; in.A = A; in.H = H; in.include_time = include_time; in.time0 = time0;
    for (int d = 0; d < D; ++d) in.mu0[d] = mu0_host[d];
    LqrRiccatiArgs r{};
    r.V = ws + pl.V; r.cost = h->cost.p;
    r.E = E; r.D = D; r.A = A; r.H = H; r.info_stride = info.stride;
    for (long long b0 = 0; b0 < B; b0 += pl.chunk) {
        const int rows = (int)((B - b0) < pl.chunk ? (B - b0) : pl.chunk);
        in.rows = rows;
        in.actions = actions + (size_t)b0 * H * A;
        in.mu = mu + (size_t)b0 * (H + 1) * D;
        const unsigned blocks = (unsigned)(((long long)rows * E + 255) / 256);
        for (int t = 0; t <= H; ++t) {
            in.t = t;
            hipLaunchKernelGGL(lqr_inputs_kernel, dim3(blocks), dim3(256), 0, s, in);
            if (t == H) break;
            rc = run_moments_linear(h, ws + pl.xq, nullptr, rows, ws + pl.M, nullptr, ws + pl.V + (size_t)t * rows * E * D, s);
            if (rc) return rc;
        }
        const size_t io = (size_t)b0 * info.stride;
        hipLaunchKernelGGL(ilqr_cost_kernel, dim3(rows), dim3(64), 0, s, in.mu, in.actions, h->cost.p, D, A, H, info.cost + io,
                           info.stride);
        r.rows = rows;
        r.gains = gains + (size_t)b0 * H * A * D;
        r.reg_dev = reg_dev + b0;
        r.status = status ? status + b0 : nullptr;
        r.mu = in.mu;
        r.actions = in.actions;
        r.ff = ff + (size_t)b0 * H * A;
        r.dV = info.dV + io; r.step = info.step + io; r.fflags = info.flags + io;
        r.reserved = info.reserved ? info.reserved + io : nullptr;
        hipLaunchKernelGGL(lqr_riccati_kernel<true>, dim3(rows), dim3(64), 0, s, r);
        GPMPC_HIP_CHECK(h, hipGetLastError());
    }
    return GPMPC_OK;
}

int forward(Handle* h, const double* actions, const double* gains, const double* ff, const double* mu_nom, const double* mu0_host,
            int B, int H, int A, int include_time, double time0, const double* alphas_host, int L, double* trial_actions,
            double* trial_cost, double* trial_mu, hipStream_t s) {
    const int D = h->D, E = h->E;
    IlqrPlan pl;
    plan_ilqr(D, E, H, L, B, h->opt_ilqr_chunk, pl);
    int rc = grow(h, h->ilqrws, pl.total);
    if (rc) return rc;
    double* ws = h->ilqrws.p;
    IlqrForwardArgs f{};
    f.Xq = ws + pl.xq; f.M = ws + pl.M;
    f.L = L; f.E = E; f.D = D; f.A = A; f.H = H; f.time0 = time0;
    for (int l = 0; l < L; ++l) f.alphas[l] = alphas_host[l];
    for (int d = 0; d < D; ++d) f.mu0[d] = mu0_host[d];
    (void)include_time;                                      // (E = D + A + 1 says it)
    for (long long b0 = 0; b0 < B; b0 += pl.chunk) {
        const int cands = (int)((B - b0) < pl.chunk ? (B - b0) : pl.chunk);
        const int rows = cands * L;
        f.rows = rows;
        f.actions = actions + (size_t)b0 * H * A;
        f.gains = gains + (size_t)b0 * H * A * D;
        f.ff = ff + (size_t)b0 * H * A;
        f.mu_nom = mu_nom + (size_t)b0 * (H + 1) * D;
        f.tmu = trial_mu ? trial_mu + (size_t)b0 * L * (H + 1) * D : ws + pl.tmu;
        f.tact = trial_actions + (size_t)b0 * L * H * A;
        const unsigned blocks = (unsigned)(((long long)rows * E + 255) / 256);
        for (int t = 0; t <= H; ++t) {
            f.t = t;
            hipLaunchKernelGGL(ilqr_forward_kernel, dim3(blocks), dim3(256), 0, s, f);
            if (t == H) break;
            rc = run_moments_linear(h, ws + pl.xq, nullptr, rows, ws + pl.M, nullptr, nullptr, s);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(ilqr_cost_kernel, dim3(rows), dim3(64), 0, s, f.tmu, f.tact, h->cost.p, D, A, H,
                           trial_cost + (size_t)b0 * L, 1);
        GPMPC_HIP_CHECK(h, hipGetLastError());
    }
    return GPMPC_OK;
}

}  // namespace

int run_ilqr_backward(Handle* h, const double* actions, const double* mu0_host, int B, int H, int A, int include_time, double time0,
                      const double* reg_dev, double* gains_out, double* ff_out, double* mu_out, double* info_out, hipStream_t s) {
    const IlqrInfo info{info_out, info_out + 1, info_out + 2, info_out + 3, info_out + 4, 5};
    return backward(h, actions, mu0_host, B, H, A, include_time, time0, reg_dev, nullptr, gains_out, ff_out, mu_out, info, 1, s);
}

int run_ilqr_forward(Handle* h, const double* actions, const double* gains, const double* ff, const double* mu_nom,
                     const double* mu0_host, int B, int H, int A, int include_time, double time0, const double* alphas_host, int L,
                     double* trial_actions_out, double* trial_cost_out, double* trial_mu_out, hipStream_t s) {
    return forward(h, actions, gains, ff, mu_nom, mu0_host, B, H, A, include_time, time0, alphas_host, L, trial_actions_out,
                   trial_cost_out, trial_mu_out, s);
}

int run_ilqr_init(Handle* h, const double* x0_dev, int B, int H, int A, int L, double reg0, double* state_dev, hipStream_t s) {
    IlqrInitArgs p;
    p.x0 = x0_dev; p.state = state_dev; p.B = B; p.H = H; p.A = A; p.D = h->D; p.L = L; p.reg0 = reg0;
    const size_t total = make_ilqr_layout(B, H, A, h->D, L).total;
    hipLaunchKernelGGL(ilqr_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

int run_ilqr_step(Handle* h, const double* mu0_host, int B, int H, int A, int include_time, double time0, int L, double reg0,
                  double reg_factor, double reg_max, double tol, double* st, hipStream_t s) {
    const IlqrLayout Y = make_ilqr_layout(B, H, A, h->D, L);
    const IlqrInfo info{st + Y.cost, st + Y.dV, st + Y.step, st + Y.flags, nullptr, 1};
    int rc = backward(h, st + Y.actions, mu0_host, B, H, A, include_time, time0, st + Y.reg, st + Y.status, st + Y.gains, st + Y.ff,
                      st + Y.mu, info, L, s);
    if (rc) return rc;
    double alphas[kIlqrMaxL];
    double al = 1.0;
    for (int l = 0; l < L; ++l, al *= 0.5) alphas[l] = al;
    rc = forward(h, st + Y.actions, st + Y.gains, st + Y.ff, st + Y.mu, mu0_host, B, H, A, include_time, time0, alphas, L,
                 st + Y.trial_actions, st + Y.trial_cost, nullptr, s);
    if (rc) return rc;
    IlqrAcceptArgs p;
    p.state = st; p.B = B; p.H = H; p.A = A; p.D = h->D; p.L = L;
    p.reg0 = reg0; p.reg_factor = reg_factor; p.reg_max = reg_max; p.tol = tol;
    hipLaunchKernelGGL(ilqr_accept_kernel, dim3(B), dim3(64), 0, s, p);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

int run_ilqr_search(Handle* h, RolloutArgs& a, int iterations, int L, double reg0, double reg_factor, double reg_max, double tol,
                    const double* x0_dev, double* st, double* best_out_dev, hipStream_t s) {
    const int B = a.B, H = a.H, A = a.A;
    const IlqrLayout Y = make_ilqr_layout(B, H, A, h->D, L);
    int rc = run_ilqr_init(h, x0_dev, B, H, A, L, reg0, st, s);
    if (rc) return rc;
    for (int it = 0; it < iterations; ++it) {
        rc = run_ilqr_step(h, a.mu0, B, H, A, a.include_time, a.time0, L, reg0, reg_factor, reg_max, tol, st, s);
        if (rc) return rc;
    }
    // the library's LCB objective of the final sequences: gpmpc_rollout_linear's launches, J only
    rollout_objective_only(a, st + Y.actions, st + Y.J);
    rc = run_rollout_linear(h, a, s);
    if (rc) return rc;
    if (best_out_dev) return launch_argmin_to(h, st + Y.J, B, 0, st + Y.actions, H * A, best_out_dev, nullptr, s);
    return GPMPC_OK;
}

}  // namespace gpmpc_hip
