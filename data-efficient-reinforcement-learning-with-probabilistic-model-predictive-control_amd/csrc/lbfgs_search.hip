// lbfgs_search.hip -- device-resident gradient search (include/gpmpc.h: gpmpc_lbfgs_init / _step / _search).
//
// A box-constrained (projected) L-BFGS over [0, 1]^(H A) for B restarts in lockstep.  Every iteration evaluates exactly one trial
// point per restart -- the line search is spread over iterations -- so the launch sequence
//     objective + gradient of the B trial sequences      the hot path (gpmpc_rollout_grad's launches, or the linearised pair)
//     lbfgs_step_kernel                                   chain rule, accept / reject, pair ring, two-loop recursion, next trial point
// never depends on data and is enqueued back to back on the caller's stream; nothing is read back until the winner.
//
// lbfgs_step_kernel: one wavefront per restart, lanes stride over the n coordinates, every dot product is a lane's serial sum over
// its coordinates followed by wave_sum -- an order fixed by n alone, so a restart's bits depend neither on B nor on its slot.  The
// mapper's sum over the horizon runs on one lane per action dimension (action_mapper.h, shared with search.hip).  No atomics,
// nothing waits for another workgroup.  LDS: gt (n) | q (n) | the recursion's coefficients (history).
#include "device_common.h"
#include "lbfgs_state.h"

namespace gpmpc_hip {

namespace {

struct LbfgsStepArgs {
    const double* J;       // (B)
    const double* G;       // (B, H, A) dJ / d(model actions)
    double* state;
    int B, H, A, m, k;
    double c1, pgtol;
    ActionMapper mp;
};

struct LbfgsInitArgs {
    const double* x0;      // (B, n)
    double* state;
    int B, H, A, m;
    ActionMapper mp;
};

__device__ inline double wave_max(double v) {
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

// optimiser vector (LDS) -> model actions, and the gradient back: one lane per action dimension (action_mapper.h); the identity is
// a plain copy, which all lanes share
__device__ inline void lbfgs_map(int lane, int H, int A, const ActionMapper& mp, const double* xt, double* actions) {
    if (mp.mapper == 0) {
        for (int i = lane; i < H * A; i += kWave) actions[i] = xt[i];
        return;
    }
    for (int a = lane; a < A; a += kWave) map_actions(mp, a, H, A, xt + a, actions + a);
}

__device__ inline void lbfgs_map_backward(int lane, int H, int A, const ActionMapper& mp, const double* G, double* gt) {
    if (mp.mapper == 0) {
        for (int i = lane; i < H * A; i += kWave) gt[i] = G[i];
        return;
    }
    for (int a = lane; a < A; a += kWave) map_actions_backward(mp, a, H, A, G + a, gt + a);
}

__global__ __launch_bounds__(64) void lbfgs_init_kernel(const LbfgsInitArgs p) {
    extern __shared__ double lds[];
    const int b = blockIdx.x, lane = threadIdx.x, n = p.H * p.A, m = p.m;
    const LbfgsLayout L = make_lbfgs_layout(p.B, n, m);
    double* st = p.state;
    const size_t bn = (size_t)b * n;
    for (int i = lane; i < n; i += kWave) {
        const double v = clip01(p.x0[bn + i]);
        st[L.xt + bn + i] = v;
        lds[i] = v;
        st[L.x + bn + i] = 0.0;
        st[L.g + bn + i] = 0.0;
        st[L.d + bn + i] = 0.0;
    }
    for (int i = lane; i < m * n; i += kWave) {
        st[L.S + bn * m + i] = 0.0;
        st[L.Y + bn * m + i] = 0.0;
    }
    for (int j = lane; j < m; j += kWave) {
        st[L.sy + (size_t)b * m + j] = 0.0;
        st[L.yy + (size_t)b * m + j] = 0.0;
    }
    if (lane == 0) {
        st[L.J + b] = 0.0;
        st[L.alpha + b] = 1.0;
        st[L.status + b] = 0.0;
        st[L.pushes + b] = 0.0;
    }
    wave_lds_sync();
    lbfgs_map(lane, p.H, p.A, p.mp, lds, st + L.actions + bn);
}

__global__ __launch_bounds__(64) void lbfgs_step_kernel(const LbfgsStepArgs p) {
    extern __shared__ double lds[];
    const int b = blockIdx.x, lane = threadIdx.x, H = p.H, A = p.A, n = H * A, m = p.m;
    const LbfgsLayout L = make_lbfgs_layout(p.B, n, m);
    double* st = p.state;
    if (st[L.status + b] != 0.0) return;              // (uniform) a finished restart: its state no longer changes
    const size_t bn = (size_t)b * n, bm = (size_t)b * m;
    double* x = st + L.x + bn;
    double* g = st + L.g + bn;
    double* d = st + L.d + bn;
    double* xt = st + L.xt + bn;
    double* S = st + L.S + bn * m;
    double* Y = st + L.Y + bn * m;
    double* sy = st + L.sy + bm;
    double* yy = st + L.yy + bm;
    double* gt = lds;                                 // gradient wrt the optimiser vector; later the new trial point
    double* q = lds + n;
    double* coef = lds + 2 * (size_t)n;

    // 1. chain rule
    lbfgs_map_backward(lane, H, A, p.mp, p.G + bn, gt);
    wave_lds_sync();

    // 2. accept or reject
    const double Jt = p.J[b];
    bool lane_bad = false;
    for (int i = lane; i < n; i += kWave) lane_bad = lane_bad || !finite_d(gt[i]);
    const bool bad = !finite_d(Jt) || __ballot(lane_bad) != 0ull;
    bool accept = true;
    if (p.k > 0) {
        double pgs = 0.0;
        for (int i = lane; i < n; i += kWave) pgs += g[i] * (xt[i] - x[i]);
        const double gs = wave_sum(pgs);
        accept = !bad && Jt <= st[L.J + b] + p.c1 * gs;
    }

    if (!accept) {
        // 4. reject: halve the step along the same direction
        const double alpha = st[L.alpha + b] * 0.5;
        const bool under = alpha < 0x1p-40;
        for (int i = lane; i < n; i += kWave) {
            const double v = under ? x[i] : clip01(x[i] + alpha * d[i]);
            xt[i] = v;
            gt[i] = v;
        }
        if (lane == 0) {
            st[L.alpha + b] = alpha;
            if (under) st[L.status + b] = 2.0;
        }
        wave_lds_sync();
        lbfgs_map(lane, H, A, p.mp, gt, st + L.actions + bn);
        return;
    }

    // 3. accept
    int pushes = (int)st[L.pushes + b];
    if (p.k > 0) {
        double psy = 0.0, pss = 0.0, pyy = 0.0;
        for (int i = lane; i < n; i += kWave) {
            const double s = xt[i] - x[i], y = gt[i] - g[i];
            psy += s * y;
            pss += s * s;
            pyy += y * y;
        }
        const double vsy = wave_sum(psy), vss = wave_sum(pss), vyy = wave_sum(pyy);
        if (vsy > 1e-10 * (sqrt(vss) * sqrt(vyy))) {
            const int slot = pushes % m;
            for (int i = lane; i < n; i += kWave) {
                S[(size_t)slot * n + i] = xt[i] - x[i];
                Y[(size_t)slot * n + i] = gt[i] - g[i];
            }
            sy[slot] = vsy;                          // every lane stores the same value: each reads back its own store below
            yy[slot] = vyy;
            pushes += 1;
        }
    }
    for (int i = lane; i < n; i += kWave) { x[i] = xt[i]; g[i] = gt[i]; }
    if (lane == 0) st[L.J + b] = Jt;
    if (p.k == 0 && bad) {                            // non-finite start: xt = x already
        if (lane == 0) st[L.status + b] = 3.0;
        return;
    }

    // 5. new direction: gradient on the free set
    double pmax = 0.0, pgg = 0.0;
    for (int i = lane; i < n; i += kWave) {
        const double xv = xt[i], gv = gt[i];
        const bool fixed = (xv <= 0.0 && gv > 0.0) || (xv >= 1.0 && gv < 0.0);
        const double gf = fixed ? 0.0 : gv;
        q[i] = gf;
        pmax = fmax(pmax, fabs(gf));
        pgg += gf * gf;
    }
    const double gmax = wave_max(pmax);
    if (gmax <= p.pgtol) {                            // converged: xt = x already
        if (lane == 0) { st[L.status + b] = 1.0; st[L.pushes + b] = (double)pushes; }
        return;
    }
    const double gg = wave_sum(pgg);
    const int held = pushes < m ? pushes : m;
    for (int j = 0; j < held; ++j) {                  // newest -> oldest
        const int slot = (pushes - 1 - j) % m;
        double ps = 0.0;
        for (int i = lane; i < n; i += kWave) ps += S[(size_t)slot * n + i] * q[i];
        const double aj = wave_sum(ps) / sy[slot];
        coef[j] = aj;
        for (int i = lane; i < n; i += kWave) q[i] -= aj * Y[(size_t)slot * n + i];
    }
    const int newest = held > 0 ? (pushes - 1) % m : 0;
    const double gamma = held > 0 ? sy[newest] / yy[newest] : 1.0 / sqrt(gg);
    for (int i = lane; i < n; i += kWave) q[i] *= gamma;
    for (int j = held - 1; j >= 0; --j) {             // oldest -> newest
        const int slot = (pushes - 1 - j) % m;
        double py = 0.0;
        for (int i = lane; i < n; i += kWave) py += Y[(size_t)slot * n + i] * q[i];
        const double bj = wave_sum(py) / sy[slot];
        const double c = coef[j] - bj;
        for (int i = lane; i < n; i += kWave) q[i] += c * S[(size_t)slot * n + i];
    }
    double pdg = 0.0;
    for (int i = lane; i < n; i += kWave) {
        const double xv = xt[i], gv = gt[i];
        const bool fixed = (xv <= 0.0 && gv > 0.0) || (xv >= 1.0 && gv < 0.0);
        const double dv = fixed ? 0.0 : -q[i];
        q[i] = dv;
        pdg += dv * (fixed ? 0.0 : gv);
    }
    const double dg = wave_sum(pdg);
    const bool reset = !(dg < 0.0);                   // no descent (or NaN): steepest descent, the pairs are dropped
    if (reset) pushes = 0;
    for (int i = lane; i < n; i += kWave) {
        const double xv = xt[i], gv = gt[i];
        const bool fixed = (xv <= 0.0 && gv > 0.0) || (xv >= 1.0 && gv < 0.0);
        const double dv = reset ? (fixed ? 0.0 : -gv) : q[i];
        d[i] = dv;
        const double v = clip01(xv + dv);
        xt[i] = v;
        q[i] = v;
    }
    if (lane == 0) { st[L.alpha + b] = 1.0; st[L.pushes + b] = (double)pushes; }
    wave_lds_sync();
    lbfgs_map(lane, H, A, p.mp, q, st + L.actions + bn);
}

__global__ __launch_bounds__(256) void lbfgs_ones_kernel(double* v, int B) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < B) v[i] = 1.0;
}

size_t step_lds_bytes(int n, int m) { return (2 * (size_t)n + m) * sizeof(double); }

int launch_step(Handle* h, const LbfgsStepArgs& p, hipStream_t s) {
    int rc = allow_full_lds(h, reinterpret_cast<const void*>(lbfgs_step_kernel));
    if (rc) return rc;
    hipLaunchKernelGGL(lbfgs_step_kernel, dim3(p.B), dim3(64), step_lds_bytes(p.H * p.A, p.m), s, p);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

}  // namespace

int run_lbfgs_init(Handle* h, const double* x0_dev, int B, int H, int A, int history, const ActionMapper& mp, double* state_dev,
                   hipStream_t s) {
    LbfgsInitArgs p;
    p.x0 = x0_dev; p.state = state_dev; p.B = B; p.H = H; p.A = A; p.m = history; p.mp = mp;
    hipLaunchKernelGGL(lbfgs_init_kernel, dim3(B), dim3(64), (size_t)H * A * sizeof(double), s, p);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

int run_lbfgs_step(Handle* h, const double* J_dev, const double* grad_model_dev, int B, int H, int A, int iteration, int history,
                   double c1, double pgtol, const ActionMapper& mp, double* state_dev, hipStream_t s) {
    LbfgsStepArgs p;
    p.J = J_dev; p.G = grad_model_dev; p.state = state_dev; p.B = B; p.H = H; p.A = A; p.m = history; p.k = iteration;
    p.c1 = c1; p.pgtol = pgtol; p.mp = mp;
    return launch_step(h, p, s);
}

int run_lbfgs_search(Handle* h, RolloutArgs& a, int propagation, int first_iteration, int iterations, int history, double c1,
                     double pgtol, const ActionMapper& mp, const double* x0_dev, double* state_dev, double* best_out_dev,
                     hipStream_t s) {
    const int B = a.B, H = a.H, A = a.A, n = H * A;
    // the gradient launch is planned first: a shape outside its kernels is reported before anything is enqueued or written
    int rc;
    if (propagation == 0) {
        if (a.D > 8) rc = check_rollout_grad_wide(h, a.N, a.D, A, a.E, H, B);
        else {
            rc = ensure_rollout_tables(h, a.N, a.D);
            if (rc) return rc;
            GradPlan gp;
            rc = plan_rollout_grad(h, a.N, a.D, A, a.E, H, B, B, false, gp);
        }
        if (rc) return rc;
    }
    // (propagation 1 has nothing to plan: run_rollout_linear and run_rollout_linear_backward take every shape of a cached model and
    // return allocation and HIP errors only.  Should they ever gain a capability limit, it has to be asked for HERE, before the
    // init below writes the caller's state.)
    // workspace: J (B) | dJ/d(model actions) (B n) | ones (B)
    rc = grow(h, h->lbfgsws, 2 * (size_t)B + (size_t)B * n);
    if (rc) return rc;
    double* J = h->lbfgsws.p;
    double* G = J + B;
    double* ones = G + (size_t)B * n;
    const LbfgsLayout L = make_lbfgs_layout(B, n, history);
    if (first_iteration == 0) {
        rc = run_lbfgs_init(h, x0_dev, B, H, A, history, mp, state_dev, s);
        if (rc) return rc;
    }
    if (propagation == 1) {
        hipLaunchKernelGGL(lbfgs_ones_kernel, dim3((B + 255) / 256), dim3(256), 0, s, ones, B);
        GPMPC_HIP_CHECK(h, hipGetLastError());
    }
    rollout_objective_only(a, state_dev + L.actions, J);
    for (int it = 0; it < iterations; ++it) {
        RolloutArgs ai = a;
        if (propagation == 0) {
            rc = launch_rollout_grad(h, ai, G, s);
        } else {
            rc = run_rollout_linear(h, ai, s);
            if (rc) return rc;
            const RolloutSeeds sd{nullptr, nullptr, nullptr, nullptr, ones, nullptr, nullptr, true};
            rc = run_rollout_linear_backward(h, ai, sd, G, s);
        }
        if (rc) return rc;
        rc = run_lbfgs_step(h, J, G, B, H, A, first_iteration + it, history, c1, pgtol, mp, state_dev, s);
        if (rc) return rc;
    }
    if (best_out_dev) return launch_argmin_to(h, state_dev + L.J, B, 0, state_dev + L.x, n, best_out_dev, nullptr, s);
    return GPMPC_OK;
}

}  // namespace gpmpc_hip
