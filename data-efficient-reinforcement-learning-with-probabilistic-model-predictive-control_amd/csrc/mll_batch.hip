// mll_batch.hip -- the batched training loss (include/gpmpc.h: gpmpc_mll_batch) and the multi-restart hyper-parameter search built
// on it (gpmpc_train_search).
//
// Problem p = r D + a is restart r of GP a: loss = -log p(y_a | X, theta_p) / N and its gradient, the definition of gpmpc_mll
// (prepare.hip: mll_finish_kernel).  One workgroup of 1024 threads owns one problem from the box map to the gradient; R D problems
// fill the chip where one gpmpc_mll evaluation is D workgroups.  Phases, each handed to the next by a workgroup barrier:
//   P0  theta = box map of the parameter row (LDS), inputs scaled by 1 / l
//   P1-P4  Gram matrix, blocked Cholesky, L^-1, beta: the functions of small_factor.h, the ones prepare_small_kernel runs
//   P5  iK = Y^T Y, lower triangle
//   P6  contraction: sum over i >= j of (beta_i beta_j - iK_ij) K'_ij {d2_ije, 1} (K' = K without the noise, recomputed from the
//       scaled inputs in LDS; off-diagonal terms count twice), 8 input dimensions per pass; log det, y.beta and the trace term
//       from the diagonal; chain rule of the box map; the results
// No T table, no packed inputs: three N x N matrices per problem (L in place of K) in a workspace the handle owns for `chunk`
// problems at a time.  Every sum is a lane's serial sum in an order fixed by N and E, a wavefront butterfly, then the 16 wavefront
// totals in order: no atomics, so a problem's bits depend neither on R, nor on its position, nor on the chunk.
// A matrix that is not positive definite is a RESULT: the first pivot that is not positive and finite is remembered in LDS, the
// workgroup runs to its end all the same (no loop bound and no barrier depends on the data) and then writes loss = +inf,
// gradient = 0, info = the order of the failing leading minor.
#include "small_factor.h"
#include "lbfgs_state.h"

namespace gpmpc_hip {

namespace {

// theta of the optimiser coordinate x in [0, 1]: lo + (hi - lo) x, or lo (hi / lo)^x; `chain` = d theta / d x
__device__ inline double box_map(double x, double lo, double hi, int log_scale, double& chain) {
    if (log_scale) {
        const double ratio = hi / lo;
        const double v = lo * pow(ratio, x);
        chain = v * log(ratio);
        return v;
    }
    chain = hi - lo;
    return fma(hi - lo, x, lo);
}

struct MllBatchArgs {
    const double *X, *Y;       // (N, E), (N, D)
    const double* params;      // (P, n) theta, or x in [0, 1]^n with a box
    const double *lo, *hi;     // (D, n), or both NULL
    int N, D, E, log_scale;
    int first;                 // first problem of this launch (blockIdx.x = its workspace slot)
    double* ws;                // per slot: K -> L (N, N) | L^-1 (N, N) | iK (N, N) | z (N) | beta (N)
    double *loss, *grad, *theta;
    int* info;
};

constexpr int kMllDimsPerPass = 8;
constexpr int kMllRedStride = kMllDimsPerPass + 1;
// LDS after the factorisation's arrays: theta (32) | d theta / d x (32) | the pivot flag
constexpr size_t kMllLdsExtra = 32 + 32 + 2;
// ... and inside them once the factorisation is done: scaled inputs padded to whole passes (N, 8 ceil(E / 8) + 1) | wavefront
// totals (16, 9) | sums (25) | diagonal totals (16, 3)
constexpr size_t kMllXsMax = (size_t)kSmallMaxN * (GPMPC_MAX_E + 1);
static_assert(GPMPC_MAX_E % kMllDimsPerPass == 0, "the padded row of the contraction holds whole passes");
static_assert(GPMPC_MAX_E + 2 <= 32, "theta and its chain factors have 32 LDS slots each");
static_assert(kMllXsMax + 16 * kMllRedStride + 32 + 16 * 3 <= kSmallLdsP2, "the contraction's arrays reuse the factorisation's LDS");

__global__ __launch_bounds__(1024) void mll_batch_kernel(const MllBatchArgs p) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int slot = blockIdx.x, prob = p.first + slot, a = prob % p.D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = p.N, D = p.D, E = p.E, n = E + 2;
    const SmallLds lds = small_lds(sm);
    double* th = sm + small_lds_doubles(N, E);
    double* ch = th + 32;
    int* flag = reinterpret_cast<int*>(ch + 32);
    double* K = p.ws + (size_t)slot * (3 * (size_t)N * N + 2 * (size_t)N);
    double* Yv = K + (size_t)N * N;
    double* iK = Yv + (size_t)N * N;
    double* zv = iK + (size_t)N * N;
    double* be = zv + N;
    const double* ycol = p.Y + a;
    SmallCholProf prof;

    // ---- P0: theta, scaled inputs ------------------------------------------------------------------------------------------
    if (tid < n) {
        double v = p.params[(size_t)prob * n + tid], c = 1.0;
        if (p.lo) v = box_map(v, p.lo[a * n + tid], p.hi[a * n + tid], p.log_scale, c);
        th[tid] = v;
        ch[tid] = c;
        if (p.theta) p.theta[(size_t)prob * n + tid] = v;
    }
    if (tid == 0) *flag = 0;
    __syncthreads();
    const double va = th[E], nz = th[E + 1];
    small_scale_inputs(p.X, th, N, E, lds.xs, tid);
    __syncthreads();

    // ---- P1 - P4 -----------------------------------------------------------------------------------------------------------------
    small_gram(lds.xs, va, nz, N, E, K, Yv, tid);
    __syncthreads();
    // (loads of 4 k-steps in flight in the panel update and in L^-1 where prepare_small_kernel has 8 and 16: the loss's extra
    // live values then fit the 128 registers of a 1024-thread workgroup without scratch; the sums keep their order)
    small_cholesky<4>(K, Yv, N, lds, [&](double pivot, int order) {
        if (!(pivot > 0.0 && pivot <= 1.7976931348623157e308) && *flag == 0) *flag = order;
    }, tid, prof);
    small_trinv<4>(K, Yv, iK, N, tid);                       // (scratch in iK, which P5 overwrites)
    small_beta(Yv, ycol, D, N, zv, be, tid);

    // ---- P5: iK = Y^T Y, lower triangle --------------------------------------------------------------------------------------
    small_syrk_lower<8>(Yv, N, tid, [&](int row, int col, double v) { iK[(size_t)row * N + col] = v; });

    // ---- P6: contraction ---------------------------------------------------------------------------------------------------------
    const int npass = (E + kMllDimsPerPass - 1) / kMllDimsPerPass;
    const int ESP = npass * kMllDimsPerPass + 1;             // odd row stride: conflict-free column reads
    double* xs = sm;
    double* red = sm + kMllXsMax;                            // (16, 9)
    double* sums = red + 16 * kMllRedStride;                 // S_e (E) at [e], sum of the weights at [24]
    double* dred = sums + 32;                                // (16, 3)
    for (int idx = tid; idx < N * ESP; idx += 1024) {
        const int pt = idx / ESP, e = idx - pt * ESP;
        double v = 0.0;
        if (e < E) { const double l = th[e]; v = p.X[(size_t)pt * E + e] * sqrt(1.0 / (l * l)); }
        xs[idx] = v;
    }
    {
        __syncthreads();                                     // iK and the scaled inputs are complete
        // the diagonal: y.beta, log det L, tr(beta beta^T - iK)
        double yb = 0.0, ld = 0.0, tq = 0.0;
        if (tid < N) {
            const double b = be[tid];
            yb = ycol[(size_t)tid * D] * b;
            ld = log(K[(size_t)tid * N + tid]);
            tq = b * b - iK[(size_t)tid * N + tid];
        }
        yb = wave_xor_sum(yb); ld = wave_xor_sum(ld); tq = wave_xor_sum(tq);
        if (lane == 0) { dred[wave * 3] = yb; dred[wave * 3 + 1] = ld; dred[wave * 3 + 2] = tq; }
    }
    for (int c = 0; c < npass; ++c) {
        double acc[kMllRedStride];
#pragma unroll
        for (int u = 0; u < kMllRedStride; ++u) acc[u] = 0.0;
        // row N - 1 - f and row f together are N + 1 entries of the lower triangle: every folded row is the same work
        for (int f = wave; f < (N + 1) / 2; f += 16) {
            const int ia = N - 1 - f, ib = f;
            const int la = ia + 1, lb = (ib != ia) ? ib + 1 : 0;
            for (int cc = lane; cc < la + lb; cc += 64) {
                const int row = cc < la ? ia : ib, col = cc < la ? cc : cc - la;
                const double* xr = xs + row * ESP;
                const double* xc = xs + col * ESP;
                double s = 0.0;
                for (int e = 0; e < E; ++e) { const double d = xr[e] - xc[e]; s = fma(d, d, s); }
                const double q = be[row] * be[col] - iK[(size_t)row * N + col];
                double w = q * (va * exp(-0.5 * s));
                if (row != col) w *= 2.0;
#pragma unroll
                for (int u = 0; u < kMllDimsPerPass; ++u) {
                    const double d = xr[c * kMllDimsPerPass + u] - xc[c * kMllDimsPerPass + u];
                    acc[u] = fma(w, d * d, acc[u]);
                }
                acc[kMllDimsPerPass] += w;
            }
        }
#pragma unroll
        for (int u = 0; u < kMllRedStride; ++u) {
            const double v = wave_xor_sum(acc[u]);
            if (lane == 0) red[wave * kMllRedStride + u] = v;
        }
        __syncthreads();
        if (tid < kMllRedStride) {
            double v = 0.0;
            for (int w = 0; w < 16; ++w) v += red[w * kMllRedStride + tid];
            if (tid < kMllDimsPerPass) sums[c * kMllDimsPerPass + tid] = v;
            else if (c == 0) sums[24] = v;
        }
        __syncthreads();
    }

    // ---- results ---------------------------------------------------------------------------------------------------------------
    const int lost = *flag;
    const double invn = 1.0 / (double)N;
    if (tid < n) {
        double g;
        if (tid < E) g = -0.5 * invn * sums[tid] / th[tid];                  // S_e / l_e
        else if (tid == E) g = -0.5 * invn * sums[24] / va;
        else {
            double tqs = 0.0;
            for (int w = 0; w < 16; ++w) tqs += dred[w * 3 + 2];
            g = -0.5 * invn * tqs;
        }
        p.grad[(size_t)prob * n + tid] = lost ? 0.0 : g * ch[tid];
    }
    if (tid == 0) {
        double ybs = 0.0, lds_ = 0.0;
        for (int w = 0; w < 16; ++w) { ybs += dred[w * 3]; lds_ += dred[w * 3 + 1]; }
        p.loss[prob] = lost ? INFINITY : (0.5 * ybs + lds_ + 0.5 * N * 1.8378770664093453) * invn;      // log(2 pi)
        if (p.info) p.info[prob] = lost;
    }
}

// best_out[a] = [loss | restart | status | theta (n)] of the best restart of GP a that did not start non-finite (status 3): the
// lowest J, ties to the lowest restart; [+inf | -1 | 3 | theta of restart 0's x] where there is none.  One wavefront per GP.
struct TrainBestArgs {
    const double* state;
    const double *lo, *hi;
    int R, D, n, m, log_scale;
    double* out;
};

__global__ __launch_bounds__(64) void train_best_kernel(const TrainBestArgs p) {
    const int a = blockIdx.x, lane = threadIdx.x, D = p.D, n = p.n;
    const LbfgsLayout L = make_lbfgs_layout(p.R * D, n, p.m);
    const double* J = p.state + L.J;
    const double* status = p.state + L.status;
    constexpr int kNone = 0x7fffffff;
    double bj = INFINITY;
    int br = kNone;
    for (int r = lane; r < p.R; r += kWave) {
        const double v = J[r * D + a];
        if (status[r * D + a] != 3.0 && (v < bj || (v == bj && r < br))) { bj = v; br = r; }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const double oj = __shfl_xor(bj, off, 64);
        const int orr = __shfl_xor(br, off, 64);
        if (oj < bj || (oj == bj && orr < br)) { bj = oj; br = orr; }
    }
    const bool none = br == kNone;
    const int src = none ? 0 : br;
    double* o = p.out + (size_t)a * (3 + n);
    if (lane == 0) {
        o[0] = none ? INFINITY : bj;
        o[1] = none ? -1.0 : (double)br;
        o[2] = none ? 3.0 : status[br * D + a];
    }
    for (int k = lane; k < n; k += kWave) {
        double c;
        o[3 + k] = box_map(p.state[L.x + (size_t)(src * D + a) * n + k], p.lo[a * n + k], p.hi[a * n + k], p.log_scale, c);
    }
}

}  // namespace

int run_mll_batch(Handle* h, const double* X, const double* Y, int N, int D, int E, const double* params, int R, const double* lo,
                  const double* hi, int log_scale, double* loss_out, double* grad_out, double* theta_out, int* info_out,
                  hipStream_t s) {
    static_assert(kSmallLdsP2 >= (size_t)kSmallMaxN * (GPMPC_MAX_E | 1), "the scaled inputs of N <= 256 points fit the panel's LDS");
    const int P = R * D;
    const int chunk = h->opt_mll_batch_chunk > 0 ? h->opt_mll_batch_chunk : h->num_cu;
    const int slots = chunk < P ? chunk : P;
    const size_t per = 3 * (size_t)N * N + 2 * (size_t)N;
    int rc = grow(h, h->mllbws, (size_t)slots * per);
    if (rc) return rc;
    rc = allow_full_lds(h, reinterpret_cast<const void*>(mll_batch_kernel));
    if (rc) return rc;
    MllBatchArgs p;
    p.X = X; p.Y = Y; p.params = params; p.lo = lo; p.hi = hi;
    p.N = N; p.D = D; p.E = E; p.log_scale = log_scale;
    p.ws = h->mllbws.p;
    p.loss = loss_out; p.grad = grad_out; p.theta = theta_out; p.info = info_out;
    const size_t lds = (small_lds_doubles(N, E) + kMllLdsExtra) * sizeof(double);
    for (int first = 0; first < P; first += slots) {
        p.first = first;
        const int cnt = P - first < slots ? P - first : slots;
        hipLaunchKernelGGL(mll_batch_kernel, dim3(cnt), dim3(1024), lds, s, p);
    }
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

int run_train_search(Handle* h, const double* X, const double* Y, int N, int D, int E, int R, const double* lo, const double* hi,
                     int log_scale, int first_iteration, int iterations, int history, double c1, double pgtol, const double* x0_dev,
                     double* state_dev, double* best_out_dev, hipStream_t s) {
    const int P = R * D, n = E + 2;
    // workspace: loss (P) | d loss / d x (P, n)
    int rc = grow(h, h->trainws, (size_t)P * (1 + n));
    if (rc) return rc;
    double* J = h->trainws.p;
    double* G = J + P;
    ActionMapper mp;
    mp.mapper = 0;
    const LbfgsLayout L = make_lbfgs_layout(P, n, history);
    if (first_iteration == 0) {
        rc = run_lbfgs_init(h, x0_dev, P, 1, n, history, mp, state_dev, s);
        if (rc) return rc;
    }
    for (int it = 0; it < iterations; ++it) {
        rc = run_mll_batch(h, X, Y, N, D, E, state_dev + L.actions, R, lo, hi, log_scale, J, G, nullptr, nullptr, s);
        if (rc) return rc;
        rc = run_lbfgs_step(h, J, G, P, 1, n, first_iteration + it, history, c1, pgtol, mp, state_dev, s);
        if (rc) return rc;
    }
    if (best_out_dev) {
        TrainBestArgs b;
        b.state = state_dev; b.lo = lo; b.hi = hi; b.R = R; b.D = D; b.n = n; b.m = history; b.log_scale = log_scale;
        b.out = best_out_dev;
        hipLaunchKernelGGL(train_best_kernel, dim3(D), dim3(64), 0, s, b);
        GPMPC_HIP_CHECK(h, hipGetLastError());
    }
    return GPMPC_OK;
}

}  // namespace gpmpc_hip
