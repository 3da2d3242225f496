// search.hip -- device-resident candidate optimisation.
//
// The reference optimises the action sequence with `restarts_optim` sequential scipy L-BFGS-B solves, every
// evaluation one Python call of compute_mean_lcb_trajectory (gp_mpc_controller.py:125-141).  gpmpc_cem_search is a
// cross-entropy search over the same box [0, 1]^(H A) whose whole loop stays on the GPU: per iteration
//     cem_sample_kernel   B optimiser vectors around the current mean / std (iteration 0: uniform; slot 0 = the incumbent,
//                         or the caller's warm start), counter-based Philox draws (or draws supplied by the caller)
//     cem_map_kernel      the action mapper (action_mapper.h, its parameters in the kernel argument block) -> model
//                         actions (B, H, A)
//     rollout launch      the hot path: objective of the B sequences
//     cem_refit_kernel    one workgroup: NaN -> +inf, bitonic sort of (J, index) (ties by index = numpy's stable
//                         argsort), incumbent update, mean / population std (+ 1e-3) of the elites per coordinate
// are enqueued back to back on the caller's stream; nothing is read back between iterations.  The caller synchronises
// once, for the best vector and its objective.
//
// Candidates sharded over GPUs take the same steps in two halves: run_cem_local = the population step of a slice +
// cem_elites_kernel (the slice's leaders as records), run_cem_merge = cem_merge_kernel on the gathered records.  The three
// single-workgroup kernels share ONE sort (cem_sort), ONE key load (cem_load_keys) and ONE refit (cem_refit: the incumbent rule
// and the elite statistics, over a row accessor), and both drivers ONE population step (cem_population_step): so every GPU
// reaches, bit for bit, the state the single-GPU search reaches on the same draws.
#include "action_mapper.h"
#include "device_common.h"

namespace gpmpc_hip {

namespace {

constexpr int kCemMaxB = 4096;
static_assert(kMaxE <= kMaxMapperA, "a cached model's A < E <= kMaxE: the mapper's parameters fit the argument block");

__device__ inline void philox_round(unsigned& c0, unsigned& c1, unsigned& c2, unsigned& c3, unsigned k0, unsigned k1) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}

// Philox4x32-10: two uniform doubles in (0, 1] from (counter, key).  x = 2^53 - 1 gives exactly 1.0 ((double)x + 0.5 rounds to
// 2^53), which is harmless: log(1) = 0 and 1.0 lies inside the box; x = 0 gives 2^-54, so the logarithm is always finite.
__device__ inline void philox_uniform2(unsigned long long seed, unsigned a, unsigned b, unsigned c, double& u0, double& u1) {
    unsigned c0 = a, c1 = b, c2 = c, c3 = 0x9E3779B9u;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    const unsigned long long x0 = ((unsigned long long)c0 << 21) ^ (unsigned long long)(c1 >> 11);      // 53 bits
    const unsigned long long x1 = ((unsigned long long)c2 << 21) ^ (unsigned long long)(c3 >> 11);
    u0 = ((double)(x0 & ((1ull << 53) - 1)) + 0.5) * (1.0 / 9007199254740992.0);
    u1 = ((double)(x1 & ((1ull << 53) - 1)) + 0.5) * (1.0 / 9007199254740992.0);
}

// one thread per (candidate, coordinate): optimiser vectors of this iteration
// (`b0`, `B_total`: this launch draws candidates [b0, b0 + B) of a population of B_total -- the counters and the caller's
// noise are indexed by the GLOBAL candidate, so the union of the slices of several GPUs is the single-GPU population)
__global__ __launch_bounds__(256) void cem_sample_kernel(int it, int B, int n, unsigned long long seed, const double* __restrict__ noise,
                                                         const double* __restrict__ mean, const double* __restrict__ stdv,
                                                         const double* __restrict__ best, int have_first,
                                                         const double* __restrict__ first, double* __restrict__ X, int b0, int B_total) {
    const int lidx = blockIdx.x * 256 + threadIdx.x;
    if (lidx >= B * n) return;
    const int b = lidx / n + b0, k = lidx - (lidx / n) * n;
    const int idx = b * n + k;
    double v;
    if (b == 0 && it > 0) v = best[k];                             // keep the incumbent
    else if (b == 0 && have_first) v = first[k];                   // warm start (previous solution shifted by one step)
    else {
        double draw;
        if (noise) draw = noise[(size_t)it * B_total * n + idx];
        else {
            double u0, u1;
            philox_uniform2(seed, (unsigned)idx, (unsigned)it, 0x243F6A88u, u0, u1);
            draw = (it == 0) ? u0 : sqrt(-2.0 * log(u0)) * cos(6.283185307179586 * u1);
        }
        v = (it == 0) ? draw : clip01(fma(stdv[k], draw, mean[k]));
    }
    X[lidx] = v;
}

// one thread per (candidate, action dimension): optimiser vector -> model actions
__global__ __launch_bounds__(256) void cem_map_kernel(int B, int H, int A, const ActionMapper mp, const double* __restrict__ X,
                                                      double* __restrict__ actions) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * A) return;
    const int b = idx / A, a = idx - b * A;
    map_actions(mp, a, H, A, X + (size_t)b * H * A + a, actions + (size_t)b * H * A + a);
}

// ---- the single-workgroup kernels (1024 threads): key load, sort, refit ----------------------------------------------------------
__device__ inline int pow2_at_least(int n) {
    int P2 = 1;
    while (P2 < n) P2 <<= 1;
    return P2;
}

// (J with NaN -> +inf, index) of the B candidates into LDS, padded with (+inf, INT_MAX) to the power of two it returns
__device__ inline int cem_load_keys(const double* __restrict__ J, int B, double* key, int* val, int tid) {
    const int P2 = pow2_at_least(B);
    for (int i = tid; i < P2; i += 1024) {
        double v = (i < B) ? J[i] : INFINITY;
        if (v != v) v = INFINITY;
        key[i] = v;
        val[i] = (i < B) ? i : 0x7fffffff;
    }
    __syncthreads();
    return P2;
}

// in-LDS bitonic sort of (key, val), ascending, ties by val; P2 = power of two >= the number of entries
__device__ inline void cem_sort(double* key, int* val, int P2, int tid) {
    for (int size = 2; size <= P2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < P2 / 2; i += 1024) {
                const int lo = 2 * i - (i & (stride - 1));              // index with bit `stride` clear
                const int hi = lo + stride;
                const bool up = ((lo & size) == 0);
                const double klo = key[lo], khi = key[hi];
                const int vlo = val[lo], vhi = val[hi];
                const bool gt = (klo > khi) || (klo == khi && vlo > vhi);
                if (gt == up) { key[lo] = khi; key[hi] = klo; val[lo] = vhi; val[hi] = vlo; }
            }
            __syncthreads();
        }
    }
}

// Incumbent rule and elite statistics: row(e) = the optimiser vector (n) of the e-th leader, lead_J the objective of leader 0.
// Both sums run over e = 0 .. n_elite - 1.  best = x (n) | J.
template <typename Row>
__device__ inline void cem_refit(int n, int n_elite, double lead_J, Row row, double* __restrict__ mean, double* __restrict__ stdv,
                                 double* __restrict__ best, int first_iteration, int tid) {
    const double bestJ_old = first_iteration ? INFINITY : best[n];
    // the first iteration always adopts its leader (even when every objective is non-finite): `best` is then never read
    // uninitialised by the sampler of the next iteration
    const bool improve = first_iteration || lead_J < bestJ_old;
    __syncthreads();                                       // every thread has read best[n] before thread 0 replaces it
    for (int k = tid; k < n; k += 1024) {
        double s = 0.0;
        for (int e = 0; e < n_elite; ++e) s += row(e)[k];
        const double m = s / (double)n_elite;
        double q = 0.0;
        for (int e = 0; e < n_elite; ++e) { const double d = row(e)[k] - m; q = fma(d, d, q); }
        mean[k] = m;
        stdv[k] = sqrt(q / (double)n_elite) + 1e-3;
        if (improve) best[k] = row(0)[k];
    }
    if (tid == 0) best[n] = improve ? lead_J : bestJ_old;
}

// the whole population on one GPU: an elite's row is its candidate's optimiser vector
__global__ __launch_bounds__(1024) void cem_refit_kernel(int B, int n, int n_elite, const double* __restrict__ J,
                                                         const double* __restrict__ X, double* __restrict__ mean,
                                                         double* __restrict__ stdv, double* __restrict__ best /* n + 1: x | J */,
                                                         int first_iteration) {
    __shared__ double key[kCemMaxB];
    __shared__ int val[kCemMaxB];
    const int tid = threadIdx.x;
    cem_sort(key, val, cem_load_keys(J, B, key, val, tid), tid);
    cem_refit(n, n_elite, key[0], [&](int e) { return X + (size_t)val[e] * n; }, mean, stdv, best, first_iteration, tid);
}

// Candidates sharded over GPUs: the n_elite best of THIS slice as records [J (NaN -> +inf) | global index | optimiser vector (n)],
// sorted like numpy's stable argsort; a slice shorter than n_elite pads with (+inf, INT_MAX, 0 ...) records, which sort behind
// every real candidate.
__global__ __launch_bounds__(1024) void cem_elites_kernel(int B, int n, int n_elite, int b0, const double* __restrict__ J,
                                                          const double* __restrict__ X, double* __restrict__ rec) {
    __shared__ double key[kCemMaxB];
    __shared__ int val[kCemMaxB];
    const int tid = threadIdx.x;
    cem_sort(key, val, cem_load_keys(J, B, key, val, tid), tid);
    const int RS = n + 2;
    for (int i = tid; i < n_elite * RS; i += 1024) {
        const int e = i / RS, c = i - e * RS;
        const bool real = e < B;
        double v;
        if (c == 0) v = real ? key[e] : INFINITY;
        else if (c == 1) v = real ? (double)(val[e] + b0) : 2147483647.0;
        else v = real ? X[(size_t)val[e] * n + (c - 2)] : 0.0;
        rec[i] = v;
    }
}

// ... and the refit on the union of the slices' elite records (R = lists x n_elite of them, gathered over RCCL): an elite's row
// is its record's vector.  state = mean (n) | std (n) | best (n) | best J.
__global__ __launch_bounds__(1024) void cem_merge_kernel(int R, int n, int n_elite, const double* __restrict__ rec,
                                                         double* __restrict__ state, int first_iteration) {
    __shared__ double key[kCemMaxB];
    __shared__ int val[kCemMaxB];          // global candidate index (the sort's tie-break)
    __shared__ int slot[kCemMaxB];         // record slot of each of the n_elite leaders
    const int tid = threadIdx.x;
    const int RS = n + 2;
    const int P2 = pow2_at_least(R);
    for (int i = tid; i < P2; i += 1024) {
        key[i] = (i < R) ? rec[(size_t)i * RS] : INFINITY;
        val[i] = (i < R) ? (int)rec[(size_t)i * RS + 1] : 0x7fffffff;
    }
    __syncthreads();
    cem_sort(key, val, P2, tid);
    // global indices are unique among real records
    for (int e = tid; e < n_elite; e += 1024) {
        int r0 = 0;
        for (int r = 0; r < R; ++r) if ((int)rec[(size_t)r * RS + 1] == val[e]) { r0 = r; break; }
        slot[e] = r0;
    }
    __syncthreads();
    cem_refit(n, n_elite, key[0], [&](int e) { return rec + (size_t)slot[e] * RS + 2; }, state, state + n, state + 2 * n,
              first_iteration, tid);
}

// workspace of a population step: X (B n) | model actions (B n) | J (B) | warm start (n) | mean (n) | std (n), the last two being
// run_cem_search's own (the sharded search keeps them in the caller's state)
struct CemWork {
    double *X, *acts, *J, *first, *mean, *stdv;
};

// One population step for the candidates [b0, b0 + a.B) of B_total, a.B >= 1: checks the mapper's arguments, carves the workspace
// (`w`), uploads the warm start where it is slot 0's, draws around (mean, stdv, best) -- which iteration 0 does not read --, maps
// and rolls out: w.X and w.J then hold the slice's optimiser vectors and objectives.
int cem_population_step(Handle* h, RolloutArgs& a, int B_total, int b0, int it, unsigned long long seed, const double* first_host,
                        int mapper, const double* max_change_host, const double* a_prev_host, const double* noise_dev,
                        const double* mean, const double* stdv, const double* best, CemWork& w, hipStream_t s) {
    const int B = a.B, H = a.H, A = a.A, n = H * A;
    ActionMapper mp{};
    if (mapper != 0) {                   // (any value but 0 is the derivative mapper)
        if (!max_change_host || !a_prev_host) { h->err = "cem: the derivative mapper needs max_change and the previous action"; return GPMPC_ERR_ARG; }
        mp.mapper = 1;
        for (int i = 0; i < A; ++i) { mp.max_change[i] = max_change_host[i]; mp.action_prev[i] = a_prev_host[i]; }
    }
    int rc = grow(h, h->cemws, 2 * (size_t)B * n + B + 3 * (size_t)n);
    if (rc) return rc;
    w.X = h->cemws.p;
    w.acts = w.X + (size_t)B * n;
    w.J = w.acts + (size_t)B * n;
    w.first = w.J + B;
    w.mean = w.first + n;
    w.stdv = w.mean + n;
    const bool use_first = first_host && it == 0 && b0 == 0;
    if (use_first) GPMPC_HIP_CHECK(h, hipMemcpyAsync(w.first, first_host, n * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(cem_sample_kernel, dim3((B * n + 255) / 256), dim3(256), 0, s, it, B, n, seed, noise_dev, mean, stdv, best,
                       use_first ? 1 : 0, w.first, w.X, b0, B_total);
    hipLaunchKernelGGL(cem_map_kernel, dim3((B * A + 255) / 256), dim3(256), 0, s, B, H, A, mp, w.X, w.acts);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    rollout_objective_only(a, w.acts, w.J);
    RolloutArgs ai = a;
    ai.B_plan = B_total;                 // every slice takes the form (and so the summation order) of the whole population
    return launch_rollout(h, ai, s);
}

}  // namespace

int run_cem_search(Handle* h, RolloutArgs& a, int iterations, int n_elite, unsigned long long seed, const double* first_host,
                   int mapper, const double* max_change_host, const double* a_prev_host, const double* noise_dev,
                   double* best_out_dev, hipStream_t s) {
    const int B = a.B, n = a.H * a.A;
    if (B < 2 || B > kCemMaxB || iterations < 1 || n_elite < 1 || n_elite > B) { h->err = "cem: need 2 <= B <= 4096, 1 <= n_elite <= B"; return GPMPC_ERR_ARG; }
    CemWork w{};
    for (int it = 0; it < iterations; ++it) {
        int rc = cem_population_step(h, a, B, 0, it, seed, first_host, mapper, max_change_host, a_prev_host, noise_dev, w.mean, w.stdv,
                                     best_out_dev, w, s);
        if (rc) return rc;
        hipLaunchKernelGGL(cem_refit_kernel, dim3(1), dim3(1024), 0, s, B, n, n_elite, w.J, w.X, w.mean, w.stdv, best_out_dev, it == 0 ? 1 : 0);
        GPMPC_HIP_CHECK(h, hipGetLastError());
    }
    return GPMPC_OK;
}

// One iteration of the search for the slice [b0, b0 + Bl) of a population of B_total candidates (a.B = Bl): the population step +
// the slice's elite records.  `state` = mean | std | best | best J as left by run_cem_merge of the previous iteration.
int run_cem_local(Handle* h, RolloutArgs& a, int B_total, int b0, int it, int n_elite, unsigned long long seed,
                  const double* first_host, int mapper, const double* max_change_host, const double* a_prev_host,
                  const double* noise_dev, const double* state_dev, double* elites_out_dev, hipStream_t s) {
    const int Bl = a.B, n = a.H * a.A;
    if (B_total < 2 || B_total > kCemMaxB || Bl < 0 || b0 < 0 || b0 + Bl > B_total || it < 0 || n_elite < 1 || n_elite > B_total) {
        h->err = "cem: need 2 <= B_total <= 4096, a slice inside it, 1 <= n_elite <= B_total"; return GPMPC_ERR_ARG;
    }
    CemWork w{};                         // (Bl == 0, more GPUs than candidates: padding records only, X and J are not read)
    if (Bl > 0) {
        int rc = cem_population_step(h, a, B_total, b0, it, seed, first_host, mapper, max_change_host, a_prev_host, noise_dev, state_dev,
                                     state_dev + n, state_dev + 2 * n, w, s);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(cem_elites_kernel, dim3(1), dim3(1024), 0, s, Bl, n, n_elite, b0, w.J, w.X, elites_out_dev);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

int run_cem_merge(Handle* h, const double* elites_dev, int lists, int n_elite, int n, int it, double* state_dev, hipStream_t s) {
    if (lists < 1 || n_elite < 1 || n < 1 || (long long)lists * n_elite > kCemMaxB) {
        h->err = "cem: lists x n_elite must not exceed 4096 records"; return GPMPC_ERR_LIMIT;
    }
    hipLaunchKernelGGL(cem_merge_kernel, dim3(1), dim3(1024), 0, s, lists * n_elite, n, n_elite, elites_dev, state_dev, it == 0 ? 1 : 0);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

}  // namespace gpmpc_hip
