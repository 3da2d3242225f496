// sparse_update.hip -- kernels of gpmpc_sparse_append and gpmpc_sparse_forget for gfx950 (MI355X, CDNA4): one memory point (x, y)
// joins (+) or leaves (-) the sparse GP gpmpc_prepare_sparse cached, in O(M^2) per output and without touching anything of size N.
// One recurrence with a sign chosen at compile time (template <bool Forget>; upper sign: append, lower sign: forget).  With Z and
// the hyper-parameters fixed the point is a rank-one change of B = I + V V^T / n: B' = B +- u u^T = LB (I +- p p^T) LB^T.  Per output
// a (n = noise_a, sigma2 = var_a), from the record (Yu = Lu^-1, Yb = LB^-1, w = V y, noises) that gpmpc_prepare_sparse leaves:
//   kz = k_a(Z, x)                                  the arithmetic of sparse_panel_kernel: differences per element, libm's exp
//   v  = Yu kz,  u = v / sqrt(n),  p = Yb u
//   t_0 = 1,  t_{i+1} = t_i +- p_i^2 (i ascending),  tau = t_M = 1 +- p^T p
//   forget: LOST PIVOT if some t_{i+1} is not > 0 (NaN included), or tau < 1 / (2 (1 + sigma2 / n))
//   g  = Yu^T (Yb^T p)                              with the OLD Yb
//   iK_eff[i,j] +-= g_i g_j / tau                   B'^-1 = B^-1 -+ (B^-1 u)(B^-1 u)^T / tau: the bracket I - B^-1 grows / shrinks by a rank one
//   d_i = sqrt(t_{i+1} / t_i),  c_i = p_i / sqrt(t_i t_{i+1})      chol(I +- p p^T): diagonal d_i, +- p_i c_j below it
//   per column j:  acc = 0;  for i = j .. M-1:  Yb'[i,j] = (Yb[i,j] -+ p_i acc) / d_i;  acc += c_i Yb'[i,j]       Yb' = chol(I +- p p^T)^-1 Yb
//   w' = w +- v y
// The append's t_i are sums of positives >= 1: there is no pivot to lose.  The forget subtracts from positive quantities; for a point
// that is in the model tau >= 1 / (1 + sigma2 / n), and half of that separates rounding from a point that never was.  Two launches
// per point:
//   sparse_update_vectors_kernel   a workgroup per output runs the chain kz -> v -> p -> t -> Yb^T p -> g; the vectors of an output
//                                  live in LDS; the products with Yu / Yb are a wavefront per row, the transposed ones a lane per
//                                  column with the rows of a column tile split into groups whose partial sums are added in group
//                                  order.  The append forms w' here; a forgetting output that loses its pivot writes 1 + the
//                                  point's number into its failure word and stops;
//   sparse_update_update_kernel    per (output, 64-column tile) the Yb' recurrence in place (columns are independent), beside it in
//                                  the same launch the element-wise update of iK_eff, and the forget's w' (the first workgroup of
//                                  an output).
// The forget's kernels read the failure words first and do nothing once one is set by an earlier launch: the model then stays that
// of the points removed before, and the driver (run_sparse_update, prepare.hip) reports GPMPC_ERR_NOT_PD.  beta_eff and the T table
// follow once per call (launch_sparse_beta, launch_tm).  Plain kernels: no atomics, no waits between workgroups; every sum runs in an
// order fixed by M, D and E alone.
#include "device_common.h"
#include "sparse_update_plan.h"

// every fused multiply-add of this file is written out as fma(): the recurrence's sums round as gpmpc.h writes them
#pragma clang fp contract(off)

namespace gpmpc_hip {

namespace {

// a + b for the append, a - b for the forget
template <bool Forget>
__device__ inline double signed_sum(double a, double b) {
    if constexpr (Forget) return a - b;
    else return a + b;
}

// a row of a lower-triangular matrix times x (LDS): lane-strided partial sums, then the xor tree -- every lane gets the total
__device__ inline double row_dot(const double* __restrict__ row, const double* x, int i, int lane) {
    double s = 0.0;
    for (int k = lane; k <= i; k += 64) s = fma(row[k], x[k], s);
    return wave_xor_sum(s);
}

// out = A^T x for a lower-triangular row-major A (M, M), x in LDS: work item (column tile, row group) per wavefront, lane = column,
// rows ascending inside a group (the first row of column j is j); then the groups' partial sums in group order
__device__ inline void trans_product(const double* __restrict__ A, const double* x, int M, int nct, int groups, int rpg,
                                     double* part, double* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int it = wave; it < nct * groups; it += kUpdVecWaves) {
        const int tile = it % nct, grp = it / nct;
        const int j = tile * kUpdTile + lane;
        if (j >= M) continue;
        const int r1 = (grp + 1) * rpg < M ? (grp + 1) * rpg : M;
        int i = grp * rpg > j ? grp * rpg : j;
        double s = 0.0;
#pragma unroll 4
        for (; i < r1; ++i) s = fma(A[(size_t)i * M + j], x[i], s);
        part[(size_t)grp * M + j] = s;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < M; j += kUpdVecThreads) {
        double s = part[j];
        for (int q = 1; q < groups; ++q) s += part[(size_t)q * M + j];
        out[j] = s;
    }
    __syncthreads();
}

// The vectors of one point (number `point` of the call), a workgroup per output.  Dynamic LDS (plan_sparse_update): x / l and 1 / l
// (2 x 24) | kz, later q = Yb^T p (M) | u (M) | p (M) | t (M + 1) | partial sums of the transposed products (groups x M) | the
// forget's verdict (1).  The append reads y and updates w (wall); the forget keeps v (vall) for the update kernel and uses the
// failure words: one holding another point's mark was set by an earlier launch and nothing is done; one holding this point's mark
// is being written by another output's workgroup of this launch and is ignored, so what an output does never depends on timing.
template <bool Forget>
__global__ __launch_bounds__(kUpdVecThreads) void sparse_update_vectors_kernel(
    const double* __restrict__ Zt, const double* __restrict__ ils2, const double* __restrict__ var, const double* __restrict__ Yuall,
    const double* __restrict__ Yball, const double* __restrict__ noise, const double* __restrict__ xpt,
    const double* __restrict__ ypt, int M, int D, int E, int nct, int groups, int rpg, int point, double* __restrict__ wall,
    double* __restrict__ vall, double* __restrict__ pall, double* __restrict__ call, double* __restrict__ dall,
    double* __restrict__ gall, double* __restrict__ tauall, int* fail) {
    extern __shared__ double lds[];
    double* xs = lds;
    double* il = lds + 24;
    double* a0 = lds + 48;
    double* u = a0 + M;
    double* p = u + M;
    double* t = p + M;
    double* part = t + M + 1;
    double* verdict = part + (size_t)groups * M;
    const int a = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* Yu = Yuall + (size_t)a * M * M;
    const double* Yb = Yball + (size_t)a * M * M;
    if constexpr (Forget) {
        if (tid == 0) {
            bool dead = false;
            for (int b = 0; b < D; ++b) {
                const int f = fail[b];
                dead = dead || (f != 0 && f != point + 1);
            }
            verdict[0] = dead ? 1.0 : 0.0;
        }
    }
    if (tid < E) {
        const double l = sqrt(ils2[a * E + tid]);
        il[tid] = l;
        xs[tid] = xpt[tid] * l;
    }
    __syncthreads();
    if constexpr (Forget) {
        if (verdict[0] != 0.0) return;
    }
    // kz = k_a(Z, x)
    const double va = var[a];
    for (int k = tid; k < M; k += kUpdVecThreads) {
        double s = 0.0;
        for (int e = 0; e < E; ++e) {
            const double d = Zt[(size_t)e * M + k] * il[e] - xs[e];
            s = fma(d, d, s);
        }
        a0[k] = va * exp(-0.5 * s);
    }
    __syncthreads();
    // v = Yu kz, u = v / sqrt(n); the append's w' = w + v y, the forget keeps v for its w'
    const double nz = noise[a];
    const double sn = sqrt(nz);
    double y = 0.0;
    if constexpr (!Forget) y = ypt[a];
    for (int i = wave; i < M; i += kUpdVecWaves) {
        const double v = row_dot(Yu + (size_t)i * M, a0, i, lane);
        if (lane == 0) {
            u[i] = v / sn;
            if constexpr (Forget) vall[(size_t)a * M + i] = v;
            else wall[(size_t)a * M + i] = wall[(size_t)a * M + i] + v * y;
        }
    }
    __syncthreads();
    // p = Yb u
    for (int i = wave; i < M; i += kUpdVecWaves) {
        const double pi = row_dot(Yb + (size_t)i * M, u, i, lane);
        if (lane == 0) p[i] = pi;
    }
    __syncthreads();
    // t: one chain, i ascending; the forget's links must stay positive and the last one above the floor of a point that is in the model
    if (tid == 0) {
        double ti = 1.0;
        [[maybe_unused]] bool lost = false;
        t[0] = ti;
        for (int i = 0; i < M; ++i) {
            ti = signed_sum<Forget>(ti, p[i] * p[i]);
            t[i + 1] = ti;
            if constexpr (Forget) lost = lost || !(ti > 0.0);
        }
        if constexpr (Forget) lost = lost || ti < 1.0 / (2.0 * (1.0 + va / nz));
        tauall[a] = ti;
        if constexpr (Forget) {
            if (lost) {
                fail[a] = point + 1;
                verdict[0] = 1.0;
            }
        }
    }
    __syncthreads();
    if constexpr (Forget) {
        if (verdict[0] != 0.0) return;
    }
    for (int i = tid; i < M; i += kUpdVecThreads) {
        pall[(size_t)a * M + i] = p[i];
        dall[(size_t)a * M + i] = sqrt(t[i + 1] / t[i]);
        call[(size_t)a * M + i] = p[i] / sqrt(t[i] * t[i + 1]);
    }
    // g = Yu^T (Yb^T p), with the Yb of before this point
    trans_product(Yb, p, M, nct, groups, rpg, part, a0);
    trans_product(Yu, a0, M, nct, groups, rpg, part, gall + (size_t)a * M);
}

// Workgroups [0, rec_blocks) of an output: the Yb' recurrence of one 64-column tile, in place, a lane per column (p, c, d of the
// rows from the tile's first on in LDS); the forget's first also forms w' = w - v y.  The others: iK_eff[i,j] +-= g_i g_j / tau
// element by element -- the product taken as g_min(i,j) g_max(i,j), so that with the exactly symmetric iK_eff every writer of a
// sparse model leaves, [i,j] and [j,i] see the same three operands in the same order: the bits of forming i <= j and mirroring,
// with coalesced stores.  The forget does nothing once any output has lost its pivot (no launch writes the words meanwhile).
template <bool Forget>
__global__ __launch_bounds__(kUpdThreads) void sparse_update_update_kernel(
    double* __restrict__ Yball, double* __restrict__ iKall, double* __restrict__ wall, const double* __restrict__ vall,
    const double* __restrict__ pall, const double* __restrict__ call, const double* __restrict__ dall, const double* __restrict__ gall,
    const double* __restrict__ tauall, const double* __restrict__ ypt, const int* __restrict__ fail, int M, int D, int rec_blocks) {
    extern __shared__ double lds[];
    const int a = blockIdx.y;
    const int tid = threadIdx.x;
    if constexpr (Forget) {
        for (int b = 0; b < D; ++b)
            if (fail[b] != 0) return;
    }
    if ((int)blockIdx.x < rec_blocks) {
        double* sp = lds;
        double* sc = lds + M;
        double* sd = lds + 2 * (size_t)M;
        const int j0 = blockIdx.x * kUpdTile;
        for (int i = j0 + tid; i < M; i += kUpdThreads) {
            sp[i] = pall[(size_t)a * M + i];
            sc[i] = call[(size_t)a * M + i];
            sd[i] = dall[(size_t)a * M + i];
        }
        if constexpr (Forget) {
            if (blockIdx.x == 0) {
                const double y = ypt[a];
                for (int i = tid; i < M; i += kUpdThreads) wall[(size_t)a * M + i] = wall[(size_t)a * M + i] - vall[(size_t)a * M + i] * y;
            }
        }
        __syncthreads();
        const int j = j0 + tid;
        if (tid >= kUpdTile || j >= M) return;
        double* Yb = Yball + (size_t)a * M * M;
        double acc = 0.0;
#pragma unroll 4
        for (int i = j; i < M; ++i) {
            const double yn = signed_sum<!Forget>(Yb[(size_t)i * M + j], sp[i] * acc) / sd[i];      // the opposite sign: - p_i acc for the append
            Yb[(size_t)i * M + j] = yn;
            acc = acc + sc[i] * yn;
        }
        return;
    }
    const double* g = gall + (size_t)a * M;
    double* iK = iKall + (size_t)a * M * M;
    const double tau = tauall[a];
    const size_t MM = (size_t)M * M;
    const size_t base = (size_t)(blockIdx.x - rec_blocks) * (kUpdThreads * kUpdPerThread) + tid;
#pragma unroll
    for (int q = 0; q < kUpdPerThread; ++q) {
        const size_t idx = base + (size_t)q * kUpdThreads;
        if (idx < MM) {
            const int i = (int)(idx / M), j = (int)(idx - (size_t)i * M);
            const int lo = i < j ? i : j, hi = i < j ? j : i;
            iK[idx] = signed_sum<Forget>(iK[idx], (g[lo] * g[hi]) / tau);
        }
    }
}

// The limits are raised for the instantiation that launch_point<Forget> launches: each is a kernel of its own to the runtime.
template <bool Forget>
int check_lds(Handle* h, const SparseUpdatePlan& p) {
    if (p.lds_bytes > (size_t)h->lds_limit || p.upd_lds_bytes > (size_t)h->lds_limit) {
        h->err = std::string(Forget ? "sparse_forget" : "sparse_append") + ": M inducing inputs need more LDS than a workgroup has";
        return GPMPC_ERR_LIMIT;
    }
    int rc;
    if (p.lds_bytes > 64 * 1024 && (rc = allow_full_lds(h, (const void*)sparse_update_vectors_kernel<Forget>))) return rc;
    if (p.upd_lds_bytes > 64 * 1024 && (rc = allow_full_lds(h, (const void*)sparse_update_update_kernel<Forget>))) return rc;
    return GPMPC_OK;
}

template <bool Forget>
int launch_point(Handle* h, const SparseUpdatePlan& p, const double* Yu, double* rec, double* ws, const double* x, const double* y,
                 int point, int M, int D, int E, hipStream_t s) {
    int* fail = reinterpret_cast<int*>(ws + p.fail);
    hipLaunchKernelGGL(sparse_update_vectors_kernel<Forget>, dim3(D), dim3(kUpdVecThreads), p.lds_bytes, s, h->Xt.p, h->ils2.p,
                       h->var.p, Yu, rec + p.yb, rec + p.noise, x, y, M, D, E, p.nct, p.groups, p.rows_per_group, point, rec + p.w,
                       ws + p.v, ws + p.p, ws + p.c, ws + p.d, ws + p.g, ws + p.tau, fail);
    hipLaunchKernelGGL(sparse_update_update_kernel<Forget>, dim3(p.upd_rec_blocks + p.upd_ik_blocks, D), dim3(kUpdThreads),
                       p.upd_lds_bytes, s, rec + p.yb, h->iK.p, rec + p.w, ws + p.v, ws + p.p, ws + p.c, ws + p.d, ws + p.g, ws + p.tau,
                       y, fail, M, D, p.upd_rec_blocks);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// Before the first launch of a call: the dynamic LDS of the two kernels within the device's limit (GPMPC_ERR_LIMIT otherwise),
// their limits raised where they need more than the default 64 KiB
int check_sparse_update(Handle* h, const SparseUpdatePlan& p, bool forget) {
    return forget ? check_lds<true>(h, p) : check_lds<false>(h, p);
}

// Point number `point` of the call (x (E), y (D)) joins or leaves the record: Yu (D, M, M) read, Yb and w (at `rec`) and h->iK
// updated in place; `ws` is the scratch block of `p` (h->Xt / ils2 / var hold the packed Z and hyper-parameters)
int launch_sparse_update_point(Handle* h, const SparseUpdatePlan& p, const double* Yu, double* rec, double* ws, const double* x,
                               const double* y, int point, bool forget, int M, int D, int E, hipStream_t s) {
    return forget ? launch_point<true>(h, p, Yu, rec, ws, x, y, point, M, D, E, s)
                  : launch_point<false>(h, p, Yu, rec, ws, x, y, point, M, D, E, s);
}

}  // namespace gpmpc_hip
