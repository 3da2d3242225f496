// sparse_append.hip -- kernels of gpmpc_sparse_append for gfx950 (MI355X, CDNA4): one more memory point (x, y) joins the sparse GP
// gpmpc_prepare_sparse cached, in O(M^2) per output and without touching anything of size N.  With Z and the hyper-parameters fixed
// the point is a rank-one change of B = I + V V^T / n: B' = B + u u^T = LB (I + p p^T) LB^T.  Per output a (n = noise_a), from the
// record (Yu = Lu^-1, Yb = LB^-1, w = V y) that gpmpc_prepare_sparse leaves:
//   kz = k_a(Z, x)                                  the arithmetic of sparse_panel_kernel: differences per element, libm's exp
//   v  = Yu kz,  u = v / sqrt(n),  p = Yb u
//   t_0 = 1,  t_{i+1} = t_i + p_i^2 (i ascending),  tau = t_M = 1 + p^T p
//   g  = Yu^T (Yb^T p)                              with the OLD Yb
//   iK_eff[i,j] += g_i g_j / tau                    B'^-1 = B^-1 - (B^-1 u)(B^-1 u)^T / tau: the bracket I - B^-1 GROWS by a rank one
//   d_i = sqrt(t_{i+1} / t_i),  c_i = p_i / sqrt(t_i t_{i+1})      chol(I + p p^T): diagonal d_i, p_i c_j below it
//   per column j:  acc = 0;  for i = j .. M-1:  Yb'[i,j] = (Yb[i,j] - p_i acc) / d_i;  acc += c_i Yb'[i,j]       Yb' = chol(I + p p^T)^-1 Yb
//   w' = w + v y
// Every t_i is a sum of positives >= 1: there is no pivot to lose.  Two launches per point:
//   sparse_append_vectors_kernel   a workgroup per output runs the chain kz -> v -> p -> t -> Yb^T p -> g (and w'); the vectors of
//                                  an output live in LDS; the products with Yu / Yb are a wavefront per row, the transposed ones a
//                                  lane per column with the rows of a column tile split into groups whose partial sums are added
//                                  in group order;
//   sparse_append_update_kernel    per (output, 64-column tile) the Yb' recurrence in place (columns are independent), and beside
//                                  it in the same launch the element-wise update of iK_eff.
// beta_eff and the T table follow once per call (launch_sparse_beta, tm_kernel).  Plain kernels: no atomics, no waits between
// workgroups; every sum runs in an order fixed by M, D and E alone.  The driver (run_sparse_append) is in prepare.hip.
#include "device_common.h"
#include "sparse_append_plan.h"
#include "sparse_rank_one.h"

// every fused multiply-add of this file is written out as fma(): the recurrence's sums round as gpmpc.h writes them
#pragma clang fp contract(off)

namespace gpmpc_hip {

namespace {

// The vectors of one appended point, a workgroup per output.  Dynamic LDS (plan_sparse_append): x / l and 1 / l (2 x 24) | kz, later
// q = Yb^T p (M) | u (M) | p (M) | t (M + 1) | partial sums of the transposed products (groups x M).
__global__ __launch_bounds__(kAppendThreads) void sparse_append_vectors_kernel(
    const double* __restrict__ Zt, const double* __restrict__ ils2, const double* __restrict__ var, const double* __restrict__ Yuall,
    const double* __restrict__ Yball, const double* __restrict__ noise, const double* __restrict__ xnew,
    const double* __restrict__ ynew, int M, int D, int E, int nct, int groups, int rpg, double* __restrict__ wall,
    double* __restrict__ pall, double* __restrict__ call, double* __restrict__ dall, double* __restrict__ gall,
    double* __restrict__ tauall) {
    extern __shared__ double lds[];
    double* xs = lds;
    double* il = lds + 24;
    double* a0 = lds + 48;
    double* u = a0 + M;
    double* p = u + M;
    double* t = p + M;
    double* part = t + M + 1;
    const int a = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* Yu = Yuall + (size_t)a * M * M;
    const double* Yb = Yball + (size_t)a * M * M;
    if (tid < E) {
        const double l = sqrt(ils2[a * E + tid]);
        il[tid] = l;
        xs[tid] = xnew[tid] * l;
    }
    __syncthreads();
    // kz = k_a(Z, x)
    const double va = var[a];
    for (int k = tid; k < M; k += kAppendThreads) {
        double s = 0.0;
        for (int e = 0; e < E; ++e) {
            const double d = Zt[(size_t)e * M + k] * il[e] - xs[e];
            s = fma(d, d, s);
        }
        a0[k] = va * exp(-0.5 * s);
    }
    __syncthreads();
    // v = Yu kz, u = v / sqrt(n), w' = w + v y
    const double sn = sqrt(noise[a]);
    const double y = ynew[a];
    for (int i = wave; i < M; i += kAppendWaves) {
        const double v = row_dot(Yu + (size_t)i * M, a0, i, lane);
        if (lane == 0) {
            u[i] = v / sn;
            wall[(size_t)a * M + i] = wall[(size_t)a * M + i] + v * y;
        }
    }
    __syncthreads();
    // p = Yb u
    for (int i = wave; i < M; i += kAppendWaves) {
        const double pi = row_dot(Yb + (size_t)i * M, u, i, lane);
        if (lane == 0) p[i] = pi;
    }
    __syncthreads();
    // t: one chain, i ascending
    if (tid == 0) {
        double ti = 1.0;
        t[0] = ti;
        for (int i = 0; i < M; ++i) {
            ti = ti + p[i] * p[i];
            t[i + 1] = ti;
        }
        tauall[a] = ti;
    }
    __syncthreads();
    for (int i = tid; i < M; i += kAppendThreads) {
        pall[(size_t)a * M + i] = p[i];
        dall[(size_t)a * M + i] = sqrt(t[i + 1] / t[i]);
        call[(size_t)a * M + i] = p[i] / sqrt(t[i] * t[i + 1]);
    }
    // g = Yu^T (Yb^T p), with the Yb of before this point
    trans_product(Yb, p, M, nct, groups, rpg, part, a0);
    trans_product(Yu, a0, M, nct, groups, rpg, part, gall + (size_t)a * M);
}

// Workgroups [0, rec_blocks) of an output: the Yb' recurrence of one 64-column tile, in place, a lane per column (p, c, d of the
// rows from the tile's first on in LDS).  The others: iK_eff[i,j] += g_i g_j / tau element by element -- the product taken as
// g_min(i,j) g_max(i,j), so that with the exactly symmetric iK_eff every writer of a sparse model leaves, [i,j] and [j,i] see the
// same three operands in the same order: the bits of forming i <= j and mirroring, with coalesced stores.
__global__ __launch_bounds__(kAppendUpdThreads) void sparse_append_update_kernel(
    double* __restrict__ Yball, double* __restrict__ iKall, const double* __restrict__ pall, const double* __restrict__ call,
    const double* __restrict__ dall, const double* __restrict__ gall, const double* __restrict__ tauall, int M, int rec_blocks) {
    extern __shared__ double lds[];
    const int a = blockIdx.y;
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < rec_blocks) {
        double* sp = lds;
        double* sc = lds + M;
        double* sd = lds + 2 * (size_t)M;
        const int j0 = blockIdx.x * kAppendTile;
        for (int i = j0 + tid; i < M; i += kAppendUpdThreads) {
            sp[i] = pall[(size_t)a * M + i];
            sc[i] = call[(size_t)a * M + i];
            sd[i] = dall[(size_t)a * M + i];
        }
        __syncthreads();
        const int j = j0 + tid;
        if (tid >= kAppendTile || j >= M) return;
        double* Yb = Yball + (size_t)a * M * M;
        double acc = 0.0;
#pragma unroll 4
        for (int i = j; i < M; ++i) {
            const double yn = (Yb[(size_t)i * M + j] - sp[i] * acc) / sd[i];
            Yb[(size_t)i * M + j] = yn;
            acc = acc + sc[i] * yn;
        }
        return;
    }
    const double* g = gall + (size_t)a * M;
    double* iK = iKall + (size_t)a * M * M;
    const double tau = tauall[a];
    const size_t MM = (size_t)M * M;
    const size_t base = (size_t)(blockIdx.x - rec_blocks) * (kAppendUpdThreads * kAppendUpdPerThread) + tid;
#pragma unroll
    for (int q = 0; q < kAppendUpdPerThread; ++q) {
        const size_t idx = base + (size_t)q * kAppendUpdThreads;
        if (idx < MM) {
            const int i = (int)(idx / M), j = (int)(idx - (size_t)i * M);
            const int lo = i < j ? i : j, hi = i < j ? j : i;
            iK[idx] = iK[idx] + (g[lo] * g[hi]) / tau;
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// Before the first launch of a call: the dynamic LDS of the two kernels within the device's limit (GPMPC_ERR_LIMIT otherwise),
// their limits raised where they need more than the default 64 KiB
int check_sparse_append(Handle* h, const SparseAppendPlan& ap) {
    if (ap.lds_bytes > (size_t)h->lds_limit || ap.upd_lds_bytes > (size_t)h->lds_limit) {
        h->err = "sparse_append: M inducing inputs need more LDS than a workgroup has";
        return GPMPC_ERR_LIMIT;
    }
    int rc;
    if (ap.lds_bytes > 64 * 1024 && (rc = allow_full_lds(h, (const void*)sparse_append_vectors_kernel))) return rc;
    if (ap.upd_lds_bytes > 64 * 1024 && (rc = allow_full_lds(h, (const void*)sparse_append_update_kernel))) return rc;
    return GPMPC_OK;
}

// One point (x (E), y (D)) joins the record: Yu (D, M, M) read, `rec` (the layout of `ap`) updated in place together with h->iK
// (h->Xt / ils2 / var hold the packed Z and hyper-parameters)
int launch_sparse_append_point(Handle* h, const SparseAppendPlan& ap, const double* Yu, double* rec, const double* x, const double* y,
                               int M, int D, int E, hipStream_t s) {
    hipLaunchKernelGGL(sparse_append_vectors_kernel, dim3(D), dim3(kAppendThreads), ap.lds_bytes, s, h->Xt.p, h->ils2.p, h->var.p, Yu,
                       rec + ap.yb, rec + ap.noise, x, y, M, D, E, ap.nct, ap.groups, ap.rows_per_group, rec + ap.w, rec + ap.p,
                       rec + ap.c, rec + ap.d, rec + ap.g, rec + ap.tau);
    hipLaunchKernelGGL(sparse_append_update_kernel, dim3(ap.upd_rec_blocks + ap.upd_ik_blocks, D), dim3(kAppendUpdThreads),
                       ap.upd_lds_bytes, s, rec + ap.yb, h->iK.p, rec + ap.p, rec + ap.c, rec + ap.d, rec + ap.g, rec + ap.tau, M,
                       ap.upd_rec_blocks);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

}  // namespace gpmpc_hip
