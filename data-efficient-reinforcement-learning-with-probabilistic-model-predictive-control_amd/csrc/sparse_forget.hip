// sparse_forget.hip -- kernels of gpmpc_sparse_forget for gfx950 (MI355X, CDNA4): one memory point (x, y) leaves the sparse GP
// gpmpc_prepare_sparse cached, in O(M^2) per output and without touching anything of size N -- the append of sparse_append.hip with
// the opposite sign.  With Z and the hyper-parameters fixed the point is a rank-one change of B = I + V V^T / n:
// B' = B - u u^T = LB (I - p p^T) LB^T.  Per output a (n = noise_a, sigma2 = var_a), from the record (Yu, Yb, w, noises):
//   kz = k_a(Z, x)                                  the arithmetic of sparse_panel_kernel: differences per element, libm's exp
//   v  = Yu kz,  u = v / sqrt(n),  p = Yb u
//   t_0 = 1,  t_{i+1} = t_i - p_i^2 (i ascending),  tau = t_M = 1 - p^T p
//   LOST PIVOT if some t_{i+1} is not > 0 (NaN included), or tau < 1 / (2 (1 + sigma2 / n))
//   g  = Yu^T (Yb^T p)                              with the OLD Yb
//   iK_eff[i,j] -= g_i g_j / tau                    B'^-1 = B^-1 + (B^-1 u)(B^-1 u)^T / tau: the bracket I - B^-1 SHRINKS by a rank one
//   d_i = sqrt(t_{i+1} / t_i),  c_i = p_i / sqrt(t_i t_{i+1})      chol(I - p p^T): diagonal d_i, -p_i c_j below it
//   per column j:  acc = 0;  for i = j .. M-1:  Yb'[i,j] = (Yb[i,j] + p_i acc) / d_i;  acc += c_i Yb'[i,j]       Yb' = chol(I - p p^T)^-1 Yb
//   w' = w - v y
// Unlike the append this subtracts from positive quantities.  For a point that is in the model tau >= 1 / (1 + sigma2 / n); half
// of that separates rounding from a point that never was.  Two launches per point:
//   sparse_forget_vectors_kernel   a workgroup per output runs the chain kz -> v -> p -> t -> Yb^T p -> g in LDS; an output that
//                                  loses its pivot writes 1 + the point's number into its failure word and stops;
//   sparse_forget_update_kernel    per (output, 64-column tile) the Yb' recurrence in place, beside it the element-wise update of
//                                  iK_eff, and w' (the first workgroup of an output).
// Both read the failure words first and do nothing once one is set by an earlier launch: the model then stays that of the points
// removed before, and the driver (run_sparse_forget, prepare.hip) reports GPMPC_ERR_NOT_PD.  beta_eff and the T table follow once per
// call (launch_sparse_beta, tm_kernel).  Plain kernels: no atomics, no waits between workgroups; every sum runs in an order fixed by
// M, D and E alone.  The two products with Yu / Yb are the append's (sparse_rank_one.h).
#include "device_common.h"
#include "sparse_forget_plan.h"
#include "sparse_rank_one.h"

// every fused multiply-add of this file is written out as fma(): the recurrence's sums round as gpmpc.h writes them
#pragma clang fp contract(off)

namespace gpmpc_hip {

namespace {

// The vectors of one removed point (number `point` of the call), a workgroup per output.  Dynamic LDS (plan_sparse_forget): x / l
// and 1 / l (2 x 24) | kz, later q = Yb^T p (M) | u (M) | p (M) | t (M + 1) | partial sums (groups x M) | the verdict (1).
// A failure word holding another point's mark was set by an earlier launch: nothing is done.  One holding this point's mark is
// being written by another output's workgroup of this launch and is ignored, so what an output does never depends on timing.
__global__ __launch_bounds__(kAppendThreads) void sparse_forget_vectors_kernel(
    const double* __restrict__ Zt, const double* __restrict__ ils2, const double* __restrict__ var, const double* __restrict__ Yuall,
    const double* __restrict__ Yball, const double* __restrict__ noise, const double* __restrict__ xold, int M, int D, int E,
    int nct, int groups, int rpg, int point, double* __restrict__ vall, double* __restrict__ pall, double* __restrict__ call,
    double* __restrict__ dall, double* __restrict__ gall, double* __restrict__ tauall, int* fail) {
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
    if (tid == 0) {
        bool dead = false;
        for (int b = 0; b < D; ++b) {
            const int f = fail[b];
            dead = dead || (f != 0 && f != point + 1);
        }
        verdict[0] = dead ? 1.0 : 0.0;
    }
    if (tid < E) {
        const double l = sqrt(ils2[a * E + tid]);
        il[tid] = l;
        xs[tid] = xold[tid] * l;
    }
    __syncthreads();
    if (verdict[0] != 0.0) return;
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
    // v = Yu kz (kept for w'), u = v / sqrt(n)
    const double nz = noise[a];
    const double sn = sqrt(nz);
    for (int i = wave; i < M; i += kAppendWaves) {
        const double v = row_dot(Yu + (size_t)i * M, a0, i, lane);
        if (lane == 0) {
            u[i] = v / sn;
            vall[(size_t)a * M + i] = v;
        }
    }
    __syncthreads();
    // p = Yb u
    for (int i = wave; i < M; i += kAppendWaves) {
        const double pi = row_dot(Yb + (size_t)i * M, u, i, lane);
        if (lane == 0) p[i] = pi;
    }
    __syncthreads();
    // t: one chain, i ascending; every link must stay positive and the last one above the floor of a point that is in the model
    if (tid == 0) {
        double ti = 1.0;
        bool lost = false;
        t[0] = ti;
        for (int i = 0; i < M; ++i) {
            ti = ti - p[i] * p[i];
            t[i + 1] = ti;
            lost = lost || !(ti > 0.0);
        }
        lost = lost || ti < 1.0 / (2.0 * (1.0 + va / nz));
        tauall[a] = ti;
        if (lost) {
            fail[a] = point + 1;
            verdict[0] = 1.0;
        }
    }
    __syncthreads();
    if (verdict[0] != 0.0) return;
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
// rows from the tile's first on in LDS); the first of them also forms w' = w - v y.  The others: iK_eff[i,j] -= g_i g_j / tau
// element by element -- the product taken as g_min(i,j) g_max(i,j), as the append forms it, so that [i,j] and [j,i] see the same
// three operands in the same order.  Nothing is done once any output has lost its pivot (no launch writes the words meanwhile).
__global__ __launch_bounds__(kAppendUpdThreads) void sparse_forget_update_kernel(
    double* __restrict__ Yball, double* __restrict__ iKall, double* __restrict__ wall, const double* __restrict__ vall,
    const double* __restrict__ pall, const double* __restrict__ call, const double* __restrict__ dall, const double* __restrict__ gall,
    const double* __restrict__ tauall, const double* __restrict__ yold, const int* __restrict__ fail, int M, int D, int rec_blocks) {
    extern __shared__ double lds[];
    const int a = blockIdx.y;
    const int tid = threadIdx.x;
    for (int b = 0; b < D; ++b)
        if (fail[b] != 0) return;
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
        if (blockIdx.x == 0) {
            const double y = yold[a];
            for (int i = tid; i < M; i += kAppendUpdThreads) wall[(size_t)a * M + i] = wall[(size_t)a * M + i] - vall[(size_t)a * M + i] * y;
        }
        __syncthreads();
        const int j = j0 + tid;
        if (tid >= kAppendTile || j >= M) return;
        double* Yb = Yball + (size_t)a * M * M;
        double acc = 0.0;
#pragma unroll 4
        for (int i = j; i < M; ++i) {
            const double yn = (Yb[(size_t)i * M + j] + sp[i] * acc) / sd[i];
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
            iK[idx] = iK[idx] - (g[lo] * g[hi]) / tau;
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// Before the first launch of a call: the dynamic LDS of the two kernels within the device's limit (GPMPC_ERR_LIMIT otherwise),
// their limits raised where they need more than the default 64 KiB
int check_sparse_forget(Handle* h, const SparseForgetPlan& fp) {
    if (fp.lds_bytes > (size_t)h->lds_limit || fp.upd_lds_bytes > (size_t)h->lds_limit) {
        h->err = "sparse_forget: M inducing inputs need more LDS than a workgroup has";
        return GPMPC_ERR_LIMIT;
    }
    int rc;
    if (fp.lds_bytes > 64 * 1024 && (rc = allow_full_lds(h, (const void*)sparse_forget_vectors_kernel))) return rc;
    if (fp.upd_lds_bytes > 64 * 1024 && (rc = allow_full_lds(h, (const void*)sparse_forget_update_kernel))) return rc;
    return GPMPC_OK;
}

// Point number `point` of the call (x (E), y (D)) leaves the record: Yu (D, M, M) read, Yb and w (at `rec`, the layout of `ap`) and
// h->iK updated in place; `ws` is the scratch of `fp` (h->Xt / ils2 / var hold the packed Z and hyper-parameters)
int launch_sparse_forget_point(Handle* h, const SparseAppendPlan& ap, const SparseForgetPlan& fp, const double* Yu, double* rec,
                               double* ws, const double* x, const double* y, int point, int M, int D, int E, hipStream_t s) {
    int* fail = reinterpret_cast<int*>(ws + fp.fail);
    hipLaunchKernelGGL(sparse_forget_vectors_kernel, dim3(D), dim3(kAppendThreads), fp.lds_bytes, s, h->Xt.p, h->ils2.p, h->var.p, Yu,
                       rec + ap.yb, rec + ap.noise, x, M, D, E, fp.nct, fp.groups, fp.rows_per_group, point, ws + fp.v, ws + fp.p,
                       ws + fp.c, ws + fp.d, ws + fp.g, ws + fp.tau, fail);
    hipLaunchKernelGGL(sparse_forget_update_kernel, dim3(fp.upd_rec_blocks + fp.upd_ik_blocks, D), dim3(kAppendUpdThreads),
                       fp.upd_lds_bytes, s, rec + ap.yb, h->iK.p, rec + ap.w, ws + fp.v, ws + fp.p, ws + fp.c, ws + fp.d, ws + fp.g,
                       ws + fp.tau, y, fail, M, D, fp.upd_rec_blocks);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

}  // namespace gpmpc_hip
