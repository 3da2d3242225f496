// select_inducing.hip -- gpmpc_select_inducing for gfx950 (MI355X, CDNA4): greedy variance selection of M inducing inputs among the
// N memory points (Burt et al. 2019; Fine & Scheinberg 2001), a pivoted partial Cholesky of the D kernel matrices K_a = k_a(X, X)
// run in lockstep over the outputs because gpmpc_prepare_sparse takes one Z for all of them.  State: d_a(i) = sigma2_a, L_a = 0
// (M x N).  Step m picks the unpicked point p of largest s(i) = sum_a max(d_a(i), 0) / sigma2_a and, per output with
// d_a(p) > jitter_rel sigma2_a, appends the row c(i) = (k_a(x_i, x_p) - sum_{j<m} L_a[j, i] L_a[j, p]) / sqrt(d_a(p)) to L_a and
// takes c(i)^2 off d_a(i) (include/gpmpc.h has the whole contract).
//
// The recurrence is M dependent steps, each a stream over the rows of L written so far: ONE PLAIN LAUNCH PER STEP (a persistent
// kernel would need a grid-wide barrier per step).  A workgroup owns one 64-point tile, wavefront a of it owns output a.  Step
// m's prologue reduces the records (best score, point) the tiles left at step m - 1 to the pick p -- every workgroup does so
// redundantly, there are ceil(N / 64) records -- then each wavefront stages L_a[j, p] through LDS 64 rows at a time and streams
// L_a[j, tile] coalesced (L is stored (D, M, N), N contiguous), updates d_a, and the first wavefront sums the scores over the
// outputs through LDS (a ascending) and writes the tile's new record and its partial trace.  Records and d come in two
// generations (step m reads what step m - 1 wrote and writes the other one): a workgroup still in its prologue never sees this
// step's stores.  No atomics, no waits between workgroups; every sum runs in an order fixed by N, M, D and E alone.  A last
// small launch writes idx, gathers Z and sums the tile traces in ascending order.
#include <climits>
#include <cmath>
#include <cstdio>

#include "device_common.h"
#include "gpmpc_internal.h"
#include "select_inducing_plan.h"

namespace gpmpc_hip {

namespace {

struct SelectArgs {
    const double* X;         // (N, E)
    const double* ls;        // (D, E)
    const double* os;        // (D)
    double jitter_rel;
    int N, M, D, E, tiles;
    double* L;               // (D, M, N)
    double* d;               // (2, D, N)
    double* tpart;           // (M, tiles)
    double* rec_score;       // (2, tiles)
    int* rec_index;          // (2, tiles)
    int* picks;              // (M)
    int* picked;             // (N)
};

// the better of two records: the larger score, the lower point on a tie (scores here are finite or -inf, never NaN)
__device__ inline void take_better(double& k, int& i, double ok, int oi) {
    if (ok > k || (ok == k && oi < i)) { k = ok; i = oi; }
}

__global__ __launch_bounds__(64 * kMaxD) void select_step_kernel(SelectArgs g, int m) {
    __shared__ double dsq[kMaxE][kSparseTile];       // (x_ie - x_pe)^2 of the tile's points: shared by the outputs
    __shared__ double il2[kMaxD][kMaxE];             // 1 / l_ae^2
    __shared__ double lp[kMaxD][kSelectStage];       // L_a[j0 .. j0 + 63, p], one strip per wavefront
    __shared__ double sc[kMaxD][kSparseTile];        // max(d_a(i), 0) / sigma2_a
    __shared__ int p_s;
    const int tid = threadIdx.x, lane = tid & 63, a = tid >> 6;
    const int N = g.N, D = g.D, E = g.E, T = g.tiles, tile = blockIdx.x;
    const long long i = (long long)tile * kSparseTile + lane;
    const bool valid = i < N;

    // -- the pick of this step from the records of the last one (step 0: every score is exactly D, the lowest index wins)
    if (a == 0) {
        int p = 0;
        if (m > 0) {
            const double* rs = g.rec_score + (size_t)((m - 1) & 1) * T;
            const int* ri = g.rec_index + (size_t)((m - 1) & 1) * T;
            double bk = -INFINITY;
            int bi = INT_MAX;
            for (int t = lane; t < T; t += 64) take_better(bk, bi, rs[t], ri[t]);
            for (int off = 32; off >= 1; off >>= 1) {
                const double ok = __shfl_xor(bk, off, 64);
                const int oi = __shfl_xor(bi, off, 64);
                take_better(bk, bi, ok, oi);
            }
            p = ((unsigned)bi < (unsigned)N) ? bi : 0;           // (M <= N: an unpicked point always exists)
        }
        if (lane == 0) {
            p_s = p;
            if (tile == 0) g.picks[m] = p;
        }
    }
    for (int idx = tid; idx < D * E; idx += blockDim.x) {
        const double l = g.ls[idx];
        il2[idx / E][idx % E] = 1.0 / (l * l);
    }
    __syncthreads();
    const int p = p_s;
    {
        const size_t base = (size_t)tile * kSparseTile * E;
        const size_t have = ((size_t)N - (size_t)tile * kSparseTile) * E;      // doubles of X from the tile's first row on
        for (int idx = tid; idx < kSparseTile * E; idx += blockDim.x) {
            const int r = idx / E, e = idx - r * E;
            const double df = ((size_t)idx < have) ? g.X[base + idx] - g.X[(size_t)p * E + e] : 0.0;
            dsq[e][r] = df * df;
        }
    }
    __syncthreads();

    // -- output a: the new row of L_a over the tile, d_a
    const double va = g.os[a];
    const double* dold = g.d + ((size_t)((m - 1) & 1) * D + a) * N;
    double* dnew = g.d + ((size_t)(m & 1) * D + a) * N;
    const double dp = (m == 0) ? va : dold[p];
    double di = (m == 0) ? va : (valid ? dold[i] : 0.0);
    double* La = g.L + (size_t)a * g.M * N;
    double c = 0.0;
    if (dp > g.jitter_rel * va) {                                  // the same for the whole wavefront; else the pivot floor
        double sq = 0.0;
        for (int e = 0; e < E; ++e) sq = fma(dsq[e][lane], il2[a][e], sq);
        const double k = va * exp(-0.5 * sq);
        double s = 0.0;
        for (int j0 = 0; j0 < m; j0 += kSelectStage) {
            const int nj = (m - j0 < kSelectStage) ? m - j0 : kSelectStage;
            wave_lds_sync();                                       // the strip's last contents are consumed
            if (lane < nj) lp[a][lane] = La[(size_t)(j0 + lane) * N + p];
            wave_lds_sync();
            if (valid) {
                const double* col = La + (size_t)j0 * N + i;
#pragma unroll 8
                for (int jj = 0; jj < nj; ++jj) s = fma(col[(size_t)jj * N], lp[a][jj], s);
            }
        }
        c = (k - s) / sqrt(dp);
        di -= c * c;
    }
    if (valid) {
        La[(size_t)m * N + i] = c;
        dnew[i] = di;
    }
    sc[a][lane] = valid ? (di < 0.0 ? 0.0 : di) / va : 0.0;
    __syncthreads();

    // -- the tile's scores, partial trace and record
    if (a == 0) {
        double s = 0.0;
        for (int b = 0; b < D; ++b) s += sc[b][lane];
        int pk = 1;
        if (valid) {
            pk = (m == 0) ? 0 : g.picked[i];
            if (i == p) pk = 1;
            g.picked[i] = pk;
        }
        const double tr = wave_xor_sum(s);
        double bk = (!pk && isfinite(s)) ? s : -INFINITY;
        int bi = pk ? INT_MAX : (int)i;
        for (int off = 32; off >= 1; off >>= 1) {
            const double ok = __shfl_xor(bk, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            take_better(bk, bi, ok, oi);
        }
        if (lane == 0) {
            g.tpart[(size_t)m * T + tile] = tr;
            g.rec_score[(size_t)(m & 1) * T + tile] = bk;
            g.rec_index[(size_t)(m & 1) * T + tile] = bi;
        }
    }
}

// idx, Z = X[idx] (bit for bit) and trace[m] = the tile traces of step m summed in ascending order: a thread per step
__global__ __launch_bounds__(256) void select_finish_kernel(SelectArgs g, int* __restrict__ idx_out, double* __restrict__ Z_out,
                                                            double* __restrict__ trace_out) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= g.M) return;
    const int p = g.picks[m];
    idx_out[m] = p;
    if (Z_out)
        for (int e = 0; e < g.E; ++e) Z_out[(size_t)m * g.E + e] = g.X[(size_t)p * g.E + e];
    if (trace_out) {
        double t = 0.0;
        for (int k = 0; k < g.tiles; ++k) t += g.tpart[(size_t)m * g.tiles + k];
        trace_out[m] = t;
    }
}

}  // namespace

// gpmpc_select_inducing (validated by the entry point: pointers, 1 <= M <= N, jitter_rel, D and E within the compiled limits).
// Touches nothing of the cached model: its only buffer is h->selws.
int run_select_inducing(Handle* h, const double* X, int N, int M, const double* ls, const double* os, double jitter_rel, int D, int E,
                        int* idx_out, double* Z_out, double* trace_out, hipStream_t s) {
    SelectPlan sp;
    const unsigned long long max_mb = h->opt_select_max_mb > 0 ? (unsigned long long)h->opt_select_max_mb : kSelectDefaultMaxMb;
    if (!plan_select_inducing(N, M, D, max_mb, sp)) {
        char msg[256];
        if (sp.bytes == ~0ULL)
            snprintf(msg, sizeof msg, "select_inducing: the workspace of N = %d, M = %d, D = %d does not fit 64 bits", N, M, D);
        else
            snprintf(msg, sizeof msg, "select_inducing: the workspace of N = %d, M = %d, D = %d is %.1f MiB (D M N doubles of the "
                     "partial factors), beyond the cap of %llu MiB (option \"select_inducing_max_mb\")", N, M, D,
                     (double)sp.bytes / 1048576.0, max_mb);
        h->err = msg;
        return GPMPC_ERR_LIMIT;
    }
    int rc;
    if ((rc = grow(h, h->selws, sp.total))) return rc;
    double* ws = h->selws.p;
    SelectArgs g;
    g.X = X; g.ls = ls; g.os = os; g.jitter_rel = jitter_rel;
    g.N = N; g.M = M; g.D = D; g.E = E; g.tiles = sp.tiles;
    g.L = ws + sp.L; g.d = ws + sp.d; g.tpart = ws + sp.tpart; g.rec_score = ws + sp.rec_score;
    g.rec_index = reinterpret_cast<int*>(ws + sp.rec_index);
    g.picks = reinterpret_cast<int*>(ws + sp.picks);
    g.picked = reinterpret_cast<int*>(ws + sp.picked);
    for (int m = 0; m < M; ++m) hipLaunchKernelGGL(select_step_kernel, dim3(sp.tiles), dim3(64 * D), 0, s, g, m);
    hipLaunchKernelGGL(select_finish_kernel, dim3((M + 255) / 256), dim3(256), 0, s, g, idx_out, Z_out, trace_out);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

}  // namespace gpmpc_hip
