// prepare_sparse.hip -- kernels of gpmpc_prepare_sparse for gfx950 (MI355X, CDNA4): a sparse GP in the DTC / projected-process form
// (Quinonero-Candela & Rasmussen 2005, section 5; Seeger et al. 2003) on M inducing inputs Z, built from the N memory points
// without anything of size N x N or M x N.  Per output a (sigma2_a, n_a: outputscale and noise):
//   Kuu = k_a(Z, Z) + jitter_rel sigma2_a I,  Lu = chol(Kuu),  Yu = Lu^-1         (the factorisation launchers of prepare.hip)
//   V   = Yu k_a(Z, X)                        one chunk of points at a time: panel kernel here, then the tiled product
//   G   = V V^T,  w = V y_a                   accumulated over the chunks here
//   B   = I + G / n_a,  LB = chol(B),  Yb = LB^-1
//   beta_eff = Yu^T Yb^T Yb w / n_a,   iK_eff = Yu^T (I - Yb^T Yb) Yu             (the bracket first; lower tiles, mirrored on store)
// Each point's column of the cross-Gram is whitened BEFORE the rank update: no M x M product of unwhitened cross-Grams is ever
// reduced (DESIGN.md 4.4.2 has the conditioning measurements behind that order).  Every sum runs in an order fixed by N, M, D and E:
// the accumulators of G and w travel through memory between chunks and pick up where the chunk before left them (chunks are
// multiples of 64 points, so the k-groups of the matrix instruction and the lanes of w sit at the same absolute point indices
// whatever the chunk size is), no atomics.  The driver (run_prepare_sparse) is in prepare.hip beside the launchers it shares.
#include "device_common.h"
#include "prepare_sparse_plan.h"

namespace gpmpc_hip {

namespace {

constexpr int TS = 64;            // tile edge
constexpr int KC = 32;            // k-slice
constexpr int SI = KC + 2;        // LDS stride, i-major tiles (rows x k)
constexpr int SK = TS + 16;       // LDS stride, k-major tiles (k x columns)

// jitter_rel * outputscale_a: what the Gram kernels of prepare.hip add to the diagonal in the place of the noise
__global__ void sparse_jitter_kernel(const double* __restrict__ os, double jitter_rel, int D, double* __restrict__ jit) {
    if ((int)threadIdx.x < D) jit[threadIdx.x] = jitter_rel * os[threadIdx.x];
}

// Kuf[a][k][c] = sigma2_a exp(-1/2 sum_e ((z_ke - x_ne) / l_ae)^2), n = n0 + c, for one chunk of points: 64 x 64 tiles, lane =
// point (its x_n / l_a in registers), the 16 inducing rows a thread visits read z_k / l_a as LDS broadcasts -- the arithmetic of
// gram_kernel (differences per element, libm's exp).  Columns of points past N are written as zeros.
template <int EP>
__global__ __launch_bounds__(256) void sparse_panel_kernel(const double* __restrict__ Zt, const double* __restrict__ X,
                                                           const double* __restrict__ ils2, const double* __restrict__ var,
                                                           int M, int N, int E, int n0, int Cs, double* __restrict__ Kuf) {
    __shared__ double zi[64][EP + 1];
    const int a = blockIdx.z;
    const int k0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double il[EP];
#pragma unroll
    for (int e = 0; e < EP; ++e) il[e] = (e < E) ? sqrt(ils2[a * E + e]) : 0.0;
    for (int idx = threadIdx.x; idx < 64 * EP; idx += 256) {
        const int r = idx / EP, e = idx - r * EP;
        const int k = k0 + r;
        zi[r][e] = (e < E && k < M) ? Zt[(size_t)e * M + k] * sqrt(ils2[a * E + e]) : 0.0;
    }
    const long long n = (long long)n0 + c0 + lane;
    double xj[EP];
#pragma unroll
    for (int e = 0; e < EP; ++e) xj[e] = (e < E && n < N) ? X[(size_t)n * E + e] * il[e] : 0.0;
    __syncthreads();
    const double va = var[a];
    double* Ka = Kuf + (size_t)a * M * Cs;
#pragma unroll 4
    for (int rr = 0; rr < 16; ++rr) {
        const int r = wave * 16 + rr;
        double s = 0.0;
#pragma unroll
        for (int e = 0; e < EP; ++e) { const double d = zi[r][e] - xj[e]; s = fma(d, d, s); }
        const double v = va * exp(-0.5 * s);
        if (k0 + r < M) Ka[(size_t)(k0 + r) * Cs + c0 + lane] = (n < N) ? v : 0.0;
    }
}

// G[a] += V[a] V[a]^T over the cn points of the chunk, 64 x 64 tiles of the lower tile triangle (whole diagonal tiles: both of
// their halves see the same products in the same order, so G stays exactly symmetric there).  Both operands are rows of V:
// i-major staging as in syrk_outer_kernel.  The accumulators START from G, so the sum over the points is one chain in point order.
__global__ __launch_bounds__(256) void sparse_syrk_acc_kernel(const double* __restrict__ Vall, int M, int Cs, int cn,
                                                              double* __restrict__ Gall) {
    __shared__ double As[TS * SI];
    __shared__ double Bs[TS * SI];
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj > ti) return;
    const double* V = Vall + (size_t)blockIdx.z * M * Cs;
    double* G = Gall + (size_t)blockIdx.z * M * M;
    const int i0 = ti * TS, j0 = tj * TS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
    const int srow = tid >> 5, sk = tid & 31;
    d4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i0 + wi + 16 * x + lk + 4 * r, col = j0 + wj + 16 * y + li;
                acc[x][y][r] = (row < M && col < M) ? G[(size_t)row * M + col] : 0.0;
            }
    double av[8], bv[8];
    auto fetch = [&](int p0) {
        const bool kin = (p0 + sk < cn);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int row = 8 * u + srow;
            const int ra = (i0 + row < M) ? i0 + row : M - 1, rb = (j0 + row < M) ? j0 + row : M - 1;
            av[u] = kin ? V[(size_t)ra * Cs + p0 + sk] : 0.0;
            bv[u] = kin ? V[(size_t)rb * Cs + p0 + sk] : 0.0;
        }
    };
    fetch(0);
    for (int p0 = 0; p0 < cn; p0 += KC) {
        __syncthreads();                                             // previous slice consumed
#pragma unroll
        for (int u = 0; u < 8; ++u) { As[(8 * u + srow) * SI + sk] = av[u]; Bs[(8 * u + srow) * SI + sk] = bv[u]; }
        __syncthreads();
        if (p0 + KC < cn) fetch(p0 + KC);                            // next slice travels while this one is multiplied
#pragma unroll
        for (int kk = 0; kk < KC; kk += 4) {
            const double a0 = As[(wi + li) * SI + kk + lk], a1 = As[(wi + 16 + li) * SI + kk + lk];
            const double b0 = Bs[(wj + li) * SI + kk + lk], b1 = Bs[(wj + 16 + li) * SI + kk + lk];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i0 + wi + 16 * x + lk + 4 * r, col = j0 + wj + 16 * y + li;
                if (row < M && col < M) G[(size_t)row * M + col] = acc[x][y][r];
            }
}

// w = V y: a wavefront per (output, inducing point), lane l adds the points n = l (mod 64) of the chunk to its partial sum, which
// travels through wpart (D, M, 64) between chunks
__global__ __launch_bounds__(256) void sparse_wacc_kernel(const double* __restrict__ Vall, const double* __restrict__ Y, int M, int Cs,
                                                          int n0, int cn, int D, double* __restrict__ wpart) {
    const int a = blockIdx.y;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= M) return;
    const double* v = Vall + ((size_t)a * M + i) * Cs;
    double acc = wpart[((size_t)a * M + i) * kSparseLanes + lane];
    for (int c = lane; c < cn; c += 64) acc = fma(v[c], Y[((size_t)n0 + c) * D + a], acc);
    wpart[((size_t)a * M + i) * kSparseLanes + lane] = acc;
}

// ... and the 64 partial sums in lane order
__global__ __launch_bounds__(256) void sparse_wreduce_kernel(const double* __restrict__ wpart, int n, double* __restrict__ w) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    double s = 0.0;
    for (int l = 0; l < kSparseLanes; ++l) s += wpart[(size_t)idx * kSparseLanes + l];
    w[idx] = s;
}

// B = I + G / n_a, the full symmetric matrix from the lower triangle of G
__global__ __launch_bounds__(256) void sparse_bmat_kernel(const double* __restrict__ Gall, const double* __restrict__ noise, int M,
                                                          double* __restrict__ Ball) {
    const int a = blockIdx.z, i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const int hi = i > j ? i : j, lo = i > j ? j : i;
    const double g = Gall[((size_t)a * M + hi) * M + lo] / noise[a];
    Ball[((size_t)a * M + i) * M + j] = (i == j) ? 1.0 + g : g;
}

// out = Y x (trans = 0) or Y^T x (trans = 1) of a lower-triangular Y (D, M, M), one thread per (output, row), the sum in index
// order; `div` (D) or NULL: the result divided by div[a]
__global__ __launch_bounds__(256) void sparse_trmv_kernel(const double* __restrict__ Yall, const double* __restrict__ x, int M, int trans,
                                                          const double* __restrict__ div, double* __restrict__ out) {
    const int a = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const double* Y = Yall + (size_t)a * M * M;
    const double* xa = x + (size_t)a * M;
    double s = 0.0;
    if (trans) for (int p = i; p < M; ++p) s = fma(Y[(size_t)p * M + i], xa[p], s);
    else for (int k = 0; k <= i; ++k) s = fma(Y[(size_t)i * M + k], xa[k], s);
    out[(size_t)a * M + i] = div ? s / div[a] : s;
}

// C = A^T B (ident_minus: I - A^T B) for a lower-triangular A (A[p][c] = 0 for p < c) and a B for which the product is symmetric
// (B = A, or B = S A with S symmetric): 64 x 64 tiles of the lower triangle, mirrored on store -- exactly symmetric.  Both
// operands are columns: k-major staging as in syrk_inverse_tiled_kernel.
__global__ __launch_bounds__(256) void sparse_atb_sym_kernel(const double* __restrict__ Aall, const double* __restrict__ Ball, int M,
                                                             double* __restrict__ Call, int ident_minus) {
    __shared__ double As[KC * SK];
    __shared__ double Bs[KC * SK];
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj > ti) return;
    const double* A = Aall + (size_t)blockIdx.z * M * M;
    const double* B = Ball + (size_t)blockIdx.z * M * M;
    double* C = Call + (size_t)blockIdx.z * M * M;
    const int i0 = ti * TS, j0 = tj * TS;                            // j0 <= i0
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
    const int sp = tid >> 6, scol = tid & 63;
    d4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = {0.0, 0.0, 0.0, 0.0};
    double av[8], bv[8];
    auto fetch = [&](int p0) {
        const int ci = i0 + scol, cj = j0 + scol;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int p = p0 + 4 * u + sp;
            av[u] = (p < M && ci < M) ? A[(size_t)p * M + ci] : 0.0;
            bv[u] = (p < M && cj < M) ? B[(size_t)p * M + cj] : 0.0;
        }
    };
    fetch(i0);
    for (int p0 = i0; p0 < M; p0 += KC) {                            // rows p < i0 of the A columns are zero
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 8; ++u) { As[(4 * u + sp) * SK + scol] = av[u]; Bs[(4 * u + sp) * SK + scol] = bv[u]; }
        __syncthreads();
        if (p0 + KC < M) fetch(p0 + KC);
#pragma unroll
        for (int kk = 0; kk < KC; kk += 4) {
            const double a0 = As[(kk + lk) * SK + wi + li], a1 = As[(kk + lk) * SK + wi + 16 + li];
            const double b0 = Bs[(kk + lk) * SK + wj + li], b1 = Bs[(kk + lk) * SK + wj + 16 + li];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i0 + wi + 16 * x + lk + 4 * r, col = j0 + wj + 16 * y + li;
                if (row < M && col <= row) {
                    double v = acc[x][y][r];
                    if (ident_minus) v = (row == col ? 1.0 : 0.0) - v;
                    C[(size_t)row * M + col] = v;
                    if (row != col) C[(size_t)col * M + row] = v;
                }
            }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// Launchers (the driver in prepare.hip strings them together with the factorisation's)
int launch_sparse_jitter(Handle* h, const double* os, double jitter_rel, int D, double* jit, hipStream_t s) {
    hipLaunchKernelGGL(sparse_jitter_kernel, dim3(1), dim3(64), 0, s, os, jitter_rel, D, jit);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

// Kuf of the points [n0, n0 + cn) into kuf (D, M, Cs): the columns up to cn rounded up to 64 are written (zeros past N)
int launch_sparse_panel(Handle* h, const double* X, int N, int M, int D, int E, int n0, int cn, int Cs, double* kuf, hipStream_t s) {
    const dim3 grid((cn + 63) / 64, (M + 63) / 64, D);
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, h->Xt.p, X, h->ils2.p, h->var.p, M, N, E, n0, Cs, kuf); };
    if (E <= 4) go(sparse_panel_kernel<4>);
    else if (E <= 8) go(sparse_panel_kernel<8>);
    else if (E <= 16) go(sparse_panel_kernel<16>);
    else go(sparse_panel_kernel<24>);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

// G += V V^T and the partial sums of w += V y over the cn points of the chunk that starts at point n0
int launch_sparse_accumulate(Handle* h, const double* v, const double* Y, int M, int D, int n0, int cn, int Cs, double* G,
                             double* wpart, hipStream_t s) {
    const int nt = (M + TS - 1) / TS;
    hipLaunchKernelGGL(sparse_syrk_acc_kernel, dim3(nt, nt, D), dim3(256), 0, s, v, M, Cs, cn, G);
    hipLaunchKernelGGL(sparse_wacc_kernel, dim3((M + 3) / 4, D), dim3(256), 0, s, v, Y, M, Cs, n0, cn, D, wpart);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

// B = I + G / n into Bm (D, M, M), w (D, M) from its partial sums
int launch_sparse_bmat(Handle* h, const double* G, const double* wpart, const double* noise, int M, int D, double* Bm, double* w,
                       hipStream_t s) {
    hipLaunchKernelGGL(sparse_bmat_kernel, dim3((M + 255) / 256, M, D), dim3(256), 0, s, G, noise, M, Bm);
    hipLaunchKernelGGL(sparse_wreduce_kernel, dim3((D * M + 255) / 256), dim3(256), 0, s, wpart, D * M, w);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

// beta_eff = Yu^T Yb^T Yb w / n  (t1, t2: (D, M) scratch)
int launch_sparse_beta(Handle* h, const double* Yu, const double* Yb, const double* w, const double* noise, int M, int D, double* t1,
                       double* t2, double* beta, hipStream_t s) {
    const dim3 grid((M + 255) / 256, D);
    hipLaunchKernelGGL(sparse_trmv_kernel, grid, dim3(256), 0, s, Yb, w, M, 0, (const double*)nullptr, t1);
    hipLaunchKernelGGL(sparse_trmv_kernel, grid, dim3(256), 0, s, Yb, (const double*)t1, M, 1, (const double*)nullptr, t2);
    hipLaunchKernelGGL(sparse_trmv_kernel, grid, dim3(256), 0, s, Yu, (const double*)t2, M, 1, noise, beta);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

// C = A^T B, or I - A^T B, exactly symmetric (see sparse_atb_sym_kernel)
int launch_sparse_atb_sym(Handle* h, const double* A, const double* B, int M, int D, double* C, bool ident_minus, hipStream_t s) {
    const int nt = (M + TS - 1) / TS;
    hipLaunchKernelGGL(sparse_atb_sym_kernel, dim3(nt, nt, D), dim3(256), 0, s, A, B, M, C, ident_minus ? 1 : 0);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

}  // namespace gpmpc_hip
