// predict.hip -- GP posterior at deterministic query inputs (gpmpc_predict):
//   mean_a(x*) = k_a(x*)^T beta_a,   var_a(x*) = sigma2_a - k_a(x*)^T iK_a k_a(x*)   (+ noise_a)
// with k_a(x*)_i = sigma2_a exp(-1/2 sum_e (x*_e - x_ie)^2 / l_ae^2), from the cached Xt / ils2 / var / beta / iK.
//
// Structure ("Posterior prediction at query points"):
//   predict_tile_kernel   one workgroup per (64 query rows, 256-column block of iK_a, output a).  The k loop walks the
//                         memory points i in steps of 16: it builds the 64 x 16 tile of K*_a on the fly (never stored in
//                         global memory) and stages the 16 x 256 tile of iK_a in LDS; P = K*_a iK_a accumulates on
//                         v_mfma_f64_16x16x4_f64.  The epilogue rebuilds K*_a at the block's 256 columns and forms, per
//                         query row, the partial sums  sum_j P_mj K*_mj  and  sum_j K*_mj beta_j  of the block.
//   predict_finish_kernel adds the column blocks' partials of a row in block order and writes mean / var.
// Every sum of a row runs in an order fixed by N alone (k steps, lanes, waves, column blocks): a point's bits do not depend on
// M, on its place in the batch or on the other points.  No atomics.  M is processed in chunks of Mc rows so the workspace
// (2 D nCB Mc doubles) stays within kWsBudget.  Without var_out the k loop is compiled out (the mean is a GEMV).
//
// gpmpc_predict_backward ("Gradients of posterior prediction") reuses the grid and the k loop:
//   predict_backward_tile_kernel   forms P = K*_a iK_a as above (compiled out without var_bar), then per 64-column slice stages
//                                  c.k = (mean_bar beta_j - 2 var_bar P_mj) K*_mj in LDS and contracts it against (x_je - x*_me),
//                                  one thread per (row, input e) pair walking the slice's columns in order.
//   predict_backward_finish_kernel adds the column blocks in block order, then the outputs a in order, each scaled by ils2_ae.
// The same invariance: every sum runs in an order fixed by N, E and D; no atomics; workspace D nCB Mc E doubles.
#include "device_common.h"

namespace gpmpc_hip {

namespace {

constexpr int kBM = 64;                  // query rows per workgroup
constexpr int kBN = 256;                 // columns of iK per workgroup (64 per wave)
constexpr int kBK = 16;                  // memory points per k step
constexpr int kAPitch = kBM + 16;        // LDS row pitch (doubles) of the K* tile, stored [k][row]: rows 32 banks apart
constexpr int kBPitch = kBN + 16;        // ... and of the iK tile [k][column]
constexpr size_t kWsBudget = (size_t)4 << 20;   // bytes of partial sums per chunk

struct PredictArgs {
    const double* Xq;        // (M, E) query inputs, this chunk's first row
    const double* Xt;        // (E, N)
    const double* ils2;      // (D, E)
    const double* var;       // (D)
    const double* beta;      // (D, N)
    const double* iK;        // (D, N, N)
    double* part;            // (2, D, nCB, Mc): sum_j P K* | sum_j K* beta
    double* mean_out;        // (M, D) of this chunk, or NULL
    double* var_out;         // (M, D) of this chunk, or NULL
    int rows, N, E, D, nCB, Mc;
    int with_noise;
    double noise[kMaxD];
};

template <int EP>
__device__ inline double kstar(const double* xq, const double (&xi)[EP], const double (&il)[EP], double sig2) {
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < EP; ++e) {
        const double d = xq[e] - xi[e];
        s = fma(d * d, il[e], s);
    }
    return sig2 * exp(-0.5 * s);
}

// P = K*_a iK_a for the workgroup's 64 rows and 256 columns (acc: the f64 MFMA C/D layout, see the epilogues).  The k loop walks
// the memory points in steps of kBK: it builds the 64 x 16 tile of K*_a on the fly into s_A and stages the 16 x 256 tile of iK_a in
// s_B; the next iK tile is loaded under the MFMAs.  The k loop of predict_tile_kernel, which keeps its own copy so that the
// forward's code is unchanged; both form P with the same operations in the same order.
template <int EP>
__device__ inline void kstar_ik_product(const double* Xt, const double* iKa, int N, int E, int j0, const double (&il)[EP],
                                        double sig2, const double (&s_xq)[kBM][EP + 1], double (&s_A)[kBK][kAPitch],
                                        double (&s_B)[kBK][kBPitch], d4 (&acc)[4][4]) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // staging map: K* element (row gr + 16 q, point gi); iK elements (row bk, columns bc + 16 q)
    const int gi = tid & 15, gr = tid >> 4;
    const int bk = tid >> 4, bc = tid & 15;
    const int nk = (N + kBK - 1) / kBK;
    double breg[16];
    auto load_b = [&](int i0) {
        const int i = i0 + bk;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int j = j0 + bc + 16 * q;
            breg[q] = (i < N && j < N) ? iKa[(size_t)i * N + j] : 0.0;
        }
    };
    load_b(0);
    for (int ks = 0; ks < nk; ++ks) {
        const int i0 = ks * kBK;
        __syncthreads();                         // the previous step's MFMAs have read s_A / s_B
#pragma unroll
        for (int q = 0; q < 16; ++q) s_B[bk][bc + 16 * q] = breg[q];
        {
            const int i = i0 + gi;
            double xi[EP];
#pragma unroll
            for (int e = 0; e < EP; ++e) xi[e] = (e < E && i < N) ? Xt[(size_t)e * N + i] : 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = gr + 16 * q;
                s_A[gi][r] = (i < N) ? kstar<EP>(s_xq[r], xi, il, sig2) : 0.0;
            }
        }
        __syncthreads();
        if (ks + 1 < nk) load_b(i0 + kBK);       // next iK tile in flight under the MFMAs
#pragma unroll
        for (int s = 0; s < kBK / 4; ++s) {
            const int k = 4 * s + (lane >> 4);
            double av[4], bv[4];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) av[rt] = s_A[k][16 * rt + (lane & 15)];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) bv[ct] = s_B[k][64 * w + 16 * ct + (lane & 15)];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
                    acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[rt], bv[ct], acc[rt][ct], 0, 0, 0);
        }
    }
}

template <int EP, bool VAR>
__global__ __launch_bounds__(256) void predict_tile_kernel(PredictArgs p) {
    __shared__ double s_xq[kBM][EP + 1];
    __shared__ double s_red[2][4][kBM];
    __shared__ double s_A[VAR ? kBK : 1][VAR ? kAPitch : 1];
    __shared__ double s_B[VAR ? kBK : 1][VAR ? kBPitch : 1];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int m0 = blockIdx.x * kBM;                 // first row of the tile (within the chunk)
    const int cb = blockIdx.y, j0 = cb * kBN;
    const int a = blockIdx.z;
    const int N = p.N, E = p.E;
    const double sig2 = p.var[a];
    double il[EP];
#pragma unroll
    for (int e = 0; e < EP; ++e) il[e] = (e < E) ? p.ils2[a * E + e] : 0.0;
    for (int idx = tid; idx < kBM * EP; idx += 256) {
        const int r = idx / EP, e = idx - r * EP;
        s_xq[r][e] = (e < E && m0 + r < p.rows) ? p.Xq[(size_t)(m0 + r) * E + e] : 0.0;
    }
    __syncthreads();

    d4 acc[4][4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = d4{0.0, 0.0, 0.0, 0.0};

    if constexpr (VAR) {
        const double* iKa = p.iK + (size_t)a * N * N;
        // staging map: K* element (row gr + 16 q, point gi); iK elements (row bk, columns bc + 16 q)
        const int gi = tid & 15, gr = tid >> 4;
        const int bk = tid >> 4, bc = tid & 15;
        const int nk = (N + kBK - 1) / kBK;
        double breg[16];
        auto load_b = [&](int i0) {
            const int i = i0 + bk;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int j = j0 + bc + 16 * q;
                breg[q] = (i < N && j < N) ? iKa[(size_t)i * N + j] : 0.0;
            }
        };
        load_b(0);
        for (int ks = 0; ks < nk; ++ks) {
            const int i0 = ks * kBK;
            __syncthreads();                         // the previous step's MFMAs have read s_A / s_B
#pragma unroll
            for (int q = 0; q < 16; ++q) s_B[bk][bc + 16 * q] = breg[q];
            {
                const int i = i0 + gi;
                double xi[EP];
#pragma unroll
                for (int e = 0; e < EP; ++e) xi[e] = (e < E && i < N) ? p.Xt[(size_t)e * N + i] : 0.0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int r = gr + 16 * q;
                    s_A[gi][r] = (i < N) ? kstar<EP>(s_xq[r], xi, il, sig2) : 0.0;
                }
            }
            __syncthreads();
            if (ks + 1 < nk) load_b(i0 + kBK);       // next iK tile in flight under the MFMAs
#pragma unroll
            for (int s = 0; s < kBK / 4; ++s) {
                const int k = 4 * s + (lane >> 4);
                double av[4], bv[4];
#pragma unroll
                for (int rt = 0; rt < 4; ++rt) av[rt] = s_A[k][16 * rt + (lane & 15)];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) bv[ct] = s_B[k][64 * w + 16 * ct + (lane & 15)];
#pragma unroll
                for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct)
                        acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[rt], bv[ct], acc[rt][ct], 0, 0, 0);
            }
        }
    }

    // epilogue: f64 C/D layout -- acc[rt][ct][r] = P[16 rt + (lane >> 4) + 4 r][64 w + 16 ct + (lane & 15)]
    double rd[4][4], mn[4][4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) rd[rt][r] = mn[rt][r] = 0.0;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const int j = j0 + 64 * w + 16 * ct + (lane & 15);
        if (j < N) {                                  // columns past N contribute nothing (P there is 0 as well)
            double xj[EP];
#pragma unroll
            for (int e = 0; e < EP; ++e) xj[e] = (e < E) ? p.Xt[(size_t)e * N + j] : 0.0;
            const double bj = p.beta[(size_t)a * N + j];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double k = kstar<EP>(s_xq[16 * rt + (lane >> 4) + 4 * r], xj, il, sig2);
                    if constexpr (VAR) rd[rt][r] = fma(acc[rt][ct][r], k, rd[rt][r]);
                    mn[rt][r] = fma(k, bj, mn[rt][r]);
                }
        }
    }
    // the 16 lanes of a row (lane & 15), then the 4 waves in order
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) {
                if constexpr (VAR) rd[rt][r] += __shfl_xor(rd[rt][r], off, 64);
                mn[rt][r] += __shfl_xor(mn[rt][r], off, 64);
            }
            if ((lane & 15) == 0) {
                const int row = 16 * rt + (lane >> 4) + 4 * r;
                s_red[0][w][row] = VAR ? rd[rt][r] : 0.0;
                s_red[1][w][row] = mn[rt][r];
            }
        }
    __syncthreads();
    if (tid < 2 * kBM) {
        const int which = tid / kBM, row = tid - which * kBM;
        if (m0 + row < p.rows) {
            const double v = ((s_red[which][0][row] + s_red[which][1][row]) + s_red[which][2][row]) + s_red[which][3][row];
            p.part[(((size_t)which * p.D + a) * p.nCB + cb) * p.Mc + m0 + row] = v;
        }
    }
}

__global__ __launch_bounds__(256) void predict_finish_kernel(PredictArgs p) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.rows * p.D) return;
    const int m = idx / p.D, a = idx - m * p.D;
    const double* pv = p.part + (size_t)a * p.nCB * p.Mc + m;
    const double* pm = p.part + ((size_t)p.D + a) * p.nCB * p.Mc + m;
    double sv = 0.0, sm = 0.0;
    for (int cb = 0; cb < p.nCB; ++cb) {
        sv += pv[(size_t)cb * p.Mc];
        sm += pm[(size_t)cb * p.Mc];
    }
    if (p.mean_out) p.mean_out[idx] = sm;
    if (p.var_out) {
        double v = p.var[a] - sv;                     // not clamped (gp_model.py:112-180 at zero input variance)
        if (p.with_noise) v += p.noise[a];
        p.var_out[idx] = v;
    }
}

template <int EP>
void launch_tiles(const PredictArgs& p, dim3 grid, bool var, hipStream_t s) {
    if (var) hipLaunchKernelGGL((predict_tile_kernel<EP, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((predict_tile_kernel<EP, false>), grid, dim3(256), 0, s, p);
}

// ---- gpmpc_predict_backward: d/dx* of <mean_bar, mean> + <var_bar, var> --------------------------------------------------------
// With c_amj = mean_bar_ma beta_aj - 2 var_bar_ma P_amj (P = K*_a iK_a, iK_a taken as symmetric):
//   Xq_bar_me = sum_a ils2_ae sum_j c_amj k_amj (x_je - x*_me)
// The differences are formed per element: the factored form sum_j c k x_j - x* sum_j c k cancels digits with a time input.

constexpr int kSlice = 64;               // columns of c.k staged in LDS at a time (16 per wave)
constexpr int kCkPitch = kBM + 2;        // LDS pitch (doubles) of s_ck [column][row]: 32 lanes of a write hit distinct banks

struct PredictBackwardArgs {
    const double* Xq;        // (M, E) query inputs, this chunk's first row
    const double* Xt;        // (E, N)
    const double* ils2;      // (D, E)
    const double* var;       // (D)
    const double* beta;      // (D, N)
    const double* iK;        // (D, N, N)
    const double* mean_bar;  // (M, D) of this chunk, or NULL (= 0)
    const double* var_bar;   // (M, D) of this chunk, or NULL (= 0)
    double* part;            // (D, nCB, Mc, E): sum_j c k (x_j - x*) of a column block
    double* out;             // (M, E) of this chunk
    int rows, N, E, D, nCB, Mc;
};

// Grid and k loop of predict_tile_kernel.  Epilogue, per slice of 64 columns: every lane forms c.k for its 16 rows x 1 column
// into s_ck and the slice's x_j into s_xj; then each thread owns one row and the inputs e = w + 4 q and walks the slice's
// columns in order.  s_ck reuses the k loop's s_A / s_B.
template <int EP, bool VAR>
__global__ __launch_bounds__(256) void predict_backward_tile_kernel(PredictBackwardArgs p) {
    constexpr int kLoop = kBK * kAPitch + kBK * kBPitch;
    constexpr int kMem = (VAR && kLoop > kSlice * kCkPitch) ? kLoop : kSlice * kCkPitch;
    constexpr int kQ = EP / 4;                       // inputs per thread in the contraction
    __shared__ double s_xq[kBM][EP + 1];
    __shared__ double s_xj[kSlice][EP + 1];
    __shared__ double s_mb[kBM], s_vb[kBM];          // mean_bar, -2 var_bar of the tile's rows
    __shared__ double s_mem[kMem];
    double (*s_ck)[kCkPitch] = reinterpret_cast<double (*)[kCkPitch]>(s_mem);

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int m0 = blockIdx.x * kBM;
    const int cb = blockIdx.y, j0 = cb * kBN;
    const int a = blockIdx.z;
    const int N = p.N, E = p.E, D = p.D;
    const double sig2 = p.var[a];
    double il[EP];
#pragma unroll
    for (int e = 0; e < EP; ++e) il[e] = (e < E) ? p.ils2[a * E + e] : 0.0;
    for (int idx = tid; idx < kBM * EP; idx += 256) {
        const int r = idx / EP, e = idx - r * EP;
        s_xq[r][e] = (e < E && m0 + r < p.rows) ? p.Xq[(size_t)(m0 + r) * E + e] : 0.0;
    }
    if (tid < kBM) {
        const bool in = m0 + tid < p.rows;
        s_mb[tid] = (in && p.mean_bar) ? p.mean_bar[(size_t)(m0 + tid) * D + a] : 0.0;
        s_vb[tid] = (in && p.var_bar) ? -2.0 * p.var_bar[(size_t)(m0 + tid) * D + a] : 0.0;
    }
    __syncthreads();

    d4 acc[4][4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = d4{0.0, 0.0, 0.0, 0.0};
    if constexpr (VAR) {
        auto& s_A = *reinterpret_cast<double (*)[kBK][kAPitch]>(s_mem);
        auto& s_B = *reinterpret_cast<double (*)[kBK][kBPitch]>(s_mem + kBK * kAPitch);
        kstar_ik_product<EP>(p.Xt, p.iK + (size_t)a * N * N, N, E, j0, il, sig2, s_xq, s_A, s_B, acc);
    }

    // contraction state: row `crow`, inputs e = w + 4 q
    const int crow = tid & 63;
    double xo[kQ], g[kQ];
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
        xo[q] = s_xq[crow][w + 4 * q];
        g[q] = 0.0;
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        __syncthreads();                             // the k loop's MFMAs / the previous slice's contraction are done
        const int c = 16 * w + (lane & 15);          // this lane's column within the slice
        const int j = j0 + 64 * w + 16 * ct + (lane & 15);
        double xj[EP];
#pragma unroll
        for (int e = 0; e < EP; ++e) xj[e] = (e < E && j < N) ? p.Xt[(size_t)e * N + j] : 0.0;
        if ((lane >> 4) == 0) {
#pragma unroll
            for (int e = 0; e < EP; ++e) s_xj[c][e] = xj[e];
        }
        const double bj = (j < N) ? p.beta[(size_t)a * N + j] : 0.0;
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * rt + (lane >> 4) + 4 * r;
                double ck = 0.0;                     // columns past N contribute nothing
                if (j < N) {
                    const double k = kstar<EP>(s_xq[row], xj, il, sig2);
                    double cc = s_mb[row] * bj;
                    if constexpr (VAR) cc = fma(s_vb[row], acc[rt][ct][r], cc);
                    ck = cc * k;
                }
                s_ck[c][row] = ck;
            }
        __syncthreads();
#pragma unroll 4
        for (int cs = 0; cs < kSlice; ++cs) {
            const double ck = s_ck[cs][crow];
#pragma unroll
            for (int q = 0; q < kQ; ++q) g[q] = fma(ck, s_xj[cs][w + 4 * q] - xo[q], g[q]);
        }
    }
    if (m0 + crow < p.rows) {
        double* dst = p.part + (((size_t)a * p.nCB + cb) * p.Mc + m0 + crow) * E;
#pragma unroll
        for (int q = 0; q < kQ; ++q)
            if (w + 4 * q < E) dst[w + 4 * q] = g[q];
    }
}

// Per (row, e): the column blocks in block order, then the outputs a in order, each scaled by ils2_ae.
__global__ __launch_bounds__(256) void predict_backward_finish_kernel(PredictBackwardArgs p) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.rows * p.E) return;
    const int m = idx / p.E, e = idx - m * p.E;
    double s = 0.0;
    for (int a = 0; a < p.D; ++a) {
        const double* pa = p.part + ((size_t)a * p.nCB * p.Mc + m) * p.E + e;
        double t = 0.0;
        for (int cb = 0; cb < p.nCB; ++cb) t += pa[(size_t)cb * p.Mc * p.E];
        s = fma(p.ils2[a * p.E + e], t, s);
    }
    p.out[idx] = s;
}

template <int EP>
void launch_backward_tiles(const PredictBackwardArgs& p, dim3 grid, bool var, hipStream_t s) {
    if (var) hipLaunchKernelGGL((predict_backward_tile_kernel<EP, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((predict_backward_tile_kernel<EP, false>), grid, dim3(256), 0, s, p);
}

}  // namespace

int run_predict(Handle* h, const double* Xq, int M, const double* noises_host, double* mean_out, double* var_out, hipStream_t s) {
    const int N = h->N, D = h->D, E = h->E;
    if (M == 0 || (!mean_out && !var_out)) return GPMPC_OK;
    const int nCB = (N + kBN - 1) / kBN;
    // rows per chunk: a multiple of the tile height, as many as the workspace budget allows, no more than M needs
    long long Mc = (long long)(kWsBudget / (2 * sizeof(double) * (size_t)D * nCB)) / kBM * kBM;
    if (h->opt_predict_chunk > 0) Mc = h->opt_predict_chunk;
    if (Mc < kBM) Mc = kBM;
    const long long Mneed = ((long long)M + kBM - 1) / kBM * kBM;
    if (Mc > Mneed) Mc = Mneed;
    int rc = grow(h, h->predws, 2 * (size_t)D * nCB * (size_t)Mc);
    if (rc) return rc;
    PredictArgs p{};
    p.Xt = h->Xt.p; p.ils2 = h->ils2.p; p.var = h->var.p; p.beta = h->beta.p; p.iK = h->iK.p;
    p.part = h->predws.p;
    p.N = N; p.E = E; p.D = D; p.nCB = nCB; p.Mc = (int)Mc;
    p.with_noise = noises_host != nullptr;
    for (int a = 0; a < D; ++a) p.noise[a] = noises_host ? noises_host[a] : 0.0;
    const bool var = var_out != nullptr;
    for (long long m0 = 0; m0 < M; m0 += Mc) {
        const int rows = (int)((M - m0) < Mc ? (M - m0) : Mc);
        p.rows = rows;
        p.Xq = Xq + (size_t)m0 * E;
        p.mean_out = mean_out ? mean_out + (size_t)m0 * D : nullptr;
        p.var_out = var_out ? var_out + (size_t)m0 * D : nullptr;
        const dim3 grid((rows + kBM - 1) / kBM, nCB, D);
        if (E <= 4) launch_tiles<4>(p, grid, var, s);
        else if (E <= 8) launch_tiles<8>(p, grid, var, s);
        else if (E <= 16) launch_tiles<16>(p, grid, var, s);
        else launch_tiles<24>(p, grid, var, s);
        hipLaunchKernelGGL(predict_finish_kernel, dim3((rows * D + 255) / 256), dim3(256), 0, s, p);
    }
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

int run_predict_backward(Handle* h, const double* Xq, int M, const double* mean_bar, const double* var_bar, double* Xq_bar,
                         hipStream_t s) {
    const int N = h->N, D = h->D, E = h->E;
    if (M == 0) return GPMPC_OK;
    if (!mean_bar && !var_bar) {                      // a zero upstream: the gradient is zero
        GPMPC_HIP_CHECK(h, hipMemsetAsync(Xq_bar, 0, (size_t)M * E * sizeof(double), s));
        return GPMPC_OK;
    }
    const int nCB = (N + kBN - 1) / kBN;
    // rows per chunk: as run_predict, for a workspace of E partial sums per (output, column block, row)
    long long Mc = (long long)(kWsBudget / (sizeof(double) * (size_t)D * nCB * E)) / kBM * kBM;
    if (h->opt_predict_bwd_chunk > 0) Mc = h->opt_predict_bwd_chunk;
    if (Mc < kBM) Mc = kBM;
    const long long Mneed = ((long long)M + kBM - 1) / kBM * kBM;
    if (Mc > Mneed) Mc = Mneed;
    int rc = grow(h, h->predbws, (size_t)D * nCB * (size_t)Mc * E);
    if (rc) return rc;
    PredictBackwardArgs p{};
    p.Xt = h->Xt.p; p.ils2 = h->ils2.p; p.var = h->var.p; p.beta = h->beta.p; p.iK = h->iK.p;
    p.part = h->predbws.p;
    p.N = N; p.E = E; p.D = D; p.nCB = nCB; p.Mc = (int)Mc;
    const bool var = var_bar != nullptr;
    for (long long m0 = 0; m0 < M; m0 += Mc) {
        const int rows = (int)((M - m0) < Mc ? (M - m0) : Mc);
        p.rows = rows;
        p.Xq = Xq + (size_t)m0 * E;
        p.mean_bar = mean_bar ? mean_bar + (size_t)m0 * D : nullptr;
        p.var_bar = var_bar ? var_bar + (size_t)m0 * D : nullptr;
        p.out = Xq_bar + (size_t)m0 * E;
        const dim3 grid((rows + kBM - 1) / kBM, nCB, D);
        if (E <= 4) launch_backward_tiles<4>(p, grid, var, s);
        else if (E <= 8) launch_backward_tiles<8>(p, grid, var, s);
        else if (E <= 16) launch_backward_tiles<16>(p, grid, var, s);
        else launch_backward_tiles<24>(p, grid, var, s);
        hipLaunchKernelGGL(predict_backward_finish_kernel, dim3((rows * E + 255) / 256), dim3(256), 0, s, p);
    }
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

}  // namespace gpmpc_hip
