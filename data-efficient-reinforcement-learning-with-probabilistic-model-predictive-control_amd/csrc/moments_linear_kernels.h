// moments_linear_kernels.h -- the kernels the linearised family shares (gfx950 / MI355X): moments_linear.hip (gpmpc_moments_linear,
// gpmpc_rollout_linear, gpmpc_rollout_linear_feedback; gpmpc_lqr_gains through run_moments_linear) and
// moments_linear_backward.hip (their three gradients) launch the one copy here, so a trajectory recomputed by a gradient has the
// forward entry's bits because it is the forward entry's code.  See the moments_linear.hip header for the notation.
//   lin_tile_kernel<EP, KLOOP, BWD>   one workgroup per (64 rows, 256-column block of iK_a, output a): P = K*_a iK_a by the k loop
//                                     of predict.hip (K* tile built on the fly, iK tile staged in LDS, the next one loaded under
//                                     the MFMAs; predict.hip and predict_cov.hip keep their own copies), compiled out without
//                                     KLOOP.  The epilogue walks the block in four slices of 64 columns: every lane forms k for
//                                     its 16 rows x 1 column and stages a weight times k in LDS; then each thread owns one row and
//                                     the inputs e = w + 4 q and walks the slice's columns in order.  Forward form: the weight is
//                                     beta_j, P k goes to the row sums, and per row the block leaves
//                                     sum_j P_mj k_mj | sum_j k_mj beta_j | E sums beta_j k_mj (x_je - m_e).  Reverse form (BWD):
//                                     the weight is c_mj, from the row's coefficients M_bar_a | s_a | W[e,a] / l_ae^2 (staged in
//                                     LDS) and P, and the block leaves the E sums  sum_j c k (x_jg - m_g).
//   rollout_linear_init_kernel /      one wavefront per candidate: index 0 of the stored trajectory; step t -> t + 1 after the
//   rollout_linear_step_kernel<FB>    step's tile launch, open loop or (FB) closed loop, keeping the step's M and V for a reverse
//                                     sweep where the caller gives the arrays.
#pragma once
#include "device_common.h"
#include "moments_linear_plan.h"

namespace gpmpc_hip {

namespace {

constexpr int kBM = kLinBM;              // rows per workgroup
constexpr int kBN = kLinBN;              // columns of iK per workgroup (64 per wave)
constexpr int kBK = 16;                  // memory points per k step
constexpr int kAPitch = kBM + 16;        // LDS row pitch (doubles) of the K* tile, stored [k][row]: rows 32 banks apart
constexpr int kBPitch = kBN + 16;        // ... and of the iK tile [k][column]
constexpr int kSlice = 64;               // columns of beta k / c k staged in LDS at a time (16 per wave)
constexpr int kCkPitch = kBM + 2;        // LDS pitch (doubles) of s_ck [column][row]: 32 lanes of a write hit distinct banks

struct LinTileArgs {
    const double* Xq;        // (rows, E) input means of this chunk
    const double* Xt;        // (E, N)
    const double* ils2;      // (D, E)
    const double* var;       // (D)
    const double* beta;      // (D, N)
    const double* iK;        // (D, N, N)
    const double* coef;      // (D, NW, Mc) reverse form: M_bar_a | s_a | E weights W[e,a] / l_ae^2 (forward form: NULL)
    double* part;            // (D, nCB, NW, Mc) forward: sum_j P k | sum_j k beta | E sums; reverse: - | - | E sums
    int rows, N, E, D, nCB, NW;
    long long Mc;
};

struct LinStepArgs {
    const double* part;
    const double* ils2;      // (D, E)
    const double* var;       // (D)
    const double* actions;   // (rows, H, A) of this chunk
    const double* gains;     // closed loop: (H, A, D) of the chunk's first candidate
    long long gain_stride;   // doubles between two candidates' gains (0: one gain sequence shared by all)
    double* mu;              // (rows, H + 1, D) of this chunk
    double* Sig;             // (rows, H + 1, D, D) of this chunk
    double* keepM;           // (rows, H, D) every step's M, or NULL (not kept)
    double* keepV;           // (rows, H, D, D) the state rows of its V [state input][output] (closed loop: (rows, H, D + A, D),
                             // and the action rows), or NULL
    double* Xq;              // (Mc, E) model inputs of the next tile launch
    int E, D, A, H, nCB, NW, t, include_time;
    long long Mc;
    double time0;
    double mu0[kMaxD];       // read by the init kernel
    double S0[kMaxD * kMaxD];
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

// P = K*_a iK_a for the workgroup's 64 rows and 256 columns (acc: the f64 MFMA C/D layout, see the epilogue).  The k loop of
// predict_tile_kernel: the same operations in the same order.
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

// Grid and k loop of predict_tile_kernel.  s_ck reuses the k loop's s_A / s_B.  KLOOP: P = K* iK is formed (forward: the variance
// sum is wanted; reverse: s_a may be non-zero).  BWD: the reverse form.  The forward form's mean and Jacobian sums are the same
// operations with and without KLOOP: they keep their bits when S is not asked for.
template <int EP, bool KLOOP, bool BWD>
__global__ __launch_bounds__(256) void lin_tile_kernel(LinTileArgs p) {
    constexpr int kLoop = kBK * kAPitch + kBK * kBPitch;
    constexpr int kMem = (KLOOP && kLoop > kSlice * kCkPitch) ? kLoop : kSlice * kCkPitch;
    constexpr int kQ = EP / 4;                       // inputs per thread in the contraction
    constexpr int kCfRows = BWD ? kBM : 1;
    __shared__ double s_xq[kBM][EP + 1];
    __shared__ double s_xj[kSlice][EP + 1];
    __shared__ double s_cf[kCfRows][EP + 3];         // reverse form: M_bar_a | s_a | W[e,a] / l_ae^2 of the tile's rows
    __shared__ double s_red[4][kBM];
    __shared__ double s_mem[kMem];
    double (*s_ck)[kCkPitch] = reinterpret_cast<double (*)[kCkPitch]>(s_mem);

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
    if constexpr (BWD) {
        for (int idx = tid; idx < kBM * (EP + 2); idx += 256) {
            const int c = idx / kBM, r = idx - c * kBM;
            s_cf[r][c] = (c < E + 2 && m0 + r < p.rows) ? p.coef[((size_t)a * p.NW + c) * (size_t)p.Mc + m0 + r] : 0.0;
        }
    }
    __syncthreads();

    d4 acc[4][4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = d4{0.0, 0.0, 0.0, 0.0};
    if constexpr (KLOOP) {
        auto& s_A = *reinterpret_cast<double (*)[kBK][kAPitch]>(s_mem);
        auto& s_B = *reinterpret_cast<double (*)[kBK][kBPitch]>(s_mem + kBK * kAPitch);
        kstar_ik_product<EP>(p.Xt, p.iK + (size_t)a * N * N, N, E, j0, il, sig2, s_xq, s_A, s_B, acc);
    }

    // epilogue: f64 C/D layout -- acc[rt][ct][r] = P[16 rt + (lane >> 4) + 4 r][64 w + 16 ct + (lane & 15)]
    [[maybe_unused]] double rd[4][4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) rd[rt][r] = 0.0;
    // contraction state: row `crow`, inputs e = w + 4 q; forward form: wave 0 also sums beta k itself (the mean)
    const int crow = tid & 63;
    double xo[kQ], g[kQ];
    [[maybe_unused]] double mn = 0.0;
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
                double ck = 0.0;                     // columns past N contribute nothing (P there is 0 as well)
                if (j < N) {
                    const double k = kstar<EP>(s_xq[row], xj, il, sig2);
                    if constexpr (BWD) {
                        double u = 0.0;              // sum_e W[e,a] r_aje
#pragma unroll
                        for (int e = 0; e < EP; ++e) u = fma(s_cf[row][2 + e], xj[e] - s_xq[row][e], u);
                        double cc = bj * (s_cf[row][0] + u);
                        if constexpr (KLOOP) cc = fma(-2.0 * s_cf[row][1], acc[rt][ct][r], cc);
                        ck = cc * k;
                    } else {
                        if constexpr (KLOOP) rd[rt][r] = fma(acc[rt][ct][r], k, rd[rt][r]);
                        ck = bj * k;
                    }
                }
                s_ck[c][row] = ck;
            }
        __syncthreads();
#pragma unroll 4
        for (int cs = 0; cs < kSlice; ++cs) {
            const double ck = s_ck[cs][crow];
            if constexpr (!BWD) {
                if (w == 0) mn += ck;
            }
#pragma unroll
            for (int q = 0; q < kQ; ++q) g[q] = fma(ck, s_xj[cs][w + 4 * q] - xo[q], g[q]);
        }
    }
    const size_t rstride = (size_t)p.Mc;
    double* dst = p.part + ((size_t)a * p.nCB + cb) * p.NW * rstride;      // [which][row]
    if (m0 + crow < p.rows) {
        if constexpr (!BWD) {
            if (w == 0) dst[rstride + m0 + crow] = mn;
        }
#pragma unroll
        for (int q = 0; q < kQ; ++q)
            if (w + 4 * q < E) dst[(size_t)(2 + w + 4 * q) * rstride + m0 + crow] = g[q];
    }
    if constexpr (KLOOP && !BWD) {
        // sum_j P k: the 16 lanes of a row (lane & 15), then the 4 waves in order
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int off = 8; off >= 1; off >>= 1) rd[rt][r] += __shfl_xor(rd[rt][r], off, 64);
                if ((lane & 15) == 0) s_red[w][16 * rt + (lane >> 4) + 4 * r] = rd[rt][r];
            }
        __syncthreads();
        if (tid < kBM && m0 + tid < p.rows)
            dst[m0 + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
    }
}

// BWD is a compile-time choice so that a file that launches the forward form only holds no reverse-form kernel.
template <int EP, bool BWD>
void launch_lin_tiles_ep(const LinTileArgs& p, bool kloop, hipStream_t s) {
    const dim3 grid((p.rows + kBM - 1) / kBM, p.nCB, p.D);
    if (kloop) hipLaunchKernelGGL((lin_tile_kernel<EP, true, BWD>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((lin_tile_kernel<EP, false, BWD>), grid, dim3(256), 0, s, p);
}

template <bool BWD>
void launch_lin_tiles(const LinTileArgs& p, bool kloop, hipStream_t s) {
    if (p.E <= 4) launch_lin_tiles_ep<4, BWD>(p, kloop, s);
    else if (p.E <= 8) launch_lin_tiles_ep<8, BWD>(p, kloop, s);
    else if (p.E <= 16) launch_lin_tiles_ep<16, BWD>(p, kloop, s);
    else launch_lin_tiles_ep<24, BWD>(p, kloop, s);
}

// sum over the column blocks, in block order, of partial sum `which` of (output a, row)
__device__ inline double block_sum(const double* part, int a, int which, size_t row, int nCB, int NW, size_t Mc) {
    const double* src = part + ((size_t)a * nCB * NW + which) * Mc + row;
    double s = 0.0;
    for (int cb = 0; cb < nCB; ++cb) s += src[(size_t)cb * NW * Mc];
    return s;
}

// Index 0 of the stored trajectory and the model inputs of step 0.
__global__ __launch_bounds__(64) void rollout_linear_init_kernel(LinStepArgs p) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int D = p.D, E = p.E, A = p.A, H = p.H;
    double* mu = p.mu + (size_t)b * (H + 1) * D;
    double* Sg = p.Sig + (size_t)b * (H + 1) * D * D;
    double* xq = p.Xq + (size_t)b * E;
    for (int idx = tid; idx < D * D; idx += 64) Sg[idx] = p.S0[idx];
    if (tid < D) {
        mu[tid] = p.mu0[tid];
        xq[tid] = p.mu0[tid];
    }
    if (tid < A) xq[D + tid] = p.actions[(size_t)b * H * A + tid];
    if (p.include_time && tid == 0) xq[E - 1] = p.time0;
}

// One wavefront per candidate: step t -> t + 1 of the stored trajectory
//   mu' = mu + M,  T = Sigma J,  Sigma' = Sigma + (J^T Sigma J + diag v) + T + T^T
// and the model inputs of step t + 1.  Open loop: J = V_s, the state rows of V.  Closed loop (FB): the policy
// u = ubar_t + K_t (x - mu_t) makes the model input's covariance G Sigma_t G^T with G = [I ; K_t ; 0], so J = C = G^T V =
// V_s + K_t^T V_u (V_u: the action rows of V).  The mean takes the same operations in both (its bits do not depend on the gains).
// keepM / keepV: the step's M and the rows of V it read are kept for a reverse sweep.
template <bool FB>
__global__ __launch_bounds__(64) void rollout_linear_step_kernel(LinStepArgs p) {
    constexpr int kVR = FB ? kMaxE : kMaxD;          // rows of V read: the state inputs (FB: and the action inputs)
    __shared__ double s_sum[kMaxD][kVR + 2];         // sum P k | sum k beta | the Jacobian sums of those inputs
    __shared__ double s_V[kVR][kMaxD];               // V [input][output]
    [[maybe_unused]] __shared__ double s_K[FB ? kMaxE : 1][kMaxD];      // FB: K_t [action][state]
    [[maybe_unused]] __shared__ double s_C[FB ? kMaxD : 1][kMaxD];      // FB: C = V_s + K_t^T V_u
    __shared__ double s_S[kMaxD][kMaxD];             // Sigma_t
    __shared__ double s_T[kMaxD][kMaxD];             // Sigma_t J
    const int b = blockIdx.x, tid = threadIdx.x;
    const int D = p.D, E = p.E, A = p.A, H = p.H, t = p.t, NV = FB ? D + A : D, NS = NV + 2;
    const double* mu_t = p.mu + ((size_t)b * (H + 1) + t) * D;
    const double* Sg_t = p.Sig + ((size_t)b * (H + 1) + t) * D * D;
    double* mu_n = p.mu + ((size_t)b * (H + 1) + t + 1) * D;
    double* Sg_n = p.Sig + ((size_t)b * (H + 1) + t + 1) * D * D;
    for (int idx = tid; idx < D * NS; idx += 64) {
        const int a = idx / NS, which = idx - a * NS;
        s_sum[a][which] = block_sum(p.part, a, which, (size_t)b, p.nCB, p.NW, (size_t)p.Mc);
    }
    for (int idx = tid; idx < D * D; idx += 64) s_S[idx / D][idx % D] = Sg_t[idx];
    if constexpr (FB) {
        const double* K = p.gains + (size_t)b * (size_t)p.gain_stride + (size_t)t * A * D;
        for (int idx = tid; idx < A * D; idx += 64) s_K[idx / D][idx % D] = K[idx];
    }
    __syncthreads();
    for (int idx = tid; idx < NV * D; idx += 64) {
        const int i = idx / D, a = idx - i * D;
        const double v = p.ils2[a * E + i] * s_sum[a][2 + i];
        s_V[i][a] = v;
        if (p.keepV) p.keepV[((size_t)b * H + t) * NV * D + idx] = v;
    }
    __syncthreads();
    const double (*s_J)[kMaxD] = s_V;
    if constexpr (FB) {
        for (int idx = tid; idx < D * D; idx += 64) {            // C = V_s + K^T V_u, the actions in order
            const int i = idx / D, c = idx - i * D;
            double v = 0.0;
            for (int u = 0; u < A; ++u) v = fma(s_K[u][i], s_V[D + u][c], v);
            s_C[i][c] = s_V[i][c] + v;
        }
        __syncthreads();
        s_J = s_C;
    }
    for (int idx = tid; idx < D * D; idx += 64) {                // T = Sigma_t J
        const int i = idx / D, c = idx - i * D;
        double v = 0.0;
        for (int k = 0; k < D; ++k) v = fma(s_S[i][k], s_J[k][c], v);
        s_T[i][c] = v;
    }
    __syncthreads();
    for (int idx = tid; idx < D * D; idx += 64) {                // a <= c, mirrored: exactly symmetric
        const int a = idx / D, c = idx - a * D;
        if (a > c) continue;
        double q = 0.0;
        for (int i = 0; i < D; ++i) q = fma(s_J[i][a], s_T[i][c], q);
        if (a == c) q += p.var[a] - s_sum[a][0];                 // not clamped
        const double v = (s_S[a][c] + q) + (s_T[a][c] + s_T[c][a]);
        Sg_n[a * D + c] = v;
        Sg_n[c * D + a] = v;
    }
    const bool more = t + 1 < H;
    double* xq = p.Xq + (size_t)b * E;
    if (tid < D) {
        const double v = mu_t[tid] + s_sum[tid][1];
        if (p.keepM) p.keepM[((size_t)b * H + t) * D + tid] = s_sum[tid][1];
        mu_n[tid] = v;
        if (more) xq[tid] = v;
    }
    if (more) {
        if (tid < A) xq[D + tid] = p.actions[((size_t)b * H + t + 1) * A + tid];
        if (p.include_time && tid == 0) xq[E - 1] = p.time0 + (double)(t + 1);
    }
}

}  // namespace

}  // namespace gpmpc_hip
