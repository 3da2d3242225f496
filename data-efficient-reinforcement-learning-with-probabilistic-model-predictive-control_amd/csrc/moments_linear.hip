// moments_linear.hip -- first-order (linearised) propagation of a Gaussian input through the GP posterior (gpmpc_moments_linear)
// and the horizon rollout built on it (gpmpc_rollout_linear).  Per point with input mean m (E), covariance Sigma (E x E), output a:
//   k_aj = sigma2_a exp(-1/2 sum_e (m_e - x_je)^2 / l_ae^2)
//   M_a = sum_j k_aj beta_aj                              posterior mean at m
//   V[e,a] = (1 / l_ae^2) sum_j beta_aj k_aj (x_je - m_e)   its Jacobian dM_a / dm_e
//   v_a = sigma2_a - k_a^T iK_a k_a                       posterior variance at m (not clamped, no noise)
//   S = V^T Sigma V + diag(v)
// from the cached Xt / ils2 / var / beta / iK.  The differences x_je - m_e are formed per element: the factored form
// sum_j c x_j - m sum_j c cancels digits with a time input.
//
// Structure ("Linearised propagation"):
//   moments_linear_tile_kernel    one workgroup per (64 rows, 256-column block of iK_a, output a): P = K*_a iK_a by the k loop of
//                                 predict.hip (K* tile built on the fly, iK tile staged in LDS, the next one loaded under the MFMAs;
//                                 predict.hip and predict_cov.hip keep their own copies, so that their code is unchanged).  The
//                                 epilogue walks the block in four slices of 64 columns: every lane forms k for its 16 rows x 1
//                                 column, adds P k to its row sums and stages beta k in LDS; then each thread owns one row and the
//                                 inputs e = w + 4 q and walks the slice's columns in order.  Per row it leaves the block's partial
//                                 sums  sum_j P_mj k_mj | sum_j k_mj beta_j | E sums beta_j k_mj (x_je - m_e).  Without S the k
//                                 loop is compiled out.
//   moments_linear_finish_kernel  one wavefront per point: adds the column blocks in block order, scales the Jacobian, forms
//                                 Sigma V and V^T (Sigma V) for a <= b and mirrors.
//   rollout_linear_init_kernel /  the rollout is batch-major: per horizon step one tile launch over all candidates of the chunk,
//   rollout_linear_step_kernel    then one wavefront per candidate adds the blocks, advances (mu, Sigma) in the stored trajectory
//                                   mu' = mu + M,  T = Sigma V_s,  Sigma' = Sigma + (V_s^T Sigma V_s + diag v) + T + T^T
//                                 (V_s: the state rows of V) and writes the next step's model inputs [mu' | action | time0 + t + 1].
//   rollout_linear_feedback_step_kernel /   the closed-loop rollout (gpmpc_rollout_linear_feedback): the same init kernel and tile
//   traj_cost_feedback_kernel     launches; the step uses C = V_s + K_t^T V_u in place of V_s, the cost kernel the state-action
//                                 covariance [I ; K_t] Sigma_t [I ; K_t]^T in place of block_diag(Sigma_t, 0).
// Every sum runs in an order fixed by N, E and D alone (k steps, lanes, waves, slices, column blocks): a point's bits do not depend
// on the batch size, on its place in the batch, on its neighbours or on the chunks.  Plain kernels: no atomics, no waits between
// workgroups.  The workspace (Handle::linws) is this file's own, sized by plan_moments_linear (moments_linear_plan.h); a chunk of
// candidates runs its whole horizon.  There is no fused-horizon form: with few candidates a 64-row tile is mostly padding and
// every step costs two launches.
#include "device_common.h"
#include "moments_linear_plan.h"

namespace gpmpc_hip {

namespace {

constexpr int kBM = kLinBM;              // rows per workgroup
constexpr int kBN = kLinBN;              // columns of iK per workgroup (64 per wave)
constexpr int kBK = 16;                  // memory points per k step
constexpr int kAPitch = kBM + 16;        // LDS row pitch (doubles) of the K* tile, stored [k][row]: rows 32 banks apart
constexpr int kBPitch = kBN + 16;        // ... and of the iK tile [k][column]
constexpr int kSlice = 64;               // columns of beta k staged in LDS at a time (16 per wave)
constexpr int kCkPitch = kBM + 2;        // LDS pitch (doubles) of s_ck [column][row]: 32 lanes of a write hit distinct banks

struct LinTileArgs {
    const double* Xq;        // (rows, E) input means of this chunk
    const double* Xt;        // (E, N)
    const double* ils2;      // (D, E)
    const double* var;       // (D)
    const double* beta;      // (D, N)
    const double* iK;        // (D, N, N)
    double* part;            // (D, nCB, NW, Mc): sum_j P k | sum_j k beta | E sums beta k (x_j - m)
    int rows, N, E, D, nCB, NW;
    long long Mc;
};

struct LinFinishArgs {
    const double* part;
    const double* ils2;      // (D, E)
    const double* var;       // (D)
    const double* Sig;       // (rows, E, E) of this chunk, or NULL (= 0)
    double* M_out;           // (rows, D) of this chunk, or NULL
    double* S_out;           // (rows, D, D) of this chunk, or NULL
    double* V_out;           // (rows, E, D) of this chunk, or NULL
    int rows, E, D, nCB, NW;
    long long Mc;
};

struct LinStepArgs {
    const double* part;
    const double* ils2;      // (D, E)
    const double* var;       // (D)
    const double* actions;   // (rows, H, A) of this chunk
    double* mu;              // (rows, H + 1, D) of this chunk
    double* Sig;             // (rows, H + 1, D, D) of this chunk
    double* Xq;              // (Mc, E) model inputs of the next tile launch
    int rows, E, D, A, H, nCB, NW, t, include_time;
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

// Grid and k loop of predict_tile_kernel.  s_ck reuses the k loop's s_A / s_B.  The mean and Jacobian sums are the same
// operations in both instantiations: they keep their bits when S is not asked for.
template <int EP, bool VAR>
__global__ __launch_bounds__(256) void moments_linear_tile_kernel(LinTileArgs p) {
    constexpr int kLoop = kBK * kAPitch + kBK * kBPitch;
    constexpr int kMem = (VAR && kLoop > kSlice * kCkPitch) ? kLoop : kSlice * kCkPitch;
    constexpr int kQ = EP / 4;                       // inputs per thread in the contraction
    __shared__ double s_xq[kBM][EP + 1];
    __shared__ double s_xj[kSlice][EP + 1];
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

    // epilogue: f64 C/D layout -- acc[rt][ct][r] = P[16 rt + (lane >> 4) + 4 r][64 w + 16 ct + (lane & 15)]
    double rd[4][4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) rd[rt][r] = 0.0;
    // contraction state: row `crow`, inputs e = w + 4 q; wave 0 also sums beta k itself (the mean)
    const int crow = tid & 63;
    double xo[kQ], g[kQ], mn = 0.0;
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
                    if constexpr (VAR) rd[rt][r] = fma(acc[rt][ct][r], k, rd[rt][r]);
                    ck = bj * k;
                }
                s_ck[c][row] = ck;
            }
        __syncthreads();
#pragma unroll 4
        for (int cs = 0; cs < kSlice; ++cs) {
            const double ck = s_ck[cs][crow];
            if (w == 0) mn += ck;
#pragma unroll
            for (int q = 0; q < kQ; ++q) g[q] = fma(ck, s_xj[cs][w + 4 * q] - xo[q], g[q]);
        }
    }
    const size_t rstride = (size_t)p.Mc;
    double* dst = p.part + ((size_t)a * p.nCB + cb) * p.NW * rstride;      // [which][row]
    if (m0 + crow < p.rows) {
        if (w == 0) dst[rstride + m0 + crow] = mn;
#pragma unroll
        for (int q = 0; q < kQ; ++q)
            if (w + 4 * q < E) dst[(size_t)(2 + w + 4 * q) * rstride + m0 + crow] = g[q];
    }
    if constexpr (VAR) {
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

// sum over the column blocks, in block order, of partial sum `which` of (output a, row)
__device__ inline double block_sum(const double* part, int a, int which, size_t row, int nCB, int NW, size_t Mc) {
    const double* src = part + ((size_t)a * nCB * NW + which) * Mc + row;
    double s = 0.0;
    for (int cb = 0; cb < nCB; ++cb) s += src[(size_t)cb * NW * Mc];
    return s;
}

// One wavefront per point.
__global__ __launch_bounds__(64) void moments_linear_finish_kernel(LinFinishArgs p) {
    __shared__ double s_sum[kMaxD][kMaxE + 2];
    __shared__ double s_V[kMaxE][kMaxD];
    __shared__ double s_T[kMaxE][kMaxD];
    const int m = blockIdx.x, tid = threadIdx.x;
    const int D = p.D, E = p.E, NW = p.NW;
    const bool with_S = p.S_out != nullptr;
    for (int idx = tid; idx < D * NW; idx += 64) {
        const int a = idx / NW, which = idx - a * NW;
        s_sum[a][which] = (which == 0 && !with_S) ? 0.0 : block_sum(p.part, a, which, (size_t)m, p.nCB, NW, (size_t)p.Mc);
    }
    __syncthreads();
    for (int idx = tid; idx < E * D; idx += 64) {
        const int e = idx / D, a = idx - e * D;
        const double v = p.ils2[a * E + e] * s_sum[a][2 + e];
        s_V[e][a] = v;
        if (p.V_out) p.V_out[(size_t)m * E * D + idx] = v;
    }
    if (p.M_out && tid < D) p.M_out[(size_t)m * D + tid] = s_sum[tid][1];
    if (!with_S) return;
    __syncthreads();
    if (p.Sig) {
        const double* Sg = p.Sig + (size_t)m * E * E;
        for (int idx = tid; idx < E * D; idx += 64) {            // T = Sigma V
            const int e = idx / D, b = idx - e * D;
            double t = 0.0;
            for (int f = 0; f < E; ++f) t = fma(Sg[e * E + f], s_V[f][b], t);
            s_T[e][b] = t;
        }
        __syncthreads();
    }
    double* S = p.S_out + (size_t)m * D * D;
    for (int idx = tid; idx < D * D; idx += 64) {                // a <= b, mirrored: exactly symmetric
        const int a = idx / D, b = idx - a * D;
        if (a > b) continue;
        double q = 0.0;
        if (p.Sig)
            for (int e = 0; e < E; ++e) q = fma(s_V[e][a], s_T[e][b], q);
        if (a == b) q += p.var[a] - s_sum[a][0];                 // not clamped
        S[a * D + b] = q;
        S[b * D + a] = q;
    }
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

// One wavefront per candidate: step t -> t + 1 of the stored trajectory, and the model inputs of step t + 1.
__global__ __launch_bounds__(64) void rollout_linear_step_kernel(LinStepArgs p) {
    __shared__ double s_sum[kMaxD][kMaxD + 2];       // sum P k | sum k beta | the Jacobian sums of the state inputs
    __shared__ double s_V[kMaxD][kMaxD];             // V_s [state input][output]
    __shared__ double s_S[kMaxD][kMaxD];             // Sigma_t
    __shared__ double s_T[kMaxD][kMaxD];             // Sigma_t V_s
    const int b = blockIdx.x, tid = threadIdx.x;
    const int D = p.D, E = p.E, A = p.A, H = p.H, t = p.t, NS = D + 2;
    const double* mu_t = p.mu + ((size_t)b * (H + 1) + t) * D;
    const double* Sg_t = p.Sig + ((size_t)b * (H + 1) + t) * D * D;
    double* mu_n = p.mu + ((size_t)b * (H + 1) + t + 1) * D;
    double* Sg_n = p.Sig + ((size_t)b * (H + 1) + t + 1) * D * D;
    for (int idx = tid; idx < D * NS; idx += 64) {
        const int a = idx / NS, which = idx - a * NS;
        s_sum[a][which] = block_sum(p.part, a, which, (size_t)b, p.nCB, p.NW, (size_t)p.Mc);
    }
    for (int idx = tid; idx < D * D; idx += 64) s_S[idx / D][idx % D] = Sg_t[idx];
    __syncthreads();
    for (int idx = tid; idx < D * D; idx += 64) {
        const int i = idx / D, a = idx - i * D;
        s_V[i][a] = p.ils2[a * E + i] * s_sum[a][2 + i];
    }
    __syncthreads();
    for (int idx = tid; idx < D * D; idx += 64) {                // T = Sigma_t V_s
        const int i = idx / D, c = idx - i * D;
        double v = 0.0;
        for (int k = 0; k < D; ++k) v = fma(s_S[i][k], s_V[k][c], v);
        s_T[i][c] = v;
    }
    __syncthreads();
    for (int idx = tid; idx < D * D; idx += 64) {                // a <= c, mirrored: exactly symmetric
        const int a = idx / D, c = idx - a * D;
        if (a > c) continue;
        double q = 0.0;
        for (int i = 0; i < D; ++i) q = fma(s_V[i][a], s_T[i][c], q);
        if (a == c) q += p.var[a] - s_sum[a][0];                 // not clamped
        const double v = (s_S[a][c] + q) + (s_T[a][c] + s_T[c][a]);
        Sg_n[a * D + c] = v;
        Sg_n[c * D + a] = v;
    }
    const bool more = t + 1 < H;
    double* xq = p.Xq + (size_t)b * E;
    if (tid < D) {
        const double v = mu_t[tid] + s_sum[tid][1];
        mu_n[tid] = v;
        if (more) xq[tid] = v;
    }
    if (more) {
        if (tid < A) xq[D + tid] = p.actions[((size_t)b * H + t + 1) * A + tid];
        if (p.include_time && tid == 0) xq[E - 1] = p.time0 + (double)(t + 1);
    }
}

// ------------------------------------------------------------------------------------------
// Closed-loop form (gpmpc_rollout_linear_feedback): the policy u = ubar_t + K_t (x - mu_t) makes the model input's covariance
// G Sigma_t G^T with G = [I ; K_t ; 0], so the step's D x D Jacobian is C = G^T V = V_s + K_t^T V_u (V_u: the action rows of V).
struct LinFbStepArgs {
    const double* part;
    const double* ils2;      // (D, E)
    const double* var;       // (D)
    const double* actions;   // (rows, H, A) of this chunk
    const double* gains;     // (H, A, D) of the chunk's first candidate
    long long gain_stride;   // doubles between two candidates' gains (0: one gain sequence shared by all)
    double* mu;              // (rows, H + 1, D) of this chunk
    double* Sig;             // (rows, H + 1, D, D) of this chunk
    double* Xq;              // (Mc, E) model inputs of the next tile launch
    int rows, E, D, A, H, nCB, NW, t, include_time;
    long long Mc;
    double time0;
};

// One wavefront per candidate: rollout_linear_step_kernel with C in place of V_s.  The mean takes the same operations as there
// (its bits do not depend on the gains).
__global__ __launch_bounds__(64) void rollout_linear_feedback_step_kernel(LinFbStepArgs p) {
    __shared__ double s_sum[kMaxD][kMaxE + 2];       // sum P k | sum k beta | the Jacobian sums of the state and action inputs
    __shared__ double s_V[kMaxE][kMaxD];             // V [state or action input][output]
    __shared__ double s_K[kMaxE][kMaxD];             // K_t [action][state]
    __shared__ double s_C[kMaxD][kMaxD];             // C = V_s + K_t^T V_u
    __shared__ double s_S[kMaxD][kMaxD];             // Sigma_t
    __shared__ double s_T[kMaxD][kMaxD];             // Sigma_t C
    const int b = blockIdx.x, tid = threadIdx.x;
    const int D = p.D, E = p.E, A = p.A, H = p.H, t = p.t, DA = D + A, NS = DA + 2;
    const double* mu_t = p.mu + ((size_t)b * (H + 1) + t) * D;
    const double* Sg_t = p.Sig + ((size_t)b * (H + 1) + t) * D * D;
    double* mu_n = p.mu + ((size_t)b * (H + 1) + t + 1) * D;
    double* Sg_n = p.Sig + ((size_t)b * (H + 1) + t + 1) * D * D;
    const double* K = p.gains + (size_t)b * (size_t)p.gain_stride + (size_t)t * A * D;
    for (int idx = tid; idx < D * NS; idx += 64) {
        const int a = idx / NS, which = idx - a * NS;
        s_sum[a][which] = block_sum(p.part, a, which, (size_t)b, p.nCB, p.NW, (size_t)p.Mc);
    }
    for (int idx = tid; idx < D * D; idx += 64) s_S[idx / D][idx % D] = Sg_t[idx];
    for (int idx = tid; idx < A * D; idx += 64) s_K[idx / D][idx % D] = K[idx];
    __syncthreads();
    for (int idx = tid; idx < DA * D; idx += 64) {
        const int i = idx / D, a = idx - i * D;
        s_V[i][a] = p.ils2[a * E + i] * s_sum[a][2 + i];
    }
    __syncthreads();
    for (int idx = tid; idx < D * D; idx += 64) {                // C = V_s + K^T V_u, the actions in order
        const int i = idx / D, c = idx - i * D;
        double v = 0.0;
        for (int u = 0; u < A; ++u) v = fma(s_K[u][i], s_V[D + u][c], v);
        s_C[i][c] = s_V[i][c] + v;
    }
    __syncthreads();
    for (int idx = tid; idx < D * D; idx += 64) {                // T = Sigma_t C
        const int i = idx / D, c = idx - i * D;
        double v = 0.0;
        for (int k = 0; k < D; ++k) v = fma(s_S[i][k], s_C[k][c], v);
        s_T[i][c] = v;
    }
    __syncthreads();
    for (int idx = tid; idx < D * D; idx += 64) {                // a <= c, mirrored: exactly symmetric
        const int a = idx / D, c = idx - a * D;
        if (a > c) continue;
        double q = 0.0;
        for (int i = 0; i < D; ++i) q = fma(s_C[i][a], s_T[i][c], q);
        if (a == c) q += p.var[a] - s_sum[a][0];                 // not clamped
        const double v = (s_S[a][c] + q) + (s_T[a][c] + s_T[c][a]);
        Sg_n[a * D + c] = v;
        Sg_n[c * D + a] = v;
    }
    const bool more = t + 1 < H;
    double* xq = p.Xq + (size_t)b * E;
    if (tid < D) {
        const double v = mu_t[tid] + s_sum[tid][1];
        mu_n[tid] = v;
        if (more) xq[tid] = v;
    }
    if (more) {
        if (tid < A) xq[D + tid] = p.actions[((size_t)b * H + t + 1) * A + tid];
        if (p.include_time && tid == 0) xq[E - 1] = p.time0 + (double)(t + 1);
    }
}

// Stage / terminal costs and the objective of the closed-loop trajectory: traj_cost_body (one wavefront per candidate, lanes over
// the H + 1 steps, wave_xor_sum for J) with the state-action covariance Sigma_z = G Sigma_t G^T, G = [I ; K_t], in place of
// block_diag(Sigma_t, 0).  Sigma_z enters the quadratic cost only through
//   tr(Sigma_z W) = tr(Sigma_t Wg),  tr(2 (W Sigma_z)^2) = tr(2 (Wg Sigma_t)^2),  e^T W Sigma_z W e = (G^T W^T e)^T Sigma_t (G^T W e)
// with Wg = G^T W G, so a lane keeps D^2 + 2 D values (DP: the array bound) instead of (D + A)^2.  Terminal step: G = I, W = W_T.
template <int DP>
__global__ __launch_bounds__(64) void traj_cost_feedback_kernel(const double* __restrict__ mu, const double* __restrict__ Sig,
                                                                const double* __restrict__ actions,
                                                                const double* __restrict__ gains, long long gain_stride,
                                                                const double* __restrict__ cost, int D, int A, int H,
                                                                double kappa, int clip, int use_constraints,
                                                                double* __restrict__ cm_out, double* __restrict__ cv_out,
                                                                double* __restrict__ J_out) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int DA = D + A;
    const double* target = cost;
    const double* W = cost + DA;
    const double* WT = W + DA * DA;
    const double* smin = WT + D * D;
    const double* smax = smin + D;
    double jsum = 0.0;
    for (int t = lane; t <= H; t += 64) {
        const bool terminal = (t == H);
        const int n = terminal ? D : DA, Au = terminal ? 0 : A;
        const double* Wm = terminal ? WT : W;
        const double* m = mu + ((size_t)c * (H + 1) + t) * D;
        const double* S = Sig + ((size_t)c * (H + 1) + t) * D * D;
        const double* a = actions + ((size_t)c * H + (terminal ? 0 : t)) * A;
        const double* K = gains + (size_t)c * (size_t)gain_stride + (size_t)(terminal ? 0 : t) * A * D;      // [action][state]
        auto err = [&](int i) { return (i < D ? m[i] : a[i - D]) - target[i]; };
        double Wg[DP * DP], p1[DP], p2[DP];
        for (int i = 0; i < D; ++i) {
            for (int j = 0; j < D; ++j) {
                double w = Wm[i * n + j];
                for (int u = 0; u < Au; ++u) {
                    w = fma(Wm[i * n + D + u], K[u * D + j], w);
                    w = fma(K[u * D + i], Wm[(D + u) * n + j], w);
                    double kw = 0.0;
                    for (int v = 0; v < Au; ++v) kw = fma(Wm[(D + u) * n + D + v], K[v * D + j], kw);
                    w = fma(K[u * D + i], kw, w);
                }
                Wg[i * DP + j] = w;
            }
            double v1 = 0.0, v2 = 0.0;                           // (G^T W^T e)_i, (G^T W e)_i
            for (int k = 0; k < n; ++k) {
                v1 = fma(err(k), Wm[k * n + i], v1);
                v2 = fma(Wm[i * n + k], err(k), v2);
            }
            for (int u = 0; u < Au; ++u) {
                double r1 = 0.0, r2 = 0.0;
                for (int k = 0; k < n; ++k) {
                    r1 = fma(err(k), Wm[k * n + D + u], r1);
                    r2 = fma(Wm[(D + u) * n + k], err(k), r2);
                }
                v1 = fma(K[u * D + i], r1, v1);
                v2 = fma(K[u * D + i], r2, v2);
            }
            p1[i] = v1;
            p2[i] = v2;
        }
        double cm = 0.0, cv = 0.0;
        // tr(Sigma Wg) and e^T W e
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) cm = fma(S[i * D + j], Wg[j * DP + i], cm);
        for (int i = 0; i < n; ++i) {
            const double ei = err(i);
            for (int j = 0; j < n; ++j) cm = fma(ei * Wm[i * n + j], err(j), cm);
        }
        // tr(2 TS TS) with TS = Wg Sigma, 4 p1^T Sigma p2
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) {
                double tij = 0.0, tji = 0.0;
                for (int k = 0; k < D; ++k) {
                    tij = fma(Wg[i * DP + k], S[k * D + j], tij);
                    tji = fma(Wg[j * DP + k], S[k * D + i], tji);
                }
                cv = fma(2.0 * tij, tji, cv);
                cv = fma(4.0 * p1[i] * S[i * D + j], p2[j], cv);
            }
        if (use_constraints && !terminal) {                      // state marginals only, as traj_cost_body
            for (int d = 0; d < D; ++d) {
                const double sg = S[d * D + d];
                cm += 0.5 * (1.0 + erf((smin[d] - m[d]) / (sg * 1.4142135623730951)))
                    + (1.0 - 0.5 * (1.0 + erf((smax[d] - m[d]) / (sg * 1.4142135623730951))));
            }
        }
        double ucb = -cm + kappa * sqrt(cv);
        if (clip) ucb = fmin(ucb, 0.0);
        jsum -= ucb;
        if (cm_out) cm_out[(size_t)c * (H + 1) + t] = cm;
        if (cv_out) cv_out[(size_t)c * (H + 1) + t] = cv;
    }
    jsum = wave_xor_sum(jsum);
    if (lane == 0 && J_out) J_out[c] = jsum / (double)(H + 1);
}

template <int EP>
void launch_lin_tiles_ep(const LinTileArgs& p, bool var, hipStream_t s) {
    const dim3 grid((p.rows + kBM - 1) / kBM, p.nCB, p.D);
    if (var) hipLaunchKernelGGL((moments_linear_tile_kernel<EP, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((moments_linear_tile_kernel<EP, false>), grid, dim3(256), 0, s, p);
}

void launch_lin_tiles(const LinTileArgs& p, bool var, hipStream_t s) {
    if (p.E <= 4) launch_lin_tiles_ep<4>(p, var, s);
    else if (p.E <= 8) launch_lin_tiles_ep<8>(p, var, s);
    else if (p.E <= 16) launch_lin_tiles_ep<16>(p, var, s);
    else launch_lin_tiles_ep<24>(p, var, s);
}

}  // namespace

int launch_traj_cost_feedback(Handle* h, const RolloutArgs& a, int rows, const double* mu, const double* Sig, const double* actions,
                              const double* gains, long long gain_stride, double* cm, double* cv, double* J, hipStream_t s) {
    const int D = a.D, A = a.A, H = a.H;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(rows), dim3(64), 0, s, mu, Sig, actions, gains, gain_stride, a.cost, D, A, H, a.kappa,
                           a.clip, a.use_constraints, cm, cv, J);
    };
    static_assert(kMaxD <= 16, "traj_cost_feedback_kernel: per-lane arrays");
    if (D <= 4) launch(traj_cost_feedback_kernel<4>);
    else if (D <= 8) launch(traj_cost_feedback_kernel<8>);
    else launch(traj_cost_feedback_kernel<16>);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

int run_moments_linear(Handle* h, const double* mu, const double* Sig, int P, double* M_out, double* S_out, double* V_out,
                       hipStream_t s) {
    const int N = h->N, D = h->D, E = h->E;
    if (P == 0 || (!M_out && !S_out && !V_out)) return GPMPC_OK;
    LinearPlan pl;
    plan_moments_linear(N, D, E, P, 0, false, h->opt_moments_linear_chunk, pl);
    int rc = grow(h, h->linws, pl.total);
    if (rc) return rc;
    LinTileArgs p{};
    p.Xt = h->Xt.p; p.ils2 = h->ils2.p; p.var = h->var.p; p.beta = h->beta.p; p.iK = h->iK.p;
    p.part = h->linws.p;
    p.N = N; p.E = E; p.D = D; p.nCB = pl.nCB; p.NW = pl.NW; p.Mc = pl.Mc;
    LinFinishArgs f{};
    f.part = p.part; f.ils2 = p.ils2; f.var = p.var;
    f.E = E; f.D = D; f.nCB = pl.nCB; f.NW = pl.NW; f.Mc = pl.Mc;
    for (long long m0 = 0; m0 < P; m0 += pl.chunk) {
        const int rows = (int)((P - m0) < pl.chunk ? (P - m0) : pl.chunk);
        p.rows = rows;
        p.Xq = mu + (size_t)m0 * E;
        launch_lin_tiles(p, S_out != nullptr, s);
        f.rows = rows;
        f.Sig = Sig ? Sig + (size_t)m0 * E * E : nullptr;
        f.M_out = M_out ? M_out + (size_t)m0 * D : nullptr;
        f.S_out = S_out ? S_out + (size_t)m0 * D * D : nullptr;
        f.V_out = V_out ? V_out + (size_t)m0 * E * D : nullptr;
        hipLaunchKernelGGL(moments_linear_finish_kernel, dim3(rows), dim3(64), 0, s, f);
    }
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

// a: filled by the entry point (model, cost settings, actions, shape, initial state, outputs -- each output may be NULL).
// gains != NULL: the closed-loop rollout under u = ubar_t + K_t (x - mu_t), gains (B, H, A, D) when per_candidate, else (H, A, D)
// shared by all candidates -- the same plan, workspace, init kernel and tile launches with the step and cost kernels exchanged; a
// chunk of candidates offsets the gain pointer only when the gains are per candidate.
int run_rollout_linear(Handle* h, const RolloutArgs& a, hipStream_t s, const double* gains, bool per_candidate) {
    const int N = a.N, D = a.D, E = a.E, A = a.A, H = a.H, B = a.B;
    const bool own_traj = !a.mu_out || !a.Sig_out;
    const bool costs = a.cm_out || a.cv_out || a.J_out;
    LinearPlan pl;
    plan_moments_linear(N, D, E, B, H, own_traj, h->opt_moments_linear_chunk, pl);
    int rc = grow(h, h->linws, pl.total);
    if (rc) return rc;
    LinTileArgs p{};
    p.Xt = h->Xt.p; p.ils2 = h->ils2.p; p.var = h->var.p; p.beta = h->beta.p; p.iK = h->iK.p;
    p.part = h->linws.p;
    p.Xq = h->linws.p + pl.part;
    p.N = N; p.E = E; p.D = D; p.nCB = pl.nCB; p.NW = pl.NW; p.Mc = pl.Mc;
    double* own_mu = h->linws.p + pl.part + pl.xq;
    double* own_Sig = own_mu + (size_t)pl.chunk * (H + 1) * D;
    LinStepArgs q{};
    q.part = p.part; q.ils2 = p.ils2; q.var = p.var;
    q.Xq = h->linws.p + pl.part;
    q.E = E; q.D = D; q.A = A; q.H = H; q.nCB = pl.nCB; q.NW = pl.NW; q.Mc = pl.Mc;
    q.include_time = a.include_time; q.time0 = a.time0;
    for (int d = 0; d < D; ++d) q.mu0[d] = a.mu0[d];
    for (int d = 0; d < D * D; ++d) q.S0[d] = a.S0[d];
    LinFbStepArgs f{};
    f.part = p.part; f.ils2 = p.ils2; f.var = p.var;
    f.Xq = q.Xq;
    f.E = E; f.D = D; f.A = A; f.H = H; f.nCB = pl.nCB; f.NW = pl.NW; f.Mc = pl.Mc;
    f.include_time = a.include_time; f.time0 = a.time0;
    f.gain_stride = per_candidate ? (long long)H * A * D : 0;
    for (long long b0 = 0; b0 < B; b0 += pl.chunk) {
        const int rows = (int)((B - b0) < pl.chunk ? (B - b0) : pl.chunk);
        p.rows = rows; q.rows = rows; f.rows = rows;
        q.actions = a.actions + (size_t)b0 * H * A;
        q.mu = a.mu_out ? a.mu_out + (size_t)b0 * (H + 1) * D : own_mu;
        q.Sig = a.Sig_out ? a.Sig_out + (size_t)b0 * (H + 1) * D * D : own_Sig;
        q.t = 0;
        f.actions = q.actions; f.mu = q.mu; f.Sig = q.Sig;
        f.gains = gains ? gains + (size_t)b0 * (size_t)f.gain_stride : nullptr;
        hipLaunchKernelGGL(rollout_linear_init_kernel, dim3(rows), dim3(64), 0, s, q);
        for (int t = 0; t < H; ++t) {
            launch_lin_tiles(p, true, s);
            q.t = t; f.t = t;
            if (gains) hipLaunchKernelGGL(rollout_linear_feedback_step_kernel, dim3(rows), dim3(64), 0, s, f);
            else hipLaunchKernelGGL(rollout_linear_step_kernel, dim3(rows), dim3(64), 0, s, q);
        }
        GPMPC_HIP_CHECK(h, hipGetLastError());
        if (costs && gains) {                         // closed-loop stage costs + objective of the chunk's stored trajectory
            double* cm = a.cm_out ? a.cm_out + (size_t)b0 * (H + 1) : nullptr;
            double* cv = a.cv_out ? a.cv_out + (size_t)b0 * (H + 1) : nullptr;
            double* J = a.J_out ? a.J_out + b0 : nullptr;
            rc = launch_traj_cost_feedback(h, a, rows, f.mu, f.Sig, f.actions, f.gains, f.gain_stride, cm, cv, J, s);
            if (rc) return rc;
        } else if (costs) {                           // stage costs + objective of the chunk's stored trajectory
            RolloutArgs c = a;
            c.B = rows;
            c.actions = q.actions;
            c.mu_out = q.mu; c.Sig_out = q.Sig;
            rc = launch_traj_cost(h, c, a.cm_out ? a.cm_out + (size_t)b0 * (H + 1) : nullptr,
                                  a.cv_out ? a.cv_out + (size_t)b0 * (H + 1) : nullptr, a.J_out ? a.J_out + b0 : nullptr, s);
            if (rc) return rc;
        }
    }
    return GPMPC_OK;
}

}  // namespace gpmpc_hip
