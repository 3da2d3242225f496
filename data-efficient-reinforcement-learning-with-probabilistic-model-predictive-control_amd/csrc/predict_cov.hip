// predict_cov.hip -- joint GP posterior covariance between query points (gpmpc_predict_cov):
//   t_a(x, x') = sigma2_a exp(-1/2 sum_e (x_e - x'_e)^2 / l_ae^2)  -  k_a(x)^T iK_a k_a(x')
// with k_a(x)_i = sigma2_a exp(-1/2 sum_e (x_e - x_ie)^2 / l_ae^2), from the cached Xt / ils2 / var / iK.
// Cross form: cov[a, i, j] = t_a(xa_i, xb_j).  Joint form: cov[a, i, j] = 1/2 (t_a(x_i, x_j) + t_a(x_j, x_i)) (+ noise_a on the
// diagonal), exactly symmetric whatever iK is.
//
// Structure ("Joint posterior covariance between query points"):
//   predict_cov_p_kernel     one workgroup per (64 rows of Xa, 256-column block of iK_a, output a): P = K*_a(Xa) iK_a by the k
//                            loop of predict.hip (K* tile built on the fly, iK tile staged in LDS, the next one loaded under the
//                            MFMAs), the accumulators stored to the workspace P (D, Mc, ldp), ldp = N rounded up to 256 (the
//                            columns past N hold zeros).
//   predict_cov_tile_kernel  one workgroup per (128 rows of Xa, 128 points of Xb, output a), a wave per 64 x 64 quadrant: the k
//                            loop walks the memory points in steps of 16, stages the 128 x 16 tile of P in LDS (the next one loaded
//                            under the MFMAs) and builds the 16 x 128 tile of K*_a(Xb)^T on the fly; P K*^T accumulates on
//                            v_mfma_f64_16x16x4_f64.  The epilogue subtracts it from the prior term of the two query points.
//   predict_cov_sym_kernel   joint form only, in place on the output: per pair of 32 x 32 tiles (I, J), (J, I) the average
//                            1/2 (t_ij + t_ji) goes to both places, the noise onto the diagonal.
// Every sum of an element runs over the memory points in an order fixed by N alone (k steps of 16, four points per MFMA): its bits
// depend on its two points only -- not on Ma / Mb, on where the points sit, on their neighbours or on the row chunks.  No atomics.
// Ma is processed in chunks of Mc rows so the workspace (D Mc ldp doubles) stays within kCovWsBudget, or one 64-row tile's need.
#include "device_common.h"

namespace gpmpc_hip {

namespace {

constexpr int kBM = 64;                  // rows of Xa per workgroup of the P kernel
constexpr int kBN = 256;                 // columns of iK per workgroup (64 per wave)
constexpr int kBK = 16;                  // memory points per k step
constexpr int kAPitch = kBM + 16;        // LDS row pitch (doubles) of the K* tile, stored [k][row]: rows 32 banks apart
constexpr int kBPitch = kBN + 16;        // ... and of the iK tile [k][column]
constexpr int kTM = 128;                 // rows of Xa / points of Xb per workgroup of the tile kernel (64 x 64 per wave)
constexpr int kTPitch = kTM + 16;        // LDS row pitch of its P tile [k][row] and K*(Xb) tile [k][point]
constexpr int kSym = 32;                 // tile edge of the symmetrisation
constexpr size_t kCovWsBudget = (size_t)256 << 20;  // bytes of P per chunk of rows (N = 4096, D = 16: 512 rows, so that a chunk's
                                                    // tile launch has 512 workgroups; one 64-row tile needs 32 MB there)

struct CovArgs {
    const double* Xa;        // (rows, E) this chunk's rows of Xa
    const double* Xb;        // (Mb, E)
    const double* Xt;        // (E, N)
    const double* ils2;      // (D, E)
    const double* var;       // (D)
    const double* iK;        // (D, N, N)
    double* P;               // (D, Mc, ldp)
    double* out;             // (D, Ma, Mb), at this chunk's first row
    size_t out_stride;       // Ma * Mb
    int rows, Mb, N, E, D, Mc, ldp;
};

struct CovSymArgs {
    double* out;             // (D, M, M)
    int M;
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

// P = K*_a(Xa) iK_a for 64 rows and 256 columns: the k loop of predict_tile_kernel (predict.hip keeps its own copy, so that
// gpmpc_predict's code is unchanged); the accumulators go to the workspace instead of being reduced.
template <int EP>
__global__ __launch_bounds__(256) void predict_cov_p_kernel(CovArgs p) {
    __shared__ double s_xq[kBM][EP + 1];
    __shared__ double s_A[kBK][kAPitch];
    __shared__ double s_B[kBK][kBPitch];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int m0 = blockIdx.x * kBM;                 // first row of the tile (within the chunk)
    const int j0 = blockIdx.y * kBN;
    const int a = blockIdx.z;
    const int N = p.N, E = p.E;
    const double sig2 = p.var[a];
    double il[EP];
#pragma unroll
    for (int e = 0; e < EP; ++e) il[e] = (e < E) ? p.ils2[a * E + e] : 0.0;
    for (int idx = tid; idx < kBM * EP; idx += 256) {
        const int r = idx / EP, e = idx - r * EP;
        s_xq[r][e] = (e < E && m0 + r < p.rows) ? p.Xa[(size_t)(m0 + r) * E + e] : 0.0;
    }
    __syncthreads();

    d4 acc[4][4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = d4{0.0, 0.0, 0.0, 0.0};

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

    // f64 C/D layout -- acc[rt][ct][r] = P[16 rt + (lane >> 4) + 4 r][64 w + 16 ct + (lane & 15)]; columns past N hold 0
    double* Pa = p.P + (size_t)a * p.Mc * p.ldp;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = m0 + 16 * rt + (lane >> 4) + 4 * r;
            if (row < p.rows) {
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
                    Pa[(size_t)row * p.ldp + j0 + 64 * w + 16 * ct + (lane & 15)] = acc[rt][ct][r];
            }
        }
}

// t_a(xa_i, xb_j) for 128 rows of the chunk and 128 points of Xb; wave w owns the quadrant (64 (w >> 1), 64 (w & 1)).
template <int EP>
__global__ __launch_bounds__(256, 2) void predict_cov_tile_kernel(CovArgs p) {
    __shared__ double s_xb[kTM][EP + 1];
    __shared__ double s_A[kBK][kTPitch];             // P tile [k][row]
    __shared__ double s_B[kBK][kTPitch];             // K*_a(Xb) tile [k][point of Xb]

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wr = 64 * (w >> 1), wc = 64 * (w & 1);
    const int m0 = blockIdx.x * kTM;                 // first row of the tile (within the chunk)
    const int c0 = blockIdx.y * kTM;                 // first point of Xb
    const int a = blockIdx.z;
    const int N = p.N, E = p.E;
    const double sig2 = p.var[a];
    double il[EP];
#pragma unroll
    for (int e = 0; e < EP; ++e) il[e] = (e < E) ? p.ils2[a * E + e] : 0.0;
    for (int idx = tid; idx < kTM * EP; idx += 256) {
        const int c = idx / EP, e = idx - c * EP;
        s_xb[c][e] = (e < E && c0 + c < p.Mb) ? p.Xb[(size_t)(c0 + c) * E + e] : 0.0;
    }

    d4 acc[4][4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = d4{0.0, 0.0, 0.0, 0.0};

    const double* Pa = p.P + (size_t)a * p.Mc * p.ldp;
    // staging map: P elements (rows gr + 16 q, point gi); K* elements (points of Xb gr + 16 q, memory point gi)
    const int gi = tid & 15, gr = tid >> 4;
    const int nk = (N + kBK - 1) / kBK;              // nk kBK <= ldp: the columns of P past N hold zeros
    double areg[8];
    auto load_a = [&](int i0) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int row = m0 + gr + 16 * q;
            areg[q] = (row < p.rows) ? Pa[(size_t)row * p.ldp + i0 + gi] : 0.0;
        }
    };
    load_a(0);
    for (int ks = 0; ks < nk; ++ks) {
        const int i0 = ks * kBK;
        __syncthreads();                         // s_xb is staged / the previous step's MFMAs have read s_A / s_B
#pragma unroll
        for (int q = 0; q < 8; ++q) s_A[gi][gr + 16 * q] = areg[q];
        {
            const int i = i0 + gi;
            double xi[EP];
#pragma unroll
            for (int e = 0; e < EP; ++e) xi[e] = (e < E && i < N) ? p.Xt[(size_t)e * N + i] : 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int c = gr + 16 * q;
                s_B[gi][c] = (i < N) ? kstar<EP>(s_xb[c], xi, il, sig2) : 0.0;
            }
        }
        __syncthreads();
        if (ks + 1 < nk) load_a(i0 + kBK);       // next P tile in flight under the MFMAs
#pragma unroll
        for (int s = 0; s < kBK / 4; ++s) {
            const int k = 4 * s + (lane >> 4);
            double av[4], bv[4];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) av[rt] = s_A[k][wr + 16 * rt + (lane & 15)];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) bv[ct] = s_B[k][wc + 16 * ct + (lane & 15)];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
                    acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[rt], bv[ct], acc[rt][ct], 0, 0, 0);
        }
    }

    // epilogue: acc[rt][ct][r] = (P K*^T)[wr + 16 rt + (lane >> 4) + 4 r][wc + 16 ct + (lane & 15)]; prior term minus it
    double* outa = p.out + (size_t)a * p.out_stride;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = m0 + wr + 16 * rt + (lane >> 4) + 4 * r;
            if (row >= p.rows) continue;
            double xa[EP];
#pragma unroll
            for (int e = 0; e < EP; ++e) xa[e] = (e < E) ? p.Xa[(size_t)row * E + e] : 0.0;
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const int c = wc + 16 * ct + (lane & 15);
                if (c0 + c < p.Mb) outa[(size_t)row * p.Mb + c0 + c] = kstar<EP>(s_xb[c], xa, il, sig2) - acc[rt][ct][r];
            }
        }
}

// Joint form, in place: workgroup (J, I, a) with I <= J reads the tiles (I, J) and (J, I) of T and writes 1/2 (t_ij + t_ji) to
// both (the sum of two doubles does not depend on their order); the noise goes onto the diagonal.
__global__ __launch_bounds__(256) void predict_cov_sym_kernel(CovSymArgs p) {
    __shared__ double s_U[kSym][kSym + 1];
    __shared__ double s_L[kSym][kSym + 1];
    const int tj = blockIdx.x, ti = blockIdx.y, a = blockIdx.z;
    if (ti > tj) return;
    const int M = p.M;
    double* T = p.out + (size_t)a * M * M;
    const int i0 = ti * kSym, j0 = tj * kSym;
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    for (int r = r0; r < kSym; r += 8) {
        s_U[r][c] = (i0 + r < M && j0 + c < M) ? T[(size_t)(i0 + r) * M + j0 + c] : 0.0;
        s_L[r][c] = (j0 + r < M && i0 + c < M) ? T[(size_t)(j0 + r) * M + i0 + c] : 0.0;
    }
    __syncthreads();
    const double nz = p.with_noise ? p.noise[a] : 0.0;
    for (int r = r0; r < kSym; r += 8) {
        if (i0 + r < M && j0 + c < M) {
            double v = 0.5 * (s_U[r][c] + s_L[c][r]);
            if (p.with_noise && i0 + r == j0 + c) v += nz;
            T[(size_t)(i0 + r) * M + j0 + c] = v;
        }
        if (ti != tj && j0 + r < M && i0 + c < M) T[(size_t)(j0 + r) * M + i0 + c] = 0.5 * (s_L[r][c] + s_U[c][r]);
    }
}

template <int EP>
void launch_cov(const CovArgs& p, hipStream_t s) {
    const dim3 gp((p.rows + kBM - 1) / kBM, p.ldp / kBN, p.D);
    hipLaunchKernelGGL((predict_cov_p_kernel<EP>), gp, dim3(256), 0, s, p);
    const dim3 gt((p.rows + kTM - 1) / kTM, (p.Mb + kTM - 1) / kTM, p.D);
    hipLaunchKernelGGL((predict_cov_tile_kernel<EP>), gt, dim3(256), 0, s, p);
}

}  // namespace

int run_predict_cov(Handle* h, const double* Xa, int Ma, const double* Xb, int Mb, const double* noises_host, double* out,
                    hipStream_t s) {
    const int N = h->N, D = h->D, E = h->E;
    const bool joint = Xb == nullptr;
    if (joint) { Xb = Xa; Mb = Ma; }
    if (Ma == 0 || Mb == 0) return GPMPC_OK;
    const int ldp = (N + kBN - 1) / kBN * kBN;
    // rows per chunk: a multiple of the P kernel's tile height, as many as the workspace budget allows, no more than Ma needs
    long long Mc = (long long)(kCovWsBudget / (sizeof(double) * (size_t)D * ldp)) / kBM * kBM;
    if (h->opt_predict_cov_chunk > 0) Mc = h->opt_predict_cov_chunk;
    if (Mc < kBM) Mc = kBM;
    const long long Mneed = ((long long)Ma + kBM - 1) / kBM * kBM;
    if (Mc > Mneed) Mc = Mneed;
    int rc = grow(h, h->covws, (size_t)D * (size_t)Mc * ldp);
    if (rc) return rc;
    CovArgs p{};
    p.Xb = Xb; p.Xt = h->Xt.p; p.ils2 = h->ils2.p; p.var = h->var.p; p.iK = h->iK.p;
    p.P = h->covws.p;
    p.out_stride = (size_t)Ma * Mb;
    p.Mb = Mb; p.N = N; p.E = E; p.D = D; p.Mc = (int)Mc; p.ldp = ldp;
    for (long long m0 = 0; m0 < Ma; m0 += Mc) {
        p.rows = (int)((Ma - m0) < Mc ? (Ma - m0) : Mc);
        p.Xa = Xa + (size_t)m0 * E;
        p.out = out + (size_t)m0 * Mb;
        if (E <= 4) launch_cov<4>(p, s);
        else if (E <= 8) launch_cov<8>(p, s);
        else if (E <= 16) launch_cov<16>(p, s);
        else launch_cov<24>(p, s);
    }
    if (joint) {
        CovSymArgs q{};
        q.out = out; q.M = Ma;
        q.with_noise = noises_host != nullptr;
        for (int a = 0; a < D; ++a) q.noise[a] = noises_host ? noises_host[a] : 0.0;
        const int nt = (Ma + kSym - 1) / kSym;
        hipLaunchKernelGGL(predict_cov_sym_kernel, dim3(nt, nt, D), dim3(256), 0, s, q);
    }
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

}  // namespace gpmpc_hip
