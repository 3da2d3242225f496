// moments_common.h -- the pieces gpmpc_moments (moments.hip) and gpmpc_moments_backward (moments_backward.hip) share: the
// argument block, the pair numbering and the per-(point, problem) setup kernel (C_a^-1 | log det B_a, Q_ab | log det R_ab and,
// for the backward, A_ab^-1).  See the moments.hip header for the notation.
#pragma once
#include "device_common.h"

namespace gpmpc_hip {

namespace {

constexpr int kTile = 64;                       // rows / columns of a pair tile
constexpr int kWaves = 4;                       // wavefronts of a pair-pass / point-pass workgroup
constexpr int kLdsE = kMaxE + 1;                // LDS row pitch of the setup kernel's E x E matrices
constexpr size_t kWsBudget = (size_t)32 << 20;  // bytes of workspace (setup results + pair partials) per chunk of points

struct MomentsArgs {
    const double* Xt;        // (E, N)
    const double* ils2;      // (D, E)  1 / l^2
    const double* var;       // (D)     sigma2
    const double* logvar;    // (D)
    const double* beta;      // (D, N)
    const double* Tm;        // (D, N + kTPad, N)    beta beta^T - iK, upper triangle, diagonal halved
    const double* mu;        // (P, E) of this chunk
    const double* Sig;       // (P, E, E) of this chunk, or NULL (= 0)
    double* setup;           // (Pc, D + npairs, E * E + 1): C_a^-1 | log det B_a, then Q_ab | log det R_ab
    double* ainv;            // (Pc, npairs, E * E): A_ab^-1 = (I + Lambda_ab^1/2 Sigma Lambda_ab^1/2)^-1, or NULL (forward)
    double* part;            // (Pc, npairs, nt * nt, kWaves) pair partial sums
    double* M_out;           // (P, D) of this chunk
    double* S_out;           // (P, D, D) of this chunk, or NULL
    double* V_out;           // (P, E, D) of this chunk, or NULL
    int rows;                // points in this chunk
    int N, D, E, npairs, nt, tpad;
    int nprob;               // setup problems per point: D, or D + npairs with S
};

__host__ __device__ inline size_t setup_stride(int E) { return (size_t)E * E + 1; }

// ----------------------------------------------------------------------------------------------------------------------------
// Setup: one wavefront per (point, problem).
__global__ __launch_bounds__(64) void moments_setup_kernel(MomentsArgs p) {
    __shared__ double s_A[kMaxE][kLdsE];      // the SPD matrix, then its Cholesky factor L (lower)
    __shared__ double s_Li[kMaxE][kLdsE];     // L^-1 (lower)
    __shared__ double s_d[kMaxE];             // scaling of Sigma's rows / columns
    const int lane = threadIdx.x;
    const int pt = blockIdx.x / p.nprob, prob = blockIdx.x - pt * p.nprob;
    const int E = p.E, D = p.D;
    const double* Sg = p.Sig ? p.Sig + (size_t)pt * E * E : nullptr;
    const bool pairp = prob >= D;
    int a = prob, b = prob;
    if (pairp) decode_tri(prob - D, D, a, b);
    if (lane < E) s_d[lane] = pairp ? sqrt(p.ils2[a * E + lane] + p.ils2[b * E + lane]) : sqrt(p.ils2[a * E + lane]);
    __syncthreads();
    // A = D Sigma D + I  (B_a with D = 1/l_a; I + G with D = Lambda_ab^1/2)
    for (int idx = lane; idx < E * E; idx += 64) {
        const int r = idx / E, c = idx - r * E;
        const double sv = Sg ? Sg[idx] : 0.0;
        s_A[r][c] = s_d[r] * sv * s_d[c] + (r == c ? 1.0 : 0.0);
    }
    __syncthreads();
    // Cholesky, right-looking (lower triangle)
    for (int k = 0; k < E; ++k) {
        const double dk = sqrt(s_A[k][k]);
        __syncthreads();
        if (lane == 0) s_A[k][k] = dk;
        for (int r = k + 1 + lane; r < E; r += 64) s_A[r][k] /= dk;
        __syncthreads();
        const int m = E - k - 1;
        for (int idx = lane; idx < m * m; idx += 64) {
            const int r = k + 1 + idx / m, c = k + 1 + idx % m;
            if (c <= r) s_A[r][c] -= s_A[r][k] * s_A[c][k];
        }
        __syncthreads();
    }
    // L^-1, one column per lane (forward substitution)
    if (lane < E) {
        const int j = lane;
        for (int i = 0; i < E; ++i) {
            double v = (i == j) ? 1.0 : 0.0;
            if (i < j) { s_Li[i][j] = 0.0; continue; }
            for (int k = j; k < i; ++k) v -= s_A[i][k] * s_Li[k][j];
            s_Li[i][j] = v / s_A[i][i];
        }
    }
    __syncthreads();
    double* out = p.setup + ((size_t)pt * p.nprob + prob) * setup_stride(E);
    if (lane == 0) {
        double ld = 0.0;
        for (int k = 0; k < E; ++k) ld += log(s_A[k][k]);
        out[E * E] = 2.0 * ld;                           // log det B_a  or  log det R_ab
    }
    if (!pairp) {
        for (int idx = lane; idx < E * E; idx += 64) out[idx] = s_Li[idx / E][idx % E];
        return;
    }
    if (p.ainv) {                                         // A^-1 = L^-T L^-1 (the backward's adjoints of Q and log det R)
        double* ai = p.ainv + ((size_t)pt * p.npairs + (prob - D)) * E * E;
        for (int idx = lane; idx < E * E; idx += 64) {
            const int r = idx / E, c = idx - r * E;
            double v = 0.0;
            for (int k = r > c ? r : c; k < E; ++k) v = fma(s_Li[k][r], s_Li[k][c], v);
            ai[idx] = v;
        }
    }
    // Y = A^-1 G = L^-T (L^-1 G), one column of G per lane; G = A - I off the diagonal, A_jj - 1 on it (rebuilt from Sigma)
    double y[kMaxE];
    if (lane < E) {
        const int j = lane;
        double w[kMaxE];
#pragma unroll
        for (int i = 0; i < kMaxE; ++i) {
            double v = 0.0;
            if (i < E)
                for (int k = 0; k <= i; ++k) {
                    const double g = Sg ? s_d[k] * Sg[k * E + j] * s_d[j] : 0.0;
                    v = fma(s_Li[i][k], g, v);
                }
            w[i] = v;
        }
#pragma unroll
        for (int i = kMaxE - 1; i >= 0; --i) {
            double v = 0.0;
            if (i < E)
#pragma unroll
                for (int k = kMaxE - 1; k >= 0; --k)
                    if (k >= i && k < E) v = fma(s_Li[k][i], w[k], v);
            y[i] = v;
        }
    }
    __syncthreads();                                      // everybody is done with s_A
    if (lane < E) {
#pragma unroll
        for (int i = 0; i < kMaxE; ++i)
            if (i < E) s_A[i][lane] = y[i];
    }
    __syncthreads();
    // Q = 1/2 Lambda^-1/2 sym(Y) Lambda^-1/2
    for (int idx = lane; idx < E * E; idx += 64) {
        const int r = idx / E, c = idx - r * E;
        out[idx] = 0.25 * (s_A[r][c] + s_A[c][r]) / (s_d[r] * s_d[c]);
    }
}

}  // namespace

}  // namespace gpmpc_hip
