// small_factor.h -- the phases of a whole small factorisation (N <= 256) by ONE workgroup of 1024 threads, as __device__ functions:
// Gram matrix, blocked Cholesky, triangular inverse, beta and Y^T Y, as prepare_small_kernel (prepare_small.hip) runs them for the
// cached model, here for mll_batch_kernel (mll_batch.hip: the batched training loss) on its own operands.  prepare_small_kernel
// keeps its own text: built from these functions it was 2.7 % slower at config 2 (0.2144 against 0.2088 ms on one device, the two
// builds alternating; 54 spilled VGPRs against 46), DESIGN.md section 4.6.2.  A change to a phase there belongs here too.
// Every function is called by all 1024 threads of the workgroup; each says which barrier it ends with.  What bounds the
// factorisation, and why the pivot loop looks the way it does, is told at the head of prepare_small.hip.
#pragma once
#include "device_common.h"

namespace gpmpc_hip {

constexpr int kSB = 32;            // panel width (prepare_small.hip has its own copy of these two)
constexpr int kSmallMaxN = 256;

// LDS of the phases, in doubles from the start of the dynamic segment
struct SmallLds {
    double* xs;        // (N, E | 1) inputs scaled by 1 / l_a (P1)
    double* Lp;        // P2: (N - k0 + 32, 33) panel + 32 identity rows (xs is dead by then)
    double* colb;      // 2 x (N + 32) current / next pivot column
    double* sinv;      // (32) 1 / L_kk of the panel
    double* Yt;        // (32, 33) L11^-T of the panel
};
constexpr size_t kSmallLdsP2 = (size_t)(kSmallMaxN + kSB) * 33 + 2 * (kSmallMaxN + kSB) + kSB + kSB * 33;
__host__ __device__ inline size_t small_lds_doubles(int N, int E) {
    const size_t lds_a = (size_t)((N * (E | 1) + 1) & ~1);                                      // P1: scaled inputs
    return lds_a > kSmallLdsP2 ? lds_a : kSmallLdsP2;                                           // P2: panel, pivot columns, 1 / L_kk, L11^-T
}
__device__ inline SmallLds small_lds(double* sm) {
    SmallLds l;
    l.xs = sm;
    l.Lp = sm;
    l.colb = l.Lp + (kSmallMaxN + kSB) * 33;
    l.sinv = l.colb + 2 * (kSmallMaxN + kSB);
    l.Yt = l.sinv + kSB;
    return l;
}

// cycle counts of the parts of P2 (GPMPC_PROF_ON builds only)
struct SmallCholProf { long long potrf = 0, trsm = 0, trail = 0; };

// ---- scaled inputs: xs[pt, e] = X[pt, e] * sqrt(1 / l_e^2), the same x * sqrt(1 / l^2) as gram_kernel of prepare.hip; row stride
// E | 1 (odd: conflict-free column reads).  No barrier.
__device__ inline void small_scale_inputs(const double* __restrict__ X, const double* ls, int N, int E, double* xs, int tid) {
    const int ES = E | 1;
    for (int idx = tid; idx < N * E; idx += 1024) {
        const int pt = idx / E, e = idx - pt * E;
        const double l = ls[e];
        xs[pt * ES + e] = X[idx] * sqrt(1.0 / (l * l));
    }
}

// ---- P1: Gram matrix, lower triangle (gp_model.py:425,427); Y := 0.  No barrier.
__device__ inline void small_gram(const double* xs, double va, double nz, int N, int E, double* __restrict__ K,
                                  double* __restrict__ Yv, int tid) {
    const int lane = tid & 63, wave = tid >> 6, ES = E | 1;
    for (int i = wave; i < N; i += 16) {
        for (int j = lane; j <= i; j += 64) {
            double s = 0.0;
            for (int e = 0; e < E; ++e) { const double d = xs[i * ES + e] - xs[j * ES + e]; s = fma(d, d, s); }
            double v = va * exp(-0.5 * s);
            if (i == j) v += nz;
            K[(size_t)i * N + j] = v;
        }
    }
    for (int idx = tid; idx < N * N; idx += 1024) Yv[idx] = 0.0;
}

// ---- P2: blocked LEFT-looking Cholesky, panel width 32 (gp_model.py:427) ------------------------------------------
// Per panel: (a) panel -= L[k0:, :k0] L[k0:k0+32, :k0]^T on the matrix cores (operands streamed from L2, 8 k-steps of
// loads in flight), result into LDS; (b) unblocked elimination of the 32 x 32 diagonal block in registers -- thread
// (row rr, column c) owns element (rr, c), a wavefront owns two columns and drops out once both are done -- with the
// pivot column handed on through LDS, one barrier per pivot.  The 32 x 32 identity rides along under the block: it
// comes out as L11^-T, which is both the panel solve (L21 = A21 L11^-T, a product on the matrix cores with both
// operands in LDS) and the inverse of the diagonal block the row-block recursion of P3 needs.
// L replaces the lower triangle of K; the inverted diagonal blocks go to Yv.  `lost(pivot, order)` is called by ONE thread per
// pivot, with a barrier between two calls: it records a pivot that is not positive (the elimination goes on regardless: no loop
// bound and no barrier depends on the data).  Ends with a barrier.
template <int UP = 8, typename Lost>
__device__ inline void small_cholesky(double* __restrict__ K, double* __restrict__ Yv, int N, const SmallLds& l, Lost lost, int tid,
                                      SmallCholProf& prof) {
    const int lane = tid & 63, wave = tid >> 6;
    double* Lp = l.Lp;
    double* colb = l.colb;
    double* sinv = l.sinv;
    double* Yt = l.Yt;
    const int c32 = tid >> 5, r32 = tid & 31;                // column-major over the wavefronts: wave w <-> columns 2w, 2w + 1
    const int li = lane & 15, lk = lane >> 4;
    for (int k0 = 0; k0 < N; k0 += kSB) {
        const int nb = (N - k0 < kSB) ? (N - k0) : kSB;
        const int nr = N - k0;                               // rows of the panel
#ifdef GPMPC_PROF_ON
        const long long tp0 = __builtin_readcyclecounter();
#endif
        // (a) updated panel -> Lp
        {
            const int nrt = (nr + 15) >> 4;
            for (int t = wave; t < nrt; t += 16) {
                const int i0 = k0 + t * 16;
                d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
                double c0v[4], c1v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {                // the Gram values of this tile (lower triangle only is defined)
                    const int row = i0 + lk + 4 * r;
                    const bool in0 = row < N && li < nb && k0 + li <= row, in1 = row < N && 16 + li < nb && k0 + 16 + li <= row;
                    c0v[r] = in0 ? K[(size_t)row * N + k0 + li] : 0.0;
                    c1v[r] = in1 ? K[(size_t)row * N + k0 + 16 + li] : 0.0;
                }
                if (k0 > 0) {
                    const int ra = (i0 + li < N) ? i0 + li : N - 1;
                    const int rb0 = (li < nb) ? k0 + li : k0, rb1 = (16 + li < nb) ? k0 + 16 + li : k0;
                    const double* Ar = K + (size_t)ra * N;
                    const double* B0 = K + (size_t)rb0 * N;
                    const double* B1 = K + (size_t)rb1 * N;
                    constexpr int U = UP;
                    static_assert(kSB % (4 * U) == 0, "k0 is a multiple of 32: whole groups of U k-steps");
                    for (int pp = 0; pp < k0; pp += 4 * U) {
                        double av[U], b0[U], b1[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) { const int pk = pp + 4 * u + lk; av[u] = Ar[pk]; b0[u] = B0[pk]; b1[u] = B1[pk]; }
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], b0[u], acc0, 0, 0, 0);
                            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], b1[u], acc1, 0, 0, 0);
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int lr = t * 16 + lk + 4 * r;      // row inside the panel
                    Lp[lr * 33 + li] = c0v[r] - acc0[r];
                    Lp[lr * 33 + 16 + li] = c1v[r] - acc1[r];
                }
            }
        }
        __syncthreads();
#ifdef GPMPC_PROF_ON
        const long long tp1 = __builtin_readcyclecounter();
        prof.potrf += tp1 - tp0;
#endif
        // (b) elimination of the diagonal block (element (rr, c)) and of the identity under it (element (32 + rr, c))
        double a0 = (r32 < nb && c32 < nb && c32 <= r32) ? Lp[r32 * 33 + c32] : 0.0;
        double a1 = (r32 == c32) ? 1.0 : 0.0;
        if (c32 == 0) { colb[r32] = a0; colb[kSB + r32] = a1; }
        if (tid == 0) {
            lost(a0, k0 + 1);
            sinv[0] = inv_sqrt_pos(a0);
        }
        if (tid >= nb && tid < kSB) sinv[tid] = 0.0;
        __syncthreads();
        for (int k = 0; k + 1 < nb; ++k) {
            if (2 * wave + 1 > k) {                          // wave-uniform: both columns of a finished wave are final
                const double* cb = colb + (k & 1) * (kSmallMaxN + kSB);
                double* cn = colb + ((k + 1) & 1) * (kSmallMaxN + kSB);
                const double inv = sinv[k];
                if (c32 > k && c32 < nb) {
                    const double lc = cb[c32] * inv;
                    a0 = fma(-(cb[r32] * inv), lc, a0);
                    a1 = fma(-(cb[kSB + r32] * inv), lc, a1);
                    if (c32 == k + 1) {
                        cn[r32] = a0;
                        cn[kSB + r32] = a1;
                        if (r32 == k + 1) {
                            lost(a0, k0 + k + 2);
                            sinv[k + 1] = inv_sqrt_pos(a0);
                        }
                    }
                }
            }
            __syncthreads();
        }
#ifdef GPMPC_PROF_ON
        const long long tp2 = __builtin_readcyclecounter();
        prof.trsm += tp2 - tp1;
#endif
        // scale on the way out: L_rc = value / L_cc; the identity rows are L11^-T (row m, column c = Y11[c][m])
        {
            const double sc = sinv[c32];                     // 0 for c >= nb
            const double lv = (c32 <= r32) ? a0 * sc : 0.0, y = (r32 <= c32) ? a1 * sc : 0.0;
            Yt[r32 * 33 + c32] = y;
            if (r32 < nb && c32 <= r32) K[(size_t)(k0 + r32) * N + k0 + c32] = lv;
            if (r32 < nb && c32 < nb) Yv[(size_t)(k0 + c32) * N + k0 + r32] = y;
        }
        __syncthreads();
        // panel solve on the matrix cores: L21 = A21 L11^-T, A21 = rows 32.. of Lp, B[k][j] = Yt[k][j]
        {
            const int M = nr - nb;
            const int nrt = (M + 15) >> 4;
            for (int t = wave; t < 2 * nrt; t += 16) {
                const int i0 = (t >> 1) * 16, j0 = (t & 1) * 16;
                d4 acc = {0.0, 0.0, 0.0, 0.0};
                const double* Ar = Lp + (size_t)(nb + i0 + li) * 33;
#pragma unroll
                for (int kk = 0; kk < kSB; kk += 4)
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ar[kk + lk], Yt[(kk + lk) * 33 + j0 + li], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = i0 + lk + 4 * r, col = j0 + li;
                    if (row < M && col < nb) K[(size_t)(k0 + nb + row) * N + k0 + col] = acc[r];
                }
            }
        }
        __syncthreads();
#ifdef GPMPC_PROF_ON
        prof.trail += __builtin_readcyclecounter() - tp2;
#endif
    }
}

// ---- P3: Y = L^-1 by row blocks: Y[k, c] = -Ykk (L[k, :k] Y[:k, c]) for c < k; W: scratch of 32 x (N - 32) doubles in global
// memory.  Ends with a barrier (none at all for N <= 32).
template <int U = 16>
__device__ inline void small_trinv(const double* __restrict__ K, double* __restrict__ Yv, double* __restrict__ W, int N, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    for (int k0 = kSB; k0 < N; k0 += kSB) {
        const int nb = (N - k0 < kSB) ? (N - k0) : kSB;
        const int nct = k0 >> 4;                               // column tiles of 16 (k0 is a multiple of 32)
        // W = L[k, 0:k0] Y[0:k0, 0:k0] (32 x k0, row stride k0)
        for (int t = wave; t < 2 * nct; t += 16) {
            const int i0 = (t & 1) * 16, c0 = (t >> 1) * 16;
            d4 acc = {0.0, 0.0, 0.0, 0.0};
            const bool rowin = (i0 + li < nb);
            const double* Arow = K + (size_t)(k0 + (rowin ? i0 + li : 0)) * N;
            const double* Bcol = Yv + c0 + li;
            mfma_kloop<U>(acc, c0, k0, lk,                                              // Y[p][c] = 0 for p < c
                          [&](int pk) { return rowin ? Arow[pk] : 0.0; },
                          [&](int pk) { return Bcol[(size_t)pk * N]; });
#pragma unroll
            for (int r = 0; r < 4; ++r) W[(size_t)(i0 + lk + 4 * r) * k0 + c0 + li] = acc[r];
        }
        __syncthreads();
        // Y[k, c] = -Ykk W   (Ykk = the block's inverse of P2b; lower triangular)
        for (int t = wave; t < 2 * nct; t += 16) {
            const int i0 = (t & 1) * 16, c0 = (t >> 1) * 16;
            d4 acc = {0.0, 0.0, 0.0, 0.0};
            const bool rowin = (i0 + li < nb);
            const double* Arow = Yv + (size_t)(k0 + (rowin ? i0 + li : 0)) * N + k0;
            const double* Bcol = W + c0 + li;
            mfma_kloop<8>(acc, 0, kSB, lk,
                          [&](int m) { return (rowin && m < nb) ? Arow[m] : 0.0; },
                          [&](int m) { return Bcol[(size_t)m * k0]; });
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i0 + lk + 4 * r;
                if (row < nb) Yv[(size_t)(k0 + row) * N + c0 + li] = -acc[r];
            }
        }
        __syncthreads();
    }
}

// ---- P4: z = Y y, beta = Y^T z (= cholesky_solve(y, L), gp_model.py:429-430); y[q] = ycol[q * ystride].  Ends with a barrier.
__device__ inline void small_beta(const double* __restrict__ Yv, const double* __restrict__ ycol, int ystride, int N,
                                  double* __restrict__ zv, double* __restrict__ be, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    for (int row = wave; row < N; row += 16) {
        double s = 0.0;
        for (int q = lane; q <= row; q += 64) s = fma(Yv[(size_t)row * N + q], ycol[(size_t)q * ystride], s);
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) zv[row] = s;
    }
    __syncthreads();
    {
        // four threads per column (rows q = i + part, i + part + 4, ...), partial sums combined in a fixed order;
        // loads of 8 rows in flight
        const int i = tid >> 2, part = tid & 3;
        double s = 0.0;
        if (i < N) {
            for (int q0 = i + part; q0 < N; q0 += 32) {
                double yv[8], zz[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int q = q0 + 4 * u;
                    yv[u] = (q < N) ? Yv[(size_t)q * N + i] : 0.0;
                    zz[u] = (q < N) ? zv[q] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) s = fma(yv[u], zz[u], s);
            }
        }
        const double s1 = __shfl_xor(s, 1, 64);
        const double pair = (part & 1) ? s1 + s : s + s1;
        const double s2 = __shfl_xor(pair, 2, 64);
        if (i < N && part == 0) be[i] = pair + s2;
    }
    __syncthreads();
}

// ---- P5: iK = Y^T Y (gp_model.py:428) by 16 x 16 tiles of the lower triangle dealt to the wavefronts: store(row, col, value) is
// called once for every col <= row < N.  No barrier.
template <int U = 16, typename Store>
__device__ inline void small_syrk_lower(const double* __restrict__ Yv, int N, int tid, Store store) {
    const int lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int nt = (N + 15) >> 4;
    const int ntri = nt * (nt + 1) / 2;
    for (int t = wave; t < ntri; t += 16) {
        int ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
        while (ti * (ti + 1) / 2 > t) --ti;
        while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
        const int tj = t - ti * (ti + 1) / 2;
        const int i0 = ti * 16, j0 = tj * 16;              // j0 <= i0
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        const int ci = (i0 + li < N) ? i0 + li : N - 1, cj = (j0 + li < N) ? j0 + li : N - 1;    // clamped: masked on store
        mfma_kloop<U>(acc, i0, N, lk,                                                              // Y[p][c] = 0 for p < c
                      [&](int pk) { return Yv[(size_t)pk * N + ci]; },
                      [&](int pk) { return Yv[(size_t)pk * N + cj]; });
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = i0 + lk + 4 * r, col = j0 + li;
            if (row < N && col < N && col <= row) store(row, col, acc[r]);
        }
    }
}

}  // namespace gpmpc_hip
