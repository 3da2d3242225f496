// moments_backward.hip -- reverse-mode product of gpmpc_moments (gpmpc_moments_backward): for P independent Gaussian inputs
// N(m_p, Sigma_p) and upstream gradients Mb (D), Sb (D, D), Vb (E, D) per point, the gradients mb (E) and Sigmab (E, E) of
// <Mb, M> + <Sb, S> + <Vb, V>: what torch autograd through predict_next_state_change (gp_model.py:112-180) gives, with
// Sigmab the symmetric part (the only part a symmetric dSigma sees).  Notation of moments.hip.
//
// Maths ("Gradients of moment matching"):
//   S = S_raw - M M^T folds into an effective mean gradient  Mbe = Mb - (Sb + Sb^T) M.
//   Mean / V part, per output a (s = 1/l_a, u_i = s o (x_i - m), y = B^-1 (s o Vb[:, a]), c = c_a):
//     sums S0 = sum lb_i, S1 = sum lb_i u_i, S2 = sum lb_i u_i u_i^T, S3 = sum lb_i (y.u_i) u_i u_i^T
//     mb += c s o (B^-1 (Mbe S1 + S2 y) - S0 y)
//     Sigmab += diag(s) [ -1/2 L B^-1 + 1/2 c B^-1 (Mbe S2 + S3) B^-1 - 1/2 c (y t^T + t y^T) ] diag(s),
//     L = c (Mbe S0 + y.S1),  t = B^-1 S1.
//   Pair part, per pair a <= b with weight g = Sb_ab + Sb_ba (a != b) or Sb_aa, w_ij = T_ab(i,j) exp(e_ij), p_ij = z_ai + z_bj,
//   W = sum w, P1 = sum w p, P2 = sum w p p^T, R^-1 = Lambda^-1/2 A^-1 Lambda^1/2 (A = I + Lambda^1/2 Sigma Lambda^1/2),
//   f = g / sqrt(det R):
//     mb += f R^-T P1                                     (d e_ij / dm = (I - 2 Lambda Q) p_ij = R^-T p_ij)
//     Sigmab += f/2 (R^-T P2 R^-1 - W Lambda^1/2 A^-1 Lambda^1/2)      (dQ = 1/2 R^-1 dSigma R^-T; d log det R)
//   P2 = sum_i r_i z_ai z_ai^T + sum_j c_j z_bj z_bj^T + sum_i (z_ai Y_i^T + Y_i z_ai^T), r / c the row / column sums of w and
//   Y_i = sum_j w_ij z_bj, so the N^2 pass accumulates r_i, Y_i and c_j only.  Diagonal pairs sum the stored triangle (diagonal
//   halved) and double it, as the forward does.
//
// Kernels:
//   moments_setup_kernel  (moments_common.h) per (point, problem); with the pairs it also writes A_ab^-1.
//   mb_point_kernel       one workgroup per (point, output): S0, S1 in registers (the forward's order), y; the two weighted second
//                         moments over rows staged in LDS, one (entry, row slice) per thread, slices added in order.
//   mb_pair_kernel        one workgroup per (point, pair, 64-row tile): sweeps the column tiles (those on and right of the
//                         diagonal for a = b); per element the forward's one exp, then the row sums and Y_i in registers and
//                         the column sums reduced and contracted per column tile; after the sweep the row side is contracted.
//                         Writes one (W, P1, P2) partial per (point, pair, row tile).
//   mb_finish_kernel      one workgroup per point: M, Mbe, then every output and every pair in a fixed order, E x E algebra in
//                         LDS; writes sym(Sigmab) and mb.
// Every sum has an order fixed by N, E and D alone and there are no atomics: a point's results are bitwise the same whatever P
// is, wherever it sits and however the batch is chunked.  Points are chunked so the workspace stays within 32 MB (or one point's
// need when that is more).
#include "moments_common.h"
#include "device_common.h"

namespace gpmpc_hip {

namespace {

constexpr int kRows = 256;      // rows staged per step of the point pass

struct BackArgs {
    MomentsArgs f;           // mu, Sig, setup, ainv and the model of this chunk (f.M_out / S_out / V_out unused)
    const double* Mb;        // (P, D) of this chunk, or NULL (= 0)
    const double* Sb;        // (P, D, D) of this chunk, or NULL (= 0: no pair work at all)
    const double* Vb;        // (P, E, D) of this chunk, or NULL (= 0)
    double* psum;            // (Pc, D, psum_stride): S0 | S1 (E) | y (E) | S2 (E x E) | S3 (E x E)
    double* ppart;           // (Pc, npairs, nt, pp_stride): P2 (E x E) | P1 (E) | W
    double* mb_out;          // (P, E) of this chunk, or NULL
    double* vb_out;          // (P, E, E) of this chunk, or NULL
};

__host__ __device__ inline size_t psum_stride(int E) { return 1 + 2 * (size_t)E + 2 * (size_t)E * E; }
__host__ __device__ inline size_t pp_stride(int E) { return (size_t)E * E + E + 1; }

// ----------------------------------------------------------------------------------------------------------------------------
// O(N) pass: one workgroup per (point, output a).
template <int EP>
__global__ __launch_bounds__(256) void mb_point_kernel(BackArgs q) {
    const MomentsArgs& p = q.f;
    __shared__ double s_Ci[EP * EP];
    __shared__ double s_red[kWaves][EP + 1];
    __shared__ double s_tab[64];
    __shared__ double s_m[EP], s_il[EP], s_y[EP];
    __shared__ double s_u[EP][kRows];         // staged u_i of one step
    __shared__ double s_lb[2][kRows];         // lb_i, lb_i (y.u_i)
    __shared__ double s_acc[2][kRows + 64];   // per-(slice, entry) partials of S2, S3
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int pt = blockIdx.x / p.D, a = blockIdx.x - pt * p.D;
    const int E = p.E, N = p.N, D = p.D;
    const double* su = p.setup + ((size_t)pt * p.nprob + a) * setup_stride(E);
    double* ps = q.psum + ((size_t)pt * D + a) * psum_stride(E);
    for (int idx = tid; idx < EP * EP; idx += 256) {
        const int r = idx / EP, c = idx - r * EP;
        s_Ci[idx] = (r < E && c < E) ? su[r * E + c] : 0.0;
    }
    if (tid < 64) s_tab[tid] = kExp2Tab[tid];
    if (tid < EP) {
        s_m[tid] = tid < E ? p.mu[(size_t)pt * E + tid] : 0.0;
        s_il[tid] = tid < E ? sqrt(p.ils2[a * E + tid]) : 0.0;
    }
    __syncthreads();
    if (tid == 0) {                           // y = B^-1 (s o Vb[:, a]) = C^-T (C^-1 v)
        double v[EP], w[EP];
#pragma unroll
        for (int e = 0; e < EP; ++e) v[e] = (e < E && q.Vb) ? s_il[e] * q.Vb[((size_t)pt * E + e) * D + a] : 0.0;
#pragma unroll
        for (int r = 0; r < EP; ++r) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k <= r; ++k) t = fma(s_Ci[r * EP + k], v[k], t);
            w[r] = t;
        }
#pragma unroll
        for (int r = 0; r < EP; ++r) {
            double t = 0.0;
#pragma unroll
            for (int k = EP - 1; k >= r; --k) t = fma(s_Ci[k * EP + r], w[k], t);
            s_y[r] = t;
            if (r < E) ps[1 + E + r] = t;
        }
    }
    // second-moment ownership: (entry, row slice) per thread, or two entries per thread when there are more than 256
    const int nent = E * (E + 1) / 2;
    const int slices = nent <= 256 ? 256 / nent : 1;
    const int ent0 = nent <= 256 ? tid % nent : tid, slice = nent <= 256 ? tid / nent : 0;
    const bool own0 = slice < slices && ent0 < nent, own1 = nent > 256 && tid + 256 < nent;
    int e0 = 0, f0 = 0, e1 = 0, f1 = 0;
    if (own0) decode_tri(ent0, E, e0, f0);
    if (own1) decode_tri(tid + 256, E, e1, f1);
    double a2[2] = {0.0, 0.0}, a3[2] = {0.0, 0.0};
    __syncthreads();
    double s0 = 0.0, s1[EP];
#pragma unroll
    for (int e = 0; e < EP; ++e) s1[e] = 0.0;
    for (int c0 = 0; c0 < N; c0 += kRows) {
        const int i = c0 + tid;
        double u[EP], lb = 0.0, yu = 0.0;
#pragma unroll
        for (int e = 0; e < EP; ++e) u[e] = 0.0;
        if (i < N) {
            asm volatile("" ::: "memory");
#pragma unroll
            for (int e = 0; e < EP; ++e) u[e] = e < E ? (p.Xt[(size_t)e * N + i] - s_m[e]) * s_il[e] : 0.0;
            double qf = 0.0;
#pragma unroll
            for (int r = 0; r < EP; ++r) {
                double w = 0.0;
#pragma unroll
                for (int c = 0; c <= r; ++c) w = fma(s_Ci[r * EP + c], u[c], w);
                qf = fma(w, w, qf);
            }
            lb = fast_exp(-0.5 * qf, s_tab) * p.beta[(size_t)a * N + i];
            s0 += lb;
#pragma unroll
            for (int e = 0; e < EP; ++e) {
                s1[e] = fma(lb, u[e], s1[e]);
                yu = fma(s_y[e], u[e], yu);
            }
        }
#pragma unroll
        for (int e = 0; e < EP; ++e)
            if (e < E) s_u[e][tid] = u[e];
        s_lb[0][tid] = lb;
        s_lb[1][tid] = lb * yu;
        __syncthreads();
        const int cnt = min(kRows, N - c0);
        if (own0)
            for (int r = slice; r < cnt; r += slices) {
                const double uu = s_u[e0][r] * s_u[f0][r];
                a2[0] = fma(s_lb[0][r], uu, a2[0]);
                a3[0] = fma(s_lb[1][r], uu, a3[0]);
            }
        if (own1)
            for (int r = 0; r < cnt; ++r) {
                const double uu = s_u[e1][r] * s_u[f1][r];
                a2[1] = fma(s_lb[0][r], uu, a2[1]);
                a3[1] = fma(s_lb[1][r], uu, a3[1]);
            }
        __syncthreads();
    }
    // S0, S1: the 64 lanes (butterfly), then the 4 wavefronts in order -- the forward's order
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s0 += __shfl_xor(s0, off, 64);
#pragma unroll
        for (int e = 0; e < EP; ++e) s1[e] += __shfl_xor(s1[e], off, 64);
    }
    if (lane == 0) {
        s_red[wv][EP] = s0;
#pragma unroll
        for (int e = 0; e < EP; ++e) s_red[wv][e] = s1[e];
    }
    if (own0) { s_acc[0][slice * nent + ent0] = a2[0]; s_acc[1][slice * nent + ent0] = a3[0]; }
    if (own1) { s_acc[0][tid + 256] = a2[1]; s_acc[1][tid + 256] = a3[1]; }
    __syncthreads();
    if (tid == 0) {
        ps[0] = ((s_red[0][EP] + s_red[1][EP]) + s_red[2][EP]) + s_red[3][EP];
        for (int e = 0; e < E; ++e) ps[1 + e] = ((s_red[0][e] + s_red[1][e]) + s_red[2][e]) + s_red[3][e];
    }
    double* S2 = ps + 1 + 2 * E;
    double* S3 = S2 + E * E;
    for (int k = tid; k < nent; k += 256) {
        double v2 = 0.0, v3 = 0.0;
        for (int sl = 0; sl < slices; ++sl) { v2 += s_acc[0][sl * nent + k]; v3 += s_acc[1][sl * nent + k]; }
        int e, f;
        decode_tri(k, E, e, f);
        S2[e * E + f] = v2; S2[f * E + e] = v2;
        S3[e * E + f] = v3; S3[f * E + e] = v3;
    }
}

// ----------------------------------------------------------------------------------------------------------------------------
// Pair pass.  Lane map of the forward: wavefront w owns rows 16 w .. 16 w + 15 of a tile, lane l rows 16 w + 4 (l >> 4) + {0..3}
// and columns 4 (l & 15) + {0..3}.
template <int EP>
__global__ __launch_bounds__(256) void mb_pair_kernel(BackArgs q) {
    const MomentsArgs& p = q.f;
    __shared__ double s_za[EP][kTile];        // z_ai of the row tile
    __shared__ double s_g[EP][kTile];         // Q z_ai
    __shared__ double s_w[EP][kTile];         // 2 z_bj of the current column tile
    __shared__ double s_k[2][kTile];          // ka'_i, kb'_j
    __shared__ double s_c[kWaves][kTile];     // column sums per wavefront
    __shared__ double s_cs[kTile];            // column sums of the tile
    __shared__ double s_y[EP][kTile];         // after the sweep: 2 Y_i
    __shared__ double s_r[kTile];             //                  r_i
    __shared__ double s_tab[64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nt = p.nt, N = p.N, E = p.E, D = p.D;
    const int rt = blockIdx.x, pr = blockIdx.y, pt = blockIdx.z;
    int a, b;
    decode_tri(pr, D, a, b);
    const bool diag = a == b;
    const int r0 = rt * kTile;
    const int lr = 16 * wv + 4 * (lane >> 4), lc = 4 * (lane & 15);
    const bool rows_live = r0 + 16 * wv < N;
    const double* Q = p.setup + ((size_t)pt * p.nprob + D + pr) * setup_stride(E);
    const double* mu = p.mu + (size_t)pt * E;
    // side builder (the forward's): z, Q z (rows) or 2 z (columns), k'
    auto build = [&](int side, int i0, int idx) {
        const int o = side ? b : a, i = i0 + idx;
        const bool live = i < N;
        double z[EP], dz = 0.0;
#pragma unroll
        for (int e = 0; e < EP; ++e) {
            const double d = (e < E && live) ? p.Xt[(size_t)e * N + i] - mu[e] : 0.0;
            z[e] = e < E ? d * p.ils2[o * E + e] : 0.0;
            dz = fma(d, z[e], dz);
        }
        double zqz = 0.0;
#pragma unroll
        for (int e = 0; e < EP; ++e) {
            double h = 0.0;
            if (e < E)
#pragma unroll
                for (int f = 0; f < EP; ++f)
                    if (f < E) h = fma(Q[e * E + f], z[f], h);
            zqz = fma(z[e], h, zqz);
            if (e < E) {
                if (side) s_w[e][idx] = 2.0 * z[e];
                else { s_za[e][idx] = z[e]; s_g[e][idx] = h; }
            }
        }
        s_k[side][idx] = live ? (p.logvar[o] - 0.5 * dz) + zqz : -4096.0;
    };
    if (tid < 64) { s_tab[tid] = kExp2Tab[tid]; build(0, r0, tid); }
    // contraction entries owned by this thread: P2 upper triangle, then P1, then W
    const int nent = E * (E + 1) / 2, ntot = nent + E + 1;
    int ke[2], kf[2], kind[2];                // kind: 0 P2 (ke, kf), 1 P1 ke, 2 W, -1 none
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int k = tid + 256 * s;
        ke[s] = kf[s] = 0;
        kind[s] = k < nent ? 0 : k < nent + E ? 1 : k < ntot ? 2 : -1;
        if (kind[s] == 0) decode_tri(k, E, ke[s], kf[s]);
        else if (kind[s] == 1) ke[s] = k - nent;
    }
    double acc[2] = {0.0, 0.0};
    double racc[4], yacc[4][EP];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        racc[r] = 0.0;
#pragma unroll
        for (int e = 0; e < EP; ++e) yacc[r][e] = 0.0;
    }
    for (int ct = diag ? rt : 0; ct < nt; ++ct) {
        const int c0 = ct * kTile;
        __syncthreads();                      // the tile before is contracted (s_w, s_cs free); the rows are built
        if (tid >= 64 && tid < 128) build(1, c0, tid - 64);
        double w[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int i = r0 + lr + r, j = c0 + lc + c;
                double v = 0.0;
                if (i < N && j < N)
                    v = diag ? p.Tm[((size_t)a * (N + p.tpad) + i) * N + j] : p.beta[(size_t)a * N + i] * p.beta[(size_t)b * N + j];
                w[r][c] = v;
            }
        __syncthreads();
        double csum[4] = {0.0, 0.0, 0.0, 0.0};
        if (rows_live) {
            double dot[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) dot[r][c] = 0.0;
#pragma unroll
            for (int e = 0; e < EP; ++e) {
                if (e >= E) break;
                double g[4], wc[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) g[r] = s_g[e][lr + r];
#pragma unroll
                for (int c = 0; c < 4; ++c) wc[c] = s_w[e][lc + c];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) dot[r][c] = fma(g[r], wc[c], dot[r][c]);
            }
            double kr[4], kc[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) kr[r] = s_k[0][lr + r];
#pragma unroll
            for (int c = 0; c < 4; ++c) kc[c] = s_k[1][lc + c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) w[r][c] = fast_exp((kr[r] + kc[c]) + dot[r][c], s_tab) * w[r][c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) { racc[r] += w[r][c]; csum[c] += w[r][c]; }
#pragma unroll
            for (int e = 0; e < EP; ++e) {
                if (e >= E) break;
                double wc[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) wc[c] = s_w[e][lc + c];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) yacc[r][e] = fma(w[r][c], wc[c], yacc[r][e]);
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            csum[c] += __shfl_xor(csum[c], 16, 64);
            csum[c] += __shfl_xor(csum[c], 32, 64);
        }
        if (lane < 16)
#pragma unroll
            for (int c = 0; c < 4; ++c) s_c[wv][lc + c] = csum[c];
        __syncthreads();
        if (tid < kTile) s_cs[tid] = ((s_c[0][tid] + s_c[1][tid]) + s_c[2][tid]) + s_c[3][tid];
        __syncthreads();
        // column side: sum_j c_j z_bj z_bj^T, sum_j c_j z_bj (z_bj = s_w / 2, exact); W is the row side's
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (kind[s] < 0 || kind[s] == 2) continue;
            double v = acc[s];
            for (int j = 0; j < kTile; ++j) {
                const double cj = s_cs[j];
                const double t = kind[s] == 0 ? (0.5 * s_w[ke[s]][j]) * (0.5 * s_w[kf[s]][j]) : 0.5 * s_w[ke[s]][j];
                v = fma(cj, t, v);
            }
            acc[s] = v;
        }
    }
    // row side: the 16 lanes of a row group, then sum_i r_i z_ai z_ai^T + z_ai Y_i^T + Y_i z_ai^T, sum_i r_i z_ai, sum_i r_i
#pragma unroll
    for (int off = 1; off <= 8; off <<= 1)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            racc[r] += __shfl_xor(racc[r], off, 64);
#pragma unroll
            for (int e = 0; e < EP; ++e) yacc[r][e] += __shfl_xor(yacc[r][e], off, 64);
        }
    if ((lane & 15) == 0)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s_r[lr + r] = racc[r];
#pragma unroll
            for (int e = 0; e < EP; ++e)
                if (e < E) s_y[e][lr + r] = yacc[r][e];
        }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (kind[s] < 0) continue;
        double v = acc[s];
        for (int i = 0; i < kTile; ++i) {
            const double ri = s_r[i];
            if (kind[s] == 0) {
                const double ze = s_za[ke[s]][i], zf = s_za[kf[s]][i];
                v = fma(ri * ze, zf, v);
                v = fma(ze, 0.5 * s_y[kf[s]][i], v);
                v = fma(0.5 * s_y[ke[s]][i], zf, v);
            } else {
                v = fma(ri, kind[s] == 1 ? s_za[ke[s]][i] : 1.0, v);
            }
        }
        acc[s] = v;
    }
    double* out = q.ppart + (((size_t)pt * p.npairs + pr) * nt + rt) * pp_stride(E);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (kind[s] == 0) { out[ke[s] * E + kf[s]] = acc[s]; out[kf[s] * E + ke[s]] = acc[s]; }
        else if (kind[s] == 1) out[E * E + ke[s]] = acc[s];
        else if (kind[s] == 2) out[E * E + E] = acc[s];
    }
}

// ----------------------------------------------------------------------------------------------------------------------------
// Finish: one workgroup per point.  Every output, then every pair, in order; E x E products one entry per thread.
__global__ __launch_bounds__(256) void mb_finish_kernel(BackArgs q) {
    const MomentsArgs& p = q.f;
    __shared__ double s_G[kMaxE][kMaxE];      // Sigmab (not yet symmetrised)
    __shared__ double s_X[kMaxE][kMaxE];      // B^-1, or R^-1
    __shared__ double s_H[kMaxE][kMaxE];      // Mbe S2 + S3, or P2
    __shared__ double s_T[kMaxE][kMaxE];      // H B^-1, or P2 R^-1
    __shared__ double s_mb[kMaxE], s_s[kMaxE], s_v1[kMaxE], s_v3[kMaxE];
    __shared__ double s_M[kMaxD], s_Mbe[kMaxD], s_sc[2];
    const int tid = threadIdx.x;
    const int pt = blockIdx.x;
    const int E = p.E, D = p.D, EE = E * E;
    const double* Sb = q.Sb ? q.Sb + (size_t)pt * D * D : nullptr;
    if (tid < D) {
        const int a = tid;
        const double ldB = p.setup[((size_t)pt * p.nprob + a) * setup_stride(E) + EE];
        s_M[a] = q.psum[((size_t)pt * D + a) * psum_stride(E)] * (p.var[a] * exp(-0.5 * ldB));
    }
    for (int idx = tid; idx < EE; idx += 256) s_G[idx / E][idx % E] = 0.0;
    if (tid < E) s_mb[tid] = 0.0;
    __syncthreads();
    if (tid < D) {
        const int a = tid;
        double v = q.Mb ? q.Mb[(size_t)pt * D + a] : 0.0;
        if (Sb)
            for (int b = 0; b < D; ++b) v -= (Sb[a * D + b] + Sb[b * D + a]) * s_M[b];
        s_Mbe[a] = v;
    }
    __syncthreads();
    // ---- mean / V part
    for (int a = 0; a < D; ++a) {
        const double* su = p.setup + ((size_t)pt * p.nprob + a) * setup_stride(E);
        const double* ps = q.psum + ((size_t)pt * D + a) * psum_stride(E);
        const double S0 = ps[0], *S1 = ps + 1, *y = ps + 1 + E, *S2 = ps + 1 + 2 * E, *S3 = S2 + EE;
        const double c = p.var[a] * exp(-0.5 * su[EE]);
        const double Mbe = s_Mbe[a];
        // B^-1 = C^-T C^-1 (C^-1 lower);  H = Mbe S2 + S3
        for (int idx = tid; idx < EE; idx += 256) {
            const int r = idx / E, cc = idx - r * E;
            double v = 0.0;
            for (int k = r > cc ? r : cc; k < E; ++k) v = fma(su[k * E + r], su[k * E + cc], v);
            s_X[r][cc] = v;
            s_H[r][cc] = fma(Mbe, S2[idx], S3[idx]);
        }
        if (tid < E) {
            s_s[tid] = sqrt(p.ils2[a * E + tid]);
            double h = Mbe * S1[tid];
            for (int k = 0; k < E; ++k) h = fma(S2[tid * E + k], y[k], h);
            s_v3[tid] = h;                                        // Mbe S1 + S2 y
        }
        if (tid == 0) {
            double L = Mbe * S0;
            for (int k = 0; k < E; ++k) L = fma(y[k], S1[k], L);
            s_sc[0] = c * L;
        }
        __syncthreads();
        if (tid < E) {
            double t1 = 0.0, t2 = 0.0;
            for (int k = 0; k < E; ++k) { t1 = fma(s_X[tid][k], S1[k], t1); t2 = fma(s_X[tid][k], s_v3[k], t2); }
            s_v1[tid] = t1;                                       // t = B^-1 S1
            s_mb[tid] += c * s_s[tid] * (t2 - S0 * y[tid]);
        }
        for (int idx = tid; idx < EE; idx += 256) {
            const int r = idx / E, cc = idx - r * E;
            double v = 0.0;
            for (int k = 0; k < E; ++k) v = fma(s_H[r][k], s_X[k][cc], v);
            s_T[r][cc] = v;
        }
        __syncthreads();
        const double L = s_sc[0];
        for (int idx = tid; idx < EE; idx += 256) {
            const int r = idx / E, cc = idx - r * E;
            double u = 0.0;
            for (int k = 0; k < E; ++k) u = fma(s_X[r][k], s_T[k][cc], u);
            const double bb = -0.5 * L * s_X[r][cc] + 0.5 * c * u - 0.5 * c * (y[r] * s_v1[cc] + s_v1[r] * y[cc]);
            s_G[r][cc] += s_s[r] * s_s[cc] * bb;
        }
        __syncthreads();
    }
    // ---- pair part
    if (Sb) {
        const int nt = p.nt;
        for (int pr = 0; pr < p.npairs; ++pr) {
            int a, b;
            decode_tri(pr, D, a, b);
            const bool diag = a == b;
            const double gam = diag ? Sb[a * D + a] : Sb[a * D + b] + Sb[b * D + a];
            const double ldR = p.setup[((size_t)pt * p.nprob + D + pr) * setup_stride(E) + EE];
            const double fs = gam * exp(-0.5 * ldR) * (diag ? 2.0 : 1.0);
            const double* pp = q.ppart + ((size_t)pt * p.npairs + pr) * nt * pp_stride(E);
            const double* Ai = p.ainv + ((size_t)pt * p.npairs + pr) * EE;
            if (tid < E) s_s[tid] = sqrt(p.ils2[a * E + tid] + p.ils2[b * E + tid]);
            __syncthreads();
            for (int idx = tid; idx < EE + E + 1; idx += 256) {     // the row tiles' partials, in order
                double v = 0.0;
                for (int k = 0; k < nt; ++k) v += pp[(size_t)k * pp_stride(E) + idx];
                if (idx < EE) {
                    const int r = idx / E, cc = idx - r * E;
                    s_H[r][cc] = v;
                    s_X[r][cc] = Ai[idx] * s_s[cc] / s_s[r];           // R^-1
                } else if (idx < EE + E) s_v1[idx - EE] = v;
                else s_sc[1] = v;
            }
            __syncthreads();
            for (int idx = tid; idx < EE; idx += 256) {
                const int r = idx / E, cc = idx - r * E;
                double v = 0.0;
                for (int k = 0; k < E; ++k) v = fma(s_H[r][k], s_X[k][cc], v);
                s_T[r][cc] = v;
            }
            if (tid < E) {
                double v = 0.0;
                for (int k = 0; k < E; ++k) v = fma(s_X[k][tid], s_v1[k], v);
                s_mb[tid] += fs * v;
            }
            __syncthreads();
            const double W = s_sc[1];
            for (int idx = tid; idx < EE; idx += 256) {
                const int r = idx / E, cc = idx - r * E;
                double u = 0.0;
                for (int k = 0; k < E; ++k) u = fma(s_X[k][r], s_T[k][cc], u);
                s_G[r][cc] += 0.5 * fs * (u - W * (s_s[r] * Ai[idx] * s_s[cc]));
            }
            __syncthreads();
        }
    }
    if (q.vb_out)
        for (int idx = tid; idx < EE; idx += 256) {
            const int r = idx / E, cc = idx - r * E;
            q.vb_out[(size_t)pt * EE + idx] = 0.5 * (s_G[r][cc] + s_G[cc][r]);
        }
    if (q.mb_out && tid < E) q.mb_out[(size_t)pt * E + tid] = s_mb[tid];
}

template <int EP>
void launch_backward_sums(const BackArgs& q, bool pairs, hipStream_t s) {
    hipLaunchKernelGGL(mb_point_kernel<EP>, dim3(q.f.rows * q.f.D), dim3(256), 0, s, q);
    if (pairs) hipLaunchKernelGGL(mb_pair_kernel<EP>, dim3(q.f.nt, q.f.npairs, q.f.rows), dim3(256), 0, s, q);
}

}  // namespace

int run_moments_backward(Handle* h, const double* mu, const double* Sig, int P, const double* Mb, const double* Sb,
                         const double* Vb, double* mb_out, double* vb_out, hipStream_t s) {
    const int N = h->N, D = h->D, E = h->E;
    if (P == 0 || (!mb_out && !vb_out)) return GPMPC_OK;
    const bool pairs = Sb != nullptr;
    const int npairs = D * (D + 1) / 2;
    const int nt = (N + kTile - 1) / kTile;
    const int nprob = D + (pairs ? npairs : 0);
    const size_t n_setup = nprob * setup_stride(E), n_ainv = pairs ? (size_t)npairs * E * E : 0;
    const size_t n_psum = (size_t)D * psum_stride(E), n_pp = pairs ? (size_t)npairs * nt * pp_stride(E) : 0;
    const size_t per_point = n_setup + n_ainv + n_psum + n_pp;
    long long Pc = (long long)(kWsBudget / (sizeof(double) * per_point));
    if (Pc < 1) Pc = 1;
    if (h->opt_moments_bwd_chunk > 0) Pc = h->opt_moments_bwd_chunk;
    if (Pc > P) Pc = P;
    int rc = grow(h, h->mombws, per_point * (size_t)Pc);
    if (rc) return rc;
    BackArgs q{};
    MomentsArgs& p = q.f;
    p.Xt = h->Xt.p; p.ils2 = h->ils2.p; p.var = h->var.p; p.logvar = h->logvar.p; p.beta = h->beta.p; p.Tm = h->Tm.p;
    p.setup = h->mombws.p;
    p.ainv = pairs ? p.setup + (size_t)Pc * n_setup : nullptr;
    q.psum = h->mombws.p + (size_t)Pc * (n_setup + n_ainv);
    q.ppart = q.psum + (size_t)Pc * n_psum;
    p.N = N; p.D = D; p.E = E; p.npairs = npairs; p.nt = nt; p.tpad = kTPad; p.nprob = nprob;
    for (long long p0 = 0; p0 < P; p0 += Pc) {
        const int rows = (int)((P - p0) < Pc ? (P - p0) : Pc);
        p.rows = rows;
        p.mu = mu + (size_t)p0 * E;
        p.Sig = Sig ? Sig + (size_t)p0 * E * E : nullptr;
        q.Mb = Mb ? Mb + (size_t)p0 * D : nullptr;
        q.Sb = Sb ? Sb + (size_t)p0 * D * D : nullptr;
        q.Vb = Vb ? Vb + (size_t)p0 * E * D : nullptr;
        q.mb_out = mb_out ? mb_out + (size_t)p0 * E : nullptr;
        q.vb_out = vb_out ? vb_out + (size_t)p0 * E * E : nullptr;
        hipLaunchKernelGGL(moments_setup_kernel, dim3(rows * nprob), dim3(64), 0, s, p);
        if (E <= 4) launch_backward_sums<4>(q, pairs, s);
        else if (E <= 8) launch_backward_sums<8>(q, pairs, s);
        else if (E <= 12) launch_backward_sums<12>(q, pairs, s);
        else if (E <= 16) launch_backward_sums<16>(q, pairs, s);
        else if (E <= 20) launch_backward_sums<20>(q, pairs, s);
        else launch_backward_sums<24>(q, pairs, s);
        hipLaunchKernelGGL(mb_finish_kernel, dim3(rows), dim3(256), 0, s, q);
    }
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

}  // namespace gpmpc_hip
