// moments.hip -- moment-matched one-step prediction at uncertain inputs (gpmpc_moments): predict_next_state_change
// (gp_model.py:112-180) for P independent Gaussian inputs N(m_p, Sigma_p) with a general (full E x E) Sigma_p.
//   M_a = c_a sum_i lb_a(i),  lb_a(i) = beta_a(i) exp(-1/2 |C_a^-1 u_ai|^2),  u_ai = (x_i - m) / l_a,  c_a = sigma2_a / sqrt(det B_a)
//   V[:,a] = c_a B_a^-1 (sum_i lb_a(i) u_ai) / l_a,        B_a = diag(1/l_a) Sigma diag(1/l_a) + I = C_a C_a^T
//   S_ab = [sum_ij L_ab(i,j) (beta_a(i) beta_b(j) - delta_ab iK_a(i,j))] / sqrt(det R_ab) + delta_ab sigma2_a - M_a M_b
//   L_ab(i,j) = exp(ka'_i + kb'_j + g_i . w_j),  ka'_i = k_a(i) + z_ai^T Q z_ai,  g_i = Q z_ai,  w_j = 2 z_bj,
//   z_ai = (x_i - m) / l_a^2,  k_a(i) = log sigma2_a - 1/2 |u_ai|^2,  Q = Q_ab = 1/2 R_ab^-1 Sigma,  R_ab = Sigma Lambda_ab + I.
//
// Structure ("Moment matching at uncertain inputs"):
//   moments_setup_kernel  one wavefront per (point, problem).  Problem a < D: the Cholesky factor of B_a, its inverse (lower
//                         triangle) and log det B_a.  Problem D + pair: Q_ab through the SPD A = I + G, G = Lambda^1/2 Sigma
//                         Lambda^1/2 (det A = det R_ab): R^-1 Sigma = Lambda^-1/2 A^-1 G Lambda^-1/2, and A^-1 G (= I - A^-1,
//                         formed without that cancellation) is symmetric, so Q is symmetrised exactly.  All in LDS.
//   moments_point_kernel  one workgroup per (point, output a): the O(N E^2) sums of M_a and V[:,a].
//   moments_pair_kernel   batch-major: a workgroup owns (pair, 64-row tile, 64-column tile) and loops over kPPW points.  Its
//                         T_a tile (diagonal pairs) or beta_a(i) beta_b(j) (off-diagonal) stays in registers across the
//                         points; per point it builds g_i, ka'_i of its rows and w_j, kb'_j of its columns in LDS (double
//                         buffered: one barrier per point) and every lane sums 4 x 4 elements, one exp per element.  Each
//                         wavefront writes its partial sum; diagonal pairs only visit the tiles on and above the diagonal.
//   moments_finish_kernel one wavefront per (point, pair): the partials in a fixed order, / sqrt(det R), + sigma2, - M M^T, mirror.
// Every sum a point goes through has an order fixed by N, E and the pair alone, and there are no atomics: a point's M, S and V
// are bitwise the same whatever P is, wherever it sits in the batch, whoever its neighbours are and however the points are
// chunked.  P is processed in chunks so the workspace stays within kWsBudget whatever P is.
#include "moments_common.h"
#include "device_common.h"

namespace gpmpc_hip {

namespace {

constexpr int kPPW = 8;                         // points per pair-pass workgroup

// ----------------------------------------------------------------------------------------------------------------------------
// O(N) pass: one workgroup (4 wavefronts) per (point, output a).
template <int EP>
__global__ __launch_bounds__(256) void moments_point_kernel(MomentsArgs p) {
    __shared__ double s_Ci[EP * EP];
    __shared__ double s_red[kWaves][EP + 1];
    __shared__ double s_tab[64];
    __shared__ double s_m[EP], s_il[EP];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int pt = blockIdx.x / p.D, a = blockIdx.x - pt * p.D;
    const int E = p.E, N = p.N;
    const bool wantV = p.V_out != nullptr;
    const double* su = p.setup + ((size_t)pt * p.nprob + a) * setup_stride(E);
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
    double s0 = 0.0, s1[EP];
#pragma unroll
    for (int e = 0; e < EP; ++e) s1[e] = 0.0;
    for (int i = tid; i < N; i += 256) {
        asm volatile("" ::: "memory");           // re-read C^-1 from LDS every point (hoisting it costs more than it saves)
        double u[EP];
#pragma unroll
        for (int e = 0; e < EP; ++e) u[e] = e < E ? (p.Xt[(size_t)e * N + i] - s_m[e]) * s_il[e] : 0.0;
        double q = 0.0;
#pragma unroll
        for (int r = 0; r < EP; ++r) {
            double w = 0.0;
#pragma unroll
            for (int c = 0; c <= r; ++c) w = fma(s_Ci[r * EP + c], u[c], w);
            q = fma(w, w, q);
        }
        const double lb = fast_exp(-0.5 * q, s_tab) * p.beta[(size_t)a * N + i];      // gp_model.py:148
        s0 += lb;
        if (wantV)
#pragma unroll
            for (int e = 0; e < EP; ++e) s1[e] = fma(lb, u[e], s1[e]);
    }
    // the 64 lanes (butterfly), then the 4 wavefronts in order
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s0 += __shfl_xor(s0, off, 64);
        if (wantV)
#pragma unroll
            for (int e = 0; e < EP; ++e) s1[e] += __shfl_xor(s1[e], off, 64);
    }
    if (lane == 0) {
        s_red[wv][EP] = s0;
#pragma unroll
        for (int e = 0; e < EP; ++e) s_red[wv][e] = s1[e];
    }
    __syncthreads();
    if (tid != 0) return;
    const double c = p.var[a] * exp(-0.5 * su[E * E]);                   // sigma2_a / sqrt(det B_a)   :150
    const double S0 = ((s_red[0][EP] + s_red[1][EP]) + s_red[2][EP]) + s_red[3][EP];
    p.M_out[(size_t)pt * p.D + a] = S0 * c;                              // :152
    if (!wantV) return;
    double t[EP], v[EP];
#pragma unroll
    for (int e = 0; e < EP; ++e) t[e] = ((s_red[0][e] + s_red[1][e]) + s_red[2][e]) + s_red[3][e];
    // B_a^-1 t = C^-T (C^-1 t)
#pragma unroll
    for (int r = 0; r < EP; ++r) {
        double w = 0.0;
#pragma unroll
        for (int k = 0; k <= r; ++k) w = fma(s_Ci[r * EP + k], t[k], w);
        v[r] = w;
    }
#pragma unroll
    for (int r = 0; r < EP; ++r) {
        double w = 0.0;
#pragma unroll
        for (int k = EP - 1; k >= r; --k) w = fma(s_Ci[k * EP + r], v[k], w);
        if (r < E) p.V_out[((size_t)pt * E + r) * p.D + a] = w * s_il[r] * c;     // :149, :153
    }
}

// ----------------------------------------------------------------------------------------------------------------------------
// Pair pass.  Lane map: wavefront w owns rows 16 w .. 16 w + 15 of the tile, lane l rows 16 w + 4 (l >> 4) + {0..3} and
// columns 4 (l & 15) + {0..3}.
template <int EP>
__global__ __launch_bounds__(256) void moments_pair_kernel(MomentsArgs p) {
    __shared__ double s_g[2][EP][kTile];      // g_i (rows), per point buffer
    __shared__ double s_w[2][EP][kTile];      // w_j (columns)
    __shared__ double s_k[2][2][kTile];       // ka'_i, kb'_j
    __shared__ double s_tab[64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nt = p.nt, N = p.N, E = p.E;
    const int tile = blockIdx.x, rt = tile / nt, ct = tile - rt * nt;
    const int pr = blockIdx.y;
    int a, b;
    decode_tri(pr, p.D, a, b);
    const bool diag = a == b;
    if (diag && rt > ct) return;                                          // lower tiles of a diagonal pair: nothing
    const int pt0 = blockIdx.z * kPPW;
    if (pt0 >= p.rows) return;
    const int pt1 = min(pt0 + kPPW, p.rows);
    if (tid < 64) s_tab[tid] = kExp2Tab[tid];
    const int r0 = rt * kTile, c0 = ct * kTile;
    const int lr = 16 * wv + 4 * (lane >> 4), lc = 4 * (lane & 15);
    const bool rows_live = r0 + 16 * wv < N;                              // the wavefront has rows inside the memory
    // coefficients: T_a (diagonal pairs) or beta_a(i) beta_b(j), zero outside the memory
    double cf[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = r0 + lr + r, j = c0 + lc + c;
            double v = 0.0;
            if (i < N && j < N)
                v = diag ? p.Tm[((size_t)a * (N + p.tpad) + i) * N + j] : p.beta[(size_t)a * N + i] * p.beta[(size_t)b * N + j];
            cf[r][c] = v;
        }
    // builder map: threads 0..63 the rows (side a), 64..127 the columns (side b)
    const int bside = tid >> 6, bidx = tid & 63;
    const int bo = bside ? b : a;                                         // uniform per wavefront
    const int bi = (bside ? c0 : r0) + bidx;
    const bool blive = bi < N;
    const double blogv = p.logvar[bo];
    auto build = [&](int pt, int buf) {
        if (tid >= 128) return;
        const double* Q = p.setup + ((size_t)pt * p.nprob + p.D + pr) * setup_stride(E);
        const double* mu = p.mu + (size_t)pt * E;
        double z[EP], dz = 0.0;
#pragma unroll
        for (int e = 0; e < EP; ++e) {
            const double d = (e < E && blive) ? p.Xt[(size_t)e * N + bi] - mu[e] : 0.0;      // 0 outside the memory
            z[e] = e < E ? d * p.ils2[bo * E + e] : 0.0;
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
            if (bside) s_w[buf][e][bidx] = 2.0 * z[e];
            else s_g[buf][e][bidx] = h;
        }
        // far below any live term outside the memory (fast_exp needs a finite argument)
        s_k[buf][bside][bidx] = blive ? (blogv - 0.5 * dz) + zqz : -4096.0;
    };
    double* part = p.part + (((size_t)pt0 * p.npairs + pr) * nt * nt + tile) * kWaves + wv;
    const size_t pstride = (size_t)p.npairs * nt * nt * kWaves;
    build(pt0, 0);
    for (int pt = pt0; pt < pt1; ++pt) {
        const int buf = (pt - pt0) & 1;
        __syncthreads();                       // buffer `buf` is built; everybody is done with the point before's
        if (pt + 1 < pt1) build(pt + 1, buf ^ 1);
        double acc = 0.0;
        if (rows_live) {
            double dot[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) dot[r][c] = 0.0;
#pragma unroll
            for (int e = 0; e < EP; ++e) {
                double g[4], w[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) g[r] = s_g[buf][e][lr + r];
#pragma unroll
                for (int c = 0; c < 4; ++c) w[c] = s_w[buf][e][lc + c];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) dot[r][c] = fma(g[r], w[c], dot[r][c]);
            }
            double kr[4], kc[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) kr[r] = s_k[buf][0][lr + r];
#pragma unroll
            for (int c = 0; c < 4; ++c) kc[c] = s_k[buf][1][lc + c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc = fma(fast_exp((kr[r] + kc[c]) + dot[r][c], s_tab), cf[r][c], acc);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) part[(size_t)(pt - pt0) * pstride] = acc;
    }
}

// ----------------------------------------------------------------------------------------------------------------------------
// Finish: one wavefront per (point, pair).
__global__ __launch_bounds__(64) void moments_finish_kernel(MomentsArgs p) {
    const int lane = threadIdx.x;
    const int pt = blockIdx.x / p.npairs, pr = blockIdx.x - pt * p.npairs;
    int a, b;
    decode_tri(pr, p.D, a, b);
    const bool diag = a == b;
    const int nt = p.nt, nw = nt * nt * kWaves;
    const double* part = p.part + ((size_t)pt * p.npairs + pr) * nw;
    double s = 0.0;
    for (int k = lane; k < nw; k += 64) {
        const int tile = k / kWaves, rt = tile / nt, ct = tile - rt * nt;
        if (!diag || rt <= ct) s += part[k];
    }
    s = wave_xor_sum(s);
    if (lane != 0) return;
    const int D = p.D;
    const double ldR = p.setup[((size_t)pt * p.nprob + D + pr) * setup_stride(p.E) + (size_t)p.E * p.E];
    double v = (diag ? 2.0 * s : s) * exp(-0.5 * ldR);                   // :170-176
    if (diag) v += p.var[a];                                              // :177
    v -= p.M_out[(size_t)pt * D + a] * p.M_out[(size_t)pt * D + b];       // :178
    p.S_out[((size_t)pt * D + a) * D + b] = v;
    p.S_out[((size_t)pt * D + b) * D + a] = v;
}

template <int EP>
void launch_sums(const MomentsArgs& p, bool pairs, hipStream_t s) {
    hipLaunchKernelGGL(moments_point_kernel<EP>, dim3(p.rows * p.D), dim3(256), 0, s, p);
    if (pairs)
        hipLaunchKernelGGL(moments_pair_kernel<EP>, dim3(p.nt * p.nt, p.npairs, (p.rows + kPPW - 1) / kPPW), dim3(256), 0, s, p);
}

}  // namespace

int run_moments(Handle* h, const double* mu, const double* Sig, int P, double* M_out, double* S_out, double* V_out,
                hipStream_t s) {
    const int N = h->N, D = h->D, E = h->E;
    if (P == 0) return GPMPC_OK;
    const bool pairs = S_out != nullptr;
    const int npairs = D * (D + 1) / 2;
    const int nt = (N + kTile - 1) / kTile;
    const int nprob = D + (pairs ? npairs : 0);
    // points per chunk: as many as the workspace budget holds (a multiple of kPPW), no more than P needs
    const size_t per_point = nprob * setup_stride(E) + (pairs ? (size_t)npairs * nt * nt * kWaves : 0);
    long long Pc = (long long)(kWsBudget / (sizeof(double) * per_point)) / kPPW * kPPW;
    if (Pc < 1) Pc = 1;
    if (h->opt_moments_chunk > 0) Pc = h->opt_moments_chunk;
    if (Pc > P) Pc = P;
    int rc = grow(h, h->momws, per_point * (size_t)Pc);
    if (rc) return rc;
    MomentsArgs p{};
    p.Xt = h->Xt.p; p.ils2 = h->ils2.p; p.var = h->var.p; p.logvar = h->logvar.p; p.beta = h->beta.p; p.Tm = h->Tm.p;
    p.setup = h->momws.p;
    p.part = h->momws.p + (size_t)Pc * nprob * setup_stride(E);
    p.N = N; p.D = D; p.E = E; p.npairs = npairs; p.nt = nt; p.tpad = kTPad; p.nprob = nprob;
    for (long long p0 = 0; p0 < P; p0 += Pc) {
        const int rows = (int)((P - p0) < Pc ? (P - p0) : Pc);
        p.rows = rows;
        p.mu = mu + (size_t)p0 * E;
        p.Sig = Sig ? Sig + (size_t)p0 * E * E : nullptr;
        p.M_out = M_out + (size_t)p0 * D;
        p.S_out = S_out ? S_out + (size_t)p0 * D * D : nullptr;
        p.V_out = V_out ? V_out + (size_t)p0 * E * D : nullptr;
        hipLaunchKernelGGL(moments_setup_kernel, dim3(rows * nprob), dim3(64), 0, s, p);
        if (E <= 4) launch_sums<4>(p, pairs, s);
        else if (E <= 8) launch_sums<8>(p, pairs, s);
        else if (E <= 12) launch_sums<12>(p, pairs, s);
        else if (E <= 16) launch_sums<16>(p, pairs, s);
        else if (E <= 20) launch_sums<20>(p, pairs, s);
        else launch_sums<24>(p, pairs, s);
        if (pairs) hipLaunchKernelGGL(moments_finish_kernel, dim3(rows * npairs), dim3(64), 0, s, p);
    }
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

}  // namespace gpmpc_hip
