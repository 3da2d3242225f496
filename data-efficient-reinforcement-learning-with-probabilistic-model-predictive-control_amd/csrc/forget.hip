// forget.hip -- the shrinking half of the incremental factorisation (gpmpc_forget) for gfx950 (MI355X, CDNA4).
//
// Removing memory point j from K = L L^T (n points) in O(n^2) per GP, no n^3 product.  With R = L^-1, iK = R^T R, beta = iK y:
//   iK'   = iK[-j,-j] - c c^T / d,  beta' = beta[-j] - c beta_j / d          (c = iK[-j, j], d = iK[j, j]: one streaming pass)
//   R'    : rows above j keep their entries (column j of them is zero); below j, with w = -R[j+1:, j] / R[j, j] and
//           Z = [ R[j+1:, :j] + w R[j, :j] | R[j+1:, j+1:] ],  R'[j:, :] = G^-1 Z,  G = chol(I + w w^T).
// G is semiseparable: with t_0 = 1, t_{i+1} = t_i + w_i^2 the solve is a running sum per column,
//   z'_i = (z_i - w_i S_i) sqrt(t_i / t_{i+1}),   S_{i+1} = S_i + w_i z'_i / sqrt(t_i t_{i+1}),
// which the kernel walks in the shifted form U_i = S_i - R[j, c] (U_0 = -R[j, c]; 0 for the columns right of j):
//   z'_i = g_i R[j+1+i, c] - (w_i g_i) U_i,   U_{i+1} = p_i U_i + q_i R[j+1+i, c],   g_i = sqrt(p_i), p_i = t_i / t_{i+1}, q_i = w_i / t_{i+1}
// -- one dependent fma per row, and only sums of positive terms in the coefficients (nothing cancels).  The coefficients depend
// on w alone and are formed once per removal (forget_coef_kernel); the columns are independent (forget_apply_kernel).
// The outputs are row-major compactions of the inputs ((n-1) x (n-1)): the caller ping-pongs the buffers as the border update does.
#include "device_common.h"

namespace gpmpc_hip {

constexpr int kForgetRows = 16;       // rows of a column block in flight per wavefront
static_assert(4 * kForgetRows == kWave, "a group's coefficients are one value per lane");

// the value lane `l` (a constant) holds, in a scalar register
__device__ inline double lane_read(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// Per GP (one workgroup): u = iK[j, :] / sqrt(d) (n entries, source numbering), beta_j / sqrt(d), and the recurrence's
// coefficients (g, w g, p, q) of the n - 1 - j rows below j.  ws per GP: [u (ldw) | 4 coefficients per row (4 ldw)]; bs (D).
// A non-positive (or NaN) d or R[j, j], or a t that left the finite range, is reported like a lost pivot: info[a] = j + 1.
__global__ __launch_bounds__(256) void forget_coef_kernel(const double* __restrict__ iK, const double* __restrict__ linv,
                                                          const double* __restrict__ beta, int n, int j, int ldw,
                                                          double* __restrict__ ws, double* __restrict__ bs, int* __restrict__ info) {
    __shared__ double part[256];
    const int a = blockIdx.x, t = threadIdx.x;
    const double* iKa = iK + (size_t)a * n * n;
    const double* Ra = linv + (size_t)a * n * n;
    double* u = ws + (size_t)a * 5 * ldw;
    double* co = u + ldw;
    const double d = iKa[(size_t)j * n + j], rho = Ra[(size_t)j * n + j];
    bool lost = !(d > 0.0) || !(rho > 0.0);
    const double rsd = 1.0 / sqrt(d);
    for (int i = t; i < n; i += 256) u[i] = iKa[(size_t)j * n + i] * rsd;
    if (t == 0) bs[a] = beta[(size_t)a * n + j] * rsd;
    // t_i = 1 + sum_{l < i} w_l^2: each thread owns a run of consecutive rows; the runs' totals are chained in a fixed order
    const int m = n - 1 - j;
    const int run = (m + 255) / 256;
    const int i0 = t * run < m ? t * run : m, i1 = i0 + run < m ? i0 + run : m;
    const double* col = Ra + (size_t)(j + 1) * n + j;                 // R[j + 1 + i, j] = col[i n]
    double s = 0.0;
    for (int i = i0; i < i1; ++i) { const double w = -col[(size_t)i * n] / rho; s = fma(w, w, s); }
    part[t] = s;
    __syncthreads();
    double tt = 1.0;
    for (int k = 0; k < t; ++k) tt += part[k];
    for (int i = i0; i < i1; ++i) {
        const double w = -col[(size_t)i * n] / rho;
        const double t1 = fma(w, w, tt);
        const double p = tt / t1, g = sqrt(p);
        co[4 * (size_t)i] = g;
        co[4 * (size_t)i + 1] = w * g;
        co[4 * (size_t)i + 2] = p;
        co[4 * (size_t)i + 3] = w / t1;
        tt = t1;
    }
    lost = lost || !(tt < INFINITY);
    if (lost && info[a] == 0) info[a] = j + 1;
}

// iK', beta' and R' of one removal in ONE launch.  Workgroups [0, nbR) of a GP: the factor -- a wavefront owns 64 adjacent
// output columns (lane = column: every row is one coalesced 512-byte segment in and out), copies the rows above j and walks the
// rows below in order with U in a register, the next 16 rows and their coefficients in flight (one dependent fma per row);
// columns right of j are zero until their diagonal, so the walk starts at the wavefront's first column.  Upper-triangle
// entries are written as zeros (the target buffer holds something else).  The other workgroups: the Schur update, one
// streaming pass, 4 rows x 64 columns each; u_i u_j is formed the same way on both sides of the diagonal, so iK' stays
// exactly symmetric.
__global__ __launch_bounds__(256) void forget_apply_kernel(const double* __restrict__ iK, const double* __restrict__ linv,
                                                           const double* __restrict__ beta, const double* __restrict__ ws,
                                                           const double* __restrict__ bs, int n, int j, int ldw, int nbR,
                                                           double* __restrict__ iKn, double* __restrict__ linvn,
                                                           double* __restrict__ betan) {
    const int a = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n1 = n - 1;
    const double* u = ws + (size_t)a * 5 * ldw;
    if ((int)blockIdx.x < nbR) {
        const int c0 = ((int)blockIdx.x * 4 + wave) * 64;
        if (c0 >= n1) return;
        const double* co = u + ldw;                               // (g, w g, p, q) of row j + 1 + i at co[4 i ..]
        const double* Ra = linv + (size_t)a * n * n;
        double* Rn = linvn + (size_t)a * n1 * n1;
        const int c = c0 + lane;                                  // output column; source column sc
        const bool in = c < n1;
        const int cl = in ? c : n1 - 1;                           // every load from a valid address, masked by a select: a branch
        const int sc = cl < j ? cl : cl + 1;                      // per element would serialise the loads' round trips
        for (int r0 = 0; r0 < j; r0 += kForgetRows) {
            double v[kForgetRows];
#pragma unroll
            for (int q = 0; q < kForgetRows; ++q) {
                const int r = r0 + q < j ? r0 + q : j - 1;
                v[q] = Ra[(size_t)r * n + sc];
            }
#pragma unroll
            for (int q = 0; q < kForgetRows; ++q) {
                const int r = r0 + q;
                if (in && r < j) Rn[(size_t)r * n1 + c] = c <= r ? v[q] : 0.0;
            }
        }
        const int first = c0 > j ? c0 : j;                        // wave-uniform: rows [j, first) are all zero here
        for (int r = j; r < first; ++r)
            if (in) Rn[(size_t)r * n1 + c] = 0.0;
        double U = (in && c < j) ? -Ra[(size_t)j * n + cl] : 0.0;
        // A group = 16 rows: their entries of this column block and their 64 coefficients (lane l holds coefficient l & 3 of row
        // l >> 2: one coalesced load) are fetched together, from clamped addresses and outside every guard, and the next group's
        // travel while this one's recurrence runs; a coefficient reaches the recurrence through a lane read, so the dependent
        // chain is the fma alone.
        const int ncoef = 4 * (n1 - j);
        auto fetch = [&](double (&z)[kForgetRows], double& kc, int r0) {
#pragma unroll
            for (int q = 0; q < kForgetRows; ++q) {
                const int r = r0 + q < n1 ? r0 + q : n1 - 1;
                z[q] = Ra[(size_t)(r + 1) * n + sc];
            }
            const int i = 4 * (r0 - j) + lane;
            kc = co[i < ncoef ? i : ncoef - 1];
        };
        double z[kForgetRows], zn[kForgetRows], kc = 0.0, kn = 0.0;
        if (first < n1) fetch(z, kc, first);
        for (int r0 = first; r0 < n1; r0 += kForgetRows) {
            if (r0 + kForgetRows < n1) fetch(zn, kn, r0 + kForgetRows);
#pragma unroll
            for (int q = 0; q < kForgetRows; ++q) {
                const int r = r0 + q;
                const double g = lane_read(kc, 4 * q), wg = lane_read(kc, 4 * q + 1);
                const double p = lane_read(kc, 4 * q + 2), qq = lane_read(kc, 4 * q + 3);
                const double zq = (in && c <= r) ? z[q] : 0.0;
                const double out = fma(g, zq, -(wg * U));
                U = fma(p, U, qq * zq);                              // (rows past the end run along on clamped values: not stored)
                if (in && r < n1) Rn[(size_t)r * n1 + c] = out;
            }
#pragma unroll
            for (int q = 0; q < kForgetRows; ++q) z[q] = zn[q];
            kc = kn;
        }
        return;
    }
    const int tiles = (n1 + 63) / 64;
    const int b = (int)blockIdx.x - nbR;
    const int jo = (b % tiles) * 64 + lane;
    const int io = (b / tiles) * 4 + wave;
    if (io >= n1 || jo >= n1) return;
    const int si = io < j ? io : io + 1, sj = jo < j ? jo : jo + 1;
    const double ui = u[si], uj = u[sj];
    iKn[((size_t)a * n1 + io) * n1 + jo] = fma(-ui, uj, iK[((size_t)a * n + si) * n + sj]);        // exactly symmetric
    if (io == 0) betan[(size_t)a * n1 + jo] = fma(-uj, bs[a], beta[(size_t)a * n + sj]);
}

// source row of kept row p: the removed rows are ascending, so each one at or before the running position shifts it by one
__device__ inline int forget_source_row(const ForgetRows& rm, int p) {
    const int* v = rm.k <= 8 ? rm.few : rm.many;
    for (int q = 0; q < rm.k; ++q)
        if (p >= v[q]) ++p;
    return p;
}

// The record of (X, Y) without the removed rows, and what the rollouts read of X: X^T and the per-dimension data range
// (blocks e < E reduce dimension e, as pack_record_kernel does).  Xt / xr NULL: the record alone (the caller refactorises).
__global__ __launch_bounds__(256) void forget_pack_kernel(const double* __restrict__ Xc, const double* __restrict__ Yc, const ForgetRows rm,
                                                          int n1, int D, int E, double* __restrict__ Xn, double* __restrict__ Yn,
                                                          double* __restrict__ Xt, double* __restrict__ xr) {
    const int stride = gridDim.x * 256;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < n1 * E; idx += stride) {
        const int p = idx / E, e = idx - p * E;
        const double v = Xc[(size_t)forget_source_row(rm, p) * E + e];
        Xn[idx] = v;
        if (Xt) Xt[(size_t)e * n1 + p] = v;
    }
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < n1 * D; idx += stride) {
        const int p = idx / D, a = idx - p * D;
        Yn[idx] = Yc[(size_t)forget_source_row(rm, p) * D + a];
    }
    if (xr && (int)blockIdx.x < E) {
        __shared__ double smin[4], smax[4];
        const int e = blockIdx.x;
        double lo = INFINITY, hi = -INFINITY;
        for (int p = threadIdx.x; p < n1; p += 256) {
            const double v = Xc[(size_t)forget_source_row(rm, p) * E + e];
            lo = fmin(lo, v);
            hi = fmax(hi, v);
        }
        for (int off = 32; off >= 1; off >>= 1) { lo = fmin(lo, __shfl_xor(lo, off, 64)); hi = fmax(hi, __shfl_xor(hi, off, 64)); }
        if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            xr[e] = fmin(fmin(smin[0], smin[1]), fmin(smin[2], smin[3]));
            xr[E + e] = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
        }
    }
}

// ------------------------------------------------------------------------------------------
// One removal: (iK, linv, beta) of n points -> (gram, Tm, zvec) of n - 1; the caller swaps the buffers.  fgws: [coefficients
// (5 D ldw) | beta_j / sqrt(d) (D)].
int launch_forget_step(Handle* h, int n, int j, int D, int ldw, hipStream_t s) {
    double* ws = h->fgws.p;
    double* bs = ws + (size_t)5 * D * ldw;
    const int n1 = n - 1;
    hipLaunchKernelGGL(forget_coef_kernel, dim3(D), dim3(256), 0, s, h->iK.p, h->linv.p, h->beta.p, n, j, ldw, ws, bs, h->info);
    const int nbR = (n1 + 255) / 256, tiles = (n1 + 63) / 64;
    hipLaunchKernelGGL(forget_apply_kernel, dim3(nbR + tiles * ((n1 + 3) / 4), D), dim3(256), 0, s, h->iK.p, h->linv.p, h->beta.p,
                       ws, bs, n, j, ldw, nbR, h->gram.p, h->Tm.p, h->zvec.p);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

int launch_forget_pack(Handle* h, const ForgetRows& rm, int n1, int D, int E, double* Xn, double* Yn, bool tables, hipStream_t s) {
    int nb = (n1 * (E > D ? E : D) + 255) / 256;
    if (nb > 64) nb = 64;
    if (nb < E) nb = E;
    hipLaunchKernelGGL(forget_pack_kernel, dim3(nb), dim3(256), 0, s, h->Xc.p, h->Yc.p, rm, n1, D, E, Xn, Yn,
                       tables ? h->Xt.p : nullptr, tables ? h->xrange.p : nullptr);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

}  // namespace gpmpc_hip
