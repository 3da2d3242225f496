// device_common.h -- device primitives shared by the kernel families: wavefront reductions and the LDS hand-off, the table
// exponential, the fp64 matrix-instruction helpers, the searches' clip01 / finite_d and the numbering of upper-triangle entries.
#pragma once
#include "gpmpc_internal.h"
#include <type_traits>

namespace gpmpc_hip {

// the fp64 4-vector of v_mfma_f64_16x16x4_f64 (accumulator / result of one 16 x 16 tile)
typedef double d4 __attribute__((ext_vector_type(4)));

// zero rows appended to every T_a = beta_a beta_a^T - iK_a (written by prepare, streamed by the rollout and gradient kernels):
// a wave may run CH <= 64 rows past the data and prefetches 4 more
constexpr int kTPad = 72;

// ------------------------------------------------------------------------------------------
// Wavefront sum on the DPP crossbar (no LDS round trips): inclusive scan inside each row of 16 lanes
// (row_shr 1,2,4,8), then row_bcast:15 / row_bcast:31 carry the row totals up; lane 63 holds the
// total, which is broadcast through an SGPR.  Fixed order => bitwise reproducible.
template <int CTRL, int ROW_MASK>
__device__ inline double dpp_shifted(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, true);
    return __hiloint2double(hi, lo);
}

// NV independent wavefront sums issued step by step side by side: every value goes through the SAME six DPP adds in the same
// order whatever NV is (so its bits do not depend on its neighbours); a tree on its own is six dependent DPP adds, NV of them
// fill each other's issue gaps.
template <int NV>
__device__ inline void wave_sum_n(double (&v)[NV]) {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] += dpp_shifted<0x111, 0xf>(v[k]);      // row_shr:1
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] += dpp_shifted<0x112, 0xf>(v[k]);      // row_shr:2
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] += dpp_shifted<0x114, 0xf>(v[k]);      // row_shr:4
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] += dpp_shifted<0x118, 0xf>(v[k]);      // row_shr:8
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] += dpp_shifted<0x142, 0xa>(v[k]);      // row_bcast:15 -> rows 1, 3
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] += dpp_shifted<0x143, 0xc>(v[k]);      // row_bcast:31 -> rows 2, 3
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int lo = __builtin_amdgcn_readlane(__double2loint(v[k]), 63);
        const int hi = __builtin_amdgcn_readlane(__double2hiint(v[k]), 63);
        v[k] = __hiloint2double(hi, lo);
    }
}

// One wavefront sum: the tree above for a single value (ONE copy of the order the bit fixtures depend on).
__device__ inline double wave_sum(double v) {
    double t[1] = {v};
    wave_sum_n(t);
    return t[0];
}

// Wavefront sum by an xor butterfly over offsets 32, 16, ..., 1: every lane ends with the total.  Fixed order.
__device__ inline double wave_xor_sum(double v) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ inline int wave_max_i32(int v) {
    auto step = [&](auto ctrl, auto rmask) {
        const int o = __builtin_amdgcn_update_dpp(0, v, decltype(ctrl)::value, decltype(rmask)::value, 0xf, true);
        v = o > v ? o : v;
    };
    step(std::integral_constant<int, 0x111>{}, std::integral_constant<int, 0xf>{});
    step(std::integral_constant<int, 0x112>{}, std::integral_constant<int, 0xf>{});
    step(std::integral_constant<int, 0x114>{}, std::integral_constant<int, 0xf>{});
    step(std::integral_constant<int, 0x118>{}, std::integral_constant<int, 0xf>{});
    step(std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{});
    step(std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{});
    return __builtin_amdgcn_readlane(v, 63);        // values are >= 0, so the zero fill is neutral
}

// LDS hand-off between lanes of ONE wavefront (no workgroup barrier): LDS operations of a wave
// complete in issue order; the fences keep the compiler from moving accesses across.
__device__ inline void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Sums over the wavefront of 16 (8) values per lane without the LDS crossbar: the halving "transpose" steps ride on
// v_permlane32_swap / v_permlane16_swap (gfx950: lanes 0-31 <-> 32-63, even <-> odd rows of 16) and on DPP row rotations with
// bank masks (lane bits 3 and 2) -- one exchange hands over the half a lane gives up AND brings in the partner's half of what it
// keeps, no selects -- then two quad_perm butterflies.  Lane l ends with the total of value (l >> 2) [& 7].  57 VALU instructions for
// 16 values against ~70 plus six dependent ds_bpermute round trips for the 8 values of wave_sum8 (rollout_kernel.h).  Fixed order.
__device__ inline double dbl_of(unsigned lo, unsigned hi) { return __hiloint2double((int)hi, (int)lo); }

template <int KIND>                     // 32: lane bit 5, 16: lane bit 4
__device__ inline double swap_add(double a, double b) {
    const unsigned a0 = (unsigned)__double2loint(a), a1 = (unsigned)__double2hiint(a);
    const unsigned b0 = (unsigned)__double2loint(b), b1 = (unsigned)__double2hiint(b);
    if constexpr (KIND == 32) {
        const auto r0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
        const auto r1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
        return dbl_of(r0[0], r1[0]) + dbl_of(r0[1], r1[1]);
    } else {
        const auto r0 = __builtin_amdgcn_permlane16_swap(a0, b0, false, false);
        const auto r1 = __builtin_amdgcn_permlane16_swap(a1, b1, false, false);
        return dbl_of(r0[0], r1[0]) + dbl_of(r0[1], r1[1]);
    }
}

template <int CTRL, int BANKS>
__device__ inline double dpp_merge(double old, double src) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(src), CTRL, 0xf, BANKS, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(src), CTRL, 0xf, BANKS, false);
    return __hiloint2double(hi, lo);
}

// lanes with bit 3 (2) clear keep `a`, the others `b`; both get the partner's (lane ^ 8, lane ^ 4) share of what they keep
__device__ inline double rot_add8(double a, double b) { return dpp_merge<0x128, 0x3>(b, a) + dpp_merge<0x128, 0xc>(a, b); }
__device__ inline double rot_add4(double a, double b) { return dpp_merge<0x12c, 0x5>(b, a) + dpp_merge<0x124, 0xa>(a, b); }

__device__ inline double quad_total(double r) {
    r += dpp_merge<0x4e, 0xf>(r, r);          // quad_perm [2, 3, 0, 1]
    r += dpp_merge<0xb1, 0xf>(r, r);          // quad_perm [1, 0, 3, 2]
    return r;
}

__device__ inline double wave_reduce16(const double (&v)[16]) {
    double w8[8], w4[4], w2[2];
#pragma unroll
    for (int k = 0; k < 8; ++k) w8[k] = swap_add<32>(v[k], v[k + 8]);
#pragma unroll
    for (int k = 0; k < 4; ++k) w4[k] = swap_add<16>(w8[k], w8[k + 4]);
#pragma unroll
    for (int k = 0; k < 2; ++k) w2[k] = rot_add8(w4[k], w4[k + 2]);
    return quad_total(rot_add4(w2[0], w2[1]));
}

__device__ inline double wave_reduce8(const double (&v)[8]) {
    double w4[4], w2[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) w4[k] = swap_add<16>(v[k], v[k + 4]);
#pragma unroll
    for (int k = 0; k < 2; ++k) w2[k] = rot_add8(w4[k], w4[k + 2]);
    const double r = quad_total(rot_add4(w2[0], w2[1]));
    return swap_add<32>(r, r);
}

// ------------------------------------------------------------------------------------------
// exp(x) for the direct (fallback) evaluation: x = (64 m + j) ln2/64 + r, |r| <= ln2/128,
// exp(x) = 2^m * 2^(j/64) * (1 + r + r^2/2 + ... + r^5/120); 2^(j/64) from a 64-entry table, truncation
// 3.5e-17, total error ~1 ulp.  No overflow/underflow special-casing: arguments on this path are sums of
// log-kernel terms (<= a few units), and ldexp flushes tiny results to zero like exp does.
__device__ const double kExp2Tab[64] = {
    0x1.0000000000000p+0, 0x1.02c9a3e778061p+0, 0x1.059b0d3158574p+0, 0x1.0874518759bc8p+0,
    0x1.0b5586cf9890fp+0, 0x1.0e3ec32d3d1a2p+0, 0x1.11301d0125b51p+0, 0x1.1429aaea92de0p+0,
    0x1.172b83c7d517bp+0, 0x1.1a35beb6fcb75p+0, 0x1.1d4873168b9aap+0, 0x1.2063b88628cd6p+0,
    0x1.2387a6e756238p+0, 0x1.26b4565e27cddp+0, 0x1.29e9df51fdee1p+0, 0x1.2d285a6e4030bp+0,
    0x1.306fe0a31b715p+0, 0x1.33c08b26416ffp+0, 0x1.371a7373aa9cbp+0, 0x1.3a7db34e59ff7p+0,
    0x1.3dea64c123422p+0, 0x1.4160a21f72e2ap+0, 0x1.44e086061892dp+0, 0x1.486a2b5c13cd0p+0,
    0x1.4bfdad5362a27p+0, 0x1.4f9b2769d2ca7p+0, 0x1.5342b569d4f82p+0, 0x1.56f4736b527dap+0,
    0x1.5ab07dd485429p+0, 0x1.5e76f15ad2148p+0, 0x1.6247eb03a5585p+0, 0x1.6623882552225p+0,
    0x1.6a09e667f3bcdp+0, 0x1.6dfb23c651a2fp+0, 0x1.71f75e8ec5f74p+0, 0x1.75feb564267c9p+0,
    0x1.7a11473eb0187p+0, 0x1.7e2f336cf4e62p+0, 0x1.82589994cce13p+0, 0x1.868d99b4492edp+0,
    0x1.8ace5422aa0dbp+0, 0x1.8f1ae99157736p+0, 0x1.93737b0cdc5e5p+0, 0x1.97d829fde4e50p+0,
    0x1.9c49182a3f090p+0, 0x1.a0c667b5de565p+0, 0x1.a5503b23e255dp+0, 0x1.a9e6b5579fdbfp+0,
    0x1.ae89f995ad3adp+0, 0x1.b33a2b84f15fbp+0, 0x1.b7f76f2fb5e47p+0, 0x1.bcc1e904bc1d2p+0,
    0x1.c199bdd85529cp+0, 0x1.c67f12e57d14bp+0, 0x1.cb720dcef9069p+0, 0x1.d072d4a07897cp+0,
    0x1.d5818dcfba487p+0, 0x1.da9e603db3285p+0, 0x1.dfc97337b9b5fp+0, 0x1.e502ee78b3ff6p+0,
    0x1.ea4afa2a490dap+0, 0x1.efa1bee615a27p+0, 0x1.f50765b6e4540p+0, 0x1.fa7c1819e90d8p+0};

// kExp2Tab into LDS for fast_exp: thread `tid` of `nthreads` copies every nthreads-th entry
__device__ inline void stage_exp_tab(double* tab, int tid, int nthreads) {
    for (int i = tid; i < 64; i += nthreads) tab[i] = kExp2Tab[i];
}

__device__ inline double fast_exp(double x, const double* tab /* kExp2Tab copied to LDS */) {
    const double n = __builtin_rint(x * 0x1.71547652b82fep+6);
    double r = fma(n, -0x1.62e42fefa0000p-7, x);
    r = fma(n, -0x1.cf79abc9e3b3ap-46, r);
    const int ni = (int)n;
    const double t = tab[ni & 63];
    double q = fma(r, 0x1.1111111111111p-7, 0x1.5555555555555p-5);     // 1/120, 1/24
    q = fma(q, r, 0x1.5555555555555p-3);                                 // 1/6
    q = fma(q, r, 0.5);
    const double p = fma(q * r, r, r);                                    // e^r - 1
    return ldexp(fma(t, p, t), ni >> 6);
}

// ------------------------------------------------------------------------------------------
// 1 / sqrt(d), d > 0: fp32 v_rsq seed (1 ulp) + two Newton steps y <- y (1.5 - 0.5 d y^2): relative error ~2^-85 before
// rounding, 6 dependent fp64 operations instead of ~35 for sqrt + divide
__device__ inline double inv_sqrt_pos(double d) {
    double y = (double)__builtin_amdgcn_rsqf((float)d);
    const double h = 0.5 * d;
    y = y * fma(-h * y, y, 1.5);
    y = y * fma(-h * y, y, 1.5);
    return y;
}

// acc += sum over p in [pbeg, pend) of A(p) B(p) for one 16 x 16 tile with the operands straight from global memory:
// the loads of U k-steps are issued before the first MFMA of the group, so a group costs one memory round trip, not U
// (without it every v_mfma waited for its own two loads: the N^3 kernels ran at L2 latency, 8-21 TFLOP/s at N = 4096).
template <int U, typename FA, typename FB>
__device__ inline void mfma_kloop(d4& acc, int pbeg, int pend, int lk, FA loadA, FB loadB) {
    for (int pp = pbeg; pp < pend; pp += 4 * U) {
        double av[U], bv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int pk = pp + 4 * u + lk;
            const bool in = pk < pend;
            av[u] = in ? loadA(pk) : 0.0;
            bv[u] = in ? loadB(pk) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
    }
}

// ------------------------------------------------------------------------------------------
// The searches' scalar helpers.  clip01 sends NaN to 0 (fmax drops it); ilqr_clip01 (ilqr.hip) lets NaN through on purpose.
__device__ inline double clip01(double v) { return fmin(fmax(v, 0.0), 1.0); }
__device__ inline bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN

// ------------------------------------------------------------------------------------------
// Upper-triangle entries (d, e), d <= e < D, numbered row by row: (0,0) (0,1) .. (0,D-1) (1,1) ..
__host__ __device__ inline int tri_index(int d, int e, int D) { return d * D - (d * (d - 1)) / 2 + (e - d); }
// ... and back: k -> (d, e)
__device__ inline void decode_tri(int k, int D, int& d, int& e) {
    d = 0;
    while (k >= D - d) { k -= D - d; ++d; }
    e = d + k;
}

}  // namespace gpmpc_hip
