// grad.hip -- host-side dispatch of the analytic-gradient kernels (grad_kernels.h).
#include "grad_stream_kernel.h"
#include "grad_sep_kernel.h"
#include "moment_schedule.h"
#include <cstring>

namespace gpmpc_hip {

namespace {

constexpr int kMomThreads = 512;

template <int DP, int NXP>
int launch_moments(Handle* h, const GradArgs& g, size_t lds_bytes, hipStream_t s) {
    auto go = [&](auto kern, int nt) -> int {
        int rc = allow_full_lds(h, reinterpret_cast<const void*>(kern));
        if (rc) return rc;
        hipLaunchKernelGGL(kern, dim3(g.H, g.B, g.gz), dim3(nt), lds_bytes, s, g);
        GPMPC_HIP_CHECK(h, hipGetLastError());
        return GPMPC_OK;
    };
    if constexpr (DP <= 3) {
        // two 512-thread workgroups per CU (see pair_moments_kernel), or
        // 16 waves per (candidate, step): the accumulators fit the 128-VGPR budget of a 1024-thread workgroup
        if (g.share_cu) return go(pair_moments_kernel<DP, NXP, 512, 1>, 512);
        return go(pair_moments_kernel<DP, NXP, 1024, 1>, 1024);
    } else {
        return go(pair_moments_kernel<DP, NXP, kMomThreads, 1>, kMomThreads);
    }
}

// Few candidates (B x H x 2 <= CUs: the reference's one-sequence-per-evaluation regime): the element-wise moment pass, the mean
// moments and the stage costs / objective of the stored trajectory are independent of each other and each fills a fraction of
// the chip -- ONE grid runs them side by side (z < gz: pair groups, z = gz: mean moments, z = gz + 1 and x = 0: the candidate's
// costs) instead of three launches in a row (config-2 shape, B = 1: 23 + 7.5 + 12 us and two launch gaps -> ~24 us).
struct CostSlice {
    const double* cost; double kappa; int clip, use_constraints; double* cm; double* cv; double* J;
};
template <int DP, int NXP, int NT>
__global__ __launch_bounds__(NT) void few_candidate_moments_kernel(const GradArgs p, const CostSlice cs) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    if ((int)blockIdx.z < p.gz) { pair_moments_body<DP, NXP, NT, 1>(p, smem); return; }
    if ((int)blockIdx.z == p.gz) {
        if ((int)threadIdx.x >= 64 * DP) return;
        mean_moments_body<DP, NXP>(p, smem);
        return;
    }
    if (blockIdx.x != 0 || threadIdx.x >= 64) return;
    traj_cost_body<DP>(blockIdx.y, threadIdx.x, p.mu, p.Sig, p.actions, cs.cost, p.D, p.A, p.H, cs.kappa, cs.clip, cs.use_constraints,
                       cs.cm, cs.cv, cs.J);
}

// (cs.cost NULL: no stage costs are wanted -- the grid stops before the cost slice)
template <int DP, int NXP>
int launch_few_candidate_moments(Handle* h, const GradArgs& g, const CostSlice& cs, size_t lds_bytes, hipStream_t s) {
    constexpr int NT = DP <= 3 ? 1024 : kMomThreads;
    auto kern = few_candidate_moments_kernel<DP, NXP, NT>;
    int rc = allow_full_lds(h, reinterpret_cast<const void*>(kern));
    if (rc) return rc;
    hipLaunchKernelGGL(kern, dim3(g.H, g.B, g.gz + (cs.cost ? 2 : 1)), dim3(NT), lds_bytes, s, g, cs);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

template <int DP>
int launch_few_candidate_moments_dp(Handle* h, const GradArgs& g, const CostSlice& cs, size_t lds_bytes, hipStream_t s) {
    if (g.NXP == 1) return launch_few_candidate_moments<DP, 1>(h, g, cs, lds_bytes, s);
    return g.NXP == 2 ? launch_few_candidate_moments<DP, 2>(h, g, cs, lds_bytes, s) : launch_few_candidate_moments<DP, 6>(h, g, cs, lds_bytes, s);
}

template <int DP, int NT, bool SEEDED>
int launch_sweep(Handle* h, const std::conditional_t<SEEDED, SeededGradArgs, GradArgs>& g, size_t lds_bytes, hipStream_t s) {
    auto kern = (g.D == DP) ? adjoint_sweep_kernel<DP, NT, DP, SEEDED> : adjoint_sweep_kernel<DP, NT, 0, SEEDED>;
    int rc = allow_full_lds(h, reinterpret_cast<const void*>(kern));
    if (rc) return rc;
    hipLaunchKernelGGL(kern, dim3(g.B), dim3(NT), lds_bytes, s, g);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

template <int DP, int NXP>
int launch_moments_stream(Handle* h, const GradArgs& g, size_t lds_bytes, hipStream_t s) {
    auto kern = pair_moments_stream_kernel<DP, NXP>;
    int rc = allow_full_lds(h, reinterpret_cast<const void*>(kern));
    if (rc) return rc;
    hipLaunchKernelGGL(kern, dim3(g.H, g.B, g.gz), dim3(kGsThreads), lds_bytes, s, g);
    GPMPC_HIP_CHECK(h, hipGetLastError());
    return GPMPC_OK;
}

template <int DP>
int launch_moments_stream_dp(Handle* h, const GradArgs& g, size_t lds_bytes, hipStream_t s) {
    if (g.NXP == 1) return launch_moments_stream<DP, 1>(h, g, lds_bytes, s);
    return g.NXP == 2 ? launch_moments_stream<DP, 2>(h, g, lds_bytes, s) : launch_moments_stream<DP, 6>(h, g, lds_bytes, s);
}

template <int DP>
int launch_moments_dp(Handle* h, const GradArgs& g, size_t lds_bytes, hipStream_t s) {
    if (g.NXP == 1) return launch_moments<DP, 1>(h, g, lds_bytes, s);
    return g.NXP == 2 ? launch_moments<DP, 2>(h, g, lds_bytes, s) : launch_moments<DP, 6>(h, g, lds_bytes, s);
}

template <bool SEEDED>
int dispatch_sweep(Handle* h, const std::conditional_t<SEEDED, SeededGradArgs, GradArgs>& g, int DP, int sweep_nt, size_t lds,
                   hipStream_t s) {
    switch (DP) {
        case 2:  return sweep_nt == 512 ? launch_sweep<2, 512, SEEDED>(h, g, lds, s) : (sweep_nt == 256 ? launch_sweep<2, 256, SEEDED>(h, g, lds, s) : launch_sweep<2, 64, SEEDED>(h, g, lds, s));
        case 3:  return sweep_nt == 512 ? launch_sweep<3, 512, SEEDED>(h, g, lds, s) : (sweep_nt == 256 ? launch_sweep<3, 256, SEEDED>(h, g, lds, s) : launch_sweep<3, 64, SEEDED>(h, g, lds, s));
        case 4:  return sweep_nt == 512 ? launch_sweep<4, 512, SEEDED>(h, g, lds, s) : (sweep_nt == 256 ? launch_sweep<4, 256, SEEDED>(h, g, lds, s) : launch_sweep<4, 64, SEEDED>(h, g, lds, s));
        case 6:  return launch_sweep<6, 256, SEEDED>(h, g, lds, s);
        default: return launch_sweep<8, 256, SEEDED>(h, g, lds, s);
    }
}

}  // namespace

int plan_rollout_grad(Handle* h, int N, int D, int A, int E, int H, int B, int Bp, bool seeded, GradPlan& p) {
    p = GradPlan{};
    const int NX = E - D, P = D * (D + 1) / 2;
    int DP = 0;
    for (int v : {2, 3, 4, 6, 8}) if (D <= v) { DP = v; break; }
    if (DP == 0 || NX > 6) { h->err = "gradient: supported for D <= 8 with A (+ time) <= 6, and for 8 < D <= 16"; return GPMPC_ERR_LIMIT; }
    const int NXP = NX <= 1 ? 1 : (NX <= 2 ? 2 : 6);
    const int RS = grad_row_stride(DP, NXP);
    const int NSP = 1 + DP + DP * (DP + 1) / 2 + NXP;
    p.DP = DP; p.NXP = NXP; p.RS = RS; p.NSP = NSP;

    // tiling of the pairwise pass: row chunks of CH rows (64 to start with; the LDS-resident pass re-plans with the schedule model's
    // answer once it is known which pairs it is left with), as many output pairs per group as the LDS holds
    // one column per lane (two need > 128 VGPRs, i.e. 8 waves instead of 16 per workgroup: measured slower at config 2,
    // 2.86 vs 2.10 ms, round 3 -- that instantiation is no longer built)
    const int cols = 1;
    const int NCU = (N + cols - 1) / cols;
    // D <= 4: the sweep is one wavefront's, its prologue (cost adjoints and state-independent algebra of all H steps) every
    // wavefront's of the launch -- 8 of them (512 threads: 256 VGPRs, the 1024-thread form spills at D = 4) while each candidate has a CU to itself, 4 up to four per CU, else the one
    p.sweep_nt = DP <= 4 ? (B <= h->num_cu ? 512 : (B <= 4 * h->num_cu ? 256 : 64)) : 256;
    MomTiling& m = p.pass;
    int pairs_left = P;              // pairs the LDS-resident pass works on
    size_t lds_budget = (size_t)h->lds_limit;
    // pairs per group (as many as the LDS budget holds, 0: none) and the LDS bytes for row chunks of `chunk_rows`
    auto fit = [&](int chunk_rows, int npairs, size_t budget, size_t& bytes) {
        const int rc_ = (N + chunk_rows - 1) / chunk_rows, nr_ = rc_ * chunk_rows, wpp_ = (rc_ * NCU + 63) / 64;
        for (int gg = npairs; gg >= 1; --gg) {
            const MomLayout L = make_mom_layout(N, D, E, gg, RS, nr_, wpp_, NSP);
            if ((size_t)L.total * 8 <= budget) { bytes = (size_t)L.total * 8; return gg; }
        }
        bytes = 0;
        return 0;
    };
    auto plan = [&](int chunk_rows) {
        m.CH = chunk_rows; m.RC = (N + m.CH - 1) / m.CH;
        const int NR = m.RC * m.CH;
        m.wpp = (m.RC * NCU + 63) / 64;
        m.gz = 1;
        m.G = fit(m.CH, pairs_left, lds_budget, m.lds);
        // a small batch leaves most CUs idle: spread the pair groups of each (candidate, step) over up to P workgroups
        if (m.G > 0 && (long long)B * H * 2 <= h->num_cu) {
            int zmax = h->num_cu / (B * H);
            if (zmax > P) zmax = P;
            const int Gs = (P + zmax - 1) / zmax;            // pairs per workgroup
            if (Gs < m.G) { m.G = Gs; const MomLayout L = make_mom_layout(N, D, E, m.G, RS, NR, m.wpp, NSP); m.lds = (size_t)L.total * 8; }
            m.gz = (P + m.G - 1) / m.G;
        }
        return m.G > 0 && (unsigned long long)m.RC * NCU * NCU < 0x100000000ULL && (unsigned long long)m.G * m.wpp * m.wpp < 0x100000000ULL;
    };
    const int CH0 = (N >= 64) ? 64 : ((N + 3) & ~3);
    plan(CH0);
    if (DP <= 4) {               // state-independent small algebra of all steps up front when it fits beside the rest
        const SweepLayout Lp = make_sweep_layout(D, A, E, H, NSP, p.sweep_nt / 64, 0, H);
        if ((size_t)Lp.total * 8 <= 96 * 1024) p.pre_steps = H;
    }
    const SweepLayout SL = make_sweep_layout(D, A, E, H, NSP, p.sweep_nt / 64, DP <= 4 ? 0 : kSweepAug, p.pre_steps, seeded ? H + 1 : 0);
    p.sweep_lds = (size_t)SL.total * 8;
    if (p.sweep_lds > (size_t)h->lds_limit) { h->err = "gradient: horizon too long for the reverse sweep's LDS"; return GPMPC_ERR_LIMIT; }
    // memories whose per-point arrays do not fit the LDS (or on request) take the streaming moment pass
    p.stream = (m.G == 0) || h->opt_grad_stream == 1;
    if (p.stream) {
        const GsLayout GL = make_gs_layout(N, D, E, DP, NXP, RS, NSP);
        p.gs_lds = (size_t)GL.total * 8;
        if (p.gs_lds > (size_t)h->lds_limit) { h->err = "gradient: N too large for the column-factor array of the streaming moment pass"; return GPMPC_ERR_LIMIT; }
        m.gz = 1;
        if ((long long)B * H * 2 <= h->num_cu) { m.gz = h->num_cu / (B * H); if (m.gz > P) m.gz = P; }
    } else if ((unsigned long long)m.RC * NCU * NCU >= 0x100000000ULL || (unsigned long long)m.G * m.wpp * m.wpp >= 0x100000000ULL) {
        h->err = "gradient: index range too large for the multiply-high division"; return GPMPC_ERR_LIMIT;
    }
    p.first = m;

    // Diagonal pairs batch-major (pair_tile_grad_kernel.h) once the tables T_a are large and the batch fills the chip.  When the
    // forward itself takes the batch-major path, its tile pass forms these moments on the way (the same E_ij would otherwise be
    // evaluated twice: once for the forward's sums, once for the moments).
    p.tiles = h->opt_grad_tiles != 0 && D >= 2 && D <= 4 && tile_moments_supported(*h, D, E, NSP) &&
              (h->opt_grad_tiles == 2 || (tables_outgrow_l2(N, D) && (long long)B * H >= 2LL * h->num_cu));
    // few candidates: the stage costs / objective ride in the moment launch (few_candidate_moments_kernel)
    p.few = DP <= 4 && !p.stream && h->opt_grad_mean != 0 && (long long)B * H * 2 <= h->num_cu && m.lds >= 64 * sizeof(double);
    int rc = plan_rollout(*h, N, D, A, E, H, Bp, RolloutRequest{p.tiles, p.few}, p.fwd);
    if (rc) { h->err = p.fwd.err; return rc; }
    p.fused = p.fwd.fused_tiles;

    // Off-diagonal pairs in separable form on the matrix cores (grad_sep_kernel.h) where the Taylor degree allows; the
    // element-wise kernels skip the pairs it wrote.  Monomial tables: those of the forward kernel (ensure_monomials).
    // Measured (round 3, objective + gradient per launch, separable / element-wise): config 1 (N = 50, B = 256) 0.77 / 0.66 ms,
    // config 2 (N = 200) B = 256: 2.22 / 2.57 ms, B = 1: 0.65 / 0.61 ms (25 workgroups: the element-wise pass spreads its pair
    // groups over the idle CUs), config 3 (N = 500, B = 1024) 18.9 / 24.8 ms, config 4 (N = 1000, B = 2048): 69 ms for the 6
    // off-diagonal pairs against ~650 ms.  Hence from N = 128 on when the items fill the chip (option "grad_separable": 0 never,
    // 1 auto, 2 always).
    if (h->opt_grad_sep != 0 && ((N >= 128 && (long long)B * H >= h->num_cu) || h->opt_grad_sep == 2) && D >= 2 && D <= 4 && h->mono_D == D && h->mono_CM > 0 &&
        h->opt_force_path == 0) {
        int kmax = 0;
        for (int k = 1; k <= h->sep_kmax && k <= kMaxTaylor; ++k)
            if (h->mono_cum[k] <= 16 * kSepGradBlocks) kmax = k;
        const int nWt = 1 + D + D * (D + 1) / 2 + NX;
        if (kmax > 0 && nWt <= 32) {
            // weightings beyond a multiple of 16 (one or two) are accumulated on the VALU instead of opening another A block
            const int NE = (nWt > 16 && nWt % 16 != 0 && nWt % 16 <= 2) ? nWt % 16 : 0;
            const int NA = NE ? nWt / 16 : (nWt + 15) / 16;
            const bool v2 = sep_grad_version(DP) == 2;
            const int PS = v2 ? sep_grad_point_words(D, 16 * NA + NE, kmax) : sep_grad_point_words_v1(D, NX, kmax);
            const int chunk = v2 ? sep_grad_chunk(DP) : 64;
            const int mat_words = nWt * 16 * kSepGradBlocks;          // moment matrix of a (pair, side): weightings x monomial slots
            const int wave_words = chunk * PS > mat_words ? chunk * PS : mat_words;
            const int Poff = P - D;
            const size_t lds = ((size_t)rnd2(E) + rnd2(D * E) + rnd2((Poff > 0 ? Poff : 1) * DP * DP) + 64 + 8 + 16 * kSepGradBlocks
                                + 8 * kSepGradBlocks + 8 + (size_t)sep_grad_waves(DP) * wave_words) * sizeof(double);
            if (lds <= (size_t)h->lds_limit) {
                p.sep = true;
                p.sep_kmax = kmax; p.sep_NA = NA; p.sep_NE = NE; p.sep_PS = PS; p.sep_wave_words = wave_words; p.sep_lds = lds;
            }
        }
    }
    // the few-candidate launch takes the element-wise moments, the mean moments and the stage costs when no other pass took pairs
    p.merged = p.few && !p.sep && !p.tiles;
    p.path = (p.sep ? 1 : 0) | (p.tiles ? 2 : 0) | (p.fused ? 16 : 0) | (p.stream ? 4 : 0) |
             (DP <= 4 && h->opt_grad_mean != 0 ? 32 : 0) | (p.merged ? 64 : 0);
    pairs_left = P - (p.tiles ? D : 0) - (p.sep ? P - D : 0);
    p.pairs_left = pairs_left = pairs_left > 0 ? pairs_left : 1;
    if (p.stream) return GPMPC_OK;

    // Two workgroups per CU, half the LDS each (option "grad_share_cu": 0 auto, 1 wherever it fits, 2 never).  Measured
    // (profiles/r04j_grad_sweep.txt, objective + gradient per launch): config 2 B = 256 2.04 -> 1.84 ms, B = 1024 7.57 -> 7.01,
    // config 1 B = 2048 3.58 -> 2.92, config 3 B = 1024 18.2 -> 17.7; nothing at B = 1 -- hence from two workgroups per CU on.
    bool share = DP <= 3 && cols == 1 && h->opt_grad_share != 2 && (h->opt_grad_share == 1 || (long long)B * H >= 2LL * h->num_cu);
    if (share) {
        lds_budget = (size_t)h->lds_limit / 2;
        if (!plan(CH0)) { share = false; lds_budget = (size_t)h->lds_limit; }
    }
    // Row-chunk length from the schedule model (moment_schedule.h), as a function of the MODEL'S SHAPE ONLY -- evaluated for the
    // throughput configuration (the pairs the element-wise pass keeps when the separable pass takes the off-diagonal ones,
    // two workgroups per CU where they fit, no spreading over blockIdx.z) whatever the batch at hand: every pair's sums are
    // then formed in the same order for any batch size, grouping and workgroup shape.  The objective and gradient of a
    // candidate as a whole are bit-identical alone and inside a batch only while both launches take the same forms: the
    // cooperative forward and the few-candidate moment launch, i.e. 2 B H <= CUs (tests/test_gpu_batch_invariance.py); past
    // that the forward's and the moment pass's summation orders change with the batch (1e-9 relative at N = 200, B = 128).
    int want = CH0;
    if (h->opt_grad_chunk > 0) want = h->opt_grad_chunk < CH0 ? h->opt_grad_chunk : CH0;
    else {
        const bool sep_shape = h->opt_grad_sep != 0 && N >= 128 && D >= 2 && D <= 4 && h->opt_force_path == 0;
        std::vector<int> pair_is_diag;
        for (int a1 = 0; a1 < D; ++a1)
            for (int b1 = a1; b1 < D; ++b1)
                if (a1 == b1 || !sep_shape) pair_is_diag.push_back(a1 == b1 ? 1 : 0);
        const int npairs = (int)pair_is_diag.size();
        size_t bytes = 0;
        const bool two = DP <= 3 && cols == 1 && h->opt_grad_share != 2 && fit(CH0, npairs, (size_t)h->lds_limit / 2, bytes) > 0;
        const size_t budget = two ? (size_t)h->lds_limit / 2 : (size_t)h->lds_limit;
        const int NW = (cols == 2 || two) ? 8 : (DP <= 3 ? 16 : 8);
        const int key[8] = {N, D, E, cols, NW, (int)(budget >> 10), npairs, sep_shape ? 1 : 0};
        if (memcmp(key, h->chunk_key, sizeof key) == 0 && h->chunk_rows > 0) want = h->chunk_rows;
        else {
            want = choose_moment_chunk(N, cols, NW, CH0, pair_is_diag, [&](int c, int& Gc, int& gzc) {
                size_t bb = 0;
                Gc = fit(c, npairs, budget, bb);
                gzc = 1;
                return Gc > 0;
            });
            memcpy(h->chunk_key, key, sizeof key);
            h->chunk_rows = want;
        }
    }
    if (!plan(want) && share) {                 // the chosen chunk does not fit twice: one workgroup per CU rather than another chunk length
        share = false;
        lds_budget = (size_t)h->lds_limit;
    }
    if (!plan(want)) plan(CH0);
    p.share_cu = share;
    return GPMPC_OK;
}

int launch_rollout_grad(Handle* h, RolloutArgs& a, double* grad_out, hipStream_t s, const RolloutSeeds* seeds) {
    const int N = a.N, D = a.D, A = a.A, E = a.E, H = a.H, B = a.B;
    const int NX = E - D, P = D * (D + 1) / 2;
    h->last_grad_path = 0;
    if (D > 8) { h->last_grad_path = 8; return launch_rollout_grad_wide(h, a, grad_out, s, seeds); }
    const bool costs = !seeds || seeds->cost;      // (a backward of the trajectory alone: no stage costs, no cost settings read)
    int rc = ensure_rollout_tables(h, N, D);
    if (rc) return rc;
    GradPlan p;
    rc = plan_rollout_grad(h, N, D, A, E, H, B, a.B_plan > B ? a.B_plan : B, seeds != nullptr, p);
    if (rc) return rc;
    const int DP = p.DP, NXP = p.NXP, NSP = p.NSP;

    // workspace: moments, mean sums, cost variances (when the caller does not keep them), flags of the separable pass
    const size_t n_mom = (size_t)B * H * P * NSP, n_ms = (size_t)B * H * D * mean_moment_count(D, NX), n_cv = (size_t)B * (H + 1);
    const size_t n_flag = ((size_t)B * H * P + 1) / 2;
    rc = grow(h, h->gradws, n_mom + n_ms + n_cv + n_flag);
    if (rc) return rc;
    GradArgs g;
    memset(&g, 0, sizeof g);
    g.mom = h->gradws.p;
    g.msum = g.mom + n_mom;
    int* sep_flags = reinterpret_cast<int*>(g.msum + n_ms + n_cv);
    if (!a.cv_out && costs) a.cv_out = g.msum + n_ms;
    // (the flags of the diagonal pairs are written DURING the forward when its tile pass forms their moments)
    if (p.tiles) GPMPC_HIP_CHECK(h, hipMemsetAsync(sep_flags, 0, (size_t)B * H * P * sizeof(int), s));
    if (p.fused) { a.grad_mom = g.mom; a.grad_done = sep_flags; a.grad_NSP = NSP; a.grad_NXP = NXP; }
    double* want_cm = a.cm_out; double* want_J = a.J_out;
    rc = launch_rollout(h, a, p.fwd, s);            // forward: trajectory, costs, J (+ the fused tile moments)
    if (rc) return rc;
    h->last_grad_path = p.path;

    g.Xt = a.Xt; g.beta = a.beta; g.Tm = a.Tm; g.ils2 = a.ils2; g.var = a.var; g.logvar = a.logvar; g.cost = a.cost;
    g.kappa = a.kappa; g.use_constraints = a.use_constraints;
    g.actions = a.actions; g.mu = a.mu_out; g.Sig = a.Sig_out; g.cv = a.cv_out;
    g.N = N; g.D = D; g.A = A; g.E = E; g.H = H; g.B = B; g.include_time = a.include_time; g.time0 = a.time0;
    g.grad = grad_out;
    g.DP = DP; g.NXP = NXP; g.NSP = NSP;
    g.pre_steps = p.pre_steps;
    g.cols = 1;
    g.host_out = h->hx_out; g.host_src = h->hx_src; g.host_n = (B == 1) ? h->hx_n : 0;
    g.host_flag = h->hio_flag_dev; g.host_flag_value = h->hio_seq;
    auto publish = [&](const MomTiling& m) {
        g.G = m.G; g.CH = m.CH; g.RC = m.RC; g.wpp = m.wpp; g.gz = m.gz;
        g.magic_N = magic_div((unsigned)N); g.magic_wpp = magic_div((unsigned)m.wpp);
    };
    publish(p.first);
    g.xrange = h->xrange.p; g.force_path = h->opt_force_path;
    if (p.sep) {
        SepGradArgs sg;
        memset(&sg, 0, sizeof sg);
        sg.Xt = a.Xt; sg.beta = a.beta; sg.ils2 = a.ils2; sg.logvar = a.logvar; sg.xrange = h->xrange.p; sg.actions = a.actions;
        sg.mu = a.mu_out; sg.Sig = a.Sig_out; sg.mono_exp = h->mono_exp; sg.mono_w = h->mono_w.p;
        sg.mom = g.mom; sg.done = sep_flags;
        for (int k = 0; k < 16; ++k) sg.mono_cum[k] = h->mono_cum[k];
        sg.N = N; sg.D = D; sg.A = A; sg.E = E; sg.H = H; sg.B = B; sg.include_time = a.include_time; sg.time0 = a.time0;
        sg.NSP = NSP; sg.NXP = NXP; sg.kmax = p.sep_kmax; sg.force_path = h->opt_force_path;
        sg.keep_diag_flags = p.fused ? 1 : 0;          // the fused forward already wrote the diagonal pairs' flags
        sg.PS = p.sep_PS; sg.wave_words = p.sep_wave_words;
        auto launch = [&](auto kern) -> int {
            int r2 = allow_full_lds(h, reinterpret_cast<const void*>(kern));
            if (r2) return r2;
            hipLaunchKernelGGL(kern, dim3(H, B), dim3(64 * sep_grad_waves(DP)), p.sep_lds, s, sg);
            GPMPC_HIP_CHECK(h, hipGetLastError());
            return GPMPC_OK;
        };
        if (DP == 2) rc = launch(sep_grad_moments_kernel<2, 1>);
        else if (DP == 3) rc = launch(sep_grad_moments_kernel<3, 1>);
        else if (p.sep_NE) rc = (p.sep_NE == 1) ? launch(sep_grad_moments_kernel<4, 1, 1>) : launch(sep_grad_moments_kernel<4, 1, 2>);
        else rc = (p.sep_NA == 1) ? launch(sep_grad_moments_kernel<4, 1>) : launch(sep_grad_moments_kernel<4, 2>);
        if (rc) return rc;
        g.sepdone = sep_flags;
    }
    // Diagonal pairs batch-major over all (candidate, step) items of the stored trajectory when the forward did not form them;
    // the element-wise pass below keeps the mean sums and whatever is flagged 0.
    if (p.tiles && !p.fused) {
        if (!p.sep) GPMPC_HIP_CHECK(h, hipMemsetAsync(sep_flags, 0, (size_t)B * H * P * sizeof(int), s));
        rc = launch_tile_moments(h, a, g.mom, sep_flags, NSP, NXP, s);
        if (rc) return rc;
    }
    if (p.tiles) g.sepdone = sep_flags;
    if (p.few && !p.merged && costs) {
        // (the separable / tile passes took pairs after all: the costs as their own launch)
        rc = launch_traj_cost(h, a, want_cm, a.cv_out, want_J, s);
        if (rc) return rc;
    }
    if (DP <= 4 && h->opt_grad_mean != 0 && !p.merged) {
        // the mean part on its own, lanes over points (mean_moments_kernel): 22 -> ~1 ms of a config-4 launch (streaming pass); in the
        // LDS-resident pass it was a quarter of the kernel's time per (candidate, step) at config 2 (profiles/r04j_moment_phases.txt)
        auto launch = [&](auto kern) -> int {
            hipLaunchKernelGGL(kern, dim3(H, B), dim3(64 * DP), 0, s, g);
            GPMPC_HIP_CHECK(h, hipGetLastError());
            return GPMPC_OK;
        };
        if (DP == 2) rc = NXP == 1 ? launch(mean_moments_kernel<2, 1>) : (NXP == 2 ? launch(mean_moments_kernel<2, 2>) : launch(mean_moments_kernel<2, 6>));
        else if (DP == 3) rc = NXP == 1 ? launch(mean_moments_kernel<3, 1>) : (NXP == 2 ? launch(mean_moments_kernel<3, 2>) : launch(mean_moments_kernel<3, 6>));
        else rc = NXP == 1 ? launch(mean_moments_kernel<4, 1>) : (NXP == 2 ? launch(mean_moments_kernel<4, 2>) : launch(mean_moments_kernel<4, 6>));
        if (rc) return rc;
        g.mean_done = 1;
    }
    if (p.stream) {
        switch (DP) {
            case 2:  rc = launch_moments_stream_dp<2>(h, g, p.gs_lds, s); break;
            case 3:  rc = launch_moments_stream_dp<3>(h, g, p.gs_lds, s); break;
            case 4:  rc = launch_moments_stream_dp<4>(h, g, p.gs_lds, s); break;
            case 6:  rc = launch_moments_stream_dp<6>(h, g, p.gs_lds, s); break;
            default: rc = launch_moments_stream_dp<8>(h, g, p.gs_lds, s); break;
        }
    } else {
        g.share_cu = p.share_cu ? 1 : 0;
        publish(p.pass);
        if (p.merged) {
            g.mean_done = 1;
            const CostSlice cs{costs ? a.cost : nullptr, a.kappa, a.clip, a.use_constraints, want_cm, a.cv_out, want_J};
            switch (DP) {
                case 2:  rc = launch_few_candidate_moments_dp<2>(h, g, cs, p.pass.lds, s); break;
                case 3:  rc = launch_few_candidate_moments_dp<3>(h, g, cs, p.pass.lds, s); break;
                default: rc = launch_few_candidate_moments_dp<4>(h, g, cs, p.pass.lds, s); break;
            }
        } else {
            switch (DP) {
                case 2:  rc = launch_moments_dp<2>(h, g, p.pass.lds, s); break;
                case 3:  rc = launch_moments_dp<3>(h, g, p.pass.lds, s); break;
                case 4:  rc = launch_moments_dp<4>(h, g, p.pass.lds, s); break;
                case 6:  rc = launch_moments_dp<6>(h, g, p.pass.lds, s); break;
                default: rc = launch_moments_dp<8>(h, g, p.pass.lds, s); break;
            }
        }
    }
    if (rc) return rc;
    if (seeds) {
        SeededGradArgs sg;
        static_cast<GradArgs&>(sg) = g;
        sg.host_n = 0;
        sg.sd = SweepSeeds{seeds->mu, seeds->Sig, seeds->cm, seeds->cv, seeds->J, seeds->mu0_bar, seeds->S0_bar};
        return dispatch_sweep<true>(h, sg, DP, p.sweep_nt, p.sweep_lds, s);
    }
    return dispatch_sweep<false>(h, g, DP, p.sweep_nt, p.sweep_lds, s);
}

}  // namespace gpmpc_hip
