// Internal declarations shared by the HIP translation units of libgpmpc_hip.so.
// gfx950 (MI355X / CDNA4) only: 64-lane wavefronts, 160 KiB LDS per CU, 256 CUs.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdio>
#include <string>
#include <unordered_set>

#include "../../include/gpmpc.h"

namespace gpmpc_hip {

constexpr int kMaxD = GPMPC_MAX_D;
constexpr int kMaxE = GPMPC_MAX_E;
constexpr int kWave = 64;

// ---------------------------------------------------------------------------------------
// Static owners of a horizon step's work items among the CS members of a candidate (cooperative form of the fused-horizon kernel,
// rollout_kernel.h), planned once per launch on the host and read by the kernel (owner tables, LDS slots of the pairs a member
// holds records of) and by the host (sizing those slots):
//   diagonal pairs (always element-wise): their D * wtri items in order, an equal contiguous share per member;
//   off-diagonal pair of ordinal o: k = max(1, CS / P_off) consecutive members starting at o k (mod CS) share its wpp element-wise
//   slots; the one of them with the fewest diagonal items owns the pair when it is separable (a separable pair is up to 14 more
//   items, and a member with more items than wavefronts runs a second round) -- so a member holds records of at most ~2 diagonal
//   and ~1 off-diagonal pairs whatever forms the step takes (all P pairs would not fit the LDS at D = 4 or large N);
//   mean sums of output a: one member each, counted down from the last, past the owners of separable pairs (a member with a
//   separable pair AND a mean sum runs three trips of the per-point pass where the others run two).
struct ClusterMap {
    int CS, D, P, P_off, wpp, wtri, koff;
    int CSd;                            // members that own diagonal items (all of them, or all but the separable pairs' owners)
    unsigned char sepown[8];            // owner of off-diagonal pair o when it is separable (D <= 4: P_off <= 6)
    unsigned char meanown[4];           // owner of the mean sums of output a
    unsigned char dmem[32];             // the diagonal members in order, and ...
    unsigned char didx[32];             // ... a member's position among them (255: none)
    __host__ __device__ int diag_owner(int ord, int slot) const { return dmem[((ord * wtri + slot) * CSd) / (D * wtri)]; }
    __host__ __device__ int off_owner(int ord, int slot) const { return ((slot * koff) / wpp + ord * koff) % CS; }
    __host__ __device__ int sep_owner(int ord) const { return sepown[ord]; }
    __host__ __device__ int mean_owner(int a) const { return meanown[a]; }
    __host__ __device__ bool diag_needed(int ord, int m) const {
        const int i = didx[m];
        return i != 255 && ((ord * wtri) * CSd) / (D * wtri) <= i && i <= (((ord + 1) * wtri - 1) * CSd) / (D * wtri);
    }
    __host__ __device__ bool off_needed(int ord, int m) const {            // owns an element-wise slot, or the separable pair
        if (sep_owner(ord) == m) return true;
        const int mp = ((m - (ord * koff) % CS) % CS + CS) % CS;
        if (mp >= koff) return false;
        const int s0 = (mp * wpp + koff - 1) / koff;
        return s0 < wpp && (s0 * koff) / wpp == mp;
    }
    int diag_count(int m) const {                                          // element-wise items of the diagonal pairs member m owns
        const int i = didx[m], T = D * wtri;
        return i == 255 ? 0 : ((i + 1) * T + CSd - 1) / CSd - (i * T + CSd - 1) / CSd;
    }
    int slots_needed(int m) const {                                        // pairs member m holds per-point records of
        int n = 0;
        for (int a = 0; a < D; ++a) n += diag_needed(a, m) ? 1 : 0;
        for (int o = 0; o < P_off; ++o) n += off_needed(o, m) ? 1 : 0;
        return n;
    }
    void plan(int cs, int d, int wpp_, int wtri_) {                        // host
        CS = cs; D = d; P = d * (d + 1) / 2; P_off = d * (d - 1) / 2; wpp = wpp_; wtri = wtri_ > 0 ? wtri_ : 1;
        koff = P_off > 0 ? CS / P_off : 1;
        if (koff < 1) koff = 1;
        auto everybody = [&] { CSd = CS; for (int m = 0; m < 32; ++m) { dmem[m] = (unsigned char)(m < CS ? m : 0); didx[m] = (unsigned char)(m < CS ? m : 255); } };
        everybody();
        bool taken[64] = {false};
        // Members to spare (two per diagonal pair remain): the separable pairs get owners of their OWN, without diagonal items.
        // A member's per-point pass then covers two problems (a diagonal pair + a mean sum, or the two sides of its off-diagonal
        // pair) = one trip of its lanes at N <= ~220 instead of two (round 6, config 2: the three members that owned a separable
        // pair AND diagonal items had 600-800 per-point items on 448 lanes, and everybody waited for them once per step).
        const bool dedicated = P_off > 0 && P_off <= 8 && CS - P_off >= 2 * D && koff * P_off <= CS;
        for (int o = 0; o < P_off && o < 8; ++o) {
            int best = (o * koff) % CS;
            if (!dedicated)
                for (int k = 1; k < koff; ++k) {
                    const int m = (o * koff + k) % CS;
                    if (diag_count(m) <= diag_count(best)) best = m;
                }
            sepown[o] = (unsigned char)best;
            taken[best] = true;
        }
        if (dedicated) {
            CSd = 0;
            for (int m = 0; m < 32; ++m) didx[m] = 255;
            for (int m = 0; m < CS; ++m)
                if (!taken[m]) { dmem[CSd] = (unsigned char)m; didx[m] = (unsigned char)CSd; ++CSd; }
        }
        for (int a = 0; a < D && a < 4; ++a) {
            int pick = -1;
            for (int m = CS - 1, k = 0; m >= 0 && pick < 0; --m)
                if (!taken[m]) { if (k == a) pick = m; ++k; }
            meanown[a] = (unsigned char)(pick >= 0 ? pick : (a * CS / D) % CS);
        }
    }
};

// ---------------------------------------------------------------------------------------
// Kernel argument block of the rollout kernel (passed by value, < 4 KiB).
constexpr int kInlineActs = 64;
struct RolloutArgs {
    // cached model (device)
    const double* Xt;      // (E, N)  inputs, structure-of-arrays
    const double* beta;    // (D, N)
    const double* Tm;      // (D, N, N)  beta beta^T - iK with the diagonal halved
    const double* ils2;    // (D, E)  1 / lengthscale^2
    const double* var;     // (D)     outputscale
    const double* logvar;  // (D)
    // cost block (device): target (D+A) | W (D+A)^2 | W_T D^2 | smin D | smax D
    const double* cost;
    double kappa;
    int clip;
    int use_constraints;
    // problem
    const double* actions;  // (B, H, A)
    int N, D, A, E, H, B;
    int B_plan;              // batch the kernel form is planned for (0: B): a slice of a population plans like the population
    int include_time;
    double time0;
    // outputs (nullable)
    double* mu_out;
    double* Sig_out;
    double* cm_out;
    double* cv_out;
    double* J_out;
    // Taylor / separable evaluation of exp(g.w)
    const double* xrange;    // (2, E) per-input-dimension min and max of the memory points
    const int* mono_exp;     // (CM, 4) exponents of the monomials, graded order
    const double* mono_w;    // (CM) 1 / alpha!
    int mono_cum[16];        // mono_cum[k] = number of monomials of degree <= k
    int sep_kmax;            // highest degree the separable path supports (0 = disabled)
    int CM;                  // monomial capacity per (pair, side) in LDS
    int force_path;          // 0 auto, 1 always direct exp, 2 Taylor but never separable (tests)
    int force_sep;           // 1: separable whenever the degree allows, ignoring the cost model (tests)
    int x_in_lds;            // 1: X^T is copied to LDS once per launch (the per-point pass reads it every step)
    int cols2;               // 1: two adjacent columns per lane in the pairwise pass (halves the LDS broadcast traffic)
    // tiling
    int G;        // output pairs per group
    int CH;       // rows per chunk
    int RC;       // row chunks per column
    unsigned magic_N;        // ceil(2^32 / NC):  x / NC  == umulhi(x, magic_N), NC = N (or ceil(N / 2) with cols2)
    unsigned magic_wpp;      // ceil(2^32 / wpp): x / wpp == umulhi(x, magic_wpp)
    unsigned magic_pt;       // ceil(2^32 / N):   x / N   == umulhi(x, magic_pt)  (per-point pass: item -> (problem, point))
    // batch-major path (pair_tile_kernel.h): the per-candidate kernel runs the horizon slice [t_begin, t_end) from the
    // state stored in mu_out / Sig_out and takes the diagonal pairs' sums from tile_part (B, D, ntiles)
    int tiled;               // host side: 1 = launch the TILED instantiation
    int t_begin, t_end;
    int ntiles;
    const double* tile_part;
    const int* slow;         // (B) t + 1: the candidate's step t is this kernel's (off-diagonal pair outside the separable range)
    // gradient launches: when the forward takes the batch-major path, its tile pass forms the moments of the diagonal pairs as
    // well (pair_tile_grad_kernel.h, FUSED) instead of being repeated by a separate moment pass over the stored trajectory
    double* grad_mom;        // (B, H, P, NSP) moment array, or NULL
    int* grad_done;          // (B, H, P) flags
    int grad_NSP, grad_NXP;
    // few-candidate cooperative form (rollout_kernel<..., CL = true>): `cluster` workgroups share one candidate's horizon step
    // and exchange their partial sums as tagged 8-byte granules through `xch` (per candidate: 2 buffers x xch_n values x 2 words)
    int cluster;                 // workgroups per candidate (1: the plain kernel)
    ClusterMap cmap;             // owners of the step's work items among the members (host-planned)
    int cl_slots;                // pairs whose per-point records a member keeps in LDS (ClusterMap::slots_needed, maximum over the members)
    int xch_n;                   // values per exchange
    unsigned xch_tag0;           // tags of this launch: xch_tag0 + step + 1 (unique over the life of the buffer)
    unsigned long long* xch;
    unsigned long long* xch_uc;  // the same layout in uncached device memory (members on several XCDs; the placement prologue)
    int cl_dbg;                  // option cluster_debug: 4 the exchange's general form, 8 members spread over the XCDs (tests)
    // one sequence from the host (gpmpc_objective_grad_host): the actions ride in this block instead of an upload launch; the
    // fused-horizon kernel takes them from here and leaves a copy at `act_store` (= actions) for the gradient's kernels
    int act_inline_n;            // H * A (<= kInlineActs), or 0
    double* act_store;
    double act_inline[kInlineActs];
    // initial state distribution
    double mu0[kMaxD];
    double S0[kMaxD * kMaxD];
};

// the searches' launches: the objective J (B) of `actions` (B, H, A) and nothing else
inline void rollout_objective_only(RolloutArgs& a, const double* actions, double* J) {
    a.actions = actions;
    a.J_out = J;
    a.mu_out = nullptr; a.Sig_out = nullptr; a.cm_out = nullptr; a.cv_out = nullptr;
}

// A device buffer that only ever grows.
struct Buf {
    double* p = nullptr;
    size_t cap = 0;      // doubles
};

struct Handle {
    int device = 0;
    std::string err;
    // shapes of the cached model
    int N = 0, D = 0, E = 0;
    bool ready = false;
    // device buffers owned by the handle
    Buf Xt;       // (E, N)
    Buf beta;     // (D, N)
    Buf iK;       // (D, N, N)
    Buf Tm;       // (D, N, N)
    Buf ils2;     // (D, E)
    Buf var;      // (D)
    Buf logvar;   // (D)
    Buf gram;     // (D, N, N)  K + noise I, then L in its lower triangle (prepare workspace)
    Buf linv;     // (D, N, N)  L^-1 (prepare workspace)
    Buf zvec;     // (D, N)     temp for beta
    Buf cost;     // target | W | W_T | smin | smax
    Buf best;     // argmin result: [best_J, best_idx bits]
    Buf traj;     // (B, H+1, D) + (B, H+1, D, D) when the caller does not want the trajectory
    Buf xrange;   // (2, E) min / max of the inputs
    Buf gradws;   // gradient workspace: pair moments | mean sums | cost variances
    Buf mllws;    // marginal-likelihood workspace: tile partial sums | results
    Buf mllbws;   // gpmpc_mll_batch: per problem of one chunk K -> L | L^-1 | iK (N, N each) | z | beta (N each) (mll_batch.hip)
    Buf trainws;  // gpmpc_train_search: loss (R D) | d loss / d x (R D, E + 2) of the trial points
    Buf cemws;    // cross-entropy search workspace: optimiser vectors | model actions | J | warm start | mean | std
    Buf tilews;   // batch-major path: step records of the candidates | per-tile partial sums | hand-over flags
    Buf tgradws;  // gradient's tile pass: records of a block of (candidate, step) items | per-tile partial moments
    Buf predws;   // gpmpc_predict: per-(query row, column block) partial sums of one chunk of query rows
    Buf predbws;  // gpmpc_predict_backward: per-(output, column block, query row, input) partial sums of one chunk of query rows
    Buf covws;    // gpmpc_predict_cov: P = K*_a(Xa) iK_a of one chunk of rows of Xa
    Buf momws;    // gpmpc_moments: per-point setup results (C_a^-1, Q_ab, log dets) | per-(point, pair, tile) partial sums of one chunk
    Buf mombws;   // gpmpc_moments_backward: setup results | A_ab^-1 | per-(point, output) sums | per-(point, pair, row tile) partials
    Buf linws;    // gpmpc_moments_linear / gpmpc_rollout_linear: per-(output, column block, row) partial sums | model inputs | trajectory of one chunk
    Buf linbws;   // gpmpc_moments_linear_backward / gpmpc_rollout_linear_backward / gpmpc_rollout_linear_feedback_backward: partial sums | coefficients | model inputs | recomputed trajectory, step results and adjoints of one chunk
    Buf fbws;     // gpmpc_rollout_feedback: model inputs (means | covariances) | M | S | V of the step at hand | trajectory | zero gains of one chunk of candidates (rollout_feedback_plan.h)
    Buf fbbws;    // gpmpc_rollout_feedback_backward: model inputs | M | S | recomputed trajectory | every step's V | cost variances | adjoints | cotangents and results of the moment gradient | zero gains of one chunk of candidates (rollout_feedback_backward_plan.h)
    Buf lqrws;    // gpmpc_lqr_gains: model inputs | M of the step at hand | every step's V of one chunk of candidates
    Buf lbfgsws;  // gpmpc_lbfgs_search: J (B) | dJ/d(model actions) (B, H, A) | ones (B), the J_bar of the linearised gradient
    Buf ilqrws;   // gpmpc_ilqr_*: model inputs | M of the step at hand | every step's V of the nominal | trial trajectories of one chunk of candidates (ilqr_plan.h)
    struct SepTable* septab = nullptr;   // monomial bands of the separable evaluation (point_pass_kernel.h), device copy
    Buf sepw;                            // their weights 1 / alpha!
    int septab_D = -1, sep_ks = 0, sep_cmax = 0;
    hipStream_t side_stream = nullptr;   // prepare: the inverse's launches beside the factorisation's
    hipEvent_t ev_params = nullptr, ev_points = nullptr;
    // incremental factorisation: what the cached factors were computed from, and border-update scratch
    Buf Xc, Yc;   // (N, E), (N, D) copies of the memory points of the last prepare
    Buf hyp;      // lengthscales (D*E) | outputscales (D) | noises (D) of the last prepare
    Buf kv, vv;   // (D, N) k(X, x_new), iK k
    Buf sc;       // (D, 2) 1 / Schur complement, v^T y
    int* mismatch = nullptr;     // device flag of the prefix comparison
    int inc_updates = 0;         // border updates since the last full factorisation
    bool have_state = false;     // Xc / Yc / hyp describe the cached factors
    // gpmpc_forget: the record's ping-pong partners, the downdate's coefficients | a copy of hyp for the full path, removed rows
    Buf Xf, Yf;   // (N, E), (N, D): trade places with Xc / Yc
    Buf fgws;
    Buf spws;     // gpmpc_prepare_sparse: Yu | R | partial sums of w | w | jitter | Kuf and V of one chunk of points (prepare_sparse_plan.h)
    Buf selws;    // gpmpc_select_inducing: partial factors L | d | tile traces | tile records | picks | flags (select_inducing_plan.h)
    int* fidx = nullptr;         // device copy of the removed rows when there are more than 8
    size_t fidx_cap = 0;         // ints
    Buf hio;      // gpmpc_objective_grad_host: actions | J | grad | mu | Sig | cost_mu | cost_var of one candidate (device side)
    double* hio_host = nullptr;      // ... and its pinned, device-mapped host mirror (results)
    double* hio_host_dev = nullptr;
    size_t hio_host_cap = 0;
    // ... whose results the reverse sweep itself copies to the host mirror before it raises a sequence number there (the host
    // polls that word instead of synchronising the stream): set for the one launch of gpmpc_objective_grad_host
    unsigned long long* hio_flag = nullptr;          // pinned host word and its device address
    unsigned long long* hio_flag_dev = nullptr;
    unsigned long long hio_seq = 0;
    double* hx_out = nullptr; const double* hx_src = nullptr; int hx_n = 0;      // export request (hx_n = 0: none)
    Buf xch;      // exchange granules of the cooperative few-candidate kernel (zeroed when (re)allocated, tags never repeat)
    unsigned long long* xch_uc = nullptr;    // ... its uncached twin (hipExtMallocWithFlags)
    size_t xch_uc_cap = 0;       // 8-byte words
    unsigned xch_epoch = 1;      // launches that used the exchange buffers, from 1: tag 0 is what a zeroed buffer holds and must never be
                                 // a tag anybody waits for (a fresh handle's first launch accepted the zeros as the members' XCD ids)
    int opt_cluster = 0;         // workgroups per candidate of the few-candidate path: 0 auto, 1 never, n >= 2 fixed
    int opt_cl_dbg = 0;
    int last_cluster = 1;        // what the last fused-horizon launch used
    int last_pair_groups = 1;    // groups of output pairs per horizon step of the last fused-horizon / batch-major launch
    Buf mono_w;   // (CM) 1 / alpha!
    int* mono_exp = nullptr;    // (CM, 4)
    int mono_D = -1;            // state dimension the monomial tables were built for
    int mono_cum[16] = {0};
    int sep_kmax = 0;
    int mono_CM = 0;
    int* info = nullptr;        // (kMaxD) first non-positive pivot + 1, or 0
    std::unordered_set<const void*> lds_configured;   // kernels whose dynamic-LDS limit was raised on this device
    // cost settings
    int cost_D = -1, cost_A = -1;
    double kappa = 1.0;
    int clip = 0;
    int use_constraints = 0;
    // options
    int opt_threads = 0;
    int opt_lds_kb = 0;              // > 0: LDS budget (KiB) of a fused-horizon workgroup (with threads = 512: two workgroups per CU)
    int opt_force_global = 0;
    int opt_rows_per_chunk = 0;
    int opt_force_path = 0;
    int opt_force_sep = 0;
    int opt_grad_stream = 0;         // 1: always the streaming moment pass of the gradient (tests); otherwise only when N needs it
    int opt_grad_share = 0;          // moment pass of the gradient, D <= 3: two 512-thread workgroups per CU -- 0 auto (grad.hip), 1 where the LDS fits twice, 2 never
    int opt_grad_chunk = 0;          // rows per work item of the LDS-resident moment pass: 0 = chosen by the schedule model (grad.hip), else fixed (multiple of 4, <= 64)
    int chunk_key[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // the model's last answer: (N, D, E, columns per lane, waves, LDS KiB, small-batch items, pairs left) -> chunk_rows
    int chunk_rows = 0;
    int opt_grad_tiles = 1;          // diagonal pairs of the gradient's moment pass batch-major (pair_tile_grad_kernel.h): 0 never, 1 auto, 2 always
    int opt_grad_sep = 1;            // off-diagonal pairs of the gradient's moment pass in separable form on the matrix cores:
                                     // 0 never (element-wise), 1 from N = 128 on when B x H fills the chip (measured crossover, grad.hip), 2 always (tests, A/B)
    int opt_cols_per_lane = 0;       // 0 auto, 1 / 2: columns per lane in the pairwise pass of the rollout kernel
    int opt_incremental = 1;         // reuse / border-update the cached factors when the memory only grew
    int opt_refresh_every = 32;      // full refactorisation after this many border updates (bounds drift)
    int opt_outer2 = 2;              // large N: binary outer levels of the trailing update, up to 128 * 2^value columns (0: 128 only)
    int opt_outer_min_n = 640;       // memories from this size on take the outer-panel factorisation path (measured crossover:
                                     // N = 500: 0.61 vs 0.66 ms, 640: 0.92 vs 0.92, 768: 1.22 vs 1.07, 1000: 1.81 vs 1.37; tools/gpu_outer_min_n.py)
    int opt_block128 = 1;            // large N: a whole 128-column outer panel in two launches (LDS-resident block factorisation + tiled solve)
    int opt_inner_left = 1;          // large N: left-looking 32-column panels inside an outer panel; 0: right-looking (A/B)
    int opt_tile128 = 1;             // large N: 128 x 128 tiles (8 wavefronts) for the tiled products; 0: 64 x 64 (A/B)
    int opt_outer_block = 1;         // large N: outer panels of 128 columns + LDS-tiled products; 0: the 32-wide path only (A/B, tests)
    int opt_pair_tiles = 0;          // batch-major pairwise pass of the diagonal pairs: 0 auto (by N, D, B), 1 always (D <= 4), 2 never
    int last_rollout_path = 0;       // what the last rollout launch used: 0 fused-horizon kernel, 1 streaming kernel, 2 batch-major tiles
    int opt_grad_mean = 1;           // moment pass (D <= 4): the mean part by mean_moments_kernel (lanes over points); 0: inside the pass (A/B, tests)
    int last_grad_path = 0;          // moment passes of the last gpmpc_rollout_grad: bit 0 separable off-diagonal pairs, bit 1 tile moments of
                                     // the diagonal pairs, bit 2 streaming element-wise pass, bit 3 the wide (8 < D <= 16) pass
    int opt_prepare_inv_batch = 4;   // 32-wide panel path: row blocks of L^-1 per side-stream launch (1: one launch per row block)
    int opt_prepare_invcols = 1;     // 32-wide panel path, N <= 352 (measured crossover; option 2: up to 544): L^-1 in one launch after the factorisation (0: row blocks beside / after the panels)
    int opt_prepare_fuse = 1;        // 32-wide panel path: trailing update fused with the next diagonal block's factorisation (0: separate launches, A/B)
    int opt_prepare_overlap = 1;     // 32-wide panel path: the inverse's launches on a side stream beside the factorisation's (0: one stream, A/B)
    int opt_gram_shared = 1;         // large N: K of all GPs by one workgroup per tile, squared differences shared (0: per-GP kernel, A/B)
    int opt_fused_prepare = 1;       // N <= 256: the whole factorisation in one launch (prepare_small.hip); 0: panel path (A/B, tests)
    int last_prepare_mode = 0;       // 0 full, 1 border update(s), 2 unchanged (cache hit), 3 downdate (gpmpc_forget), 4 sparse (gpmpc_prepare_sparse), 5 sparse append (gpmpc_sparse_append), 6 sparse forget (gpmpc_sparse_forget)
    int opt_sparse_chunk = 0;        // gpmpc_prepare_sparse: memory points per chunk (0: as many as a 64 MB workspace holds; else a multiple of 64)
    long long opt_select_max_mb = 0; // gpmpc_select_inducing: cap on its workspace in MiB (0: 4096)
    int opt_predict_chunk = 0;       // gpmpc_predict: query rows per chunk (0: as many as a 4 MB workspace holds; tests set a small one)
    int opt_predict_bwd_chunk = 0;   // gpmpc_predict_backward: the same for its chunks
    int opt_predict_cov_chunk = 0;   // gpmpc_predict_cov: rows of Xa per chunk (0: as many as a 256 MB workspace holds; tests set a small one)
    int opt_moments_chunk = 0;       // gpmpc_moments: points per chunk (0: as many as a 32 MB workspace holds; tests set small ones)
    int opt_moments_bwd_chunk = 0;   // gpmpc_moments_backward: the same for its chunks
    int opt_moments_linear_chunk = 0;   // gpmpc_moments_linear / gpmpc_rollout_linear: points / candidates per chunk (0: as many as a 16 MB workspace holds; tests set small ones)
    int opt_moments_linear_bwd_chunk = 0;   // gpmpc_moments_linear_backward / gpmpc_rollout_linear_backward: the same for their chunks
    int opt_rollout_feedback_bwd_chunk = 0; // gpmpc_rollout_feedback_backward: the same for its chunks
    int opt_rollout_feedback_chunk = 0; // gpmpc_rollout_feedback: candidates per chunk (0: as many as a 16 MB workspace holds; tests set small ones)
    int opt_lqr_gains_chunk = 0;     // gpmpc_lqr_gains: candidates per chunk (0: as many as a 16 MB workspace holds; tests set small ones)
    int opt_mll_batch_chunk = 0;     // gpmpc_mll_batch / gpmpc_train_search: problems per launch and in the workspace (0: one per CU; results do not depend on it)
    int opt_ilqr_chunk = 0;          // gpmpc_ilqr_*: candidates per chunk (0: as many as a 16 MB workspace holds; tests set small ones)
    int lds_limit = 160 * 1024;
    int num_cu = 256;
    Buf sprec;    // gpmpc_sparse_append / gpmpc_sparse_forget: the record of the last gpmpc_prepare_sparse (Yb | w | noises; sparse_update_plan.h)
    bool sp_have = false;        // ... is there: Yu at spws + sp_yu, Yb / w / noises in sprec, Z and the hyper-parameters packed in the handle
    size_t sp_yu = 0;
    Buf spupd;    // ... and their scratch, allocated with the record: the forget's failure words | vectors of the point at hand
};

// Raise a kernel's dynamic-LDS limit to the device maximum once per handle (= per device).
inline int allow_full_lds(Handle* h, const void* kernel);

#define GPMPC_HIP_CHECK(h, expr)                                                         \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) {                                                          \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                \
            return GPMPC_ERR_HIP;                                                        \
        }                                                                                \
    } while (0)

inline int allow_full_lds(Handle* h, const void* kernel) {
    if (h->lds_configured.count(kernel)) return GPMPC_OK;
    GPMPC_HIP_CHECK(h, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, h->lds_limit));
    h->lds_configured.insert(kernel);
    return GPMPC_OK;
}

// exact division by multiply-high: for d >= 2, umulhi(x, ceil(2^32 / d)) == x / d whenever x * d < 2^32 (0 encodes d == 1: no division)
inline unsigned magic_div(unsigned d) { return d <= 1 ? 0u : (unsigned)((0x100000000ULL + d - 1) / d); }

// The upper triangles of the D tables T_a no longer stay in an XCD's 4 MiB L2 from this size on: the batch-major passes of the
// diagonal pairs (pair_tile_kernel.h, pair_tile_grad_kernel.h) amortise a tile over many candidates instead.
constexpr double kTileTableBytes = 6.0e6;
inline bool tables_outgrow_l2(int N, int D) { return 4.0 * D * (double)N * N >= kTileTableBytes; }

// ---------------------------------------------------------------------------------------
// Kernel form of a rollout launch (rollout.hip: plan_rollout).  Planned from the shape, the PLANNED batch Bp, the handle's options
// and device limits alone -- never from the launched batch: a slice of a population takes the population's form (same chunk
// lengths, same summation order) while the grid still covers the candidates launched.
struct RolloutRequest {        // what a gradient launch asks of its forward
    bool fused_tiles;          // the batch-major tile pass also forms the diagonal pairs' moments (RolloutArgs::grad_mom)
    bool costs_to_caller;      // the stage costs / objective are left to the caller (the few-candidate moment launch)
};
struct RolloutPlan {
    int DP;                    // padded state dimension of the instantiation
    int nt;                    // threads per workgroup
    int path;                  // 0 fused-horizon kernel, 1 streaming kernel, 2 batch-major tiles (Handle::last_rollout_path)
    int cols2, G, CH, RC, x_in_lds;          // the RolloutArgs fields of the same names
    size_t lds_bytes;
    int cluster, cl_slots, xch_n;            // cooperative form (cluster 1: the plain kernel)
    ClusterMap cmap;
    unsigned magic_N, magic_wpp, magic_pt;
    int CM, sep_kmax;
    bool fused_tiles;          // the request, where the form honours it (batch-major only)
    bool costs_to_caller;
    const char* err;           // why the shape is over a limit (GPMPC_ERR_LIMIT)
};

// Kernel forms of a gradient launch with D <= 8 (grad.hip: plan_rollout_grad), the forward's included.
struct MomTiling {             // moment pass: pairs per group, rows per chunk, row chunks, work-item slots per pair, pair groups, LDS
    int G, CH, RC, wpp, gz;
    size_t lds;
};
struct GradPlan {
    int DP, NXP, RS, NSP;
    int sweep_nt, pre_steps;   // reverse sweep: threads, steps whose state-independent algebra runs up front
    size_t sweep_lds;
    bool stream;               // streaming element-wise pass (per-point arrays beyond the LDS), else LDS-resident
    size_t gs_lds;
    MomTiling first;           // what the launches before the element-wise pass see (64-row chunks, all pairs)
    MomTiling pass;            // the element-wise pass: re-planned for the pairs left and the schedule model's chunk (LDS-resident)
    bool share_cu;             // two 512-thread workgroups per CU
    bool tiles, fused;         // diagonal pairs batch-major; formed by the forward's tile pass
    bool sep;                  // off-diagonal pairs in separable form on the matrix cores, with:
    int sep_kmax, sep_NA, sep_NE, sep_PS, sep_wave_words;
    size_t sep_lds;
    int pairs_left;            // pairs the element-wise pass works on
    bool few, merged;          // few candidates; element-wise + mean moments + stage costs in one launch
    int path;                  // Handle::last_grad_path
    RolloutPlan fwd;
};

// ---------------------------------------------------------------------------------------
// Launch forms of a full factorisation (prepare.hip: plan_prepare), from N, the handle's options and device limits alone.
// Crossover of the single launch (prepare_small.hip) with the panel chain, measured (round 3, tools/gpu_prepare_bench.py; the LDS
// arrays were sized by N for the test): N = 200: 0.217 vs 0.240 ms, 256: 0.344 vs 0.299, 300: 0.387 vs 0.337, 400: 0.84 vs 0.49,
// 500: 1.15 vs 0.60 -- one CU's matrix cores do the N^3 / 3 of the panel updates, so the single launch loses once the chain's
// launches fill more than a CU.
constexpr int kSmallPathMaxN = 240;
// One workgroup per GP is the right shape for the factorisation (a chain of 200 dependent pivots) but not for the N^3 products
// after it: on one CU they are matrix-core-bound at ~50 k cycles each for N = 200.  From this size on only the factorisation stays
// in the single launch (option "fused_prepare" = 2 forces everything into it, 3 never).
constexpr int kSmallCholeskyMinN = 96;
// 32-wide panel chain: L^-1 in one launch after the factorisation up to this size (measured: 0.286 -> 0.254 ms at N = 257,
// 0.315 -> 0.297 at 300, 0.404 vs 0.420 at 400, slower from 500 on) -- or, with option "prepare_invcols" = 2, up to 544 points
// (17 row blocks of the block column in LDS)
constexpr int kInvColsMaxN = 352;
constexpr int kInvColsWideMaxN = 544;
// Y^T Y by the LDS-tiled kernel (64 x 64 tiles) from this size on, the 32 x 32 one below it
constexpr int kSyrkTiledMinN = 512;
// All GPs per Gram tile, squared differences shared (gram_lower_kernel), once its one-workgroup-per-tile grid fills the chip
// (measured, profiles/r06_gram_ab.txt: N = 4096, D = 16: 985 -> 264 us = 4.1 TB/s of stores; N = 1000, D = 4 (136 tiles):
// 15.0 -> 17.4 us, hence a rule on the tile count): from this many tiles per CU on
constexpr int kGramSharedTilesPerCu = 2;

enum class PreparePath {
    small_whole,               // everything in one launch (prepare_small.hip)
    small_cholesky,            // the factorisation and L^-1 by prepare_small.hip, then the tail of prepare.hip
    panel32,                   // the 32-wide panel chain
    outer,                     // outer panels of 128 columns (N >= option "outer_min_n")
};
enum class GramForm { full, lower, shared_lower };                 // per-GP full matrix, per-GP lower triangle, all GPs per tile
enum class Inv32Form { rows, cols, side };      // L^-1 of the 32-wide chain: a row block inline per step, one column-block
                                                // launch after the factorisation, or row batches on the side stream
enum class OuterInvForm { rows128, doubling, doubling_ykk };       // 128-row blocks; recursive doubling (after a separate Y_KK step)
enum class SyrkInvForm { w32, tiled, t128 };                       // Y^T Y: 32 x 32, 64 x 64 or 128 x 128 tiles
struct PreparePlan {
    PreparePath path;
    GramForm gram;
    // 32-wide chain (panel32, and the inner steps of outer panels without block128)
    bool round2;               // round-2 panel kernels (option "outer_block" = 0: the round-1 ones)
    bool fuse_next;            // trailing update fused with the next diagonal block's factorisation (panel32)
    Inv32Form inv32;           // (panel32)
    int inv_batch;             // row blocks per side-stream launch
    // outer panels
    bool tile128;              // 128 x 128 tiles for the tiled products (also decides the beta form, see beta_partial)
    bool block128;             // a whole outer panel in two launches
    bool inner_left;           // left-looking 32-column steps inside an outer panel (else right-looking)
    int outer2;                // binary outer levels of the trailing update, up to 128 * 2^outer2 columns
    OuterInvForm outer_inv;
    // tail
    bool beta_partial;         // beta by column-chunk partials + a reduction
    SyrkInvForm syrk;
};

// Rows gpmpc_forget removes, ascending (kernel argument): up to 8 ride in the block itself, more come from device memory
struct ForgetRows {
    int k;
    int few[8];
    const int* many;
};

// rollout.hip
int ensure_rollout_tables(Handle* h, int N, int D);      // what the plan reads: monomial tables, the batch-major path's bands
int plan_rollout(const Handle& h, int N, int D, int A, int E, int H, int Bp, const RolloutRequest& req, RolloutPlan& p);
int launch_rollout(Handle* h, RolloutArgs& a, const RolloutPlan& p, hipStream_t s);
int launch_rollout(Handle* h, RolloutArgs& a, hipStream_t s);
int launch_argmin(Handle* h, const double* J, int B, long long first, hipStream_t s);
int launch_traj_cost(Handle* h, const RolloutArgs& a, double* cm, double* cv, double* J, hipStream_t s);     // stage costs + objective of the stored trajectory
// pair_tile.hip: the batch-major pass of horizon step t (a.mu_out / a.Sig_out hold the state), a.tile_part / a.ntiles set on return
int ensure_sep_table(Handle* h, int D);
bool tile_path_fits(const Handle& h, int N, int D, int E);          // (reads the table of ensure_sep_table)
int tile_workspace(Handle* h, RolloutArgs& a);
int launch_tile_state_init(Handle* h, const RolloutArgs& a, hipStream_t s);
int launch_pair_tiles(Handle* h, const RolloutArgs& a, int t, hipStream_t s);
bool tile_moments_supported(const Handle& h, int D, int E, int NSP);
int launch_tile_moments(Handle* h, const RolloutArgs& a, double* mom, int* done, int NSP, int NXP, hipStream_t s);
// grad.hip
// Cotangents of gpmpc_rollout_backward (each NULL = 0) and its initial-state outputs (each NULL = not written); `cost`: a cost or
// objective seed is given (the forward then computes the stage costs, the sweep reads the loaded cost settings)
struct RolloutSeeds {
    const double* mu; const double* Sig; const double* cm; const double* cv; const double* J;
    double* mu0_bar; double* S0_bar;
    bool cost;
};
// (updates the schedule model's memo, Handle::chunk_key / chunk_rows)
int plan_rollout_grad(Handle* h, int N, int D, int A, int E, int H, int B, int Bp, bool seeded, GradPlan& p);
// seeds == NULL: gpmpc_rollout_grad's LCB gradient; otherwise the same launch sequence with the seeded reverse sweep
int launch_rollout_grad(Handle* h, RolloutArgs& a, double* grad_out, hipStream_t s, const RolloutSeeds* seeds = nullptr);
int launch_rollout_grad_wide(Handle* h, RolloutArgs& a, double* grad_out, hipStream_t s,          // grad_wide.hip: 8 < D <= 16
                             const RolloutSeeds* seeds = nullptr);
int check_rollout_grad_wide(Handle* h, int N, int D, int A, int E, int H, int B,           // ... its limits, before anything is
                            size_t* mom_lds = nullptr, size_t* sweep_lds = nullptr);     // launched, and its kernels' LDS bytes
int launch_argmin_to(Handle* h, const double* J, int B, long long first, const double* actions, int HA, double* out_dev,
                     double* out_host, hipStream_t s);     // out_host: device address of pinned host memory, or NULL
// prepare.hip (allow_reuse = false: a full factorisation even where the cached factors could be reused or border-updated)
void plan_prepare(const Handle& h, int N, PreparePlan& p);
int run_prepare(Handle* h, const double* X, const double* Y, const double* ls, const double* os,
                const double* noise, int N, int D, int E, hipStream_t s, bool allow_reuse = true);
int run_set_factors(Handle* h, const double* X, const double* iK, const double* beta,
                    const double* ls, const double* os, int N, int D, int E, hipStream_t s);
int ensure_model_buffers(Handle* h, int N, int D, int E, bool need_factor_ws);
int run_mll(Handle* h, const double* X, const double* Y, const double* ls, const double* os, const double* noise,
            int N, int D, int E, double* out_host, hipStream_t s);
int grow(Handle* h, Buf& b, size_t need);
// ... gpmpc_forget: rows idx_host (validated: strictly ascending, in range, 1 <= k < N) leave the cached model
int run_forget(Handle* h, const int* idx_host, int k, hipStream_t s);
// ... gpmpc_prepare_sparse: the DTC model of (X, Y) on the inducing inputs Z, left in the state run_set_factors(Z, iK_eff, beta_eff)
// would leave (validated by the entry point)
int run_prepare_sparse(Handle* h, const double* X, const double* Y, int N, const double* Z, int M, const double* ls, const double* os,
                       const double* noise, double jitter_rel, int D, int E, hipStream_t s);
// prepare_sparse.hip: the launches of its stream over the memory points and of its tail (h->Xt / ils2 / var hold the packed Z)
int launch_sparse_jitter(Handle* h, const double* os, double jitter_rel, int D, double* jit, hipStream_t s);
int launch_sparse_panel(Handle* h, const double* X, int N, int M, int D, int E, int n0, int cn, int Cs, double* kuf, hipStream_t s);
int launch_sparse_accumulate(Handle* h, const double* v, const double* Y, int M, int D, int n0, int cn, int Cs, double* G,
                             double* wpart, hipStream_t s);
int launch_sparse_bmat(Handle* h, const double* G, const double* wpart, const double* noise, int M, int D, double* Bm, double* w,
                       hipStream_t s);
int launch_sparse_beta(Handle* h, const double* Yu, const double* Yb, const double* w, const double* noise, int M, int D, double* t1,
                       double* t2, double* beta, hipStream_t s);
int launch_sparse_atb_sym(Handle* h, const double* A, const double* B, int M, int D, double* C, bool ident_minus, hipStream_t s);
// ... gpmpc_sparse_append / gpmpc_sparse_forget: k memory points (X (k, E), Y (k, D)) join the sparse model of the record, or --
// `forget`, by their VALUES -- leave it (validated by the entry point: a record, k >= 1).  The append is asynchronous on s; the forget
// synchronises s and reports a lost pivot (GPMPC_ERR_NOT_PD: no model, no record)
int run_sparse_update(Handle* h, const double* X, const double* Y, int k, bool forget, hipStream_t s);
// sparse_update.hip: the LDS check before a call's first launch, and the two launches of point number `point` of the call
struct SparseUpdatePlan;
int check_sparse_update(Handle* h, const SparseUpdatePlan& p, bool forget);
int launch_sparse_update_point(Handle* h, const SparseUpdatePlan& p, const double* Yu, double* rec, double* ws, const double* x,
                               const double* y, int point, bool forget, int M, int D, int E, hipStream_t s);
// select_inducing.hip: greedy variance selection of M of the N points X as inducing inputs (validated by the entry point; Z_out and
// trace_out may be NULL); asynchronous on s, the cached model is neither read nor written
int run_select_inducing(Handle* h, const double* X, int N, int M, const double* ls, const double* os, double jitter_rel, int D, int E,
                        int* idx_out, double* Z_out, double* trace_out, hipStream_t s);
// forget.hip: one removal (iK, linv, beta) -> (gram, Tm, zvec); the record (and, with `tables`, X^T and the data range) without the rows
int launch_forget_step(Handle* h, int n, int j, int D, int ldw, hipStream_t s);
int launch_forget_pack(Handle* h, const ForgetRows& rm, int n1, int D, int E, double* Xn, double* Yn, bool tables, hipStream_t s);
// predict.hip: posterior mean / variance at M query inputs from the cached model (mean_out / var_out may be NULL)
int run_predict(Handle* h, const double* Xq, int M, const double* noises_host, double* mean_out, double* var_out, hipStream_t s);
// ... and its gradient wrt Xq for upstream mean_bar / var_bar (each may be NULL = 0), written to Xq_bar (M, E)
int run_predict_backward(Handle* h, const double* Xq, int M, const double* mean_bar, const double* var_bar, double* Xq_bar,
                         hipStream_t s);
// predict_cov.hip: posterior covariance between the rows of Xa and of Xb (cross form), or of Xa with itself (Xb NULL: joint form,
// exactly symmetric, noises_host on the diagonal), written to out (D, Ma, Mb)
int run_predict_cov(Handle* h, const double* Xa, int Ma, const double* Xb, int Mb, const double* noises_host, double* out,
                    hipStream_t s);
// moments.hip: moment-matched prediction at P Gaussian inputs from the cached model (Sig NULL = 0; S_out / V_out may be NULL)
int run_moments(Handle* h, const double* mu, const double* Sig, int P, double* M_out, double* S_out, double* V_out,
                hipStream_t s);
// moments_linear.hip: first-order (linearised) propagation at P Gaussian inputs from the cached model (Sig NULL = 0; each output may
// be NULL; without S_out no matrix product runs), and the horizon rollout built on it (`a` as fill_args leaves it plus the outputs)
int run_moments_linear(Handle* h, const double* mu, const double* Sig, int P, double* M_out, double* S_out, double* V_out,
                       hipStream_t s);
// (gains != NULL: in closed loop under the linear feedback u = ubar_t + K_t (x - mu_t), gains (B, H, A, D) when per_candidate, else
// (H, A, D) shared by the candidates)
int run_rollout_linear(Handle* h, const RolloutArgs& a, hipStream_t s, const double* gains = nullptr, bool per_candidate = false);
// ... the closed-loop stage costs and objective (traj_cost_feedback_kernel) of `rows` stored trajectories mu (rows, H + 1, D),
// Sig (rows, H + 1, D, D): gains of the first of them, gain_stride doubles between two candidates' gains (0: shared); cost
// settings of `a`; each output may be NULL
int launch_traj_cost_feedback(Handle* h, const RolloutArgs& a, int rows, const double* mu, const double* Sig, const double* actions,
                              const double* gains, long long gain_stride, double* cm, double* cv, double* J, hipStream_t s);
// rollout_feedback.hip: the moment-matched horizon rollout in closed loop under u = ubar_t + K_t (x - mu_t) (`a` as fill_args leaves
// it plus the outputs; gains (B, H, A, D) when per_candidate, else (H, A, D) shared, or NULL = all zero): run_moments per step
int run_rollout_feedback(Handle* h, const RolloutArgs& a, hipStream_t s, const double* gains, bool per_candidate);
// rollout_feedback_backward.hip: gradients of run_rollout_feedback wrt the actions, the gains (gains_bar (B, H, A, D) per candidate,
// or NULL) and the initial state for the cotangents `sd` (forward recomputed inside; gains as there, NULL = all zero)
int run_rollout_feedback_backward(Handle* h, const RolloutArgs& a, const RolloutSeeds& sd, const double* gains, bool per_candidate,
                                  double* actions_bar, double* gains_bar, hipStream_t s);
// lqr_gains.hip: the LQR gains (B, H, A, D) of the linearisation along each candidate's nominal trajectory on the loaded quadratic
// cost (validated by the entry point: model, cost for this (D, A), 1 <= A <= kLqrMaxA, reg >= 0); P_out (B, H + 1, D, D) and
// flags_out (B) may be NULL
int run_lqr_gains(Handle* h, const double* actions, const double* mu0_host, int B, int H, int A, int include_time, double time0,
                  double reg, double* gains_out, double* P_out, int* flags_out, hipStream_t s);
// moments_backward.hip: gradients of run_moments wrt mu and Sig (symmetric part) for upstream Mb / Sb / Vb (each may be NULL)
int run_moments_backward(Handle* h, const double* mu, const double* Sig, int P, const double* Mb, const double* Sb,
                         const double* Vb, double* mb_out, double* vb_out, hipStream_t s);
// moments_linear_backward.hip: gradients of run_moments_linear wrt mu and Sig (symmetric part) for upstream Mb / Sb / Vb (each may
// be NULL), and of run_rollout_linear wrt the actions and the initial state for the cotangents `sd` (forward recomputed inside)
int run_moments_linear_backward(Handle* h, const double* mu, const double* Sig, int P, const double* Mb, const double* Sb,
                                const double* Vb, double* mb_out, double* vb_out, hipStream_t s);
int run_rollout_linear_backward(Handle* h, const RolloutArgs& a, const RolloutSeeds& sd, double* actions_bar, hipStream_t s);
// ... and of the closed-loop run_rollout_linear (gains as there, not NULL) wrt the actions, the gains (gains_bar (B, H, A, D) per
// candidate, or NULL) and the initial state
int run_rollout_linear_feedback_backward(Handle* h, const RolloutArgs& a, const RolloutSeeds& sd, const double* gains,
                                         bool per_candidate, double* actions_bar, double* gains_bar, hipStream_t s);
// search.hip: cross-entropy search whose loop stays on the device (actions / J_out of `a` are set inside)
int run_cem_search(Handle* h, RolloutArgs& a, int iterations, int n_elite, unsigned long long seed, const double* first_host,
                   int mapper, const double* max_change_host, const double* a_prev_host, const double* noise_dev,
                   double* best_out_dev, hipStream_t s);
// ... and its per-iteration halves for candidates sharded over GPUs (a.B = the slice length)
int run_cem_local(Handle* h, RolloutArgs& a, int B_total, int b0, int it, int n_elite, unsigned long long seed,
                  const double* first_host, int mapper, const double* max_change_host, const double* a_prev_host,
                  const double* noise_dev, const double* state_dev, double* elites_out_dev, hipStream_t s);
int run_cem_merge(Handle* h, const double* elites_dev, int lists, int n_elite, int n, int it, double* state_dev, hipStream_t s);
// lbfgs_search.hip: box-constrained L-BFGS over B restarts in lockstep whose loop stays on the device (lbfgs_state.h: the state
// buffer and the argument checks).  `a` as fill_args leaves it (actions / J_out are set inside); propagation 0 moment matching,
// 1 linearised; best_out_dev [J | restart | x (n)] or NULL
struct ActionMapper;
int run_lbfgs_init(Handle* h, const double* x0_dev, int B, int H, int A, int history, const ActionMapper& mp, double* state_dev,
                   hipStream_t s);
int run_lbfgs_step(Handle* h, const double* J_dev, const double* grad_model_dev, int B, int H, int A, int iteration, int history,
                   double c1, double pgtol, const ActionMapper& mp, double* state_dev, hipStream_t s);
int run_lbfgs_search(Handle* h, RolloutArgs& a, int propagation, int first_iteration, int iterations, int history, double c1,
                     double pgtol, const ActionMapper& mp, const double* x0_dev, double* state_dev, double* best_out_dev,
                     hipStream_t s);
// ilqr.hip: clamped iLQR on the mean dynamics of the linearised propagation, B candidates in lockstep (ilqr_state.h: the state buffer
// and the argument checks; validated by the entry points).  backward: gains (B, H, A, D), feed-forward (B, H, A), nominal trajectory
// (B, H + 1, D) and info (B, 5) = [cost | dV | step | flags | 0] at `actions` with the per-candidate reg_dev (B); forward: the trial
// actions (B, L, H, A), costs (B, L) and, where wanted, trajectories (B, L, H + 1, D) of the L step sizes alphas_host
int run_ilqr_backward(Handle* h, const double* actions, const double* mu0_host, int B, int H, int A, int include_time, double time0,
                      const double* reg_dev, double* gains_out, double* ff_out, double* mu_out, double* info_out, hipStream_t s);
int run_ilqr_forward(Handle* h, const double* actions, const double* gains, const double* ff, const double* mu_nom,
                     const double* mu0_host, int B, int H, int A, int include_time, double time0, const double* alphas_host, int L,
                     double* trial_actions_out, double* trial_cost_out, double* trial_mu_out, hipStream_t s);
int run_ilqr_init(Handle* h, const double* x0_dev, int B, int H, int A, int L, double reg0, double* state_dev, hipStream_t s);
int run_ilqr_step(Handle* h, const double* mu0_host, int B, int H, int A, int include_time, double time0, int L, double reg0,
                  double reg_factor, double reg_max, double tol, double* state_dev, hipStream_t s);
// ... `a` as fill_args leaves it (actions / J_out are set inside); best_out_dev [J | restart | actions (H A)] or NULL
int run_ilqr_search(Handle* h, RolloutArgs& a, int iterations, int L, double reg0, double reg_factor, double reg_max, double tol,
                    const double* x0_dev, double* state_dev, double* best_out_dev, hipStream_t s);
// mll_batch.hip: the training loss and gradient of R hyper-parameter sets per GP, left on the device (validated by the entry
// points; lo / hi both NULL: params is theta itself), and the multi-restart search built on it and on run_lbfgs_step; both are
// asynchronous on s and neither read nor write the cached model
int run_mll_batch(Handle* h, const double* X, const double* Y, int N, int D, int E, const double* params, int R, const double* lo,
                  const double* hi, int log_scale, double* loss_out, double* grad_out, double* theta_out, int* info_out,
                  hipStream_t s);
int run_train_search(Handle* h, const double* X, const double* Y, int N, int D, int E, int R, const double* lo, const double* hi,
                     int log_scale, int first_iteration, int iterations, int history, double c1, double pgtol, const double* x0_dev,
                     double* state_dev, double* best_out_dev, hipStream_t s);
// prepare_small.hip: the single-launch paths of a plan (PreparePath::small_whole / small_cholesky)
int launch_prepare_small(Handle* h, const PreparePlan& pp, const double* X, const double* Y, const double* ls, const double* os,
                         const double* noise, int N, int D, int E, hipStream_t s);

}  // namespace gpmpc_hip
