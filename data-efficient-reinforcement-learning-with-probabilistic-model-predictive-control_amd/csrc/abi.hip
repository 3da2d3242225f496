// abi.hip -- extern "C" entry points of libgpmpc_hip.so (declared in include/gpmpc.h).
#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <dlfcn.h>

#include "gpmpc_internal.h"
#include "lqr_gains_plan.h"
#include "lbfgs_state.h"
#include "ilqr_state.h"

// ROCTx ranges around the entry points (tracing row): visible in `rocprofv3 --marker-trace` timelines
// as gpmpc_prepare / gpmpc_rollout / gpmpc_rollout_grad / gpmpc_argmin.  The marker library is looked up at first use
// (rocprofiler-sdk's roctx, then the older roctracer one); without it the ranges cost one predictable branch.
namespace {
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        for (const char* lib : {"librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
            void* hnd = dlopen(lib, RTLD_LAZY | RTLD_LOCAL);
            if (!hnd) continue;
            push = reinterpret_cast<int (*)(const char*)>(dlsym(hnd, "roctxRangePushA"));
            pop = reinterpret_cast<int (*)()>(dlsym(hnd, "roctxRangePop"));
            if (push && pop) return;
            push = nullptr; pop = nullptr;
        }
    }
};
struct Range {
    static const Roctx& api() { static Roctx r; return r; }
    explicit Range(const char* name) { if (api().push) api().push(name); }
    ~Range() { if (api().pop) api().pop(); }
    Range(const Range&) = delete;
    Range& operator=(const Range&) = delete;
};
}  // namespace

using namespace gpmpc_hip;

struct gpmpc {
    Handle h;
};

#define H_(x) (&(x)->h)

static int bad(gpmpc_t* g, const char* msg) {
    if (g) g->h.err = msg;
    return GPMPC_ERR_ARG;
}

static void free_buf(Buf& b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

// gpmpc_set_option: one row per name.  A row with a message rejects, with that message, a value outside [lo, hi] or off the
// multiple `mult` (a power of two); a row without one takes any value through the (int) cast, raised to `lo`.
struct Option {
    const char* name;
    int Handle::*field;
    long long lo = INT_MIN, hi = INT_MAX;
    int mult = 1;
    const char* msg = nullptr;
    long long Handle::*wide = nullptr;   // the one option wider than an int
    bool cast_first = false;             // the value goes through the (int) cast before the range check
};

constexpr long long kChunkMax = 1 << 24;
const Option kOptions[] = {
    {"threads", &Handle::opt_threads},
    {"lds_limit_kb", &Handle::opt_lds_kb},
    {"force_global_scratch", &Handle::opt_force_global},
    {"rows_per_chunk", &Handle::opt_rows_per_chunk},
    {"force_path", &Handle::opt_force_path},
    {"force_separable", &Handle::opt_force_sep},
    {"cols_per_lane", &Handle::opt_cols_per_lane},
    {"grad_share_cu", &Handle::opt_grad_share},
    {"grad_chunk_rows", &Handle::opt_grad_chunk, 0, 64, 4, "grad_chunk_rows: 0 (auto) or a multiple of 4 up to 64", nullptr, true},
    {"predict_chunk_rows", &Handle::opt_predict_chunk, 0, kChunkMax, 64, "predict_chunk_rows: 0 (auto) or a multiple of 64"},
    {"predict_backward_chunk_rows", &Handle::opt_predict_bwd_chunk, 0, kChunkMax, 64,
     "predict_backward_chunk_rows: 0 (auto) or a multiple of 64"},
    {"predict_cov_chunk_rows", &Handle::opt_predict_cov_chunk, 0, kChunkMax, 64, "predict_cov_chunk_rows: 0 (auto) or a multiple of 64"},
    {"moments_chunk_points", &Handle::opt_moments_chunk, 0, kChunkMax, 1, "moments_chunk_points: 0 (auto) or a number of points"},
    {"moments_backward_chunk_points", &Handle::opt_moments_bwd_chunk, 0, kChunkMax, 1,
     "moments_backward_chunk_points: 0 (auto) or a number of points"},
    {"moments_linear_chunk_points", &Handle::opt_moments_linear_chunk, 0, kChunkMax, 1,
     "moments_linear_chunk_points: 0 (auto) or a number of points"},
    {"moments_linear_backward_chunk_points", &Handle::opt_moments_linear_bwd_chunk, 0, kChunkMax, 1,
     "moments_linear_backward_chunk_points: 0 (auto) or a number of points"},
    {"rollout_feedback_chunk_points", &Handle::opt_rollout_feedback_chunk, 0, kChunkMax, 1,
     "rollout_feedback_chunk_points: 0 (auto) or a number of candidates"},
    {"rollout_feedback_backward_chunk_points", &Handle::opt_rollout_feedback_bwd_chunk, 0, kChunkMax, 1,
     "rollout_feedback_backward_chunk_points: 0 (auto) or a number of candidates"},
    {"lqr_gains_chunk_points", &Handle::opt_lqr_gains_chunk, 0, kChunkMax, 1, "lqr_gains_chunk_points: 0 (auto) or a number of candidates"},
    {"ilqr_chunk_points", &Handle::opt_ilqr_chunk, 0, kChunkMax, 1, "ilqr_chunk_points: 0 (auto) or a number of candidates"},
    {"mll_batch_chunk", &Handle::opt_mll_batch_chunk, 1, kChunkMax, 1, "mll_batch_chunk: a number of problems >= 1"},
    {"sparse_chunk_points", &Handle::opt_sparse_chunk, 0, kChunkMax, 64, "sparse_chunk_points: 0 (auto) or a multiple of 64"},
    {"select_inducing_max_mb", nullptr, 1, LLONG_MAX, 1, "select_inducing_max_mb: a number of MiB >= 1", &Handle::opt_select_max_mb},
    {"incremental", &Handle::opt_incremental},
    {"grad_stream", &Handle::opt_grad_stream},
    {"grad_separable", &Handle::opt_grad_sep},
    {"grad_tiles", &Handle::opt_grad_tiles},
    {"grad_mean", &Handle::opt_grad_mean},
    {"prepare_overlap", &Handle::opt_prepare_overlap},
    {"prepare_fuse", &Handle::opt_prepare_fuse},
    {"prepare_invcols", &Handle::opt_prepare_invcols},
    {"prepare_inv_batch", &Handle::opt_prepare_inv_batch},
    {"fused_prepare", &Handle::opt_fused_prepare},
    {"gram_shared", &Handle::opt_gram_shared},
    {"outer_block", &Handle::opt_outer_block},
    {"tile128", &Handle::opt_tile128},
    {"block128", &Handle::opt_block128},
    {"outer_min_n", &Handle::opt_outer_min_n, 256},
    {"inner_left", &Handle::opt_inner_left},
    {"outer2", &Handle::opt_outer2},
    {"refresh_every", &Handle::opt_refresh_every},
    {"pair_tiles", &Handle::opt_pair_tiles},
    {"cluster_debug", &Handle::opt_cl_dbg},
    {"cluster", &Handle::opt_cluster, 0, 32, 1, "cluster: 0 (auto), 1 (never) or 2..32 workgroups per candidate"},
};

// The checks the seven query-point entries (gpmpc_predict*, gpmpc_moments*) share, in their order: a handle, a cached model, for
// the moments entries the compiled limits, the model's D and E, a count >= 0.  `name` heads the messages; `count_name` is the
// count's letter in them, NULL for gpmpc_predict_cov, which checks its own two counts.
static int query_checks(gpmpc_t* g, const char* name, const char* count_name, int count, int D, int E, bool check_limits) {
    if (!g) return GPMPC_ERR_ARG;
    Handle* h = H_(g);
    auto fail = [&](const char* tail) { return bad(g, (std::string(name) + tail).c_str()); };
    if (!h->ready) return fail(" before prepare / set_factors / mll");
    if (check_limits && (D > GPMPC_MAX_D || E > GPMPC_MAX_E)) {
        fail(": D or E beyond the compiled limits");
        return GPMPC_ERR_LIMIT;
    }
    if (D != h->D || E != h->E) return fail(": D / E differ from the cached model");
    if (count_name && count < 0) return fail((std::string(": ") + count_name + " < 0").c_str());
    return GPMPC_OK;
}

// ... and what all of them but gpmpc_predict_cov do next: the entry's own pointers (`have_ptrs`) where there is work to do,
// nothing for an empty call, then the device and the entry's run_* function.
template <class Run>
static int query_entry(gpmpc_t* g, const char* name, const char* count_name, int count, int D, int E, bool check_limits,
                       bool have_ptrs, Run run) {
    int rc = query_checks(g, name, count_name, count, D, E, check_limits);
    if (rc) return rc;
    if (count > 0 && !have_ptrs) return bad(g, "null argument");
    if (count == 0) return GPMPC_OK;
    GPMPC_HIP_CHECK(H_(g), hipSetDevice(g->h.device));
    return run(H_(g));
}

extern "C" {

int gpmpc_abi_version(void) { return 29; }

int gpmpc_create(gpmpc_t** out, int device_id) {
    if (!out) return GPMPC_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return GPMPC_ERR_HIP;
    if (hipSetDevice(device_id) != hipSuccess) return GPMPC_ERR_HIP;
    gpmpc_t* g = new (std::nothrow) gpmpc();
    if (!g) return GPMPC_ERR_HIP;
    g->h.device = device_id;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) {
        g->h.num_cu = prop.multiProcessorCount;
        if (prop.maxSharedMemoryPerMultiProcessor >= 64 * 1024)
            g->h.lds_limit = (int)prop.maxSharedMemoryPerMultiProcessor;
        if (g->h.lds_limit > 160 * 1024) g->h.lds_limit = 160 * 1024;
    }
    *out = g;
    return GPMPC_OK;
}

int gpmpc_destroy(gpmpc_t* g) {
    if (!g) return GPMPC_ERR_ARG;
    Handle* h = H_(g);
    (void)hipSetDevice(h->device);
    Buf* all[] = {&h->Xt, &h->beta, &h->iK, &h->Tm, &h->ils2, &h->var, &h->logvar, &h->gram,
                  &h->linv, &h->zvec, &h->cost, &h->best, &h->xrange, &h->mono_w, &h->traj, &h->Xc, &h->Yc,
                  &h->hyp, &h->kv, &h->vv, &h->sc, &h->gradws, &h->mllws, &h->mllbws, &h->trainws, &h->cemws, &h->tilews, &h->sepw, &h->tgradws, &h->xch, &h->hio, &h->predws, &h->predbws, &h->covws, &h->momws, &h->mombws, &h->linws, &h->linbws, &h->fbws, &h->fbbws, &h->lqrws, &h->lbfgsws, &h->ilqrws, &h->Xf, &h->Yf, &h->fgws, &h->spws, &h->sprec, &h->selws, &h->spupd};
    for (Buf* b : all) free_buf(*b);
    if (h->hio_host) (void)hipHostFree(h->hio_host);
    if (h->hio_flag) (void)hipHostFree(h->hio_flag);
    if (h->xch_uc) (void)hipFree(h->xch_uc);
    if (h->info) (void)hipFree(h->info);
    if (h->fidx) (void)hipFree(h->fidx);
    if (h->mono_exp) (void)hipFree(h->mono_exp);
    if (h->septab) (void)hipFree(h->septab);
    if (h->side_stream) (void)hipStreamDestroy(h->side_stream);
    if (h->ev_params) (void)hipEventDestroy(h->ev_params);
    if (h->ev_points) (void)hipEventDestroy(h->ev_points);
    delete g;
    return GPMPC_OK;
}

const char* gpmpc_last_error(const gpmpc_t* g) { return g ? g->h.err.c_str() : "null handle"; }

int gpmpc_set_option(gpmpc_t* g, const char* name, long long value) {
    if (!g || !name) return GPMPC_ERR_ARG;
    Handle* h = H_(g);
    for (const Option& o : kOptions) {
        if (strcmp(name, o.name)) continue;
        const long long v = (!o.msg || o.cast_first) ? (long long)(int)value : value;
        if (o.msg && (v < o.lo || v > o.hi || (v & (o.mult - 1)))) { h->err = o.msg; return GPMPC_ERR_ARG; }
        if (o.wide) h->*o.wide = v;
        else h->*o.field = (int)(v < o.lo ? o.lo : v);
        return GPMPC_OK;
    }
    return bad(g, "unknown option");
}

static int check_dims(gpmpc_t* g, int N, int D, int E) {
    if (N < 1 || D < 1 || E < D) return bad(g, "need N >= 1, D >= 1, E >= D");
    if (D > kMaxD || E > kMaxE) { g->h.err = "shape outside compiled limits (D <= 16, E <= 24)"; return GPMPC_ERR_LIMIT; }
    return GPMPC_OK;
}

int gpmpc_prepare(gpmpc_t* g, const double* X, const double* Y, const double* ls, const double* os,
                  const double* noise, int N, int D, int E, void* stream) {
    Range roctx_range("gpmpc_prepare");
    if (!g || !X || !Y || !ls || !os || !noise) return bad(g, "null argument");
    int rc = check_dims(g, N, D, E);
    if (rc) return rc;
    GPMPC_HIP_CHECK(H_(g), hipSetDevice(g->h.device));
    return run_prepare(H_(g), X, Y, ls, os, noise, N, D, E, (hipStream_t)stream);
}

int gpmpc_prepare_sparse(gpmpc_t* g, const double* X, const double* Y, int N, const double* Z, int M, const double* ls,
                         const double* os, const double* noise, double jitter_rel, int D, int E, void* stream) {
    Range roctx_range("gpmpc_prepare_sparse");
    if (!g || !X || !Y || !Z || !ls || !os || !noise) return bad(g, "null argument");
    if (M < 1) return bad(g, "prepare_sparse: need M >= 1 inducing inputs");
    if (!(jitter_rel >= 0.0) || !std::isfinite(jitter_rel)) return bad(g, "prepare_sparse: jitter_rel must be finite and >= 0");
    int rc = check_dims(g, N, D, E);
    if (rc) return rc;
    GPMPC_HIP_CHECK(H_(g), hipSetDevice(g->h.device));
    return run_prepare_sparse(H_(g), X, Y, N, Z, M, ls, os, noise, jitter_rel, D, E, (hipStream_t)stream);
}

int gpmpc_select_inducing(gpmpc_t* g, const double* X, int N, int M, const double* ls, const double* os, double jitter_rel, int D,
                          int E, int* idx_out, double* Z_out, double* trace_out, void* stream) {
    Range roctx_range("gpmpc_select_inducing");
    if (!g || !X || !ls || !os || !idx_out) return bad(g, "null argument");
    if (N < 1) return bad(g, "select_inducing: need N >= 1 memory points");
    if (M < 1 || M > N) return bad(g, "select_inducing: need 1 <= M <= N inducing inputs");
    if (!(jitter_rel >= 0.0) || !std::isfinite(jitter_rel)) return bad(g, "select_inducing: jitter_rel must be finite and >= 0");
    int rc = check_dims(g, N, D, E);
    if (rc) return rc;
    GPMPC_HIP_CHECK(H_(g), hipSetDevice(g->h.device));
    return run_select_inducing(H_(g), X, N, M, ls, os, jitter_rel, D, E, idx_out, Z_out, trace_out, (hipStream_t)stream);
}

int gpmpc_set_factors(gpmpc_t* g, const double* X, const double* iK, const double* beta, const double* ls,
                      const double* os, int N, int D, int E, void* stream) {
    Range roctx_range("gpmpc_set_factors");
    if (!g || !X || !iK || !beta || !ls || !os) return bad(g, "null argument");
    int rc = check_dims(g, N, D, E);
    if (rc) return rc;
    GPMPC_HIP_CHECK(H_(g), hipSetDevice(g->h.device));
    return run_set_factors(H_(g), X, iK, beta, ls, os, N, D, E, (hipStream_t)stream);
}

int gpmpc_get_factors(gpmpc_t* g, const double** iK, const double** beta) {
    if (!g || !g->h.ready) return bad(g, "no factors cached: call gpmpc_prepare first");
    if (iK) *iK = g->h.iK.p;
    if (beta) *beta = g->h.beta.p;
    return GPMPC_OK;
}

int gpmpc_read_factors(gpmpc_t* g, double* iK_dst, double* beta_dst, void* stream) {
    if (!g || !g->h.ready) return bad(g, "no factors cached: call gpmpc_prepare first");
    Handle* h = H_(g);
    GPMPC_HIP_CHECK(h, hipSetDevice(h->device));
    const size_t DN = (size_t)h->D * h->N;
    if (iK_dst) GPMPC_HIP_CHECK(h, hipMemcpyAsync(iK_dst, h->iK.p, DN * h->N * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (beta_dst) GPMPC_HIP_CHECK(h, hipMemcpyAsync(beta_dst, h->beta.p, DN * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return GPMPC_OK;
}

int gpmpc_predict(gpmpc_t* g, const double* Xq, int M, int D, int E, const double* noises_host, double* mean_out,
                  double* var_out, void* stream) {
    Range roctx_range("gpmpc_predict");
    return query_entry(g, "predict", "M", M, D, E, false, Xq != nullptr, [&](Handle* h) {
        return run_predict(h, Xq, M, noises_host, mean_out, var_out, (hipStream_t)stream);
    });
}

int gpmpc_predict_backward(gpmpc_t* g, const double* Xq, int M, int D, int E, const double* mean_bar, const double* var_bar,
                           double* Xq_bar_out, void* stream) {
    Range roctx_range("gpmpc_predict_backward");
    return query_entry(g, "predict_backward", "M", M, D, E, false, Xq && Xq_bar_out, [&](Handle* h) {
        return run_predict_backward(h, Xq, M, mean_bar, var_bar, Xq_bar_out, (hipStream_t)stream);
    });
}

int gpmpc_predict_cov(gpmpc_t* g, const double* Xa, int Ma, const double* Xb, int Mb, int D, int E, const double* noises_host,
                      double* cov_out, void* stream) {
    Range roctx_range("gpmpc_predict_cov");
    int rc = query_checks(g, "predict_cov", nullptr, 0, D, E, false);
    if (rc) return rc;
    if (Ma < 0 || (Xb && Mb < 0)) return bad(g, "predict_cov: negative number of points");
    if (Xb && noises_host) return bad(g, "predict_cov: the cross form takes no noise");
    if (Ma > (1 << 22) || (Xb && Mb > (1 << 22))) return bad(g, "predict_cov: more than 2^22 points");
    if (Ma == 0 || (Xb && Mb == 0)) return GPMPC_OK;
    if (!Xa || !cov_out) return bad(g, "null argument");
    GPMPC_HIP_CHECK(H_(g), hipSetDevice(g->h.device));
    return run_predict_cov(H_(g), Xa, Ma, Xb, Mb, noises_host, cov_out, (hipStream_t)stream);
}

int gpmpc_moments(gpmpc_t* g, const double* mu, const double* var, int P, int D, int E, double* M_out, double* S_out,
                  double* V_out, void* stream) {
    Range roctx_range("gpmpc_moments");
    return query_entry(g, "moments", "P", P, D, E, true, mu && M_out, [&](Handle* h) {
        return run_moments(h, mu, var, P, M_out, S_out, V_out, (hipStream_t)stream);
    });
}

int gpmpc_moments_linear(gpmpc_t* g, const double* mu, const double* var, int P, int D, int E, double* M_out, double* S_out,
                         double* V_out, void* stream) {
    Range roctx_range("gpmpc_moments_linear");
    return query_entry(g, "moments_linear", "P", P, D, E, true, mu != nullptr, [&](Handle* h) {
        return run_moments_linear(h, mu, var, P, M_out, S_out, V_out, (hipStream_t)stream);
    });
}

int gpmpc_moments_backward(gpmpc_t* g, const double* mu, const double* var, int P, int D, int E, const double* M_bar,
                           const double* S_bar, const double* V_bar, double* mu_bar_out, double* var_bar_out, void* stream) {
    Range roctx_range("gpmpc_moments_backward");
    return query_entry(g, "moments_backward", "P", P, D, E, true, mu != nullptr, [&](Handle* h) {
        return run_moments_backward(h, mu, var, P, M_bar, S_bar, V_bar, mu_bar_out, var_bar_out, (hipStream_t)stream);
    });
}

int gpmpc_moments_linear_backward(gpmpc_t* g, const double* mu, const double* var, int P, int D, int E, const double* M_bar,
                                  const double* S_bar, const double* V_bar, double* mu_bar_out, double* var_bar_out,
                                  void* stream) {
    Range roctx_range("gpmpc_moments_linear_backward");
    return query_entry(g, "moments_linear_backward", "P", P, D, E, true, mu != nullptr, [&](Handle* h) {
        return run_moments_linear_backward(h, mu, var, P, M_bar, S_bar, V_bar, mu_bar_out, var_bar_out, (hipStream_t)stream);
    });
}

int gpmpc_mll(gpmpc_t* g, const double* X, const double* Y, const double* ls, const double* os, const double* noise,
              int N, int D, int E, double* out_host, void* stream) {
    Range roctx_range("gpmpc_mll");
    if (!g) return GPMPC_ERR_ARG;
    if (!X || !Y || !ls || !os || !noise || !out_host) return bad(g, "null argument");
    int rc = check_dims(g, N, D, E);
    if (rc) return rc;
    GPMPC_HIP_CHECK(H_(g), hipSetDevice(g->h.device));
    return run_mll(H_(g), X, Y, ls, os, noise, N, D, E, out_host, (hipStream_t)stream);
}

int gpmpc_forget(gpmpc_t* g, const int* idx_host, int k, void* stream) {
    Range roctx_range("gpmpc_forget");
    if (!g) return GPMPC_ERR_ARG;
    Handle* h = H_(g);
    if (!h->ready || !h->have_state) return bad(g, "forget: the handle holds no record of a gpmpc_prepare");
    if (!idx_host) return bad(g, "null argument");
    if (k < 1 || k >= h->N) return bad(g, "forget: need 1 <= k < N");
    for (int q = 0; q < k; ++q)
        if (idx_host[q] < 0 || idx_host[q] >= h->N || (q > 0 && idx_host[q] <= idx_host[q - 1]))
            return bad(g, "forget: indices must be strictly ascending and in [0, N)");
    GPMPC_HIP_CHECK(h, hipSetDevice(h->device));
    return run_forget(h, idx_host, k, (hipStream_t)stream);
}

int gpmpc_last_prepare_mode(gpmpc_t* g) { return g ? g->h.last_prepare_mode : GPMPC_ERR_ARG; }

int gpmpc_last_rollout_path(gpmpc_t* g) { return g ? g->h.last_rollout_path : GPMPC_ERR_ARG; }
int gpmpc_last_cluster(gpmpc_t* g) { return g ? g->h.last_cluster : GPMPC_ERR_ARG; }
int gpmpc_last_pair_groups(gpmpc_t* g) { return g ? g->h.last_pair_groups : GPMPC_ERR_ARG; }

int gpmpc_last_grad_path(gpmpc_t* g) { return g ? g->h.last_grad_path : GPMPC_ERR_ARG; }

#ifndef GPMPC_BUILD_ID
#define GPMPC_BUILD_ID "unknown"
#endif
const char* gpmpc_build_id(void) { return GPMPC_BUILD_ID; }

int gpmpc_set_cost(gpmpc_t* g, const double* target, const double* W, const double* W_T, double kappa,
                   int clip, const double* smin, const double* smax, int D, int A) {
    if (!g || !target || !W || !W_T) return bad(g, "null argument");
    if (D < 1 || A < 0 || D > kMaxD || D + A > kMaxE) return bad(g, "bad D / A");
    if ((smin == nullptr) != (smax == nullptr)) return bad(g, "state_min and state_max must both be given or both be NULL");
    Handle* h = H_(g);
    GPMPC_HIP_CHECK(h, hipSetDevice(h->device));
    const int DA = D + A;
    const size_t n = (size_t)DA + (size_t)DA * DA + (size_t)D * D + 2 * (size_t)D;
    int rc = grow(h, h->cost, n);
    if (rc) return rc;
    double host[kMaxE + kMaxE * kMaxE + kMaxD * kMaxD + 2 * kMaxD];
    double* q = host;
    memcpy(q, target, DA * sizeof(double)); q += DA;
    memcpy(q, W, (size_t)DA * DA * sizeof(double)); q += DA * DA;
    memcpy(q, W_T, (size_t)D * D * sizeof(double)); q += D * D;
    for (int d = 0; d < D; ++d) q[d] = smin ? smin[d] : 0.0;
    q += D;
    for (int d = 0; d < D; ++d) q[d] = smax ? smax[d] : 0.0;
    GPMPC_HIP_CHECK(h, hipMemcpy(h->cost.p, host, n * sizeof(double), hipMemcpyHostToDevice));
    h->cost_D = D; h->cost_A = A; h->kappa = kappa; h->clip = clip; h->use_constraints = smin ? 1 : 0;
    return GPMPC_OK;
}

static int fill_args(gpmpc_t* g, RolloutArgs& a, const double* actions, const double* mu0, const double* S0,
                     int B, int H, int A, int include_time, double time0, bool need_cost = true) {
    Handle* h = H_(g);
    if (!h->ready) return bad(g, "rollout before prepare / set_factors");
    if (!actions || !mu0 || !S0) return bad(g, "null argument");
    if (B < 1 || H < 1 || A < 0) return bad(g, "need B >= 1, H >= 1");
    if (h->D + A + (include_time ? 1 : 0) != h->E) return bad(g, "D + A (+1 with time) must equal the model's input dim E");
    if (need_cost && (h->cost_D != h->D || h->cost_A != A)) return bad(g, "gpmpc_set_cost not called for this (D, A)");
    memset(&a, 0, sizeof a);
    a.Xt = h->Xt.p; a.beta = h->beta.p; a.Tm = h->Tm.p; a.ils2 = h->ils2.p; a.var = h->var.p; a.logvar = h->logvar.p;
    a.cost = h->cost.p; a.kappa = h->kappa; a.clip = h->clip; a.use_constraints = h->use_constraints;
    a.actions = actions;
    a.N = h->N; a.D = h->D; a.A = A; a.E = h->E; a.H = H; a.B = B;
    a.include_time = include_time; a.time0 = time0;
    memcpy(a.mu0, mu0, h->D * sizeof(double));
    memcpy(a.S0, S0, (size_t)h->D * h->D * sizeof(double));
    return GPMPC_OK;
}

// The body of the three forward rollout entries: `linear` false is moment matching (no gains), true the linearised step, in closed
// loop where `gains` is given.  The trajectory alone (predict_trajectory, gp_model.py:60-110) needs no cost settings.
static int rollout_entry(gpmpc_t* g, bool linear, const double* actions, const double* gains, int gains_per_candidate,
                         const double* mu0, const double* S0, int B, int H, int A, int include_time, double time0, double* mu_out,
                         double* Sig_out, double* cm_out, double* cv_out, double* J_out, void* stream) {
    if (!g) return GPMPC_ERR_ARG;
    RolloutArgs a;
    int rc = fill_args(g, a, actions, mu0, S0, B, H, A, include_time, time0, cm_out || cv_out || J_out);
    if (rc) return rc;
    if (gains && A < 1) return bad(g, "feedback gains need A >= 1");
    GPMPC_HIP_CHECK(H_(g), hipSetDevice(g->h.device));
    a.mu_out = mu_out; a.Sig_out = Sig_out; a.cm_out = cm_out; a.cv_out = cv_out; a.J_out = J_out;
    if (!linear) return launch_rollout(H_(g), a, (hipStream_t)stream);
    return run_rollout_linear(H_(g), a, (hipStream_t)stream, gains, gains && gains_per_candidate != 0);
}

int gpmpc_rollout(gpmpc_t* g, const double* actions, const double* mu0, const double* S0, int B, int H, int A,
                  int include_time, double time0, double* mu_out, double* Sig_out, double* cm_out, double* cv_out,
                  double* J_out, void* stream) {
    Range roctx_range("gpmpc_rollout");
    return rollout_entry(g, false, actions, nullptr, 0, mu0, S0, B, H, A, include_time, time0, mu_out, Sig_out, cm_out, cv_out, J_out,
                         stream);
}

int gpmpc_rollout_linear(gpmpc_t* g, const double* actions, const double* mu0, const double* S0, int B, int H, int A,
                         int include_time, double time0, double* mu_out, double* Sig_out, double* cm_out, double* cv_out,
                         double* J_out, void* stream) {
    Range roctx_range("gpmpc_rollout_linear");
    return rollout_entry(g, true, actions, nullptr, 0, mu0, S0, B, H, A, include_time, time0, mu_out, Sig_out, cm_out, cv_out, J_out,
                         stream);
}

int gpmpc_rollout_linear_feedback(gpmpc_t* g, const double* actions, const double* gains, int gains_per_candidate,
                                  const double* mu0, const double* S0, int B, int H, int A, int include_time, double time0,
                                  double* mu_out, double* Sig_out, double* cm_out, double* cv_out, double* J_out, void* stream) {
    // without gains the call IS gpmpc_rollout_linear: the same launches, the same bits, the same range
    Range roctx_range(gains ? "gpmpc_rollout_linear_feedback" : "gpmpc_rollout_linear");
    return rollout_entry(g, true, actions, gains, gains_per_candidate, mu0, S0, B, H, A, include_time, time0, mu_out, Sig_out, cm_out,
                         cv_out, J_out, stream);
}

int gpmpc_rollout_feedback(gpmpc_t* g, const double* actions, const double* gains, int gains_per_candidate, const double* mu0,
                           const double* S0, int B, int H, int A, int include_time, double time0, double* mu_out, double* Sig_out,
                           double* cm_out, double* cv_out, double* J_out, void* stream) {
    Range roctx_range("gpmpc_rollout_feedback");
    if (!g) return GPMPC_ERR_ARG;
    RolloutArgs a;
    int rc = fill_args(g, a, actions, mu0, S0, B, H, A, include_time, time0, cm_out || cv_out || J_out);
    if (rc) return rc;
    if (gains && A < 1) return bad(g, "feedback gains need A >= 1");
    if (a.D > GPMPC_MAX_D || a.E > GPMPC_MAX_E) {
        g->h.err = "rollout_feedback: D or E beyond the compiled limits";
        return GPMPC_ERR_LIMIT;
    }
    GPMPC_HIP_CHECK(H_(g), hipSetDevice(g->h.device));
    a.mu_out = mu_out; a.Sig_out = Sig_out; a.cm_out = cm_out; a.cv_out = cv_out; a.J_out = J_out;
    // without gains: the all-zero policy through the closed-loop kernels (gpmpc_rollout to rounding, not bit for bit)
    return run_rollout_feedback(H_(g), a, (hipStream_t)stream, gains, gains && gains_per_candidate != 0);
}

int gpmpc_lqr_gains(gpmpc_t* g, const double* actions, const double* mu0, int B, int H, int A, int include_time, double time0,
                    double reg, double* gains_out, double* P_out, int* flags_out, void* stream) {
    Range roctx_range("gpmpc_lqr_gains");
    if (!g) return GPMPC_ERR_ARG;
    Handle* h = H_(g);
    if (!h->ready) return bad(g, "lqr_gains before prepare / set_factors");
    if (!actions || !mu0 || !gains_out) return bad(g, "null argument");
    if (B < 1 || H < 1 || A < 1) return bad(g, "lqr_gains: need B >= 1, H >= 1, A >= 1");
    if (h->D + A + (include_time ? 1 : 0) != h->E) return bad(g, "D + A (+1 with time) must equal the model's input dim E");
    if (!(reg >= 0.0) || !std::isfinite(reg)) return bad(g, "lqr_gains: reg must be finite and >= 0");
    if (A > kLqrMaxA) {
        h->err = "lqr_gains: A beyond the compiled limit (A <= 8)";
        return GPMPC_ERR_LIMIT;
    }
    if (h->cost_D != h->D || h->cost_A != A) return bad(g, "gpmpc_set_cost not called for this (D, A)");
    GPMPC_HIP_CHECK(h, hipSetDevice(h->device));
    return run_lqr_gains(h, actions, mu0, B, H, A, include_time, time0, reg, gains_out, P_out, flags_out, (hipStream_t)stream);
}

int gpmpc_rollout_grad(gpmpc_t* g, const double* actions, const double* mu0, const double* S0, int B, int H, int A,
                       int include_time, double time0, double* J_out, double* grad_out, double* mu_out, double* Sig_out,
                       double* cm_out, double* cv_out, void* stream) {
    Range roctx_range("gpmpc_rollout_grad");
    if (!g) return GPMPC_ERR_ARG;
    if (!grad_out) return bad(g, "null argument");
    RolloutArgs a;
    int rc = fill_args(g, a, actions, mu0, S0, B, H, A, include_time, time0);
    if (rc) return rc;
    if (A < 1) return bad(g, "gradient needs A >= 1");
    GPMPC_HIP_CHECK(H_(g), hipSetDevice(g->h.device));
    a.mu_out = mu_out; a.Sig_out = Sig_out; a.J_out = J_out; a.cm_out = cm_out; a.cv_out = cv_out;
    return launch_rollout_grad(H_(g), a, grad_out, (hipStream_t)stream);
}

// The body of the three backward rollout entries, `linear` and `gains` as in rollout_entry.  The trajectory's cotangents alone need
// no cost settings; a cost or objective seed needs gpmpc_set_cost for this (D, A).
static int rollout_backward_entry(gpmpc_t* g, bool linear, const double* actions, const double* gains, int gains_per_candidate,
                                  const double* mu0, const double* S0, int B, int H, int A, int include_time, double time0,
                                  const double* mu_bar, const double* Sig_bar, const double* cm_bar, const double* cv_bar,
                                  const double* J_bar, double* actions_bar_out, double* gains_bar_out, double* mu0_bar_out,
                                  double* S0_bar_out, void* stream) {
    if (!g) return GPMPC_ERR_ARG;
    if (!actions_bar_out) return bad(g, "null argument");
    RolloutSeeds sd{mu_bar, Sig_bar, cm_bar, cv_bar, J_bar, mu0_bar_out, S0_bar_out, cm_bar || cv_bar || J_bar};
    RolloutArgs a;
    int rc = fill_args(g, a, actions, mu0, S0, B, H, A, include_time, time0, sd.cost);
    if (rc) return rc;
    if (A < 1) return bad(g, "gradient needs A >= 1");
    GPMPC_HIP_CHECK(H_(g), hipSetDevice(g->h.device));
    hipStream_t s = (hipStream_t)stream;
    if (!linear) return launch_rollout_grad(H_(g), a, actions_bar_out, s, &sd);
    if (!gains) return run_rollout_linear_backward(H_(g), a, sd, actions_bar_out, s);
    return run_rollout_linear_feedback_backward(H_(g), a, sd, gains, gains_per_candidate != 0, actions_bar_out, gains_bar_out, s);
}

int gpmpc_rollout_backward(gpmpc_t* g, const double* actions, const double* mu0, const double* S0, int B, int H, int A,
                           int include_time, double time0, const double* mu_bar, const double* Sig_bar, const double* cm_bar,
                           const double* cv_bar, const double* J_bar, double* actions_bar_out, double* mu0_bar_out,
                           double* S0_bar_out, void* stream) {
    Range roctx_range("gpmpc_rollout_backward");
    return rollout_backward_entry(g, false, actions, nullptr, 0, mu0, S0, B, H, A, include_time, time0, mu_bar, Sig_bar, cm_bar, cv_bar,
                                  J_bar, actions_bar_out, nullptr, mu0_bar_out, S0_bar_out, stream);
}

int gpmpc_rollout_linear_backward(gpmpc_t* g, const double* actions, const double* mu0, const double* S0, int B, int H, int A,
                                  int include_time, double time0, const double* mu_bar, const double* Sig_bar,
                                  const double* cm_bar, const double* cv_bar, const double* J_bar, double* actions_bar_out,
                                  double* mu0_bar_out, double* S0_bar_out, void* stream) {
    Range roctx_range("gpmpc_rollout_linear_backward");
    return rollout_backward_entry(g, true, actions, nullptr, 0, mu0, S0, B, H, A, include_time, time0, mu_bar, Sig_bar, cm_bar, cv_bar,
                                  J_bar, actions_bar_out, nullptr, mu0_bar_out, S0_bar_out, stream);
}

int gpmpc_rollout_linear_feedback_backward(gpmpc_t* g, const double* actions, const double* gains, int gains_per_candidate,
                                           const double* mu0, const double* S0, int B, int H, int A, int include_time,
                                           double time0, const double* mu_bar, const double* Sig_bar, const double* cm_bar,
                                           const double* cv_bar, const double* J_bar, double* actions_bar_out,
                                           double* gains_bar_out, double* mu0_bar_out, double* S0_bar_out, void* stream) {
    if (g && !gains && gains_bar_out) return bad(g, "gains_bar_out without gains");
    // without gains the call IS gpmpc_rollout_linear_backward: the same launches, the same bits, the same range
    Range roctx_range(gains ? "gpmpc_rollout_linear_feedback_backward" : "gpmpc_rollout_linear_backward");
    return rollout_backward_entry(g, true, actions, gains, gains_per_candidate, mu0, S0, B, H, A, include_time, time0, mu_bar, Sig_bar,
                                  cm_bar, cv_bar, J_bar, actions_bar_out, gains_bar_out, mu0_bar_out, S0_bar_out, stream);
}

int gpmpc_rollout_feedback_backward(gpmpc_t* g, const double* actions, const double* gains, int gains_per_candidate,
                                    const double* mu0, const double* S0, int B, int H, int A, int include_time, double time0,
                                    const double* mu_bar, const double* Sig_bar, const double* cm_bar, const double* cv_bar,
                                    const double* J_bar, double* actions_bar_out, double* gains_bar_out, double* mu0_bar_out,
                                    double* S0_bar_out, void* stream) {
    Range roctx_range("gpmpc_rollout_feedback_backward");
    if (!g) return GPMPC_ERR_ARG;
    if (!actions_bar_out) return bad(g, "null argument");
    if (!gains && gains_bar_out) return bad(g, "gains_bar_out without gains");
    RolloutSeeds sd{mu_bar, Sig_bar, cm_bar, cv_bar, J_bar, mu0_bar_out, S0_bar_out, cm_bar || cv_bar || J_bar};
    RolloutArgs a;
    int rc = fill_args(g, a, actions, mu0, S0, B, H, A, include_time, time0, sd.cost);
    if (rc) return rc;
    if (A < 1) return bad(g, "gradient needs A >= 1");
    if (a.D > GPMPC_MAX_D || a.E > GPMPC_MAX_E) {
        g->h.err = "rollout_feedback_backward: D or E beyond the compiled limits";
        return GPMPC_ERR_LIMIT;
    }
    GPMPC_HIP_CHECK(H_(g), hipSetDevice(g->h.device));
    // without gains: the all-zero policy through the closed-loop kernels (gpmpc_rollout_backward to rounding, not bit for bit)
    return run_rollout_feedback_backward(H_(g), a, sd, gains, gains && gains_per_candidate != 0, actions_bar_out, gains_bar_out,
                                         (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------
// One evaluation for a host-side optimiser: the action sequence travels to the device in the forward kernel's argument block (no
// DMA engine start-up, no launch of its own for 200 bytes), the results come back through a pinned, device-mapped host buffer
// written by the last kernel of the evaluation, which then raises a sequence number the host polls.
namespace {
constexpr int kUploadMax = 480;                        // doubles in the argument block (< 4 KiB)
struct UploadArgs { double v[kUploadMax]; };
__global__ __launch_bounds__(64) void upload_kernel(double* dst, int n, const UploadArgs a) {
    for (int i = threadIdx.x; i < n; i += 64) dst[i] = a.v[i];
}
}  // namespace

int gpmpc_objective_grad_host(gpmpc_t* g, const double* actions_host, const double* mu0, const double* S0, int H, int A,
                              int include_time, double time0, const double** result_host, void* stream) {
    Range roctx_range("gpmpc_objective_grad_host");
    if (!g) return GPMPC_ERR_ARG;
    if (!actions_host || !result_host) return bad(g, "null argument");
    Handle* h = H_(g);
    hipStream_t s = (hipStream_t)stream;
    RolloutArgs a;
    int rc = fill_args(g, a, actions_host, mu0, S0, 1, H, A, include_time, time0);
    if (rc) return rc;
    if (A < 1) return bad(g, "gradient needs A >= 1");
    GPMPC_HIP_CHECK(h, hipSetDevice(h->device));
    const int D = h->D, n_act = H * A;
    const size_t n_out = 1 + (size_t)n_act + (size_t)(H + 1) * (D + D * D + 2);
    rc = grow(h, h->hio, (size_t)n_act + n_out);
    if (rc) return rc;
    if (h->hio_host_cap < n_out) {
        if (h->hio_host) GPMPC_HIP_CHECK(h, hipHostFree(h->hio_host));
        h->hio_host = nullptr; h->hio_host_dev = nullptr; h->hio_host_cap = 0;
        GPMPC_HIP_CHECK(h, hipHostMalloc(reinterpret_cast<void**>(&h->hio_host), n_out * sizeof(double), hipHostMallocMapped));
        GPMPC_HIP_CHECK(h, hipHostGetDevicePointer(reinterpret_cast<void**>(&h->hio_host_dev), h->hio_host, 0));
        h->hio_host_cap = n_out;
    }
    if (!h->hio_flag) {
        GPMPC_HIP_CHECK(h, hipHostMalloc(reinterpret_cast<void**>(&h->hio_flag), 64, hipHostMallocMapped));
        GPMPC_HIP_CHECK(h, hipHostGetDevicePointer(reinterpret_cast<void**>(&h->hio_flag_dev), h->hio_flag, 0));
        *h->hio_flag = 0;
    }
    double* act_dev = h->hio.p;
    double* out_dev = act_dev + n_act;
    a.act_inline_n = 0;
    if (n_act <= kInlineActs) {                 // in the forward kernel's argument block (launch_rollout uploads for the other paths)
        a.act_inline_n = n_act;
        a.act_store = act_dev;
        memcpy(a.act_inline, actions_host, n_act * sizeof(double));
    } else if (n_act <= kUploadMax) {
        UploadArgs u;
        memcpy(u.v, actions_host, n_act * sizeof(double));
        hipLaunchKernelGGL(upload_kernel, dim3(1), dim3(64), 0, s, act_dev, n_act, u);
        GPMPC_HIP_CHECK(h, hipGetLastError());
    } else {
        GPMPC_HIP_CHECK(h, hipMemcpyAsync(act_dev, actions_host, n_act * sizeof(double), hipMemcpyHostToDevice, s));
    }
    a.actions = act_dev;
    double* q = out_dev;
    a.J_out = q; q += 1;
    double* grad = q; q += n_act;
    a.mu_out = q; q += (size_t)(H + 1) * D;
    a.Sig_out = q; q += (size_t)(H + 1) * D * D;
    a.cm_out = q; q += H + 1;
    a.cv_out = q;
    // The reverse sweep -- the last kernel of the evaluation -- copies the results to the pinned mirror and then raises this call's
    // sequence number there; the host polls that word (a stream synchronisation costs ~10 us more than the store takes to arrive)
    // and asks the stream now and then, so that a failed launch ends the wait.
    const unsigned long long seq = ++h->hio_seq;
    const bool sweep_exports = D <= 8;               // (the wide-state sweep, 8 < D <= 16, has no export: a synchronisation and a copy)
    h->hx_out = h->hio_host_dev; h->hx_src = out_dev; h->hx_n = sweep_exports ? (int)n_out : 0;
    rc = launch_rollout_grad(h, a, grad, s);
    h->hx_n = 0;
    if (rc) return rc;
    if (!sweep_exports) {
        GPMPC_HIP_CHECK(h, hipStreamSynchronize(s));
        GPMPC_HIP_CHECK(h, hipMemcpy(h->hio_host, out_dev, n_out * sizeof(double), hipMemcpyDeviceToHost));
        *result_host = h->hio_host;
        return GPMPC_OK;
    }
    volatile unsigned long long* flag = h->hio_flag;
    for (unsigned spins = 1; *flag != seq; ++spins) {
        __builtin_ia32_pause();
        if ((spins & 0xfff) == 0) {
            const hipError_t qe = hipStreamQuery(s);
            if (qe == hipSuccess) {
                if (*flag == seq) break;
                h->err = "objective_grad_host: the launches ended without the sweep's completion word";
                return GPMPC_ERR_HIP;
            }
            if (qe != hipErrorNotReady) GPMPC_HIP_CHECK(h, qe);
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    *result_host = h->hio_host;
    return GPMPC_OK;
}

int gpmpc_cem_search(gpmpc_t* g, const double* mu0, const double* S0, int B, int H, int A, int include_time, double time0,
                     int iterations, int n_elite, unsigned long long seed, const double* first_candidate, int mapper,
                     const double* max_change, const double* action_prev, const double* noise_dev, double* best_out_dev,
                     void* stream) {
    Range roctx_range("gpmpc_cem_search");
    if (!g) return GPMPC_ERR_ARG;
    if (!best_out_dev) return bad(g, "null argument");
    Handle* h = H_(g);
    if (!h->ready) return bad(g, "search before prepare / set_factors");
    // fill_args wants an actions pointer; the search supplies its own device buffer afterwards
    RolloutArgs a;
    int rc = fill_args(g, a, best_out_dev, mu0, S0, B, H, A, include_time, time0);
    if (rc) return rc;
    GPMPC_HIP_CHECK(h, hipSetDevice(h->device));
    return run_cem_search(h, a, iterations, n_elite, seed, first_candidate, mapper, max_change, action_prev, noise_dev,
                          best_out_dev, (hipStream_t)stream);
}

int gpmpc_cem_local(gpmpc_t* g, const double* mu0, const double* S0, int B_total, int first, int B_local, int H, int A,
                    int include_time, double time0, int iteration, int n_elite, unsigned long long seed,
                    const double* first_candidate, int mapper, const double* max_change, const double* action_prev,
                    const double* noise_dev, const double* state_dev, double* elites_out_dev, void* stream) {
    Range roctx_range("gpmpc_cem_local");
    if (!g) return GPMPC_ERR_ARG;
    if (!state_dev || !elites_out_dev) return bad(g, "null argument");
    Handle* h = H_(g);
    if (!h->ready) return bad(g, "search before prepare / set_factors");
    if (B_local < 0) return bad(g, "negative slice length");
    RolloutArgs a;
    int rc = fill_args(g, a, state_dev, mu0, S0, B_local > 0 ? B_local : 1, H, A, include_time, time0);
    if (rc) return rc;
    a.B = B_local;
    GPMPC_HIP_CHECK(h, hipSetDevice(h->device));
    return run_cem_local(h, a, B_total, first, iteration, n_elite, seed, first_candidate, mapper, max_change, action_prev,
                         noise_dev, state_dev, elites_out_dev, (hipStream_t)stream);
}

int gpmpc_cem_merge(gpmpc_t* g, const double* elites_dev, int lists, int n_elite, int n, int iteration, double* state_dev,
                    void* stream) {
    Range roctx_range("gpmpc_cem_merge");
    if (!g) return GPMPC_ERR_ARG;
    if (!elites_dev || !state_dev) return bad(g, "null argument");
    Handle* h = H_(g);
    GPMPC_HIP_CHECK(h, hipSetDevice(h->device));
    return run_cem_merge(h, elites_dev, lists, n_elite, n, iteration, state_dev, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------
// Device-resident L-BFGS (lbfgs_search.hip).  The mapper's parameters travel in the kernels' argument blocks.
// the checks the three entry points share; on success `mp` holds the mapper's parameters
static int lbfgs_entry_checks(gpmpc_t* g, int B, int H, int A, int history, int mapper, const double* max_change,
                              const double* action_prev, ActionMapper& mp) {
    bool limit = false;
    const char* msg = lbfgs_check_shape(B, H, A, history, limit);
    if (!msg) msg = lbfgs_check_mapper(mapper, A, max_change != nullptr, action_prev != nullptr, limit);
    if (msg) { g->h.err = msg; return limit ? GPMPC_ERR_LIMIT : GPMPC_ERR_ARG; }
    memset(&mp, 0, sizeof mp);
    mp.mapper = mapper;
    if (mapper == 1) {
        memcpy(mp.max_change, max_change, A * sizeof(double));
        memcpy(mp.action_prev, action_prev, A * sizeof(double));
    }
    return GPMPC_OK;
}

long long gpmpc_lbfgs_state_size(int B, int n, int history) {
    bool limit = false;
    if (lbfgs_check_shape(B, n, 1, history, limit)) return -1;
    return (long long)make_lbfgs_layout(B, n, history).total;
}

int gpmpc_lbfgs_init(gpmpc_t* g, const double* x0_dev, int B, int H, int A, int history, int mapper, const double* max_change,
                     const double* action_prev, double* state_dev, void* stream) {
    Range roctx_range("gpmpc_lbfgs_init");
    if (!g) return GPMPC_ERR_ARG;
    if (!x0_dev || !state_dev) return bad(g, "null argument");
    ActionMapper mp;
    int rc = lbfgs_entry_checks(g, B, H, A, history, mapper, max_change, action_prev, mp);
    if (rc) return rc;
    GPMPC_HIP_CHECK(H_(g), hipSetDevice(g->h.device));
    return run_lbfgs_init(H_(g), x0_dev, B, H, A, history, mp, state_dev, (hipStream_t)stream);
}

int gpmpc_lbfgs_step(gpmpc_t* g, const double* J_dev, const double* grad_model_dev, int B, int H, int A, int iteration, int history,
                     double c1, double pgtol, int mapper, const double* max_change, const double* action_prev, double* state_dev,
                     void* stream) {
    Range roctx_range("gpmpc_lbfgs_step");
    if (!g) return GPMPC_ERR_ARG;
    if (!J_dev || !grad_model_dev || !state_dev) return bad(g, "null argument");
    ActionMapper mp;
    int rc = lbfgs_entry_checks(g, B, H, A, history, mapper, max_change, action_prev, mp);
    if (rc) return rc;
    if (const char* msg = lbfgs_check_step(iteration, c1, pgtol)) return bad(g, msg);
    GPMPC_HIP_CHECK(H_(g), hipSetDevice(g->h.device));
    return run_lbfgs_step(H_(g), J_dev, grad_model_dev, B, H, A, iteration, history, c1, pgtol, mp, state_dev, (hipStream_t)stream);
}

int gpmpc_lbfgs_search(gpmpc_t* g, const double* mu0, const double* S0, int B, int H, int A, int include_time, double time0,
                       int propagation, int first_iteration, int iterations, int history, double c1, double pgtol, int mapper,
                       const double* max_change, const double* action_prev, const double* x0_dev, double* state_dev,
                       double* best_out_dev, void* stream) {
    Range roctx_range("gpmpc_lbfgs_search");
    if (!g) return GPMPC_ERR_ARG;
    if (!state_dev || (first_iteration == 0 && !x0_dev)) return bad(g, "null argument");
    Handle* h = H_(g);
    if (!h->ready) return bad(g, "search before prepare / set_factors");
    ActionMapper mp;
    int rc = lbfgs_entry_checks(g, B, H, A, history, mapper, max_change, action_prev, mp);
    if (rc) return rc;
    if (const char* msg = lbfgs_check_step(first_iteration, c1, pgtol)) return bad(g, msg);
    if (iterations < 1) return bad(g, "lbfgs: need iterations >= 1");
    if (propagation != 0 && propagation != 1) return bad(g, "lbfgs: propagation must be 0 (moment matching) or 1 (linearised)");
    // fill_args wants an actions pointer; the search points it at the state's model actions afterwards
    RolloutArgs a;
    rc = fill_args(g, a, state_dev, mu0, S0, B, H, A, include_time, time0);
    if (rc) return rc;
    GPMPC_HIP_CHECK(h, hipSetDevice(h->device));
    return run_lbfgs_search(h, a, propagation, first_iteration, iterations, history, c1, pgtol, mp, x0_dev, state_dev, best_out_dev,
                            (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------
// Batched training loss and the multi-restart search on it (mll_batch.hip).  The checks the two entries share, in their order:
// pointers and counts (GPMPC_ERR_ARG), then the compiled limits (GPMPC_ERR_LIMIT).
static int mll_batch_checks(gpmpc_t* g, bool ptrs_ok, const double* lo, const double* hi, bool need_box, int N, int D, int E, int R,
                            int log_scale) {
    if (!ptrs_ok) return bad(g, "null argument");
    if ((lo == nullptr) != (hi == nullptr)) return bad(g, "mll_batch: lo and hi must both be given or both be NULL");
    if (need_box && !lo) return bad(g, "train_search: the box (lo, hi) is required");
    if (N < 1 || R < 1 || D < 1 || E < 1) return bad(g, "mll_batch: need N >= 1, R >= 1, D >= 1, E >= 1");
    if (log_scale != 0 && log_scale != 1) return bad(g, "mll_batch: log_scale must be 0 (linear map) or 1 (log map)");
    const char* over = nullptr;
    if (N > 256) over = "mll_batch: at most 256 memory points (one workgroup per problem)";
    else if (D > kMaxD || E > kMaxE) over = "shape outside compiled limits (D <= 16, E <= 24)";
    else if ((long long)R * D > kLbfgsMaxB) over = "mll_batch: at most 4096 problems (R * D)";
    if (over) { g->h.err = over; return GPMPC_ERR_LIMIT; }
    return GPMPC_OK;
}

int gpmpc_mll_batch(gpmpc_t* g, const double* X, const double* Y, int N, int D, int E, const double* params, int R,
                    const double* lo, const double* hi, int log_scale, double* loss_out, double* grad_out, double* theta_out,
                    int* info_out, void* stream) {
    Range roctx_range("gpmpc_mll_batch");
    if (!g) return GPMPC_ERR_ARG;
    int rc = mll_batch_checks(g, X && Y && params && loss_out && grad_out, lo, hi, false, N, D, E, R, log_scale);
    if (rc) return rc;
    GPMPC_HIP_CHECK(H_(g), hipSetDevice(g->h.device));
    return run_mll_batch(H_(g), X, Y, N, D, E, params, R, lo, hi, log_scale, loss_out, grad_out, theta_out, info_out,
                         (hipStream_t)stream);
}

int gpmpc_train_search(gpmpc_t* g, const double* X, const double* Y, int N, int D, int E, int R, const double* lo, const double* hi,
                       int log_scale, int first_iteration, int iterations, int history, double c1, double pgtol,
                       const double* x0_dev, double* state_dev, double* best_out_dev, void* stream) {
    Range roctx_range("gpmpc_train_search");
    if (!g) return GPMPC_ERR_ARG;
    int rc = mll_batch_checks(g, X && Y && state_dev && (first_iteration != 0 || x0_dev), lo, hi, true, N, D, E, R, log_scale);
    if (rc) return rc;
    bool limit = false;
    if (const char* msg = lbfgs_check_shape((long long)R * D, 1, E + 2, history, limit)) {
        g->h.err = msg;
        return limit ? GPMPC_ERR_LIMIT : GPMPC_ERR_ARG;
    }
    if (const char* msg = lbfgs_check_step(first_iteration, c1, pgtol)) return bad(g, msg);
    if (iterations < 1) return bad(g, "lbfgs: need iterations >= 1");
    GPMPC_HIP_CHECK(H_(g), hipSetDevice(g->h.device));
    return run_train_search(H_(g), X, Y, N, D, E, R, lo, hi, log_scale, first_iteration, iterations, history, c1, pgtol, x0_dev,
                            state_dev, best_out_dev, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------
// Device-resident iLQR (ilqr.hip).  The one argument-check body of the five entries that take a handle: each names what it needs
// (`ptrs_ok`: its own required pointers; `params`: reg0 / reg_factor / reg_max / tol are its arguments; iterations: 1 where it has none).
struct IlqrParams { double reg0, reg_factor, reg_max, tol; };
static int ilqr_entry_checks(gpmpc_t* g, bool ptrs_ok, int B, int H, int A, int include_time, int L, int iterations,
                             const double* reg0, const IlqrParams* params) {
    if (!g) return GPMPC_ERR_ARG;
    Handle* h = H_(g);
    if (!h->ready) return bad(g, "ilqr before prepare / set_factors");
    if (!ptrs_ok) return bad(g, "null argument");
    bool limit = false;
    if (const char* msg = ilqr_check_shape(B, H, A, L, limit)) {
        h->err = msg;
        return limit ? GPMPC_ERR_LIMIT : GPMPC_ERR_ARG;
    }
    if (h->D + A + (include_time ? 1 : 0) != h->E) return bad(g, "D + A (+1 with time) must equal the model's input dim E");
    if (iterations < 1) return bad(g, "ilqr: need iterations >= 1");
    if (reg0)
        if (const char* msg = ilqr_check_reg0(*reg0)) return bad(g, msg);
    if (params)
        if (const char* msg = ilqr_check_step(params->reg0, params->reg_factor, params->reg_max, params->tol)) return bad(g, msg);
    if (h->cost_D != h->D || h->cost_A != A) return bad(g, "gpmpc_set_cost not called for this (D, A)");
    GPMPC_HIP_CHECK(h, hipSetDevice(h->device));
    return GPMPC_OK;
}

long long gpmpc_ilqr_state_size(int B, int H, int A, int D, int L) {
    bool limit = false;
    if (ilqr_check_shape(B, H, A, L, limit) || D < 1 || D > kMaxD) return -1;
    return (long long)make_ilqr_layout(B, H, A, D, L).total;
}

int gpmpc_ilqr_backward(gpmpc_t* g, const double* actions, const double* mu0, int B, int H, int A, int include_time, double time0,
                        const double* reg_dev, double* gains_out, double* ff_out, double* mu_out, double* info_out, void* stream) {
    Range roctx_range("gpmpc_ilqr_backward");
    int rc = ilqr_entry_checks(g, actions && mu0 && reg_dev && gains_out && ff_out && mu_out && info_out, B, H, A, include_time, 1, 1,
                               nullptr, nullptr);
    if (rc) return rc;
    return run_ilqr_backward(H_(g), actions, mu0, B, H, A, include_time, time0, reg_dev, gains_out, ff_out, mu_out, info_out,
                             (hipStream_t)stream);
}

int gpmpc_ilqr_forward(gpmpc_t* g, const double* actions, const double* gains, const double* ff, const double* mu_nom,
                       const double* mu0, int B, int H, int A, int include_time, double time0, const double* alphas, int L,
                       double* trial_actions_out, double* trial_cost_out, double* trial_mu_out, void* stream) {
    Range roctx_range("gpmpc_ilqr_forward");
    int rc = ilqr_entry_checks(g, actions && gains && ff && mu_nom && mu0 && alphas && trial_actions_out && trial_cost_out, B, H, A,
                               include_time, L, 1, nullptr, nullptr);
    if (rc) return rc;
    return run_ilqr_forward(H_(g), actions, gains, ff, mu_nom, mu0, B, H, A, include_time, time0, alphas, L, trial_actions_out,
                            trial_cost_out, trial_mu_out, (hipStream_t)stream);
}

int gpmpc_ilqr_init(gpmpc_t* g, const double* x0_dev, int B, int H, int A, int L, double reg0, double* state_dev, void* stream) {
    Range roctx_range("gpmpc_ilqr_init");
    int rc = ilqr_entry_checks(g, x0_dev && state_dev, B, H, A, g && H_(g)->E - H_(g)->D - A == 1, L, 1, &reg0, nullptr);
    if (rc) return rc;
    return run_ilqr_init(H_(g), x0_dev, B, H, A, L, reg0, state_dev, (hipStream_t)stream);
}

int gpmpc_ilqr_step(gpmpc_t* g, const double* mu0, int B, int H, int A, int include_time, double time0, int L, double reg0,
                    double reg_factor, double reg_max, double tol, double* state_dev, void* stream) {
    Range roctx_range("gpmpc_ilqr_step");
    const IlqrParams pr{reg0, reg_factor, reg_max, tol};
    int rc = ilqr_entry_checks(g, mu0 && state_dev, B, H, A, include_time, L, 1, nullptr, &pr);
    if (rc) return rc;
    return run_ilqr_step(H_(g), mu0, B, H, A, include_time, time0, L, reg0, reg_factor, reg_max, tol, state_dev, (hipStream_t)stream);
}

int gpmpc_ilqr_search(gpmpc_t* g, const double* mu0, const double* S0, int B, int H, int A, int include_time, double time0,
                      int iterations, int L, double reg0, double reg_factor, double reg_max, double tol, const double* x0_dev,
                      double* state_dev, double* best_out_dev, void* stream) {
    Range roctx_range("gpmpc_ilqr_search");
    const IlqrParams pr{reg0, reg_factor, reg_max, tol};
    int rc = ilqr_entry_checks(g, mu0 && S0 && x0_dev && state_dev, B, H, A, include_time, L, iterations, nullptr, &pr);
    if (rc) return rc;
    // fill_args wants an actions pointer; the search points it at the state's actions afterwards
    RolloutArgs a;
    rc = fill_args(g, a, state_dev, mu0, S0, B, H, A, include_time, time0);
    if (rc) return rc;
    return run_ilqr_search(H_(g), a, iterations, L, reg0, reg_factor, reg_max, tol, x0_dev, state_dev, best_out_dev,
                           (hipStream_t)stream);
}

int gpmpc_rollout_timed(gpmpc_t* g, const double* actions, const double* mu0, const double* S0, int B, int H, int A,
                        int include_time, double time0, double* J_out, int reps, float* ms, void* stream) {
    if (!g || !ms || reps < 1) return GPMPC_ERR_ARG;
    Handle* h = H_(g);
    RolloutArgs a;
    int rc = fill_args(g, a, actions, mu0, S0, B, H, A, include_time, time0);
    if (rc) return rc;
    GPMPC_HIP_CHECK(h, hipSetDevice(h->device));
    a.J_out = J_out;
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t e0, e1;
    GPMPC_HIP_CHECK(h, hipEventCreate(&e0));
    GPMPC_HIP_CHECK(h, hipEventCreate(&e1));
    GPMPC_HIP_CHECK(h, hipEventRecord(e0, s));
    for (int r = 0; r < reps; ++r) {
        rc = launch_rollout(h, a, s);
        if (rc) break;
    }
    GPMPC_HIP_CHECK(h, hipEventRecord(e1, s));
    GPMPC_HIP_CHECK(h, hipEventSynchronize(e1));
    float t = 0.f;
    GPMPC_HIP_CHECK(h, hipEventElapsedTime(&t, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ms = t / (float)reps;
    return rc;
}

int gpmpc_argmin(gpmpc_t* g, const double* J, int B, long long first, double* best_J, long long* best_idx, void* stream) {
    Range roctx_range("gpmpc_argmin");
    if (!g || !J || B < 1 || first < 0) return bad(g, "bad argument");
    Handle* h = H_(g);
    GPMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    int rc = launch_argmin(h, J, B, first, s);
    if (rc) return rc;
    double out[2];
    GPMPC_HIP_CHECK(h, hipMemcpyAsync(out, h->best.p, sizeof out, hipMemcpyDeviceToHost, s));
    GPMPC_HIP_CHECK(h, hipStreamSynchronize(s));
    if (best_J) *best_J = out[0];
    if (best_idx) memcpy(best_idx, &out[1], sizeof(long long));
    return GPMPC_OK;
}

int gpmpc_argmin_async(gpmpc_t* g, const double* J, int B, long long first, const double* actions, int HA, double* out_dev,
                       void* stream) {
    Range roctx_range("gpmpc_argmin_async");
    if (!g || !J || !out_dev || B < 1 || first < 0 || HA < 0) return bad(g, "bad argument");
    Handle* h = H_(g);
    GPMPC_HIP_CHECK(h, hipSetDevice(h->device));
    return launch_argmin_to(h, J, B, first, actions, HA, out_dev, nullptr, (hipStream_t)stream);
}

int gpmpc_argmin_export(gpmpc_t* g, const double* J, int B, long long first, const double* actions, int HA, double* out_dev,
                        double* out_host, void* stream) {
    Range roctx_range("gpmpc_argmin_export");
    if (!g || !J || !out_dev || !out_host || B < 1 || first < 0 || HA < 0) return bad(g, "bad argument");
    Handle* h = H_(g);
    GPMPC_HIP_CHECK(h, hipSetDevice(h->device));
    // out_host must be pinned host memory this device can address: the kernel stores the record there itself
    hipPointerAttribute_t attr;
    void* dev_view = nullptr;
    if (hipPointerGetAttributes(&attr, out_host) != hipSuccess || attr.type != hipMemoryTypeHost ||
        hipHostGetDevicePointer(&dev_view, out_host, 0) != hipSuccess || !dev_view) {
        (void)hipGetLastError();         // the query's own error must not stay behind as the runtime's last error
        return bad(g, "out_host must be pinned (page-locked, device-mapped) host memory");
    }
    return launch_argmin_to(h, J, B, first, actions, HA, out_dev, static_cast<double*>(dev_view), (hipStream_t)stream);
}

// the checks gpmpc_sparse_append and gpmpc_sparse_forget share (`name` heads the messages), then the update itself
static int sparse_update_entry(gpmpc_t* g, const char* name, const double* X, const double* Y, int k, int D, int E, bool forget,
                               void* stream) {
    if (!g) return GPMPC_ERR_ARG;
    Handle* h = H_(g);
    const std::string pre = std::string(name) + ": ";
    if (!h->ready || !h->sp_have) return bad(g, (pre + "the handle holds no record of a gpmpc_prepare_sparse").c_str());
    if (!X || !Y) return bad(g, "null argument");
    if (k < 1) return bad(g, (pre + "need k >= 1 points").c_str());
    if (D != h->D || E != h->E) return bad(g, (pre + "D and E must be those of the cached sparse model").c_str());
    GPMPC_HIP_CHECK(h, hipSetDevice(h->device));
    return run_sparse_update(h, X, Y, k, forget, (hipStream_t)stream);
}

int gpmpc_sparse_append(gpmpc_t* g, const double* Xnew, const double* Ynew, int k, int D, int E, void* stream) {
    Range roctx_range("gpmpc_sparse_append");
    return sparse_update_entry(g, "sparse_append", Xnew, Ynew, k, D, E, false, stream);
}

int gpmpc_sparse_forget(gpmpc_t* g, const double* Xold, const double* Yold, int k, int D, int E, void* stream) {
    Range roctx_range("gpmpc_sparse_forget");
    return sparse_update_entry(g, "sparse_forget", Xold, Yold, k, D, E, true, stream);
}

}  // extern "C"
