/*
 * gpmpc.h -- C ABI of the MI355X-native GP-MPC hot path (libgpmpc_hip.so).
 *
 * The reference (SimonRennotte/Data-Efficient-RL-with-Probabilistic-MPC) has no FFI: its boundary is the duck-typed Python
 * interface AbstractStateTransitionModel (rl_gp_mpc/control_objects/models/abstract_model.py:5-28) plus the candidate loop of
 * GpMpcController._get_optimal_actions (controllers/gp_mpc_controller.py:114-153).  Each entry point names the reference code it
 * replaces.  The Python mirror of those classes (package `..._amd/control_objects/`) calls ONLY these functions for arithmetic;
 * INTEGRATION.md shows the ctypes stub a reference maintainer adds.
 *
 * Conventions: every array is fp64 (the reference forces fp64: config_classes/total_config.py:11), row-major, contiguous;
 * `*_dev` = DEVICE pointers on the handle's GPU, `*_host` = HOST pointers read before the call returns; `stream` = hipStream_t
 * (NULL = default stream), calls are asynchronous on it unless stated; the caller owns all in / out buffers, the handle its
 * workspace; return GPMPC_OK or a negative error, gpmpc_last_error() gives the text; one handle per device, not thread-safe.
 */
#ifndef GPMPC_H
#define GPMPC_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpmpc gpmpc_t;

enum {
    GPMPC_OK = 0,
    GPMPC_ERR_ARG = -1,    /* bad argument / shape / state */
    GPMPC_ERR_NOT_PD = -2, /* Cholesky hit a non-positive pivot (reference: uncaught torch.linalg.cholesky error, gp_model.py:427) */
    GPMPC_ERR_HIP = -3,    /* HIP runtime error */
    GPMPC_ERR_LIMIT = -4   /* shape outside compiled limits (D <= 16, D + A + time <= 24) */
};
#define GPMPC_MAX_D 16
#define GPMPC_MAX_E 24

int gpmpc_abi_version(void);            /* bumped on any signature change */
const char* gpmpc_build_id(void);       /* hash over the library's sources: counter files under profiles/ name their build */
int gpmpc_create(gpmpc_t** out, int device_id);
int gpmpc_destroy(gpmpc_t* h);
const char* gpmpc_last_error(const gpmpc_t* h);

/*
 * gpmpc_prepare  <->  GpStateTransitionModel.prepare_inference + calculate_factorizations (gp_model.py:182-191, 400-431): per
 * output a, K_a = outputscale_a exp(-1/2 sum_e ((x_e - x'_e) / l_ae)^2) (gpytorch ScaleKernel(RBFKernel(ard)), :391, :425),
 * L_a = chol(K_a + noise_a I) (:427), iK_a (:428), beta_a = iK_a y_a (:429-430) and the tables the rollout streams.
 *   X_dev (N,E)  Y_dev (N,D)  lengthscales_dev (D,E)  outputscales_dev (D)  noises_dev (D)
 * Synchronises `stream` (a failed factorisation is reported here: GPMPC_ERR_NOT_PD).  Reuse across control steps (the reference
 * refactorises every step, gp_mpc_controller.py:117): gpmpc_last_prepare_mode = 0 full factorisation, 1 border update (the
 * cached memory plus <= 8 appended points, same hyper-parameters), 2 cache hit, 3 downdate (gpmpc_forget), 4 sparse model
 * (gpmpc_prepare_sparse), 5 points appended to a sparse model (gpmpc_sparse_append), 6 points removed from one
 * (gpmpc_sparse_forget).
 */
int gpmpc_prepare(gpmpc_t* h, const double* X_dev, const double* Y_dev, const double* lengthscales_dev,
                  const double* outputscales_dev, const double* noises_dev, int N, int D, int E, void* stream);
int gpmpc_last_prepare_mode(gpmpc_t* h);

/*
 * gpmpc_forget: the memory points idx_host (k rows of the X / Y of the last gpmpc_prepare) leave the cached model -- the
 * shrinking half of the incremental factorisation (the reference has no counterpart: its memory only grows, gp_memory.py, and
 * is refactorised every step).  Afterwards the handle is in the state gpmpc_prepare would leave for the reduced (X, Y) with the
 * same hyper-parameters: iK, beta, the tables of the rollouts, N, and the record the reuse rules of gpmpc_prepare compare
 * against -- so a following gpmpc_prepare of the reduced memory plus <= 8 appended points is a border update (mode 1, with nothing
 * appended a cache hit), and predict / moments / the rollouts and their gradients run on the reduced model with no further call.
 *   idx_host (k)  rows to remove: strictly ascending, each in [0, N), 1 <= k < N
 * O(k N^2) per GP: iK' = iK[-j,-j] - c c^T / d (c = iK[-j, j], d = iK[j, j]; exactly symmetric), beta' = beta[-j] - c beta_j / d,
 * and L^-1 is downdated to the inverse Cholesky factor of the reduced matrix (positive sums only), rows from the highest down.
 * Removals count toward "refresh_every" together with appended points: past it, or with "incremental" = 0, the reduced memory
 * is factorised in full from the record instead.  gpmpc_last_prepare_mode: 3 downdate, 0 that full factorisation.  Synchronises
 * `stream`; a lost pivot is GPMPC_ERR_NOT_PD, as in gpmpc_prepare.  GPMPC_ERR_ARG, with the cached model untouched: no record of
 * a gpmpc_prepare (no model yet, or gpmpc_set_factors supplied the factors; gpmpc_mll factorises through gpmpc_prepare's path
 * and leaves a record, so rows can be forgotten from its model), idx_host NULL, k < 1, k >= N, an index out of range, unsorted or
 * repeated.  GPMPC_ERR_NOT_PD and GPMPC_ERR_HIP leave no model, as after a failed gpmpc_prepare: prepare again.
 */
int gpmpc_forget(gpmpc_t* h, const int* idx_host, int k, void* stream);

/*
 * gpmpc_prepare_sparse: a sparse GP on M inducing inputs Z in place of the exact one on all N memory points (the reference has
 * no counterpart; PILCO, the method it follows, ships one for the same reason).  DTC / projected-process form (Quinonero-Candela
 * & Rasmussen 2005, section 5; Seeger et al. 2003): it predicts with the formulas of an exact GP whose memory is Z and whose
 * factors are iK_eff (D,M,M), beta_eff (D,M), so every other entry point runs on it unchanged at the cost of an M-point memory.
 *   X_dev (N,E)  Y_dev (N,D)  Z_dev (M,E)  lengthscales_dev (D,E)  outputscales_dev (D)  noises_dev (D)  (as in gpmpc_prepare)
 * Per output a (sigma2_a, n_a: outputscale and noise), in this order of operations:
 *   Kuu = k_a(Z, Z) + jitter_rel sigma2_a I,  Lu = chol(Kuu),  Yu = Lu^-1
 *   V   = Yu k_a(Z, X)                          (M x N: exists one chunk of points at a time)
 *   B   = I + V V^T / n_a,  w = V y_a,  LB = chol(B),  Yb = LB^-1
 *   beta_eff = Yu^T Yb^T Yb w / n_a,   iK_eff = Yu^T (I - Yb^T Yb) Yu    (the bracket first; exactly symmetric)
 * so that the mean is k_a(x, Z) beta_eff and the variance sigma2_a - k_a(x, Z) iK_eff k_a(Z, x), the DTC variance (>= 0 in exact
 * arithmetic, not clamped).  Each point's column is whitened before the rank update: the textbook form Kuu^-1 - (Kuu + Kuf Kfu /
 * n)^-1 loses 5 to 9 more digits of the mean at the same sizes.  Nothing of size N x N or M x N is allocated: the
 * workspace is O(D M^2) plus one chunk of points within 64 MB (option "sparse_chunk_points": 0 auto, else a multiple of 64; every
 * output bit is the same whatever it is, and every sum runs in an order fixed by N, M, D and E alone).  N < M is legal.
 * Afterwards the handle is exactly in the state gpmpc_set_factors(Z, iK_eff, beta_eff, ..., N := M) would leave: no (X, Y) record,
 * so gpmpc_forget answers GPMPC_ERR_ARG and a later gpmpc_prepare is a full factorisation; gpmpc_last_prepare_mode = 4.
 * Synchronises `stream`.  GPMPC_ERR_ARG, with the cached model untouched: a NULL pointer, N < 1, M < 1, jitter_rel negative or not
 * finite; GPMPC_ERR_LIMIT: D or E beyond the compiled limits; GPMPC_ERR_NOT_PD: a lost pivot in either Cholesky -- it leaves no
 * model, as after a failed gpmpc_prepare.
 */
int gpmpc_prepare_sparse(gpmpc_t* h, const double* X_dev, const double* Y_dev, int N, const double* Z_dev, int M,
                         const double* lengthscales_dev, const double* outputscales_dev, const double* noises_dev,
                         double jitter_rel, int D, int E, void* stream);

/*
 * gpmpc_sparse_append: k more memory points join the sparse model cached by the last gpmpc_prepare_sparse, with the same Z,
 * hyper-parameters and jitter, in O(M^2) per point and output -- the growing half of an incremental sparse model (the exact model's
 * is the border update of gpmpc_prepare).  Nothing of size N is touched: with Z fixed a new point is a rank-one change of
 * B = I + V V^T / n_a, and gpmpc_prepare_sparse keeps what follows it as a record: Yu, Yb (D,M,M), w (D,M) and the noises.
 *   Xnew_dev (k,E)  Ynew_dev (k,D)      D, E: those of the cached model
 * Per output a (n = n_a) and per new point (x, y) in ascending row order, in this order of operations:
 *   kz = k_a(Z, x)                                   (differences per element, as in gpmpc_prepare_sparse)
 *   v  = Yu kz          u = v / sqrt(n)              p = Yb u
 *   t_0 = 1,  t_{i+1} = t_i + p_i^2  (i ascending)   tau = t_M  ( = 1 + p^T p )
 *   g  = Yu^T (Yb^T p)                               with the OLD Yb
 *   iK_eff[i,j] += g_i g_j / tau                     (exactly symmetric)
 *   d_i = sqrt(t_{i+1} / t_i),  c_i = p_i / sqrt(t_i t_{i+1})
 *   per column j:  acc = 0;  for i = j .. M-1:  Yb'[i,j] = (Yb[i,j] - p_i acc) / d_i;   acc += c_i Yb'[i,j]
 *   w' = w + v y
 *   beta_eff' = Yu^T Yb'^T Yb' w' / n                (as in gpmpc_prepare_sparse; once per call, after the last point)
 * B' = B + u u^T = LB (I + p p^T) LB^T, and chol(I + p p^T) has the diagonal d_i and the entries p_i c_j below it, so Yb' is the
 * inverse Cholesky factor of B'; B'^-1 = B^-1 - (B^-1 u)(B^-1 u)^T / tau, so the bracket I - Yb^T Yb of iK_eff GROWS by a positive
 * semidefinite rank one.  Nothing is subtracted from a positive quantity and every t_i is a sum of positives >= 1: there is no
 * pivot to lose and no GPMPC_ERR_NOT_PD.  Afterwards the handle is in the state gpmpc_prepare_sparse would leave for the old memory
 * followed by these rows, up to rounding (after 800 appended points the error is still 0.5 to 3 times that of a
 * float64 build from scratch): iK_eff, beta_eff and the tables of the rollouts; no (X, Y) record, N stays M, every other entry
 * point runs on the result unchanged, and the record follows, so calls chain.  gpmpc_last_prepare_mode = 5.  Two plain launches per
 * point and four per call; every sum runs in an order fixed by M, D and E alone, no atomics, no waits between workgroups: two runs
 * give the same bits, and k points in one call give the bits of k calls of one point each.  Asynchronous on `stream`, no host
 * synchronisation inside.  The record is dropped by gpmpc_prepare, gpmpc_set_factors, gpmpc_mll, a failed
 * gpmpc_prepare_sparse and a HIP error in here.  Errors are reported before anything is launched, with the cached model and the
 * record untouched.  GPMPC_ERR_ARG: no record of a gpmpc_prepare_sparse, a NULL pointer, k < 1, D or E different from the model's;
 * GPMPC_ERR_LIMIT: M beyond what a workgroup's LDS holds (about 4000).  GPMPC_ERR_HIP leaves no model, as after a failed prepare.
 */
int gpmpc_sparse_append(gpmpc_t* h, const double* Xnew_dev, const double* Ynew_dev, int k, int D, int E, void* stream);

/*
 * gpmpc_sparse_forget: k memory points leave the sparse model cached by gpmpc_prepare_sparse (and grown by gpmpc_sparse_append),
 * with the same Z, hyper-parameters and jitter, in O(M^2) per point and output -- the shrinking half of an incremental sparse
 * model (the exact model's is gpmpc_forget).  Nothing of size N is touched: removing a point is the rank-one change of
 * B = I + V V^T / n_a that gpmpc_sparse_append makes, with the opposite sign, from the same record (Yu, Yb, w, the noises).
 *   Xold_dev (k,E)  Yold_dev (k,D)      the VALUES of the rows that leave (a sparse model keeps no (X, Y) record, so indices would
 *                                       mean nothing);  D, E: those of the cached model
 * Per output a (n = n_a, sigma2 = sigma2_a) and per removed point (x, y) in ascending row order, in this order of operations:
 *   kz = k_a(Z, x)                                   (differences per element, as in gpmpc_sparse_append)
 *   v  = Yu kz          u = v / sqrt(n)              p = Yb u
 *   t_0 = 1,  t_{i+1} = t_i - p_i^2  (i ascending)   tau = t_M  ( = 1 - p^T p )
 *   LOST PIVOT if some t_{i+1} is not > 0 (NaN included), or tau < 1 / (2 (1 + sigma2 / n))
 *   g  = Yu^T (Yb^T p)                               with the OLD Yb
 *   iK_eff[i,j] -= g_i g_j / tau                     (exactly symmetric)
 *   d_i = sqrt(t_{i+1} / t_i),  c_i = p_i / sqrt(t_i t_{i+1})
 *   per column j:  acc = 0;  for i = j .. M-1:  Yb'[i,j] = (Yb[i,j] + p_i acc) / d_i;   acc += c_i Yb'[i,j]
 *   w' = w - v y
 *   beta_eff' = Yu^T Yb'^T Yb' w' / n                (as in gpmpc_prepare_sparse; once per call, after the last point)
 * B' = B - u u^T = LB (I - p p^T) LB^T, and chol(I - p p^T) has the diagonal d_i and the entries -p_i c_j below it, so Yb' is the
 * inverse Cholesky factor of B'; B'^-1 = B^-1 + (B^-1 u)(B^-1 u)^T / tau.  Unlike the append this subtracts from positive
 * quantities: a pivot can be lost, and digits are lost when most of the data behind an inducing input leaves, so
 * count removals toward a periodic gpmpc_prepare_sparse.  The floor on tau is no tuning knob: for a point that is in the model
 * tau = 1 / (1 + u^T B'^-1 u) >= 1 / (1 + sigma2 / n), since v^T v <= k(x, x) = sigma2; half of that separates rounding from a point
 * that never was in the model.
 * CALLER'S CONTRACT: the call cannot know whether a row really is in the model.  A row that never was either trips the pivot check
 * or silently yields the model of "the memory minus a phantom point".  The call puts no bound on k: removing every point, or more
 * than were ever there, is the caller's error (the model layer enforces k < rows).
 * Afterwards the handle is in the state gpmpc_prepare_sparse would leave for the memory without those rows, up to rounding:
 * iK_eff, beta_eff and the tables of the rollouts; no (X, Y) record, N stays M, every other entry point runs on the result
 * unchanged, and the record follows, so forgets and appends chain in any order.  gpmpc_last_prepare_mode = 6.  Two plain launches
 * per point and four per call; every sum runs in an order fixed by M, D and E alone, no atomics, no waits between workgroups: two
 * runs give the same bits, and k points in one call give the bits of k calls of one point each.  Synchronises `stream` at the
 * end, as gpmpc_forget does, to report a lost pivot.  The record is dropped by gpmpc_prepare, gpmpc_set_factors, gpmpc_mll, a
 * failed gpmpc_prepare_sparse, and GPMPC_ERR_NOT_PD or GPMPC_ERR_HIP in here.
 *   reported before anything is launched, the cached model and the record untouched:
 *     GPMPC_ERR_ARG     no record of a gpmpc_prepare_sparse, a NULL pointer, k < 1, D or E different from the model's
 *     GPMPC_ERR_LIMIT   M beyond what a workgroup's LDS holds (about 4000, as for gpmpc_sparse_append)
 *   reported after the call's launches have completed:
 *     GPMPC_ERR_NOT_PD  a lost pivot: the kernels stop at the first point that loses one (the points before it have left), and the
 *                       call leaves no model and no record, as after a failed prepare; gpmpc_last_error names point and output
 *     GPMPC_ERR_HIP     likewise leaves no model
 */
int gpmpc_sparse_forget(gpmpc_t* h, const double* Xold_dev, const double* Yold_dev, int k, int D, int E, void* stream);

/*
 * gpmpc_select_inducing: chooses the M inducing inputs of gpmpc_prepare_sparse among the N memory points on the device (the
 * reference has no counterpart).  Greedy variance selection (Burt et al. 2019; Fine & Scheinberg 2001): a pivoted partial Cholesky
 * of the D kernel matrices K_a = k_a(X, X), k_a(x, x') = sigma2_a exp(-1/2 sum_e ((x_e - x'_e) / l_ae)^2), run in lockstep over
 * the outputs because gpmpc_prepare_sparse takes one Z for all of them.  There is no Y and no noise: the choice depends on the
 * inputs and the kernel alone.
 *   X_dev (N,E)  lengthscales_dev (D,E)  outputscales_dev (D)
 *   idx_out_dev (M) int, required: the picks, distinct;  Z_out_dev (M,E) or NULL: row m = X[p_m], bit for bit;
 *   trace_out_dev (M) or NULL: trace[m] = sum_i s(i) over all N points after step m's update = sum_a tr(K_a - Q_a) / sigma2_a of
 *   the first m + 1 picks (the trace term of the Titsias bound: it tells a caller when more points stop paying)
 * State: d_a(i) = sigma2_a for every point, L_a (M x N) = 0.  At step m = 0 .. M-1:
 *   score   s(i) = sum_a max(d_a(i), 0) / sigma2_a, a ascending
 *   pick    p_m = the point of largest score among the points not yet picked; the lowest index wins a tie, a score that is not
 *           finite ranks below every finite one (step 0: every score is exactly D, so p_0 = 0 always)
 *   update  per output a, if d_a(p) > jitter_rel sigma2_a:
 *             c(i) = (k_a(x_i, x_p) - sum_{j<m} L_a[j,i] L_a[j,p]) / sqrt(d_a(p)), j ascending;  L_a[m,i] = c(i);  d_a(i) -= c(i)^2
 *           otherwise (the pivot floor gpmpc_prepare_sparse puts on the diagonal of k(Z, Z)) row m of L_a stays zero and d_a is
 *           unchanged: no NaN and no abort.
 * One plain launch per step (a workgroup per 64-point tile, a wavefront per output) and one to write the outputs: the partial
 * trace of a tile is summed in a fixed tree, the tiles in ascending order; every sum runs in an order fixed by N, M, D and E alone,
 * no atomics, no waits between workgroups: two calls give the same bits, and a NULL output changes no bit of the others.  No
 * cached model is needed and none is touched; gpmpc_last_* is not written; the workspace is the call's own: D M N doubles of L plus
 * O(D N + M N / 64), capped at 4 GiB (option "select_inducing_max_mb").  Asynchronous on `stream`, no host synchronisation inside.
 * Errors are reported before anything is launched, the outputs untouched.  GPMPC_ERR_ARG: NULL X / lengthscales / outputscales /
 * idx_out, N < 1, M < 1, M > N, jitter_rel negative or not finite; GPMPC_ERR_LIMIT: D or E beyond the compiled limits, or a
 * workspace beyond the cap (gpmpc_last_error has the size).
 */
int gpmpc_select_inducing(gpmpc_t* h, const double* X_dev, int N, int M, const double* lengthscales_dev,
                          const double* outputscales_dev, double jitter_rel, int D, int E,
                          int* idx_out_dev, double* Z_out_dev, double* trace_out_dev, void* stream);

/* Training objective: per GP -log p(y_a | X, theta_a) / N and its gradient wrt lengthscales, outputscale and
 * noise -- what gpytorch's ExactMarginalLogLikelihood + autograd give the reference's LBFGS loop (gp_model.py:262-275).
 * out_host (D, E + 3) = [loss | d/d lengthscale (E) | d/d outputscale | d/d noise]; synchronous; REPLACES the cached factors. */
int gpmpc_mll(gpmpc_t* h, const double* X_dev, const double* Y_dev, const double* lengthscales_dev,
              const double* outputscales_dev, const double* noises_dev, int N, int D, int E, double* out_host, void* stream);

/* The cached state with iK (D,N,N), beta (D,N) supplied by the caller (test hook; callers that keep their own factorisation);
 * borrowed pointers to / copies of the cached factors  <->  attributes self.iK, self.beta (gp_model.py:187). */
int gpmpc_set_factors(gpmpc_t* h, const double* X_dev, const double* iK_dev, const double* beta_dev,
                      const double* lengthscales_dev, const double* outputscales_dev, int N, int D, int E, void* stream);
int gpmpc_get_factors(gpmpc_t* h, const double** iK_dev, const double** beta_dev);
int gpmpc_read_factors(gpmpc_t* h, double* iK_dst_dev, double* beta_dst_dev, void* stream);

/*
 * gpmpc_predict  <->  the model plot's likelihood(model(x)) on its grid and on the memory points (static_3d_graph.py:77-80, 116):
 * the exact posterior of each zero-mean ScaleKernel(RBFKernel(ard)) GP (gp_model.py:388-397) with the cached factors iK_a, beta_a
 * (:425-430); it is also predict_next_state_change (:112-180) at zero input variance, whose S is then diagonal with these entries.
 *   Xq_dev (M,E)        query inputs in the model-input space of the cached memory (state | action | time when the model has one)
 *   mean_out_dev (M,D)  k_a(x*)^T beta_a
 *   var_out_dev (M,D)   sigma2_a - k_a(x*)^T iK_a k_a(x*)  (+ noises_host[a] when noises_host (D) is non-NULL, as likelihood(...) adds)
 * with k_a(x*)_i = sigma2_a exp(-1/2 sum_e (x*_e - x_ie)^2 / l_ae^2).  The exact posterior, not gpytorch's fast_pred_var (LOVE)
 * approximation the plot enables; the variance is not clamped, as in the reference's formula.  Either output may be NULL; without
 * var_out_dev no matrix product is run (the mean is a GEMV).  A point's results are bitwise the same whatever M is and wherever it
 * sits in the batch.  Asynchronous on `stream`; uses whatever prepare / set_factors / mll cached last; M = 0 launches nothing.
 * GPMPC_ERR_ARG: no cached model, D / E different from the cached model, M < 0.
 */
int gpmpc_predict(gpmpc_t* h, const double* Xq_dev, int M, int D, int E, const double* noises_host, double* mean_out_dev,
                  double* var_out_dev, void* stream);

/*
 * gpmpc_predict_backward  <->  torch autograd through likelihood(model(x)) with respect to x (static_3d_graph.py:77-80, 116): the
 * reverse-mode product (vector-Jacobian product) of gpmpc_predict at the same M query inputs.  For upstream gradients mean_bar,
 * var_bar it returns the gradient of <mean_bar, mean> + <var_bar, var> with respect to Xq:
 *   c_amj = mean_bar_ma beta_aj - 2 var_bar_ma P_amj   (P_a = K*_a iK_a, k_amj = k_a(x*_m)_j as in gpmpc_predict)
 *   Xq_bar_me = sum_a (1 / l_ae^2) sum_j c_amj k_amj (x_je - x*_me)
 *   Xq_dev (M,E)          query inputs, as in gpmpc_predict
 *   mean_bar_dev (M,D)    upstream gradient of the mean, or NULL (= 0)
 *   var_bar_dev (M,D)     upstream gradient of the variance, or NULL (= 0): then no matrix product is run (O(N E D) per query);
 *                         with both NULL the call writes zeros and launches no tile kernel
 *   Xq_bar_out_dev (M,E)  required; overwritten, not accumulated into
 * The likelihood noise gpmpc_predict may add is a constant: it has no gradient, and this entry takes none.  2 K* iK is the
 * gradient of k^T iK k only for a symmetric iK: prepare and mll store iK exactly symmetric; a non-symmetric iK passed through
 * gpmpc_set_factors gets 2 K* iK, not K* (iK + iK^T).  Uses whatever prepare / set_factors / mll cached last.  A point's gradient
 * is bitwise the same whatever M is, wherever it sits in the batch, whatever its neighbours are and however the call chunks the
 * rows internally (workspace within 4 MB, or one 64-row tile's need if that is more: 2.6 MB at N = 4096, D = 16, E = 20); a NULL
 * upstream and an all-zero one give the same bits.  Touches no other workspace and no gpmpc_last_* state.  Asynchronous on
 * `stream`; M = 0 launches nothing.  GPMPC_ERR_ARG: no cached model, D / E different from the cached model, M < 0, Xq_dev or
 * Xq_bar_out_dev NULL with M > 0.
 */
int gpmpc_predict_backward(gpmpc_t* h, const double* Xq_dev, int M, int D, int E, const double* mean_bar_dev,
                           const double* var_bar_dev, double* Xq_bar_out_dev, void* stream);

/*
 * gpmpc_predict_cov  <->  likelihood(model(x)).covariance_matrix (static_3d_graph.py:77-80, gp_model.py:394-397): the joint
 * posterior covariance between query points, of which gpmpc_predict's variance is the diagonal -- what posterior function
 * samples, joint confidence regions and the variance of a linear functional of the prediction need.  For every output a of the
 * cached model, with k_a(x) as in gpmpc_predict,
 *   t_a(x, x') = sigma2_a exp(-1/2 sum_e (x_e - x'_e)^2 / l_ae^2)  -  k_a(x)^T iK_a k_a(x')
 *   Xa_dev (Ma,E), Xb_dev (Mb,E)  query inputs in the model-input space of the cached memory
 *   cov_out_dev (D,Ma,Mb)         required; overwritten
 * Cross form (Xb_dev non-NULL): cov[a,i,j] = t_a(xa_i, xb_j); noises_host must be NULL (two different sets share no likelihood
 * noise).  Joint form (Xb_dev NULL, Mb ignored, output (D,Ma,Ma)): cov[a,i,j] = 1/2 (t_a(x_i, x_j) + t_a(x_j, x_i)), exactly
 * symmetric (cov[a,i,j] and cov[a,j,i] are the same bits), plus noises_host[a] on the diagonal when noises_host (D) is non-NULL, as
 * likelihood(...) adds.  Not clamped and no jitter added: the caller decides how to regularise before factorising it.  The exact
 * posterior, not gpytorch's LOVE approximation.  iK is used as given: prepare and mll store it exactly symmetric; with a
 * non-symmetric iK passed through gpmpc_set_factors the joint form still returns the symmetric average above, the posterior
 * covariance of the symmetric part of iK.  An element's bits depend only on the two points it belongs to (cross form: the ordered
 * pair; joint form: the unordered pair) -- not on Ma / Mb, on where the points sit, on their neighbours or on how the call chunks
 * the rows internally; every sum runs in an order fixed by N alone, no atomics.  The diagonal agrees with gpmpc_predict's variance
 * to rounding, not bit for bit (the sums are grouped differently).  Workspace of its own: P = K*_a(Xa) iK_a for a chunk of rows,
 * within 256 MB, or one 64-row tile's need if that is more (32 MB at N = 4096, D = 16, which gives chunks of 512 rows), whatever
 * Ma and Mb are.  Touches no other workspace and no gpmpc_last_* state.  Asynchronous on `stream`; Ma = 0 (or Mb = 0 in the cross
 * form) launches nothing.  GPMPC_ERR_ARG: no cached model, D / E different from the cached model, a negative count or one beyond
 * 2^22, Xa_dev or cov_out_dev NULL with work to do, noises_host with the cross form.
 */
int gpmpc_predict_cov(gpmpc_t* h, const double* Xa_dev, int Ma, const double* Xb_dev, int Mb, int D, int E,
                      const double* noises_host, double* cov_out_dev, void* stream);

/*
 * gpmpc_moments  <->  predict_next_state_change(input_mu, input_var) (gp_model.py:112-180) at P independent Gaussian model inputs
 * N(m_p, Sigma_p): the moment-matched one-step prediction of the state change, with a general symmetric E x E Sigma_p (any block
 * may be non-zero: state, action and time inputs alike; the rollouts only ever pass a state-block one).
 *   mu_dev (P,E)       input means, in the model-input space of the cached memory (state | action | time when the model has one)
 *   var_dev (P,E,E)    input covariances, or NULL for all zero
 *   M_out_dev (P,D)    mean state change (the reference's M.t())
 *   S_out_dev (P,D,D)  its covariance (S), or NULL: then the pairwise pass is not run at all
 *   V_out_dev (P,E,D)  Sigma^-1 Cov[x, delta] = dM/dm (V.t()), or NULL
 * Reads the factors cached by the last prepare / set_factors / mll (X, lengthscales, outputscales, iK, beta).  Sigma is used as
 * given: it is assumed symmetric positive semi-definite, and is not checked -- a Sigma that is not gives NaN, as in the reference.
 * A point's M, S and V are bitwise the same whatever P is, wherever the point sits in the batch, whatever its neighbours are and
 * however the call chunks the batch internally; M and V keep their bits when S_out / V_out are NULL.  The points are processed in
 * chunks whose workspace stays within 32 MB (or one point's need if that is more: 18 MB at N = 4096, D = 16, E = 20), whatever
 * P is.  Touches no rollout / gradient workspace and no gpmpc_last_* state.  Asynchronous on `stream`; P = 0 launches nothing.
 * GPMPC_ERR_ARG: no cached model, D / E different from the cached model, P < 0.  GPMPC_ERR_LIMIT: D > GPMPC_MAX_D or
 * E > GPMPC_MAX_E.
 */
int gpmpc_moments(gpmpc_t* h, const double* mu_dev, const double* var_dev, int P, int D, int E, double* M_out_dev,
                  double* S_out_dev, double* V_out_dev, void* stream);

/*
 * gpmpc_moments_backward  <->  torch autograd through predict_next_state_change (gp_model.py:112-180): the reverse-mode product
 * (vector-Jacobian product) of gpmpc_moments at the same P inputs.  For upstream gradients M_bar, S_bar, V_bar it returns the
 * gradients of <M_bar, M> + <S_bar, S> + <V_bar, V> with respect to the input mean and the input covariance.
 *   mu_dev, var_dev    as in gpmpc_moments (var_dev NULL = all-zero covariances; the gradient at Sigma = 0 is still returned)
 *   M_bar_dev (P,D)    upstream gradient of M, or NULL (= 0)
 *   S_bar_dev (P,D,D)  upstream gradient of S, or NULL (= 0): then the pairwise pass is not run at all (O(N) per point)
 *   V_bar_dev (P,E,D)  upstream gradient of V (the layout of V_out), or NULL (= 0)
 *   mu_bar_out_dev (P,E)      d/d mu, or NULL (not written)
 *   var_bar_out_dev (P,E,E)   d/d Sigma, its symmetric part, or NULL (not written)
 * Outputs are overwritten, not accumulated into.  Sigma's gradient is the symmetric part sym(G) = (G + G^T) / 2: the reference's
 * formula is not symmetric in Sigma away from symmetric matrices, so autograd's raw G is not symmetric, but <G, dSigma> =
 * <sym(G), dSigma> for every symmetric dSigma; a caller that parametrises Sigma = A A^T gets 2 sym(G) A either way.  Hyper-
 * parameters and the memory get no gradient.  A point's results are bitwise the same whatever P is, wherever the point sits,
 * whatever its neighbours are and however the batch is chunked; the chunks' workspace stays within 32 MB (or one point's need if
 * that is more: 29 MB at N = 4096, D = 16, E = 20).  Touches no rollout / gradient / gpmpc_moments workspace and no gpmpc_last_*
 * state.  Asynchronous on `stream`; P = 0 launches nothing.  Errors as gpmpc_moments (GPMPC_ERR_ARG also for mu_dev NULL with
 * P > 0).
 */
int gpmpc_moments_backward(gpmpc_t* h, const double* mu_dev, const double* var_dev, int P, int D, int E, const double* M_bar_dev,
                           const double* S_bar_dev, const double* V_bar_dev, double* mu_bar_out_dev, double* var_bar_out_dev,
                           void* stream);

/*
 * gpmpc_moments_linear: the first-order (Taylor) propagation of Girard et al. / Hewing et al. ("Cautious MPC using GP regression")
 * at P independent Gaussian model inputs N(m_p, Sigma_p), with the arguments of gpmpc_moments and the same cached factors: the
 * posterior is evaluated at the input mean and the input covariance goes through the Jacobian of the posterior mean.  Per point
 * and output a, with k_aj = sigma2_a exp(-1/2 sum_e (m_e - x_je)^2 / l_ae^2) as in gpmpc_predict:
 *   M_a    = sum_j k_aj beta_aj
 *   V[e,a] = (1 / l_ae^2) sum_j beta_aj k_aj (x_je - m_e)     = dM_a / dm_e  (differences formed per element)
 *   v_a    = sigma2_a - k_a^T iK_a k_a                         (not clamped, no noise added)
 *   S      = V^T Sigma V + diag(v)
 *   mu_dev (P,E), var_dev (P,E,E) or NULL (= 0); M_out_dev (P,D), S_out_dev (P,D,D), V_out_dev (P,E,D), each may be NULL
 * It is a different approximation from moment matching, not a faster evaluation of it: it drops the 1/2 tr(H Sigma) term of the
 * mean and the curvature terms of S; the two agree to first order in Sigma and coincide at Sigma = 0 (M, V and the then diagonal
 * S, to rounding).  It costs one K* iK product per output, O(N^2 D) per point, and no O(N^2 D^2) pair pass.  Without S_out_dev no
 * matrix product runs at all: M and the whole mean Jacobian V come from one O(N E D) pass.  Sigma is used as given and not
 * checked.  S is exactly symmetric (S[a,b] and S[b,a] are the same bits) and exactly diagonal with var_dev NULL.  A point's M, S
 * and V are bitwise the same whatever P is, wherever the point sits in the batch, whatever its neighbours are and however the call
 * chunks the batch internally; M and V keep their bits when S_out / V_out are NULL.  Every sum runs in an order fixed by N, E and
 * D alone; no atomics.  M, V and diag S agree with gpmpc_predict / gpmpc_predict_backward / gpmpc_moments (var NULL) to rounding,
 * not bit for bit.  Workspace of its own: partial sums of one chunk of points, within 16 MB (or one 64-row tile's need if that is
 * more).  Touches no other workspace and no gpmpc_last_* state.  Asynchronous on `stream`; P = 0 launches nothing.
 * GPMPC_ERR_ARG: no cached model, D / E different from the cached model, P < 0, mu_dev NULL with P > 0.  GPMPC_ERR_LIMIT:
 * D > GPMPC_MAX_D or E > GPMPC_MAX_E.
 */
int gpmpc_moments_linear(gpmpc_t* h, const double* mu_dev, const double* var_dev, int P, int D, int E, double* M_out_dev,
                         double* S_out_dev, double* V_out_dev, void* stream);

/*
 * gpmpc_moments_linear_backward: the reverse-mode product (vector-Jacobian product) of gpmpc_moments_linear at the same P inputs
 * -- what torch autograd gives through the formulas of gpmpc_moments_linear.  For upstream gradients M_bar, S_bar, V_bar it
 * returns the gradients of <M_bar, M> + <S_bar, S> + <V_bar, V> with respect to the input mean m and the input covariance Sigma.
 * Arguments, layouts and NULL rules are those of gpmpc_moments_backward:
 *   mu_dev (P,E), var_dev (P,E,E) or NULL (= 0; the gradient at Sigma = 0 is still returned)
 *   M_bar_dev (P,D), S_bar_dev (P,D,D), V_bar_dev (P,E,D)   upstream gradients, each NULL (= 0)
 *   mu_bar_out_dev (P,E), var_bar_out_dev (P,E,E)           each NULL (not written); overwritten, not accumulated into
 * With d_je = x_je - m_e (formed per element, as the forward does), r_aje = d_je / l_ae^2, k_aj as in gpmpc_moments_linear and
 * q_a = iK_a k_a (a row of K* iK):
 *   var_bar  = sym(V S_bar V^T)                       (E x E, exactly symmetric; the symmetric part, by the rule of
 *                                                      gpmpc_moments_backward)
 *   W        = V_bar + Sigma V (S_bar + S_bar^T)      (E x D)
 *   s_a      = S_bar[a,a],   u_aj = sum_e W[e,a] r_aje,   c_aj = beta_aj (M_bar_a + u_aj) - 2 s_a q_aj
 *   mu_bar_g = sum_a [ sum_j c_aj k_aj r_ajg  -  W[g,a] M_a / l_ag^2 ]
 * (dM_a/dm_g = V[g,a]; dV[e,a]/dm_g = sum_j beta k r_e r_g - delta_eg M_a / l_ae^2; dv_a/dm_g = -2 sum_j q_aj k_aj r_ajg).  Sigma
 * is taken as symmetric in W.  iK is treated as symmetric, with the caveat of gpmpc_predict_backward: a non-symmetric iK passed
 * through gpmpc_set_factors gets 2 K* iK, not K* (iK + iK^T).  Hyper-parameters and the memory get no gradient.  W depends on
 * the forward's V: the call runs the forward's M / V pass (O(N E D) per point, no matrix product), then one tile launch whose k
 * loop forms q on the matrix cores and whose epilogue contracts c k r.  With S_bar_dev NULL no matrix product runs at all; with
 * all three upstream gradients NULL the outputs are zeros and no kernel of the model runs.  A point's results are bitwise the
 * same whatever P is, wherever the point sits, whatever its neighbours are and however the batch is chunked
 * ("moments_linear_backward_chunk_points"); a NULL upstream and an all-zero one give the same bits.  Every sum runs in an order
 * fixed by N, E and D alone; no atomics.  Workspace of its own, within 16 MB (or one 64-row tile's need if that is more).  Touches
 * no other workspace and no gpmpc_last_* state.  Asynchronous on `stream`; P = 0 launches nothing.  Errors as
 * gpmpc_moments_backward: GPMPC_ERR_ARG for no cached model, D / E different from the cached model, P < 0, mu_dev NULL with
 * P > 0; GPMPC_ERR_LIMIT for D > GPMPC_MAX_D or E > GPMPC_MAX_E.
 */
int gpmpc_moments_linear_backward(gpmpc_t* h, const double* mu_dev, const double* var_dev, int P, int D, int E,
                                  const double* M_bar_dev, const double* S_bar_dev, const double* V_bar_dev,
                                  double* mu_bar_out_dev, double* var_bar_out_dev, void* stream);

/*
 * Options.  Behaviour: "incremental" (0/1, default 1: reuse / border-update the cached factors), "refresh_every" (32: border
 * updates between full factorisations), "cluster" (few-candidate cooperative form: 0 auto, 1 never, 2..32 workgroups per
 * candidate), "threads" (fused-horizon workgroup: 0 auto, 256 / 512 / 1024), "pair_tiles" (batch-major rollout path: 0 auto,
 * 1 always, 2 never).  Dispatch hooks of the parity tests: "rows_per_chunk", "cols_per_lane", "force_path" (1 direct exp,
 * 2 element-wise Taylor), "force_separable", "force_global_scratch", "grad_separable" / "grad_tiles" / "grad_stream" /
 * "grad_mean" / "grad_share_cu" / "grad_chunk_rows", "fused_prepare", "outer_min_n", "predict_chunk_rows" (gpmpc_predict's
 * query rows per internal chunk: 0 auto, else a multiple of 64), "predict_backward_chunk_rows" (the same for
 * gpmpc_predict_backward), "predict_cov_chunk_rows" (the same for gpmpc_predict_cov's rows of Xa),"moments_chunk_points" (gpmpc_moments' points per internal
 * chunk: 0 auto), "moments_backward_chunk_points" (the same for gpmpc_moments_backward),
 * "moments_linear_chunk_points" (points of gpmpc_moments_linear / candidates of gpmpc_rollout_linear per internal chunk: 0 auto),
 * "moments_linear_backward_chunk_points" (the same for gpmpc_moments_linear_backward / gpmpc_rollout_linear_backward /
 * gpmpc_rollout_linear_feedback_backward), "rollout_feedback_chunk_points" (candidates of gpmpc_rollout_feedback per internal
 * chunk: 0 auto), "rollout_feedback_backward_chunk_points" (the same for gpmpc_rollout_feedback_backward), "lqr_gains_chunk_points" (candidates of gpmpc_lqr_gains per internal chunk: 0 auto),
 * "ilqr_chunk_points" (candidates of gpmpc_ilqr_* per internal chunk: 0 auto),
 * "sparse_chunk_points" (memory points of gpmpc_prepare_sparse per internal chunk: 0 auto, else a multiple of 64),
 * "select_inducing_max_mb" (cap on the workspace of gpmpc_select_inducing in MiB, >= 1; 4096 unless set).
 * Measurement (A/B) switches of single
 * kernels are listed with their measurements in csrc/gpmpc_internal.h (struct Handle, opt_*).  Unknown names: GPMPC_ERR_ARG.
 */
int gpmpc_set_option(gpmpc_t* h, const char* name, long long value);

/* Quadratic cost of SetpointStateRewardMapper (setpoint_distance_reward_mapper.py:12-68, 124-142) and the LCB settings of
 * compute_mean_lcb_trajectory (gp_mpc_controller.py:270-276): target_host (D+A), W_host (D+A,D+A), W_T_host (D,D),
 * kappa = exploration_factor, clip_to_zero = clip_lower_bound_cost_to_0, state_min/max_host (D) or NULL = use_constraints False. */
int gpmpc_set_cost(gpmpc_t* h, const double* target_host, const double* W_host, const double* W_T_host, double kappa,
                   int clip_to_zero, const double* state_min_host, const double* state_max_host, int D, int A);

/*
 * gpmpc_rollout  <->  B x [ predict_trajectory (gp_model.py:60-110, H calls of predict_next_state_change :112-180) +
 * get_rewards_trajectory (setpoint_distance_reward_mapper.py:144-149) + the value of compute_mean_lcb_trajectory
 * (gp_mpc_controller.py:267-276) ], all H steps inside one launch.
 *   actions_dev (B,H,A) model-space actions in [0,1];  mu0_host (D), S0_host (D,D): initial state (same for all candidates);
 *   include_time / time0: ModelConfig.include_time_model, current_time_idx (gp_model.py:101-102)
 * Outputs (each nullable): mu_out_dev (B,H+1,D), Sig_out_dev (B,H+1,D,D) (index 0 = input state, :91-92), cost_mu_out_dev
 * (B,H+1) = -rewards, cost_var_out_dev (B,H+1), J_out_dev (B) = the objective the optimiser / argmin sees.  The cost outputs need
 * gpmpc_set_cost for this (D, A); with all three NULL the call is the plain predict_trajectory.
 * gpmpc_last_rollout_path: 0 = fused-horizon kernel (a workgroup per candidate), 1 = streaming kernel (per-point arrays beyond the
 * LDS), 2 = batch-major path (per step: workgroups own 128 x 128 tiles of beta beta^T - iK and loop over candidates; D <= 4, tables
 * beyond an XCD's L2, B >= 2 x CUs).  gpmpc_last_cluster: workgroups per candidate of the last fused-horizon launch; > 1 = the
 * few-candidate cooperative form -- the reference evaluates ONE sequence per objective call (restarts_optim 1-2,
 * gp_mpc_controller.py:125-141), so while candidates x cluster fit the chip a cluster of workgroups shares each candidate's
 * horizon step (bit-identical to one workgroup per candidate at equal "rows_per_chunk").  gpmpc_last_pair_groups: groups of output
 * pairs the last fused-horizon or batch-major launch walked per horizon step (1 = the records of all pairs fit the LDS together;
 * more under a small "lds_limit_kb"); 1 for the streaming kernel.
 */
int gpmpc_rollout(gpmpc_t* h, const double* actions_dev, const double* mu0_host, const double* S0_host, int B, int H, int A,
                  int include_time, double time0, double* mu_out_dev, double* Sig_out_dev, double* cost_mu_out_dev,
                  double* cost_var_out_dev, double* J_out_dev, void* stream);
int gpmpc_last_rollout_path(gpmpc_t* h);
int gpmpc_last_cluster(gpmpc_t* h);
int gpmpc_last_pair_groups(gpmpc_t* h);

/*
 * gpmpc_rollout_linear: gpmpc_rollout -- the same arguments and outputs -- with the step of gpmpc_moments_linear in place of
 * predict_next_state_change in the recurrence of predict_trajectory (gp_model.py:95-108).  The model input of step t is
 * [mu_t | action_t | time0 + t], its covariance non-zero in the state block only; with V_s the first D rows of V,
 *   mu_{t+1} = mu_t + M,   T = Sigma_t V_s,   Sigma_{t+1} = Sigma_t + (V_s^T Sigma_t V_s + diag v) + T + T^T
 * Index 0 of the outputs is the input state; Sigma_t (t >= 1) is exactly symmetric.  Stage costs, terminal cost and J come from
 * the trajectory cost kernel gpmpc_rollout uses, on the stored trajectory with the loaded gpmpc_set_cost settings: constraints,
 * clipping and kappa behave as there.  The cost outputs need gpmpc_set_cost for this (D, A); with all three NULL the call is the
 * plain trajectory.  Batch-major: per horizon step one tile launch over all candidates of a chunk and one small finish launch
 * (there is no fused-horizon form: with few candidates a 64-row tile is mostly padding).  A candidate's results are bitwise the
 * same alone and at any position of any batch, whatever "moments_linear_chunk_points" is.  Workspace of its own (the partial
 * sums and model inputs of one chunk of candidates, and their trajectory where the caller keeps none; a chunk runs its whole
 * horizon), within 16 MB or one 64-row tile's need.  Touches no other workspace and no gpmpc_last_* state.  Asynchronous on
 * `stream`.  Argument errors as gpmpc_rollout (GPMPC_ERR_ARG: no cached model, NULL actions / mu0 / S0, B < 1, H < 1, A < 0,
 * D + A (+1) != E, cost outputs without gpmpc_set_cost for this (D, A)).
 */
int gpmpc_rollout_linear(gpmpc_t* h, const double* actions_dev, const double* mu0_host, const double* S0_host, int B, int H, int A,
                         int include_time, double time0, double* mu_out_dev, double* Sig_out_dev, double* cost_mu_out_dev,
                         double* cost_var_out_dev, double* J_out_dev, void* stream);

/*
 * gpmpc_rollout_linear_feedback: gpmpc_rollout_linear in closed loop, under the ancillary linear feedback of cautious GP-MPC
 *   u = ubar_t + K_t (x - mu_t),  x ~ N(mu_t, Sigma_t),  ubar = actions_dev,  K_t (A, D) in model space.
 * gains_dev is (B,H,A,D) when gains_per_candidate != 0, else (H,A,D) shared by all candidates.  The gains never move the mean:
 * the model input mean of step t is [mu_t | ubar_t | time0 + t], and mu_out is bit for bit gpmpc_rollout_linear's for the same
 * actions, whatever the gains are.  The model input covariance is G_t Sigma_t G_t^T with G_t = [I_D ; K_t ; 0] (E x D, the time
 * row zero); with M, V, v of gpmpc_moments_linear at that mean, V_s / V_u the state / action rows of V,
 *   C_t = G_t^T V = V_s + K_t^T V_u,   T = Sigma_t C_t,
 *   mu_{t+1} = mu_t + M,   Sigma_{t+1} = Sigma_t + (C_t^T Sigma_t C_t + diag v) + T + T^T
 * computed for a <= b and mirrored: Sigma_t (t >= 1) is exactly symmetric.  Stage costs (t < H): the quadratic cost with the full
 * state-action covariance Sigma_z = [I ; K_t] Sigma_t [I ; K_t]^T in place of block_diag(Sigma_t, 0),
 *   cost_mu = tr(Sigma_z W) + e^T W e,   cost_var = tr(2 (W Sigma_z)^2) + 4 e^T W Sigma_z W e,   e = [mu_t | ubar_t] - target;
 * the constraint term (state marginals only), the terminal cost, kappa, clipping and J are those of gpmpc_rollout_linear.
 * NOT modelled: the realised action u is not clipped to [0, 1] -- this is a linearisation, and the covariance it propagates is
 * that of the unclipped policy.
 * gains_dev == NULL: the call IS gpmpc_rollout_linear (every output has the same bits).  Outputs, their nullability, the cost
 * rules and the asynchrony are gpmpc_rollout_linear's; so are the workspace (its own, within 16 MB or one 64-row tile's need; no
 * other workspace and no gpmpc_last_* state is touched) and the option "moments_linear_chunk_points".  A candidate's results
 * are bitwise the same alone and at any position of any batch, whatever the chunk size is, and whether its gains arrive shared
 * or per candidate.  Every sum runs in an order fixed by N, E, D and A alone; no atomics.  Errors: those of
 * gpmpc_rollout_linear, plus GPMPC_ERR_ARG for a non-NULL gains_dev with A < 1.
 */
int gpmpc_rollout_linear_feedback(gpmpc_t* h, const double* actions_dev, const double* gains_dev, int gains_per_candidate,
                                  const double* mu0_host, const double* S0_host, int B, int H, int A, int include_time,
                                  double time0, double* mu_out_dev, double* Sig_out_dev, double* cost_mu_out_dev,
                                  double* cost_var_out_dev, double* J_out_dev, void* stream);

/*
 * gpmpc_rollout_feedback: gpmpc_rollout -- moment matching, the reference's own propagation -- in closed loop under the policy of
 * gpmpc_rollout_linear_feedback,
 *   u = ubar_t + K_t (x - mu_t),  x ~ N(mu_t, Sigma_t),  ubar = actions_dev,  K_t (A, D) in model space.
 * Arguments, layouts, output nullability and asynchrony are those of gpmpc_rollout_linear_feedback: gains_dev is (B,H,A,D) when
 * gains_per_candidate != 0, else (H,A,D) shared by all candidates.  Per step t, with G_t = [I_D ; K_t ; 0] (E x D, the time row
 * zero): the model input mean is [mu_t | ubar_t | time0 + t], the model input covariance Sigma_in = G_t Sigma_t G_t^T, formed by
 * blocks (Sigma_t, K_t Sigma_t, its transpose, K_t Sigma_t K_t^T) for i <= j and mirrored -- exactly symmetric, the time row and
 * column exactly zero.  With M, S, V of gpmpc_moments (its kernels) at that input,
 *   C = (first D rows of Sigma_in) V = Sigma_t (V_s + K_t^T V_u),
 *   mu_{t+1} = mu_t + M,   Sigma_{t+1} = Sigma_t + S + C + C^T
 * computed for a <= b and mirrored: Sigma_t (t >= 1) is exactly symmetric; index 0 of the outputs is the input state.  This is the
 * recurrence of predict_trajectory (gp_model.py:95-108) fed the policy's full input covariance.  UNLIKE the linearised form, the
 * gains DO move the mean: M depends on Sigma_in, so mu_out differs from gpmpc_rollout's for the same actions.  Sigma_in has rank D
 * in E dimensions, which is harmless: only I + Lambda Sigma_in forms are factorised, never Sigma_in itself.
 * Stage costs (t < H): the quadratic cost with the full state-action covariance [I ; K_t] Sigma_t [I ; K_t]^T; the constraint term
 * (state marginals only), the terminal cost, kappa, clipping and J are those of gpmpc_rollout_linear_feedback (the same cost
 * kernel, on the stored trajectory).  The cost outputs need gpmpc_set_cost for this (D, A); with all three NULL the call is the
 * plain trajectory.  NOT modelled, as there: the realised action u is not clipped to [0, 1].
 * gains_dev == NULL: the all-zero-gain policy through these same kernels (bit for bit the call with a zero gain array).  It equals
 * gpmpc_rollout to rounding, NOT bit for bit: the moments come from gpmpc_moments' kernels, the costs from the closed-loop kernel.
 * Batch-major, per chunk of candidates: one init launch; per horizon step the setup / point / pair / finish launches of
 * gpmpc_moments over the chunk and one step launch (five launches a step); the cost launch.  There is no fused-horizon form.
 * Workspace of its own (a chunk's model input means and covariances, M, S, V, the trajectory where the caller keeps none, and the
 * zero gains of a call without gains), within 16 MB or one candidate's need: option "rollout_feedback_chunk_points" (candidates
 * per chunk, 0 auto).  The call ALSO uses gpmpc_moments' workspace and honours "moments_chunk_points".  It touches no other
 * workspace and no gpmpc_last_* state.  A candidate's results are bitwise the same alone, at any position of any batch, for any
 * value of "rollout_feedback_chunk_points" or "moments_chunk_points", and whether its gains arrive shared or per candidate.
 * Every sum runs in an order fixed by N, E, D and A alone; no atomics.  Reads only the cached factors, so it works unchanged on a
 * model from gpmpc_prepare_sparse / gpmpc_set_factors.
 * Errors (no output is written): GPMPC_ERR_ARG for no cached model, NULL actions / mu0 / S0, B < 1, H < 1, A < 0,
 * D + A (+1) != E, cost outputs without gpmpc_set_cost for this (D, A), a non-NULL gains_dev with A < 1; GPMPC_ERR_LIMIT for
 * D > GPMPC_MAX_D or E > GPMPC_MAX_E.
 */
int gpmpc_rollout_feedback(gpmpc_t* h, const double* actions_dev, const double* gains_dev, int gains_per_candidate,
                           const double* mu0_host, const double* S0_host, int B, int H, int A, int include_time, double time0,
                           double* mu_out_dev, double* Sig_out_dev, double* cost_mu_out_dev, double* cost_var_out_dev,
                           double* J_out_dev, void* stream);

/*
 * gpmpc_lqr_gains: the feedback gains gpmpc_rollout_linear_feedback takes as given -- per candidate, the finite-horizon LQR gains
 * of the linearisation along its nominal (mean) trajectory on the loaded quadratic cost, as cautious GP-MPC chooses its ancillary
 * controller.  Inputs as gpmpc_rollout_linear (actions_dev (B,H,A) = ubar, mu0_host (D), include_time / time0); there is no S0:
 * NO covariance enters, and no K* iK product runs.
 * Nominal trajectory: the model input of step t is [mu_t | ubar_t | time0 + t], mu_0 = mu0, mu_{t+1} = mu_t + M, with M and the
 * mean Jacobian V (E x D, V[e,a] = dM_a / dm_e) of gpmpc_moments_linear at that input: mu_t is bit for bit
 * gpmpc_rollout_linear's.  The time row of V is ignored.  With V_s / V_u the state / action rows of V,
 *   A_t = I_D + V_s^T (D x D),   B_t = V_u^T (D x A):   delta x_{t+1} = A_t delta x_t + B_t delta u_t.
 * Cost: the block loaded by gpmpc_set_cost for this (D, A): W_s = (W + W^T) / 2, Q = W_s[:D,:D], N = W_s[:D,D:], R = W_s[D:,D:],
 * P_H = (W_T + W_T^T) / 2.  Target, kappa, clipping and the state constraints do not enter: linear terms and the LCB do not
 * change the optimal deviation gain.  The gain is CERTAINTY-EQUIVALENT: it is designed on the mean dynamics alone, and the
 * variance term of the LCB is not part of the design.  NOT modelled, as in gpmpc_rollout_linear_feedback: the action box [0, 1]
 * (the realised action is not clipped).
 * Riccati sweep, for t = H-1 .. 0:
 *   F = P_{t+1} A_t,   Huu = R + B_t^T P_{t+1} B_t + reg I (A x A, formed for i <= j and mirrored),   Hux = N^T + B_t^T F (A x D),
 *   Huu = L L^T (Cholesky),   K_t = -Huu^-1 Hux (A x D),   P_t = Q + A_t^T F + Hux^T K_t (formed for i <= j and mirrored: exactly
 *   symmetric).
 * A pivot of the factorisation that is <= 0 or not finite does not abort the call and produces no NaN: that step gets K_t = 0 and
 * P_t = Q + A_t^T F (for i <= j, mirrored), and the candidate's flag counts such steps (0: a clean sweep).
 * Outputs: gains_out_dev (B,H,A,D), required -- K_t [action][state] with the sign and layout gpmpc_rollout_linear_feedback expects
 * for gains_per_candidate != 0 (u = ubar_t + K_t (x - mu_t)); P_out_dev (B,H+1,D,D) the cost-to-go matrices (index H = P_H), or
 * NULL; flags_out_dev (B) ints, or NULL.  A NULL P_out_dev / flags_out_dev does not change the gains' bits.
 * Per step one launch that writes the chunk's model inputs and the no-matrix-product form of gpmpc_moments_linear (its kernels and
 * workspace, unchanged); after the H steps one launch with a wavefront per candidate runs the sweep.  Plain kernels: no atomics, no
 * waits between workgroups; every sum runs in an order fixed by N, E, D and A alone.  A candidate's gains, P and flag are bitwise
 * the same alone, at any position of any batch, and whatever "lqr_gains_chunk_points" (and "moments_linear_chunk_points") is.
 * Workspace of its own (a chunk's model inputs, M and the V of all H steps), within 16 MB or one 64-candidate chunk's need, beside
 * gpmpc_moments_linear's; no gpmpc_last_* state is touched.  Asynchronous on `stream`.
 * GPMPC_ERR_ARG: no cached model, NULL actions / mu0 / gains, B < 1, H < 1, A < 1, D + A (+1) != E, reg < 0 or not finite, no
 * gpmpc_set_cost for this (D, A).  GPMPC_ERR_LIMIT: A > 8.  No output is written on an error.
 */
int gpmpc_lqr_gains(gpmpc_t* h, const double* actions_dev, const double* mu0_host, int B, int H, int A, int include_time,
                    double time0, double reg, double* gains_out_dev, double* P_out_dev, int* flags_out_dev, void* stream);

/*
 * Objective AND analytic gradient: J_out_dev (B), grad_out_dev (B,H,A) = dJ/d(actions) -- what the reference obtains with
 * `mean_cost.backward()` (gp_mpc_controller.py:277) and hands to scipy as `jac` (:132-139, :285): forward rollout, pairwise
 * moment pass over the stored trajectory, reverse sweep.  clip_lower_bound_cost_to_0 clips the value only (pass-through clamp).
 * Other outputs as gpmpc_rollout (nullable).  Supported for D <= 8 with A (+ time) <= 6 and for 8 < D <= 16; otherwise
 * GPMPC_ERR_LIMIT (callers then difference gpmpc_rollout).  gpmpc_last_grad_path (bit mask, a test hook: which moment passes ran):
 * 1 separable off-diagonal pairs (matrix cores), 2 tile moments of the diagonal pairs, 4 streaming element-wise pass, 8 the
 * 8 < D <= 16 pass, 16 tile moments formed inside the batch-major forward, 32 mean part by its own kernel.
 */
int gpmpc_rollout_grad(gpmpc_t* h, const double* actions_dev, const double* mu0_host, const double* S0_host, int B, int H, int A,
                       int include_time, double time0, double* J_out_dev, double* grad_out_dev, double* mu_out_dev,
                       double* Sig_out_dev, double* cost_mu_out_dev, double* cost_var_out_dev, void* stream);
int gpmpc_last_grad_path(gpmpc_t* h);

/*
 * gpmpc_rollout_backward  <->  torch autograd through predict_trajectory (gp_model.py:60-110) and get_rewards_trajectory
 * (setpoint_distance_reward_mapper.py:144-149) -- what compute_mean_lcb_trajectory (gp_mpc_controller.py:229-285) differentiates
 * with its LCB, for any upstream cost: the reverse-mode product (vector-Jacobian product) of gpmpc_rollout for B candidates.
 * It returns the gradients of
 *     sum_t <mu_bar_t, mu_t> + <Sig_bar_t, Sig_t> + cost_mu_bar_t cost_mu_t + cost_var_bar_t cost_var_t  +  J_bar J
 * (mu_t, Sig_t, cost_mu_t, cost_var_t, J: what gpmpc_rollout writes for the same inputs and the same loaded cost) with respect to
 * each candidate's actions and to the initial mean and covariance, per candidate (a shared initial state's gradient is the sum
 * over B).  Inputs as gpmpc_rollout; cotangents (each NULL = 0):
 *   mu_bar_dev (B,H+1,D)  Sig_bar_dev (B,H+1,D,D)  cost_mu_bar_dev (B,H+1)  cost_var_bar_dev (B,H+1)  J_bar_dev (B)
 * Outputs, overwritten (not accumulated into):
 *   actions_bar_out_dev (B,H,A)  required
 *   mu0_bar_out_dev (B,D)        or NULL (not written)
 *   S0_bar_out_dev (B,D,D)       or NULL (not written): the symmetric part sym(G) = (G + G^T) / 2 of the covariance gradient, by
 *                                the rule of gpmpc_moments_backward; Sig_bar is symmetrised on entry (exact: every Sig_t is a
 *                                symmetric function of its inputs)
 * clip_to_zero is pass-through for J (as gpmpc_rollout_grad); the time input is not differentiated.  The cost cotangents weigh the
 * stage-cost partials as the LCB does: wm_t = cost_mu_bar_t + J_bar / (H+1), wv_t = cost_var_bar_t + J_bar (-kappa /
 * (2 sqrt(cost_var_t))) / (H+1); with J_bar = 1 alone actions_bar_out is bit for bit gpmpc_rollout_grad's grad_out.
 * The call runs gpmpc_rollout_grad's launch sequence for that B (forward rollout, the same moment passes and dispatch rules)
 * and then the reverse sweep in a seeded form: the forward is RECOMPUTED inside the call, so nothing is kept between an autograd
 * forward and its backward (the entry is stateless).  Coverage as gpmpc_rollout_grad: D <= 8 with A (+ time) <= 6, and
 * 8 < D <= 16; otherwise GPMPC_ERR_LIMIT.  GPMPC_ERR_ARG: actions_bar_out_dev NULL, A < 1, or a cost / J cotangent without
 * gpmpc_set_cost for this (D, A) (the trajectory's cotangents alone need no cost settings).  gpmpc_last_grad_path reports the
 * moment passes that ran.  Shares gpmpc_rollout_grad's workspace: stream-ordered, not concurrent with gpmpc_rollout /
 * gpmpc_rollout_grad / gpmpc_objective_grad_host on one handle.  Asynchronous on `stream`.
 */
int gpmpc_rollout_backward(gpmpc_t* h, const double* actions_dev, const double* mu0_host, const double* S0_host, int B, int H, int A,
                           int include_time, double time0, const double* mu_bar_dev, const double* Sig_bar_dev,
                           const double* cost_mu_bar_dev, const double* cost_var_bar_dev, const double* J_bar_dev,
                           double* actions_bar_out_dev, double* mu0_bar_out_dev, double* S0_bar_out_dev, void* stream);

/*
 * gpmpc_rollout_linear_backward: the reverse-mode product (vector-Jacobian product) of gpmpc_rollout_linear for B candidates, with
 * the arguments of gpmpc_rollout_backward without any change of meaning.  It returns the gradients of
 *     sum_t <mu_bar_t, mu_t> + <Sig_bar_t, Sig_t> + cost_mu_bar_t cost_mu_t + cost_var_bar_t cost_var_t  +  J_bar J
 * (mu_t, Sig_t, cost_mu_t, cost_var_t, J: what gpmpc_rollout_linear writes for the same inputs and the same loaded cost) with
 * respect to each candidate's actions and to the initial mean and covariance, per candidate.  Cotangents (each NULL = 0):
 *   mu_bar_dev (B,H+1,D)  Sig_bar_dev (B,H+1,D,D)  cost_mu_bar_dev (B,H+1)  cost_var_bar_dev (B,H+1)  J_bar_dev (B)
 * Outputs, overwritten (not accumulated into):
 *   actions_bar_out_dev (B,H,A)  required
 *   mu0_bar_out_dev (B,D)        or NULL (not written)
 *   S0_bar_out_dev (B,D,D)       or NULL (not written): the symmetric part of the covariance gradient, exactly symmetric;
 *                                Sig_bar is symmetrised on entry
 * clip_to_zero is pass-through for J; the time input is not differentiated; the cost cotangents weigh the stage-cost partials by
 * the rule of gpmpc_rollout_backward: wm_t = cost_mu_bar_t + J_bar / (H+1), wv_t = cost_var_bar_t + J_bar (-kappa /
 * (2 sqrt(cost_var_t))) / (H+1); constraints and the terminal weight enter as there.
 * Reverse sweep: with A_t = I + V_s (V_s: the state rows of step t's V) the forward recurrence is Sigma_{t+1} = A_t^T Sigma_t A_t
 * + diag v.  The adjoints lambda_t (D) and Lambda_t (D x D, symmetric) start from mu_bar_t, sym(Sig_bar_t) and the stage /
 * terminal cost partials; for t = H-1 .. 0 the step formula of gpmpc_moments_linear_backward runs with M_bar = lambda_{t+1},
 * W = 2 Sigma_t A_t Lambda_{t+1} on the state rows (0 elsewhere), s_a = Lambda_{t+1}[a,a] and gives x_bar (E); then
 *   lambda_t += lambda_{t+1} + x_bar[:D],   actions_bar_t = (cost partial) + x_bar[D:D+A],   Lambda_t += A_t Lambda_{t+1} A_t^T
 * The forward is RECOMPUTED inside the call (the entry is stateless) and keeps every step's M and V_s beside the trajectory, per
 * chunk of candidates.  Batch-major like the forward: per reverse step one tile launch over all candidates of a chunk (its k
 * loop on the matrix cores) and one wavefront per candidate for the D x E algebra.  A candidate's results are bitwise the same
 * alone and at any position of any batch, whatever "moments_linear_backward_chunk_points" is; a NULL cotangent and an all-zero
 * one give the same bits.  Every sum runs in an order fixed by N, E and D alone; no atomics.  Workspace of its own (a chunk runs
 * its forward and its whole reverse sweep), within 16 MB or one 64-row tile's need.  Touches no other workspace and no
 * gpmpc_last_* state.  Asynchronous on `stream`.  GPMPC_ERR_ARG: actions_bar_out_dev NULL, A < 1, a cost / J cotangent without
 * gpmpc_set_cost for this (D, A) (the trajectory's cotangents alone need no cost settings), and the argument errors of
 * gpmpc_rollout_linear (no cached model, NULL actions / mu0 / S0, B < 1, H < 1, D + A (+1) != E).
 */
int gpmpc_rollout_linear_backward(gpmpc_t* h, const double* actions_dev, const double* mu0_host, const double* S0_host, int B,
                                  int H, int A, int include_time, double time0, const double* mu_bar_dev,
                                  const double* Sig_bar_dev, const double* cost_mu_bar_dev, const double* cost_var_bar_dev,
                                  const double* J_bar_dev, double* actions_bar_out_dev, double* mu0_bar_out_dev,
                                  double* S0_bar_out_dev, void* stream);

/*
 * gpmpc_rollout_linear_feedback_backward: the reverse-mode product (vector-Jacobian product) of gpmpc_rollout_linear_feedback for
 * B candidates: the gradients of
 *     sum_t <mu_bar_t, mu_t> + <Sig_bar_t, Sig_t> + cost_mu_bar_t cost_mu_t + cost_var_bar_t cost_var_t  +  J_bar J
 * (what gpmpc_rollout_linear_feedback writes for the same inputs and the same loaded cost) with respect to each candidate's
 * actions ubar, its gains K_t and the initial mean and covariance, per candidate.  Inputs as gpmpc_rollout_linear_feedback
 * (gains_dev (B,H,A,D) when gains_per_candidate != 0, else (H,A,D) shared); cotangents, conventions, NULL rules and errors as
 * gpmpc_rollout_linear_backward.  Outputs, overwritten (not accumulated into):
 *   actions_bar_out_dev (B,H,A)  required
 *   gains_bar_out_dev (B,H,A,D)  or NULL (not written): ALWAYS per candidate, whatever the layout of gains_dev; a shared gain's
 *                                gradient is the sum over B (the rule of the shared initial state) -- the entry does not reduce
 *   mu0_bar_out_dev (B,D), S0_bar_out_dev (B,D,D)  or NULL (not written); S0_bar the symmetric part, exactly symmetric
 * Forward, per candidate and step t (V_s / V_u the state / action rows of step t's V, K_t (A x D)):
 *   C_t = V_s + K_t^T V_u,   A_t = I + C_t,   Sigma_{t+1} = A_t^T Sigma_t A_t + diag v,   mu_{t+1} = mu_t + M
 * Reverse sweep t = H-1 .. 0 with the adjoints lambda_{t+1} (D), Lambda_{t+1} (D x D, symmetric):
 *   C_bar = 2 Sigma_t A_t Lambda_{t+1}                    (D x D)
 *   W     = [ C_bar ; K_t C_bar ; 0 ]                     (E x D: state rows, action rows, time row)
 *   x_bar = the step formula of gpmpc_moments_linear_backward with M_bar = lambda_{t+1}, this W, s_a = Lambda_{t+1}[a,a]
 *   actions_bar_t = (cost partial wrt ubar_t) + x_bar[D:D+A]
 *   gains_bar_t   = (cost partial wrt K_t) + V_u C_bar^T                                  (A x D)
 *   lambda_t = lambda_{t+1} + x_bar[:D] + (cost partial and seed wrt mu_t)
 *   Lambda_t = sym(A_t Lambda_{t+1} A_t^T) + sym(cost partial and seed wrt Sigma_t)       (i <= j, mirrored)
 * Stage cost partials (t < H), with G = [I ; K_t], Sigma_z = G Sigma_t G^T, e = [mu_t | ubar_t] - target, the loaded W (not
 * assumed symmetric), Q = W Sigma_z W and the weights wm, wv of gpmpc_rollout_backward (cost_var_t: the closed-loop one):
 *   Sz_bar = wm W^T + 4 wv (Q^T + (W^T e)(W e)^T),   e_bar = wm (W + W^T) e + 4 wv (Q + Q^T) e
 *   wrt Sigma_t: G^T Sz_bar G (then symmetrised)     wrt K_t: the action rows of (Sz_bar + Sz_bar^T) G Sigma_t
 *   wrt mu_t: e_bar[:D]                              wrt ubar_t: e_bar[D:]
 * The constraint term (state marginals only: no partial wrt K_t), the terminal step (G = I, W_T, no action, no gain) and the clip
 * (pass-through) are gpmpc_rollout_linear_backward's.
 * The forward is RECOMPUTED inside the call, with the arithmetic of gpmpc_rollout_linear_feedback (the recomputed trajectory has
 * its bits), and keeps every step's M and the D + A state and action rows of V, per chunk of candidates.  The tile launches are
 * gpmpc_rollout_linear_backward's; the closed loop fills the action rows of their weights.  A candidate's results are bitwise the
 * same alone and at any position of any batch, whatever "moments_linear_backward_chunk_points" is and whether its gains arrive
 * shared or per candidate; a NULL cotangent and an all-zero one give the same bits; NULL outputs do not change the others' bits.
 * Every sum runs in an order fixed by N, E, D and A alone; no atomics.  Workspace: gpmpc_rollout_linear_backward's own (within
 * 16 MB or one 64-row tile's need).  Touches no other workspace and no gpmpc_last_* state.  Asynchronous on `stream`.
 * gains_dev == NULL with gains_bar_out_dev == NULL: the call IS gpmpc_rollout_linear_backward (the same bits); gains_dev == NULL
 * with gains_bar_out_dev != NULL: GPMPC_ERR_ARG.  Other errors: those of gpmpc_rollout_linear_backward.
 */
int gpmpc_rollout_linear_feedback_backward(gpmpc_t* h, const double* actions_dev, const double* gains_dev, int gains_per_candidate,
                                           const double* mu0_host, const double* S0_host, int B, int H, int A, int include_time,
                                           double time0, const double* mu_bar_dev, const double* Sig_bar_dev,
                                           const double* cost_mu_bar_dev, const double* cost_var_bar_dev, const double* J_bar_dev,
                                           double* actions_bar_out_dev, double* gains_bar_out_dev, double* mu0_bar_out_dev,
                                           double* S0_bar_out_dev, void* stream);

/*
 * gpmpc_rollout_feedback_backward: the reverse-mode product (vector-Jacobian product) of gpmpc_rollout_feedback for B candidates:
 * the gradients of
 *     sum_t <mu_bar_t, mu_t> + <Sig_bar_t, Sig_t> + cost_mu_bar_t cost_mu_t + cost_var_bar_t cost_var_t  +  J_bar J
 * (what gpmpc_rollout_feedback writes for the same inputs and the same loaded cost) with respect to each candidate's actions ubar,
 * its gains K_t and the initial mean and covariance, per candidate.  Arguments as gpmpc_rollout_linear_feedback_backward, one for
 * one (gains_dev (B,H,A,D) when gains_per_candidate != 0, else (H,A,D) shared); its conventions hold: outputs are overwritten, a
 * NULL cotangent is zero, Sig_bar is symmetrised on entry, the clip is pass-through for J, the time input is not differentiated,
 * the cost weights are wm_t = cost_mu_bar_t + J_bar / (H+1), wv_t = cost_var_bar_t + J_bar (-kappa / (2 sqrt(cost_var_t))) / (H+1).
 * Outputs:
 *   actions_bar_out_dev (B,H,A)  required
 *   gains_bar_out_dev (B,H,A,D)  or NULL (not written): ALWAYS per candidate, whatever the layout of gains_dev; a shared gain's
 *                                gradient is the sum over B -- the entry does not reduce
 *   mu0_bar_out_dev (B,D), S0_bar_out_dev (B,D,D)  or NULL (not written); S0_bar the symmetric part, exactly symmetric
 * Forward, per candidate and step t, with x_t = [mu_t | ubar_t | time0 + t] and G_t = [I_D ; K_t ; 0] (E x D):
 *   Sigma_in = G_t Sigma_t G_t^T,   (M, S, V) = moments(x_t, Sigma_in),   R = Sigma_in[:D, :] (D x E),   C = R V,
 *   mu_{t+1} = mu_t + M,   Sigma_{t+1} = Sigma_t + S + C + C^T
 * Reverse sweep t = H-1 .. 0 with the adjoints lambda_{t+1} (D), Lambda_{t+1} (D x D, symmetric), which start from mu_bar_H,
 * sym(Sig_bar_H) and the terminal cost partials:
 *   M_bar = lambda_{t+1},   S_bar = Lambda_{t+1},   C_bar = 2 Lambda_{t+1}
 *   V_bar = R^T C_bar  (E x D, time row zero),   R_bar = C_bar V^T  (D x E)
 *   (x_bar, P) = the step formula of gpmpc_moments_backward at (x_t, Sigma_in) with (M_bar, S_bar, V_bar); P the symmetric part
 *   Z = P + sym([R_bar ; 0])                                                              (E x E, R_bar in the first D rows)
 *   actions_bar_t = x_bar[D:D+A] + (cost partial wrt ubar_t)
 *   gains_bar_t   = the action rows of 2 Z G_t Sigma_t + (cost partial wrt K_t)           (A x D)
 *   lambda_t = lambda_{t+1} + x_bar[:D] + mu_bar_t + (cost partial wrt mu_t)
 *   Lambda_t = Lambda_{t+1} + G_t^T Z G_t + sym(Sig_bar_t + cost partial wrt Sigma_t)     (i <= j, mirrored)
 * and mu0_bar = lambda_0, S0_bar = Lambda_0.  Stage and terminal cost partials: those of gpmpc_rollout_linear_feedback_backward
 * (the same device code).
 * The forward is RECOMPUTED inside the call by gpmpc_rollout_feedback's own kernels (the recomputed trajectory and model inputs
 * have its bits) and keeps every step's V, per chunk of candidates; each reverse step runs gpmpc_moments_backward's launches over
 * the chunk.  The call is stateless.  Bitwise contracts: a candidate's four outputs are the same bits alone and at any position of
 * any batch; for any value of "rollout_feedback_backward_chunk_points", "moments_chunk_points" and
 * "moments_backward_chunk_points"; and whether its gains arrive shared or per candidate.  A NULL cotangent and an all-zero one
 * give the same bits; NULL optional outputs do not change the others' bits.  Every sum runs in an order fixed by N, E, D and A
 * alone; no atomics.  Workspace: its own (model inputs, recomputed trajectory, every step's V, adjoints, the cotangents and results
 * of the moment gradient), within 16 MB or one candidate's need: option "rollout_feedback_backward_chunk_points" (candidates per
 * chunk, 0 = auto); it also uses gpmpc_moments' and gpmpc_moments_backward's workspaces and honours their chunk options.  Touches
 * no gpmpc_last_* state.  Asynchronous on `stream`.
 * gains_dev == NULL with gains_bar_out_dev == NULL: the zero-gain policy through these same kernels (gpmpc_rollout_backward to
 * rounding, not bit for bit); gains_dev == NULL with gains_bar_out_dev != NULL: GPMPC_ERR_ARG.  Other errors (no output is written
 * on an error): the argument and limit errors of gpmpc_rollout_feedback; GPMPC_ERR_ARG for actions_bar_out_dev == NULL, for A < 1,
 * and for a cost or J cotangent without gpmpc_set_cost for this (D, A).
 */
int gpmpc_rollout_feedback_backward(gpmpc_t* h, const double* actions_dev, const double* gains_dev, int gains_per_candidate,
                                    const double* mu0_host, const double* S0_host, int B, int H, int A, int include_time,
                                    double time0, const double* mu_bar_dev, const double* Sig_bar_dev,
                                    const double* cost_mu_bar_dev, const double* cost_var_bar_dev, const double* J_bar_dev,
                                    double* actions_bar_out_dev, double* gains_bar_out_dev, double* mu0_bar_out_dev,
                                    double* S0_bar_out_dev, void* stream);

/*
 * gpmpc_objective_grad_host  <->  ONE call of compute_mean_lcb_trajectory (gp_mpc_controller.py:229-285) as scipy's L-BFGS-B
 * makes it (:133-141: one action sequence per evaluation, host arrays in, (float, host gradient) out): gpmpc_rollout_grad for
 * B = 1 with host buffers on both sides; returns when the results are in *result_host (the last kernel raises a completion word
 * the call polls; `stream` itself may still be draining).  actions_host (H,A).  *result_host: pinned host
 * buffer owned by the handle, valid until the next call: J (1) | grad (H,A) | mu (H+1,D) | Sig (H+1,D,D) | cost_mu (H+1) |
 * cost_var (H+1) (trajectory and stage costs: what the reference caches for IterationInformation, :279-283).
 */
int gpmpc_objective_grad_host(gpmpc_t* h, const double* actions_host, const double* mu0_host, const double* S0_host,
                              int H, int A, int include_time, double time0, const double** result_host, void* stream);

/*
 * gpmpc_argmin  <->  the keep-the-best rule of gp_mpc_controller.py:146-148 on a vector of objectives: first strict minimum wins;
 * a NaN in GLOBAL slot 0 is adopted and never displaced; any other NaN is never selected.  `first_global_index` = global index of
 * J_dev[0] (the shard offset when candidates are sharded over GPUs); the returned index is global; nothing selectable: index -1,
 * J = +inf.  gpmpc_argmin synchronises and writes HOST memory; gpmpc_argmin_async does not: it writes the device record
 * out_dev[0] = best J, [1] = (double) global index, [2 .. 2+HA) = the winning sequence when actions_dev (B,HA) is given -- ready
 * to be all-gathered over RCCL as is (the ONE exchange of a sharded control step).  gpmpc_argmin_export is gpmpc_argmin_async
 * whose kernel ALSO stores the same record to out_host (2 + HA doubles of PINNED host memory this device can address, e.g.
 * hipHostMalloc / a pinned torch tensor) and fences at system scope: the single-GPU step needs no device-to-host copy behind it
 * (gp_mpc_controller.py:146-148 reads the winner on the host).  The record is complete once the stream has passed the call (wait
 * for an event recorded behind it); any other kind of out_host pointer is GPMPC_ERR_ARG.
 */
int gpmpc_argmin(gpmpc_t* h, const double* J_dev, int B, long long first_global_index, double* best_J_host,
                 long long* best_idx_host, void* stream);
int gpmpc_argmin_async(gpmpc_t* h, const double* J_dev, int B, long long first_global_index, const double* actions_dev, int HA,
                       double* out_dev, void* stream);
int gpmpc_argmin_export(gpmpc_t* h, const double* J_dev, int B, long long first_global_index, const double* actions_dev, int HA,
                        double* out_dev, double* out_host, void* stream);

/*
 * Candidate optimisation whose loop stays on the device (replaces B sequential scipy restarts, gp_mpc_controller.py:125-141, by a
 * cross-entropy search over the same box [0,1]^(H*A)): per iteration B vectors are drawn around the current mean / std
 * (iteration 0: uniform; slot 0 = the incumbent / `first_candidate_host`), mapped to model actions (mapper 0: identity reshape,
 * normalization_action_mapper.py:21-23; 1: scaled deltas + cumulative sum + pass-through clamp, derivative_action_mapper.py:28-35,
 * with max_change_host (A), action_prev_host (A)), evaluated by one rollout launch, and the n_elite best refit mean and std.
 * Nothing is read back between iterations.  best_out_dev (H*A + 1) = [best vector | its objective].  Draws: Philox4x32-10 keyed
 * by `seed`, or noise_dev (iterations, B, H*A) (iteration 0 uniforms, later standard normals: the parity tests' hook).  2 <= B <= 4096.
 *
 * Sharded over GPUs: gpmpc_cem_local = this GPU's slice [first, first + B_local) of iteration `iteration` (draws
 * indexed by the GLOBAL candidate, so the union of the slices is the single-GPU population) -> elites_out_dev (n_elite, 2 + H*A)
 * = [J | global index | vector], sorted, padded with (+inf, INT_MAX); the caller all-gathers them (RCCL); gpmpc_cem_merge refits
 * on the union (lists * n_elite <= 4096) -> state_dev = [mean | std | best vector | best J], bit for bit the single-GPU state.
 */
int gpmpc_cem_search(gpmpc_t* h, const double* mu0_host, const double* S0_host, int B, int H, int A, int include_time, double time0,
                     int iterations, int n_elite, unsigned long long seed, const double* first_candidate_host, int mapper,
                     const double* max_change_host, const double* action_prev_host, const double* noise_dev, double* best_out_dev,
                     void* stream);
int gpmpc_cem_local(gpmpc_t* h, const double* mu0_host, const double* S0_host, int B_total, int first, int B_local, int H, int A,
                    int include_time, double time0, int iteration, int n_elite, unsigned long long seed,
                    const double* first_candidate_host, int mapper, const double* max_change_host, const double* action_prev_host,
                    const double* noise_dev, const double* state_dev, double* elites_out_dev, void* stream);
int gpmpc_cem_merge(gpmpc_t* h, const double* elites_dev, int lists, int n_elite, int n, int iteration, double* state_dev,
                    void* stream);

/*
 * Gradient-based candidate optimisation whose loop stays on the device: a box-constrained (projected) L-BFGS over [0,1]^n,
 * n = H*A, for B restarts in lockstep -- the counterpart of gpmpc_cem_search for the analytic gradient (the reference: one scipy
 * L-BFGS-B solve per restart, gp_mpc_controller.py:125-141).  EVERY iteration evaluates exactly ONE trial point per restart, so
 * the launch sequence never depends on data: the line search (Armijo, constant c1, step halved on a reject) is spread over
 * iterations.  Iteration k is handed (Jt, Gt) = objective and dJ/d(model actions) at the state's `actions`:
 *   chain rule to the optimiser vector (mapper 0: Gt; 1: gt[s,a] = 2 max_change[a] sum_{t>=s} Gt[t,a], clamp passed through);
 *   k = 0 accepts (non-finite Jt / gt: status 3); k > 0 accepts when Jt and gt are finite and Jt <= J + c1 g.(xt - x);
 *   accept (k > 0): the pair s = xt - x, y = gt - g joins the ring of `history` pairs when s.y > 1e-10 |s| |y| (the oldest
 *     leaves), then (x, J, g) <- (xt, Jt, gt);
 *   reject: alpha <- alpha / 2, below 2^-40 status 2, else xt = clip(x + alpha d);
 *   after an accept: free set F = coordinates not (x <= 0, g > 0) and not (x >= 1, g < 0), gf = g on F; max |gf| <= pgtol: status 1;
 *     else the two-loop recursion on gf (initial scaling s.y / y.y of the newest pair, 1 / |gf| without pairs), d = -r on F;
 *     d.gf not < 0: d = -gf and all pairs are dropped; alpha = 1, xt = clip(x + d);
 *   a restart whose status != 0 keeps xt = x, is still evaluated (lockstep) and its state no longer changes;
 *   actions = mapper(xt) (mapper as in gpmpc_cem_search: 0 identity reshape, 1 scaled deltas + running sum + pass-through clamp).
 * J never increases along x, so x is each restart's best point.  status: 0 running, 1 converged, 2 step underflow, 3 non-finite
 * start.
 *
 * state_dev is the CALLER's buffer of gpmpc_lbfgs_state_size(B, n, history) doubles (< 0: bad arguments), m = history:
 *   x (B,n) | g (B,n) | d (B,n) | xt (B,n) | actions (B,n) | J (B) | alpha (B) | status (B) | pushes (B)
 *   | S (B,m,n) | Y (B,m,n) | sy (B,m) | yy (B,m)
 * status and pushes are whole numbers stored as doubles; `pushes` counts the pairs pushed since the last drop: min(pushes, m) are
 * held, the newest in ring slot (pushes - 1) mod m.  sy / yy = s.y and y.y of the slot's pair.
 *
 * gpmpc_lbfgs_init: xt = clip(x0_dev (B,n)), actions = mapper(xt), status 0, alpha 1, everything else 0.  gpmpc_lbfgs_step: one
 * iteration k = `iteration` from supplied J_dev (B) and grad_model_dev (B,H,A) -- the unit the search is built from (and the parity
 * tests' hook); neither needs a model.  gpmpc_lbfgs_search (model and gpmpc_set_cost needed): with first_iteration == 0 the init
 * from x0_dev, then `iterations` times [objective + gradient of the state's actions; step k = first_iteration + i] -- propagation
 * 0: the launches of gpmpc_rollout_grad, 1: those of gpmpc_rollout_linear then gpmpc_rollout_linear_backward with J_bar = 1 --
 * and the winner by gpmpc_argmin's rule over the restarts' J to best_out_dev (2 + n) = [J | restart | x] (may be NULL).
 * first_iteration > 0 continues a state (x0_dev unused).  All three are asynchronous on `stream`, without host synchronisation;
 * the host arrays are read before the call returns.
 *
 * Limits: 1 <= B <= 4096, 1 <= history <= 32, 1 <= n <= 4096, iterations >= 1, first_iteration / iteration >= 0, 0 < c1 < 1,
 * pgtol >= 0; mapper 1 needs max_change_host (A) and action_prev_host (A) (GPMPC_ERR_ARG) and A <= 24 (GPMPC_ERR_LIMIT).  A shape
 * outside the gradient kernels is GPMPC_ERR_LIMIT as in gpmpc_rollout_grad.  Every such error is reported before anything is
 * enqueued or written.
 */
long long gpmpc_lbfgs_state_size(int B, int n, int history);
int gpmpc_lbfgs_init(gpmpc_t* h, const double* x0_dev, int B, int H, int A, int history, int mapper, const double* max_change_host,
                     const double* action_prev_host, double* state_dev, void* stream);
int gpmpc_lbfgs_step(gpmpc_t* h, const double* J_dev, const double* grad_model_dev, int B, int H, int A, int iteration, int history,
                     double c1, double pgtol, int mapper, const double* max_change_host, const double* action_prev_host,
                     double* state_dev, void* stream);
int gpmpc_lbfgs_search(gpmpc_t* h, const double* mu0_host, const double* S0_host, int B, int H, int A, int include_time, double time0,
                       int propagation, int first_iteration, int iterations, int history, double c1, double pgtol, int mapper,
                       const double* max_change_host, const double* action_prev_host, const double* x0_dev, double* state_dev,
                       double* best_out_dev, void* stream);

/*
 * Hyper-parameter training whose loop stays on the device: the training loss of gpmpc_mll for R hyper-parameter sets per GP in one
 * launch per chunk, left on the device, and a multi-restart search built on it and on gpmpc_lbfgs_step.  n = E + 2; a parameter
 * row is [lengthscale (E) | outputscale | noise]; problem p = r D + a is restart r of GP a, P = R D.
 *
 * gpmpc_mll_batch: per problem loss_out_dev[p] = -log p(y_a | X, theta_p) / N and grad_out_dev[p] (n), gpmpc_mll's definition.
 * Without a box (lo_dev = hi_dev = NULL) params_dev (R, D, n) is theta itself and the gradient is wrt theta.  With a box (D, n)
 * params_dev is x in [0,1]^n, theta = lo + (hi - lo) x (log_scale 0) or theta = lo (hi / lo)^x (log_scale 1), and the gradient is
 * wrt x (times hi - lo, or theta ln(hi / lo)).  theta_out_dev (R, D, n), may be NULL: the theta that was used.  Box validity
 * (lo <= hi; lo > 0 under the log map) is the caller's to check.  A K_p + noise I that is not positive definite is a RESULT, not an
 * error: loss = +inf, gradient = 0 and info_out_dev[p] (may be NULL) = the order of the first leading minor whose pivot is not
 * positive and finite; otherwise info = 0.  gpmpc_lbfgs_step rejects a non-finite trial value and gives a non-finite start status 3.
 * One workgroup per problem, N <= 256; every sum in a fixed order without atomics: two calls agree bit for bit, and a problem's
 * result depends neither on R, nor on its position, nor on the chunk.  The workspace is the handle's, for option "mll_batch_chunk"
 * problems at a time (default: one per CU), launched chunk after chunk on `stream`.
 *
 * gpmpc_train_search: with first_iteration == 0 gpmpc_lbfgs_init from x0_dev (R, D, n) (mapper 0, H = 1, A = n), then `iterations`
 * times [gpmpc_mll_batch of the state's `actions` with the box; gpmpc_lbfgs_step k = first_iteration + i], then per GP a
 * best_out_dev[a] (3 + n, may be NULL) = [loss | restart | status | theta]: the lowest state J over the restarts whose status != 3,
 * ties to the lowest restart, theta = the box map of that restart's x; [+inf | -1 | 3 | theta of restart 0's x] where every restart
 * has status 3.  state_dev: the caller's gpmpc_lbfgs_state_size(R D, n, history) doubles, laid out as for gpmpc_lbfgs_search.
 * first_iteration > 0 continues a state (x0_dev unused).  The box is required.
 *
 * Both are asynchronous on `stream` without host synchronisation or a copy to the host, and neither read nor write the cached
 * model, its record or the gpmpc_last_* state: a gpmpc_rollout after the call returns the bits it returned before.  Errors are
 * reported before anything is enqueued or written.  GPMPC_ERR_ARG: NULL X / Y / params / loss / grad (train_search: state, x0 with
 * first_iteration == 0, the box), only one of lo and hi, N < 1, R < 1, log_scale not 0 or 1, and for train_search history < 1,
 * iterations < 1, first_iteration < 0, c1 outside (0, 1), pgtol < 0.  GPMPC_ERR_LIMIT: N > 256, D > GPMPC_MAX_D, E > GPMPC_MAX_E,
 * R D > 4096, history > 32.
 */
int gpmpc_mll_batch(gpmpc_t* h, const double* X_dev, const double* Y_dev, int N, int D, int E, const double* params_dev, int R,
                    const double* lo_dev, const double* hi_dev, int log_scale, double* loss_out_dev, double* grad_out_dev,
                    double* theta_out_dev, int* info_dev, void* stream);
int gpmpc_train_search(gpmpc_t* h, const double* X_dev, const double* Y_dev, int N, int D, int E, int R, const double* lo_dev,
                       const double* hi_dev, int log_scale, int first_iteration, int iterations, int history, double c1,
                       double pgtol, const double* x0_dev, double* state_dev, double* best_out_dev, void* stream);

/*
 * Second-order candidate optimisation whose loop stays on the device: a clamped iLQR on the MEAN dynamics of the linearised
 * propagation, for B candidates in lockstep -- the trajectory optimiser beside gpmpc_cem_search and gpmpc_lbfgs_search.  Per
 * candidate, with ubar (H,A) in [0,1]:
 *   dynamics  x_{t+1} = x_t + M([x_t | u_t | time0 + t]), x_0 = mu0 (M: the posterior mean of gpmpc_moments_linear);
 *   cost      W_s = (W + W^T) / 2 = (Q | N ; N^T | R), P_H = (W_T + W_T^T) / 2, e_t = [x_t | u_t] - target, e_H = x_H - target[:D],
 *             c = (sum_{t<H} e_t^T W_s e_t + e_H^T P_H e_H) / (H + 1)    on the block loaded by gpmpc_set_cost for this (D, A).
 * The design is CERTAINTY-EQUIVALENT: kappa, the variance terms of the LCB, clipping of the cost and the state constraints do NOT
 * enter.  It is CLAMPED iLQR: the box [0,1] is honoured by clipping the realised action of the forward pass, not by a box QP in
 * the sweep.
 *
 * gpmpc_ilqr_backward: at actions_dev (B,H,A) with the per-candidate regularisation reg_dev (B, a DEVICE array: the loop never
 * reads it back).  A_t, B_t, F, Huu (+ reg I), Hux, the Cholesky factorisation, K_t and P_t are exactly gpmpc_lqr_gains's; beside
 * them, for t = H-1 .. 0,
 *   p_H = P_H e_H,   q = W_s e_t = [q_x ; q_u],   g_x = q_x + A_t^T p_{t+1},   g_u = q_u + B_t^T p_{t+1},
 *   k_t = -Huu^-1 g_u (the same factor as K_t),   p_t = g_x + Hux^T k_t,
 *   dV = sum_t g_u^T k_t / (H + 1)  (<= 0; the model predicts a change of (2 alpha - alpha^2) dV for the step size alpha),
 *   step = max_{t,a} |clip(ubar_t + k_t, 0, 1) - ubar_t|.
 * A lost pivot (<= 0 or not finite) is handled as in gpmpc_lqr_gains: the step gets K_t = 0, k_t = 0, p_t = g_x, and the
 * candidate's flag counts it.  Outputs (all required): gains_out_dev (B,H,A,D), ff_out_dev (B,H,A) = k_t, mu_out_dev (B,H+1,D) the
 * nominal trajectory, info_out_dev (B,5) = [cost | dV | step | flags | reserved 0] (flags a whole number stored as a double).
 * mu_out is gpmpc_rollout_linear's mu bit for bit; the gains are gpmpc_lqr_gains's bit for bit for the same reg.
 *
 * gpmpc_ilqr_forward: for the L step sizes alphas_host, x_0 = mu0, u_t = clip(ubar_t + alpha k_t + K_t (x_t - xbar_t), 0, 1),
 * x_{t+1} = x_t + M(.): trial_actions_out_dev (B,L,H,A) (the clipped actions), trial_cost_out_dev (B,L) = c(alpha), and
 * trial_mu_out_dev (B,L,H+1,D) or NULL.  All B L rows run in the same launches.  With nominal actions in the box and finite gains,
 * alpha = 0 returns the nominal actions, the nominal mu and gpmpc_ilqr_backward's cost bit for bit, whatever the gains are: the
 * nominal and every trial cost come from one kernel, so equal trajectories get equal bits.
 *
 * state_dev is the CALLER's buffer of gpmpc_ilqr_state_size(B, H, A, D, L) doubles (< 0: bad arguments):
 *   actions (B,H,A) | cost (B) | reg (B) | status (B) | accepts (B) | chosen (B) | dV (B) | step (B) | flags (B) | J (B)
 *   | trial_cost (B,L) | gains (B,H,A,D) | ff (B,H,A) | mu (B,H+1,D) | trial_actions (B,L,H,A)
 * Whole numbers are stored as doubles.  status: 0 running, 1 converged (step <= tol: in the interior, or resting on the box with
 * the feed-forward pointing outward), 2 regularisation above reg_max, 3 non-finite cost.
 *
 * gpmpc_ilqr_init: actions = clip(x0_dev (B,H,A)), reg = reg0, chosen = -1, everything else 0.  gpmpc_ilqr_step: one iteration.
 * Candidates whose status != 0 are still evaluated (lockstep) and their state no longer changes.  In order:
 *   1. backward at the state's actions with the candidate's reg: gains, ff, mu, cost, dV, step, flags;
 *   2. cost not finite: status 3;   3. else step <= tol: status 1;
 *   4. forward for the ladder alpha_l = 2^-l, l = 0 .. L-1: trial_actions, trial_cost;
 *   5. l* = the finite trial of lowest cost, ties to the smallest l; accept iff trial_cost[l*] < cost (strict):
 *        accept: actions <- trial_actions[l*], cost <- trial_cost[l*], reg <- max(reg / reg_factor, reg0), accepts += 1, chosen = l*;
 *        else:   chosen = -1, reg <- reg reg_factor, and status 2 once reg > reg_max.
 * cost never increases.  gpmpc_ilqr_search: init from x0_dev, `iterations` steps, then one gpmpc_rollout_linear launch sequence
 * over the B final sequences with mu0, S0 (J only) into the state's J -- the library's LCB objective, so the winner composes with
 * the other optimisers -- and the winner by gpmpc_argmin's rule to best_out_dev (2 + H A) = [J | restart | actions] (may be NULL).
 * gpmpc_ilqr_search(iterations = k) leaves the state of gpmpc_ilqr_init plus k gpmpc_ilqr_step calls (J aside).
 *
 * All entries are asynchronous on `stream`: no host synchronisation, no read-back, a launch sequence fixed by the arguments; host
 * arrays are read before the call returns.  Plain kernels: no atomics, no waits between workgroups; every sum runs in an order
 * fixed by N, E, D, A, H and L alone -- a candidate's results are bitwise the same alone, at any place of any batch and whatever
 * "ilqr_chunk_points" / "moments_linear_chunk_points" are.  Workspace of its own (a chunk's model inputs, M, the nominal V of all
 * H steps and the trial trajectories), within 16 MB or one chunk's need, beside those of gpmpc_moments_linear /
 * gpmpc_rollout_linear; no gpmpc_last_* state is touched.
 * GPMPC_ERR_ARG: no cached model, a NULL required pointer, B < 1 or B > 4096, H < 1, A < 1, D + A (+1) != E, L < 1 or L > 16,
 * iterations < 1, reg0 not finite or < 0, reg_factor not > 1, reg_max < reg0, tol < 0, no gpmpc_set_cost for this (D, A).
 * GPMPC_ERR_LIMIT: A > 8.  Every such error is reported before anything is enqueued or written.
 */
long long gpmpc_ilqr_state_size(int B, int H, int A, int D, int L);
int gpmpc_ilqr_backward(gpmpc_t* h, const double* actions_dev, const double* mu0_host, int B, int H, int A, int include_time,
                        double time0, const double* reg_dev, double* gains_out_dev, double* ff_out_dev, double* mu_out_dev,
                        double* info_out_dev, void* stream);
int gpmpc_ilqr_forward(gpmpc_t* h, const double* actions_dev, const double* gains_dev, const double* ff_dev, const double* mu_nom_dev,
                       const double* mu0_host, int B, int H, int A, int include_time, double time0, const double* alphas_host, int L,
                       double* trial_actions_out_dev, double* trial_cost_out_dev, double* trial_mu_out_dev, void* stream);
int gpmpc_ilqr_init(gpmpc_t* h, const double* x0_dev, int B, int H, int A, int L, double reg0, double* state_dev, void* stream);
int gpmpc_ilqr_step(gpmpc_t* h, const double* mu0_host, int B, int H, int A, int include_time, double time0, int L, double reg0,
                    double reg_factor, double reg_max, double tol, double* state_dev, void* stream);
int gpmpc_ilqr_search(gpmpc_t* h, const double* mu0_host, const double* S0_host, int B, int H, int A, int include_time, double time0,
                      int iterations, int L, double reg0, double reg_factor, double reg_max, double tol, const double* x0_dev,
                      double* state_dev, double* best_out_dev, void* stream);

/* bench.py: `reps` rollouts back to back bracketed by HIP events recorded on `stream`; average ms per launch in *ms_host. */
int gpmpc_rollout_timed(gpmpc_t* h, const double* actions_dev, const double* mu0_host, const double* S0_host, int B, int H, int A,
                        int include_time, double time0, double* J_out_dev, int reps, float* ms_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPMPC_H */
