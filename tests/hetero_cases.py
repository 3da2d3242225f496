"""Workloads of tests/test_hetero_reference.py (CPU) and tests/test_gpu_hetero_outputs.py (GPU): hyper-parameters that DIFFER
per output.  One function builds every case, so that the two tiers can never disagree about the inputs.

Every other workload of the suite (oracle/synth.make_workload, the fixtures under tests/golden/) gives all outputs the same
outputscale and the same noise and draws the lengthscales from 0.5 ... 1.5, so an index mix-up between outputs (var[0] for
every output, var[a] where var[b] belongs, noise a in the factorisation of output b) changes nothing there.  Here

  * outputscales are distinct and span >= 100x inside the training box [1e-3, 0.95], noise variances are distinct and span
    >= 100x, small noise paired with small outputscale (cond(K_a) stays below ~1e6), Y[:, a] scaled by sqrt(outputscale_a / 0.05);
  * the lengthscales of the state and action columns are log-uniform in [0.3, 4] (the time column stays as make_workload drew it);
    the case "n33_d3_short" gives one output lengthscales of 0.15, which puts its pairs on the exact-exp loop (degree 0);
  * the initial covariance is dense, D^(1/2) C D^(1/2) with a random correlation matrix C and a diagonal from 1e-6 to 1e-2;
  * every case has a reversed-outputs twin ("..._rev"): the same problem with the outputs in the opposite order, whose truth is
    the permuted truth -- it catches any a < b assumption.

Shapes: the smallest that reach each unit of the fused-horizon kernel (tests/item_loop_cases.SHAPES) plus one D = 6 case;
A = 1 (2 for D >= 4), H = 4, B = 3.

The error metric of both tiers is per output: an entry is scaled by its OWN outputs, so that an error in a small-variance output
cannot hide behind a large-variance one (`err_out`, `err_cov`, `err_in_out`)."""
import dataclasses
import functools

import numpy as np

from oracle import synth
from oracle import gpmpc_oracle as orc
from oracle import extended_precision as xp

H = 4
B = 3

OUTPUTSCALES = [0.6, 0.004, 0.05, 0.2, 0.012, 0.9]
NOISES = [4e-3, 1e-6, 1e-5, 3e-4, 2e-6, 1e-2]
S0_DIAG = [1e-6, 1e-2, 1e-3, 1e-4, 3e-5, 3e-3]

# name -> (N, D, include_time, output with lengthscales of 0.15 or None)
BASE = {
    "n33_d3": (33, 3, False, None),
    "n33_d3_short": (33, 3, False, 1),
    "n130_d3": (130, 3, False, None),
    "n47_d3_time": (47, 3, True, None),
    "n70_d2": (70, 2, False, None),
    "n66_d4": (66, 4, False, None),
    "n40_d6": (40, 6, False, None),
}
NAMES = [n + s for n in BASE for s in ("", "_rev")]
D3_NAMES = [n for n in BASE if BASE[n][1] == 3]


def reverse_outputs(w):
    """The same problem with the outputs (= state dimensions) in the opposite order."""
    N, D, A, E, _, _ = w.dims
    cols = np.concatenate([np.arange(D)[::-1], np.arange(D, E)])           # state columns reversed, action / time columns stay
    tcols = cols[:D + A]
    return dataclasses.replace(
        w, X=np.ascontiguousarray(w.X[:, cols]), Y=np.ascontiguousarray(w.Y[:, ::-1]),
        lengthscales=np.ascontiguousarray(w.lengthscales[::-1][:, cols]), outputscales=w.outputscales[::-1].copy(),
        noises=w.noises[::-1].copy(), mu0=w.mu0[::-1].copy(), S0=np.ascontiguousarray(w.S0[::-1, ::-1]),
        target=w.target[tcols].copy(), W=np.ascontiguousarray(w.W[np.ix_(tcols, tcols)]),
        W_T=np.ascontiguousarray(w.W_T[::-1, ::-1]))


@functools.lru_cache(maxsize=None)
def make_case(name):
    """The workload `name` of NAMES (a synth.Workload; treat it as read-only: it is shared between tests)."""
    if name.endswith("_rev"):
        return reverse_outputs(make_case(name[:-4]))
    N, D, tm, short = BASE[name]
    A = 2 if D >= 4 else 1
    seed = 9000 + 10 * N + D
    w = synth.make_workload(N=N, D=D, A=A, H=H, B=B, include_time=tm, seed=seed, dynamics="contracting",
                            time0=float(N) if tm else 0.0)
    rng = np.random.default_rng(seed + 5)
    osc = np.array(OUTPUTSCALES[:D])
    nz = np.array(NOISES[:D])
    ls = w.lengthscales.copy()
    ls[:, :D + A] = np.exp(rng.uniform(np.log(0.3), np.log(4.0), size=(D, D + A)))
    if short is not None:
        ls[short, :D] = 0.15
    G = rng.standard_normal((D, D))
    C = G @ G.T + 0.5 * np.eye(D)
    C = C / np.sqrt(np.outer(np.diag(C), np.diag(C)))                      # a dense correlation matrix
    sd = np.sqrt(np.array(S0_DIAG[:D]))
    S0 = sd[:, None] * C * sd[None, :]
    S0 = 0.5 * (S0 + S0.T)
    return dataclasses.replace(w, Y=w.Y * np.sqrt(osc / 0.05)[None, :], lengthscales=ls, outputscales=osc, noises=nz, S0=S0)


# ---------------------------------------------------------------------------------------------------- the per-output metric
def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _scale(ref, axis):
    """max |ref| over everything but `axis` (one value per output); 1 where an output is identically zero."""
    ref = np.abs(_f64(ref))
    s = np.max(np.moveaxis(ref, axis, -1).reshape(-1, ref.shape[axis]), axis=0)
    return np.where(s > 0, s, 1.0)


def err_out(a, ref):
    """(..., D) arrays: max_a ( max |a - ref|_a / max |ref_a| )."""
    a, ref = _f64(a), _f64(ref)
    return float(np.max(np.abs(a - ref) / _scale(ref, -1)))


def err_cov(a, ref):
    """(..., D, D) arrays: max |a - ref|_ab / sqrt(max |ref_aa| max |ref_bb|)."""
    a, ref = _f64(a), _f64(ref)
    d = _scale(np.diagonal(ref, axis1=-2, axis2=-1), -1)
    return float(np.max(np.abs(a - ref) / np.sqrt(d[:, None] * d[None, :])))


def err_in_out(a, ref):
    """(..., E, D) input-output arrays: column a scaled by output a."""
    return err_out(a, ref)


def err_per_gp(a, ref):
    """(D, ...) arrays with the output in FRONT (iK (D, N, N), beta (D, N), losses (D,)): each output on its own scale."""
    a, ref = _f64(a), _f64(ref)
    D = ref.shape[0]
    return err_out(a.reshape(D, -1).T, ref.reshape(D, -1).T)


# ------------------------------------------------------------------------------------------------------------- references
def hyper(w, **mutated):
    """The hyper-parameter arguments (lengthscales, outputscales, noises) of `w`, some of them replaced."""
    return (mutated.get("lengthscales", w.lengthscales), mutated.get("outputscales", w.outputscales),
            mutated.get("noises", w.noises))


def oracle_factors(w, **mutated):
    ls, osc, nz = hyper(w, **mutated)
    return orc.Factors(w.X, w.Y, ls, osc, nz)


@functools.lru_cache(maxsize=None)
def truth_factors(name):
    w = make_case(name)
    return xp.Factors(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)


@functools.lru_cache(maxsize=None)
def truth(name):
    """The longdouble evaluation of case `name`, rounded to fp64: dict(iK, beta, mu (B, H+1, D), Sig (B, H+1, D, D), cost_mu,
    cost_var, J) -- the costs are gpmpc_oracle's on the truth trajectory."""
    w = make_case(name)
    f = truth_factors(name)
    tr = [xp.predict_trajectory(f, w.actions[c], w.mu0, w.S0, w.include_time, w.time0) for c in range(w.actions.shape[0])]
    mu = np.stack([_f64(t[0]) for t in tr])
    Sig = np.stack([_f64(t[1]) for t in tr])
    cm, cv = orc.stage_costs(mu, Sig, w.actions, w.target, w.W, w.W_T)
    return dict(iK=_f64(f.iK), beta=_f64(f.beta), mu=mu, Sig=Sig, cost_mu=cm, cost_var=cv, J=orc.lcb_objective(cm, cv, w.kappa))


@functools.lru_cache(maxsize=None)
def oracle_result(name):
    """The fp64 numpy oracle on case `name`: the factors and orc.evaluate_candidates' dict."""
    w = make_case(name)
    f = oracle_factors(w)
    return f, orc.evaluate_candidates(f, w)


@functools.lru_cache(maxsize=None)
def oracle_floor(name):
    """|numpy oracle - longdouble truth| in the per-output metric: the floor the GPU results are measured against."""
    f, o = oracle_result(name)
    t = truth(name)
    return dict(iK=err_per_gp(f.iK, t["iK"]), beta=err_per_gp(f.beta, t["beta"]), mu=err_out(o["mu"], t["mu"]),
                Sig=err_cov(o["Sig"], t["Sig"]), cost_mu=err_out(o["cost_mu"][..., None], t["cost_mu"][..., None]),
                cost_var=err_out(o["cost_var"][..., None], t["cost_var"][..., None]), J=err_out(o["J"][:, None], t["J"][:, None]))


# ------------------------------------------------------------------------------------------ the kernels' degree selection
def taylor_degrees(w, mu, Sig, max_arg):
    """The Taylor degree the fused-horizon kernel selects for every output pair a <= b (row-major) at every step of ONE
    trajectory mu (H+1, D), Sig (H+1, D, D): cmax = sum_dd' |Z_dd'| umax_d wmax_d' with Z = R^-1 Sigma and the data range of the
    memory points about the step's mean (csrc/rollout_kernel.h, "chain, P1"); degree 0 = the exact-exp loop (cmax above the last
    entry of `max_arg` = kTaylorMaxArg), otherwise the smallest K whose truncation stays below fp64 rounding.
    Returns (degrees (H, P) int, cmax (H, P), the pairs [(a, b)])."""
    N, D, A, E, _, _ = w.dims
    ils2 = 1.0 / w.lengthscales ** 2
    lo, hi = w.X.min(axis=0)[:D], w.X.max(axis=0)[:D]
    kmax = len(max_arg) - 1
    pairs = [(a, b) for a in range(D) for b in range(a, D)]
    Hs = mu.shape[0] - 1
    deg = np.zeros((Hs, len(pairs)), dtype=int)
    cm = np.zeros((Hs, len(pairs)))
    for t in range(Hs):
        rg = np.maximum(np.abs(lo - mu[t]), np.abs(hi - mu[t]))
        for q, (a, b) in enumerate(pairs):
            R = Sig[t] * (ils2[a, :D] + ils2[b, :D])[None, :] + np.eye(D)
            Z = np.linalg.solve(R, Sig[t])
            c = float(np.sum(np.abs(Z) * np.outer(rg * ils2[a, :D], rg * ils2[b, :D])))
            cm[t, q] = c
            if c <= max_arg[kmax]:
                deg[t, q] = 1 + sum(1 for k in range(1, kmax) if c > max_arg[k])
    return deg, cm, pairs


# ------------------------------------------------------------------------------- inputs shared by the two tiers, per case
def queries(w, seed=1):
    """Query inputs of predict / predict_cov: six random points of the memory's box, three memory points."""
    rng = np.random.default_rng(seed)
    lo, hi = w.X.min(axis=0), w.X.max(axis=0)
    return np.concatenate([lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(6, w.X.shape[1])),
                           w.X[rng.choice(w.X.shape[0], 3, replace=False)]])


def moment_inputs(w, seed=2):
    """Gaussian inputs of the one-step calls, (P, E) and (P, E, E), P = 3: the rollout's own first input (mu0, the first
    action, S0 in the state block) and two random means of the box with dense covariances of a fifth of a lengthscale."""
    N, D, A, E, _, _ = w.dims
    rng = np.random.default_rng(seed)
    lo, hi = w.X.min(axis=0), w.X.max(axis=0)
    mu = lo + (hi - lo) * rng.uniform(0.1, 0.9, size=(3, E))
    mu[0, :D], mu[0, D:D + A] = w.mu0, w.actions[0, 0]
    if w.include_time:
        mu[:, -1] = w.time0
    ls = w.lengthscales.min(axis=0)
    G = rng.standard_normal((3, E, E)) * (0.2 * ls)[None, :, None]
    var = G @ G.transpose(0, 2, 1) + 1e-6 * np.diag(ls ** 2)[None]
    var[0] = 0.0
    var[0, :D, :D] = w.S0
    return mu, var


# ---------------------------------------------------------------------------------------------- wrong hyper-parameters
MUTANTS = ("outputscales_swapped", "noises_swapped", "lengthscale_rows_swapped", "outputscales_mean")


def mutant(w, kind):
    """The hyper-parameter arguments a kernel with that indexing mistake would effectively use (outputs 0 and 1 exchanged)."""
    swap = np.arange(w.Y.shape[1])
    swap[[0, 1]] = [1, 0]
    if kind == "outputscales_swapped":
        return dict(outputscales=w.outputscales[swap])
    if kind == "noises_swapped":
        return dict(noises=w.noises[swap])
    if kind == "lengthscale_rows_swapped":
        return dict(lengthscales=np.ascontiguousarray(w.lengthscales[swap]))
    if kind == "outputscales_mean":
        return dict(outputscales=np.full_like(w.outputscales, w.outputscales.mean()))
    raise KeyError(kind)


# ------------------------------------------------------------------------------------------------------------ tolerances
# Flat bounds: the ones the family's existing GPU test file applies (named behind each), here in the per-output metric.
TOL = {
    "iK": 1e-8, "beta": 1e-8,                                  # test_gpu_parity.py::test_factorisation_*
    "mu": 1e-9, "Sig_cap": 1e-5,                               # test_gpu_parity.py::test_covariances_against_extended_precision
    "cost_mu": 1e-8, "cost_var": 1e-7, "J": 1e-7,              # test_gpu_parity.py::_check_traj
    "predict_mean": 1e-10,                                     # test_gpu_predict.py::test_against_extended_precision
    "moments_M": 1e-9, "moments_V": 1e-9, "moments_S_cap": 1e-5,   # test_gpu_moments.py::test_against_extended_precision
    "grad": 1e-7, "grad_J": 1e-7,                              # test_gpu_gradient.py, test_gpu_rollout_backward.py (TOL)
    "vjp": 1e-7,                                               # the backward test files' TOL
    "mll_loss": 1e-9, "mll_grad": 1e-7,                        # test_gpu_mll_batch.py
}
SIG_FLOOR = 1e-8          # test_covariances_against_extended_precision: 3 * max(reference's error, oracle's error, 1e-8)
VAR_FLOOR = 1e-12         # test_gpu_predict.py: 3 * max(numpy's error, 1e-12 * outputscale)


def three_times(err_numpy, floor):
    """The project's rule where a longdouble truth exists: the HIP result may be 3x as far from it as a plain fp64 evaluation
    (or the floor, where that one is closer than the floor)."""
    return 3.0 * max(float(err_numpy), floor)


# ------------------------------------------------------------------ the one-step quantities: references, metrics and bounds
def err_by_outputscale(a, ref, osc, axis):
    """max |a - ref| / outputscale of the entry's output (`axis`): the scale of test_gpu_predict.py's variance rule."""
    a, ref = _f64(a), _f64(ref)
    shape = [1] * ref.ndim
    shape[axis] = -1
    return float(np.max(np.abs(a - ref) / np.asarray(osc).reshape(shape)))


def err_S_by_outputscale(a, ref, osc):
    """(..., D, D): |a - ref|_ab / sqrt(outputscale_a outputscale_b)."""
    a, ref = _f64(a), _f64(ref)
    return float(np.max(np.abs(a - ref) / np.sqrt(np.outer(osc, osc))))


def one_step(w, fa, dtype=np.float64):
    """What predict, predict_cov, moments and moments_linear return at `queries(w)` / `moment_inputs(w)` from the factors
    fa = (X, lengthscales, outputscales, iK, beta), evaluated in `dtype` (float64 or longdouble) by the references the
    families' own test files use: dict key -> array."""
    import linear_moments_ref as lin
    from predict_cov_ref import closed_form_cov
    from moments_fd import xfactors
    X, ls, osc, iK, beta = fa
    Xq = queries(w)
    mu, var = moment_inputs(w)
    out = {}
    M, _, _, v = lin.step(X, ls, osc, iK, beta, Xq, None, dtype=dtype)
    out["predict_mean"], out["predict_var"] = M, v
    out["predict_cov"] = closed_form_cov(X, ls, osc, iK, Xq, dtype=dtype)
    out["linear_M"], out["linear_S"], out["linear_V"] = lin.step(X, ls, osc, iK, beta, mu, var, dtype=dtype)[:3]
    if dtype is np.longdouble:
        fx = xfactors(X, ls, osc, iK, beta)
        res = [xp.moment_match_step(fx, xp._ld(mu[p]), xp._ld(var[p])) for p in range(mu.shape[0])]
        out["moments_M"], out["moments_S"], out["moments_V"] = (np.stack([r[k] for r in res]) for k in range(3))
    else:
        f = orc.Factors(X, None, ls, osc, np.zeros(len(osc)), iK=iK, beta=beta)
        out["moments_M"], out["moments_S"], out["moments_V"] = orc.moment_match_step(f, mu, var)
    return out


def one_step_error(key, a, ref, osc):
    """The per-output error of quantity `key` of `one_step`."""
    if key in ("predict_mean", "linear_M", "linear_V", "moments_M", "moments_V"):
        return err_out(a, ref)
    if key == "predict_var":
        return err_by_outputscale(a, ref, osc, -1)
    if key == "predict_cov":
        return err_by_outputscale(a, ref, osc, 0)
    if key == "linear_S":
        return err_S_by_outputscale(a, ref, osc)
    if key == "moments_S":
        return err_cov(a, ref)
    raise KeyError(key)


def _groups(key, D):
    """Index tuples that select one output (one output pair for the (..., D, D) arrays) of quantity `key`."""
    if key == "predict_cov":
        return [(a,) for a in range(D)]
    if key in ("linear_S", "moments_S"):
        return [(Ellipsis, a, b) for a in range(D) for b in range(D)]
    return [(Ellipsis, a) for a in range(D)]


def one_step_share(key, a, r64, rld, osc):
    """max over the outputs (output pairs) of |a - longdouble| / bound, the bound being the one of the family's own test file
    applied to EVERY OUTPUT ON ITS OWN: <= 1 passes.  `a` against the longdouble reference `rld`; `r64` is the plain fp64 numpy
    evaluation whose own error the 3x rule is about.
      predict_mean, moments_M, moments_V: TOL[key] of the output's own largest magnitude;
      predict_var, predict_cov, linear_S: 3 max(numpy's error on that output, 1e-12 max(outputscales))   (test_gpu_predict.py,
                                          test_gpu_predict_cov.py, test_gpu_moments_linear.py: their floor, verbatim);
      linear_M, linear_V:                 3 max(numpy's error on that output, 1e-12 max|reference|)       (test_gpu_moments_linear.py);
      moments_S:                          min(1e-5, 3 max(numpy's error, 1e-8)) of sqrt(max|S_aa| max|S_bb|) (test_gpu_moments.py's
                                          cap, test_gpu_parity.py's rule for the same covariance).
    The floor of the variance-type quantities stays those files' 1e-12 max(outputscales), not 1e-12 outputscale_a: the rounding of
    outputscale_a - k^T iK_a k scales with sum |terms| ~ outputscale_a^2 / noise_a, and for the output (0.004, 1e-6) of "n70_d2_rev"
    two fp64 summation orders on the CPU already differ by more than a per-output floor would allow (numpy 1.1e-12, a sequential
    sum 1.9e-12 of outputscale_a; the kernel 3.3e-12).  What is per output is the comparison with numpy's error."""
    a, r64, rld = _f64(a), _f64(r64), _f64(rld)
    D = len(osc)
    if key == "moments_S":
        return err_cov(a, rld) / min(TOL["moments_S_cap"], three_times(err_cov(r64, rld), SIG_FLOOR))
    share = 0.0
    for g in _groups(key, D):
        e_hip, e_np = float(np.max(np.abs(a[g] - rld[g]))), float(np.max(np.abs(r64[g] - rld[g])))
        if key in ("predict_mean", "moments_M", "moments_V"):
            bound = TOL[key] * float(np.max(np.abs(rld[g])))
        elif key in ("linear_M", "linear_V"):
            bound = three_times(e_np, VAR_FLOOR * float(np.max(np.abs(rld))))
        else:
            bound = three_times(e_np, VAR_FLOOR * float(np.max(osc)))
        share = max(share, e_hip / bound if np.isfinite(e_hip) else np.inf)
    return share
