"""Tier 2 (GPU): every kernel family with hyper-parameters that differ per output (tests/hetero_cases.py).

Until this file no test told one output's outputscale or noise from another's: make_workload and every fixture give all outputs
the same values, so a kernel reading var[0] for every output, var[a] where var[b] belongs or noise a for output b passed.  Here
the outputscales span 150x ... 225x, the noises 4000x ... 10000x and the lengthscales 0.15 ... 4 over the outputs of one model, the
pairs of a step take different Taylor degrees and forms (tests/test_hetero_reference.py proves that, and that a reference with such
a mistake misses every bound below by 1e4 or more), and each case also runs with its outputs in the opposite order.

Metric: every entry is scaled by its OWN outputs (hetero_cases.err_out / err_cov / err_per_gp / err_by_outputscale), so that an
error in a small-variance output cannot hide behind a large-variance one.  Bounds: hetero_cases.TOL -- the constants of each
family's existing test file -- and, where a longdouble truth exists, the project's rule |HIP - truth| <= 3 max(|numpy - truth|,
floor).  Truth and references are computed here on the CPU, once per case; every achieved error goes to the parity report next
to the numpy oracle's error against the same truth."""
import numpy as np
import pytest

import hetero_cases as hc
from helpers import rel_err, record
from oracle import adjoint
from oracle import gp_training

pytestmark = pytest.mark.gpu

SMALL = [n for n in hc.NAMES if hc.BASE[n.replace("_rev", "")][1] <= 4]            # D <= 4: the compile-time units


@pytest.fixture(scope="module")
def engine():
    import gp_mpc_amd
    eng = gp_mpc_amd.HipEngine(0)
    yield eng
    eng.close()


def _np(t):
    return t.detach().cpu().numpy()


def _options(engine, opts, fn):
    """fn() under the engine options `opts`; every one of them is 0 (= automatic) afterwards, the gradient switches 1."""
    defaults = {"grad_separable": 1, "grad_tiles": 1}
    for k, v in opts.items():
        engine.set_option(k, v)
    try:
        return fn()
    finally:
        for k in opts:
            engine.set_option(k, defaults.get(k, 0))


def _load(engine, name, load_by):
    """The model of case `name` on the engine; returns the factors the engine then holds, as fp64 numpy (X, ls, os, iK, beta)."""
    w = hc.make_case(name)
    if load_by == "set_factors":
        t = hc.truth(name)
        engine.set_factors(w.X, t["iK"], t["beta"], w.lengthscales, w.outputscales)
        iK, beta = t["iK"], t["beta"]
    else:
        engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        iK, beta = (_np(x) for x in engine.factors())
    engine.set_cost(w.target, w.W, w.W_T, w.kappa)
    return w, (w.X, w.lengthscales, w.outputscales, iK, beta)


# ----------------------------------------------------------------------------------------------------------- factorisation
# (path, options, memory prepared first (rows short of N) or None, last_prepare_mode, cases).  The panel chain is forced below its
# crossover with the single-launch kernel as tests/test_gpu_parity.py forces it, at the sizes it forces it (N >= 65).
PREPARE_PATHS = [("full", {}, None, 0, hc.NAMES),
                 ("panel_chain", {"fused_prepare": 0}, None, 0, [n for n in hc.NAMES if hc.BASE[n.replace("_rev", "")][0] >= 65]),
                 ("border_update", {}, 6, 1, hc.NAMES)]
PREPARE_PARAMS = [(path, name) for path in PREPARE_PATHS for name in path[4]]


@pytest.mark.parametrize("path,name", PREPARE_PARAMS, ids=[f"{p[0]}-{n}" for p, n in PREPARE_PARAMS])
def test_factorisation(name, path):
    import gp_mpc_amd
    _, opts, grow, mode, _ = path
    w, t, floor = hc.make_case(name), hc.truth(name), hc.oracle_floor(name)
    N = w.X.shape[0]
    eng = gp_mpc_amd.HipEngine(0)
    try:
        if "fused_prepare" in opts:
            eng.set_option("incremental", 0)
        for k, v in opts.items():
            eng.set_option(k, v)
        if grow:
            eng.prepare(w.X[:N - grow], w.Y[:N - grow], w.lengthscales, w.outputscales, w.noises)
            assert eng.last_prepare_mode == 0
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        assert eng.last_prepare_mode == mode
        iK, beta = (_np(x) for x in eng.factors())
    finally:
        eng.close()
    e_iK, e_beta = hc.err_per_gp(iK, t["iK"]), hc.err_per_gp(beta, t["beta"])
    record(f"hetero_factorisation[{name},{path[0]}]", iK=e_iK, beta=e_beta, numpy_iK=floor["iK"], numpy_beta=floor["beta"])
    print(f"{name} {path[0]}: iK {e_iK:.2e} (numpy {floor['iK']:.2e}) beta {e_beta:.2e} (numpy {floor['beta']:.2e})")
    assert e_iK <= hc.TOL["iK"] and e_beta <= hc.TOL["beta"]
    assert np.array_equal(iK, iK.transpose(0, 2, 1))


# ------------------------------------------------------------------------------- posterior and one moment-matched step
@pytest.mark.parametrize("load_by", ["prepare", "set_factors"])
@pytest.mark.parametrize("name", hc.NAMES)
def test_posterior_and_one_step(engine, name, load_by):
    """predict (with and without noises=), predict_cov, moments at force_path 0 / 1 / 2 and moments_linear against the
    references of their own test files, evaluated in longdouble and in fp64 on the factors the engine holds."""
    w, fa = _load(engine, name, load_by)
    osc = w.outputscales
    Xq = hc.queries(w)
    mu, var = hc.moment_inputs(w)
    r64, rld = hc.one_step(w, fa), hc.one_step(w, fa, dtype=np.longdouble)
    got = {}
    p = engine.predict(Xq)
    got["predict_mean"], got["predict_var"] = _np(p["mean"]), _np(p["var"])
    got["predict_cov"] = _np(engine.predict_cov(Xq))
    lin = engine.moments_linear(mu, var)
    got["linear_M"], got["linear_S"], got["linear_V"] = (_np(lin[k]) for k in ("M", "S", "V"))
    for fp in (0, 1, 2):
        mm = _options(engine, {"force_path": fp}, lambda: engine.moments(mu, var))
        for k in ("M", "S", "V"):
            got[f"moments_{k}@path{fp}"] = _np(mm[k])
    errs, failed = {}, []
    for key, val in got.items():
        base = key.split("@")[0]
        errs[key] = hc.one_step_error(base, val, rld[base], osc)
        errs["numpy_" + base] = hc.one_step_error(base, r64[base], rld[base], osc)
        errs["share_of_bound_" + key] = share = hc.one_step_share(base, val, r64[base], rld[base], osc)
        print(f"{name} {load_by} {key}: hip {errs[key]:.2e} numpy {errs['numpy_' + base]:.2e} share of the bound {share:.3f}")
        if not share <= 1.0:
            failed.append((key, errs[key], errs["numpy_" + base], share))
    # the noise of likelihood(model(x)): output a's own, added to the variance and to the joint covariance's diagonal
    pn = _np(engine.predict(Xq, noises=w.noises)["var"])
    cn = _np(engine.predict_cov(Xq, noises=w.noises))
    eye = np.eye(len(Xq))[None] * w.noises[:, None, None]
    for k, base, val, add in (("predict_var_noisy", "predict_var", pn, w.noises[None, :]), ("predict_cov_noisy", "predict_cov", cn, eye)):
        errs[k] = hc.one_step_error(base, val, rld[base] + add, osc)
        errs["share_of_bound_" + k] = share = hc.one_step_share(base, val, r64[base] + add, rld[base] + add, osc)
        if not share <= 1.0:
            failed.append((k, errs[k], share))
    record(f"hetero_one_step[{name},{load_by}]", **errs)
    assert not failed, failed


def _hot(shape, a, axes, rng):
    """A random cotangent of `shape` that is zero except where one of `axes` has index a (output a alone)."""
    full = rng.standard_normal(shape)
    mask = np.zeros(shape, dtype=bool)
    for ax in axes:
        idx = [slice(None)] * len(shape)
        idx[ax] = a
        mask[tuple(idx)] = True
    return np.where(mask, full, 0.0)


@pytest.mark.parametrize("name", hc.NAMES)
def test_one_step_gradients(engine, name):
    """predict_backward, moments_backward and moments_linear_backward with cotangents that select ONE output at a time (the result
    lives in input space, so this is what scales it by its own output): against the closed form of test_gpu_predict_backward.py
    in longdouble, longdouble differences (tests/moments_fd.py) and torch autograd (tests/linear_moments_torch_ref.py)."""
    import linear_moments_torch_ref as lin_t
    from moments_fd import xfactors, directional, directions
    from test_gpu_predict_backward import closed_form_grad
    w, fa = _load(engine, name, "prepare")
    N, D, A, E, _, _ = w.dims
    Xq = hc.queries(w)
    mu, var = hc.moment_inputs(w)
    P = mu.shape[0]
    fx = xfactors(*fa)
    ls = w.lengthscales.min(axis=0)
    rng = np.random.default_rng(77)
    errs, failed = {}, []
    for a in range(D):
        # predict_backward: the rule of test_gpu_predict_backward.py::test_against_extended_precision
        mb, vb = _hot((len(Xq), D), a, (1,), rng), _hot((len(Xq), D), a, (1,), rng)
        got = _np(engine.predict_backward(Xq, mb, vb))
        g64, gld = closed_form_grad(*fa, Xq, mb, vb), closed_form_grad(*fa, Xq, mb, vb, dtype=np.longdouble)
        scale = float(np.max(np.abs(gld)))
        e_hip, e_np = float(np.max(np.abs(got - gld))) / scale, float(np.max(np.abs(g64 - gld))) / scale
        errs[f"predict_backward_out{a}"], errs[f"numpy_predict_backward_out{a}"] = e_hip, e_np
        if not e_hip <= 4 * max(e_np, 1e-12):
            failed.append(("predict_backward", a, e_hip, e_np))
        # moments_backward: directional longdouble differences, 1e-7 of the terms' scale (test_extended_precision_medium)
        Mb, Sb, Vb = _hot((P, D), a, (1,), rng), _hot((P, D, D), a, (1, 2), rng), _hot((P, E, D), a, (2,), rng)
        out = engine.moments_backward(mu, var, Mb, Sb, Vb)
        worst = 0.0
        for p in range(P):
            dm, ds = directions(E, ls, rng)
            fd = directional(fx, mu[p], var[p], Mb[p], Sb[p], Vb[p], dm, 0 * ds, 1e-6) + \
                directional(fx, mu[p], var[p], Mb[p], Sb[p], Vb[p], 0 * dm, ds, 1e-6)
            mbar, vbar = _np(out["mu_bar"][p]), _np(out["var_bar"][p])
            an = float(mbar @ dm + (vbar * ds).sum())
            sc = float(np.abs(mbar) @ np.abs(dm) + (np.abs(vbar) * np.abs(ds)).sum())
            worst = max(worst, abs(an - fd) / sc)
        errs[f"moments_backward_out{a}"] = worst
        if not worst <= hc.TOL["vjp"]:
            failed.append(("moments_backward", a, worst))
        # moments_linear_backward: torch autograd of the fp64 restatement, 1e-7 of each array's scale
        mb_ref, vb_ref = lin_t.step_vjp(fa, mu, var, M_bar=Mb, S_bar=Sb, V_bar=Vb)
        lout = engine.moments_linear_backward(mu, var, Mb, Sb, Vb)
        e = max(rel_err(_np(lout["mu_bar"]), mb_ref), rel_err(_np(lout["var_bar"]), vb_ref))
        errs[f"moments_linear_backward_out{a}"] = e
        if not e <= hc.TOL["vjp"]:
            failed.append(("moments_linear_backward", a, e))
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    record(f"hetero_one_step_gradients[{name}]", **errs)
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------------------ rollout
FUSED, STREAM, TILES = 0, 1, 2
# (id, options, candidates, cases, expected last_rollout_path, expected last_cluster or None, more than one pair group)
ROLLOUT_ROWS = [("default", {}, hc.B, hc.NAMES, None, None, False)]
for _fp in (0, 1, 2):
    for _nt in (256, 1024):
        ROLLOUT_ROWS.append((f"path{_fp}_threads{_nt}", {"force_path": _fp, "threads": _nt, "cluster": 1}, hc.B, SMALL, FUSED, 1, False))
    ROLLOUT_ROWS.append((f"path{_fp}_rows16", {"force_path": _fp, "rows_per_chunk": 16, "cluster": 1}, hc.B, ["n130_d3", "n130_d3_rev"],
                         FUSED, 1, False))
ROLLOUT_ROWS += [
    ("cooperative", {"rows_per_chunk": 16, "cluster": 2}, 1, ["n130_d3", "n130_d3_rev"], FUSED, 2, False),
    ("pair_groups", {"threads": 256, "lds_limit_kb": 44, "cluster": 1}, hc.B, ["n130_d3", "n130_d3_rev"], FUSED, 1, True),
    ("pair_groups_path1", {"force_path": 1, "threads": 256, "lds_limit_kb": 48, "cluster": 1}, hc.B, ["n130_d3", "n130_d3_rev"], FUSED, 1, True),
    ("streaming", {"force_global_scratch": 1}, hc.B, hc.NAMES, STREAM, None, False),
    ("batch_major", {"pair_tiles": 1}, hc.B, SMALL, TILES, None, False),
]
ROLLOUT_PARAMS = [(row, name, load_by) for row in ROLLOUT_ROWS for name in row[3]
                  for load_by in (("prepare", "set_factors") if row[0] in ("default", "path0_threads256", "batch_major") else ("prepare",))]


def _check_trajectory(tag, name, out, nB, errs_extra=None):
    """mu, Sig against the longdouble truth; the costs against gpmpc_oracle's on the truth trajectory."""
    t, floor = hc.truth(name), hc.oracle_floor(name)
    e = dict(mu=hc.err_out(_np(out["mu"]), t["mu"][:nB]), Sig=hc.err_cov(_np(out["Sig"]), t["Sig"][:nB]),
             cost_mu=rel_err(_np(out["cost_mu"]), t["cost_mu"][:nB]), cost_var=rel_err(_np(out["cost_var"]), t["cost_var"][:nB]),
             J=rel_err(_np(out["J"]), t["J"][:nB]))
    sig_bound = min(hc.TOL["Sig_cap"], hc.three_times(floor["Sig"], hc.SIG_FLOOR))
    record(tag, **e, numpy_mu=floor["mu"], numpy_Sig=floor["Sig"], numpy_J=floor["J"], **(errs_extra or {}))
    print(tag, {k: f"{v:.2e}" for k, v in e.items()}, f"numpy mu {floor['mu']:.2e} Sig {floor['Sig']:.2e}; Sig bound {sig_bound:.2e}")
    assert e["mu"] <= hc.TOL["mu"], e
    assert e["Sig"] <= sig_bound, (e, sig_bound)
    assert e["cost_mu"] <= hc.TOL["cost_mu"] and e["cost_var"] <= hc.TOL["cost_var"] and e["J"] <= hc.TOL["J"], e
    S = _np(out["Sig"])
    assert np.array_equal(S, np.swapaxes(S, -1, -2))


@pytest.mark.parametrize("row,name,load_by", ROLLOUT_PARAMS, ids=[f"{r[0]}-{n}-{l}" for r, n, l in ROLLOUT_PARAMS])
def test_rollout(engine, row, name, load_by):
    rid, opts, nB, _, path, cluster, groups = row
    w, _ = _load(engine, name, load_by)

    def run():
        out = engine.rollout(w.actions[:nB], w.mu0, w.S0, w.include_time, w.time0)
        return out, engine.last_rollout_path, engine.last_cluster, engine.last_pair_groups
    out, got_path, got_cluster, got_groups = _options(engine, opts, run)
    if path is not None:
        assert got_path == path, (got_path, path)
    if cluster is not None:
        assert got_cluster == cluster, (got_cluster, cluster)
    if groups:
        assert got_groups > 1, got_groups
    _check_trajectory(f"hetero_rollout[{rid},{name},{load_by}]", name, out, nB)


# ---------------------------------------------------------------------------------------------------------------- gradients
# (id, options, cases, last_grad_path bit that must be set or 0)
GRAD_ROWS = [
    ("default", {}, hc.NAMES, 0),
    ("stream", {"grad_stream": 1}, SMALL, 4),
    ("separable", {"grad_separable": 2}, SMALL, 1),
    ("elementwise", {"grad_separable": 0}, SMALL, 0),
    ("tiles", {"grad_tiles": 2, "pair_tiles": 2}, SMALL, 2),
    ("tiles_fused", {"grad_tiles": 2, "pair_tiles": 1}, SMALL, 16),
]
GRAD_PARAMS = [(row, name) for row in GRAD_ROWS for name in row[2]]


@pytest.mark.parametrize("row,name", GRAD_PARAMS, ids=[f"{r[0]}-{n}" for r, n in GRAD_PARAMS])
def test_rollout_grad(engine, row, name):
    """rollout_grad against oracle.adjoint.lcb_and_gradient on the oracle's factors (as tests/test_gpu_gradient.py)."""
    rid, opts, _, bit = row
    w = hc.make_case(name)
    f = hc.oracle_result(name)[0]
    engine.set_factors(w.X, f.iK, f.beta, w.lengthscales, w.outputscales)
    engine.set_cost(w.target, w.W, w.W_T, w.kappa)

    def run():
        out = engine.rollout_grad(w.actions, w.mu0, w.S0, w.include_time, w.time0)
        return _np(out["J"]), _np(out["grad"]), engine.last_grad_path
    J, grad, gpath = _options(engine, opts, run)
    if bit:
        assert gpath & bit, (gpath, bit)
    eJ, eg = 0.0, 0.0
    for b in range(hc.B):
        J0, g0, *_ = adjoint.lcb_and_gradient(f, w.actions[b], w.mu0, w.S0, w.target, w.W, w.W_T, w.kappa, w.include_time, w.time0)
        eJ, eg = max(eJ, abs(J[b] - J0) / abs(J0)), max(eg, rel_err(grad[b], g0))
    record(f"hetero_rollout_grad[{rid},{name}]", J=eJ, grad=eg)
    print(f"{rid} {name}: J {eJ:.2e} grad {eg:.2e}")
    assert eJ <= hc.TOL["grad_J"] and eg <= hc.TOL["grad"]


@pytest.mark.parametrize("name", hc.NAMES)
def test_rollout_backward(engine, name):
    """rollout_backward with cotangents of ONE output at a time against tests/traj_vjp.py."""
    from traj_vjp import traj_vjp
    w = hc.make_case(name)
    N, D, A, E, H, B = w.dims
    f = hc.oracle_result(name)[0]
    engine.set_factors(w.X, f.iK, f.beta, w.lengthscales, w.outputscales)
    engine.set_cost(w.target, w.W, w.W_T, w.kappa)
    rng = np.random.default_rng(91)
    errs, failed = {}, []
    for a in range(D):
        mu_bar, Sig_bar = _hot((B, H + 1, D), a, (2,), rng), _hot((B, H + 1, D, D), a, (2, 3), rng)
        out = engine.rollout_backward(w.actions, w.mu0, w.S0, w.include_time, w.time0, mu_bar=mu_bar, Sig_bar=Sig_bar)
        worst = 0.0
        for b in (0, B - 1):
            ga, gm, gS = traj_vjp(f, w.actions[b], w.mu0, w.S0, w.target, w.W, w.W_T, w.kappa, mu_bar[b], Sig_bar[b],
                                  include_time=w.include_time, time0=w.time0)
            worst = max(worst, rel_err(_np(out["actions_bar"][b]), ga), rel_err(_np(out["mu0_bar"][b]), gm),
                        rel_err(_np(out["S0_bar"][b]), gS))
        errs[f"out{a}"] = worst
        if not worst <= hc.TOL["vjp"]:
            failed.append((a, worst))
    # and the cost seeds, which touch every output at once
    sd = dict(cost_mu_bar=rng.standard_normal((B, H + 1)), cost_var_bar=rng.standard_normal((B, H + 1)), J_bar=rng.standard_normal(B))
    out = engine.rollout_backward(w.actions, w.mu0, w.S0, w.include_time, w.time0, **sd)
    worst = 0.0
    for b in (0, B - 1):
        ga, gm, gS = traj_vjp(f, w.actions[b], w.mu0, w.S0, w.target, w.W, w.W_T, w.kappa, None, None, sd["cost_mu_bar"][b],
                              sd["cost_var_bar"][b], sd["J_bar"][b], w.include_time, w.time0)
        worst = max(worst, rel_err(_np(out["actions_bar"][b]), ga), rel_err(_np(out["mu0_bar"][b]), gm),
                    rel_err(_np(out["S0_bar"][b]), gS))
    errs["cost_seeds"] = worst
    if not worst <= hc.TOL["vjp"]:
        failed.append(("cost_seeds", worst))
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    record(f"hetero_rollout_backward[{name}]", **errs)
    assert not failed, failed


# ------------------------------------------------------------------------------ linearised and closed-loop propagation
LINEAR_NAMES = ["n33_d3", "n33_d3_rev", "n66_d4", "n66_d4_rev"]


def _per_output_share(got, r64, rld, pairs, floor_scale):
    """The rule of tests/test_gpu_rollout_linear.py / _linear_feedback.py / _lqr_gains.py, |HIP - longdouble| <= 3 max(|numpy -
    longdouble|, 1e-12 max|longdouble|), applied to every output (output pair) on its own: the largest |HIP - longdouble| / bound."""
    got, r64, rld = (np.asarray(x, dtype=np.float64) for x in (got, r64, rld))
    D = rld.shape[-1]
    share = 0.0
    for g in ([(Ellipsis, a, b) for a in range(D) for b in range(D)] if pairs else [(Ellipsis, a) for a in range(D)]):
        e_hip, e_np = float(np.max(np.abs(got[g] - rld[g]))), float(np.max(np.abs(r64[g] - rld[g])))
        share = max(share, e_hip / hc.three_times(e_np, hc.VAR_FLOOR * floor_scale))
    return share


def _gains_of(w, seed=5):
    N, D, A, E, H, B = w.dims
    return 0.5 * np.random.default_rng(seed).standard_normal((B, H, A, D))


@pytest.mark.parametrize("name", LINEAR_NAMES)
def test_linearised_and_closed_loop_forward(engine, name):
    """rollout_linear, rollout_linear_feedback, rollout_feedback and lqr_gains against the restatements of their own test files
    in longdouble (tests/linear_moments_ref.py, feedback_rollout_ref.py, feedback_mm_ref.py, lqr_gains_ref.py)."""
    import feedback_mm_ref as fm
    import feedback_rollout_ref as fb
    import linear_moments_ref as lin
    import lqr_gains_ref as lq
    from moments_fd import xfactors
    w, fa = _load(engine, name, "prepare")
    K = _gains_of(w)
    args = (w.mu0, w.S0, w.include_time, w.time0)
    errs, failed = {}, []

    def three_times_rule(tag, got, r64, rld, pairs):
        got, rld = np.asarray(got, dtype=np.float64), np.asarray(rld, dtype=np.float64)
        metric = hc.err_cov if pairs else hc.err_out
        errs[tag], errs["numpy_" + tag] = metric(got, rld), metric(r64, rld)
        errs["share_of_bound_" + tag] = share = _per_output_share(got, r64, rld, pairs, float(np.max(np.abs(rld))))
        if not share <= 1.0:
            failed.append((tag, errs[tag], errs["numpy_" + tag], share))

    out = engine.rollout_linear(w.actions, *args)
    m64, S64 = lin.rollout(*fa, w.actions, *args)
    mld, Sld = lin.rollout(*fa, w.actions, *args, dtype=np.longdouble)
    three_times_rule("linear_mu", _np(out["mu"]), m64, mld, False)
    three_times_rule("linear_Sig", _np(out["Sig"]), S64, Sld, True)

    out = engine.rollout_linear_feedback(w.actions, K, *args)
    m64, S64 = fb.rollout(*fa, w.actions, K, *args)
    mld, Sld = fb.rollout(*fa, w.actions, K, *args, dtype=np.longdouble)
    three_times_rule("linear_feedback_mu", _np(out["mu"]), m64, mld, False)
    three_times_rule("linear_feedback_Sig", _np(out["Sig"]), S64, Sld, True)

    out = engine.lqr_gains(w.actions, w.mu0, w.include_time, w.time0, 1e-3, want_cost_to_go=True, want_flags=True)
    assert not _np(out["flags"]).any()
    largs = (w.actions, w.mu0, w.W, w.W_T, w.include_time, w.time0, 1e-3)
    K64, P64, _ = lq.gains(*fa, *largs)
    Kld, Pld, _ = lq.gains(*fa, *largs, dtype=np.longdouble)
    three_times_rule("lqr_gains", _np(out["gains"]), K64, Kld, False)
    three_times_rule("lqr_cost_to_go", _np(out["P"]), P64, Pld, True)

    # moment matching in closed loop: the bounds of the open-loop rollout (1e-9 means; covariances 3x the fp64 recurrence's error)
    out = engine.rollout_feedback(w.actions, K, *args)
    f64 = hc.orc.Factors(fa[0], None, fa[1], fa[2], np.zeros(len(fa[2])), iK=fa[3], beta=fa[4])
    m64, S64 = fm.rollout(f64, w.actions, K, *args)
    mld, Sld = (np.asarray(x, dtype=np.float64) for x in fm.rollout_extended(xfactors(*fa), w.actions, K, *args))
    errs["feedback_mu"], errs["numpy_feedback_mu"] = hc.err_out(_np(out["mu"]), mld), hc.err_out(m64, mld)
    errs["feedback_Sig"], errs["numpy_feedback_Sig"] = hc.err_cov(_np(out["Sig"]), Sld), hc.err_cov(S64, Sld)
    if not errs["feedback_mu"] <= hc.TOL["mu"]:
        failed.append(("feedback_mu", errs["feedback_mu"]))
    if not errs["feedback_Sig"] <= min(hc.TOL["Sig_cap"], hc.three_times(errs["numpy_feedback_Sig"], hc.SIG_FLOOR)):
        failed.append(("feedback_Sig", errs["feedback_Sig"], errs["numpy_feedback_Sig"]))
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    record(f"hetero_linear_and_closed_loop[{name}]", **errs)
    assert not failed, failed


@pytest.mark.parametrize("name", LINEAR_NAMES)
def test_linearised_and_closed_loop_backward(engine, name):
    """rollout_linear_backward, rollout_linear_feedback_backward and rollout_feedback_backward against torch autograd of their
    restatements, with trajectory cotangents of ONE output at a time and once with the cost cotangents: 1e-7 of each array."""
    import feedback_mm_torch_ref as fmt
    import feedback_rollout_torch_ref as fbt
    import linear_moments_ref as lin
    import linear_moments_torch_ref as lin_t
    w, fa = _load(engine, name, "prepare")
    N, D, A, E, H, B = w.dims
    K = _gains_of(w)
    cfg = lin.reward_config_of(w)
    args = (w.mu0, w.S0, w.include_time, w.time0)
    rng = np.random.default_rng(93)
    seeds = [(f"out{a}", dict(mu_bar=_hot((B, H + 1, D), a, (2,), rng), Sig_bar=_hot((B, H + 1, D, D), a, (2, 3), rng)))
             for a in range(D)]
    seeds.append(("cost_seeds", dict(cost_mu_bar=rng.standard_normal((B, H + 1)), cost_var_bar=rng.standard_normal((B, H + 1)),
                                     J_bar=rng.uniform(0.5, 1.5, size=B))))
    families = [
        ("linear", ("actions_bar", "mu0_bar", "S0_bar"),
         lambda sd: engine.rollout_linear_backward(w.actions, *args, **sd),
         lambda sd: lin_t.rollout_vjp(fa, cfg, w.actions, *args, **sd)),
        ("linear_feedback", ("actions_bar", "gains_bar", "mu0_bar", "S0_bar"),
         lambda sd: engine.rollout_linear_feedback_backward(w.actions, K, *args, **sd),
         lambda sd: fbt.rollout_vjp(fa, cfg, w.actions, K, *args, **sd)),
        ("feedback", ("actions_bar", "gains_bar", "mu0_bar", "S0_bar"),
         lambda sd: engine.rollout_feedback_backward(w.actions, K, *args, **sd),
         lambda sd: fmt.rollout_vjp(fa, cfg, w.actions, K, *args, **sd)),
    ]
    errs, failed = {}, []
    for fam, keys, run, ref in families:
        for tag, sd in seeds:
            out, want = run(sd), ref(sd)
            worst = max(rel_err(_np(out[k]), x) for k, x in zip(keys, want))
            errs[f"{fam}_{tag}"] = worst
            if not worst <= hc.TOL["vjp"]:
                failed.append((fam, tag, worst))
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    record(f"hetero_linear_and_closed_loop_backward[{name}]", **errs)
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------ sparse and training
@pytest.mark.parametrize("name", hc.NAMES)
def test_sparse_model_predict(name):
    """prepare_sparse on M = 16 inducing points, then predict, against tests/sparse_gp_ref.py in longdouble: the bound of
    tests/test_gpu_prepare_sparse.py (10x the fp64 restatement's own error + 64 eps), per output."""
    import gp_mpc_amd
    import sparse_gp_ref as sp
    w = hc.make_case(name)
    N, D = w.X.shape[0], w.Y.shape[1]
    Z = w.X[sp.strided_rows(N, 16)]
    Xq = hc.queries(w)
    args = (w.X, w.Y, Z, w.lengthscales, w.outputscales, w.noises, 1e-6)
    ref = {}
    for dt in (np.float64, np.longdouble):
        iK, beta = sp.sparse_factors(*args, dtype=dt)
        ref[dt] = sp.predict(Z, w.lengthscales, w.outputscales, iK, beta, Xq, dtype=dt)
    eng = gp_mpc_amd.HipEngine(0)
    try:
        eng.prepare_sparse(w.X, w.Y, Z, w.lengthscales, w.outputscales, w.noises, jitter_rel=1e-6)
        assert eng.last_prepare_mode == 4
        p = eng.predict(Xq)
        mean, var = _np(p["mean"]), _np(p["var"])
    finally:
        eng.close()
    eps = np.finfo(np.float64).eps
    errs, failed = {}, []
    for k, got, r64, rld in (("mean", mean, ref[np.float64][0], ref[np.longdouble][0]), ("var", var, ref[np.float64][1], ref[np.longdouble][1])):
        rld = np.asarray(rld, dtype=np.float64)
        for a in range(D):
            e_hip, e_np = float(np.max(np.abs(got[:, a] - rld[:, a]))), float(np.max(np.abs(np.asarray(r64, float)[:, a] - rld[:, a])))
            scale = float(np.max(np.abs(rld[:, a])))
            errs[f"{k}_out{a}"], errs[f"numpy_{k}_out{a}"] = e_hip / scale, e_np / scale
            if not e_hip <= 10.0 * e_np + 64.0 * eps * scale:
                failed.append((k, a, e_hip, e_np, scale))
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    record(f"hetero_sparse_predict[{name}]", **errs)
    assert not failed, failed


@pytest.mark.parametrize("name", hc.NAMES)
def test_training_loss(engine, name):
    """mll against oracle.gp_training.neg_mll_and_grad, output by output (the bounds of tests/test_gpu_mll_batch.py)."""
    w = hc.make_case(name)
    N, D, A, E, _, _ = w.dims
    out = engine.mll(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    errs, failed = {}, []
    for a in range(D):
        loss, g_ls, g_os, g_nz = gp_training.neg_mll_and_grad(w.X, w.Y[:, a], w.lengthscales[a], w.outputscales[a], w.noises[a])
        e = dict(loss=abs(out["loss"][a] - loss) / abs(loss), d_lengthscale=rel_err(out["d_lengthscale"][a], g_ls),
                 d_outputscale=abs(out["d_outputscale"][a] - g_os) / abs(g_os), d_noise=abs(out["d_noise"][a] - g_nz) / abs(g_nz))
        for k, v in e.items():
            errs[f"{k}_out{a}"] = v
            if not v <= (hc.TOL["mll_loss"] if k == "loss" else hc.TOL["mll_grad"]):
                failed.append((k, a, v))
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    record(f"hetero_mll[{name}]", **errs)
    assert not failed, failed
