"""Tier 2 (GPU): gpmpc_moments_linear -- the first-order (linearised) propagation of a Gaussian input through the GP posterior.

Checked against the long-double restatement of tests/linear_moments_ref.py (tied to the reference's golden, to finite
differences and to the oracle's moment matching by tests/test_linear_moments_reference.py), against the entries that compute the
same quantities another way (gpmpc_predict, gpmpc_predict_backward, gpmpc_moments at zero input variance), and against the
contracts of include/gpmpc.h: exact symmetry, bitwise batch invariance, outputs that may be NULL, errors, no interference.
"""
import numpy as np
import pytest
import torch

import linear_moments_ref as lin
from helpers import load, workload_of, rel_err, record
from oracle import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import gp_mpc_amd
    eng = gp_mpc_amd.HipEngine(0)
    yield eng
    eng.close()


def _fresh():
    import gp_mpc_amd
    return gp_mpc_amd.HipEngine(0)


def _np(t):
    return t.cpu().numpy()


def _inputs(w, P, seed, scale=1e-3):
    """P input means inside the data range (the last few: memory points) and dense SPD input covariances of size `scale`."""
    rng = np.random.default_rng(seed)
    E = w.X.shape[1]
    lo, hi = w.X.min(axis=0), w.X.max(axis=0)
    mu = lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(P, E))
    n_mem = min(3, P - 1, w.X.shape[0])
    if n_mem > 0:
        mu[-n_mem:] = w.X[rng.choice(w.X.shape[0], n_mem, replace=False)]
    G = rng.standard_normal((P, E, E))
    var = scale * (G @ np.transpose(G, (0, 2, 1)) / E + 0.1 * np.eye(E))
    return mu, var


# N: 50 (no multiple of 16), 300 (two column blocks, the second partial), 513 (three); P: 1, 65, 130 (one row, two tiles with one
# row in the second, three tiles); D / E: 1 / 2, 3 / 4, 3 / 5 with a time input, and the wide instantiation 16 / 20
CASES = {
    "n50_d1_p1": (50, 1, 1, False, 1),
    "n50_d3_p65": (50, 3, 1, False, 65),
    "n300_d3t_p130": (300, 3, 1, True, 130),
    "n300_d1_p130": (300, 1, 1, False, 130),
    "n513_d3_p65": (513, 3, 1, False, 65),
    "n513_d3t_p1": (513, 3, 1, True, 1),
    "n96_d16_p65": (96, 16, 4, False, 65),
}


def _prepared(engine, N, D, A, time, seed):
    w = synth.make_workload(N, D, A, 2, 1, include_time=time, seed=seed)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    iK, beta = (_np(t) for t in engine.factors())
    return w, (w.X, w.lengthscales, w.outputscales, iK, beta)


# -- 1. extended precision ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_against_extended_precision(engine, case):
    N, D, A, time, P = CASES[case]
    w, fa = _prepared(engine, N, D, A, time, seed=200 + N + D)
    mu, var = _inputs(w, P, seed=201)
    out = engine.moments_linear(mu, var)
    got = {k: _np(out[k]) for k in ("M", "S", "V")}
    r64 = dict(zip(("M", "S", "V"), lin.step(*fa, mu, var)[:3]))
    rld = dict(zip(("M", "S", "V"), lin.step(*fa, mu, var, dtype=np.longdouble)[:3]))
    scale = {"M": float(np.max(np.abs(rld["M"]))), "V": float(np.max(np.abs(rld["V"]))), "S": float(np.max(w.outputscales))}
    errs = {}
    for k in ("M", "S", "V"):
        errs[k + "_hip"] = float(np.max(np.abs(got[k] - rld[k])))
        errs[k + "_numpy"] = float(np.max(np.abs(r64[k] - rld[k])))
    record(f"moments_linear_extended[{case}]", **errs)
    print(case, errs, scale)
    # the rule of tests/test_gpu_predict.py: the HIP evaluation rounds like a plain fp64 evaluation of the same formula
    for k in ("M", "S", "V"):
        assert errs[k + "_hip"] <= 3 * max(errs[k + "_numpy"], 1e-12 * scale[k]), (k, errs)
    assert torch.equal(out["S"], out["S"].transpose(1, 2))               # exactly symmetric


# -- 2. the reference's own step at zero input variance ----------------------------------------------------------------------
def test_step_zero_var_golden_through_the_c_abi(engine):
    g = load("step_zero_var")
    w = workload_of(g)
    D, E = w.Y.shape[1], w.X.shape[1]
    engine.set_factors(w.X, g["iK"], g["beta"], w.lengthscales, w.outputscales)
    mu = engine._dev(g["in_mean"][None])
    M = torch.empty((1, D), dtype=torch.float64, device=engine.device)
    S = torch.empty((1, D, D), dtype=torch.float64, device=engine.device)
    V = torch.empty((1, E, D), dtype=torch.float64, device=engine.device)
    for var in (None, engine._dev(g["in_var"][None])):
        engine._check(engine.lib.gpmpc_moments_linear(engine._h, mu.data_ptr(), var.data_ptr() if var is not None else None, 1, D,
                                                      E, M.data_ptr(), S.data_ptr(), V.data_ptr(), engine._stream()))
        S_h = _np(S)[0]
        assert rel_err(_np(M)[0], g["M"].ravel()) < 1e-10
        assert rel_err(_np(V)[0], g["V"]) < 1e-10
        assert rel_err(np.diag(S_h), np.diag(g["S"])[:D]) < 1e-7
        assert np.all(S_h[~np.eye(D, dtype=bool)] == 0.0)


# -- 3. the entries that compute the same quantities another way -------------------------------------------------------------
# Two fp64 evaluations of the same sums in different orders: the bounds tests/test_gpu_predict.py puts between the kernel and
# the closed form (1e-10 of the scale).
@pytest.mark.parametrize("case", ["n50_d3_p65", "n300_d3t_p130", "n96_d16_p65"])
def test_agrees_with_predict_predict_backward_and_moments(engine, case):
    N, D, A, time, P = CASES[case]
    w, _ = _prepared(engine, N, D, A, time, seed=210 + N)
    E = w.X.shape[1]
    mu, _ = _inputs(w, P, seed=211)
    out = engine.moments_linear(mu)
    M, S, V = (_np(out[k]) for k in ("M", "S", "V"))
    os_max = float(np.max(w.outputscales))
    pred = engine.predict(mu)
    assert rel_err(M, _np(pred["mean"])) < 1e-10
    assert np.max(np.abs(np.diagonal(S, axis1=1, axis2=2) - _np(pred["var"]))) < 1e-10 * os_max
    assert np.all(S[:, ~np.eye(D, dtype=bool)] == 0.0)
    for a in range(D):
        hot = np.zeros((P, D))
        hot[:, a] = 1.0
        assert rel_err(V[:, :, a], _np(engine.predict_backward(mu, mean_bar=hot))) < 1e-10, a
    mm = engine.moments(mu)
    assert rel_err(M, _np(mm["M"])) < 1e-10 and rel_err(V, _np(mm["V"])) < 1e-10
    assert np.max(np.abs(S - _np(mm["S"]))) < 1e-10 * os_max


# -- 4. bits -------------------------------------------------------------------------------------------------------------------
def test_null_outputs_keep_bits(engine):
    w, _ = _prepared(engine, 300, 3, 1, True, seed=220)
    D, E = 3, 5
    mu, var = _inputs(w, 70, seed=221)
    full = engine.moments_linear(mu, var)
    no_S = engine.moments_linear(mu, var, S=False)
    no_V = engine.moments_linear(mu, var, V=False)
    only_M = engine.moments_linear(mu, None, S=False, V=False)
    assert set(no_S) == {"M", "V"} and set(no_V) == {"M", "S"} and set(only_M) == {"M"}
    assert torch.equal(no_S["M"], full["M"]) and torch.equal(no_S["V"], full["V"])
    assert torch.equal(no_V["M"], full["M"]) and torch.equal(no_V["S"], full["S"])
    assert torch.equal(only_M["M"], full["M"])
    # M_out NULL as well: S and V alone, untouched buffers stay untouched
    mu_d, var_d = engine._dev(mu), engine._dev(var)
    S = torch.empty((70, D, D), dtype=torch.float64, device=engine.device)
    V = torch.empty((70, E, D), dtype=torch.float64, device=engine.device)
    engine._check(engine.lib.gpmpc_moments_linear(engine._h, mu_d.data_ptr(), var_d.data_ptr(), 70, D, E, None, S.data_ptr(),
                                                  V.data_ptr(), engine._stream()))
    assert torch.equal(S, full["S"]) and torch.equal(V, full["V"])
    sentinel = torch.full((70, D), 7.0, dtype=torch.float64, device=engine.device)
    engine._check(engine.lib.gpmpc_moments_linear(engine._h, mu_d.data_ptr(), var_d.data_ptr(), 0, D, E, sentinel.data_ptr(),
                                                  None, None, engine._stream()))
    engine._check(engine.lib.gpmpc_moments_linear(engine._h, mu_d.data_ptr(), var_d.data_ptr(), 70, D, E, None, None, None,
                                                  engine._stream()))
    torch.cuda.synchronize()
    assert torch.all(sentinel == 7.0)
    z = engine.moments_linear(np.zeros((0, E)))
    assert z["M"].shape == (0, D) and z["S"].shape == (0, D, D) and z["V"].shape == (0, E, D)


@pytest.mark.parametrize("N,D,A,time", [(300, 3, 1, True), (96, 16, 4, False)])
def test_batch_invariance(engine, N, D, A, time):
    w, _ = _prepared(engine, N, D, A, time, seed=230 + N)
    mu, var = _inputs(w, 130, seed=231)
    full = engine.moments_linear(mu, var)
    again = engine.moments_linear(mu, var)
    rev = engine.moments_linear(mu[::-1].copy(), var[::-1].copy())
    keys = ("M", "S", "V")
    for k in keys:
        assert torch.equal(full[k], again[k])
        assert torch.equal(full[k], rev[k].flip(0))
        assert torch.equal(full["S"], full["S"].transpose(1, 2))
    for i in (0, 63, 64, 129):
        one = engine.moments_linear(mu[i:i + 1], var[i:i + 1])
        for k in keys:
            assert torch.equal(one[k][0], full[k][i]), (k, i)
    # other neighbours, another place
    mu2, var2 = _inputs(w, 9, seed=232)
    mu2[4], var2[4] = mu[100], var[100]
    mixed = engine.moments_linear(mu2, var2)
    for k in keys:
        assert torch.equal(mixed[k][4], full[k][100]), k
    # internal chunks: results do not depend on where the chunk boundaries fall
    for chunk in (1, 7, 64):
        engine.set_option("moments_linear_chunk_points", chunk)
        try:
            chunked = engine.moments_linear(mu[:70], var[:70])
        finally:
            engine.set_option("moments_linear_chunk_points", 0)
        for k in keys:
            assert torch.equal(chunked[k], full[k][:70]), (k, chunk)


# -- 5. errors -----------------------------------------------------------------------------------------------------------------
def test_errors():
    from gp_mpc_amd import _lib as L
    eng = _fresh()
    try:
        mu = torch.zeros((4, 4), dtype=torch.float64, device=eng.device)
        M = torch.empty((4, 3), dtype=torch.float64, device=eng.device)

        def call(P, D, E, mu_ptr=mu.data_ptr()):
            return eng.lib.gpmpc_moments_linear(eng._h, mu_ptr, None, P, D, E, M.data_ptr(), None, None, eng._stream())
        assert call(4, 3, 4) == L.GPMPC_ERR_ARG and "prepare" in eng.lib.gpmpc_last_error(eng._h).decode()
        with pytest.raises(RuntimeError) as ei:
            eng.moments_linear(mu)
        assert type(ei.value).__name__ == "GpmpcError" and ei.value.code == L.GPMPC_ERR_ARG
        w = synth.make_workload(40, 3, 1, 2, 1, seed=240)
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        for P, D, E in ((4, 3, 5), (4, 2, 4), (-1, 3, 4)):
            assert call(P, D, E) == L.GPMPC_ERR_ARG
            assert eng.lib.gpmpc_last_error(eng._h).decode()
        assert call(4, 3, 4, None) == L.GPMPC_ERR_ARG
        assert call(0, 3, 4, None) == L.GPMPC_OK
        assert call(4, 17, 18) == L.GPMPC_ERR_LIMIT and call(4, 3, 25) == L.GPMPC_ERR_LIMIT
        assert eng.lib.gpmpc_set_option(eng._h, b"moments_linear_chunk_points", -1) == L.GPMPC_ERR_ARG
        assert call(4, 3, 4) == L.GPMPC_OK
    finally:
        eng.close()


# -- 6. no interference with the rest of the handle ---------------------------------------------------------------------------
def test_no_interference():
    g = load("traj_c2")
    w = workload_of(g)
    eng = _fresh()
    try:
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        before = {k: v.clone() for k, v in eng.rollout(w.actions, w.mu0, w.S0).items()}
        state = (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode, eng.last_grad_path)
        mu, var = _inputs(w, 200, seed=250)
        eng.moments_linear(mu, var)
        assert (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode, eng.last_grad_path) == state
        after = eng.rollout(w.actions, w.mu0, w.S0)
        for k in before:
            assert torch.equal(before[k], after[k]), k
    finally:
        eng.close()


# -- 7. Python level -----------------------------------------------------------------------------------------------------------
def test_transition_model_linearized_step(engine):
    from gp_mpc_amd.config_classes import ModelConfig
    from gp_mpc_amd.control_objects.models.gp_model import GpStateTransitionModel
    w = synth.make_workload(120, 3, 1, 2, 1, seed=260)
    mu, var = _inputs(w, 5, seed=261)
    model = GpStateTransitionModel(ModelConfig(uncertainty_propagation="linearized"), 3, 1, engine=engine)
    model.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    ref = engine.moments_linear(mu, var)
    out = model.predict_next_state_change_batch(torch.as_tensor(mu), torch.as_tensor(var))
    for k in ("M", "S", "V"):
        assert out[k].device.type == "cuda" and torch.equal(out[k], ref[k])
    M, S, V = model.predict_next_state_change(torch.as_tensor(mu[0]), torch.as_tensor(var[0]))
    assert M.shape == (1, 3) and torch.equal(S, ref["S"][0].cpu()) and torch.equal(V, ref["V"][0].cpu())
    mm = model.predict_next_state_change_batch(torch.as_tensor(mu), torch.as_tensor(var), propagation="moment_matching")
    assert torch.equal(mm["S"], engine.moments(mu, var)["S"])
    with pytest.raises(NotImplementedError):
        model.predict_next_state_change_batch(torch.as_tensor(mu).requires_grad_(True), torch.as_tensor(var))
