"""Tier 2 (GPU): gpmpc_moments -- moment-matched prediction at Gaussian inputs with a general covariance.

Pinned to the reference by the single-step goldens and tests/golden/moments_full_var*.npz (predict_next_state_change,
tools/gen_golden_moments.py; tests/test_moments_reference.py ties them to the oracle), to an extended-precision evaluation on
the same fp64 factors, to identities with gpmpc_predict and gpmpc_rollout, to a Monte-Carlo estimate through gpmpc_predict
that does not depend on the reference's formula, and to the contracts of include/gpmpc.h.
"""
import numpy as np
import pytest
import torch

from helpers import load, workload_of, rel_err, record
from oracle import synth
from oracle import gpmpc_oracle as orc
from oracle import extended_precision as xp

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


def _inputs(w, P, seed, scale=0.3):
    """P means in the box of the memory inputs and dense covariances of about `scale` shortest lengthscales."""
    rng = np.random.default_rng(seed)
    E = w.X.shape[1]
    lo, hi = w.X.min(axis=0), w.X.max(axis=0)
    mu = lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(P, E))
    ls = w.lengthscales.min(axis=0)
    G = rng.standard_normal((P, E, E)) * (scale * ls)[None, :, None]
    var = G @ G.transpose(0, 2, 1) + 1e-6 * np.diag(ls ** 2)[None]
    return mu, var


def _check_golden(out, M, S, V, tag):
    e_M, e_S, e_V = rel_err(_np(out["M"]), M), rel_err(_np(out["S"]), S), rel_err(_np(out["V"]), V)
    record(tag, M=e_M, S=e_S, V=e_V)
    assert e_M <= 1e-10 and e_V <= 1e-10 and e_S <= 1e-6, (e_M, e_S, e_V)


# -- 1. goldens of the reference's own code -----------------------------------------------------------------------------------
def _load(engine, g, load_by):
    w = workload_of(g)
    if load_by == "set_factors":
        engine.set_factors(w.X, g["iK"], g["beta"], w.lengthscales, w.outputscales)
    else:
        engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    return w


@pytest.mark.parametrize("name", ["step_zero_var", "step_dense_var", "step_dense_var_time"])
@pytest.mark.parametrize("load_by", ["set_factors", "prepare"])
def test_step_goldens(engine, name, load_by):
    g = load(name)
    _load(engine, g, load_by)
    out = engine.moments(g["in_mean"][None], g["in_var"][None])       # the action and time rows of V included
    _check_golden(out, g["M"], g["S"][None], g["V"][None], f"moments_golden[{name},{load_by}]")


@pytest.mark.parametrize("name", ["moments_full_var", "moments_full_var_time"])
@pytest.mark.parametrize("load_by", ["set_factors", "prepare"])
def test_full_var_goldens(engine, name, load_by):
    g = load(name)
    _load(engine, g, load_by)
    out = engine.moments(g["in_mean"], g["in_var"])
    _check_golden(out, g["M"], g["S"], g["V"], f"moments_golden[{name},{load_by}]")
    for k in range(5):                                   # every kind of covariance on its own scale
        sel = g["kind"] == k
        assert rel_err(_np(out["S"])[sel], g["S"][sel]) <= 1e-6, k


def test_golden_after_mll(engine):
    g = load("moments_full_var")
    w = workload_of(g)
    engine.mll(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    out = engine.moments(g["in_mean"], g["in_var"])
    _check_golden(out, g["M"], g["S"], g["V"], "moments_golden[mll]")


def test_transition_model_method(engine):
    from gp_mpc_amd.config_classes import ModelConfig
    from gp_mpc_amd.control_objects.models.gp_model import GpStateTransitionModel
    g = load("moments_full_var_time")
    w = workload_of(g)
    D, E = w.Y.shape[1], w.X.shape[1]
    cfg = ModelConfig(gp_init={"noise_covar.noise": list(w.noises), "outputscale": list(w.outputscales),
                               "base_kernel.lengthscale": w.lengthscales[:, :E - 1].tolist()}, include_time_model=True)
    model = GpStateTransitionModel(cfg, D, E - D - 1, engine=engine)
    with pytest.raises(RuntimeError):
        model.predict_next_state_change(torch.zeros(E), torch.zeros(E, E))
    model.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    engine.set_factors(w.X, g["iK"], g["beta"], w.lengthscales, w.outputscales)    # the reference's time lengthscales
    for p in (0, 8, 12, 16, 20):
        Mt, S, Vt = model.predict_next_state_change(torch.as_tensor(g["in_mean"][p]), torch.as_tensor(g["in_var"][p]))
        assert Mt.device.type == "cpu" and Mt.dtype == torch.float64
        assert Mt.shape == (1, D) and S.shape == (D, D) and Vt.shape == (E, D)
        _check_golden({"M": Mt, "S": S[None], "V": Vt[None]}, g["M"][p][None], g["S"][p][None], g["V"][p][None],
                      "moments_model_method")
    out = model.predict_next_state_change_batch(torch.as_tensor(g["in_mean"]), torch.as_tensor(g["in_var"]))
    assert out["M"].device.type == "cuda"
    _check_golden(out, g["M"], g["S"], g["V"], "moments_model_batch")


# -- 2. extended precision ---------------------------------------------------------------------------------------------------
def _xfactors(w, engine):
    iK, beta = (_np(t) for t in engine.factors())
    f = object.__new__(xp.Factors)
    f.X, f.lengthscales, f.variances = xp._ld(w.X), xp._ld(w.lengthscales), xp._ld(w.outputscales)
    f.iK, f.beta = xp._ld(iK), xp._ld(beta)
    return f, iK, beta


@pytest.mark.parametrize("N,D,A,P", [(500, 2, 1, 3), (1000, 4, 2, 2)])
def test_against_extended_precision(engine, N, D, A, P):
    w = synth.make_workload(N, D, A, 2, 1, seed=170 + N)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    f, _, _ = _xfactors(w, engine)
    mu, var = _inputs(w, P, seed=171)
    out = engine.moments(mu, var)
    for p in range(P):
        Mx, Sx, Vx = (np.asarray(v, dtype=np.float64) for v in xp.moment_match_step(f, xp._ld(mu[p]), xp._ld(var[p])))
        e_S = float(np.max(np.abs(_np(out["S"])[p] - Sx)) / np.max(np.abs(Sx)))
        e_M, e_V = rel_err(_np(out["M"])[p], Mx), rel_err(_np(out["V"])[p], Vx)
        record(f"moments_extended[{N},{D},{p}]", M=e_M, S=e_S, V=e_V)
        assert e_S <= 1e-5 and e_M <= 1e-9 and e_V <= 1e-9, (e_M, e_S, e_V)


def _S_pair(X, ls, os_, iK, beta, m, s, a, b):
    """S_ab of one input by gp_model.py:155-178 before the - M M^T, numpy fp64 (one pair only)."""
    E = X.shape[1]
    inp = X - m[None, :]
    R = s * (1.0 / ls[a] ** 2 + 1.0 / ls[b] ** 2)[None, :] + np.eye(E)
    Q = np.linalg.solve(R, s) / 2.0
    Xa, Xb = inp / ls[a] ** 2, -inp / ls[b] ** 2
    ka = np.log(os_[a]) - 0.5 * np.sum((inp / ls[a]) ** 2, axis=-1)
    kb = np.log(os_[b]) - 0.5 * np.sum((inp / ls[b]) ** 2, axis=-1)
    XaQ, XbQ = Xa @ Q, Xb @ Q
    maha = -2.0 * (XaQ @ Xb.T) + np.sum(XaQ * Xa, -1)[:, None] + np.sum(XbQ * Xb, -1)[None, :]
    L = np.exp(ka[:, None] + kb[None, :] + maha)
    v = beta[a] @ L @ beta[b]
    if a == b:
        v -= np.sum(iK[a] * L)
    v /= np.sqrt(np.linalg.det(R))
    return v + (os_[a] if a == b else 0.0)


def test_wide_shape_against_numpy(engine):
    N, D, A = 4096, 16, 4
    w = synth.make_workload(N, D, A, 2, 1, seed=180)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    iK, beta = (_np(t) for t in engine.factors())
    mu, var = _inputs(w, 2, seed=181)
    out = engine.moments(mu, var)
    Mg, Sg, Vg = _np(out["M"]), _np(out["S"]), _np(out["V"])
    ls = w.lengthscales
    for p in range(2):
        # M and V by gp_model.py:138-153 in numpy; S on a few pairs (the full D(D+1)/2 x N^2 pass is too slow on the host)
        inp = w.X - mu[p][None, :]
        Mn = np.empty(D)
        Vn = np.empty((w.X.shape[1], D))
        for a in range(D):
            iL = 1.0 / ls[a]
            iN = inp * iL
            Bm = iL[:, None] * var[p] * iL[None, :] + np.eye(len(iL))
            t = np.linalg.solve(Bm, iN.T).T
            lb = np.exp(-0.5 * np.sum(iN * t, axis=-1)) * beta[a]
            c = w.outputscales[a] / np.sqrt(np.linalg.det(Bm))
            Mn[a] = np.sum(lb) * c
            Vn[:, a] = (t * iL).T @ lb * c
        assert rel_err(Mg[p], Mn) <= 1e-9 and rel_err(Vg[p], Vn) <= 1e-9
        scale = np.max(np.abs(np.diagonal(Sg[p])))
        for a, b in ((0, 0), (0, 15), (7, 9), (15, 15)):
            ref = _S_pair(w.X, ls, w.outputscales, iK, beta, mu[p], var[p], a, b) - Mn[a] * Mn[b]
            assert abs(Sg[p, a, b] - ref) <= 1e-7 * scale, (a, b, Sg[p, a, b], ref)
            assert Sg[p, a, b] == Sg[p, b, a]


# -- 3. identities -----------------------------------------------------------------------------------------------------------
def test_zero_variance_is_the_posterior(engine):
    w = synth.make_workload(200, 3, 1, 2, 1, seed=190)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    mu, _ = _inputs(w, 40, seed=191)
    a = engine.moments(mu)
    b = engine.moments(mu, np.zeros((40, 4, 4)))
    for k in ("M", "S", "V"):
        assert torch.equal(a[k], b[k]), k
    pr = engine.predict(mu)
    S = _np(a["S"])
    assert rel_err(_np(a["M"]), _np(pr["mean"])) <= 1e-12
    # both sides are sigma2 minus sums of terms up to |beta|^2 sigma2^2: the reference itself differs by ~4e-12 (test_predict_reference.py)
    assert np.max(np.abs(np.diagonal(S, axis1=1, axis2=2) - _np(pr["var"]))) <= 1e-9 * w.outputscales.max()
    off = S.copy()
    off[:, range(3), range(3)] = 0.0
    assert np.max(np.abs(off)) <= 1e-9 * w.outputscales.max()


def test_V_is_the_gradient_of_M(engine):
    w = synth.make_workload(200, 3, 2, 2, 1, seed=200)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    mu, var = _inputs(w, 3, seed=201)
    E = mu.shape[1]
    V = _np(engine.moments(mu, var)["V"])
    h = 1e-5
    shifted = np.concatenate([mu + h * np.eye(E)[e][None] for e in range(E)] + [mu - h * np.eye(E)[e][None] for e in range(E)])
    Ms = _np(engine.moments(shifted, np.tile(var, (2 * E, 1, 1)), S=False, V=False)["M"]).reshape(2, E, 3, 3)
    fd = ((Ms[0] - Ms[1]) / (2 * h)).transpose(1, 0, 2)               # (P, E, D)
    err = rel_err(V, fd)
    record("moments_V_central_difference", err=err)
    assert err <= 1e-6


def test_state_block_matches_one_rollout_step(engine):
    g = load("traj_c2")
    w = workload_of(g)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    engine.set_cost(w.target, w.W, w.W_T, w.kappa)
    D = w.Y.shape[1]
    E = w.X.shape[1]
    acts = w.actions[:4, :1]
    out = engine.rollout(acts, w.mu0, w.S0)
    mu = np.concatenate([np.tile(w.mu0, (4, 1)), acts[:, 0]], axis=1)
    var = np.zeros((4, E, E))
    var[:, :D, :D] = w.S0
    m = engine.moments(mu, var)
    M, S, V = _np(m["M"]), _np(m["S"]), _np(m["V"])
    C = w.S0[None] @ V[:, :D, :]
    assert rel_err(w.mu0[None] + M, _np(out["mu"])[:, 1]) <= 1e-10
    assert rel_err(S + w.S0[None] + C + C.transpose(0, 2, 1), _np(out["Sig"])[:, 1]) <= 1e-6


# -- 4. Monte Carlo through gpmpc_predict ------------------------------------------------------------------------------------
def test_monte_carlo(engine):
    w = synth.make_workload(200, 3, 1, 2, 1, seed=210)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    mu, var = _inputs(w, 1, seed=211, scale=0.5)
    m = engine.moments(mu, var)
    M, S = _np(m["M"])[0], _np(m["S"])[0]
    rng = np.random.default_rng(212)
    n = 1 << 20
    x = rng.multivariate_normal(mu[0], var[0], size=n)
    pr = engine.predict(x)
    f, v = _np(pr["mean"]), _np(pr["var"])
    fm = f.mean(axis=0)
    dev = f - fm
    se = lambda s: s.std(axis=0) / np.sqrt(n)                                          # noqa: E731
    assert np.all(np.abs(M - fm) <= 5 * se(f)), (M, fm, se(f))
    diag = v + dev ** 2
    assert np.all(np.abs(np.diagonal(S) - diag.mean(axis=0)) <= 5 * se(diag))
    for a, b in ((0, 1), (0, 2), (1, 2)):
        c = dev[:, a] * dev[:, b]
        assert abs(S[a, b] - c.mean()) <= 5 * se(c), (a, b, S[a, b], c.mean(), se(c))
    record("moments_monte_carlo", M=float(np.max(np.abs(M - fm) / se(f))))


# -- 5. contracts ------------------------------------------------------------------------------------------------------------
def test_batch_invariance(engine):
    w = synth.make_workload(200, 3, 2, 2, 1, seed=220)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    mu, var = _inputs(w, 300, seed=221)
    full = engine.moments(mu, var)
    again = engine.moments(mu, var)
    rev = engine.moments(mu[::-1].copy(), var[::-1].copy())
    perm = np.random.default_rng(222).permutation(300)
    shuf = engine.moments(mu[perm], var[perm])
    for k in ("M", "S", "V"):
        assert torch.equal(full[k], again[k]), k
        assert torch.equal(full[k], rev[k].flip(0)), k
        assert torch.equal(full[k][perm], shuf[k]), k
    for P in (1, 2, 7, 8, 9, 63, 129):
        part = engine.moments(mu[:P], var[:P])
        for k in ("M", "S", "V"):
            assert torch.equal(part[k], full[k][:P]), (k, P)
    for i in (0, 150, 299):
        one = engine.moments(mu[i:i + 1], var[i:i + 1])
        mixed = engine.moments(np.concatenate([w.X[:5], mu[i:i + 1]]), np.concatenate([var[:5] * 9.0, var[i:i + 1]]))
        for k in ("M", "S", "V"):
            assert torch.equal(one[k][0], full[k][i]) and torch.equal(mixed[k][5], full[k][i]), (k, i)
    for chunk in (1, 5, 64):
        engine.set_option("moments_chunk_points", chunk)
        try:
            c = engine.moments(mu, var)
        finally:
            engine.set_option("moments_chunk_points", 0)
        for k in ("M", "S", "V"):
            assert torch.equal(c[k], full[k]), (k, chunk)
    # S / V not requested: M (and V) keep their bits
    m_only = engine.moments(mu, var, S=False, V=False)
    mv = engine.moments(mu, var, S=False)
    assert set(m_only) == {"M"} and set(mv) == {"M", "V"}
    assert torch.equal(m_only["M"], full["M"]) and torch.equal(mv["M"], full["M"]) and torch.equal(mv["V"], full["V"])
    # P = 0
    z = engine.moments(np.zeros((0, 5)), np.zeros((0, 5, 5)))
    assert z["M"].shape == (0, 3) and z["S"].shape == (0, 3, 3) and z["V"].shape == (0, 5, 3)


def test_large_variance_is_finite(engine):
    w = synth.make_workload(200, 3, 1, 2, 1, seed=230)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    mu, _ = _inputs(w, 6, seed=231)
    ls = w.lengthscales.max(axis=0)
    var = np.stack([np.diag((s * ls) ** 2) for s in (3.0, 10.0, 30.0, 100.0, 1e3, 1e4)])
    out = engine.moments(mu, var)
    for k in ("M", "S", "V"):
        assert torch.all(torch.isfinite(out[k])), k
    f = orc.Factors(w.X, w.Y, w.lengthscales, w.outputscales, w.noises, *(_np(t) for t in engine.factors()))
    M, S, V = orc.moment_match_step(f, mu, var)
    assert rel_err(_np(out["M"]), M) <= 1e-9 and rel_err(_np(out["S"]), S) <= 1e-6


def test_errors():
    from gp_mpc_amd import _lib as L
    eng = _fresh()
    try:
        mu = torch.zeros((4, 25), dtype=torch.float64, device=eng.device)
        out = torch.empty((4 * 25 * 16,), dtype=torch.float64, device=eng.device)

        def call(P, D, E):
            return eng.lib.gpmpc_moments(eng._h, mu.data_ptr(), None, P, D, E, out.data_ptr(), out.data_ptr(), out.data_ptr(),
                                         eng._stream())
        assert call(4, 3, 4) == L.GPMPC_ERR_ARG and "prepare" in eng.lib.gpmpc_last_error(eng._h).decode()
        with pytest.raises(RuntimeError) as ei:
            eng.moments(np.zeros((4, 4)))
        assert type(ei.value).__name__ == "GpmpcError" and ei.value.code == L.GPMPC_ERR_ARG
        w = synth.make_workload(40, 3, 1, 2, 1, seed=240)
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        for P, D, E in ((4, 3, 5), (4, 2, 4), (-1, 3, 4)):
            assert call(P, D, E) == L.GPMPC_ERR_ARG, (P, D, E)
        assert call(4, 3, 25) == L.GPMPC_ERR_LIMIT
        assert call(4, 17, 4) == L.GPMPC_ERR_LIMIT
        with pytest.raises(RuntimeError):
            eng.moments(np.zeros((4, 5)))
        assert call(0, 3, 4) == L.GPMPC_OK
        assert call(4, 3, 4) == L.GPMPC_OK
        torch.cuda.synchronize()
    finally:
        eng.close()


def test_no_interference():
    g = load("traj_c2")
    w = workload_of(g)
    eng = _fresh()
    try:
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        before = {k: v.clone() for k, v in eng.rollout(w.actions, w.mu0, w.S0).items()}
        state = (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode)
        mu, var = _inputs(w, 500, seed=250)
        eng.moments(mu, var)
        assert (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode) == state
        after = eng.rollout(w.actions, w.mu0, w.S0)
        for k in before:
            assert torch.equal(before[k], after[k]), k
        # the memory grows by 4 points: still a border update after a moments call
        x = synth.make_workload(204, 3, 1, 2, 1, seed=251)
        eng.prepare(x.X[:200], x.Y[:200], w.lengthscales, w.outputscales, w.noises)
        eng.moments(mu[:50], var[:50])
        eng.prepare(x.X, x.Y, w.lengthscales, w.outputscales, w.noises)
        assert eng.last_prepare_mode == 1
    finally:
        eng.close()
