"""Tier 2 (GPU): gpmpc_moments_backward -- gradients of moment matching with respect to the input mean and covariance.

Pinned to torch autograd through the reference's predict_next_state_change (tests/golden/moments_grad_full_var*.npz,
tools/gen_golden_moments_grad.py; tests/test_moments_backward_reference.py ties them to longdouble differences), to longdouble
and Richardson central differences, to identities that do not use the reference's formula (Stein's lemma and Price's theorem
through the forward's V), to torch autograd through the model's methods, and to the contracts of include/gpmpc.h.  The
covariance gradient is compared as its symmetric part.
"""
import numpy as np
import pytest
import torch

from helpers import load, workload_of, rel_err, record
from moments_fd import xfactors, directional, directions
from oracle import synth

pytestmark = pytest.mark.gpu

GOLDENS = ["moments_full_var", "moments_full_var_time"]


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
    return t.detach().cpu().numpy()


def _sym(G):
    return 0.5 * (G + np.swapaxes(G, -1, -2))


def _inputs(w, P, seed, scale=0.3):
    rng = np.random.default_rng(seed)
    E = w.X.shape[1]
    lo, hi = w.X.min(axis=0), w.X.max(axis=0)
    mu = lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(P, E))
    ls = w.lengthscales.min(axis=0)
    G = rng.standard_normal((P, E, E)) * (scale * ls)[None, :, None]
    var = G @ G.transpose(0, 2, 1) + 1e-6 * np.diag(ls ** 2)[None]
    return mu, var


def _upstream(P, D, E, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((P, D)), rng.standard_normal((P, D, D)), rng.standard_normal((P, E, D))


def _load(engine, g, load_by):
    w = workload_of(g)
    if load_by == "set_factors":
        engine.set_factors(w.X, g["iK"], g["beta"], w.lengthscales, w.outputscales)
    elif load_by == "mll":
        engine.mll(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    else:
        engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    return w


def _set(gg, s):
    """Upstream set s of a gradient golden, None where it is zero by construction."""
    return (gg["M_bar"][s] if s != 2 else None, gg["S_bar"][s] if s != 1 else None, gg["V_bar"][s] if s != 2 else None)


# -- 1. goldens of the reference's own autograd -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("load_by", ["set_factors", "prepare", "mll"])
def test_reference_autograd_goldens(engine, name, load_by):
    g, gg = load(name), load(name.replace("moments_", "moments_grad_"))
    _load(engine, g, load_by)
    for s in range(3):
        Mb, Sb, Vb = _set(gg, s)
        out = engine.moments_backward(gg["in_mean"], gg["in_var"], Mb, Sb, Vb)
        e_m = rel_err(_np(out["mu_bar"]), gg["mu_bar"][s])
        e_S = rel_err(_np(out["var_bar"]), _sym(gg["G"][s]))
        record(f"moments_backward_golden[{name},{load_by},set{s}]", mu_bar=e_m, var_bar=e_S)
        tol = 1e-9 if s == 1 else 1e-6
        assert e_m <= tol and e_S <= tol, (s, e_m, e_S)
        assert np.array_equal(_np(out["var_bar"]), np.swapaxes(_np(out["var_bar"]), -1, -2))


# -- 2. torch autograd through the model -------------------------------------------------------------------------------------
def _model(engine, g):
    from gp_mpc_amd.config_classes import ModelConfig
    from gp_mpc_amd.control_objects.models.gp_model import GpStateTransitionModel
    w = workload_of(g)
    D, E = w.Y.shape[1], w.X.shape[1]
    t = bool(g["include_time"])
    ls = w.lengthscales[:, :E - 1] if t else w.lengthscales
    cfg = ModelConfig(gp_init={"noise_covar.noise": list(w.noises), "outputscale": list(w.outputscales),
                               "base_kernel.lengthscale": ls.tolist()}, include_time_model=t)
    model = GpStateTransitionModel(cfg, D, E - D - int(t), engine=engine)
    model.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    engine.set_factors(w.X, g["iK"], g["beta"], w.lengthscales, w.outputscales)
    return model


@pytest.mark.parametrize("name", GOLDENS)
def test_model_backward(engine, name):
    g, gg = load(name), load(name.replace("moments_", "moments_grad_"))
    model = _model(engine, g)
    D = g["M"].shape[1]
    for p in (0, 5, 9, 13, 17, 21):
        mu = torch.tensor(gg["in_mean"][p], requires_grad=True)
        var = torch.tensor(gg["in_var"][p], requires_grad=True)
        Mt, S, Vt = model.predict_next_state_change(mu, var)
        assert Mt.grad_fn is not None and Mt.shape == (1, D) and Vt.shape == var.shape[:1] + (D,)
        loss = (torch.tensor(gg["M_bar"][0, p]) * Mt.reshape(D)).sum() + (torch.tensor(gg["S_bar"][0, p]) * S).sum() + \
            (torch.tensor(gg["V_bar"][0, p]) * Vt).sum()
        loss.backward()
        assert mu.grad.device.type == "cpu" and var.grad.device.type == "cpu"
        assert rel_err(mu.grad.numpy(), gg["mu_bar"][0, p]) <= 1e-6
        assert rel_err(var.grad.numpy(), _sym(gg["G"][0, p])) <= 1e-6
        # Sigma = A A^T: autograd reaches A as 2 sym(G) A
        A0 = np.linalg.cholesky(gg["in_var"][p] + 1e-12 * np.eye(len(mu))) if gg["kind"][p] != 3 else np.zeros_like(gg["in_var"][p])
        A = torch.tensor(A0, requires_grad=True)
        Mt, S, Vt = model.predict_next_state_change(torch.tensor(gg["in_mean"][p]), A @ A.T)
        ((torch.tensor(gg["M_bar"][0, p]) * Mt.reshape(D)).sum() + (torch.tensor(gg["S_bar"][0, p]) * S).sum() +
         (torch.tensor(gg["V_bar"][0, p]) * Vt).sum()).backward()
        assert rel_err(A.grad.numpy(), 2.0 * _sym(gg["G"][0, p]) @ A0) <= 1e-6
    with pytest.raises(RuntimeError):                        # once differentiable
        mu = torch.tensor(gg["in_mean"][0], requires_grad=True)
        Mt, S, Vt = model.predict_next_state_change(mu, torch.tensor(gg["in_var"][0]))
        (gm,) = torch.autograd.grad(Mt.sum(), mu, create_graph=True)
        gm.sum().backward()


def test_model_batch_on_device_and_no_grad_bits(engine):
    g, gg = load("moments_full_var_time"), load("moments_grad_full_var_time")
    model = _model(engine, g)
    dev = engine.device
    mu = torch.tensor(gg["in_mean"], device=dev, requires_grad=True)
    var = torch.tensor(gg["in_var"], device=dev, requires_grad=True)
    out = model.predict_next_state_change_batch(mu, var)
    Mb, Sb, Vb = (torch.tensor(a, device=dev) for a in (gg["M_bar"][0], gg["S_bar"][0], gg["V_bar"][0]))
    ((out["M"] * Mb).sum() + (out["S"] * Sb).sum() + (out["V"] * Vb).sum()).backward()
    assert mu.grad.device == mu.device and var.grad.device == var.device
    assert rel_err(_np(mu.grad), gg["mu_bar"][0]) <= 1e-6 and rel_err(_np(var.grad), _sym(gg["G"][0])) <= 1e-6
    # input_var None: the mean's gradient only (at Sigma = 0)
    mu.grad = None
    out = model.predict_next_state_change_batch(mu)
    (out["M"] * Mb).sum().backward()
    ref = engine.moments_backward(gg["in_mean"], None, gg["M_bar"][0], None, None, var_bar=False)["mu_bar"]
    assert torch.equal(mu.grad, ref)
    # without requires_grad (or under no_grad): bitwise the outputs of engine.moments, no grad_fn
    plain = engine.moments(gg["in_mean"], gg["in_var"])
    for o in (model.predict_next_state_change_batch(torch.tensor(gg["in_mean"]), torch.tensor(gg["in_var"]))
              , None):
        if o is None:
            with torch.no_grad():
                o = model.predict_next_state_change_batch(mu, var)
        for k in ("M", "S", "V"):
            assert o[k].grad_fn is None and torch.equal(o[k], plain[k]), k


def test_gradcheck_small(engine):
    w = synth.make_workload(50, 2, 1, 2, 1, seed=300)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    from gp_mpc_amd.control_objects.models.gp_model import _MomentsFunction
    mu0, var0 = _inputs(w, 2, seed=301)
    A0 = np.linalg.cholesky(var0)
    mu = torch.tensor(mu0, device=engine.device, requires_grad=True)
    A = torch.tensor(A0, device=engine.device, requires_grad=True)

    def f(mu, A):
        M, S, V = _MomentsFunction.apply(engine, mu, A @ A.transpose(1, 2))
        return M, S, V
    # S's pair sums cancel (beta beta^T - iK), so the forward's differences carry ~1e-12 absolute noise: eps 1e-4 keeps it small
    assert torch.autograd.gradcheck(f, (mu, A), eps=1e-4, atol=1e-6, rtol=1e-4)


# -- 3. extended precision ---------------------------------------------------------------------------------------------------
def test_extended_precision_medium():
    eng = _fresh()
    try:
        w = synth.make_workload(1000, 4, 2, 2, 1, seed=310)
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        iK, beta = (_np(t) for t in eng.factors())
        f = xfactors(w.X, w.lengthscales, w.outputscales, iK, beta)
        E, D = w.X.shape[1], 4
        ls = w.lengthscales.min(axis=0)
        mu, var = _inputs(w, 3, seed=311)
        var[1] = 0.0
        var[1, D:, D:] = var[0, D:, D:]                          # action block only
        var[2] = var[2] * 100.0                                  # several lengthscales wide
        Mb, Sb, Vb = _upstream(3, D, E, seed=312)
        out = eng.moments_backward(mu, var, Mb, Sb, Vb)
        rng = np.random.default_rng(313)
        errs = []
        for p in range(3):
            dm, ds = directions(E, ls, rng)
            fd = directional(f, mu[p], var[p], Mb[p], Sb[p], Vb[p], dm, 0 * ds, 1e-6) + \
                directional(f, mu[p], var[p], Mb[p], Sb[p], Vb[p], 0 * dm, ds, 1e-6)
            an = float(_np(out["mu_bar"][p]) @ dm + (_np(out["var_bar"][p]) * ds).sum())
            sc = float(np.abs(_np(out["mu_bar"][p])) @ np.abs(dm) + (np.abs(_np(out["var_bar"][p])) * np.abs(ds)).sum())
            errs.append(abs(an - fd) / sc)
        record("moments_backward_xp[N=1000,D=4,A=2]", err=max(errs))
        assert max(errs) <= 1e-7, errs
    finally:
        eng.close()


def test_large_against_richardson():
    """N = 4096, D = 16, E = 20, one point: against Richardson-extrapolated central differences of gpmpc_moments itself
    (fp64; truncation O(h^4), rounding ~1e-16 / h of the summed terms): 1e-6 of the terms' scale."""
    eng = _fresh()
    try:
        w = synth.make_workload(4096, 16, 4, 2, 1, seed=320)
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        E, D = 20, 16
        ls = w.lengthscales.min(axis=0)
        mu, var = _inputs(w, 1, seed=321)
        Mb, Sb, Vb = _upstream(1, D, E, seed=322)
        out = eng.moments_backward(mu, var, Mb, Sb, Vb)
        dm, ds = directions(E, ls, np.random.default_rng(323))

        def L(h):
            o = eng.moments(mu + h * dm[None], var + h * ds[None])
            return float((_np(o["M"]) * Mb).sum() + (_np(o["S"]) * Sb).sum() + (_np(o["V"]) * Vb).sum())
        h = 1e-3
        d1 = (L(h) - L(-h)) / (2 * h)
        d2 = (L(h / 2) - L(-h / 2)) / h
        fd = (4 * d2 - d1) / 3
        an = float(_np(out["mu_bar"][0]) @ dm + (_np(out["var_bar"][0]) * ds).sum())
        sc = float(np.abs(_np(out["mu_bar"][0])) @ np.abs(dm) + (np.abs(_np(out["var_bar"][0])) * np.abs(ds)).sum())
        record("moments_backward_richardson[N=4096,D=16,E=20]", err=abs(an - fd) / sc)
        assert abs(an - fd) <= 1e-6 * sc, (an, fd, sc)
    finally:
        eng.close()


# -- 4. identities that do not use the reference's formula --------------------------------------------------------------------
def test_stein_and_price(engine):
    w = synth.make_workload(300, 3, 2, 2, 1, seed=330)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    E, D = 5, 3
    mu, var = _inputs(w, 6, seed=331)
    Mb, _, _ = _upstream(6, D, E, seed=332)
    out = engine.moments_backward(mu, var, Mb)
    fwd = engine.moments(mu, var, S=False)
    VM = np.einsum("ped,pd->pe", _np(fwd["V"]), Mb)
    e_stein = rel_err(_np(out["mu_bar"]), VM)                  # Stein: dM/dm = V
    # Price: dM/dSigma = 1/2 d^2M/dm^2, so Sigma_bar = 1/2 sym(d(V Mb)/dm), by central differences of the forward's V
    ls = w.lengthscales.min(axis=0)
    J = np.zeros((6, E, E))
    for e in range(E):
        h = 1e-5 * ls[e]
        d = np.zeros(E)
        d[e] = h
        Vp = _np(engine.moments(mu + d, var, S=False)["V"])
        Vm = _np(engine.moments(mu - d, var, S=False)["V"])
        J[:, :, e] = np.einsum("ped,pd->pe", (Vp - Vm) / (2 * h), Mb)
    e_price = rel_err(_np(out["var_bar"]), 0.5 * _sym(J))
    record("moments_backward_identities", stein=e_stein, price=e_price)
    assert e_stein <= 1e-10 and e_price <= 1e-6, (e_stein, e_price)


# -- 5. contracts ------------------------------------------------------------------------------------------------------------
def test_batch_invariance():
    eng = _fresh()
    try:
        w = synth.make_workload(150, 3, 1, 2, 1, seed=340)
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        E, D = 4, 3
        mu, var = _inputs(w, 300, seed=341)
        Mb, Sb, Vb = _upstream(300, D, E, seed=342)
        full = eng.moments_backward(mu, var, Mb, Sb, Vb)
        ref_m, ref_S = _np(full["mu_bar"]), _np(full["var_bar"])
        for P in (1, 2, 7, 64, 299):
            o = eng.moments_backward(mu[:P], var[:P], Mb[:P], Sb[:P], Vb[:P])
            assert np.array_equal(_np(o["mu_bar"]), ref_m[:P]) and np.array_equal(_np(o["var_bar"]), ref_S[:P]), P
        for idx in (np.arange(300)[::-1], np.random.default_rng(343).permutation(300)):
            o = eng.moments_backward(mu[idx], var[idx], Mb[idx], Sb[idx], Vb[idx])
            assert np.array_equal(_np(o["mu_bar"]), ref_m[idx]) and np.array_equal(_np(o["var_bar"]), ref_S[idx])
        for chunk in (1, 5, 64):
            eng.set_option("moments_backward_chunk_points", chunk)
            o = eng.moments_backward(mu, var, Mb, Sb, Vb)
            assert np.array_equal(_np(o["mu_bar"]), ref_m) and np.array_equal(_np(o["var_bar"]), ref_S), chunk
        eng.set_option("moments_backward_chunk_points", 0)
    finally:
        eng.close()


def test_null_pointers_and_sentinels(engine):
    w = synth.make_workload(130, 3, 2, 2, 1, seed=350)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    E, D, P = 5, 3, 9
    mu, var = _inputs(w, P, seed=351)
    Mb, Sb, Vb = _upstream(P, D, E, seed=352)
    z = lambda a: np.zeros_like(a)                                   # noqa: E731
    for args in ((Mb, None, None), (None, Sb, None), (None, None, Vb), (Mb, None, Vb), (None, None, None)):
        o = engine.moments_backward(mu, var, *args)
        e = engine.moments_backward(mu, var, *(a if a is not None else z(b) for a, b in zip(args, (Mb, Sb, Vb))))
        assert torch.equal(o["mu_bar"], e["mu_bar"]) and torch.equal(o["var_bar"], e["var_bar"])
    o = engine.moments_backward(mu, None, Mb, Sb, Vb)
    e = engine.moments_backward(mu, np.zeros((P, E, E)), Mb, Sb, Vb)
    assert torch.equal(o["mu_bar"], e["mu_bar"]) and torch.equal(o["var_bar"], e["var_bar"])
    full = engine.moments_backward(mu, var, Mb, Sb, Vb)
    L = engine.lib
    dev = engine.device
    t = lambda a: torch.tensor(a, device=dev)                        # noqa: E731
    m_, v_, Mb_, Sb_, Vb_ = t(mu), t(var), t(Mb), t(Sb), t(Vb)
    sm = torch.full((P, E), 7.25, dtype=torch.float64, device=dev)
    sv = torch.full((P, E, E), 7.25, dtype=torch.float64, device=dev)
    assert L.gpmpc_moments_backward(engine._h, m_.data_ptr(), v_.data_ptr(), P, D, E, Mb_.data_ptr(), Sb_.data_ptr(),
                                    Vb_.data_ptr(), sm.data_ptr(), None, engine._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(sm, full["mu_bar"]) and torch.all(sv == 7.25)
    sm.fill_(7.25)
    assert L.gpmpc_moments_backward(engine._h, m_.data_ptr(), v_.data_ptr(), P, D, E, Mb_.data_ptr(), Sb_.data_ptr(),
                                    Vb_.data_ptr(), None, sv.data_ptr(), engine._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(sv, full["var_bar"]) and torch.all(sm == 7.25)


def test_errors():
    from gp_mpc_amd import _lib as L
    eng = _fresh()
    try:
        mu = torch.zeros((4, 25), dtype=torch.float64, device=eng.device)
        out = torch.empty((4 * 25 * 25,), dtype=torch.float64, device=eng.device)

        def call(P, D, E, m=mu):
            return eng.lib.gpmpc_moments_backward(eng._h, m.data_ptr() if m is not None else None, None, P, D, E, None, None,
                                                  None, out.data_ptr(), out.data_ptr(), eng._stream())
        assert call(4, 3, 4) == L.GPMPC_ERR_ARG and "prepare" in eng.lib.gpmpc_last_error(eng._h).decode()
        w = synth.make_workload(40, 3, 1, 2, 1, seed=360)
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        for P, D, E in ((4, 3, 5), (4, 2, 4), (-1, 3, 4)):
            assert call(P, D, E) == L.GPMPC_ERR_ARG, (P, D, E)
        assert call(4, 3, 4, m=None) == L.GPMPC_ERR_ARG
        assert call(4, 3, 25) == L.GPMPC_ERR_LIMIT
        assert call(4, 17, 4) == L.GPMPC_ERR_LIMIT
        assert call(0, 3, 4) == L.GPMPC_OK and call(0, 3, 4, m=None) == L.GPMPC_OK
        assert call(4, 3, 4) == L.GPMPC_OK
        with pytest.raises(RuntimeError):
            eng.set_option("moments_backward_chunk_points", -1)
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
        mu, var = _inputs(w, 200, seed=370)
        fwd0 = {k: v.clone() for k, v in eng.moments(mu, var).items()}
        state = (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode)
        D, E = w.Y.shape[1], w.X.shape[1]
        eng.moments_backward(mu, var, *_upstream(200, D, E, seed=371))
        assert (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode) == state
        after = eng.rollout(w.actions, w.mu0, w.S0)
        for k in before:
            assert torch.equal(before[k], after[k]), k
        eng.moments_backward(mu[:20], var[:20], *_upstream(20, D, E, seed=372))
        fwd1 = eng.moments(mu, var)
        for k in fwd0:
            assert torch.equal(fwd0[k], fwd1[k]), k
    finally:
        eng.close()


def test_wide_covariance_is_finite(engine):
    w = synth.make_workload(200, 3, 2, 2, 1, seed=380)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    mu, var = _inputs(w, 8, seed=381, scale=30.0)
    o = engine.moments_backward(mu, var, *_upstream(8, 3, 5, seed=382))
    assert torch.isfinite(o["mu_bar"]).all() and torch.isfinite(o["var_bar"]).all()
