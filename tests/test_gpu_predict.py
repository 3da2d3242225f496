"""Tier 2 (GPU): gpmpc_predict -- the GP posterior mean / variance at deterministic query inputs.

Pinned to the reference by tests/golden/predict_batch*.npz (predict_next_state_change at zero input variance,
tools/gen_golden_predict.py; tests/test_predict_reference.py ties that golden to the closed form used here), to an
extended-precision evaluation of the same formula on the same fp64 factors, and to the contracts of include/gpmpc.h:
bitwise batch invariance, outputs that may be NULL, argument errors and no interference with the rest of the handle.
"""
import numpy as np
import pytest
import torch

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


def closed_form(X, ls, os_, iK, beta, Xq, dtype=np.float64):
    """(mean, var) (M, D) of the zero-mean RBF-ARD GPs at the rows of Xq, evaluated in `dtype`."""
    X, ls, os_, beta, Xq = (np.asarray(v, dtype=dtype) for v in (X, ls, os_, beta, Xq))
    D = beta.shape[0]
    mean = np.empty((Xq.shape[0], D), dtype=dtype)
    var = np.empty((Xq.shape[0], D), dtype=dtype)
    for a in range(D):
        d = (Xq[:, None, :] - X[None, :, :]) / ls[a]
        k = os_[a] * np.exp(-0.5 * np.sum(d * d, axis=-1))
        mean[:, a] = k @ beta[a]
        var[:, a] = os_[a] - np.sum((k @ np.asarray(iK[a], dtype=dtype)) * k, axis=1)
    return mean, var


def _np(t):
    return t.cpu().numpy()


def _queries(w, M_rand, n_mem, seed):
    rng = np.random.default_rng(seed)
    lo, hi = w.X.min(axis=0), w.X.max(axis=0)
    pts = [lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(M_rand, w.X.shape[1]))]
    if n_mem:
        pts.append(w.X[rng.choice(w.X.shape[0], n_mem, replace=False)])
    return np.concatenate(pts)


# -- 1. goldens of the reference's own code -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["predict_batch", "predict_batch_time"])
@pytest.mark.parametrize("load_by", ["set_factors", "prepare"])
def test_goldens(engine, name, load_by):
    g = load(name)
    w = workload_of(g)
    if load_by == "set_factors":
        engine.set_factors(w.X, g["iK"], g["beta"], w.lengthscales, w.outputscales)
    else:
        engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    out = engine.predict(g["Xq"])
    mean, var = _np(out["mean"]), _np(out["var"])
    S = g["S"]
    e_M = rel_err(mean, g["M"])
    e_S = rel_err(var, np.diagonal(S, axis1=1, axis2=2))          # scale-relative over the batch, as the single-step tests
    record(f"predict_golden[{name},{load_by}]", M=e_M, S_diag=e_S)
    assert e_M < 1e-10
    assert e_S < 1e-7          # their covariance tolerance (test_gpu_parity.py)
    kind = g["kind"]
    assert np.all(var[kind == 2] == w.outputscales) and np.all(mean[kind == 2] == 0.0)


def test_step_zero_var_golden(engine):
    g = load("step_zero_var")
    w = workload_of(g)
    D = w.Y.shape[1]
    engine.set_factors(w.X, g["iK"], g["beta"], w.lengthscales, w.outputscales)
    out = engine.predict(g["in_mean"][None])
    assert rel_err(_np(out["mean"])[0], g["M"].ravel()) < 1e-10
    assert rel_err(_np(out["var"])[0], np.diag(g["S"])[:D]) < 1e-7


# -- 2. extended precision ---------------------------------------------------------------------------------------------------
SHAPES = {   # N, D, A, random points, memory points, rows checked in long double (all of them when None)
    "c2": (200, 3, 1, 48, 16, None),
    "c4": (1000, 4, 2, 48, 16, None),
    "c5": (4096, 16, 4, 240, 16, [0, 1, 240, 241]),      # long double products of 4096^2: a few rows
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_extended_precision(engine, shape):
    N, D, A, M_rand, n_mem, rows = SHAPES[shape]
    w = synth.make_workload(N, D, A, 2, 1, seed=70 + N)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    iK, beta = (_np(t) for t in engine.factors())
    Xq = _queries(w, M_rand, n_mem, seed=71)
    out = engine.predict(Xq)
    mean, var = _np(out["mean"]), _np(out["var"])
    sel = np.arange(len(Xq)) if rows is None else np.asarray(rows)
    m64, v64 = closed_form(w.X, w.lengthscales, w.outputscales, iK, beta, Xq[sel])
    mx, vx = closed_form(w.X, w.lengthscales, w.outputscales, iK, beta, Xq[sel], dtype=np.longdouble)
    # worst case over the batch: the HIP product's rounding is that of a plain fp64 evaluation (numpy's, same factors)
    err_hip = float(np.max(np.abs(var[sel] - vx)))
    err_np = float(np.max(np.abs(v64 - vx)))
    e_mean = rel_err(mean[sel], mx.astype(np.float64))
    record(f"predict_extended[{shape}]", mean=e_mean, var_hip=err_hip, var_numpy=err_np)
    assert err_hip <= 3 * max(err_np, 1e-12 * float(np.max(w.outputscales))), (err_hip, err_np)
    assert e_mean < 1e-10


# -- 3. bitwise batch invariance ---------------------------------------------------------------------------------------------
def test_batch_invariance_plot_shape(engine):
    w = synth.make_workload(1500, 3, 1, 2, 1, seed=80)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    rng = np.random.default_rng(81)
    g = np.linspace(0.0, 1.0, 75)
    Xq = np.tile(rng.uniform(0.0, 1.0, size=4), (75 * 75, 1))
    Xq[:, 0] = np.repeat(g, 75)
    Xq[:, 1] = np.tile(g, 75)
    full = engine.predict(Xq)
    again = engine.predict(Xq)
    rev = engine.predict(Xq[::-1].copy())
    for k in ("mean", "var"):
        assert torch.equal(full[k], again[k])
        assert torch.equal(full[k], rev[k].flip(0))
    for i in (0, 63, 64, 2812, 5624):
        one = engine.predict(Xq[i:i + 1])
        for k in ("mean", "var"):
            assert torch.equal(one[k][0], full[k][i])
    # internal chunks of 64 rows: results do not depend on where the chunk boundaries fall
    engine.set_option("predict_chunk_rows", 64)
    try:
        chunked = engine.predict(Xq[:300])
    finally:
        engine.set_option("predict_chunk_rows", 0)
    for k in ("mean", "var"):
        assert torch.equal(chunked[k], full[k][:300])
    # a different neighbourhood in the batch
    mixed = np.concatenate([Xq[100:101], w.X[:7], Xq[5000:5001]])
    out = engine.predict(mixed)
    for k in ("mean", "var"):
        assert torch.equal(out[k][0], full[k][100]) and torch.equal(out[k][8], full[k][5000])


# -- 4. noise and far points -------------------------------------------------------------------------------------------------
def test_noise_and_far_points(engine):
    w = synth.make_workload(200, 3, 1, 2, 1, seed=90)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    Xq = np.concatenate([_queries(w, 20, 8, seed=91), 1e3 + np.arange(12)[:, None] * np.ones((1, 4))])
    noises = np.array([1e-5, 3e-4, 2e-2])
    v0 = _np(engine.predict(Xq)["var"])
    o = engine.predict(Xq, noises=noises)
    vn, mn = _np(o["var"]), _np(o["mean"])
    assert np.all(np.abs((vn - v0) - noises[None, :]) <= np.spacing(np.abs(vn)))
    far = slice(28, 40)
    assert np.all(v0[far] == w.outputscales[None, :])
    assert np.all(vn[far] == w.outputscales[None, :] + noises[None, :])
    assert np.all(mn[far] == 0.0)


# -- 5. edge shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,A", [(1, 3, 1), (50, 3, 1), (203, 3, 1), (203, 1, 1), (203, 16, 2), (300, 2, 1)])
def test_edge_shapes(engine, N, D, A):
    w = synth.make_workload(N, D, A, 2, 1, seed=100 + N + D)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    iK, beta = (_np(t) for t in engine.factors())
    Xq = _queries(w, 70, min(N, 5), seed=101)
    out = engine.predict(Xq)
    m64, v64 = closed_form(w.X, w.lengthscales, w.outputscales, iK, beta, Xq)
    assert rel_err(_np(out["mean"]), m64) < 1e-10
    assert np.max(np.abs(_np(out["var"]) - v64)) < 1e-10 * w.outputscales.max()
    # one output only: the same bits as with both
    mo = engine.predict(Xq, var=False)
    vo = engine.predict(Xq, mean=False)
    assert set(mo) == {"mean"} and set(vo) == {"var"}
    assert torch.equal(mo["mean"], out["mean"]) and torch.equal(vo["var"], out["var"])
    # M = 0: nothing to do
    z = engine.predict(np.zeros((0, w.X.shape[1])))
    assert z["mean"].shape == (0, D) and z["var"].shape == (0, D)


def test_null_outputs_leave_buffers_alone(engine):
    w = synth.make_workload(64, 3, 1, 2, 1, seed=110)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    Xq = engine._dev(_queries(w, 10, 0, seed=111))
    sentinel = torch.full((10, 3), 7.0, dtype=torch.float64, device=engine.device)
    engine._check(engine.lib.gpmpc_predict(engine._h, Xq.data_ptr(), 10, 3, 4, None, None, sentinel.data_ptr(), engine._stream()))
    torch.cuda.synchronize()
    assert not torch.any(sentinel == 7.0)
    sentinel.fill_(7.0)
    engine._check(engine.lib.gpmpc_predict(engine._h, Xq.data_ptr(), 0, 3, 4, None, sentinel.data_ptr(), sentinel.data_ptr(),
                                           engine._stream()))
    torch.cuda.synchronize()
    assert torch.all(sentinel == 7.0)


# -- 6. errors ---------------------------------------------------------------------------------------------------------------
def test_errors():
    from gp_mpc_amd import _lib as L
    eng = _fresh()
    try:
        Xq = torch.zeros((4, 4), dtype=torch.float64, device=eng.device)
        out = torch.empty((4, 3), dtype=torch.float64, device=eng.device)

        def call(M, D, E):
            return eng.lib.gpmpc_predict(eng._h, Xq.data_ptr(), M, D, E, None, out.data_ptr(), out.data_ptr(), eng._stream())
        rc = call(4, 3, 4)
        assert rc == L.GPMPC_ERR_ARG and "prepare" in eng.lib.gpmpc_last_error(eng._h).decode()
        with pytest.raises(RuntimeError) as ei:          # GpmpcError (of the module the engine was loaded through)
            eng.predict(Xq)
        assert type(ei.value).__name__ == "GpmpcError" and ei.value.code == L.GPMPC_ERR_ARG
        w = synth.make_workload(40, 3, 1, 2, 1, seed=120)
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        for M, D, E in ((4, 3, 5), (4, 2, 4), (-1, 3, 4)):
            assert call(M, D, E) == L.GPMPC_ERR_ARG
            assert eng.lib.gpmpc_last_error(eng._h).decode()
        with pytest.raises(RuntimeError) as ei:          # GpmpcError (of the module the engine was loaded through)
            eng.predict(np.zeros((4, 5)))
        assert type(ei.value).__name__ == "GpmpcError" and ei.value.code == L.GPMPC_ERR_ARG
        assert call(4, 3, 4) == L.GPMPC_OK
    finally:
        eng.close()


# -- 7. no interference with the rest of the handle ---------------------------------------------------------------------------
def test_no_interference():
    g = load("traj_c2")
    w = workload_of(g)
    eng = _fresh()
    try:
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        before = {k: v.clone() for k, v in eng.rollout(w.actions, w.mu0, w.S0).items()}
        state = (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode)
        eng.predict(_queries(w, 500, 16, seed=130), noises=w.noises)
        assert (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode) == state
        after = eng.rollout(w.actions, w.mu0, w.S0)
        for k in before:
            assert torch.equal(before[k], after[k]), k
        # the memory grows by 4 points: still a border update after a predict
        x = synth.make_workload(204, 3, 1, 2, 1, seed=131)
        eng.prepare(x.X[:200], x.Y[:200], w.lengthscales, w.outputscales, w.noises)
        eng.predict(x.X[:50])
        eng.prepare(x.X, x.Y, w.lengthscales, w.outputscales, w.noises)
        assert eng.last_prepare_mode == 1
    finally:
        eng.close()


# -- 8. Python level ---------------------------------------------------------------------------------------------------------
def test_transition_model_predict(engine):
    from gp_mpc_amd.config_classes import ModelConfig
    from gp_mpc_amd.control_objects.models.gp_model import GpStateTransitionModel
    model = GpStateTransitionModel(ModelConfig(), 3, 1, engine=engine)
    w = synth.make_workload(120, 3, 1, 2, 1, seed=140)
    Xq = _queries(w, 30, 5, seed=141)
    with pytest.raises(RuntimeError):
        model.predict(Xq)
    model.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    mean, var = model.predict(Xq)
    ref = engine.predict(Xq, noises=model.noises.detach().cpu().numpy())
    assert mean.device.type == "cuda" and var.device.type == "cuda"
    assert torch.equal(mean, ref["mean"]) and torch.equal(var, ref["var"])
    mean0, var0 = model.predict(Xq, include_noise=False)
    assert torch.equal(mean0, mean)
    assert torch.equal(var0, engine.predict(Xq)["var"])
