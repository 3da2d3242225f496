"""Tier 2 (GPU): gpmpc_predict_cov -- the joint GP posterior covariance between query points.

Pinned to the reference by the diagonal of tests/golden/predict_batch*.npz (tests/test_predict_cov_reference.py ties those
goldens to the closed form of tests/predict_cov_ref.py, and its off-diagonal to an independent Schur complement), to an
extended-precision evaluation of the same formula on the same fp64 factors, and to the contracts of include/gpmpc.h: exact
symmetry, bitwise invariance of an element under everything but its two points, argument errors and no interference with
the rest of the handle.
"""
import numpy as np
import pytest
import torch

from helpers import load, workload_of, rel_err, record
from oracle import synth
from predict_cov_ref import closed_form_cov

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


def _diag(C):
    return np.diagonal(C, axis1=1, axis2=2)          # (D, M)


def _queries(w, M_rand, n_mem, n_dup, seed):
    """Random points of the memory's box, memory points, and near-duplicates of the first n_dup random points (two almost
    equal rows and columns: the prior term and the data term cancel to the last digits)."""
    rng = np.random.default_rng(seed)
    lo, hi = w.X.min(axis=0), w.X.max(axis=0)
    pts = [lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(M_rand, w.X.shape[1]))]
    if n_mem:
        pts.append(w.X[rng.choice(w.X.shape[0], n_mem, replace=False)])
    if n_dup:
        pts.append(pts[0][:n_dup] + 1e-6 * rng.standard_normal((n_dup, w.X.shape[1])))
    return np.concatenate(pts)


def _bound(err_np, w):
    """The rule of test_gpu_predict.py::test_against_extended_precision."""
    return 3 * max(err_np, 1e-12 * float(np.max(w.outputscales)))


# -- 1. goldens of the reference's own code -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["predict_batch", "predict_batch_time"])
@pytest.mark.parametrize("load_by", ["set_factors", "prepare"])
def test_goldens(engine, name, load_by):
    g = load(name)
    w = workload_of(g)
    D = w.Y.shape[1]
    if load_by == "set_factors":
        engine.set_factors(w.X, g["iK"], g["beta"], w.lengthscales, w.outputscales)
        iK = g["iK"]
    else:
        engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        iK = _np(engine.factors()[0])
    cov = _np(engine.predict_cov(g["Xq"]))
    assert cov.shape == (D, 48, 48)
    e_S = rel_err(_diag(cov).T, g["S"][:, range(D), range(D)])
    ref = closed_form_cov(w.X, w.lengthscales, w.outputscales, iK, g["Xq"])
    e_full = float(np.max(np.abs(cov - ref)))
    record(f"predict_cov_golden[{name},{load_by}]", S_diag=e_S, full_abs=e_full)
    assert e_S < 1e-7          # the covariance tolerance of test_gpu_predict.py::test_goldens
    # the same factors in numpy fp64: the bound of test_gpu_predict.py::test_edge_shapes for the variance
    assert e_full < 1e-10 * w.outputscales.max()
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2))
    far = np.flatnonzero(g["kind"] == 2)
    assert np.all(_diag(cov)[:, far] == w.outputscales[:, None])


# -- 2. extended precision ---------------------------------------------------------------------------------------------------
SHAPES = {   # N, D, A, random points, memory points, near-duplicates, rows checked in long double (all of them when None)
    "c2": (200, 3, 1, 48, 16, 8, None),
    "c4": (1000, 4, 2, 48, 16, 8, None),
    "c5": (4096, 16, 4, 240, 16, 8, [0, 1, 240, 256]),      # long double products of 4096^2: a few rows
}


def _extended(engine, shape):
    """HIP joint covariance, numpy fp64 and long double closed forms on the engine's own factors (rows `sel` of the matrix)."""
    N, D, A, M_rand, n_mem, n_dup, rows = SHAPES[shape]
    w = synth.make_workload(N, D, A, 2, 1, seed=70 + N)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    iK = _np(engine.factors()[0])
    Xq = _queries(w, M_rand, n_mem, n_dup, seed=72)
    cov = _np(engine.predict_cov(Xq))
    args = (w.X, w.lengthscales, w.outputscales, iK)
    if rows is None:
        sel = np.arange(len(Xq))
        c64 = closed_form_cov(*args, Xq)
        cx = closed_form_cov(*args, Xq, dtype=np.longdouble)
    else:
        # rows of the joint form: with an exactly symmetric iK (prepare stores one) t(x_i, x_j) = t(x_j, x_i) in exact
        # arithmetic, so the cross form of these rows against all points is the joint form's rows
        assert np.array_equal(iK, np.swapaxes(iK, 1, 2))
        sel = np.asarray(rows)
        c64 = closed_form_cov(*args, Xq[sel], Xq)
        cx = closed_form_cov(*args, Xq[sel], Xq, dtype=np.longdouble)
    return w, Xq, sel, cov, c64, cx


@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_extended_precision(engine, shape):
    w, Xq, sel, cov, c64, cx = _extended(engine, shape)
    err_hip = float(np.max(np.abs(cov[:, sel] - cx)))
    err_np = float(np.max(np.abs(c64 - cx)))
    record(f"predict_cov_extended[{shape}]", cov_hip=err_hip, cov_numpy=err_np)
    print(f"predict_cov_extended[{shape}]: HIP {err_hip:.3e} numpy {err_np:.3e}")
    assert err_hip <= _bound(err_np, w), (err_hip, err_np)
    # the cross form of the same rows against all points
    cross = _np(engine.predict_cov(Xq[sel], Xq))
    err_cross = float(np.max(np.abs(cross - cx)))
    record(f"predict_cov_extended[{shape}]", cross_hip=err_cross)
    assert err_cross <= _bound(err_np, w), (err_cross, err_np)


# -- 3. positive semi-definiteness -------------------------------------------------------------------------------------------
def test_positive_semidefinite(engine):
    w, Xq, sel, cov, c64, cx = _extended(engine, "c2")
    s2 = float(np.max(w.outputscales))
    for a in range(cov.shape[0]):
        l_hip = float(np.linalg.eigvalsh(cov[a])[0])
        l_np = float(np.linalg.eigvalsh(c64[a])[0])
        record(f"predict_cov_psd[c2,{a}]", lmin_hip=l_hip, lmin_numpy=l_np)
        print(f"predict_cov_psd[c2,{a}]: lambda_min HIP {l_hip:.3e} numpy {l_np:.3e}")
        assert l_hip >= 3 * min(l_np, 0.0) - 1e-12 * s2, (a, l_hip, l_np)
    noisy = _np(engine.predict_cov(Xq, noises=w.noises))
    for a in range(noisy.shape[0]):
        np.linalg.cholesky(noisy[a])                  # raises LinAlgError when not positive definite


# -- 4. consistency with gpmpc_predict ---------------------------------------------------------------------------------------
def test_diagonal_is_predict_variance(engine):
    w, Xq, sel, cov, c64, cx = _extended(engine, "c2")
    bound = _bound(float(np.max(np.abs(c64 - cx))), w)
    var = _np(engine.predict(Xq, mean=False)["var"])
    e0 = float(np.max(np.abs(_diag(cov).T - var)))
    noises = np.array([1e-5, 3e-4, 2e-2])
    covn = _np(engine.predict_cov(Xq, noises=noises))
    varn = _np(engine.predict(Xq, noises=noises, mean=False)["var"])
    e1 = float(np.max(np.abs(_diag(covn).T - varn)))
    record("predict_cov_vs_predict[c2]", plain=e0, noisy=e1, bound=bound)
    print(f"predict_cov_vs_predict[c2]: plain {e0:.3e} noisy {e1:.3e} bound {bound:.3e}")
    assert e0 <= bound and e1 <= bound
    off = covn - cov
    off[:, range(len(Xq)), range(len(Xq))] = 0.0
    assert np.all(off == 0.0)                         # the noise touches the diagonal only


# -- 5. bitwise invariance ---------------------------------------------------------------------------------------------------
def test_bitwise_invariance(engine):
    w = synth.make_workload(203, 3, 1, 2, 1, seed=80)                  # N not a multiple of 16
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    rng = np.random.default_rng(81)
    M = 5000
    Xq = rng.uniform(0.0, 1.0, size=(M, 4))
    full = engine.predict_cov(Xq)
    assert torch.equal(full, full.transpose(1, 2))                     # exactly symmetric
    assert torch.equal(full, engine.predict_cov(Xq))
    rev = engine.predict_cov(Xq[::-1].copy())
    assert torch.equal(rev.flip(1, 2), full)
    del rev
    # a 2-point call reproduces the element of the big call, across tile and chunk boundaries
    marks = [0, 63, 64, 127, 128, 255, 256, M - 1]
    for i, j in [(0, 63), (63, 64), (64, 0), (127, 128), (255, 256), (256, M - 1), (M - 1, 0), (64, 4111)]:
        two = engine.predict_cov(Xq[[i, j]])
        assert torch.equal(two[:, 0, 1], full[:, i, j]) and torch.equal(two[:, 1, 0], full[:, j, i]), (i, j)
        assert torch.equal(two[:, 0, 0], full[:, i, i]) and torch.equal(two[:, 1, 1], full[:, j, j]), (i, j)
    one = engine.predict_cov(Xq[300:301])
    assert one.shape == (3, 1, 1) and torch.equal(one[:, 0, 0], full[:, 300, 300])
    # a permuted subset gives the permuted block
    perm = rng.permutation(M)[:701]
    pt = torch.as_tensor(perm, device=full.device)
    assert torch.equal(engine.predict_cov(Xq[perm]), full[:, pt][:, :, pt])
    # internal chunks of 64 rows: the bits do not depend on where the chunk boundaries fall
    noises = np.array([1e-5, 3e-4, 2e-2])
    full_n = engine.predict_cov(Xq[:300], noises=noises)
    engine.set_option("predict_cov_chunk_rows", 64)
    try:
        chunked = engine.predict_cov(Xq[:300])
        chunked_n = engine.predict_cov(Xq[:300], noises=noises)
        chunked_x = engine.predict_cov(Xq[100:333], Xq[5:170])
    finally:
        engine.set_option("predict_cov_chunk_rows", 0)
    assert torch.equal(chunked, full[:, :300, :300])
    assert torch.equal(chunked_n, full_n)
    assert torch.equal(chunked_x, engine.predict_cov(Xq[100:333], Xq[5:170]))
    with pytest.raises(RuntimeError):
        engine.set_option("predict_cov_chunk_rows", 100)
    # cross forms of different subsets agree wherever they share an ordered pair (sizes not multiples of 64)
    c1 = engine.predict_cov(Xq[100:333], Xq[5:170])                    # rows 100..332, columns 5..169
    c2 = engine.predict_cov(Xq[60:201], Xq[150:451])                   # rows 60..200, columns 150..450
    assert c1.shape == (3, 233, 165) and c2.shape == (3, 141, 301)
    assert torch.equal(c1[:, 0:101, 145:165], c2[:, 40:141, 0:20])     # rows 100..200, columns 150..169
    c3 = engine.predict_cov(Xq[marks], Xq[:1])                         # Mb = 1
    c4 = engine.predict_cov(Xq[:1], Xq[marks])                         # Ma = 1
    cs = engine.predict_cov(Xq[:1000], Xq[:1000])
    mt = torch.as_tensor(marks[:-1], device=full.device)
    assert torch.equal(c3[:, :-1, 0], cs[:, mt, 0])
    assert torch.equal(c4[:, 0, :-1], cs[:, 0, mt])
    # the joint form is the average of the cross form and its transpose, bit for bit
    assert torch.equal(0.5 * (cs + cs.transpose(1, 2)), full[:, :1000, :1000])


# -- 6. edge shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,A", [(1, 3, 1), (50, 3, 1), (203, 3, 1), (203, 1, 1), (203, 8, 2), (203, 16, 2)])
def test_edge_shapes(engine, N, D, A):
    w = synth.make_workload(N, D, A, 2, 1, seed=100 + N + D)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    iK = _np(engine.factors()[0])
    E = w.X.shape[1]
    Xq = _queries(w, 70, min(N, 5), 3, seed=101)                       # Ma not a multiple of 64
    args = (w.X, w.lengthscales, w.outputscales, iK)
    tol = 1e-10 * w.outputscales.max()                                 # test_gpu_predict.py::test_edge_shapes
    cov = _np(engine.predict_cov(Xq, noises=w.noises))
    assert np.max(np.abs(cov - closed_form_cov(*args, Xq, noises=w.noises))) < tol
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2))
    for sa, sb in ((slice(0, 1), slice(0, None)), (slice(0, None), slice(3, 4)), (slice(2, 3), slice(7, 8)), (slice(0, 70), slice(5, 78))):
        cross = _np(engine.predict_cov(Xq[sa], Xq[sb]))
        assert np.max(np.abs(cross - closed_form_cov(*args, Xq[sa], Xq[sb]))) < tol
    # nothing to do
    assert engine.predict_cov(np.zeros((0, E))).shape == (D, 0, 0)
    assert engine.predict_cov(np.zeros((0, E)), Xq).shape == (D, 0, len(Xq))
    assert engine.predict_cov(Xq, np.zeros((0, E))).shape == (D, len(Xq), 0)


def test_far_points(engine):
    w = synth.make_workload(200, 3, 1, 2, 1, seed=90)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    near = _queries(w, 20, 8, 0, seed=91)
    far = 1e3 + 1e2 * np.arange(12)[:, None] * np.ones((1, 4))         # far from the memory and from each other
    Xq = np.concatenate([near, far])
    noises = np.array([1e-5, 3e-4, 2e-2])
    c0 = _np(engine.predict_cov(Xq))
    cn = _np(engine.predict_cov(Xq, noises=noises))
    f = slice(28, 40)
    eye = np.eye(12)[None]
    assert np.all(c0[:, f, f] == w.outputscales[:, None, None] * eye)
    assert np.all(cn[:, f, f] == (w.outputscales + noises)[:, None, None] * eye)
    assert np.all(c0[:, f, :28] == 0.0) and np.all(c0[:, :28, f] == 0.0)
    cross = _np(engine.predict_cov(far, near))
    assert np.all(cross == 0.0)
    assert np.all(_np(engine.predict_cov(far[:5], far[5:])) == 0.0)


# -- 7. errors and NULLs -----------------------------------------------------------------------------------------------------
def test_errors_and_nulls():
    from gp_mpc_amd import _lib as L
    eng = _fresh()
    try:
        Xa = torch.zeros((4, 4), dtype=torch.float64, device=eng.device)
        Xb = torch.zeros((5, 4), dtype=torch.float64, device=eng.device)
        out = torch.full((3, 4, 5), 7.0, dtype=torch.float64, device=eng.device)
        nz = np.full(3, 1e-3)
        nzp = nz.ctypes.data_as(L.C.c_void_p)

        def call(Ma=4, Mb=5, D=3, E=4, xa=True, xb=True, noise=False, o=True):
            return eng.lib.gpmpc_predict_cov(eng._h, Xa.data_ptr() if xa else None, Ma, Xb.data_ptr() if xb else None, Mb, D, E,
                                             nzp if noise else None, out.data_ptr() if o else None, eng._stream())
        assert call() == L.GPMPC_ERR_ARG and "prepare" in eng.lib.gpmpc_last_error(eng._h).decode()
        with pytest.raises(RuntimeError) as ei:          # GpmpcError (of the module the engine was loaded through)
            eng.predict_cov(Xa)
        assert type(ei.value).__name__ == "GpmpcError" and ei.value.code == L.GPMPC_ERR_ARG
        w = synth.make_workload(40, 3, 1, 2, 1, seed=120)
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        bad = [dict(E=5), dict(D=2), dict(Ma=-1), dict(Mb=-1), dict(Ma=-1, xb=False), dict(xa=False), dict(o=False),
               dict(xa=False, xb=False), dict(noise=True)]
        for kw in bad:
            eng.lib.gpmpc_predict_cov(eng._h, None, 0, None, 0, 3, 4, None, None, eng._stream())   # a good (empty) call in between
            assert call(**kw) == L.GPMPC_ERR_ARG, kw
            assert eng.lib.gpmpc_last_error(eng._h).decode(), kw
        torch.cuda.synchronize()
        assert torch.all(out == 7.0)
        with pytest.raises(RuntimeError) as ei:
            eng.predict_cov(np.zeros((4, 5)))
        assert type(ei.value).__name__ == "GpmpcError" and ei.value.code == L.GPMPC_ERR_ARG
        with pytest.raises(RuntimeError) as ei:
            eng.predict_cov(Xa, Xb, noises=nz)
        assert type(ei.value).__name__ == "GpmpcError" and ei.value.code == L.GPMPC_ERR_ARG
        with pytest.raises(ValueError):
            eng.predict_cov(Xa, np.zeros((5, 3)))
        with pytest.raises(ValueError):
            eng.predict_cov(Xa, noises=np.zeros(2))
        # nothing is launched and nothing written: Ma = 0 (NULL pointers allowed), Mb = 0 in the cross form
        assert call(Ma=0) == L.GPMPC_OK and call(Mb=0) == L.GPMPC_OK and call(Ma=0, xb=False, noise=True) == L.GPMPC_OK
        assert call(Ma=0, xa=False, o=False) == L.GPMPC_OK and call(Mb=0, o=False) == L.GPMPC_OK
        torch.cuda.synchronize()
        assert torch.all(out == 7.0)
        # good calls afterwards; in the joint form Mb is ignored
        assert call() == L.GPMPC_OK
        torch.cuda.synchronize()
        assert not torch.any(out == 7.0)
        jout = torch.full((3, 4, 4), 7.0, dtype=torch.float64, device=eng.device)
        rc = eng.lib.gpmpc_predict_cov(eng._h, Xa.data_ptr(), 4, None, -3, 3, 4, nzp, jout.data_ptr(), eng._stream())
        assert rc == L.GPMPC_OK
        torch.cuda.synchronize()
        assert torch.equal(jout, eng.predict_cov(Xa, noises=nz))
    finally:
        eng.close()


# -- 8. no interference with the rest of the handle ---------------------------------------------------------------------------
def test_no_interference():
    g = load("traj_c2")
    w = workload_of(g)
    eng = _fresh()
    try:
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        before = {k: v.clone() for k, v in eng.rollout(w.actions, w.mu0, w.S0).items()}
        pred = {k: v.clone() for k, v in eng.predict(w.X[:40]).items()}
        state = (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode, eng.last_grad_path)
        Xq = _queries(w, 500, 16, 4, seed=130)
        eng.predict_cov(Xq, noises=w.noises)
        eng.predict_cov(Xq[:100], Xq[50:])
        assert (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode, eng.last_grad_path) == state
        after = eng.rollout(w.actions, w.mu0, w.S0)
        for k in before:
            assert torch.equal(before[k], after[k]), k
        again = eng.predict(w.X[:40])
        for k in pred:
            assert torch.equal(pred[k], again[k]), k
        # the memory grows by 4 points: still a border update after a predict_cov
        x = synth.make_workload(204, 3, 1, 2, 1, seed=131)
        eng.prepare(x.X[:200], x.Y[:200], w.lengthscales, w.outputscales, w.noises)
        eng.predict_cov(x.X[:50])
        eng.prepare(x.X, x.Y, w.lengthscales, w.outputscales, w.noises)
        assert eng.last_prepare_mode == 1
        # after a forget the covariance is that of the reduced model
        gone = [3, 77, 200]
        eng.forget(gone)
        keep = np.setdiff1d(np.arange(204), gone)
        iK = _np(eng.factors()[0])
        assert iK.shape == (3, 201, 201)
        Xq = _queries(x, 40, 8, 2, seed=132)
        cov = _np(eng.predict_cov(Xq))
        ref = closed_form_cov(x.X[keep], w.lengthscales, w.outputscales, iK, Xq)
        assert np.max(np.abs(cov - ref)) < 1e-10 * w.outputscales.max()
    finally:
        eng.close()


# -- 9. Python level ---------------------------------------------------------------------------------------------------------
def test_transition_model_predict_cov(engine):
    from gp_mpc_amd.config_classes import ModelConfig
    from gp_mpc_amd.control_objects.models.gp_model import GpStateTransitionModel
    model = GpStateTransitionModel(ModelConfig(), 3, 1, engine=engine)
    w = synth.make_workload(120, 3, 1, 2, 1, seed=140)
    Xq = _queries(w, 30, 5, 2, seed=141)
    with pytest.raises(RuntimeError):
        model.predict_cov(Xq)
    model.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    cov = model.predict_cov(Xq)
    assert cov.device.type == "cuda" and cov.shape == (3, 37, 37)
    assert torch.equal(cov, engine.predict_cov(Xq, noises=model.noises.detach().cpu().numpy()))
    assert torch.equal(model.predict_cov(Xq, include_noise=False), engine.predict_cov(Xq))
    cross = model.predict_cov(Xq[:10], Xq[4:])
    assert torch.equal(cross, engine.predict_cov(Xq[:10], Xq[4:]))
    assert torch.equal(cross, model.predict_cov(Xq[:10], Xq[4:], include_noise=False))
    # no autograd for this entry
    xg = torch.as_tensor(Xq).requires_grad_(True)
    assert not model.predict_cov(xg).requires_grad
