"""Tier 2 (GPU): gpmpc_select_inducing -- greedy variance selection of the inducing inputs of the sparse model.

The picks are compared index for index with the longdouble restatement of tests/select_inducing_ref.py: that is meaningful because
tests/test_select_inducing_reference.py shows, for every case compared here, that the float64 and longdouble runs agree and that no
choice is closer than 1e-9 (relative) to its runner-up, four orders above the error of a float64 score.  The trace by the rule of
test_gpu_prepare_sparse.py:
    tolerance = 10 e64 + 64 eps max|trace_ld|      (e64: the float64 restatement's own error against longdouble on that case,
                                                    computed here, never taken from the GPU; eps = 2^-52)
and the contracts of include/gpmpc.h: Z = X[idx] bit for bit, NULL outputs, bitwise determinism, isolation from the cached model,
errors before any launch, the workspace cap, and the model-level option ModelConfig.inducing_selection.

Measured on an MI355X, |trace - longdouble| HIP / numpy float64 / bound: see DESIGN.md 4.4.3.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import select_inducing_ref as ref
import sparse_gp_ref as sgr
from helpers import record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import gp_mpc_amd
    eng = gp_mpc_amd.HipEngine(0)
    yield eng
    eng.close()


_RESULTS = {}


def _run(eng, name):
    """One selection per case, shared by the tests (the second call of the determinism test is its own)."""
    if name not in _RESULTS:
        c = ref.case(name)
        out = eng.select_inducing(c.X, c.M, c.ls, c.os, c.jitter_rel)
        _RESULTS[name] = {k: v.cpu().numpy() for k, v in out.items()}
    return _RESULTS[name]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# -- 1. indices -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.INDEX_CASES)
def test_indices_equal_the_longdouble_restatement(engine, name):
    c = ref.case(name)
    got = _run(engine, name)
    assert got["idx"].dtype == np.int32 and got["idx"].shape == (c.M,)
    assert np.array_equal(got["idx"], c.ld["idx"]), (name, np.flatnonzero(got["idx"] != c.ld["idx"])[:5])
    assert len(set(got["idx"].tolist())) == c.M and got["idx"][0] == 0


def test_duplicated_rows(engine):
    c = ref.case("dups")
    got = _run(engine, "dups")
    alone = ref.select(c.X[:20], 20, c.ls, c.os, c.jitter_rel, ref.LD)
    assert np.array_equal(got["idx"][:20], alone["idx"])
    assert sorted(got["idx"].tolist()) == list(range(40))
    print(f"dups: max |trace[19:]| {np.max(np.abs(got['trace'][19:])):.3e} (bound {c.tol_trace:.3e})")
    assert np.all(np.abs(got["trace"][19:]) <= c.tol_trace)


# -- 2. trace ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.INDEX_CASES)
def test_trace_against_longdouble(engine, name):
    c = ref.case(name)
    got = _run(engine, name)
    err = float(np.max(np.abs(got["trace"] - c.ld["trace"])))
    print(f"{name}: |trace - longdouble| HIP {err:.3e}  numpy {c.e64_trace:.3e}  bound {c.tol_trace:.3e}")
    record(f"select_inducing[{name}]", trace=err, numpy_trace=c.e64_trace, bound=c.tol_trace)
    assert np.all(np.isfinite(got["trace"]))
    assert err <= c.tol_trace


# -- 3. Z and nullability ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.CASE_NAMES)
def test_z_is_the_picked_rows_bit_for_bit(engine, name):
    c = ref.case(name)
    got = _run(engine, name)
    assert got["Z"].shape == (c.M, c.E)
    assert _same_bits(got["Z"], c.X[got["idx"]])
    assert np.all(np.isfinite(got["Z"])) and np.all(np.isfinite(got["trace"]))


@pytest.mark.parametrize("name", ["n257_m70", "n65_m3"])
def test_null_outputs_change_no_bit_of_the_others(engine, name):
    c = ref.case(name)
    full = _run(engine, name)
    X, ls, osc = (engine._dev(v) for v in (c.X, c.ls, c.os))
    for with_z, with_trace in ((False, True), (True, False), (False, False)):
        idx = torch.full((c.M,), -7, dtype=torch.int32, device=engine.device)
        Z = torch.full((c.M, c.E), -7.0, dtype=torch.float64, device=engine.device)
        trace = torch.full((c.M,), -7.0, dtype=torch.float64, device=engine.device)
        rc = engine.lib.gpmpc_select_inducing(engine._h, X.data_ptr(), c.N, c.M, ls.data_ptr(), osc.data_ptr(), c.jitter_rel, c.D,
                                              c.E, idx.data_ptr(), Z.data_ptr() if with_z else None,
                                              trace.data_ptr() if with_trace else None, engine._stream())
        assert rc == 0
        assert _same_bits(idx.cpu().numpy(), full["idx"])
        assert _same_bits(Z.cpu().numpy(), full["Z"] if with_z else np.full((c.M, c.E), -7.0))
        assert _same_bits(trace.cpu().numpy(), full["trace"] if with_trace else np.full(c.M, -7.0))


# -- 4. determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n1000_m130", "d16_e20", "floor_0.05"])
def test_two_calls_give_the_same_bits(engine, name):
    c = ref.case(name)
    first = _run(engine, name)
    again = {k: v.cpu().numpy() for k, v in engine.select_inducing(c.X, c.M, c.ls, c.os, c.jitter_rel).items()}
    for k in ("idx", "Z", "trace"):
        assert _same_bits(first[k], again[k]), k


# -- 5. isolation -----------------------------------------------------------------------------------------------------------------
def test_a_selection_leaves_the_cached_model_alone():
    import gp_mpc_amd
    b = sgr.case("n37_m16")
    c = ref.case("n257_m70")
    eng = gp_mpc_amd.HipEngine(0)
    try:
        eng.prepare(b.X, b.Y, b.ls, b.os, b.nz)
        mode = eng.last_prepare_mode
        before = {k: v.cpu().numpy() for k, v in eng.predict(b.Xq).items()}
        iK0, beta0 = (t.cpu().numpy() for t in eng.factors())
        got = eng.select_inducing(c.X, c.M, c.ls, c.os, c.jitter_rel)
        assert np.array_equal(got["idx"].cpu().numpy(), c.ld["idx"])
        assert eng.last_prepare_mode == mode and eng.N == b.N
        after = {k: v.cpu().numpy() for k, v in eng.predict(b.Xq).items()}
        iK1, beta1 = (t.cpu().numpy() for t in eng.factors())
        for k in before:
            assert _same_bits(before[k], after[k]), k
        assert _same_bits(iK0, iK1) and _same_bits(beta0, beta1)
    finally:
        eng.close()


def test_no_cached_model_is_needed():
    import gp_mpc_amd
    c = ref.case("n65_m3")
    eng = gp_mpc_amd.HipEngine(0)
    try:
        got = eng.select_inducing(c.X, c.M, c.ls, c.os, c.jitter_rel)
        assert np.array_equal(got["idx"].cpu().numpy(), c.ld["idx"])
    finally:
        eng.close()


# -- 6. errors --------------------------------------------------------------------------------------------------------------------
def test_errors_come_before_any_launch_and_leave_the_outputs_untouched():
    import gp_mpc_amd
    from gp_mpc_amd import _lib
    c = ref.case("n37_m16")
    big = ref.case("n1000_m130")
    eng = gp_mpc_amd.HipEngine(0)
    try:
        for kw in (dict(M=c.N + 1), dict(M=0), dict(jitter_rel=-1.0), dict(jitter_rel=float("nan"))):
            args = dict(M=c.M, jitter_rel=c.jitter_rel)
            args.update(kw)
            with pytest.raises(gp_mpc_amd.GpmpcError) as ei:
                eng.select_inducing(c.X, args["M"], c.ls, c.os, args["jitter_rel"])
            assert ei.value.code == _lib.GPMPC_ERR_ARG, kw
        with pytest.raises(ValueError):
            eng.select_inducing(c.X, c.M, c.ls[:, :3], c.os)
        with pytest.raises(ValueError):
            eng.select_inducing(c.X, c.M, c.ls, c.os[:2])

        X, ls, osc = (eng._dev(v) for v in (c.X, c.ls, c.os))
        Mbuf = c.N + 1
        idx = torch.full((Mbuf,), -7, dtype=torch.int32, device=eng.device)
        Z = torch.full((Mbuf, c.E), -7.0, dtype=torch.float64, device=eng.device)
        trace = torch.full((Mbuf,), -7.0, dtype=torch.float64, device=eng.device)

        def call(X=X.data_ptr(), N=c.N, M=c.M, ls=ls.data_ptr(), osc=osc.data_ptr(), jit=1e-6, D=c.D, E=c.E, idx=idx.data_ptr()):
            return eng.lib.gpmpc_select_inducing(eng._h, X, N, M, ls, osc, jit, D, E, idx, Z.data_ptr(), trace.data_ptr(),
                                                 eng._stream())

        def untouched():
            torch.cuda.synchronize()
            return bool((idx == -7).all()) and bool((Z == -7.0).all()) and bool((trace == -7.0).all())

        bad = [dict(X=None), dict(ls=None), dict(osc=None), dict(N=0), dict(M=0), dict(M=-1), dict(M=c.N + 1), dict(jit=-1.0),
               dict(jit=float("nan")), dict(jit=float("inf"))]
        for kw in bad:
            assert call(**kw) == _lib.GPMPC_ERR_ARG, kw
            assert untouched(), kw
        assert call(idx=None) == _lib.GPMPC_ERR_ARG and untouched()
        assert call(D=17, E=20) == _lib.GPMPC_ERR_LIMIT and call(E=25) == _lib.GPMPC_ERR_LIMIT and untouched()

        # the workspace cap: 3 x 130 x 1000 doubles of partial factors are 3 MiB
        eng.set_option("select_inducing_max_mb", 1)
        with pytest.raises(gp_mpc_amd.GpmpcError) as ei:
            eng.select_inducing(big.X, big.M, big.ls, big.os, big.jitter_rel)
        assert ei.value.code == _lib.GPMPC_ERR_LIMIT and "MiB" in str(ei.value)
        assert call() == _lib.GPMPC_OK                                # 37 / 16 fits 1 MiB ...
        torch.cuda.synchronize()
        assert np.array_equal(idx[:c.M].cpu().numpy(), c.ld["idx"]) and bool((idx[c.M:] == -7).all())
        eng.set_option("select_inducing_max_mb", 4096)                # ... and the default cap holds the larger case
        got = eng.select_inducing(big.X, big.M, big.ls, big.os, big.jitter_rel)
        assert np.array_equal(got["idx"].cpu().numpy(), big.ld["idx"])
        with pytest.raises(gp_mpc_amd.GpmpcError):
            eng.set_option("select_inducing_max_mb", 0)
    finally:
        eng.close()


# -- 7. model level ---------------------------------------------------------------------------------------------------------------
def test_model_level_greedy_beats_strided_on_a_clustered_memory():
    import gp_mpc_amd
    from gp_mpc_amd import GpStateTransitionModel
    from gp_mpc_amd.config_classes.model_config import ModelConfig
    c = ref.case("clustered_n600_m40")
    gp_init = {"noise_covar.noise": list(c.nz), "base_kernel.lengthscale": c.ls.tolist(), "outputscale": list(c.os)}
    exact = ref.exact_mean(c.X, c.Y, c.ls, c.os, c.nz, c.Xq)
    rms = {}
    for rule in ("greedy", "strided"):
        eng = gp_mpc_amd.HipEngine(0)
        try:
            model = GpStateTransitionModel(ModelConfig(gp_init=gp_init, num_inducing_points=c.M, inducing_selection=rule),
                                           dim_state=3, dim_action=1, engine=eng)
            model.prepare_inference(torch.as_tensor(c.X), torch.as_tensor(c.Y))
            assert eng.last_prepare_mode == 4 and eng.N == c.M and model.is_sparse
            if rule == "greedy":
                assert isinstance(model.inducing_idx, torch.Tensor)
                assert np.array_equal(model.inducing_idx.cpu().numpy(), c.ld["idx"])
            else:
                assert model.inducing_idx == sgr.strided_rows(c.N, c.M).tolist()
            mean = eng.predict(c.Xq)["mean"].cpu().numpy()
            rms[rule] = float(np.sqrt(np.mean((mean - exact) ** 2)))
        finally:
            eng.close()
    print(f"clustered_n600_m40: rms error of the sparse mean against the exact GP: greedy {rms['greedy']:.4f}, strided {rms['strided']:.4f}")
    record("select_inducing[model_clustered]", rms_greedy=rms["greedy"], rms_strided=rms["strided"])
    assert rms["greedy"] < rms["strided"]
