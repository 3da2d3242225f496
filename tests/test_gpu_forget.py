"""Tier 2 (GPU, through the C ABI): gpmpc_forget -- memory points leave the cached factors by an O(N^2) downdate -- against
the CPU oracle's factorisation of the reduced memory and against a second engine that factorises in full ("incremental" = 0).

Tolerances: 1e-8 on iK / beta (rel_err, the border-update tolerance of test_incremental_prepare_matches_full_factorisation, whose
workloads and seeds these tests use); rollouts 1e-9 / 1e-6 / 1e-8 on mu / Sig / J as there; predict and moments at the tolerances
of test_gpu_predict.py (1e-10 mean, 1e-7 variance) and test_gpu_moments.py (1e-10 M and V, 1e-6 S).

L^-1 has no accessor: what observes the downdated factor is the border update that works from it, so every removal here is
followed by a gpmpc_prepare with a few appended points (mode 1) and a second check of the factors.  A rollout straight after a
forget observes T, X^T and the data range as the forget's own launches wrote them.

Lost positive definiteness: no test.  A removal keeps a positive-definite K positive definite (a principal submatrix), the
downdate divides by iK[j, j] and L^-1[j, j] -- both positive for every state gpmpc_prepare accepts -- and otherwise adds positive
terms, so no memory that passes gpmpc_prepare makes gpmpc_forget report GPMPC_ERR_NOT_PD; the report (info = j + 1 for a
non-positive or non-finite pivot quantity) could only be reached by corrupting the cached factors, which no entry point allows.
"""
import numpy as np
import pytest

from helpers import rel_err, record
from oracle import gpmpc_oracle as orc
from oracle import synth

pytestmark = pytest.mark.gpu

CASES = [(40, 3, 1, False), (200, 3, 1, False), (130, 4, 2, True), (300, 3, 1, False)]


def _engines():
    import gp_mpc_amd
    inc, full = gp_mpc_amd.HipEngine(0), gp_mpc_amd.HipEngine(0)
    full.set_option("incremental", 0)
    return inc, full


def _hyp(w):
    return w.lengthscales, w.outputscales, w.noises


def _check_factors(eng, full, X, Y, w, tag):
    iK, beta = (t.cpu().numpy() for t in eng.factors())
    iKo, betao = orc.factorize(X, Y, *_hyp(w))
    full.prepare(X, Y, *_hyp(w))
    assert full.last_prepare_mode == 0
    iKf, betaf = (t.cpu().numpy() for t in full.factors())
    errs = dict(iK_vs_oracle=rel_err(iK, iKo), beta_vs_oracle=rel_err(beta, betao), iK_vs_full=rel_err(iK, iKf),
                beta_vs_full=rel_err(beta, betaf))
    record(tag, **errs)
    print(tag, errs)
    assert iK.shape == iKo.shape and beta.shape == betao.shape
    assert all(e < 1e-8 for e in errs.values()), errs
    assert np.array_equal(iK, iK.transpose(0, 2, 1))


def _check_rollout(eng, full, w, tag):
    """Both engines hold the same memory (full: by a factorisation): their rollouts agree as in the border-update test."""
    for e in (eng, full):
        e.set_cost(w.target, w.W, w.W_T, w.kappa)
    a = eng.rollout(w.actions, w.mu0, w.S0, w.include_time, w.time0)
    b = full.rollout(w.actions, w.mu0, w.S0, w.include_time, w.time0)
    errs = {k: rel_err(a[k].cpu().numpy(), b[k].cpu().numpy()) for k in ("mu", "Sig", "J")}
    record(tag, **{"rollout_" + k: v for k, v in errs.items()})
    print(tag, "rollout", errs)
    assert errs["mu"] < 1e-9 and errs["Sig"] < 1e-6 and errs["J"] < 1e-8, errs


@pytest.mark.parametrize("which", ["first", "last", "middle", "scattered5"])
@pytest.mark.parametrize("N,D,A,tm", CASES)
def test_forget_matches_factorisation_of_the_reduced_memory(N, D, A, tm, which):
    w = synth.make_workload(N + 3, D, A, 4, 4, include_time=tm, seed=N)
    idx = {"first": [0], "last": [N - 1], "middle": [N // 2],
           "scattered5": sorted({1, N // 5, N // 2 - 3, (3 * N) // 4, N - 2})}[which]
    assert which != "scattered5" or len(idx) == 5
    keep = np.setdiff1d(np.arange(N), idx)
    tag = f"forget[{N}-{D}-{A}-{int(tm)}-{which}]"
    inc, full = _engines()
    try:
        inc.prepare(w.X[:N], w.Y[:N], *_hyp(w))
        assert inc.last_prepare_mode == 0
        inc.forget(idx)
        assert inc.last_prepare_mode == 3 and inc.N == N - len(idx)
        _check_factors(inc, full, w.X[keep], w.Y[keep], w, tag)
        _check_rollout(inc, full, w, tag)                       # the tables as the forget left them, no prepare in between
        # the border update works from the downdated L^-1: three appended points, then the same checks
        grown = np.r_[keep, N:N + 3]
        inc.prepare(w.X[grown], w.Y[grown], *_hyp(w))
        assert inc.last_prepare_mode == 1
        _check_factors(inc, full, w.X[grown], w.Y[grown], w, tag + "+3")
        _check_rollout(inc, full, w, tag + "+3")
    finally:
        inc.close()
        full.close()


def test_sliding_window_of_forget_and_border_updates():
    """N = 200, 60 steps of forget-oldest then prepare-with-one-appended, nothing refactorised in between: the modes alternate
    3, 1 and the model that comes out is the one a full factorisation of the final window gives -- factors, rollouts, predict
    and moments."""
    N, steps = 200, 60
    w = synth.make_workload(N + steps, 3, 1, 4, 4, include_time=False, seed=N)
    inc, full = _engines()
    inc.set_option("refresh_every", 10 ** 6)
    try:
        inc.prepare(w.X[:N], w.Y[:N], *_hyp(w))
        modes = []
        for s in range(steps):
            inc.forget([0])
            modes.append(inc.last_prepare_mode)
            inc.prepare(w.X[s + 1:N + s + 1], w.Y[s + 1:N + s + 1], *_hyp(w))
            modes.append(inc.last_prepare_mode)
        assert modes == [3, 1] * steps
        X, Y = w.X[steps:N + steps], w.Y[steps:N + steps]
        _check_factors(inc, full, X, Y, w, "forget_sliding_window")
        for e in (inc, full):
            e.set_cost(w.target, w.W, w.W_T, w.kappa)
        a = inc.rollout(w.actions, w.mu0, w.S0, w.include_time, w.time0)
        b = full.rollout(w.actions, w.mu0, w.S0, w.include_time, w.time0)
        errs = {k: rel_err(a[k].cpu().numpy(), b[k].cpu().numpy()) for k in ("mu", "Sig", "J")}
        print("forget_sliding_window rollout", errs)
        assert errs["mu"] < 1e-9 and errs["Sig"] < 1e-6 and errs["J"] < 1e-8, errs
        rng = np.random.default_rng(7)
        Xq = X[rng.integers(0, N, 50)] + 0.05 * rng.standard_normal((50, X.shape[1]))
        pa, pb = inc.predict(Xq, noises=w.noises), full.predict(Xq, noises=w.noises)
        e_mean = rel_err(pa["mean"].cpu().numpy(), pb["mean"].cpu().numpy())
        e_var = rel_err(pa["var"].cpu().numpy(), pb["var"].cpu().numpy())
        E = X.shape[1]
        Sq = np.stack([(lambda m: 1e-3 * (m @ m.T + np.eye(E)))(rng.standard_normal((E, E))) for _ in range(8)])
        ma, mb = inc.moments(Xq[:8], Sq), full.moments(Xq[:8], Sq)
        e_M, e_S, e_V = (rel_err(ma[k].cpu().numpy(), mb[k].cpu().numpy()) for k in ("M", "S", "V"))
        record("forget_sliding_window", rollout_mu=errs["mu"], rollout_Sig=errs["Sig"], rollout_J=errs["J"], predict_mean=e_mean,
               predict_var=e_var, moments_M=e_M, moments_S=e_S, moments_V=e_V)
        print("forget_sliding_window predict", e_mean, e_var, "moments", e_M, e_S, e_V)
        assert e_mean < 1e-10 and e_var < 1e-7
        assert e_M <= 1e-10 and e_S <= 1e-6 and e_V <= 1e-10
    finally:
        inc.close()
        full.close()


def test_forget_composes_with_the_reuse_rules_of_prepare():
    import gp_mpc_amd
    w = synth.make_workload(90, 3, 1, 3, 2, seed=5)
    e = gp_mpc_amd.HipEngine(0)
    try:
        keep = np.setdiff1d(np.arange(60), [4, 30])
        e.prepare(w.X[:60], w.Y[:60], *_hyp(w)); assert e.last_prepare_mode == 0
        e.forget([4, 30]); assert e.last_prepare_mode == 3
        e.prepare(w.X[keep], w.Y[keep], *_hyp(w)); assert e.last_prepare_mode == 2          # identical: cache hit
        X1, Y1 = np.vstack([w.X[keep], w.X[60:63]]), np.vstack([w.Y[keep], w.Y[60:63]])
        e.prepare(X1, Y1, *_hyp(w)); assert e.last_prepare_mode == 1                        # + 3 points: border update
        iK, beta = e.factors()                                                              # ... from the downdated L^-1
        iKo, betao = orc.factorize(X1, Y1, *_hyp(w))
        assert rel_err(iK.cpu().numpy(), iKo) < 1e-8 and rel_err(beta.cpu().numpy(), betao) < 1e-8
        e.forget([0]); assert e.last_prepare_mode == 3
        X2, Y2 = np.vstack([X1[1:], w.X[63:72]]), np.vstack([Y1[1:], w.Y[63:72]])
        e.prepare(X2, Y2, *_hyp(w)); assert e.last_prepare_mode == 0                        # + 9 points: full
        # removals count toward the refresh interval together with appended points
        e.set_option("refresh_every", 2)
        modes, X, Y, nxt = [], X2, Y2, 72
        for _ in range(3):
            e.forget([0]); modes.append(e.last_prepare_mode)
            X, Y = np.vstack([X[1:], w.X[nxt:nxt + 1]]), np.vstack([Y[1:], w.Y[nxt:nxt + 1]])
            nxt += 1
            e.prepare(X, Y, *_hyp(w)); modes.append(e.last_prepare_mode)
        assert modes == [3, 1, 0, 1, 3, 0]
        iK, beta = e.factors()
        iKo, betao = orc.factorize(X, Y, *_hyp(w))
        assert rel_err(iK.cpu().numpy(), iKo) < 1e-8 and rel_err(beta.cpu().numpy(), betao) < 1e-8
        # a removal of two with one update left in the interval: full, from the record
        e.set_option("refresh_every", 3)
        e.prepare(X, Y, w.lengthscales, w.outputscales, w.noises * 2); assert e.last_prepare_mode == 0
        e.forget([1]); assert e.last_prepare_mode == 3
        e.forget([1]); assert e.last_prepare_mode == 3
        e.forget([1, 2]); assert e.last_prepare_mode == 0
        X, Y = np.delete(X, [1, 2, 3, 4], 0), np.delete(Y, [1, 2, 3, 4], 0)
        iK, beta = e.factors()
        iKo, betao = orc.factorize(X, Y, w.lengthscales, w.outputscales, w.noises * 2)
        assert e.N == len(X) and rel_err(iK.cpu().numpy(), iKo) < 1e-8 and rel_err(beta.cpu().numpy(), betao) < 1e-8
        e.prepare(X, Y, w.lengthscales, w.outputscales, w.noises * 2); assert e.last_prepare_mode == 2
    finally:
        e.close()


def test_forget_without_incremental_factorises_the_reduced_memory():
    import gp_mpc_amd
    w = synth.make_workload(130, 4, 2, 4, 4, include_time=True, seed=130)
    e = gp_mpc_amd.HipEngine(0)
    e.set_option("incremental", 0)
    try:
        e.prepare(w.X, w.Y, *_hyp(w))
        idx = [0, 17, 64, 65, 129]
        e.forget(idx)
        assert e.last_prepare_mode == 0 and e.N == 125
        keep = np.setdiff1d(np.arange(130), idx)
        iK, beta = e.factors()
        iKo, betao = orc.factorize(w.X[keep], w.Y[keep], *_hyp(w))
        assert rel_err(iK.cpu().numpy(), iKo) < 1e-8 and rel_err(beta.cpu().numpy(), betao) < 1e-8
    finally:
        e.close()


def test_forget_of_more_than_eight_rows():
    """More removed rows than ride in the kernel argument block (they come from device memory then)."""
    N = 130
    w = synth.make_workload(N + 2, 4, 2, 4, 4, include_time=True, seed=N)
    idx = list(range(3, N - 5, 9))
    assert len(idx) > 8
    keep = np.setdiff1d(np.arange(N), idx)
    inc, full = _engines()
    try:
        inc.prepare(w.X[:N], w.Y[:N], *_hyp(w))
        inc.forget(idx)
        assert inc.last_prepare_mode == 3
        _check_factors(inc, full, w.X[keep], w.Y[keep], w, "forget_14_rows")
        _check_rollout(inc, full, w, "forget_14_rows")
        inc.prepare(w.X[keep], w.Y[keep], *_hyp(w))
        assert inc.last_prepare_mode == 2
        grown = np.r_[keep, N:N + 2]
        inc.prepare(w.X[grown], w.Y[grown], *_hyp(w))
        assert inc.last_prepare_mode == 1
        _check_factors(inc, full, w.X[grown], w.Y[grown], w, "forget_14_rows+2")
    finally:
        inc.close()
        full.close()


def test_forget_rejects_bad_arguments_and_leaves_the_model_untouched():
    import gp_mpc_amd
    from gp_mpc_amd import _lib
    w = synth.make_workload(40, 3, 1, 4, 4, seed=40)
    e = gp_mpc_amd.HipEngine(0)
    try:
        with pytest.raises(gp_mpc_amd.GpmpcError) as ei:                  # no model yet
            e.forget([0])
        assert ei.value.code == _lib.GPMPC_ERR_ARG
        e.prepare(w.X, w.Y, *_hyp(w))
        iK0, beta0 = (t.cpu().numpy() for t in e.factors())
        bad = [[], [5, 3], [3, 3], [-1], [40], [0, 40], [7, 2 ** 31 + 7], list(range(40))]
        for idx in bad:
            with pytest.raises(gp_mpc_amd.GpmpcError) as ei:
                e.forget(np.asarray(idx, dtype=np.int64))
            assert ei.value.code == _lib.GPMPC_ERR_ARG, idx
            iK, beta = (t.cpu().numpy() for t in e.factors())
            assert e.N == 40 and np.array_equal(iK, iK0) and np.array_equal(beta, beta0), idx
        e.prepare(w.X, w.Y, *_hyp(w))
        assert e.last_prepare_mode == 2                                   # ... and the record is intact
        # set_factors drops the record of the prepare: nothing to downdate from
        e.set_factors(w.X, iK0, beta0, w.lengthscales, w.outputscales)
        with pytest.raises(gp_mpc_amd.GpmpcError) as ei:
            e.forget([0])
        assert ei.value.code == _lib.GPMPC_ERR_ARG
        iK, beta = (t.cpu().numpy() for t in e.factors())
        assert np.array_equal(iK, iK0) and np.array_equal(beta, beta0)
    finally:
        e.close()


def test_forget_after_mll_downdates_the_model_mll_left():
    """gpmpc_mll factorises through gpmpc_prepare's path and leaves its record (a prepare of the same inputs after it is a cache
    hit): rows can be forgotten from its model like from a prepare's, and the border update after it works."""
    N = 40
    w = synth.make_workload(N + 2, 3, 1, 4, 4, seed=N)
    inc, full = _engines()
    try:
        inc.mll(w.X[:N], w.Y[:N], *_hyp(w))
        inc.forget([5, 20])
        assert inc.last_prepare_mode == 3 and inc.N == N - 2
        keep = np.setdiff1d(np.arange(N), [5, 20])
        _check_factors(inc, full, w.X[keep], w.Y[keep], w, "forget_after_mll")
        grown = np.r_[keep, N:N + 2]
        inc.prepare(w.X[grown], w.Y[grown], *_hyp(w))
        assert inc.last_prepare_mode == 1
        _check_factors(inc, full, w.X[grown], w.Y[grown], w, "forget_after_mll+2")
    finally:
        inc.close()
        full.close()


def test_model_forget_drops_the_rows_from_the_shipped_memory():
    """GpStateTransitionModel.forget: the engine's model and x_mem / y_mem (what save_state ships to training) shrink together,
    and predict runs on the reduced model with no further call."""
    import torch
    import gp_mpc_amd
    from gp_mpc_amd.config_classes import ModelConfig
    from gp_mpc_amd.control_objects.models.gp_model import GpStateTransitionModel
    w = synth.make_workload(40, 3, 1, 4, 4, seed=40)
    cfg = ModelConfig(gp_init={"noise_covar.noise": list(w.noises), "base_kernel.lengthscale": w.lengthscales.tolist(),
                               "outputscale": list(w.outputscales)}, include_time_model=False)
    eng, ref = _engines()
    try:
        m = GpStateTransitionModel(cfg, 3, 1, engine=eng)
        m.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
        m.forget([0, 1, 20])
        keep = np.setdiff1d(np.arange(40), [0, 1, 20])
        assert eng.last_prepare_mode == 3
        assert np.array_equal(m.x_mem.numpy(), w.X[keep]) and np.array_equal(m.y_mem.numpy(), w.Y[keep])
        st = m.save_state()
        assert np.array_equal(np.asarray(st.inputs), w.X[keep]) and np.array_equal(np.asarray(st.states_change), w.Y[keep])
        ref.prepare(w.X[keep], w.Y[keep], *_hyp(w))
        mean, var = m.predict(torch.as_tensor(w.X[:10]))
        o = ref.predict(w.X[:10], noises=w.noises)
        assert rel_err(mean.cpu().numpy(), o["mean"].cpu().numpy()) < 1e-10
        assert rel_err(var.cpu().numpy(), o["var"].cpu().numpy()) < 1e-7
    finally:
        eng.close()
        ref.close()


def test_capped_controller_run_is_downdate_then_border_update():
    """A controller whose memory is capped (MemoryConfig.max_points_model): at steady state every control step is a forget of
    the oldest point (mode 3) and a border update of the new one (mode 1) -- no factorisation -- and the model it plans with is
    the one a full factorisation of the window gives."""
    import gp_mpc_amd
    from helpers import make_controller
    N, steps = 40, 6
    w = synth.make_workload(N, 3, 1, 4, 4, seed=N)
    eng, full = _engines()
    try:
        c = make_controller(w, engine=eng, shard=False)
        c.memory.config.max_points_model = N
        c.memory.config.check_errors_for_storage = False
        modes = []
        forget, prepare = eng.forget, eng.prepare
        eng.forget = lambda idx: (forget(idx), modes.append(eng.last_prepare_mode))
        eng.prepare = lambda *a: (prepare(*a), modes.append(eng.last_prepare_mode))
        np.random.seed(0)
        rng = np.random.default_rng(1)
        obs = w.mu0.copy()
        for s in range(steps):
            a = c.get_action(obs)
            obs_new = np.clip(obs + 0.05 * rng.standard_normal(obs.shape), 0.0, 1.0)
            c.add_memory(obs, a, obs_new, 0.0)
            obs = obs_new
        assert modes == [0] + [3, 1] * (steps - 1), modes
        x_mem, y_mem = c.memory.get()
        assert len(x_mem) == N and eng.N == N
        _check_factors(eng, full, x_mem.numpy(), y_mem.numpy(), w, "forget_capped_controller")
    finally:
        eng.close()
        full.close()
