"""Tier 2 (GPU): gpmpc_ilqr_backward / _forward / _init / _step / _search -- the device-resident clamped iLQR on the mean dynamics of
the linearised propagation -- and candidate_optimizer = "ilqr_device" behind the controller.

Checked against the long-double restatement of tests/ilqr_ref.py (itself tied to independent derivations by
tests/test_ilqr_reference.py) under the accuracy rule of DESIGN.md 4.7 / 4.11.2, against gpmpc_rollout_linear and gpmpc_lqr_gains
where the entries must agree bit for bit, and against the contracts of include/gpmpc.h: the alpha = 0 forward pass, bitwise
invariance to the batch, the place and the chunks, the accept rule recomputed from the device's own numbers, search = init + steps,
the box, the degenerate cost, errors that write nothing.  The memory is the action-driven one of tests/ilqr_cases.py; L = 4.
"""
import numpy as np
import pytest
import torch

import ilqr_cases as cases
import ilqr_ref as ref
from helpers import record, make_controller
from test_gpu_lqr_gains import CASES

pytestmark = pytest.mark.gpu

L = 4
ALPHAS = [1.0, 0.5, 0.25, 0.125]
REG0, FACTOR, REG_MAX, TOL = 1e-3, 10.0, 1e6, 1e-9


@pytest.fixture(scope="module")
def engine():
    import gp_mpc_amd
    eng = gp_mpc_amd.HipEngine(0)
    yield eng
    eng.close()


def _np(t):
    return t.cpu().numpy()


def _prepared(engine, w, W=None, W_T=None, target=None):
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    engine.set_cost(w.target if target is None else target, w.W if W is None else W, w.W_T if W_T is None else W_T, w.kappa)
    iK, beta = (_np(t) for t in engine.factors())
    return (w.X, w.lengthscales, w.outputscales, iK, beta)


def _state_np(st):
    return {k: _np(v).copy() for k, v in st.items() if isinstance(v, torch.Tensor) and k != "buffer"}


# -- 1. the long-double restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_backward_and_forward_against_extended_precision(engine, case):
    D, A, N, H, B, time = CASES[case]
    w = cases.make_workload(N, D, A, H, B, include_time=time, seed=700 + N + H + D)
    W, W_T = cases.weights(D, A, 701)
    fa = _prepared(engine, w, W, W_T)
    out = engine.ilqr_backward(w.actions, w.mu0, REG0, w.include_time, w.time0)
    fwd = engine.ilqr_forward(w.actions, out["gains"], out["ff"], out["mu"], w.mu0, ALPHAS, w.include_time, w.time0)
    assert out["gains"].shape == (B, H, A, D) and out["ff"].shape == (B, H, A) and out["mu"].shape == (B, H + 1, D)
    assert fwd["trial_actions"].shape == (B, L, H, A) and fwd["trial_cost"].shape == (B, L)
    assert fwd["trial_mu"].shape == (B, L, H + 1, D)
    assert not _np(out["flags"]).any() and not _np(out["info"][:, 4]).any()
    sel = np.unique(np.array([0, B // 2, B - 1]))
    got = {k: _np(out[k])[sel] for k in ("gains", "ff", "cost", "dV", "step")}
    got.update({k: _np(fwd[k])[sel] for k in ("trial_actions", "trial_mu", "trial_cost")})

    def restate(dtype):
        r = ref.backward(fa, w.actions[sel], w.mu0, w.target, W, W_T, w.include_time, w.time0, REG0, dtype=dtype)
        f = ref.forward(ref.gp_mean(fa, w.include_time, w.time0, dtype), w.actions[sel], r["gains"], r["ff"], r["mu"], w.mu0, ALPHAS,
                        dtype=dtype)
        n = len(sel)
        f["trial_cost"] = ref.cost(f["trial_mu"].reshape(n * L, H + 1, D), f["trial_actions"].reshape(n * L, H, A), w.target, W, W_T,
                                   dtype).reshape(n, L)
        r.update(f)
        return r
    r64, rld = restate(np.float64), restate(np.longdouble)
    assert not rld["flags"].any()
    rec = {}
    for k in got:
        e_hip = float(np.max(np.abs(got[k] - rld[k])))
        e_np = float(np.max(np.abs(r64[k] - rld[k])))
        scale = float(np.max(np.abs(rld[k])))
        rec.update({f"{k}_hip": e_hip, f"{k}_numpy": e_np, f"{k}_scale": scale})
    record(f"ilqr_extended[{case}]", **rec)
    print(case, rec)
    for k in got:
        # the rule of DESIGN.md 4.7 / 4.11.2: the HIP evaluation rounds like a plain fp64 evaluation of the same recurrence
        assert rec[f"{k}_hip"] <= 3 * max(rec[f"{k}_numpy"], 1e-12 * rec[f"{k}_scale"]), (k, rec)
    assert rec["ff_scale"] > 1e-3                                          # (a feed-forward of a size that a zero output would miss)
    assert bool((out["dV"] < 0).all())


# -- 2. bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,A,time", [(3, 1, True), (4, 2, False)])
def test_backward_agrees_with_rollout_linear_and_lqr_gains(engine, D, A, time):
    w = cases.make_workload(50, D, A, 3, 5, include_time=time, seed=710 + D)
    W, W_T = cases.weights(D, A, 711)
    _prepared(engine, w, W, W_T)
    reg = np.array([0.0, 1e-3, 1e-2, 1e-3, 0.5])
    out = engine.ilqr_backward(w.actions, w.mu0, reg, w.include_time, w.time0)
    assert torch.equal(out["mu"], engine.rollout_linear(w.actions, w.mu0, w.S0, w.include_time, w.time0)["mu"])
    for i, r in enumerate(reg):
        g = engine.lqr_gains(w.actions[i:i + 1], w.mu0, w.include_time, w.time0, float(r))["gains"]
        assert torch.equal(out["gains"][i], g[0]), i


def test_forward_at_alpha_zero_returns_the_nominal(engine):
    w = cases.make_workload(50, 4, 2, 3, 5, seed=720)
    W, W_T = cases.weights(4, 2, 721)
    _prepared(engine, w, W, W_T)
    out = engine.ilqr_backward(w.actions, w.mu0, REG0)
    gains = torch.as_tensor(np.random.default_rng(722).standard_normal((5, 3, 2, 4)) * 7.0)        # whatever the gains are
    ff = torch.as_tensor(np.random.default_rng(723).standard_normal((5, 3, 2)))
    fwd = engine.ilqr_forward(w.actions, gains, ff, out["mu"], w.mu0, [0.0, 1.0, 0.0])
    acts = engine._dev(w.actions)
    for l in (0, 2):
        assert torch.equal(fwd["trial_actions"][:, l], acts)
        assert torch.equal(fwd["trial_mu"][:, l], out["mu"])
        assert torch.equal(fwd["trial_cost"][:, l], out["cost"])
    assert not torch.equal(fwd["trial_actions"][:, 1], acts)
    # the trajectories are optional and do not change the other outputs' bits
    lean = engine.ilqr_forward(w.actions, gains, ff, out["mu"], w.mu0, [0.0, 1.0, 0.0], trajectories=False)
    assert "trial_mu" not in lean
    assert torch.equal(lean["trial_actions"], fwd["trial_actions"]) and torch.equal(lean["trial_cost"], fwd["trial_cost"])


def _run_steps(engine, w, x0, steps):
    st = engine.ilqr_state(x0.shape[0], x0.shape[1], x0.shape[2], L)
    engine.ilqr_init(st, x0, REG0)
    for _ in range(steps):
        engine.ilqr_step(st, w.mu0, REG0, FACTOR, REG_MAX, TOL, w.include_time, w.time0)
    return _state_np(st)


@pytest.mark.parametrize("N,time", [(50, True), (300, False)])
def test_batch_place_and_chunk_invariance(engine, N, time):
    B, H = 70, 3
    w = cases.make_workload(N, 3, 1, H, B, include_time=time, seed=730 + N)
    W, W_T = cases.weights(3, 1, 731)
    _prepared(engine, w, W, W_T)
    reg = np.linspace(1e-3, 1e-2, B)

    def everything(actions, regs):
        out = engine.ilqr_backward(actions, w.mu0, regs, w.include_time, w.time0)
        fwd = engine.ilqr_forward(actions, out["gains"], out["ff"], out["mu"], w.mu0, ALPHAS, w.include_time, w.time0)
        res = {k: out[k].clone() for k in ("gains", "ff", "mu", "info")}
        res.update({k: v.clone() for k, v in fwd.items()})
        return res
    full = everything(w.actions, reg)
    steps = _run_steps(engine, w, w.actions, 2)
    for i in (0, 63, 64, 69):                                              # alone = at its place of the batch
        one = everything(w.actions[i:i + 1], reg[i:i + 1])
        for k in full:
            assert torch.equal(one[k][0], full[k][i]), (k, i)
    alone = _run_steps(engine, w, w.actions[64:65], 2)
    for k in alone:
        assert np.array_equal(alone[k][0], steps[k][64]), k
    order = np.concatenate([[69], np.arange(1, 69), [0]])
    sw = everything(w.actions[order], reg[order])
    for k in full:
        assert torch.equal(sw[k][0], full[k][69]) and torch.equal(sw[k][69], full[k][0]), k
    for name, chunk in (("ilqr_chunk_points", 1), ("ilqr_chunk_points", 3), ("moments_linear_chunk_points", 7)):
        engine.set_option(name, chunk)
        try:
            chunked = everything(w.actions, reg)
            chunked_steps = _run_steps(engine, w, w.actions, 2)
        finally:
            engine.set_option(name, 0)
        for k in full:
            assert torch.equal(chunked[k], full[k]), (k, name, chunk)
        for k in steps:
            assert np.array_equal(chunked_steps[k], steps[k], equal_nan=True), (k, name, chunk)


# -- 3. the accept rule -------------------------------------------------------------------------------------------------------------
STEP_SEED = 740      # chosen on the CPU: the long-double restatement's two best trial costs differ by > 1e-9 for >= B - 1 candidates


def test_step_follows_the_rule_on_the_devices_own_numbers(engine):
    D, A, H, B = 4, 2, 3, 6
    w = cases.make_workload(50, D, A, H, B, seed=STEP_SEED)
    W, W_T = cases.weights(D, A, STEP_SEED + 1)
    fa = _prepared(engine, w, W, W_T)
    st = engine.ilqr_state(B, H, A, L)
    engine.ilqr_init(st, w.actions, REG0)
    s0 = _state_np(st)
    assert np.array_equal(s0["actions"], w.actions) and np.array_equal(s0["reg"], np.full(B, REG0))
    assert np.array_equal(s0["chosen"], np.full(B, -1.0))
    for k in s0:
        if k not in ("actions", "reg", "chosen"):
            assert not s0[k].any(), k
    # iteration 0 against the long-double restatement
    ld = ref.init(w.actions, L, REG0, np.longdouble)
    mean, linearise = ref.gp_problem(fa, w.mu0, dtype=np.longdouble)
    ref.step(ld, mean, linearise, w.mu0, w.target, W, W_T, REG0, FACTOR, REG_MAX, TOL, dtype=np.longdouble)
    tc = np.sort(ld["trial_cost"].astype(np.longdouble), axis=1)
    clear = np.asarray((tc[:, 1] - tc[:, 0]) > 1e-9 * np.abs(tc[:, 0]))
    assert clear.sum() >= B - 1
    before = s0
    for it in range(4):
        engine.ilqr_step(st, w.mu0, REG0, FACTOR, REG_MAX, TOL)
        now = _state_np(st)
        # the nominal cost the rule saw (an accept overwrites it in the state): the backward entry's, the same bits in any batch
        nominal = _np(engine.ilqr_backward(before["actions"], w.mu0, before["reg"])["cost"])
        chosen, accepts, reg, status, cost = ref.accept_rule(nominal, now["trial_cost"], now["step"], before["reg"], before["status"],
                                                             before["accepts"], REG0, FACTOR, REG_MAX, TOL)
        cost = np.where(chosen == -2, before["cost"], cost)
        live = chosen != -2
        assert np.array_equal(now["chosen"][live], chosen[live].astype(np.float64)), it
        assert np.array_equal(now["accepts"], accepts) and np.array_equal(now["reg"], reg) and np.array_equal(now["status"], status)
        assert np.array_equal(now["cost"], cost)
        want = before["actions"].copy()
        for b in range(B):
            if chosen[b] >= 0:
                want[b] = now["trial_actions"][b, chosen[b]]
        assert np.array_equal(now["actions"], want), it
        if it == 0:
            assert np.array_equal(now["chosen"][clear], ld["chosen"][clear].astype(np.float64))
            assert live.all()
        before = now


# -- 4. the search ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("time", [False, True])
def test_search_equals_manual_stepping(engine, time):
    D, A, H, B = 3, 1, 3, 5
    w = cases.make_workload(50, D, A, H, B, include_time=time, seed=750)
    W, W_T = cases.weights(D, A, 751)
    _prepared(engine, w, W, W_T)
    for k in (1, 3):
        st = engine.ilqr_state(B, H, A, L)
        best = engine.ilqr_search(st, w.mu0, w.S0, k, w.actions, REG0, FACTOR, REG_MAX, TOL, w.include_time, w.time0)
        got = _state_np(st)
        manual = _run_steps(engine, w, w.actions, k)
        for name in manual:
            if name != "J":
                assert np.array_equal(got[name], manual[name], equal_nan=True), (name, k)
        J = engine.rollout_linear(got["actions"], w.mu0, w.S0, w.include_time, w.time0, trajectories=False, stage_costs=False)["J"]
        assert np.array_equal(got["J"], _np(J))
        bj, bi = engine.argmin(st["J"])
        rec = _np(best)
        assert rec[0] == bj and rec[1] == bi and np.array_equal(rec[2:], got["actions"][bi].reshape(-1))
    costs = [_run_steps(engine, w, w.actions, k)["cost"] for k in range(1, 6)]
    for a, b in zip(costs, costs[1:]):
        assert np.all(b <= a)
    first = engine.ilqr_backward(w.actions, w.mu0, REG0, w.include_time, w.time0)["cost"]
    assert np.all(costs[0] <= _np(first)) and np.any(costs[-1] < _np(first))


# -- 5. the box and the degenerate cost ----------------------------------------------------------------------------------------------
def test_the_box(engine):
    D, A, H, B = 3, 1, 3, 4
    w = cases.make_workload(50, D, A, H, B, seed=760)
    target = w.target.copy()
    target[D:] = 1.5
    _prepared(engine, w, np.diag([1.0, 0.1, 0.1, 0.5]), w.W_T, target)
    st = engine.ilqr_state(B, H, A, L)
    engine.ilqr_search(st, w.mu0, w.S0, 6, w.actions, REG0, FACTOR, REG_MAX, TOL)
    got = _state_np(st)
    assert np.array_equal(got["actions"], np.ones((B, H, A))) and np.array_equal(got["status"], np.ones(B))
    assert np.array_equal(got["step"], np.zeros(B)) and np.all(got["dV"] < 0)
    assert np.all((got["trial_actions"] >= 0) & (got["trial_actions"] <= 1))


def test_degenerate_cost(engine):
    D, A, H, B = 4, 2, 3, 4
    w = cases.make_workload(50, D, A, H, B, seed=770)
    _prepared(engine, w, np.zeros((6, 6)), np.zeros((4, 4)))
    st = engine.ilqr_state(B, H, A, L)
    engine.ilqr_init(st, w.actions, 0.0)
    engine.ilqr_step(st, w.mu0, 0.0, FACTOR, REG_MAX, TOL)
    got = _state_np(st)
    assert np.array_equal(got["flags"], np.full(B, float(H))) and np.array_equal(got["status"], np.ones(B))
    assert np.array_equal(got["step"], np.zeros(B))
    for k, v in got.items():
        assert not np.isnan(v).any(), k
    assert not got["gains"].any() and not got["ff"].any() and np.array_equal(got["actions"], w.actions)


# -- 6. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing():
    import gp_mpc_amd
    from gp_mpc_amd import _lib as Lb
    eng = gp_mpc_amd.HipEngine(0)
    try:
        D, A, H, B = 3, 1, 3, 4
        w = cases.make_workload(50, D, A, H, B, seed=780)
        acts = eng._dev(w.actions)
        mu0, S0 = np.ascontiguousarray(w.mu0), np.ascontiguousarray(w.S0)
        al = np.array(ALPHAS)
        nan = lambda *sh: torch.full(sh, float("nan"), dtype=torch.float64, device=eng.device)     # noqa: E731
        size = int(eng.lib.gpmpc_ilqr_state_size(B, H, A, D, L))
        assert size == B * (H * A * (2 + D + L) + 9 + L + (H + 1) * D)
        for bad in ((0, H, A, D, L), (4097, H, A, D, L), (B, 0, A, D, L), (B, H, 0, D, L), (B, H, 9, D, L), (B, H, A, 0, L),
                    (B, H, A, 17, L), (B, H, A, D, 0), (B, H, A, D, 17)):
            assert eng.lib.gpmpc_ilqr_state_size(*bad) < 0, bad
        K, ff, mu, info = nan(B, H, A, D), nan(B, H, A), nan(B, H + 1, D), nan(B, 5)
        reg = torch.full((B,), REG0, dtype=torch.float64, device=eng.device)
        ta, tc, tm, state, best = nan(B, L, H, A), nan(B, L), nan(B, L, H + 1, D), nan(size), nan(2 + H * A)
        S = eng._stream

        def backward(B=B, H=H, A=A, time=0, actions=acts.data_ptr(), m0=mu0.ctypes.data, r=reg.data_ptr(), g=K.data_ptr()):
            return eng.lib.gpmpc_ilqr_backward(eng._h, actions, m0, B, H, A, time, 0.0, r, g, ff.data_ptr(), mu.data_ptr(),
                                               info.data_ptr(), S())

        def forward(B=B, H=H, A=A, time=0, L=L, alphas=al.ctypes.data, out=ta.data_ptr()):
            return eng.lib.gpmpc_ilqr_forward(eng._h, acts.data_ptr(), K.data_ptr(), ff.data_ptr(), mu.data_ptr(), mu0.ctypes.data,
                                              B, H, A, time, 0.0, alphas, L, out, tc.data_ptr(), tm.data_ptr(), S())

        def init(B=B, H=H, A=A, L=L, reg0=REG0, x0=acts.data_ptr(), st=state.data_ptr()):
            return eng.lib.gpmpc_ilqr_init(eng._h, x0, B, H, A, L, reg0, st, S())

        def step(B=B, H=H, A=A, time=0, L=L, reg0=REG0, factor=FACTOR, reg_max=REG_MAX, tol=TOL, m0=mu0.ctypes.data,
                 st=state.data_ptr()):
            return eng.lib.gpmpc_ilqr_step(eng._h, m0, B, H, A, time, 0.0, L, reg0, factor, reg_max, tol, st, S())

        def search(B=B, H=H, A=A, time=0, iterations=2, L=L, reg0=REG0, factor=FACTOR, reg_max=REG_MAX, tol=TOL, x0=acts.data_ptr(),
                   st=state.data_ptr(), s0=S0.ctypes.data):
            return eng.lib.gpmpc_ilqr_search(eng._h, mu0.ctypes.data, s0, B, H, A, time, 0.0, iterations, L, reg0, factor, reg_max, tol,
                                             x0, st, best.data_ptr(), S())

        def untouched():
            torch.cuda.synchronize()
            return all(bool(torch.isnan(t).all()) for t in (K, ff, mu, info, ta, tc, tm, state, best))
        entries = (backward, forward, init, step, search)
        for f in entries:
            assert f() == Lb.GPMPC_ERR_ARG and "prepare" in eng.lib.gpmpc_last_error(eng._h).decode()
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        for f in entries:
            assert f() == Lb.GPMPC_ERR_ARG and "set_cost" in eng.lib.gpmpc_last_error(eng._h).decode()      # no cost set
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        for f in entries:
            for kw in (dict(B=0), dict(B=4097), dict(H=0), dict(A=0), dict(A=2)):
                assert f(**kw) == Lb.GPMPC_ERR_ARG, (f.__name__, kw)
        for f in (backward, forward, step, search):
            assert f(time=1) == Lb.GPMPC_ERR_ARG, f.__name__
        for f in (forward, init, step, search):
            for kw in (dict(L=0), dict(L=17)):
                assert f(**kw) == Lb.GPMPC_ERR_ARG, (f.__name__, kw)
        for kw in (dict(actions=None), dict(m0=None), dict(r=None), dict(g=None)):
            assert backward(**kw) == Lb.GPMPC_ERR_ARG, kw
        for kw in (dict(alphas=None), dict(out=None)):
            assert forward(**kw) == Lb.GPMPC_ERR_ARG, kw
        for kw in (dict(x0=None), dict(st=None), dict(reg0=-1e-3), dict(reg0=float("nan")), dict(reg0=float("inf"))):
            assert init(**kw) == Lb.GPMPC_ERR_ARG, kw
        params = (dict(reg0=-1e-3), dict(reg0=float("nan")), dict(reg0=float("inf")), dict(factor=1.0), dict(factor=float("nan")),
                  dict(reg_max=REG0 / 2), dict(reg_max=float("nan")), dict(tol=-1.0), dict(tol=float("nan")), dict(st=None))
        for kw in params + (dict(m0=None),):
            assert step(**kw) == Lb.GPMPC_ERR_ARG, kw
        for kw in params + (dict(x0=None), dict(s0=None), dict(iterations=0)):
            assert search(**kw) == Lb.GPMPC_ERR_ARG, kw
        assert untouched()
        # the compiled limit of the sweep: A <= 8
        w9 = cases.make_workload(50, 1, 9, 3, 4, seed=781)
        eng.prepare(w9.X, w9.Y, w9.lengthscales, w9.outputscales, w9.noises)
        eng.set_cost(w9.target, w9.W, w9.W_T, w9.kappa)
        for f in entries:
            assert f(A=9) == Lb.GPMPC_ERR_LIMIT, f.__name__
        assert untouched()
        for value in (-1, (1 << 24) + 1):
            assert eng.lib.gpmpc_set_option(eng._h, b"ilqr_chunk_points", value) == Lb.GPMPC_ERR_ARG
        # ... and the calls that are in order write everything, and leave the other entries and the gpmpc_last_* state alone
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        before = {k: v.clone() for k, v in eng.rollout_linear(w.actions, w.mu0, w.S0).items()}
        lqr = eng.lqr_gains(w.actions, w.mu0, reg=REG0)["gains"].clone()
        last = (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode, eng.last_grad_path)
        assert backward() == Lb.GPMPC_OK and forward() == Lb.GPMPC_OK and search() == Lb.GPMPC_OK
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(t).all()) for t in (K, ff, mu, info, ta, tc, tm, state, best))
        assert (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode, eng.last_grad_path) == last
        after = eng.rollout_linear(w.actions, w.mu0, w.S0)
        for k in before:
            assert torch.equal(before[k], after[k]), k
        assert torch.equal(eng.lqr_gains(w.actions, w.mu0, reg=REG0)["gains"], lqr)
    finally:
        eng.close()


# -- 7. the controller ----------------------------------------------------------------------------------------------------------------
# The excess of the controller's best_candidate_J over the best J of its own starts (the search minimises the certainty-equivalent
# cost, not J, so a bound of zero is not guaranteed): measured on one MI355X over the seeds below it was -1.56e-2 / -2.81e-3 / -1.95e-2,
# negative for every seed, so the largest excess seen lies below zero and the margin is 0
CONTROLLER_MARGIN = 0.0


@pytest.mark.parametrize("seed", [7, 8, 9])
def test_controller_ilqr_device(engine, seed):
    w = cases.make_workload(50, 3, 1, 3, 1, seed=790, dense_s0=0.0)
    np.random.seed(seed)
    c = make_controller(w, optimize=True, restarts=6, engine=engine, shard=False)
    c.transition_model.config.uncertainty_propagation = "linearized"
    cc = c.config.controller
    cc.candidate_optimizer, cc.init_from_previous_actions, cc.ilqr_iterations, cc.ilqr_line_search_steps = "ilqr_device", False, 5, L
    a = c.get_action(obs_mu=w.mu0)
    assert a.shape == (1,) and np.all(np.isfinite(a)) and 0.0 <= float(a[0]) <= 1.0
    assert c.candidates_final_J.shape == (6,) and c.candidates_final_status.shape == (6,)
    assert np.asarray(c.states_mu_pred).shape == (4, 3) and np.isfinite(float(c.cost_traj_mean_lcb))
    assert c.best_candidate_J == float(np.min(c.candidates_final_J)) and c.num_rollouts >= 6 * 5
    J0 = _np(c.evaluate_candidates(c.ilqr_device_starts, torch.as_tensor(w.mu0), torch.as_tensor(w.S0))["J"])
    excess = c.best_candidate_J - float(J0.min())
    record(f"ilqr_controller[{seed}]", excess=excess, best_J=c.best_candidate_J, best_start_J=float(J0.min()))
    print(seed, "excess of best_candidate_J over the best start's J:", excess)
    assert excess <= CONTROLLER_MARGIN
