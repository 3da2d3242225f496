"""Tier 2 (GPU): the kernels of csrc/lbfgs_search.hip (gpmpc_lbfgs_init / _step / _search) against the numpy restatement of
tests/lbfgs_device_ref.py, and candidate_optimizer = "lbfgs_device" behind the controller.

How the kernels are observed: the state buffer is the caller's, so every field is read back after every step.  A step is
compared with the restatement applied to the DEVICE's own state before the step and the same (J, G): errors do not accumulate,
and a decision can only differ where its operands are within rounding of each other -- which the tests rule out first: every
Armijo, curvature and descent decision of the longdouble restatement must have a relative margin >= 1e-6 (asserted, never
skipped).

Tolerances: copies and decisions (x and g after an accept, J, status, pair count, alpha) are compared bit for bit with the float64
restatement.  Computed values (d, xt, actions, the stored pairs and their s.y, y.y) by the rule of test_gpu_cem_search.py,
    tolerance = 10 e64 + 64 eps scale            (e64: the float64 restatement's own error against the longdouble one on that case,
                                                  computed here, never taken from the GPU; eps = 2^-52)
with scale = 1 for quantities of the box (xt, s, actions) and the largest magnitude of the operands otherwise (d: the gradient
and the held pairs; y: the two gradients; s.y: s and y; y.y: y).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import lbfgs_device_ref as ref
from helpers import load, make_controller, record, workload_of
from oracle import synth

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
LD = np.longdouble
C1, PGTOL = 1e-4, 1e-5
FIELDS = ("x", "g", "d", "xt", "actions", "J", "alpha", "status", "pushes", "S", "Y", "sy", "yy")
MIN_MARGIN = 1e-6


def tol(e64, scale=1.0):
    return 10.0 * float(e64) + 64.0 * EPS * float(scale)


def err(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    if not a.size:
        return 0.0
    same = (a == b) | (np.isnan(a) & np.isnan(b))                # equal infinities / NaNs are no error
    with np.errstate(invalid="ignore"):
        return float(np.max(np.where(same, LD(0.0), np.abs(a - b))))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def engine():
    import gp_mpc_amd
    eng = gp_mpc_amd.HipEngine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def bare_engine():
    """An engine that never prepared a model: gpmpc_lbfgs_init and gpmpc_lbfgs_step need none."""
    import gp_mpc_amd
    eng = gp_mpc_amd.HipEngine(0)
    yield eng
    eng.close()


def host(state):
    flat = state["buffer"].cpu().numpy()
    out, off = {}, 0
    for k in FIELDS:
        cnt = state[k].numel()
        out[k] = flat[off:off + cnt].reshape(tuple(state[k].shape)).copy()
        off += cnt
    return out


def rows(st, sel):
    return {k: v[sel] for k, v in st.items()}


def check_step(name, before, after, J, G, k, H, A, m, kw, worst, pgtol=PGTOL):
    """`after` (device) against the restatement's step k from `before` (device) and (J, G); returns the longdouble infos."""
    mc, ap = kw.get("max_change"), kw.get("action_prev")
    s64, i64 = ref.step(before, J, G, k, H, A, m, C1, pgtol, mc, ap)
    sld, ild = ref.step(before, J, G, k, H, A, m, C1, pgtol, mc, ap, dtype=LD)
    margin = ref.min_margin(ild)
    worst["margin"] = min(worst["margin"], margin)
    assert margin >= MIN_MARGIN, f"{name} step {k}: a decision of the restatement has relative margin {margin:.3e}"
    assert [i["branch"] for i in i64] == [i["branch"] for i in ild]
    for key in ("status", "pushes", "alpha", "J", "x"):
        assert same_bits(after[key], s64[key]), (name, k, key)
    # g is a copy under the identity mapper and two exact-order operations per entry under the derivative mapper: the same bits,
    # except that IEEE 754 leaves the payload of a NaN an operation PRODUCES open (a NaN fed in G at k = 0)
    nan = np.isnan(s64["g"])
    assert np.array_equal(np.isnan(after["g"]), nan) and same_bits(np.where(nan, 0.0, after["g"]), np.where(nan, 0.0, s64["g"])), (name, k)
    if mc is None:
        assert same_bits(after["g"], s64["g"]), (name, k, "g")
    B = before["x"].shape[0]
    for b in range(B):
        if ild[b]["branch"] == "frozen":
            for key in FIELDS:
                assert same_bits(after[key][b], before[key][b]), (name, k, b, key)
            continue
        e = lambda key: err(s64[key][b], sld[key][b])            # noqa: E731
        amax = lambda v: float(np.max(np.abs(np.asarray(v, dtype=np.float64)), initial=0.0))      # noqa: E731
        gmax = amax(np.concatenate([before["g"][b], after["g"][b]])[np.isfinite(np.concatenate([before["g"][b], after["g"][b]]))])
        smax, ymax = amax(sld["S"][b]), amax(sld["Y"][b])
        tols = dict(d=tol(e("d"), max(gmax, smax, ymax)),         # operands: the gradient and the held pairs
                    xt=tol(e("xt")), actions=tol(e("actions")), S=tol(e("S")),
                    Y=tol(e("Y"), gmax), sy=tol(e("sy"), max(smax, ymax)), yy=tol(e("yy"), ymax))
        for key, t in tols.items():
            got = err(after[key][b], sld[key][b])
            if np.isfinite(t) and t > 0.0:
                worst[key] = max(worst.get(key, 0.0), got / t)
            assert got <= t, (name, k, b, key, got, t)
        assert np.all((after["xt"][b] >= 0.0) & (after["xt"][b] <= 1.0))
        assert np.all((after["actions"][b] >= 0.0) & (after["actions"][b] <= 1.0)) or mc is None
    return ild


# -- a. the step kernel alone, on hand-made J and G -------------------------------------------------------------------------------
SHAPES = {1: (1, 1), 63: (21, 3), 64: (32, 2), 65: (13, 5), 200: (50, 4)}


def mapper_kw(A, deriv):
    return dict(max_change=np.linspace(0.3, 0.9, A), action_prev=np.linspace(0.2, 0.8, A)) if deriv else {}


@pytest.mark.parametrize("deriv", [False, True])
@pytest.mark.parametrize("B", [1, 2, 65])
@pytest.mark.parametrize("m", [1, 3, 10])
@pytest.mark.parametrize("n", sorted(SHAPES))
def test_step_kernel_on_hand_made_sequences(bare_engine, n, m, B, deriv):
    eng = bare_engine
    H, A = SHAPES[n]
    kw = mapper_kw(A, deriv)
    Q, c = ref.quadratic(n, 20 + n)
    U = len(ref.SCRIPTS)
    x0u = np.random.default_rng(30 + n).uniform(0.05, 0.95, size=(U, n))
    # B = 1: the sequence with the forced branches; B = 2: it and the overflow / underflow one; B = 65: all of them, in turn
    order = {1: [1], 2: [1, 2]}.get(B, [b % U for b in range(B)])
    scripts = [ref.SCRIPTS[i] for i in order]
    uniq = sorted(set(order), key=order.index)
    first = [order.index(i) for i in uniq]                       # the first restart running each distinct sequence
    name = f"lbfgs_step[n={n},m={m},B={B},deriv={int(deriv)}]"
    st = eng.lbfgs_state(B, n, m)
    st["buffer"].fill_(-7.0)
    eng.lbfgs_init(st, x0u[order], H, A, **kw)
    before = host(st)
    want = ref.init(x0u[order], H, A, m, kw.get("max_change"), kw.get("action_prev"))
    want_ld = ref.init(x0u[order], H, A, m, kw.get("max_change"), kw.get("action_prev"), dtype=LD)
    for key in FIELDS:
        if key != "actions":
            assert same_bits(before[key], want[key]), key
    assert err(before["actions"], want_ld["actions"]) <= tol(err(want["actions"], want_ld["actions"]))
    worst, seen = dict(margin=np.inf), {s: [] for s in ref.SCRIPTS}
    for k in range(ref.SCRIPT_STEPS):
        sub = rows(before, first)
        Ju, Gu = ref.script_batch([scripts[b] for b in first], k, sub, Q, c, H, A, kw.get("max_change"))
        pick = [uniq.index(i) for i in order]
        J, G = Ju[pick], Gu[pick]
        eng.lbfgs_step(st, J, G, H, A, k, C1, PGTOL, **kw)
        after = host(st)
        for b in range(B):                                       # a restart's bits depend neither on B nor on its slot
            f = first[uniq.index(order[b])]
            if b != f:
                for key in FIELDS:
                    assert same_bits(after[key][b], after[key][f]), (k, b, key)
        infos = check_step(name, sub, rows(after, first), Ju, Gu, k, H, A, m, kw, worst)
        for i, info in zip(uniq, infos):
            seen[ref.SCRIPTS[i]].append(info)
        before = after
    record(name, **{k: v for k, v in worst.items() if np.isfinite(v)})
    # every branch was taken on the device's own trajectory
    ev = seen["events"]
    assert [ev[k]["branch"] for k in ref.EVENT_REJECTS] == ["reject"] * len(ref.EVENT_REJECTS)
    assert ev[4]["skipped"] and any(i["pushed"] for i in ev)
    assert any(i["branch"] == "converged" for i in ev)
    if B >= 2:
        ov = seen["overflow"]
        assert ov[0]["reset"] and ov[41]["branch"] == "underflow" and before["status"][order.index(2)] == 2
    if B == 65:
        for fault in ref.START_FAULTS:                           # J = NaN, +inf, -inf; one NaN, +inf, -inf entry of G
            assert seen[fault][0]["branch"] == "nonfinite_start" and before["status"][order.index(ref.SCRIPTS.index(fault))] == 3
        assert any(i["branch"] == "converged" for i in seen["natural"])
        every = seen["natural"] + ev
        assert n == 1 or (any(i["fixed_lo"] > 0 for i in every) and any(i["fixed_hi"] > 0 for i in every))
        assert same_bits(np.sort(np.unique(before["status"])), np.array([1.0, 2.0, 3.0]))


# -- b. the chain on the model ----------------------------------------------------------------------------------------------------
_WORK = {}
_LOADED = {}
T_CHAIN, M_CHAIN, PGTOL_CHAIN = ref.T_CHAIN, ref.M_CHAIN, ref.PGTOL_CHAIN
starts, chain_kw, CHAIN_SHAPES = ref.chain_starts, ref.chain_kw, ref.CHAIN_SHAPES


def setup(engine, A, H, time=False):
    """The model of (A, H, time): N = 24, D = 2; cost = distance to 0.5 with identity weights.  Prepared when it changes."""
    key = (A, H, time)
    if key not in _WORK:
        _WORK[key] = synth.make_workload(N=24, D=2, A=A, H=H, B=2, include_time=time, time0=3.0, seed=7)
    w = _WORK[key]
    if _LOADED.get(id(engine)) != key:
        engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        engine.set_cost(np.full(2 + A, 0.5), np.eye(2 + A), np.eye(2), w.kappa)
        _LOADED[id(engine)] = key
    return w


def objective(engine, w, actions, propagation):
    f = engine.rollout_grad if propagation == "moment" else engine.rollout_linear_grad
    out = f(actions, w.mu0, w.S0, include_time=w.include_time, time0=w.time0)
    return out["J"], out["grad"]


def stepwise(engine, w, x0, H, A, deriv, propagation, name=None, check=True):
    """init + T_CHAIN x [objective and gradient of the state's own actions -> lbfgs_step]; every step checked against the
    restatement fed the device's own J and G.  Returns the final state on the host."""
    B, n = x0.shape
    kw = chain_kw(A, deriv)
    st = engine.lbfgs_state(B, n, M_CHAIN)
    engine.lbfgs_init(st, x0, H, A, **kw)
    before = host(st) if check else None
    worst = dict(margin=np.inf)
    for k in range(T_CHAIN):
        J, G = objective(engine, w, st["actions"].view(B, H, A), propagation)
        engine.lbfgs_step(st, J, G, H, A, k, C1, PGTOL_CHAIN, **kw)
        if check:
            after = host(st)
            check_step(name, before, after, J.cpu().numpy(), G.cpu().numpy(), k, H, A, M_CHAIN, kw, worst, PGTOL_CHAIN)
            before = after
    if check:
        record(name, **{k: v for k, v in worst.items() if np.isfinite(v)})
    return host(st)


@pytest.mark.parametrize("propagation", ["moment", "linearized"])
@pytest.mark.parametrize("deriv", [False, True])
@pytest.mark.parametrize("B", [1, 2, 65])
@pytest.mark.parametrize("A,H,time", CHAIN_SHAPES)
def test_chain_on_the_model_then_the_whole_search(engine, A, H, time, B, deriv, propagation):
    w = setup(engine, A, H, time)
    n = H * A
    x0 = starts(A, H, B)
    kw = chain_kw(A, deriv)
    name = f"lbfgs_chain[A={A},H={H},time={int(time)},B={B},deriv={int(deriv)},{propagation}]"
    final = stepwise(engine, w, x0, H, A, deriv, propagation, name)
    assert np.all(np.isfinite(final["J"])) and np.all(final["status"] <= 1.0)
    run = dict(propagation=propagation, include_time=w.include_time, time0=w.time0, c1=C1, pgtol=PGTOL_CHAIN, **kw)
    # the whole search leaves the state of the stepwise chain, bit for bit ...
    st = engine.lbfgs_state(B, n, M_CHAIN)
    st["buffer"].fill_(-7.0)
    rec = engine.lbfgs_search(st, w.mu0, w.S0, H, A, T_CHAIN, x0=x0, **run)
    whole = host(st)
    for key in FIELDS:
        assert same_bits(whole[key], final[key]), key
    # ... its winner record is gpmpc_argmin_async's on the state's J and x ...
    want = engine.argmin_async(st["J"], actions=st["x"])
    assert same_bits(rec.cpu().numpy(), want.cpu().numpy())
    assert same_bits(rec.cpu().numpy(), ref.winner(whole))
    # ... and so do two calls of half the iterations, the second continuing the state
    st2 = engine.lbfgs_state(B, n, M_CHAIN)
    st2["buffer"].fill_(-7.0)
    engine.lbfgs_search(st2, w.mu0, w.S0, H, A, T_CHAIN // 2, x0=x0, **run)
    rec2 = engine.lbfgs_search(st2, w.mu0, w.S0, H, A, T_CHAIN - T_CHAIN // 2, first_iteration=T_CHAIN // 2, **run)
    halves = host(st2)
    for key in FIELDS:
        assert same_bits(halves[key], final[key]), key
    assert same_bits(rec2.cpu().numpy(), rec.cpu().numpy())


@pytest.mark.parametrize("propagation", ["moment", "linearized"])
@pytest.mark.parametrize("deriv", [False, True])
def test_a_restart_does_not_depend_on_the_batch(engine, deriv, propagation):
    """Restart 37 of 65 against the same start run alone.  Precondition, asserted with the gradient launch itself at the start and
    at the end of the path: that launch keeps its bits between B = 65 and B = 1 on this shape."""
    A, H = 2, 3
    w = setup(engine, A, H)
    n, r = H * A, 37
    x0 = starts(A, H)
    kw = chain_kw(A, deriv)
    run = dict(propagation=propagation, include_time=w.include_time, time0=w.time0, c1=C1, pgtol=PGTOL_CHAIN, **kw)

    def search(x):
        st = engine.lbfgs_state(x.shape[0], n, M_CHAIN)
        engine.lbfgs_search(st, w.mu0, w.S0, H, A, T_CHAIN, x0=x, **run)
        return host(st)
    full = search(x0)
    # the precondition, probed with the gradient launch itself at the start and at the end of the path
    keeps = True
    for acts in (ref.to_model(x0, H, A, kw.get("max_change"), kw.get("action_prev")), full["actions"].reshape(65, H, A)):
        J65, G65 = (t.cpu().numpy() for t in objective(engine, w, acts, propagation))
        J1, G1 = (t.cpu().numpy() for t in objective(engine, w, acts[r:r + 1], propagation))
        keeps = keeps and same_bits(J65[r:r + 1], J1) and same_bits(G65[r:r + 1], G1)
    print(f"lbfgs_batch[deriv={int(deriv)},{propagation}]: gradient launch keeps its bits between B = 65 and B = 1: {keeps}")
    record(f"lbfgs_batch[deriv={int(deriv)},{propagation}]", gradient_keeps_bits_B65_B1=float(keeps))
    # measured on an MI355X: it does, for both propagations and both mappers -- so the comparison is the strong one, against B = 1
    assert keeps, "the gradient launch no longer keeps its bits between B = 65 and B = 1 on this shape: compare at equal dispatch"
    alone = search(x0[r:r + 1])
    for key in FIELDS:
        assert same_bits(full[key][r], alone[key][0]), key
    # ... and in the same batch, a copy of the start in another slot ends with the same bits
    twin = x0.copy()
    twin[5] = x0[r]
    both = search(twin)
    for key in FIELDS:
        assert same_bits(both[key][5], both[key][r]) and same_bits(both[key][r], full[key][r]), key


# -- c. errors touch nothing ------------------------------------------------------------------------------------------------------
def test_errors_are_reported_before_anything_is_written(engine, bare_engine):
    import gp_mpc_amd
    from gp_mpc_amd import _lib as L
    Err = gp_mpc_amd.GpmpcError                                   # (the package's own class object, whatever name it was imported under)
    A, H, B, m = 2, 3, 5, 3
    n = H * A
    w = setup(engine, A, H)
    x0 = starts(A, H, B)
    mc = np.array([0.3, 0.6])
    ap = np.array([0.2, 0.7])

    def good():
        st = engine.lbfgs_state(B, n, m)
        rec = engine.lbfgs_search(st, w.mu0, w.S0, H, A, 4, x0=x0, max_change=mc, action_prev=ap)
        return np.concatenate([st["buffer"].cpu().numpy(), rec.cpu().numpy()])
    reference = good()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    mu0, S0 = np.ascontiguousarray(w.mu0), np.ascontiguousarray(w.S0)
    big = int(engine.lib.gpmpc_lbfgs_state_size(8, 64, 4))

    def c_search(eng, want, B=B, H=H, A=A, prop=0, first=0, iters=4, m=m, c1=C1, pgtol=PGTOL, mapper=0, mcv=None, apv=None):
        state = torch.full((big,), -7.0, dtype=torch.float64, device=eng.device)
        best = torch.full((2 + 4096,), -7.0, dtype=torch.float64, device=eng.device)
        x = torch.full((4200,), 0.5, dtype=torch.float64, device=eng.device)
        rc = eng.lib.gpmpc_lbfgs_search(eng._h, ptr(mu0), ptr(S0), B, H, A, 0, 0.0, prop, first, iters, m, c1, pgtol, mapper,
                                        ptr(mcv), ptr(apv), x.data_ptr(), state.data_ptr(), best.data_ptr(), eng._stream())
        torch.cuda.synchronize()
        assert rc == want, (rc, eng.lib.gpmpc_last_error(eng._h))
        assert np.all(state.cpu().numpy() == -7.0) and np.all(best.cpu().numpy() == -7.0)

    ARG, LIM = L.GPMPC_ERR_ARG, L.GPMPC_ERR_LIMIT
    c_search(engine, ARG, B=0)
    c_search(engine, LIM, B=4097)
    c_search(engine, ARG, m=0)
    c_search(engine, LIM, m=33)
    c_search(engine, LIM, H=2049)                                # n = 4098
    c_search(engine, ARG, iters=0)
    c_search(engine, ARG, first=-1)
    c_search(engine, ARG, c1=0.0)
    c_search(engine, ARG, c1=1.0)
    c_search(engine, ARG, c1=float("nan"))
    c_search(engine, ARG, pgtol=-1e-300)
    c_search(engine, ARG, pgtol=float("nan"))
    c_search(engine, ARG, prop=2)
    c_search(engine, ARG, mapper=2)
    c_search(engine, ARG, mapper=1, mcv=mc)                      # the derivative mapper without action_prev
    c_search(engine, ARG, mapper=1, apv=ap)
    c_search(engine, ARG, A=3)                                   # D + A differs from the model's input dimension
    c_search(bare_engine, ARG)                                   # a search before prepare
    assert b"prepare" in bare_engine.lib.gpmpc_last_error(bare_engine._h)

    def c_step(want, B=B, H=H, A=A, k=1, m=m, c1=C1, pgtol=PGTOL, mapper=0, mcv=None, apv=None, init=False):
        eng = bare_engine
        state = torch.full((big,), -7.0, dtype=torch.float64, device=eng.device)
        x = torch.full((4200,), 0.5, dtype=torch.float64, device=eng.device)
        if init:
            rc = eng.lib.gpmpc_lbfgs_init(eng._h, x.data_ptr(), B, H, A, m, mapper, ptr(mcv), ptr(apv), state.data_ptr(), eng._stream())
        else:
            rc = eng.lib.gpmpc_lbfgs_step(eng._h, x.data_ptr(), x.data_ptr(), B, H, A, k, m, c1, pgtol, mapper, ptr(mcv), ptr(apv),
                                          state.data_ptr(), eng._stream())
        torch.cuda.synchronize()
        assert rc == want, (rc, eng.lib.gpmpc_last_error(eng._h))
        assert np.all(state.cpu().numpy() == -7.0)

    for init in (False, True):
        c_step(ARG, B=0, init=init)
        c_step(LIM, B=4097, init=init)
        c_step(ARG, m=0, init=init)
        c_step(LIM, m=33, init=init)
        c_step(LIM, H=4097, A=1, init=init)
        c_step(ARG, mapper=1, mcv=mc, init=init)
        c_step(LIM, H=1, A=25, mapper=1, mcv=np.full(25, 0.3), apv=np.full(25, 0.5), init=init)
    c_step(ARG, k=-1)
    c_step(ARG, c1=0.0)
    c_step(ARG, c1=1.5)
    c_step(ARG, pgtol=-1.0)

    # at the engine
    st = engine.lbfgs_state(B, n, m)
    st["buffer"].fill_(-7.0)
    best = torch.full((2 + n,), -7.0, dtype=torch.float64, device=engine.device)
    for bad in (dict(iterations=0), dict(c1=0.0), dict(c1=1.0), dict(pgtol=-1.0), dict(max_change=mc), dict(action_prev=ap),
                dict(first_iteration=0, x0=None)):
        args = dict(iterations=4, x0=x0, best_out=best)
        args.update(bad)
        with pytest.raises((Err, ValueError)):
            engine.lbfgs_search(st, w.mu0, w.S0, H, A, **args)
    with pytest.raises(ValueError):
        engine.lbfgs_search(st, w.mu0, w.S0, H, A, 4, x0=x0, propagation="unscented", best_out=best)
    with pytest.raises(ValueError):
        engine.lbfgs_search(st, w.mu0, w.S0, H + 1, A, 4, x0=x0, best_out=best)
    for bad in ((0, n, m), (4097, n, m), (B, 4097, m), (B, n, 0), (B, n, 33)):
        with pytest.raises(ValueError):
            engine.lbfgs_state(*bad)
    with pytest.raises((Err, ValueError)):
        bare_engine.lbfgs_search(st, w.mu0, w.S0, H, A, 4, x0=x0, best_out=best)
    torch.cuda.synchronize()
    assert np.all(st["buffer"].cpu().numpy() == -7.0) and np.all(best.cpu().numpy() == -7.0)
    assert same_bits(good(), reference)                          # the engine still works

    # a shape outside the gradient kernels: D = 2 with A = 7 action dimensions (the rollout itself supports it)
    w7 = synth.make_workload(N=24, D=2, A=7, H=2, B=2, seed=7)
    engine.prepare(w7.X, w7.Y, w7.lengthscales, w7.outputscales, w7.noises)
    engine.set_cost(np.full(9, 0.5), np.eye(9), np.eye(2), w7.kappa)
    _LOADED[id(engine)] = None
    st7 = engine.lbfgs_state(B, 14, m)
    st7["buffer"].fill_(-7.0)
    best7 = torch.full((16,), -7.0, dtype=torch.float64, device=engine.device)
    x7 = np.random.default_rng(1).uniform(size=(B, 14))
    with pytest.raises(Err) as ei:
        engine.lbfgs_search(st7, w7.mu0, w7.S0, 2, 7, 4, x0=x7, best_out=best7)
    assert ei.value.code == LIM
    torch.cuda.synchronize()
    assert np.all(st7["buffer"].cpu().numpy() == -7.0) and np.all(best7.cpu().numpy() == -7.0)
    J = engine.rollout(ref.to_model(x7, 2, 7), w7.mu0, w7.S0, trajectories=False, stage_costs=False)["J"].cpu().numpy()
    assert np.all(np.isfinite(J))
    # ... which the linearised propagation covers
    engine.lbfgs_search(st7, w7.mu0, w7.S0, 2, 7, 4, x0=x7, best_out=best7, propagation="linearized")
    h7 = host(st7)
    assert np.all(np.isfinite(h7["J"])) and np.all(h7["J"] <= engine.rollout_linear_grad(ref.to_model(x7, 2, 7), w7.mu0, w7.S0)["J"].cpu().numpy())
    setup(engine, A, H)
    assert same_bits(good(), reference)


# -- d. the controller ------------------------------------------------------------------------------------------------------------
# (J_device - J_scipy) / |J_scipy| at the provisional defaults (30 iterations, 10 pairs) from the same 6 starts, measured on an
# MI355X: GAP_MEASURED; asserted with a factor 2 of headroom (the two methods differ in line search and in their treatment of the
# bounds, so equality is not expected); a device search that ends lower is asserted to stay so
GAP_MEASURED = 7.600009e-03


def test_lbfgs_device_in_the_controller(engine):
    g = load("lcb_grad_norm")
    w = workload_of(g)
    N, D, A, E, H, B = w.dims
    restarts = 6
    c = make_controller(w, optimize=True, restarts=restarts, engine=engine)
    c.config.controller.candidate_optimizer = "lbfgs_device"
    assert c.config.controller.lbfgs_device_iterations == 30 and c.config.controller.lbfgs_device_history == 10
    np.random.seed(7)
    a = c.get_action(obs_mu=w.mu0)
    assert a.shape == (A,) and c.num_rollouts == restarts * 30 + 1 and c.lbfgs_evaluations == 30
    J_dev, x_dev = c.best_candidate_J, c.actions_mpc_previous_iter.copy()
    assert c.candidates_final_J.shape == (restarts,) and J_dev == np.min(c.candidates_final_J)
    assert c.best_candidate_index == int(np.argmin(c.candidates_final_J))
    # strictly below the best starting point
    J0 = c.evaluate_candidates(c.lbfgs_device_starts, torch.as_tensor(w.mu0), torch.as_tensor(w.S0))["J"].cpu().numpy()
    assert J_dev < np.min(J0) and np.all(c.candidates_final_J <= J0 + 1e-12 * np.abs(J0))
    # the caches hold the winner's trajectory
    assert abs(c.cost_traj_mean_lcb.item() + J_dev) <= 1e-12 * abs(J_dev)
    # the second step warm-starts from the shifted solution
    from gp_mpc_amd.control_objects.actions_mappers.action_init_functions import generate_mpc_action_init_frompreviousiter
    c.get_action(obs_mu=w.mu0)
    shifted = np.asarray(generate_mpc_action_init_frompreviousiter(x_dev, dim_action=A)).reshape(-1)
    assert np.array_equal(c.lbfgs_device_starts[0], shifted) and np.isfinite(c.best_candidate_J)
    # the gap to the sequential scipy loop from the same starts
    seq = make_controller(w, optimize=True, restarts=restarts, engine=engine)
    np.random.seed(7)
    seq._get_optimal_actions(torch.as_tensor(w.mu0), torch.as_tensor(w.S0))
    J_seq, _ = seq.compute_mean_lcb_trajectory(seq.actions_mpc_previous_iter, torch.as_tensor(w.mu0), torch.as_tensor(w.S0))
    gap = (J_dev - J_seq) / abs(J_seq)
    print(f"lbfgs_device J {J_dev!r}  scipy J {J_seq!r}  gap {gap:.6e}  starts' best {np.min(J0)!r}")
    record("lbfgs_device_controller", J_device=J_dev, J_scipy=J_seq, gap=gap, best_start=float(np.min(J0)))
    assert gap <= (0.0 if GAP_MEASURED <= 0.0 else 2.0 * GAP_MEASURED)
