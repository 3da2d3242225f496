"""Tier 2 (GPU): gpmpc_train_search (csrc/mll_batch.hip) -- R restarts per GP of the box-constrained device L-BFGS on the batched
training loss -- against the public pieces it is made of and the numpy restatement of tests/train_device_ref.py, and
GpStateTransitionModel.train(optimizer="lbfgs_device") on top of it.

The chain init -> [mll_batch of the state's actions with the box -> lbfgs_step] is checked step by step the way
test_gpu_lbfgs_device.check_step checks a step: the restatement is applied to the DEVICE's own state before the step and the
device's own (J, G), so errors do not accumulate, and every Armijo / curvature / descent decision of the longdouble restatement
must have a relative margin >= 1e-6 (asserted).  Copies and decisions are compared bit for bit, computed values with
    tolerance = 10 e64 + 64 eps scale        (e64: the float64 restatement's own error against the longdouble one, computed here).
The whole search is then compared with that chain bit for bit.

A start that is not finite: gpmpc_lbfgs_init clips a NaN coordinate to 0, a valid corner of the box, so an x0 row of NaN is the
row of zeros (asserted below) and cannot end with status 3.  The status-3 paths of the winner rule are reached through the public
pieces instead: after the init one restart's model actions are overwritten with NaN, the first step (mll_batch: loss +inf, info
1; lbfgs_step: status 3) is taken through the pieces, and gpmpc_train_search continues that state with first_iteration = 1.
"""
import functools
import queue

import numpy as np
import pytest
import torch

import lbfgs_device_ref as ref
import train_device_ref as tref
from oracle import gp_training, synth

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
LD = np.longdouble
C1, PGTOL = 1e-4, 1e-5
FIELDS = ("x", "g", "d", "xt", "actions", "J", "alpha", "status", "pushes", "S", "Y", "sy", "yy")
MIN_MARGIN = 1e-6
STEPS, HISTORY, D = 6, 3, 2


def tol(e64, scale=1.0):
    return 10.0 * float(e64) + 64.0 * EPS * float(scale)


def err(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    if not a.size:
        return 0.0
    same = (a == b) | (np.isnan(a) & np.isnan(b))
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


def host(state):
    flat = state["buffer"].cpu().numpy()
    out, off = {}, 0
    for k in FIELDS:
        cnt = state[k].numel()
        out[k] = flat[off:off + cnt].reshape(tuple(state[k].shape)).copy()
        off += cnt
    return out


def check_step(name, before, after, J, G, k, n, m, worst):
    """`after` (device) against the restatement's step k from `before` (device) and (J, G): test_gpu_lbfgs_device.check_step for
    the identity mapper with H = 1, A = n."""
    s64, i64 = ref.step(before, J, G, k, 1, n, m, C1, PGTOL)
    sld, ild = ref.step(before, J, G, k, 1, n, m, C1, PGTOL, dtype=LD)
    margin = ref.min_margin(ild)
    worst["margin"] = min(worst["margin"], margin)
    assert margin >= MIN_MARGIN, f"{name} step {k}: a decision of the restatement has relative margin {margin:.3e}"
    assert [i["branch"] for i in i64] == [i["branch"] for i in ild]
    for key in ("status", "pushes", "alpha", "J", "x", "g"):
        assert same_bits(after[key], s64[key]), (name, k, key)
    for b in range(before["x"].shape[0]):
        if ild[b]["branch"] == "frozen":
            for key in FIELDS:
                assert same_bits(after[key][b], before[key][b]), (name, k, b, key)
            continue
        e = lambda key: err(s64[key][b], sld[key][b])            # noqa: E731
        amax = lambda v: float(np.max(np.abs(np.asarray(v, dtype=np.float64)), initial=0.0))      # noqa: E731
        gg = np.concatenate([before["g"][b], after["g"][b]])
        gmax = amax(gg[np.isfinite(gg)])
        smax, ymax = amax(sld["S"][b]), amax(sld["Y"][b])
        tols = dict(d=tol(e("d"), max(gmax, smax, ymax)), xt=tol(e("xt")), actions=tol(e("actions")), S=tol(e("S")),
                    Y=tol(e("Y"), gmax), sy=tol(e("sy"), max(smax, ymax)), yy=tol(e("yy"), ymax))
        for key, t in tols.items():
            got = err(after[key][b], sld[key][b])
            assert got <= t, (name, k, b, key, got, t)
        assert np.all((after["xt"][b] >= 0.0) & (after["xt"][b] <= 1.0))
    return ild


@functools.lru_cache(maxsize=None)
def problem(N):
    """Workload of N points with D = 2 GPs, the box [theta / 8, 8 theta] around its hyper-parameters, and 5 seeded starts."""
    w = synth.make_workload(N, D, 1, 3, 2, seed=N)
    base = np.concatenate([w.lengthscales, w.outputscales[:, None], w.noises[:, None]], axis=1)
    x0 = np.random.default_rng(40 + N).uniform(0.05, 0.95, size=(5, D, base.shape[1]))
    return w, base / 8.0, base * 8.0, x0


def evaluate(engine, w, st, R, lo, hi, log_scale):
    n = st["n"]
    out = engine.mll_batch(w.X, w.Y, st["actions"].view(R, D, n), lo=lo, hi=hi, log_scale=log_scale)
    return out["loss"].reshape(R * D), out["grad"].reshape(R * D, 1, n), out


def stepwise(engine, w, x0, lo, hi, log_scale, name, spoil=None):
    """init + STEPS x [mll_batch of the state's actions with the box -> lbfgs_step], every step checked.  `spoil`: restarts whose
    model actions are overwritten with NaN after the init.  Returns (final state on the host, state after the first step)."""
    R, _, n = x0.shape
    P = R * D
    st = engine.lbfgs_state(P, n, HISTORY)
    engine.lbfgs_init(st, x0.reshape(P, n), 1, n)
    if spoil is not None:
        st["actions"].view(R, D, n)[spoil] = float("nan")
    before = host(st)
    worst, first = dict(margin=np.inf), None
    for k in range(STEPS):
        J, G, out = evaluate(engine, w, st, R, lo, hi, log_scale)
        engine.lbfgs_step(st, J, G, 1, n, k, C1, PGTOL)
        after = host(st)
        check_step(name, before, after, J.cpu().numpy(), G.cpu().numpy(), k, n, HISTORY, worst)
        if k == 0:
            first = (st["buffer"].clone(), out["info"].cpu().numpy())
        before = after
    print(f"{name}: smallest decision margin {worst['margin']:.3e}")
    return before, first


def check_winner(rec, state, lo, hi, log_scale):
    """The device record (D, 3 + n) against the restated winner rule on the read-back state."""
    want = tref.winner(state["J"], state["status"], state["x"], lo, hi, log_scale, D)
    assert same_bits(rec[:, :3], want[:, :3]), (rec[:, :3], want[:, :3])
    n = state["x"].shape[1]
    src = np.maximum(want[:, 1].astype(int), 0) * D + np.arange(D)
    exact = tref.box_map(state["x"][src], lo, hi, log_scale, dtype=LD)
    assert np.all(np.abs(rec[:, 3:].astype(LD) - exact) <= 4 * np.spacing(np.abs(want[:, 3:]))), (rec[:, 3:], want[:, 3:])
    assert rec.shape == (D, 3 + n)


@pytest.mark.parametrize("log_scale", [False, True])
@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("N", [24, 65])
def test_chain_through_the_pieces_then_the_whole_search(engine, N, R, log_scale):
    w, lo, hi, starts = problem(N)
    x0 = starts[:R]
    n = x0.shape[2]
    name = f"train_chain[N={N},R={R},log={int(log_scale)}]"
    final, _ = stepwise(engine, w, x0, lo, hi, log_scale, name)
    assert np.all(np.isfinite(final["J"])) and np.all(final["status"] != 3.0)
    run = dict(c1=C1, pgtol=PGTOL, log_scale=log_scale)
    # the whole search leaves the state of the stepwise chain, bit for bit ...
    st = engine.lbfgs_state(R * D, n, HISTORY)
    st["buffer"].fill_(-7.0)
    rec = engine.train_search(st, w.X, w.Y, lo, hi, STEPS, x0=x0, **run).cpu().numpy()
    whole = host(st)
    for key in FIELDS:
        assert same_bits(whole[key], final[key]), key
    check_winner(rec, whole, lo, hi, log_scale)
    assert np.all(rec[:, 0] <= final["J"].reshape(R, D)[0])           # never worse than restart 0
    # ... and so do two calls of 2 and 4 iterations, the second continuing the state
    st2 = engine.lbfgs_state(R * D, n, HISTORY)
    st2["buffer"].fill_(-7.0)
    engine.train_search(st2, w.X, w.Y, lo, hi, 2, x0=x0, **run)
    rec2 = engine.train_search(st2, w.X, w.Y, lo, hi, STEPS - 2, first_iteration=2, **run).cpu().numpy()
    parts = host(st2)
    for key in FIELDS:
        assert same_bits(parts[key], final[key]), key
    assert same_bits(rec2, rec)
    # the one-synchronisation wrapper returns the same search
    res = engine.train_search_host(w.X, w.Y, x0, lo, hi, STEPS, history=HISTORY, **run)
    assert same_bits(res["J"], whole["J"].reshape(R, D)) and np.array_equal(res["status"], whole["status"].reshape(R, D))
    assert same_bits(res["theta"], rec[:, 3:]) and same_bits(res["loss"], rec[:, 0]) and np.array_equal(res["restart"], rec[:, 1])


@pytest.mark.parametrize("log_scale", [False, True])
@pytest.mark.parametrize("R", [1, 5])
def test_non_finite_starts_and_the_winner_rule(engine, R, log_scale):
    N = 24
    w, lo, hi, starts = problem(N)
    x0 = starts[:R].copy()
    n = x0.shape[2]
    run = dict(c1=C1, pgtol=PGTOL, log_scale=log_scale)
    # an x0 row of NaN is the row of zeros: gpmpc_lbfgs_init clips it to the corner of the box
    nan_row, zero_row = x0.copy(), x0.copy()
    nan_row[R - 1, 1], zero_row[R - 1, 1] = np.nan, 0.0
    got = []
    for x in (nan_row, zero_row):
        st = engine.lbfgs_state(R * D, n, HISTORY)
        got.append((engine.train_search(st, w.X, w.Y, lo, hi, STEPS, x0=x, **run).cpu().numpy(), host(st)))
    assert same_bits(got[0][0], got[1][0]) and all(same_bits(got[0][1][k], got[1][1][k]) for k in FIELDS)
    assert np.all(got[0][1]["status"] != 3.0)
    # status 3 through the pieces: restart R - 1 of GP 1 evaluates NaN actions at its start
    spoil = (R - 1, 1)
    name = f"train_status3[R={R},log={int(log_scale)}]"
    final, (after_first, info) = stepwise(engine, w, x0, lo, hi, log_scale, name, spoil=spoil)
    status = final["status"].reshape(R, D)
    assert status[spoil] == 3.0 and np.sum(status == 3.0) == 1 and info[spoil] == 1 and np.sum(info != 0) == 1
    assert final["J"].reshape(R, D)[spoil] == np.inf
    # the search continues the state after that first step: the same final state, and the winner leaves the restart out
    st = engine.lbfgs_state(R * D, n, HISTORY)
    st["buffer"].copy_(after_first)
    rec = engine.train_search(st, w.X, w.Y, lo, hi, STEPS - 1, first_iteration=1, **run).cpu().numpy()
    whole = host(st)
    for key in FIELDS:
        assert same_bits(whole[key], final[key]), key
    check_winner(rec, whole, lo, hi, log_scale)
    if R == 1:                                                       # every restart of GP 1 has status 3
        assert rec[1, 0] == np.inf and rec[1, 1] == -1.0 and rec[1, 2] == 3.0 and rec[0, 1] == 0.0
    else:
        assert rec[1, 1] != R - 1 and rec[1, 1] >= 0.0 and np.isfinite(rec[1, 0])


def test_errors_are_reported_before_anything_is_written(engine):
    import ctypes as C
    import gp_mpc_amd
    from gp_mpc_amd import _lib as L
    w, lo, hi, starts = problem(24)
    ARG, LIM = L.GPMPC_ERR_ARG, L.GPMPC_ERR_LIMIT
    dev = engine.device
    X = torch.zeros(300 * 25, dtype=torch.float64, device=dev)
    Y = torch.zeros(300 * 17, dtype=torch.float64, device=dev)
    box = torch.ones(17 * 27, dtype=torch.float64, device=dev)
    x0 = torch.full((4100 * 27,), 0.5, dtype=torch.float64, device=dev)
    big = int(engine.lib.gpmpc_lbfgs_state_size(64, 26, 32))

    def call(want, N=24, D=2, E=3, R=2, log_scale=1, first=0, iters=3, m=3, c1=C1, pgtol=PGTOL, X=X, Y=Y, lo=box, hi=box, x=x0,
             no_state=False):
        state = torch.full((big,), -7.0, dtype=torch.float64, device=dev)
        best = torch.full((16 * 29,), -7.0, dtype=torch.float64, device=dev)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
        rc = engine.lib.gpmpc_train_search(engine._h, p(X), p(Y), N, D, E, R, p(lo), p(hi), log_scale, first, iters, m, c1, pgtol,
                                           p(x), None if no_state else p(state), p(best), engine._stream())
        torch.cuda.synchronize()
        assert rc == want, (rc, engine.lib.gpmpc_last_error(engine._h))
        assert bool((state == -7.0).all()) and bool((best == -7.0).all())

    call(ARG, X=None)
    call(ARG, Y=None)
    call(ARG, x=None)                                                # first_iteration == 0 needs the starts
    call(ARG, no_state=True)
    call(ARG, lo=None)                                               # only one of lo and hi
    call(ARG, lo=None, hi=None)                                      # the box is required
    call(ARG, N=0)
    call(ARG, R=0)
    call(ARG, log_scale=2)
    call(ARG, m=0)
    call(ARG, iters=0)
    call(ARG, first=-1)
    call(ARG, c1=0.0)
    call(ARG, c1=1.0)
    call(ARG, pgtol=-1.0)
    call(LIM, N=257)
    call(LIM, D=17, E=18)
    call(LIM, E=25)
    call(LIM, D=16, E=17, R=257)
    call(LIM, m=33)
    # the wrapper's own checks
    st = engine.lbfgs_state(2 * D, 5, HISTORY)
    st["buffer"].fill_(-7.0)
    for kw in (dict(lo=None), dict(lo=None, hi=None), dict(lo=hi, hi=lo), dict(lo=-lo), dict(x0=starts[:3])):
        args = dict(lo=lo, hi=hi, x0=starts[:2])
        args.update(kw)
        with pytest.raises(ValueError):
            engine.train_search(st, w.X, w.Y, args["lo"], args["hi"], 3, x0=args["x0"])
    with pytest.raises(ValueError):
        engine.train_search(engine.lbfgs_state(2 * D, 4, HISTORY), w.X, w.Y, lo, hi, 3, x0=starts[:2])
    with pytest.raises((gp_mpc_amd.GpmpcError, ValueError)):
        engine.train_search(st, w.X, w.Y, lo, hi, 0, x0=starts[:2])
    torch.cuda.synchronize()
    assert bool((st["buffer"] == -7.0).all())


def test_training_with_the_device_search(monkeypatch):
    """GpStateTransitionModel.train(optimizer="lbfgs_device") from lengthscales 4 x too long: per GP the returned parameters are
    no worse than the incoming ones under the oracle's loss and lie inside the constraint box, and the training takes ONE host
    synchronisation -- one train_search_host call, no other loss evaluation (counted on the engine)."""
    import sys
    import gp_mpc_amd
    from train_stub_engine import engine_module_of
    GpStateTransitionModel = gp_mpc_amd.GpStateTransitionModel
    gm = sys.modules[GpStateTransitionModel.__module__]
    GpHyperParameters, SavedState, TrainingFailed = gm.GpHyperParameters, gm.SavedState, gm.TrainingFailed
    engine_module = engine_module_of(GpStateTransitionModel)         # the module `train` takes HipEngine from
    calls = {}

    class Counting(engine_module.HipEngine):
        def _count(self, name):
            calls[name] = calls.get(name, 0) + 1

        def train_search_host(self, *a, **k):
            self._count("train_search_host")
            return super().train_search_host(*a, **k)

        def train_search(self, *a, **k):
            self._count("train_search")
            return super().train_search(*a, **k)

        def mll(self, *a, **k):
            self._count("mll")
            return super().mll(*a, **k)

        def mll_batch(self, *a, **k):
            self._count("mll_batch")
            return super().mll_batch(*a, **k)

    monkeypatch.setattr(engine_module, "HipEngine", Counting)
    N = 65
    w = synth.make_workload(N, D, 1, 3, 2, seed=N)
    E = w.X.shape[1]
    cons = {"min_lengthscale": np.full((D, E), 4e-3), "max_lengthscale": np.full((D, E), 25.0),
            "min_outputscale": np.full(D, 1e-3), "max_outputscale": np.full(D, 0.95),
            "min_std_noise": np.full(D, 1e-3), "max_std_noise": np.full(D, 3e-1)}
    incoming = [GpHyperParameters(4.0 * w.lengthscales[a], w.outputscales[a], w.noises[a]).state_dict() for a in range(D)]
    st = SavedState(w.X, w.Y, incoming, cons)
    st.to_arrays()
    q = queue.Queue()
    torch.manual_seed(11)
    GpStateTransitionModel.train(q, st, 7e-3, 15, 1e-3, optimizer="lbfgs_device", restarts=8, device_iterations=30)
    out = q.get_nowait()
    assert q.empty() and not isinstance(out, TrainingFailed) and len(out) == D
    assert calls == {"train_search_host": 1, "train_search": 1}, calls
    K0, K1, K2 = GpHyperParameters.KEYS
    for a in range(D):
        ls, osc, nz = out[a][K0], out[a][K1], out[a][K2]
        assert ls.shape == (1, E) and osc.shape == () and nz.shape == (1,) and ls.dtype == osc.dtype == nz.dtype == np.float64
        up = 1 + 4 * EPS                                             # the box map is good to 4 ulp at its upper face
        assert np.all((ls >= 4e-3) & (ls <= 25.0 * up)) and 1e-3 <= float(osc) <= 0.95 * up and 1e-6 <= float(nz[0]) <= 9e-2 * up
        new = gp_training.neg_mll_and_grad(w.X, w.Y[:, a], ls.reshape(-1), float(osc), float(nz[0]))[0]
        old = gp_training.neg_mll_and_grad(w.X, w.Y[:, a], 4.0 * w.lengthscales[a], w.outputscales[a], w.noises[a])[0]
        print(f"train lbfgs_device gp {a}: oracle loss {old:.6f} -> {new:.6f}")
        assert new <= old
