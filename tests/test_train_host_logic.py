"""Tier 1 (no GPU): the host side of the device hyper-parameter search -- TrainingConfig's new keywords, what
start_training_process hands to the training process, GpStateTransitionModel.train(optimizer="lbfgs_device") against a stub engine
(tests/train_stub_engine.py), and what HipEngine.mll_batch / train_search / train_search_host hand to the C ABI (recorded with
the stand-in library of tests/engine_call_cases.py)."""
import ctypes as C
import queue
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import train_device_ref as tref
from engine_call_cases import Recorder, RecordingEngine
from gp_mpc_amd import _lib as L
from oracle import synth
from train_stub_engine import StubEngine, engine_module_of

K0, K1, K2 = "covar_module.base_kernel.lengthscale", "covar_module.outputscale", "likelihood.noise"
D = 2


class _Package:
    """The package's classes, looked up when a test runs and through the package's own attributes: the package is importable
    under two names, and a module-level import by the other one would make second copies of its modules for every test file."""

    def __getattr__(self, name):
        import sys
        import gp_mpc_amd
        if hasattr(gp_mpc_amd, name):
            return getattr(gp_mpc_amd, name)
        if name == "TrainingConfig":
            from gp_mpc_amd.config_classes import TrainingConfig
            return TrainingConfig
        return getattr(sys.modules[gp_mpc_amd.GpStateTransitionModel.__module__], name)


M = _Package()


# -- configuration ------------------------------------------------------------------------------------------------------------------
def test_training_config_validates_the_new_keywords():
    tc = M.TrainingConfig()
    assert (tc.optimizer, tc.restarts, tc.device_iterations, tc.device_history) == ("lbfgs", 16, 30, 10)
    tc = M.TrainingConfig(optimizer="lbfgs_device", restarts=4, device_iterations=7, device_history=3)
    assert (tc.optimizer, tc.restarts, tc.device_iterations, tc.device_history) == ("lbfgs_device", 4, 7, 3)
    for bad in (dict(optimizer="adam"), dict(optimizer=None), dict(restarts=0), dict(restarts=4097), dict(restarts=2.0),
                dict(restarts=True), dict(device_iterations=0), dict(device_iterations=-3), dict(device_history=0),
                dict(device_history=33), dict(device_history="10")):
        with pytest.raises(ValueError):
            M.TrainingConfig(**bad)


def test_start_training_process_forwards_the_new_fields():
    started = []

    class FakeProcess:
        def __init__(self, target=None, args=(), kwargs=None):
            self.target, self.args, self.kwargs = target, args, kwargs or {}

        def start(self):
            started.append(self)
    state = SimpleNamespace(to_arrays=lambda: None)
    tc = M.TrainingConfig(lr_train=0.1, iter_train=9, optimizer="lbfgs_device", restarts=5, device_iterations=12, device_history=4)
    fake = SimpleNamespace(transition_model=SimpleNamespace(save_state=lambda: state), config=SimpleNamespace(training=tc),
                           ctx=SimpleNamespace(Process=FakeProcess), queue_train="queue")
    M.GpMpcController.start_training_process(fake)
    (p,) = started
    assert p.target is M.GpStateTransitionModel.train and fake.p_train is p
    assert p.args == ("queue", state, 0.1, 9, tc.clip_grad_value, tc.print_train, tc.step_print_train, "auto")
    assert p.kwargs == dict(optimizer="lbfgs_device", restarts=5, device_iterations=12, device_history=4)
    # the defaults are today's loop, and train's own defaults agree with them
    fake.config.training = M.TrainingConfig()
    M.GpMpcController.start_training_process(fake)
    assert started[-1].kwargs == dict(optimizer="lbfgs", restarts=16, device_iterations=30, device_history=10)
    import inspect
    sig = inspect.signature(M.GpStateTransitionModel.train).parameters
    assert {k: sig[k].default for k in started[-1].kwargs} == started[-1].kwargs
    assert list(sig)[-4:] == ["optimizer", "restarts", "device_iterations", "device_history"]      # appended


# -- train against the stub ---------------------------------------------------------------------------------------------------------
def saved_state(N, scale=4.0, seed=None):
    w = synth.make_workload(N, D, 1, 3, 2, seed=N if seed is None else seed)
    E = w.X.shape[1]
    cons = {"min_lengthscale": np.full((D, E), 4e-3), "max_lengthscale": np.full((D, E), 25.0),
            "min_outputscale": np.full(D, 1e-3), "max_outputscale": np.full(D, 0.95),
            "min_std_noise": np.full(D, 1e-3), "max_std_noise": np.full(D, 3e-1)}
    incoming = [M.GpHyperParameters(scale * w.lengthscales[a], w.outputscales[a], w.noises[a]).state_dict() for a in range(D)]
    st = M.SavedState(w.X, w.Y, incoming, cons)
    st.to_arrays()
    lo = np.concatenate([cons["min_lengthscale"], cons["min_outputscale"][:, None], cons["min_std_noise"][:, None] ** 2], axis=1)
    hi = np.concatenate([cons["max_lengthscale"], cons["max_outputscale"][:, None], cons["max_std_noise"][:, None] ** 2], axis=1)
    theta = np.concatenate([scale * w.lengthscales, w.outputscales[:, None], w.noises[:, None]], axis=1)
    return w, st, lo, hi, theta


@pytest.fixture
def stub(monkeypatch):
    StubEngine.reset()
    monkeypatch.setattr(engine_module_of(M.GpStateTransitionModel), "HipEngine", StubEngine)
    yield StubEngine
    StubEngine.reset()


def run_train(st, **kw):
    q = queue.Queue()
    M.GpStateTransitionModel.train(q, st, 1e-1, 2, 1e-3, **kw)
    out = q.get_nowait()
    assert q.empty()                                                 # exactly one answer
    return out


def check_answer(out, E):
    assert isinstance(out, list) and not isinstance(out, M.TrainingFailed) and len(out) == D
    for p in out:
        assert sorted(p) == sorted(M.GpHyperParameters.KEYS)
        assert p[K0].shape == (1, E) and p[K1].shape == () and p[K2].shape == (1,)
        assert all(isinstance(p[k], np.ndarray) and p[k].dtype == np.float64 for k in p)


def test_train_with_the_device_search(stub):
    w, st, lo, hi, theta = saved_state(24)
    E, R = w.X.shape[1], 5
    torch.manual_seed(5)
    out = run_train(st, optimizer="lbfgs_device", restarts=R, device_iterations=6, device_history=3)
    check_answer(out, E)
    (eng,) = stub.made
    assert eng.closed and [c[0] for c in eng.calls] == ["train_search_host"]
    call = eng.calls[0][1]
    assert call["iterations"] == 6 and call["history"] == 3 and call["log_scale"] is True
    assert np.array_equal(call["X"], w.X) and np.array_equal(call["Y"], w.Y)
    assert np.array_equal(call["lo"], lo) and np.array_equal(call["hi"], hi)
    # start 0 is the incoming theta, mapped to x; starts 1 .. R - 1 are ONE (R - 1, D, n) draw
    assert call["x0"].shape == (R, D, E + 2)
    assert np.allclose(tref.box_map(call["x0"][0], lo, hi, True), theta, rtol=1e-12, atol=0)
    torch.manual_seed(5)
    assert np.array_equal(call["x0"][1:], torch.rand((R - 1, D, E + 2), dtype=torch.float64).numpy())
    # the answer is the stub's winner, which is no worse than the incoming parameters
    for a in range(D):
        got = np.concatenate([out[a][K0].reshape(-1), out[a][K1].reshape(1), out[a][K2]])
        assert np.all((got >= lo[a]) & (got <= hi[a] * (1 + 1e-15)))
        assert tref.loss_and_grad_theta(w.X, w.Y[:, a], got)[0] <= tref.loss_and_grad_theta(w.X, w.Y[:, a], theta[a])[0]


def test_incoming_parameters_outside_the_box_are_clipped_into_it(stub):
    w, st, lo, hi, theta = saved_state(24, scale=40.0)               # lengthscales of 20 .. 60 against a box up to 25
    stub.answer = lambda eng, X, Y, x0, lo, hi: {"theta": tref.box_map(x0[0], lo, hi, True), "loss": np.zeros(D),
                                                  "restart": np.zeros(D, dtype=np.int64), "J": np.zeros((1, D)),
                                                  "status": np.zeros((1, D), dtype=np.int64)}
    out = run_train(st, optimizer="lbfgs_device", restarts=1)
    x0 = stub.made[0].calls[0][1]["x0"]
    assert x0.shape == (1, D, w.X.shape[1] + 2) and np.all((x0 >= 0.0) & (x0 <= 1.0)) and np.any(x0 == 1.0)
    assert np.allclose(tref.box_map(x0[0], lo, hi, True), np.clip(theta, lo, hi), rtol=1e-12, atol=0)
    check_answer(out, w.X.shape[1])


def test_a_gp_without_a_finite_start_keeps_its_incoming_parameters(stub):
    w, st, lo, hi, theta = saved_state(24)
    E = w.X.shape[1]
    won = np.stack([lo[0] * 2.0, lo[1] * 3.0])
    stub.answer = lambda eng, X, Y, x0, lo, hi: {"theta": won, "loss": np.array([np.inf, -1.0]), "restart": np.array([-1, 2]),
                                                  "J": np.zeros((3, D)), "status": np.zeros((3, D), dtype=np.int64)}
    out = run_train(st, optimizer="lbfgs_device", restarts=3)
    check_answer(out, E)
    assert np.array_equal(out[0][K0], theta[0, :E].reshape(1, E)) and out[0][K1] == theta[0, E] and out[0][K2][0] == theta[0, E + 1]
    assert np.array_equal(out[1][K0], won[1, :E].reshape(1, E)) and out[1][K1] == won[1, E] and out[1][K2][0] == won[1, E + 1]


def test_a_memory_beyond_256_points_takes_the_host_loop(stub, capsys):
    w, st, lo, hi, theta = saved_state(257)
    torch.manual_seed(1)
    out = run_train(st, optimizer="lbfgs_device", restarts=3, print_train=True)
    check_answer(out, w.X.shape[1])
    (eng,) = stub.made
    names = [c[0] for c in eng.calls]
    assert "train_search_host" not in names and names.count("mll") >= 2 and eng.closed
    said = [line for line in capsys.readouterr().out.splitlines() if "257" in line and "256" in line]
    assert len(said) == 1
    # ... and 256 points are still the device search
    StubEngine.reset()
    w, st, lo, hi, theta = saved_state(256)
    stub.answer = lambda eng, X, Y, x0, lo, hi: {"theta": tref.box_map(x0[0], lo, hi, True), "loss": np.zeros(D),
                                                  "restart": np.zeros(D, dtype=np.int64), "J": np.zeros((2, D)),
                                                  "status": np.zeros((2, D), dtype=np.int64)}
    run_train(st, optimizer="lbfgs_device", restarts=2)
    assert [c[0] for c in stub.made[0].calls] == ["train_search_host"]


def test_a_raising_engine_yields_training_failed(stub):
    w, st, lo, hi, theta = saved_state(24)
    stub.fail = RuntimeError("the device went away")
    out = run_train(st, optimizer="lbfgs_device", restarts=2)
    assert isinstance(out, M.TrainingFailed) and "the device went away" in out.reason and len(out) == D
    assert np.array_equal(np.asarray(out[0][K0]).reshape(-1), theta[0, :w.X.shape[1]]) and stub.made[0].closed
    for bad in (dict(optimizer="adam"), dict(optimizer="lbfgs_device", loss_evaluator=lambda *a: None)):
        out = run_train(st, **bad)
        assert isinstance(out, M.TrainingFailed) and len(out) == D


# -- what the engine hands to the C ABI ---------------------------------------------------------------------------------------------
class SizedRecorder(Recorder):
    """The stand-in library with gpmpc_lbfgs_state_size answered (x g d xt actions | J alpha status pushes | S Y | sy yy)."""

    def gpmpc_lbfgs_state_size(self, B, n, m):
        return 5 * B * n + 4 * B + 2 * B * m * n + 2 * B * m


def recording_engine():
    eng = RecordingEngine(3, None)
    eng.lib = SizedRecorder()
    return eng


def data(N=6, E=3, R=2):
    rng = np.random.default_rng(0)
    t = lambda *sh: torch.as_tensor(rng.uniform(0.1, 0.9, size=sh))      # noqa: E731
    return dict(X=t(N, E), Y=t(N, D), params=t(R, D, E + 2), lo=np.full((D, E + 2), 0.25), hi=np.full((D, E + 2), 4.0))


def test_mll_batch_marshalling():
    d, eng = data(), recording_engine()
    out = eng.mll_batch(d["X"], d["Y"], d["params"], lo=d["lo"], hi=d["hi"])
    (name, a), = eng.lib.calls
    lo_d, hi_d = eng.converted[-2], eng.converted[-1]
    assert name == "gpmpc_mll_batch" and len(a) == len(L.SIGNATURES[name][1])
    assert a[1:] == (d["X"].data_ptr(), d["Y"].data_ptr(), 6, D, 3, d["params"].data_ptr(), 2, lo_d.data_ptr(), hi_d.data_ptr(), 1,
                     out["loss"].data_ptr(), out["grad"].data_ptr(), out["theta"].data_ptr(), out["info"].data_ptr(), None)
    assert np.array_equal(lo_d.numpy(), d["lo"]) and np.array_equal(hi_d.numpy(), d["hi"])
    assert {k: (tuple(v.shape), v.dtype) for k, v in out.items()} == {
        "loss": ((2, D), torch.float64), "grad": ((2, D, 5), torch.float64), "theta": ((2, D, 5), torch.float64),
        "info": ((2, D), torch.int32)}
    # without a box both pointers are NULL and theta is the rows themselves; the linear map is log_scale 0; `out` is reused
    eng.lib.calls.clear()
    again = eng.mll_batch(d["X"], d["Y"], d["params"], log_scale=False, out=out)
    (name, a), = eng.lib.calls
    assert again is out and a[8:11] == (None, None, 0) and a[11] == out["loss"].data_ptr()
    assert all(type(v) is int for v in a[3:6]) and type(a[10]) is int


def test_train_search_marshalling():
    d, eng = data(), recording_engine()
    R, n, m = 2, 5, 4
    st = eng.lbfgs_state(R * D, n, m)
    x0 = torch.full((R, D, n), 0.5, dtype=torch.float64)
    best = eng.train_search(st, d["X"], d["Y"], d["lo"], d["hi"], 7, x0=x0, c1=1e-3, pgtol=1e-6, log_scale=False)
    (name, a), = eng.lib.calls
    lo_d, hi_d = [t for t in eng.converted if tuple(t.shape) == (D, n)][-2:]
    assert name == "gpmpc_train_search" and len(a) == len(L.SIGNATURES[name][1])
    assert a[1:] == (d["X"].data_ptr(), d["Y"].data_ptr(), 6, D, 3, R, lo_d.data_ptr(), hi_d.data_ptr(), 0, 0, 7, m, 1e-3, 1e-6,
                     x0.data_ptr(), st["buffer"].data_ptr(), best.data_ptr(), None)
    assert tuple(best.shape) == (D, 3 + n) and best.dtype == torch.float64
    assert all(type(v) is int for v in a[3:7] + a[9:13]) and type(a[13]) is float and type(a[14]) is float
    # a continued state: no starts, the first iteration by value
    eng.lib.calls.clear()
    eng.train_search(st, d["X"], d["Y"], d["lo"], d["hi"], 2, first_iteration=7, best_out=best)
    (name, a), = eng.lib.calls
    assert a[9:13] == (1, 7, 2, m) and a[15] is None and a[17] == best.data_ptr()
    # the one-synchronisation wrapper: one search on a state of its own, every result from one host copy
    eng.lib.calls.clear()
    res = eng.train_search_host(d["X"], d["Y"], x0.numpy(), d["lo"], d["hi"], 3, history=2)
    assert [c[0] for c in eng.lib.calls] == ["gpmpc_train_search"] and eng.lib.calls[0][1][10:13] == (0, 3, 2)
    assert {k: (v.shape, v.dtype) for k, v in res.items()} == {
        "theta": ((D, n), np.float64), "loss": ((D,), np.float64), "restart": ((D,), np.int64), "J": ((R, D), np.float64),
        "status": ((R, D), np.int64)}


def test_wrapper_errors():
    d, eng = data(), recording_engine()
    X, Y, prm, lo, hi = d["X"], d["Y"], d["params"], d["lo"], d["hi"]
    bad = [dict(lo=lo), dict(hi=hi), dict(lo=hi, hi=lo), dict(lo=-lo, hi=hi), dict(lo=0 * lo, hi=hi), dict(lo=lo[:1], hi=hi[:1]),
           dict(lo=lo[:, :2], hi=hi[:, :2])]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.mll_batch(X, Y, prm, **kw)
    eng.mll_batch(X, Y, prm, lo=0 * lo, hi=hi, log_scale=False)      # a zero lower bound is fine under the linear map
    for args in ((X, Y, prm[:, :, :3]), (X, Y, prm[0]), (X, Y[:4], prm), (X[0], Y, prm), (X, Y[:, 0], prm)):
        with pytest.raises(ValueError):
            eng.mll_batch(*args)
    st = eng.lbfgs_state(2 * D, 5, 3)
    x0 = np.full((2, D, 5), 0.5)
    for kw in (dict(lo=None, hi=None), dict(lo=lo, hi=None), dict(lo=hi, hi=lo), dict(lo=-lo, hi=hi), dict(x0=x0[:1]),
               dict(x0=x0[:, :, :4])):
        args = dict(lo=lo, hi=hi, x0=x0)
        args.update(kw)
        with pytest.raises(ValueError):
            eng.train_search(st, X, Y, args["lo"], args["hi"], 3, x0=args["x0"])
    with pytest.raises(ValueError):
        eng.train_search(eng.lbfgs_state(2 * D + 1, 5, 3), X, Y, lo, hi, 3, x0=x0)      # not a whole number of restarts
    with pytest.raises(ValueError):
        eng.train_search(eng.lbfgs_state(2 * D, 6, 3), X, Y, lo, hi, 3, x0=x0)          # another number of coordinates
    with pytest.raises(ValueError):
        eng.train_search_host(X, Y, x0[0], lo, hi, 3)
    assert not [c for c in eng.lib.calls if c[0] == "gpmpc_train_search"]
