"""CPU tests of the capped GP memory (MemoryConfig.max_points_model): the sliding window in Memory.prepare_for_model, the evicted
positions it exposes, and the controller handing them to the model's `forget` before `prepare_inference`.  No GPU: the engine
is the CPU stand-in of tests/stub_engine.py with a `forget` added here."""
import numpy as np
import pytest
import torch

from helpers import load, make_controller
from oracle import gpmpc_oracle as orc
from oracle import synth
from stub_engine import OracleEngine


def _replay(g, cfg, every=None):
    """The seeded stream of a memory_trace golden through a Memory with `cfg`; yields the memory after every prepare_for_model."""
    from gp_mpc_amd.control_objects.memories.gp_memory import Memory
    D, A, it = int(g["D"]), int(g["A"]), bool(g["include_time"])
    mem = Memory(cfg, dim_input=D + A + int(it), dim_state=D, include_time_model=it)
    t = lambda v: torch.tensor(v, dtype=torch.float64)   # noqa: E731
    every = int(g["prepare_every"]) if every is None else every
    for k in range(len(g["states"])):
        mem.add(t(g["states"][k]), t(g["actions"][k]), t(g["states_next"][k]), float(g["rewards"][k]), iter_ctrl=k,
                predicted_state=t(g["predicted"][k]) if g["has_pred"][k] else None,
                predicted_state_std=t(g["predicted_std"][k]) if g["has_std"][k] else None)
        if (k + 1) % every == 0:
            mem.prepare_for_model()
            yield mem


def _config(g, **kw):
    from gp_mpc_amd.config_classes import MemoryConfig
    return MemoryConfig(bool(g["check"]), list(g["thresholds_err"]), list(g["thresholds_std"]), points_batch_memory=16, **kw)


@pytest.mark.parametrize("name", ["memory_trace", "memory_trace_time", "memory_trace_nocheck"])
def test_no_cap_is_the_memory_of_the_reference_trace(name):
    """max_points_model=None (the default) and a config object from before the option existed: the recorded trace of the
    reference's Memory, byte for byte, and nothing ever evicted."""
    g = load(name)
    legacy = _config(g)
    del legacy.max_points_model
    for cfg in (_config(g), _config(g, max_points_model=None), legacy):
        assert getattr(cfg, "max_points_model", None) is None
        snaps = []
        for mem in _replay(g, cfg):
            x, y = mem.get()
            snaps.append((mem.len_mem_model, x.numpy().copy(), y.numpy().copy()))
            assert len(mem.pop_evicted()) == 0
        assert [s[0] for s in snaps] == list(g["snap_len"])
        assert snaps[0][1].tobytes() == g["snap_first_x"].tobytes() and snaps[0][2].tobytes() == g["snap_first_y"].tobytes()
        assert snaps[-1][1].tobytes() == g["final_x"].tobytes() and snaps[-1][2].tobytes() == g["final_y"].tobytes()
        n = len(g["states"])
        assert np.array_equal(mem.active_data_mask[:n], g["admitted"])
        assert mem.inputs[:n].numpy().tobytes() == g["inputs"].tobytes()
        assert mem.len_mem == int(g["len_mem"]) and mem.len_mem_last_processed == int(g["len_mem_last_processed"])


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("name", ["memory_trace", "memory_trace_time"])
def test_cap_keeps_a_sliding_window_of_the_newest_points(name, every):
    g = load(name)
    cap = max(1, int(g["snap_len"][-1]) // 3)     # a third of what the uncapped memory ends with
    free, capped = _replay(g, _config(g), every), _replay(g, _config(g, max_points_model=cap), every)
    held = None                                 # the memory as the consumer of pop_evicted last saw it
    evicted_total = 0
    for mf, mc in zip(free, capped):
        xf, yf = mf.get()
        xc, yc = mc.get()
        assert len(xc) <= cap and len(xc) == len(yc) == min(cap, len(xf))
        if mf.len_mem_model == 0:
            continue
        # the window: the newest points of the uncapped memory, in order, in contiguous storage
        assert torch.equal(xc, xf[len(xf) - len(xc):]) and torch.equal(yc, yf[len(yf) - len(yc):])
        assert xc.is_contiguous() and yc.is_contiguous()
        ev = mc.pop_evicted()
        # positions 0 .. k-1 of the memory as the consumer last saw it; that those ARE the evicted points is what the window
        # comparison above and the prefix comparison below pin
        assert len(ev) == max(0, mf.len_mem_model - cap) - evicted_total
        evicted_total += len(ev)
        if held is not None and len(ev) < len(held):
            assert torch.equal(xc[:len(held) - len(ev)], held[len(ev):])        # what is left of it is a prefix of the new one
        assert len(mc.pop_evicted()) == 0                                       # consumed once
        held = xc.clone()
        # the raw replay arrays and the admission mask do not notice the cap
        n = mf.len_mem
        assert torch.equal(mc.inputs[:n], mf.inputs[:n]) and torch.equal(mc.states_next[:n], mf.states_next[:n])
        assert np.array_equal(mc.active_data_mask[:n], mf.active_data_mask[:n]) and mc.len_mem == n
        assert mc.len_mem_last_processed == mf.len_mem_last_processed
    assert evicted_total > 0


def test_cap_must_be_positive():
    from gp_mpc_amd.config_classes import MemoryConfig
    for bad in (0, -3):
        with pytest.raises(ValueError):
            MemoryConfig(max_points_model=bad)
    assert MemoryConfig(max_points_model=5).max_points_model == 5 and MemoryConfig().max_points_model is None


def test_eviction_leaves_views_handed_out_earlier_alone():
    """get() hands out views (the model keeps them as x_mem / y_mem): an eviction must not shift rows under them."""
    from gp_mpc_amd.control_objects.memories.gp_memory import Memory
    from gp_mpc_amd.config_classes import MemoryConfig
    mem = Memory(MemoryConfig(check_errors_for_storage=False, points_batch_memory=4, max_points_model=3), dim_input=2, dim_state=1)
    s = lambda k: torch.tensor([float(k)], dtype=torch.float64)   # noqa: E731
    for k in range(3):
        mem.add(s(k), s(10 + k), s(k + 1), 0.0, iter_ctrl=k)
    mem.prepare_for_model()
    x_old = mem.get()[0]
    before = x_old.clone()
    for k in range(3, 5):
        mem.add(s(k), s(10 + k), s(k + 1), 0.0, iter_ctrl=k)
    mem.prepare_for_model()
    assert torch.equal(x_old, before)
    assert np.array_equal(mem.pop_evicted(), [0, 1]) and torch.equal(mem.get()[0][0], before[2])


class ForgettingEngine(OracleEngine):
    """The stand-in engine with `forget`, and a log of the calls that change the model."""
    last_prepare_mode = 0

    def __init__(self):
        super().__init__()
        self.log = []

    def prepare(self, X, Y, lengthscales, outputscales, noises):
        self.log.append(("prepare", np.asarray(X, dtype=np.float64).copy()))
        super().prepare(X, Y, lengthscales, outputscales, noises)

    def forget(self, indices):
        idx = np.asarray(indices).reshape(-1)
        self.log.append(("forget", idx.copy()))
        keep = np.setdiff1d(np.arange(len(self.f.X)), idx)
        self.f = orc.Factors(self.f.X[keep], self.f.Y[keep], self.f.lengthscales, self.f.variances, self.f.noises)


def test_controller_forgets_evicted_points_before_it_prepares():
    N, steps = 12, 6
    w = synth.make_workload(N=N, D=2, A=1, H=3, B=1, seed=6)
    eng = ForgettingEngine()
    c = make_controller(w, engine=eng, shard=False)
    c.memory.config.max_points_model = N
    c.memory.config.check_errors_for_storage = False
    m = c.transition_model
    np.random.seed(0)
    rng = np.random.default_rng(1)
    obs = w.mu0.copy()
    for s in range(steps):
        eng.log.clear()
        x_before = None if m.x_mem is None else np.asarray(m.x_mem).copy()
        a = c.get_action(obs)
        x_mem, y_mem = c.memory.get()
        assert len(x_mem) == N
        # what the model holds (and save_state ships) is the memory
        assert np.array_equal(np.asarray(m.x_mem), x_mem.numpy()) and np.array_equal(np.asarray(m.y_mem), y_mem.numpy())
        st = m.save_state()
        assert np.array_equal(np.asarray(st.inputs), x_mem.numpy())
        kinds = [k for k, _ in eng.log]
        if s == 0:
            assert kinds == ["prepare"]                    # nothing evicted yet
        else:
            # one point came in, the oldest went: forget([0]) first, then the prepare that appends
            assert kinds == ["forget", "prepare"], kinds
            assert np.array_equal(eng.log[0][1], [0])
            assert np.array_equal(eng.log[1][1][:N - 1], x_before[1:]) and np.array_equal(eng.log[1][1], x_mem.numpy())
            assert np.array_equal(eng.f.X, x_mem.numpy())
        obs_new = np.clip(obs + 0.05 * rng.standard_normal(obs.shape), 0.0, 1.0)
        c.add_memory(obs, a, obs_new, 0.0)
        obs = obs_new
    assert len(c.memory.pop_evicted()) == 0
    assert c.memory.len_mem == steps and c.memory.len_mem_model == N


def test_controller_prepares_in_full_where_the_engine_cannot_forget():
    """An engine without `forget` (the stand-in of stub_engine.py) and one whose `forget` reports GPMPC_ERR_ARG (no record to
    downdate from): a capped run goes on, each step a plain prepare of the window."""
    from gp_mpc_amd import GpmpcError, _lib

    class Refusing(ForgettingEngine):
        def forget(self, indices):
            self.log.append(("forget", np.asarray(indices).copy()))
            raise GpmpcError(_lib.GPMPC_ERR_ARG, "no record")

    class Failing(ForgettingEngine):
        def forget(self, indices):
            raise GpmpcError(_lib.GPMPC_ERR_HIP, "device lost")

    N = 12
    w = synth.make_workload(N=N, D=2, A=1, H=3, B=1, seed=6)
    t = lambda v: torch.as_tensor(np.asarray(v), dtype=torch.float64)   # noqa: E731
    for make in (OracleEngine, Refusing, Failing):
        eng = make()
        c = make_controller(w, engine=eng, shard=False)
        c.memory.config.max_points_model = N
        c.memory.config.check_errors_for_storage = False
        np.random.seed(0)
        c.get_action(w.mu0)
        c.memory.add(t(w.mu0), t([0.5]), t(w.mu0), 0.0, iter_ctrl=1)
        if make is Failing:                       # any other error is not swallowed
            with pytest.raises(GpmpcError):
                c.get_action(w.mu0)
            continue
        c.get_action(w.mu0)
        x_mem = c.memory.get()[0].numpy()
        assert len(x_mem) == N and np.array_equal(x_mem[:-1], w.X[1:])
        assert np.array_equal(eng.f.X, x_mem) and np.array_equal(np.asarray(c.transition_model.x_mem), x_mem)
        if make is Refusing:
            assert [k for k, _ in eng.log][-2:] == ["forget", "prepare"]


def test_controller_skips_forget_for_points_the_model_never_held():
    """A memory that overflows its cap before the first prepare: nothing to downdate, the prepare factorises the window."""
    N = 12
    w = synth.make_workload(N=N, D=2, A=1, H=3, B=1, seed=6)
    eng = ForgettingEngine()
    c = make_controller(w, engine=eng, shard=False)
    c.memory.config.max_points_model = N - 4
    c.memory.config.check_errors_for_storage = False
    np.random.seed(0)
    t = lambda v: torch.as_tensor(np.asarray(v), dtype=torch.float64)   # noqa: E731
    c.memory.add(t(w.mu0), t([0.5]), t(w.mu0), 0.0, iter_ctrl=0)
    c.get_action(w.mu0)
    assert [k for k, _ in eng.log] == ["prepare"] and len(eng.log[0][1]) == N - 4
    assert np.array_equal(eng.log[0][1][:-1], w.X[5:])
