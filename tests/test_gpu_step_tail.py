"""The fixed tail of a step: the stage-cost / objective kernel (register form for D <= 4, A <= 2, generic form otherwise)
and the keep-the-best kernel that delivers the winner's record to pinned host memory (gpmpc_argmin_export).

Tolerances of the cost comparison: those tests/test_gpu_parity.py applies to the reference's rewards (1e-8 of max|reward|),
reward variances (1e-7, its default for the small memories) and objectives (1e-7).  The costs are compared on the mu / Sig the
rollout RETURNED, i.e. the cost arithmetic alone is under test; its own fp64 error is ~1e-13.  The bits of J, cost_mu and
cost_var are pinned against tests/golden/step_tail_costs.npz, written once by the build that preceded the register form
(tools/gen_step_tail_golden.py)."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from helpers import load, rel_err
from oracle import gpmpc_oracle as orc
import step_tail_cases as cases

gpu = pytest.mark.gpu

DS = [1, 2, 3, 4, 6]           # 6: generic fallback
AS = [1, 2, 3]                 # 3: generic fallback
HS = [1, 5, 63, 64, 70]        # H + 1 = 65, 71: the lanes take a second trip
BS = [1, 3, 300]


@pytest.fixture(scope="module")
def engine():
    import gp_mpc_amd
    eng = gp_mpc_amd.HipEngine(0)
    yield eng
    eng.close()


def _check_costs(engine, D, A, H, B, clip, cons, tim):
    w, smin, smax, out = cases.run_case(engine, D, A, H, B, clip, cons, tim)
    mu, Sig = out["mu"].cpu().numpy(), out["Sig"].cpu().numpy()
    cm, cv = orc.stage_costs(mu, Sig, w.actions, w.target, w.W, w.W_T, smin, smax)
    J = orc.lcb_objective(cm, cv, w.kappa, clip)
    e_m = rel_err(out["cost_mu"].cpu().numpy(), cm)
    e_v = rel_err(out["cost_var"].cpu().numpy(), cv)
    e_J = rel_err(out["J"].cpu().numpy(), J)
    tag = (D, A, H, B, clip, cons, tim)
    print(f"costs {tag}: cost_mu {e_m:.2e} cost_var {e_v:.2e} J {e_J:.2e}")
    assert np.all(np.isfinite(J)), tag
    assert e_m < 1e-8, (tag, e_m)
    assert e_v < 1e-7, (tag, e_v)
    assert e_J < 1e-7, (tag, e_J)


@gpu
@pytest.mark.parametrize("D,A", list(itertools.product(DS, AS)))
def test_costs_match_reward_mapper(engine, D, A):
    """Every (H, B) of the grid per (D, A); clip and the state constraints cycle through their four combinations, shifted
    per (D, A), so every shape class meets every combination."""
    for k, (H, B) in enumerate(itertools.product(HS, BS)):
        mode = (k + D + 2 * A) % 4
        _check_costs(engine, D, A, H, B, clip=bool(mode & 1), cons=bool(mode & 2), tim=False)


@gpu
@pytest.mark.parametrize("D,A,H,B", [(3, 1, 5, 3), (4, 2, 64, 3), (6, 3, 5, 3)])
def test_costs_with_time_input(engine, D, A, H, B):
    _check_costs(engine, D, A, H, B, clip=True, cons=True, tim=True)


@gpu
def test_cost_bits_pinned(engine):
    g = load("step_tail_costs")
    assert [tuple(int(v) for v in c) for c in g["cases"]] == [tuple(int(v) for v in c) for c in cases.GOLDEN_CASES]
    for k, (D, A, H, B, clip, cons, tim) in enumerate(cases.GOLDEN_CASES):
        w, _, _, out = cases.run_case(engine, D, A, H, B, clip, cons, tim)
        assert int(g[f"seed_{k}"]) == cases.case_seed(D, A, H, B)
        assert float(g[f"actions_sum_{k}"]) == float(w.actions.sum())           # same inputs
        for name in ("J", "cost_mu", "cost_var"):
            got = out[name].cpu().numpy()
            assert got.shape == g[f"{name}_{k}"].shape
            assert np.array_equal(got, g[f"{name}_{k}"]), (k, name, float(np.max(np.abs(got - g[f"{name}_{k}"]))))


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.int64)


def _export_variants(B, rng):
    """(label, J, first, with_actions)"""
    base = rng.uniform(1.0, 2.0, size=B)
    yield "plain", base.copy(), 0, True
    yield "first>0", base.copy(), 4096, True
    tie = base.copy()
    tie[[B // 3, B - 1]] = 0.5
    tie[B // 2] = 0.5
    yield "ties", tie, 0, True
    n0 = base.copy()
    n0[0] = np.nan
    yield "nan in slot 0", n0, 0, True
    yield "nan in slot 0, first>0", n0.copy(), 7, True        # not the GLOBAL slot 0: never selected
    ne = base.copy()
    ne[int(np.argmin(ne))] = np.nan
    ne[B - 1] = np.nan
    yield "nan elsewhere", ne, 0, True
    yield "all nan", np.full(B, np.nan), 3, True
    yield "all nan from slot 0", np.full(B, np.nan), 0, True
    yield "no actions", base.copy(), 11, False


@gpu
@pytest.mark.parametrize("B", [1, 64, 65, 257, 1500])
def test_export_record_equals_device_record(engine, B):
    import torch
    rng = np.random.default_rng(B)
    H, A = 5, 2
    acts = torch.as_tensor(rng.uniform(size=(B, H, A)), device=engine.device)
    for label, J, first, with_actions in _export_variants(B, rng):
        Jd = torch.as_tensor(J, device=engine.device)
        a = acts if with_actions else None
        n = 2 + (H * A if with_actions else 0)
        host = torch.full((n,), -7.0, dtype=torch.float64).pin_memory()
        dev = engine.argmin_async(Jd, first_global_index=first, actions=a, host_out=host)
        old = engine.argmin_async(Jd, first_global_index=first, actions=a)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(host), _bits(dev)), (label, host, dev)
        assert np.array_equal(_bits(old), _bits(dev)), (label, old, dev)
        # the rule itself (gp_mpc_controller.py:146-148 with the shard offset)
        want = -1
        for i, v in enumerate(J):
            if (first + i == 0 and np.isnan(v)):
                want = 0
                break
            if v < (math.inf if want < 0 else J[want]):
                want = i
        rec = host.numpy()
        if want < 0:
            assert rec[0] == math.inf and rec[1] == -1.0, (label, rec[:2])
        else:
            assert rec[1] == float(first + want), (label, rec[1], want)
            assert np.array_equal(rec[:1].view(np.int64), J[want:want + 1].view(np.int64)), label
            if with_actions:
                assert np.array_equal(rec[2:], acts[want].reshape(-1).cpu().numpy()), label


@gpu
def test_export_rejects_memory_that_is_not_pinned(engine):
    import torch
    Jd = torch.as_tensor(np.array([3.0, 1.0, 2.0]), device=engine.device)
    out = torch.empty(2, dtype=torch.float64, device=engine.device)
    with pytest.raises(ValueError):
        engine.argmin_async(Jd, host_out=torch.empty(2, dtype=torch.float64))
    with pytest.raises(ValueError):
        engine.argmin_async(Jd, host_out=torch.empty(3, dtype=torch.float64).pin_memory())       # wrong length
    # the library's own check, below the Python one: pageable host memory and device memory are argument errors
    pageable = np.zeros(2)
    device_mem = torch.zeros(2, dtype=torch.float64, device=engine.device)
    for ptr in (pageable.ctypes.data, device_mem.data_ptr()):
        rc = engine.lib.gpmpc_argmin_export(engine._h, Jd.data_ptr(), 3, 0, None, 0, out.data_ptr(), C.c_void_p(ptr),
                                            engine._stream())
        assert rc == -1, rc
    torch.cuda.synchronize()
    assert np.array_equal(pageable, np.zeros(2)) and torch.equal(device_mem.cpu(), torch.zeros(2, dtype=torch.float64))
    # and the engine is still usable
    assert engine.argmin(Jd)[1] == 1


@gpu
def test_pipelined_ring_matches_blocking_selection(engine):
    """50 steps as bench.py's launch / result ring runs them: two pinned slots and device records, the winner read one step
    late, the candidates changed every step.  Every step's winner == select_best_on_device on the same inputs."""
    import torch
    from gp_mpc_amd import sharding
    steps, B = 50, 40
    w, _, _ = cases.make_case(3, 1, 5, B)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    engine.set_cost(w.target, w.W, w.W_T, w.kappa)
    gen = torch.Generator().manual_seed(5)
    acts = [torch.rand((B, 5, 1), generator=gen, dtype=torch.float64).to(engine.device) for _ in range(steps)]
    bufs = {"out": None}
    pinned, records = [None, None], [None, None]

    def launch(k):
        out = bufs["out"] = engine.rollout(acts[k], w.mu0, w.S0, out=bufs["out"])
        slot = k % 2
        pend = sharding.select_best_async(engine, out["J"], acts[k], 0, B, host_buffer=pinned[slot], record=records[slot])
        if pinned[slot] is not None:
            assert pend.host is pinned[slot] and pend.record is records[slot]      # the ring's buffers are reused
        pinned[slot], records[slot] = pend.host, pend.record
        return pend

    got, inflight = [], []
    for k in range(steps):
        inflight.append(launch(k))
        if len(inflight) > 1:
            got.append(inflight.pop(0).result())
    got.append(inflight.pop(0).result())
    assert pinned[0].is_pinned() and pinned[1].is_pinned()
    winners = set()
    for k in range(steps):
        out = engine.rollout(acts[k], w.mu0, w.S0)
        J0, i0, a0 = sharding.select_best_on_device(engine, out["J"], acts[k], 0, B)
        J1, i1, a1 = got[k]
        assert (J0, i0) == (J1, i1) and torch.equal(a0, a1), (k, J0, i0, J1, i1)
        winners.add(i0)
    assert len(winners) > 5          # the steps really had different winners


class _PlainEngine:
    """An engine WITHOUT the export capability (no `argmin_exports_host`, no `host_out` parameter)."""

    def __init__(self):
        self.calls = 0

    def argmin_async(self, J, first_global_index=0, actions=None, out=None):
        import torch
        self.calls += 1
        J = np.asarray(J, dtype=np.float64)
        best = orc.first_wins_argmin(J) if first_global_index == 0 else (int(np.nanargmin(J)) if np.any(J == J) else None)
        rec = torch.zeros(2 + int(actions[0].numel()), dtype=torch.float64) if out is None else out
        rec[0] = math.inf if best is None else float(J[best])
        rec[1] = -1.0 if best is None else float(first_global_index + best)
        if best is not None:
            rec[2:] = actions[best].reshape(-1)
        return rec


class _FlaggedEngine(_PlainEngine):
    """Claims the capability; on HOST tensors select_best_async must still not ask for an export."""
    argmin_exports_host = True

    def argmin_async(self, J, first_global_index=0, actions=None, out=None, host_out=None):
        assert host_out is None
        return super().argmin_async(J, first_global_index, actions, out)


@pytest.mark.parametrize("make", [_PlainEngine, _FlaggedEngine])
def test_engine_without_export_takes_the_copy_path(make):
    import torch
    from gp_mpc_amd import sharding
    rng = np.random.default_rng(2)
    J = rng.uniform(size=9)
    J[[4, 6]] = -1.0
    acts = torch.as_tensor(rng.uniform(size=(9, 3, 2)))
    eng = make()
    pend = sharding.select_best_async(eng, torch.as_tensor(J), acts, 0, 9)
    bJ, bi, win = pend.result()
    assert eng.calls == 1 and (bJ, bi) == (-1.0, 4) and torch.equal(win, acts[4])
    assert pend.event is None and pend.record is not None
    again = sharding.select_best_async(eng, torch.as_tensor(J), acts, 20, 9, record=pend.record)
    assert again.result()[1] == 24 and again.record is pend.record
    from stub_engine import OracleEngine
    assert not hasattr(OracleEngine, "argmin_exports_host")          # the stub engines of the CPU tests keep today's path
