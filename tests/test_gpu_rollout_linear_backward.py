"""Tier 2 (GPU): gpmpc_rollout_linear_backward and HipEngine.rollout_linear_grad -- the vector-Jacobian product of the linearised
rollout with its costs.

Checked against torch autograd of the fp64 restatement (tests/linear_moments_torch_ref.py) to the project's gradient bound, 1e-7
of the largest magnitude of each output array; against central differences of gpmpc_rollout_linear's own objective; and against
the contracts of include/gpmpc.h: bitwise batch / chunk invariance, NULL = zero cotangents, exact symmetry, errors, no
interference.
"""
import numpy as np
import pytest
import torch

import linear_moments_ref as lin
import linear_moments_torch_ref as ref
from oracle import synth

pytestmark = pytest.mark.gpu
TOL = 1e-7


@pytest.fixture(scope="module")
def engine():
    import gp_mpc_amd
    eng = gp_mpc_amd.HipEngine(0)
    yield eng
    eng.close()


def _np(t):
    return t.cpu().numpy()


def _workload(N, H, B, time, seed, D=3, A=1):
    w = synth.make_workload(N, D, A, H, B, include_time=time, seed=seed, time0=3.0, dynamics="contracting", dense_s0=0.02)
    w.kappa = 2.0
    return w


def _prepared(engine, w, clip=False, smin=None, smax=None):
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    engine.set_cost(w.target, w.W, w.W_T, w.kappa, clip, smin, smax)
    iK, beta = (_np(t) for t in engine.factors())
    return (w.X, w.lengthscales, w.outputscales, iK, beta)


def _seeds(w, seed):
    N, D, A, E, H, B = w.dims
    rng = np.random.default_rng(seed)
    return dict(mu_bar=rng.standard_normal((B, H + 1, D)), Sig_bar=rng.standard_normal((B, H + 1, D, D)),
                cost_mu_bar=rng.standard_normal((B, H + 1)), cost_var_bar=rng.standard_normal((B, H + 1)),
                J_bar=rng.uniform(0.5, 1.5, size=B))


def _check(got, want, what, worst):
    scale = float(np.max(np.abs(want)))
    err = float(np.max(np.abs(got - want)))
    worst[0] = max(worst[0], err / scale if scale > 0 else 0.0)
    assert err <= TOL * scale, (what, err, scale)


def _parity(engine, w, worst, batches=(1, 4, 70)):
    N, D, A, E, H, B = w.dims
    args = (w.mu0, w.S0, w.include_time, w.time0)
    seeds = _seeds(w, 501)
    smin, smax = np.full(D, 0.05), np.full(D, 0.9)
    for mode in ("J", "all", "constraints"):
        cons = (smin, smax) if mode == "constraints" else (None, None)
        fa = _prepared(engine, w, False, *cons)
        cfg = lin.reward_config_of(w, False, *cons)
        bars = dict(J_bar=np.ones(B)) if mode == "J" else seeds
        want = ref.rollout_vjp(fa, cfg, w.actions, *args, **bars)
        for Bs in batches:
            sub = {k: v[:Bs] for k, v in bars.items()}
            out = engine.rollout_linear_backward(w.actions[:Bs], *args, **sub)
            for k, x in zip(("actions_bar", "mu0_bar", "S0_bar"), want):
                _check(_np(out[k]), x[:Bs], (k, mode, Bs), worst)
            assert torch.equal(out["S0_bar"], out["S0_bar"].transpose(1, 2))
            bare = engine.rollout_linear_backward(w.actions[:Bs], *args, want_initial=False, **sub)      # mu0_bar / S0_bar NULL
            assert set(bare) == {"actions_bar"} and torch.equal(bare["actions_bar"], out["actions_bar"])
    engine.set_cost(w.target, w.W, w.W_T, w.kappa)


# N: 50 (one partial column block), 300 (two); B: 1, 4, 70 (two row tiles); H: 1, 3
@pytest.mark.parametrize("time", [False, True])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("N", [50, 300])
def test_parity_with_autograd(engine, N, H, time):
    w = _workload(N, H, 70, time, seed=500 + N + H)
    worst = [0.0]
    _parity(engine, w, worst)
    print(f"rollout_linear_backward N={N} H={H} time={time}: worst error / scale = {worst[0]:.3e}")


def test_parity_two_actions_four_states(engine):
    w = _workload(50, 3, 5, False, seed=510, D=4, A=2)
    worst = [0.0]
    _parity(engine, w, worst, batches=(5,))
    print(f"rollout_linear_backward D=4 A=2: worst error / scale = {worst[0]:.3e}")


def test_clip_is_pass_through(engine):
    w = _workload(50, 3, 4, False, seed=515)
    w.kappa = 10.0
    fa = _prepared(engine, w, True)
    try:
        plain = engine.rollout_linear(w.actions, w.mu0, w.S0)
        ucb = -plain["cost_mu"] + w.kappa * torch.sqrt(plain["cost_var"])
        assert torch.any(ucb > 0) and torch.any(ucb < 0)                        # the clip bites in some steps ...
        got = engine.rollout_linear_grad(w.actions, w.mu0, w.S0)
        want = ref.rollout_vjp(fa, lin.reward_config_of(w, True), w.actions, w.mu0, w.S0, J_bar=np.ones(4))
        worst = [0.0]
        _check(_np(got["grad"]), want[0], "grad", worst)
    finally:
        engine.set_cost(w.target, w.W, w.W_T, w.kappa)
    unclipped = engine.rollout_linear_grad(w.actions, w.mu0, w.S0)
    assert not torch.equal(unclipped["J"], got["J"])                            # ... changes the value ...
    assert torch.equal(unclipped["grad"], got["grad"])                          # ... and no gradient


def test_gradient_against_central_differences(engine):
    w = _workload(50, 3, 1, False, seed=520)
    _prepared(engine, w)
    got = engine.rollout_linear_grad(w.actions, w.mu0, w.S0)
    assert torch.equal(got["J"], engine.rollout_linear(w.actions, w.mu0, w.S0)["J"])
    back = engine.rollout_linear_backward(w.actions, w.mu0, w.S0, J_bar=np.ones(1), want_initial=False)
    assert torch.equal(back["actions_bar"], got["grad"])
    h = 1e-5
    pert = np.repeat(w.actions, 6, axis=0)                       # (2 H A, H, A): +h / -h in each coordinate
    for i in range(3):
        pert[2 * i, i, 0] += h
        pert[2 * i + 1, i, 0] -= h
    J = _np(engine.rollout_linear(pert, w.mu0, w.S0, trajectories=False, stage_costs=False,
                                  out={"J": torch.empty(6, dtype=torch.float64, device=engine.device)})["J"])
    fd = (J[0::2] - J[1::2]) / (2 * h)
    grad = _np(got["grad"])[0, :, 0]
    print("central differences", fd, "analytic", grad)
    assert np.max(np.abs(fd - grad)) <= 1e-5 * np.max(np.abs(fd))


@pytest.mark.parametrize("N,time", [(50, True), (300, False)])
def test_bits(engine, N, time):
    w = _workload(N, 3, 70, time, seed=530 + N)
    _prepared(engine, w)
    seeds = _seeds(w, 531)
    keys = ("actions_bar", "mu0_bar", "S0_bar")

    def run(idx, **kw):
        sel = {k: (v[idx] if v is not None else None) for k, v in {**seeds, **kw}.items()}
        return engine.rollout_linear_backward(w.actions[idx], w.mu0, w.S0, w.include_time, w.time0, **sel)
    everything = np.arange(70)
    full = run(everything)
    for k in keys:
        assert torch.equal(run(everything)[k], full[k]), k
        for i in (0, 63, 64, 69):
            assert torch.equal(run(np.array([i]))[k][0], full[k][i]), (k, i)
        assert torch.equal(run(everything[::-1].copy())[k], full[k].flip(0)), k
    assert torch.equal(full["S0_bar"], full["S0_bar"].transpose(1, 2))
    for chunk in (1, 64):
        engine.set_option("moments_linear_backward_chunk_points", chunk)
        try:
            chunked = run(everything)
        finally:
            engine.set_option("moments_linear_backward_chunk_points", 0)
        for k in keys:
            assert torch.equal(chunked[k], full[k]), (k, chunk)
    for name in seeds:                                           # a NULL cotangent and an all-zero one
        a = run(everything, **{name: None})
        b = run(everything, **{name: np.zeros_like(seeds[name])})
        for k in keys:
            assert torch.equal(a[k], b[k]), (name, k)


def test_errors_and_no_interference():
    import gp_mpc_amd
    from gp_mpc_amd import _lib as L
    eng = gp_mpc_amd.HipEngine(0)
    try:
        w = _workload(50, 3, 4, False, seed=540)
        acts = eng._dev(w.actions)
        mu0, S0 = np.ascontiguousarray(w.mu0), np.ascontiguousarray(w.S0)
        mu_bar = torch.ones((4, 4, 3), dtype=torch.float64, device=eng.device)
        J_bar = torch.ones(4, dtype=torch.float64, device=eng.device)
        cm_bar = torch.ones((4, 4), dtype=torch.float64, device=eng.device)
        a_bar = torch.empty((4, 3, 1), dtype=torch.float64, device=eng.device)
        hp = lambda a: a.ctypes.data                                        # noqa: E731

        def call(B=4, H=3, A=1, time=0, actions=acts.data_ptr(), m0=hp(mu0), mub=mu_bar.data_ptr(), cmb=None, cvb=None, Jb=None,
                 out=a_bar.data_ptr()):
            return eng.lib.gpmpc_rollout_linear_backward(eng._h, actions, m0, hp(S0), B, H, A, time, 0.0, mub, None, cmb, cvb, Jb,
                                                         out, None, None, eng._stream())
        assert call() == L.GPMPC_ERR_ARG and "prepare" in eng.lib.gpmpc_last_error(eng._h).decode()     # no cached model
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        assert call() == L.GPMPC_OK                                          # trajectory cotangents need no cost settings
        for kw in (dict(Jb=J_bar.data_ptr()), dict(cmb=cm_bar.data_ptr()), dict(cvb=cm_bar.data_ptr())):
            assert call(**kw) == L.GPMPC_ERR_ARG and "set_cost" in eng.lib.gpmpc_last_error(eng._h).decode(), kw
        for kw in (dict(out=None), dict(A=0), dict(B=0), dict(H=0), dict(A=2), dict(time=1), dict(actions=None), dict(m0=None)):
            assert call(**kw) == L.GPMPC_ERR_ARG, kw
        with pytest.raises(RuntimeError) as ei:
            eng.rollout_linear_grad(w.actions, w.mu0, w.S0)
        assert type(ei.value).__name__ == "GpmpcError" and ei.value.code == L.GPMPC_ERR_ARG
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        assert call(Jb=J_bar.data_ptr(), cmb=cm_bar.data_ptr()) == L.GPMPC_OK
        # no interference: both rollouts give the same bits before and after, the gpmpc_last_* state stays
        before = {k: v.clone() for k, v in eng.rollout(w.actions, w.mu0, w.S0).items()}
        before_lin = {k: v.clone() for k, v in eng.rollout_linear(w.actions, w.mu0, w.S0).items()}
        state = (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode, eng.last_grad_path)
        out = eng.rollout_linear_grad(w.actions, w.mu0, w.S0)
        assert torch.all(torch.isfinite(out["grad"])) and torch.any(out["grad"])
        assert (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode, eng.last_grad_path) == state
        after, after_lin = eng.rollout(w.actions, w.mu0, w.S0), eng.rollout_linear(w.actions, w.mu0, w.S0)
        for k in before:
            assert torch.equal(before[k], after[k]) and torch.equal(before_lin[k], after_lin[k]), k
    finally:
        eng.close()
