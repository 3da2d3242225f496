"""Tier 2 (GPU): gpmpc_rollout_linear_feedback_backward, HipEngine.rollout_linear_feedback_backward and
HipEngine.rollout_linear_feedback_grad -- the vector-Jacobian product of the closed-loop linearised rollout with its costs, wrt
the actions, the gains and the initial state.

Checked against torch autograd of the fp64 restatement (tests/feedback_rollout_torch_ref.py) to the project's gradient bound, 1e-7
of the largest magnitude of EACH output array (gains_bar on its own scale: it is ~1e-3 beside S0_bar at ~50); against central
differences of gpmpc_rollout_linear_feedback's own objective over every action and every gain entry; and against the contracts of
include/gpmpc.h: bitwise batch / chunk / gain-layout invariance, NULL = zero cotangents, NULL outputs, exact symmetry, NULL gains =
gpmpc_rollout_linear_backward, errors, no interference.
"""
import numpy as np
import pytest
import torch

import feedback_rollout_torch_ref as fbt
import linear_moments_ref as lin
from oracle import synth

pytestmark = pytest.mark.gpu
TOL = 1e-7
KEYS = ("actions_bar", "gains_bar", "mu0_bar", "S0_bar")


@pytest.fixture(scope="module")
def engine():
    import gp_mpc_amd
    eng = gp_mpc_amd.HipEngine(0)
    yield eng
    eng.close()


def _np(t):
    return t.cpu().numpy()


def _workload(N, H, B, time, seed, D=3, A=1):
    # the recipe of tests/test_gpu_rollout_linear_backward.py
    w = synth.make_workload(N, D, A, H, B, include_time=time, seed=seed, time0=3.0, dynamics="contracting", dense_s0=0.02)
    w.kappa = 2.0
    return w


def _gains(w, seed):
    N, D, A, E, H, B = w.dims
    return np.random.default_rng(seed).standard_normal((B, H, A, D))


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
    rel = err / scale if scale > 0 else 0.0
    worst[what[0]] = max(worst.get(what[0], 0.0), rel)
    assert err <= TOL * scale, (what, err, scale)


def _parity(engine, w, K, worst, batches=(1, 4, 70)):
    N, D, A, E, H, B = w.dims
    args = (w.mu0, w.S0, w.include_time, w.time0)
    seeds = _seeds(w, 601)
    smin, smax = np.full(D, 0.05), np.full(D, 0.9)
    for mode in ("J", "all", "constraints"):
        cons = (smin, smax) if mode == "constraints" else (None, None)
        fa = _prepared(engine, w, False, *cons)
        cfg = lin.reward_config_of(w, False, *cons)
        bars = dict(J_bar=np.ones(B)) if mode == "J" else seeds
        want = fbt.rollout_vjp(fa, cfg, w.actions, K, *args, **bars)
        assert np.max(np.abs(want[1])) > 0
        for Bs in batches:
            sub = {k: v[:Bs] for k, v in bars.items()}
            out = engine.rollout_linear_feedback_backward(w.actions[:Bs], K[:Bs], *args, **sub)
            assert set(out) == set(KEYS)
            for k, x in zip(KEYS, want):
                _check(_np(out[k]), x[:Bs], (k, mode, Bs), worst)
            assert torch.equal(out["S0_bar"], out["S0_bar"].transpose(1, 2))
    engine.set_cost(w.target, w.W, w.W_T, w.kappa)


def _report(what, worst):
    print(f"rollout_linear_feedback_backward {what}: worst error / scale per array = "
          + ", ".join(f"{k} {worst.get(k, 0.0):.3e}" for k in KEYS))


# N: 50 (one partial column block), 300 (two); B: 1, 4, 70 (two row tiles); H: 1, 3; per-candidate gains of scale 1
@pytest.mark.parametrize("time", [False, True])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("N", [50, 300])
def test_parity_with_autograd(engine, N, H, time):
    w = _workload(N, H, 70, time, seed=600 + N + H)
    worst = {}
    _parity(engine, w, _gains(w, 602), worst)
    _report(f"N={N} H={H} time={time}", worst)


def test_parity_two_actions_four_states(engine):
    """D = 4, A = 2: the order of K_t^T V_u and the layout of gains_bar."""
    w = _workload(50, 3, 5, False, seed=610, D=4, A=2)
    worst = {}
    _parity(engine, w, _gains(w, 611), worst, batches=(5,))
    _report("D=4 A=2", worst)


def test_parity_nine_inputs(engine):
    """D = 6, A = 2 with time: E = 9, the EP = 16 instantiation of the tile kernel."""
    w = _workload(50, 2, 2, True, seed=612, D=6, A=2)
    worst = {}
    _parity(engine, w, _gains(w, 613), worst, batches=(2,))
    _report("D=6 A=2 time", worst)


@pytest.mark.parametrize("layout", ["steps", "one"])
def test_parity_shared_gain_layouts(engine, layout):
    """(H, A, D) and (A, D) gains: gains_bar stays per candidate and per step, and reduces to the shared gain's gradient."""
    w = _workload(50, 3, 4, True, seed=614)
    N, D, A, E, H, B = w.dims
    fa = _prepared(engine, w)
    rng = np.random.default_rng(615)
    K = rng.standard_normal((H, A, D)) if layout == "steps" else rng.standard_normal((A, D))
    args = (w.mu0, w.S0, w.include_time, w.time0)
    seeds = _seeds(w, 616)
    want = fbt.rollout_vjp(fa, lin.reward_config_of(w), w.actions, K, *args, **seeds)      # of the gains broadcast to (B, H, A, D)
    out = engine.rollout_linear_feedback_backward(w.actions, K, *args, **seeds)
    worst = {}
    assert out["gains_bar"].shape == (B, H, A, D)
    for k, x in zip(KEYS, want):
        _check(_np(out[k]), x, (k, layout), worst)
    # ... the same bits as the same gains given per candidate
    full = engine.rollout_linear_feedback_backward(w.actions, np.broadcast_to(K, (B, H, A, D)).copy(), *args, **seeds)
    for k in KEYS:
        assert torch.equal(out[k], full[k]), k
    # the shared gain's own gradient, by autograd through the broadcast
    Kt = torch.tensor(K, requires_grad=True)
    ft = fbt.factors_t(fa)
    at = fbt._t(w.actions)
    mu, Sig = fbt.rollout(*ft, at, Kt.expand(B, H, A, D), fbt._t(w.mu0).expand(B, -1), fbt._t(w.S0).expand(B, -1, -1),
                          w.include_time, w.time0)
    cm, cv, J = fbt.costs(lin.reward_config_of(w), mu, Sig, at, Kt.expand(B, H, A, D))
    obj = sum(torch.sum(fbt._t(seeds[n]) * v) for n, v in (("mu_bar", mu), ("Sig_bar", Sig), ("cost_mu_bar", cm),
                                                             ("cost_var_bar", cv), ("J_bar", J)))
    shared = torch.autograd.grad(obj, Kt)[0].numpy()
    axes = 0 if layout == "steps" else (0, 1)
    reduced = _np(out["gains_bar"]).sum(axis=axes)
    # each term is held to TOL of the per-candidate array's scale; the sum to TOL of the largest sum of magnitudes
    assert np.max(np.abs(reduced - shared)) <= TOL * np.max(np.abs(want[1]).sum(axis=axes)), layout
    _report(f"gain layout {layout}", worst)


def test_clip_is_pass_through(engine):
    w = _workload(50, 3, 4, False, seed=625)
    w.kappa = 19.0                                                              # cost_mu / sqrt(cost_var) spans 16 .. 24 here
    K = _gains(w, 626)
    fa = _prepared(engine, w, True)
    try:
        plain = engine.rollout_linear_feedback(w.actions, K, w.mu0, w.S0)
        ucb = -plain["cost_mu"] + w.kappa * torch.sqrt(plain["cost_var"])
        assert torch.any(ucb > 0) and torch.any(ucb < 0)                        # the clip bites in some steps ...
        got = engine.rollout_linear_feedback_grad(w.actions, K, w.mu0, w.S0)
        want = fbt.rollout_vjp(fa, lin.reward_config_of(w, True), w.actions, K, w.mu0, w.S0, J_bar=np.ones(4))
        worst = {}
        _check(_np(got["grad"]), want[0], ("actions_bar",), worst)
        _check(_np(got["gains_grad"]), want[1], ("gains_bar",), worst)
    finally:
        engine.set_cost(w.target, w.W, w.W_T, w.kappa)
    unclipped = engine.rollout_linear_feedback_grad(w.actions, K, w.mu0, w.S0)
    assert not torch.equal(unclipped["J"], got["J"])                            # ... changes the value ...
    assert torch.equal(unclipped["grad"], got["grad"])                          # ... and no gradient
    assert torch.equal(unclipped["gains_grad"], got["gains_grad"])


def test_grad_is_forward_then_backward(engine):
    w = _workload(50, 3, 4, True, seed=627)
    K = _gains(w, 628)
    _prepared(engine, w)
    args = (w.mu0, w.S0, w.include_time, w.time0)
    got = engine.rollout_linear_feedback_grad(w.actions, K, *args)
    assert set(got) == {"J", "grad", "gains_grad"}
    assert torch.equal(got["J"], engine.rollout_linear_feedback(w.actions, K, *args)["J"])
    back = engine.rollout_linear_feedback_backward(w.actions, K, *args, J_bar=np.ones(4), want_initial=False)
    assert set(back) == {"actions_bar", "gains_bar"}
    assert torch.equal(back["actions_bar"], got["grad"]) and torch.equal(back["gains_bar"], got["gains_grad"])


def test_gradient_against_central_differences(engine):
    """Central differences of gpmpc_rollout_linear_feedback's own J over every action and every gain entry, step 1e-4.  The bound
    is 10 x the larger of the two truncation figures of the fp64 numpy forward at this very case (measured and held by
    tests/test_feedback_backward_reference.py: 3.6e-6 for the actions, 3.4e-10 for the gains), the factor for the reordering noise
    of the device's fp64 J."""
    w, K = fbt.fd_workload()
    N, D, A, E, H, B = w.dims
    _prepared(engine, w)
    got = engine.rollout_linear_feedback_grad(w.actions, K, w.mu0, w.S0)
    h = fbt.FD_STEP
    na, nk = H * A, H * A * D
    acts = np.repeat(w.actions, 2 * (na + nk), axis=0)           # rows 2 i, 2 i + 1: +h / -h in coordinate i
    gains = np.repeat(K, 2 * (na + nk), axis=0)
    for i in range(na):
        acts[2 * i].reshape(-1)[i] += h
        acts[2 * i + 1].reshape(-1)[i] -= h
    for i in range(nk):
        gains[2 * (na + i)].reshape(-1)[i] += h
        gains[2 * (na + i) + 1].reshape(-1)[i] -= h
    J = _np(engine.rollout_linear_feedback(acts, gains, w.mu0, w.S0, trajectories=False, stage_costs=False,
                                           out={"J": torch.empty(len(acts), dtype=torch.float64, device=engine.device)})["J"])
    fd = (J[0::2] - J[1::2]) / (2 * h)
    bound = 10.0 * max(fbt.FD_CPU_DISCREPANCY.values())
    for which, d, g in (("actions", fd[:na], _np(got["grad"]).reshape(-1)), ("gains", fd[na:], _np(got["gains_grad"]).reshape(-1))):
        fig = float(np.max(np.abs(d - g)) / np.max(np.abs(d)))
        print(f"central differences, step {h:g}, {which}: relative discrepancy {fig:.3e} (bound {bound:.3e})")
        assert fig <= bound, (which, fig, d, g)


@pytest.mark.parametrize("N,time", [(50, True), (300, False)])
def test_bits(engine, N, time):
    w = _workload(N, 3, 70, time, seed=630 + N)
    K = _gains(w, 632)
    _prepared(engine, w)
    seeds = _seeds(w, 631)
    args = (w.mu0, w.S0, w.include_time, w.time0)

    def run(idx, gains=K, flags=None, **kw):
        sel = {k: (v[idx] if v is not None else None) for k, v in {**seeds, **kw}.items()}
        g = gains[idx] if gains is not None and gains.ndim == 4 else gains
        return engine.rollout_linear_feedback_backward(w.actions[idx], g, *args, **sel, **(flags or {}))
    everything = np.arange(70)
    full = run(everything)
    for k in KEYS:
        assert torch.equal(run(everything)[k], full[k]), k
        for i in (0, 63, 64, 69):
            assert torch.equal(run(np.array([i]))[k][0], full[k][i]), (k, i)
        assert torch.equal(run(everything[::-1].copy())[k], full[k].flip(0)), k
    assert torch.equal(full["S0_bar"], full["S0_bar"].transpose(1, 2))
    for chunk in (1, 64):
        engine.set_option("moments_linear_backward_chunk_points", chunk)
        try:
            chunked = run(everything)
            shared_chunked = run(everything, gains=K[0])
        finally:
            engine.set_option("moments_linear_backward_chunk_points", 0)
        for k in KEYS:
            assert torch.equal(chunked[k], full[k]), (k, chunk)
    for name in seeds:                                           # a NULL cotangent and an all-zero one
        a = run(everything, **{name: None})
        b = run(everything, **{name: np.zeros_like(seeds[name])})
        for k in KEYS:
            assert torch.equal(a[k], b[k]), (name, k)
    # shared gains give the bits of the same gains per candidate (also across chunks: the gain pointer is not offset)
    shared = run(everything, gains=K[0])
    tiled = run(everything, gains=np.broadcast_to(K[0], K.shape).copy())
    for k in KEYS:
        assert torch.equal(shared[k], tiled[k]) and torch.equal(shared_chunked[k], tiled[k]), k
    # NULL outputs leave the others' bits
    no_gains = run(everything, flags=dict(want_gains=False))
    no_init = run(everything, flags=dict(want_initial=False))
    assert set(no_gains) == {"actions_bar", "mu0_bar", "S0_bar"} and set(no_init) == {"actions_bar", "gains_bar"}
    for out in (no_gains, no_init):
        for k in out:
            assert torch.equal(out[k], full[k]), k
    # NULL gains: gpmpc_rollout_linear_backward's bits
    sel = {k: v for k, v in seeds.items()}
    open_loop = engine.rollout_linear_backward(w.actions, *args, **sel)
    null = run(everything, gains=None)
    assert set(null) == set(open_loop)
    for k in open_loop:
        assert torch.equal(null[k], open_loop[k]), k
    # ... while at zero gains the gains still have a gradient
    assert torch.any(run(everything, gains=np.zeros_like(K))["gains_bar"] != 0)


def test_errors_and_no_interference():
    import gp_mpc_amd
    from gp_mpc_amd import _lib as L
    eng = gp_mpc_amd.HipEngine(0)
    try:
        w = _workload(50, 3, 4, False, seed=640)
        K = _gains(w, 641)
        acts, gains = eng._dev(w.actions), eng._dev(K)
        mu0, S0 = np.ascontiguousarray(w.mu0), np.ascontiguousarray(w.S0)
        mu_bar = torch.ones((4, 4, 3), dtype=torch.float64, device=eng.device)
        J_bar = torch.ones(4, dtype=torch.float64, device=eng.device)
        cm_bar = torch.ones((4, 4), dtype=torch.float64, device=eng.device)
        a_bar = torch.empty((4, 3, 1), dtype=torch.float64, device=eng.device)
        K_bar = torch.empty((4, 3, 1, 3), dtype=torch.float64, device=eng.device)
        hp = lambda a: a.ctypes.data                                        # noqa: E731

        def call(B=4, H=3, A=1, time=0, actions=acts.data_ptr(), g=gains.data_ptr(), m0=hp(mu0), mub=mu_bar.data_ptr(), cmb=None,
                 cvb=None, Jb=None, out=a_bar.data_ptr(), gout=K_bar.data_ptr()):
            return eng.lib.gpmpc_rollout_linear_feedback_backward(eng._h, actions, g, 1, m0, hp(S0), B, H, A, time, 0.0, mub, None,
                                                                  cmb, cvb, Jb, out, gout, None, None, eng._stream())
        assert call() == L.GPMPC_ERR_ARG and "prepare" in eng.lib.gpmpc_last_error(eng._h).decode()     # no cached model
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        assert call() == L.GPMPC_OK                                          # trajectory cotangents need no cost settings
        assert call(gout=None) == L.GPMPC_OK
        for kw in (dict(Jb=J_bar.data_ptr()), dict(cmb=cm_bar.data_ptr()), dict(cvb=cm_bar.data_ptr())):
            assert call(**kw) == L.GPMPC_ERR_ARG and "set_cost" in eng.lib.gpmpc_last_error(eng._h).decode(), kw
        for kw in (dict(out=None), dict(g=None), dict(A=0), dict(B=0), dict(H=0), dict(A=2), dict(time=1), dict(actions=None),
                   dict(m0=None)):
            assert call(**kw) == L.GPMPC_ERR_ARG, kw
        assert call(g=None, gout=None) == L.GPMPC_OK                         # gpmpc_rollout_linear_backward
        with pytest.raises(RuntimeError) as ei:
            eng.rollout_linear_feedback_grad(w.actions, K, w.mu0, w.S0)
        assert type(ei.value).__name__ == "GpmpcError" and ei.value.code == L.GPMPC_ERR_ARG
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        assert call(Jb=J_bar.data_ptr(), cmb=cm_bar.data_ptr()) == L.GPMPC_OK
        # no interference: the rollouts and the open-loop gradient give the same bits before and after, gpmpc_last_* stays
        seeds = _seeds(w, 642)

        def others():
            return [eng.rollout(w.actions, w.mu0, w.S0), eng.rollout_linear(w.actions, w.mu0, w.S0),
                    eng.rollout_linear_feedback(w.actions, K, w.mu0, w.S0),
                    eng.rollout_linear_backward(w.actions, w.mu0, w.S0, **seeds)]
        before = [{k: v.clone() for k, v in d.items()} for d in others()]
        state = (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode, eng.last_grad_path)
        out = eng.rollout_linear_feedback_grad(w.actions, K, w.mu0, w.S0)
        assert torch.all(torch.isfinite(out["grad"])) and torch.any(out["grad"]) and torch.any(out["gains_grad"])
        assert (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode, eng.last_grad_path) == state
        for b, a in zip(before, others()):
            for k in b:
                assert torch.equal(b[k], a[k]), k
    finally:
        eng.close()
