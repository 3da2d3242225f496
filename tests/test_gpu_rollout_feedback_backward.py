"""Tier 2 (GPU): gpmpc_rollout_feedback_backward, HipEngine.rollout_feedback_backward / rollout_feedback_grad and
GpStateTransitionModel.feedback_objective_and_gradient_batch -- the vector-Jacobian product of the closed-loop moment-matched
rollout with its costs, wrt the actions, the gains and the initial state.

Checked against torch autograd of the fp64 restatement (tests/feedback_mm_torch_ref.py, itself held to long-double central
differences and to the reference-autograd goldens by tests/test_feedback_mm_backward_reference.py) to the project's gradient
bound, 1e-7 of the largest magnitude of EACH output array (gains_bar lives on a far smaller scale than S0_bar); at zero gains
against gpmpc_rollout_backward; and against the contracts of include/gpmpc.h: bitwise batch / chunk / gain-layout invariance,
NULL = zero cotangents, NULL outputs, exact symmetry, errors, no interference.  There is no central-difference test here: fp64
differences of the forward's J are dominated by rounding (1e-6 .. 5e-3 of the directional derivative, worse as the step
shrinks); the long-double check on the CPU does that job.

Every parity test prints its worst error / scale per output array before it asserts.
"""
import numpy as np
import pytest
import torch

import feedback_mm_torch_ref as fmt
import linear_moments_ref as lin
from oracle import synth

pytestmark = pytest.mark.gpu
TOL = 1e-7
KEYS = ("actions_bar", "gains_bar", "mu0_bar", "S0_bar")
CHUNK = "rollout_feedback_backward_chunk_points"


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


def _report(what, worst):
    print(f"rollout_feedback_backward {what}: worst error / scale per array = "
          + ", ".join(f"{k} {worst.get(k, 0.0):.3e}" for k in KEYS))


def _parity(engine, w, K, worst, batches):
    """Three cotangent modes (J alone, all five, all five with constraints) against autograd of the restatement; the reference is
    computed once per mode for the largest batch and shared by the smaller ones (a candidate's gradients are its own)."""
    N, D, A, E, H, B = w.dims
    args = (w.mu0, w.S0, w.include_time, w.time0)
    seeds = _seeds(w, 801)
    smin, smax = np.full(D, 0.05), np.full(D, 0.9)
    for mode in ("J", "all", "constraints"):
        cons = (smin, smax) if mode == "constraints" else (None, None)
        fa = _prepared(engine, w, False, *cons)
        cfg = lin.reward_config_of(w, False, *cons)
        bars = dict(J_bar=np.ones(B)) if mode == "J" else seeds
        want = fmt.rollout_vjp(fa, cfg, w.actions, K, *args, **bars)
        assert np.max(np.abs(want[1])) > 0
        for Bs in batches:
            sub = {k: v[:Bs] for k, v in bars.items()}
            out = engine.rollout_feedback_backward(w.actions[:Bs], K[:Bs], *args, **sub)
            assert set(out) == set(KEYS)
            for k, x in zip(KEYS, want):
                _check(_np(out[k]), x[:Bs], (k, mode, Bs), worst)
            assert torch.equal(out["S0_bar"], out["S0_bar"].transpose(1, 2))
    engine.set_cost(w.target, w.W, w.W_T, w.kappa)


# -- 1. parity with autograd ---------------------------------------------------------------------------------------------------
# N = 50: one partial 64-row tile of the moment kernels; B: 1, 9 (across the pair pass's 8 points per workgroup), 70
@pytest.mark.parametrize("H", [1, 3])
def test_parity_with_autograd(engine, H):
    w = _workload(50, H, 70, False, seed=800 + H)
    worst = {}
    _parity(engine, w, _gains(w, 802), worst, batches=(1, 9, 70))
    _report(f"D=3 A=1 N=50 H={H}", worst)


def test_parity_two_actions_time_three_tiles(engine):
    """D = 3, A = 2 with time, N = 130: three row tiles with a ragged edge, the order of the action rows and the zero time row."""
    w = _workload(130, 4, 9, True, seed=810, A=2)
    worst = {}
    _parity(engine, w, _gains(w, 811), worst, batches=(9,))
    _report("D=3 A=2 time N=130 H=4", worst)


def test_parity_seven_inputs(engine):
    """D = 5, A = 2: E = 7, the next E instantiation of the gradient kernels."""
    w = _workload(50, 3, 2, False, seed=812, D=5, A=2)
    worst = {}
    _parity(engine, w, _gains(w, 813), worst, batches=(2,))
    _report("D=5 A=2 N=50 H=3", worst)


def test_parity_shared_gains(engine):
    """(H, A, D) gains: gains_bar stays per candidate and per step."""
    w = _workload(50, 3, 4, True, seed=814)
    N, D, A, E, H, B = w.dims
    fa = _prepared(engine, w)
    K = np.random.default_rng(815).standard_normal((H, A, D))
    args = (w.mu0, w.S0, w.include_time, w.time0)
    seeds = _seeds(w, 816)
    want = fmt.rollout_vjp(fa, lin.reward_config_of(w), w.actions, K, *args, **seeds)      # of the gains broadcast to (B, H, A, D)
    out = engine.rollout_feedback_backward(w.actions, K, *args, **seeds)
    worst = {}
    assert out["gains_bar"].shape == (B, H, A, D)
    for k, x in zip(KEYS, want):
        _check(_np(out[k]), x, (k, "shared"), worst)
    _report("shared (H, A, D) gains", worst)


# -- 2. zero gains -------------------------------------------------------------------------------------------------------------
def test_zero_gains_against_the_open_loop_gradient(engine):
    """At K = 0 the policy is the open loop: actions_bar, mu0_bar and S0_bar are gpmpc_rollout_backward's to 2e-7 of each maximum
    (both sides are held to 1e-7 of autograd), with explicit zero gains and with gains None; gains_bar is not zero."""
    w = _workload(50, 3, 9, True, seed=820)
    _prepared(engine, w)
    seeds = _seeds(w, 821)
    args = (w.mu0, w.S0, w.include_time, w.time0)
    open_loop = engine.rollout_backward(w.actions, *args, **seeds)
    zero = engine.rollout_feedback_backward(w.actions, np.zeros((9, 3, 1, 3)), *args, **seeds)
    none = engine.rollout_feedback_backward(w.actions, None, *args, **seeds)
    assert set(none) == {"actions_bar", "mu0_bar", "S0_bar"}
    for k in none:
        x = _np(open_loop[k])
        fig = float(np.max(np.abs(_np(zero[k]) - x)) / np.max(np.abs(x)))
        print(f"zero gains vs rollout_backward, {k}: {fig:.3e}")
        assert fig <= 2e-7, (k, fig)
        assert torch.equal(none[k], zero[k]), k                   # the zeroed workspace gains are zero gains
    assert bool(torch.any(zero["gains_bar"] != 0))


# -- 3. bitwise contracts ------------------------------------------------------------------------------------------------------
def test_bits(engine):
    w = _workload(50, 3, 70, True, seed=830)
    K = _gains(w, 832)
    _prepared(engine, w)
    seeds = _seeds(w, 831)
    args = (w.mu0, w.S0, w.include_time, w.time0)

    def run(idx, gains=K, flags=None, **kw):
        sel = {k: (v[idx] if v is not None else None) for k, v in {**seeds, **kw}.items()}
        g = gains[idx] if gains is not None and gains.ndim == 4 else gains
        return engine.rollout_feedback_backward(w.actions[idx], g, *args, **sel, **(flags or {}))
    everything = np.arange(70)
    full = run(everything)
    for k in KEYS:
        for i in (0, 69):                                         # alone; position 0 and the last position of B = 70
            assert torch.equal(run(np.array([i]))[k][0], full[k][i]), (k, i)
        assert torch.equal(run(everything[::-1].copy())[k], full[k].flip(0)), k
    assert torch.equal(full["S0_bar"], full["S0_bar"].transpose(1, 2))
    shared_chunked = None
    for chunk in (0, 1, 8):
        engine.set_option(CHUNK, chunk)
        try:
            chunked = run(everything)
            if chunk == 8:
                shared_chunked = run(everything, gains=K[0])
        finally:
            engine.set_option(CHUNK, 0)
        for k in KEYS:
            assert torch.equal(chunked[k], full[k]), (k, chunk)
    for name in ("moments_chunk_points", "moments_backward_chunk_points"):
        engine.set_option(name, 1)
        try:
            chunked = run(everything[:9])
        finally:
            engine.set_option(name, 0)
        for k in KEYS:
            assert torch.equal(chunked[k], full[k][:9]), (k, name)
    for name in seeds:                                           # a NULL cotangent and an all-zero one
        a = run(everything[:9], **{name: None})
        b = run(everything[:9], **{name: np.zeros_like(seeds[name])})
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


# -- 4. the engine's and the model's objective-and-gradient ----------------------------------------------------------------------
def test_grad_is_forward_then_backward_and_the_model_method(engine):
    from gp_mpc_amd.config_classes import ModelConfig
    from gp_mpc_amd.control_objects.models.gp_model import GpStateTransitionModel
    w = _workload(50, 3, 4, False, seed=840)
    N, D, A, E, H, B = w.dims
    K = _gains(w, 841)
    _prepared(engine, w)
    args = (w.mu0, w.S0, w.include_time, w.time0)
    got = engine.rollout_feedback_grad(w.actions, K, *args)
    assert set(got) == {"J", "grad", "gains_grad"}
    assert torch.equal(got["J"], engine.rollout_feedback(w.actions, K, *args)["J"])
    back = engine.rollout_feedback_backward(w.actions, K, *args, J_bar=np.ones(B), want_initial=False)
    assert set(back) == {"actions_bar", "gains_bar"}
    assert torch.equal(back["actions_bar"], got["grad"]) and torch.equal(back["gains_bar"], got["gains_grad"])
    # the model method is the engine's call, with gains_grad reduced the way the gains were broadcast
    model = GpStateTransitionModel(ModelConfig(), D, A, engine=engine)
    model.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    model.set_cost(lin.reward_config_of(w))
    for gains, axes in ((K, None), (K[0], 0), (K[0, 0], (0, 1))):
        ref = engine.rollout_feedback_grad(w.actions, gains, *args)
        out = model.feedback_objective_and_gradient_batch(w.actions, gains, w.mu0, w.S0, 0)
        assert set(out) == {"J", "grad", "gains_grad"} and out["gains_grad"].shape == np.shape(gains)
        assert torch.equal(out["J"], ref["J"]) and torch.equal(out["grad"], ref["grad"])
        assert torch.equal(out["gains_grad"], ref["gains_grad"] if axes is None else ref["gains_grad"].sum(axes))
    with pytest.raises(ValueError):
        model.feedback_objective_and_gradient_batch(w.actions, "lqr", w.mu0, w.S0, 0)


# -- 5. errors, options, no interference ---------------------------------------------------------------------------------------
def test_errors_and_no_interference():
    import gp_mpc_amd
    from gp_mpc_amd import _lib as L
    eng = gp_mpc_amd.HipEngine(0)
    try:
        w = _workload(50, 3, 4, False, seed=850)
        K = _gains(w, 851)
        acts, gains = eng._dev(w.actions), eng._dev(K)
        mu0, S0 = np.ascontiguousarray(w.mu0), np.ascontiguousarray(w.S0)
        ones = lambda *s: torch.ones(s, dtype=torch.float64, device=eng.device)                  # noqa: E731
        nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=eng.device)      # noqa: E731
        mu_bar, J_bar, cm_bar = ones(4, 4, 3), ones(4), ones(4, 4)
        a_bar, K_bar, m_bar, S_bar = nan(4, 3, 1), nan(4, 3, 1, 3), nan(4, 3), nan(4, 3, 3)
        hp = lambda a: a.ctypes.data                                        # noqa: E731

        def call(B=4, H=3, A=1, time=0, actions=acts.data_ptr(), g=gains.data_ptr(), m0=hp(mu0), s0=hp(S0), mub=mu_bar.data_ptr(),
                 cmb=None, cvb=None, Jb=None, out=a_bar.data_ptr(), gout=K_bar.data_ptr()):
            return eng.lib.gpmpc_rollout_feedback_backward(eng._h, actions, g, 1, m0, s0, B, H, A, time, 0.0, mub, None, cmb, cvb, Jb,
                                                           out, gout, m_bar.data_ptr(), S_bar.data_ptr(), eng._stream())

        def untouched():
            torch.cuda.synchronize()
            return all(bool(torch.isnan(t).all()) for t in (a_bar, K_bar, m_bar, S_bar))

        assert call() == L.GPMPC_ERR_ARG and "prepare" in eng.lib.gpmpc_last_error(eng._h).decode()     # no cached model
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        for kw in (dict(Jb=J_bar.data_ptr()), dict(cmb=cm_bar.data_ptr()), dict(cvb=cm_bar.data_ptr())):
            assert call(**kw) == L.GPMPC_ERR_ARG and "set_cost" in eng.lib.gpmpc_last_error(eng._h).decode(), kw
        # gpmpc_rollout_feedback's argument errors, a NULL actions_bar, gains_bar without gains
        for kw in (dict(out=None), dict(g=None), dict(A=0), dict(A=-1), dict(B=0), dict(H=0), dict(A=2), dict(time=1),
                   dict(actions=None), dict(m0=None), dict(s0=None)):
            assert call(**kw) == L.GPMPC_ERR_ARG, kw
        assert untouched()
        # A < 1: a model whose inputs are the state alone
        w0 = synth.make_workload(50, 3, 0, 3, 4, seed=852)
        eng.prepare(w0.X, w0.Y, w0.lengthscales, w0.outputscales, w0.noises)
        assert call(A=0, g=None, gout=None) == L.GPMPC_ERR_ARG and "A >= 1" in eng.lib.gpmpc_last_error(eng._h).decode()
        assert untouched()
        # (the compiled limits D <= GPMPC_MAX_D, E <= GPMPC_MAX_E cannot be exceeded by a cached model: gpmpc_prepare refuses it)
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        assert call() == L.GPMPC_OK                                          # trajectory cotangents need no cost settings
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(t).all()) for t in (a_bar, K_bar, m_bar, S_bar))
        assert call(g=None, gout=None) == L.GPMPC_OK                         # the zero-gain policy
        with pytest.raises(RuntimeError) as ei:
            eng.rollout_feedback_grad(w.actions, K, w.mu0, w.S0)
        assert type(ei.value).__name__ == "GpmpcError" and ei.value.code == L.GPMPC_ERR_ARG
        for shape in ((3, 1), (4, 1, 3), (4, 3, 3, 1), (2, 3, 1, 3)):
            with pytest.raises(ValueError):
                eng.rollout_feedback_backward(w.actions, np.zeros(shape), w.mu0, w.S0, mu_bar=np.ones((4, 4, 3)))
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        assert call(Jb=J_bar.data_ptr(), cmb=cm_bar.data_ptr()) == L.GPMPC_OK
        # the chunk option: a bad value is refused, 0 restores the default
        seeds = _seeds(w, 853)
        base = eng.rollout_feedback_backward(w.actions, K, w.mu0, w.S0, **seeds)
        with pytest.raises(RuntimeError):
            eng.set_option(CHUNK, -1)
        eng.set_option(CHUNK, 3)
        three = eng.rollout_feedback_backward(w.actions, K, w.mu0, w.S0, **seeds)
        eng.set_option(CHUNK, 0)
        again = eng.rollout_feedback_backward(w.actions, K, w.mu0, w.S0, **seeds)
        for k in KEYS:
            assert torch.equal(three[k], base[k]) and torch.equal(again[k], base[k]), k
        # no interference through the workspaces: the forward and the moment gradient keep their bits, gpmpc_last_* stays
        m_in = np.concatenate([np.tile(w.mu0, (4, 1)), w.actions[:, 0]], axis=1)
        v_in = np.zeros((4, 4, 4))
        v_in[:, :3, :3] = w.S0
        rng = np.random.default_rng(854)
        ups = dict(M_bar=rng.standard_normal((4, 3)), S_bar=rng.standard_normal((4, 3, 3)), V_bar=rng.standard_normal((4, 4, 3)))

        def others():
            res = [eng.rollout_feedback(w.actions, K, w.mu0, w.S0), eng.moments_backward(m_in, v_in, **ups),
                   eng.rollout_backward(w.actions, w.mu0, w.S0, **seeds)]
            return [{k: v.clone() for k, v in r.items()} for r in res]
        before = others()
        state = (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode, eng.last_grad_path)
        out = eng.rollout_feedback_grad(w.actions, K, w.mu0, w.S0)
        assert bool(torch.all(torch.isfinite(out["grad"]))) and bool(torch.any(out["grad"])) and bool(torch.any(out["gains_grad"]))
        assert (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode, eng.last_grad_path) == state
        for b, a in zip(before, others()):
            for k in b:
                assert torch.equal(b[k], a[k]), k
    finally:
        eng.close()
