"""Tier 2 (GPU): gpmpc_rollout_backward -- gradients of whole predicted trajectories and their costs.

Pinned to torch autograd through the reference's predict_trajectory + get_rewards_trajectory (tests/golden/traj_grad_*.npz,
tools/gen_golden_traj_grad.py; tests/test_traj_backward_reference.py ties them to the numpy VJP and to longdouble differences),
to gpmpc_rollout_grad bit for bit with the objective's seed alone, on every moment path, to the numpy VJP of tests/traj_vjp.py
and to torch autograd through H chained predict_next_state_change_batch calls (gpmpc_moments + gpmpc_moments_backward:
independent GPU code) with random seeds, to the reference's own composition (predict_trajectory -> get_rewards_trajectory ->
LCB -> torch.autograd.grad), and to the contracts of include/gpmpc.h.  Covariance gradients are compared as symmetric parts.
"""
import numpy as np
import pytest
import torch

from helpers import load, workload_of, factors_of, rel_err, record, make_controller
from traj_vjp import traj_vjp, golden_seeds
from oracle import synth

pytestmark = pytest.mark.gpu

GOLDENS = ["traj_c1", "traj_c4_time", "traj_constraints", "traj_c5class"]
TOL = 1e-7


@pytest.fixture(scope="module")
def engine():
    import gp_mpc_amd
    eng = gp_mpc_amd.HipEngine(0)
    yield eng
    eng.close()


def _np(t):
    return t.detach().cpu().numpy()


def _sym(G):
    return 0.5 * (G + np.swapaxes(G, -1, -2))


def _load(engine, w, g=None):
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    use_c = g is not None and bool(g["use_constraints"])
    engine.set_cost(w.target, w.W, w.W_T, w.kappa, bool(g["clip"]) if g is not None else False,
                    g["state_min"] if use_c else None, g["state_max"] if use_c else None)


# -- 1. goldens of the reference's own autograd -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_reference_autograd_goldens(engine, name):
    g, gg = load(name), load(name.replace("traj_", "traj_grad_"))
    w = workload_of(g)
    _load(engine, w, g)
    C = int(gg["candidates"])
    worst = 0.0
    for s in range(3):
        seeds = [golden_seeds(gg, s, b) for b in range(C)]
        st = lambda k: np.stack([sd[k] for sd in seeds])  # noqa: E731
        out = engine.rollout_backward(w.actions[:C], w.mu0, w.S0, w.include_time, w.time0, mu_bar=st("mu_bar"),
                                      Sig_bar=st("Sig_bar"), cost_mu_bar=st("cm_bar"), cost_var_bar=st("cv_bar"))
        for b in range(C):
            e = (rel_err(_np(out["actions_bar"][b]), gg["actions_grad"][s, b]), rel_err(_np(out["mu0_bar"][b]), gg["obs_mu_grad"][s, b]),
                 rel_err(_np(out["S0_bar"][b]), _sym(gg["obs_var_grad"][s, b])))
            worst = max(worst, *e)
            assert max(e) < TOL, (name, s, b, e)
    record(f"rollout_backward_golden_{name}", max_rel_err=worst)


# -- 2./3. every moment path: bitwise with the LCB gradient, random seeds against the numpy VJP and the moments chain --------
# (name, N, D, A, H, B, include_time, options, grad-path bit that must be set, cooperative forward expected)
PATHS = [
    ("separable", 130, 3, 1, 4, 3, False, {"grad_separable": 2}, 1, False),
    ("tiles", 130, 3, 2, 3, 3, True, {"grad_tiles": 2, "pair_tiles": 2}, 2, False),
    ("stream", 70, 3, 1, 4, 3, False, {"grad_stream": 1}, 4, False),
    ("wide", 60, 10, 2, 3, 2, False, {}, 8, False),
    ("fused_c4", 300, 4, 2, 3, 2, False, {"grad_tiles": 2, "pair_tiles": 1}, 16, False),
    ("mean", 60, 3, 1, 6, 64, False, {}, 32, False),
    ("few_b1", 60, 3, 2, 6, 1, True, {}, 64, False),
    ("coop_b1", 200, 3, 1, 25, 1, False, {}, 64, True),
]
DEFAULTS = {"grad_separable": 1, "grad_tiles": 1, "pair_tiles": 0, "grad_stream": 0}


def _workload(N, D, A, H, B, tm, seed):
    return synth.make_workload(N, D, A, H, B, include_time=tm, seed=seed, s0=1e-4, time0=2.0 if tm else 0.0)


def _with_options(engine, opts, fn):
    for k, v in opts.items():
        engine.set_option(k, v)
    try:
        return fn()
    finally:
        for k in opts:
            engine.set_option(k, DEFAULTS[k])


def _random_seeds(B, H, D, seed):
    rng = np.random.default_rng(seed)
    return dict(mu_bar=rng.standard_normal((B, H + 1, D)), Sig_bar=rng.standard_normal((B, H + 1, D, D)),
                cost_mu_bar=rng.standard_normal((B, H + 1)), cost_var_bar=rng.standard_normal((B, H + 1)),
                J_bar=rng.standard_normal(B))


@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
def test_objective_seed_is_bitwise_the_lcb_gradient(engine, path):
    name, N, D, A, H, B, tm, opts, bit, coop = path
    w = _workload(N, D, A, H, B, tm, seed=N + D + B)
    _load(engine, w)

    def run():
        ref = engine.rollout_grad(w.actions, w.mu0, w.S0, w.include_time, w.time0)["grad"].clone()
        p_ref, c_ref = engine.last_grad_path, engine.last_cluster
        out = engine.rollout_backward(w.actions, w.mu0, w.S0, w.include_time, w.time0, J_bar=np.ones(B))
        return ref, p_ref, c_ref, out, engine.last_grad_path, engine.last_cluster
    ref, p_ref, c_ref, out, p_bwd, c_bwd = _with_options(engine, opts, run)
    assert p_ref & bit and p_bwd == p_ref, (name, p_ref, p_bwd)
    assert c_bwd == c_ref and (c_ref > 1 or not coop), (c_ref, c_bwd)
    assert torch.equal(out["actions_bar"], ref), name


@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
def test_random_seeds_against_numpy_vjp(engine, path):
    name, N, D, A, H, B, tm, opts, bit, coop = path
    w = _workload(N, D, A, H, B, tm, seed=N + D + B)
    _load(engine, w)
    sd = _random_seeds(B, H, D, seed=N + B)
    out = _with_options(engine, opts, lambda: engine.rollout_backward(w.actions, w.mu0, w.S0, w.include_time, w.time0, **sd))
    assert engine.last_grad_path & bit
    f = factors_of(w)
    worst = 0.0
    for b in sorted({0, B - 1}):
        ga, gm, gS = traj_vjp(f, w.actions[b], w.mu0, w.S0, w.target, w.W, w.W_T, w.kappa, sd["mu_bar"][b], sd["Sig_bar"][b],
                              sd["cost_mu_bar"][b], sd["cost_var_bar"][b], sd["J_bar"][b], w.include_time, w.time0)
        e = (rel_err(_np(out["actions_bar"][b]), ga), rel_err(_np(out["mu0_bar"][b]), gm), rel_err(_np(out["S0_bar"][b]), gS))
        worst = max(worst, *e)
        assert max(e) < TOL, (name, b, e)
    record(f"rollout_backward_vjp_{name}", max_rel_err=worst)


def _moments_chain(engine, w, acts, mu0, S0):
    """predict_trajectory restated as H chained gpmpc_moments autograd nodes (the reference's loop, gp_model.py:60-110)."""
    from gp_mpc_amd.control_objects.models.gp_model import _MomentsFunction
    B, H, A = acts.shape
    D = mu0.shape[0]
    E = w.X.shape[1]
    mu = mu0.expand(B, D)
    Sig = S0.expand(B, D, D)
    mus, Sigs = [mu], [Sig]
    for t in range(H):
        parts = [mu, acts[:, t]]
        if w.include_time:
            parts.append(torch.full((B, 1), w.time0 + t, dtype=torch.float64, device=acts.device))
        m = torch.cat(parts, 1)
        var = torch.zeros((B, E, E), dtype=torch.float64, device=acts.device)
        var[:, :D, :D] = Sig
        M, S, V = _MomentsFunction.apply(engine, m, var)
        C = var[:, :D, :] @ V
        mu, Sig = mu + M, S + Sig + C + C.transpose(1, 2)
        mus.append(mu)
        Sigs.append(Sig)
    return torch.stack(mus, 1), torch.stack(Sigs, 1)


@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
def test_trajectory_seeds_against_chained_moments_autograd(engine, path):
    name, N, D, A, H, B, tm, opts, bit, coop = path
    if B > 8:
        B = 8
    w = _workload(N, D, A, H, B, tm, seed=N + D + B)
    _load(engine, w)
    sd = _random_seeds(B, H, D, seed=N + 7)
    out = _with_options(engine, opts, lambda: engine.rollout_backward(w.actions, w.mu0, w.S0, w.include_time, w.time0,
                                                                      mu_bar=sd["mu_bar"], Sig_bar=sd["Sig_bar"]))
    dev = engine.device
    acts = torch.tensor(w.actions, device=dev, requires_grad=True)
    mu0 = torch.tensor(w.mu0, device=dev, requires_grad=True)
    S0 = torch.tensor(w.S0, device=dev, requires_grad=True)
    mus, Sigs = _moments_chain(engine, w, acts, mu0, S0)
    loss = (mus * torch.tensor(sd["mu_bar"], device=dev)).sum() + (Sigs * torch.tensor(sd["Sig_bar"], device=dev)).sum()
    ga, gm, gS = torch.autograd.grad(loss, (acts, mu0, S0))
    e = (rel_err(_np(out["actions_bar"]), _np(ga)), rel_err(_np(out["mu0_bar"].sum(0)), _np(gm)),
         rel_err(_np(out["S0_bar"].sum(0)), _sym(_np(gS))))
    record(f"rollout_backward_chain_{name}", max_rel_err=max(e))
    assert max(e) < TOL, (name, e)


# -- 4. the reference's own composition -------------------------------------------------------------------------------------
def test_reference_composition_reproduces_the_lcb_gradient(engine):
    w = synth.make_workload(50, 3, 1, 15, 2, seed=20)
    c = make_controller(w, engine=engine)
    m = c.transition_model
    m.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    m.set_cost(c.config.reward)
    H = w.actions.shape[1]
    act = torch.tensor(w.actions[0], requires_grad=True)
    obs_mu = torch.tensor(w.mu0, requires_grad=True)
    mu, Sig = m.predict_trajectory(act, obs_mu, torch.tensor(w.S0), H, 0)
    assert mu.grad_fn is not None and Sig.grad_fn is not None
    r, rv = c.state_reward_mapper.get_rewards_trajectory(mu, Sig, act)
    J = -(r + w.kappa * torch.sqrt(rv)).mean()                  # compute_mean_lcb_trajectory (gp_mpc_controller.py:270-276)
    ga, gm = torch.autograd.grad(J, (act, obs_mu))
    ref = m.objective_and_gradient_batch(w.actions[:1], w.mu0, w.S0, 0)
    e = rel_err(ga.numpy(), _np(ref["grad"][0]))
    assert e < 1e-10, e
    assert abs(float(J.detach()) - float(ref["J"][0])) < 1e-10 * abs(float(J.detach()))
    # obs_mu's gradient against a central difference of J through gpmpc_rollout
    rng = np.random.default_rng(3)
    d = rng.standard_normal(3)
    h = 1e-5
    Jp = float(engine.rollout(w.actions[:1], w.mu0 + h * d, w.S0)["J"][0])
    Jm = float(engine.rollout(w.actions[:1], w.mu0 - h * d, w.S0)["J"][0])
    fd = (Jp - Jm) / (2 * h)
    assert abs(float(gm @ torch.tensor(d)) - fd) < 1e-6 * max(1.0, abs(fd)), (float(gm @ torch.tensor(d)), fd)
    record("rollout_backward_composition", max_rel_err=e)


# -- 5. contracts ---------------------------------------------------------------------------------------------------------
def test_null_seeds_are_zero_and_outputs_are_overwritten(engine):
    w = _workload(60, 3, 1, 5, 3, False, seed=11)
    _load(engine, w)
    B, H, D = 3, 5, 3
    sd = _random_seeds(B, H, D, seed=5)
    a = engine.rollout_backward(w.actions, w.mu0, w.S0, mu_bar=sd["mu_bar"])
    z = engine.rollout_backward(w.actions, w.mu0, w.S0, mu_bar=sd["mu_bar"], Sig_bar=np.zeros((B, H + 1, D, D)),
                                cost_mu_bar=np.zeros((B, H + 1)), cost_var_bar=np.zeros((B, H + 1)), J_bar=np.zeros(B))
    for k in ("actions_bar", "mu0_bar", "S0_bar"):
        assert torch.equal(a[k], z[k]), k
    # overwritten, not accumulated: straight at the library with NaN-filled outputs, and NULL initial-state outputs
    import ctypes
    act = torch.tensor(w.actions, device=engine.device)
    outs = [torch.full(s, float("nan"), dtype=torch.float64, device=engine.device) for s in ((B, H, 1), (B, D), (B, D, D))]
    mb = torch.tensor(sd["mu_bar"], device=engine.device)
    mu0, S0 = np.ascontiguousarray(w.mu0), np.ascontiguousarray(w.S0)
    hp = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for o in (outs, [outs[0], None, None]):
        rc = engine.lib.gpmpc_rollout_backward(engine._h, act.data_ptr(), hp(mu0), hp(S0), B, H, 1, 0, 0.0, mb.data_ptr(), None,
                                               None, None, None, o[0].data_ptr(), o[1].data_ptr() if o[1] is not None else None,
                                               o[2].data_ptr() if o[2] is not None else None, engine._stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(outs[0], a["actions_bar"]) and torch.equal(outs[1], a["mu0_bar"]) and torch.equal(outs[2], a["S0_bar"])
    # S0_bar symmetric bit for bit
    full = engine.rollout_backward(w.actions, w.mu0, w.S0, **sd)
    assert torch.equal(full["S0_bar"], full["S0_bar"].transpose(1, 2))
    # want_initial=False: only actions_bar, the same bits
    only = engine.rollout_backward(w.actions, w.mu0, w.S0, want_initial=False, **sd)
    assert set(only) == {"actions_bar"} and torch.equal(only["actions_bar"], full["actions_bar"])


def test_errors_and_trajectory_seeds_without_cost(engine):
    import gp_mpc_amd
    from gp_mpc_amd import GpmpcError
    w = _workload(40, 3, 1, 3, 2, False, seed=12)
    eng = gp_mpc_amd.HipEngine(0)
    try:
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        sd = _random_seeds(2, 3, 3, seed=1)
        with pytest.raises(GpmpcError) as ei:
            eng.rollout_backward(w.actions, w.mu0, w.S0, J_bar=np.ones(2))
        assert ei.value.code == -1
        with pytest.raises(GpmpcError) as ei:
            eng.rollout_backward(w.actions, w.mu0, w.S0, cost_var_bar=sd["cost_var_bar"])
        assert ei.value.code == -1
        # the trajectory's cotangents need no cost settings; the same bits with a cost loaded
        a = eng.rollout_backward(w.actions, w.mu0, w.S0, mu_bar=sd["mu_bar"], Sig_bar=sd["Sig_bar"])
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        b = eng.rollout_backward(w.actions, w.mu0, w.S0, mu_bar=sd["mu_bar"], Sig_bar=sd["Sig_bar"])
        for k in a:
            assert torch.equal(a[k], b[k]), k
        f = factors_of(w)
        ga, gm, gS = traj_vjp(f, w.actions[1], w.mu0, w.S0, w.target, w.W, w.W_T, w.kappa, sd["mu_bar"][1], sd["Sig_bar"][1])
        assert rel_err(_np(a["actions_bar"][1]), ga) < TOL and rel_err(_np(a["S0_bar"][1]), gS) < TOL
    finally:
        eng.close()
    # A (+ time) > 6 at D <= 8: GPMPC_ERR_LIMIT from the entry
    w7 = synth.make_workload(40, 3, 7, 2, 2, seed=2)
    _load(engine, w7)
    with pytest.raises(GpmpcError) as ei:
        engine.rollout_backward(w7.actions, w7.mu0, w7.S0, J_bar=np.ones(2))
    assert ei.value.code == -4


def _model(engine, w):
    c = make_controller(w, engine=engine)
    m = c.transition_model
    m.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    m.set_cost(c.config.reward)
    return m


def test_model_autograd_contracts(engine):
    from gp_mpc_amd import GpmpcError
    w = synth.make_workload(50, 3, 2, 6, 3, seed=21)
    m = _model(engine, w)
    # without requires_grad: today's bits and no grad_fn
    plain = m.predict_trajectory_batch(w.actions, w.mu0, w.S0)
    eng = engine.rollout(w.actions, w.mu0, w.S0)
    for k in eng:
        assert torch.equal(plain[k], eng[k]) and plain[k].grad_fn is None, k
    mu, Sig = m.predict_trajectory(torch.tensor(w.actions[0]), torch.tensor(w.mu0), torch.tensor(w.S0), 6, 0)
    assert mu.grad_fn is None and torch.equal(mu, eng["mu"][0].cpu()) and torch.equal(Sig, eng["Sig"][0].cpu())
    # with requires_grad: the same values, a grad_fn on every output, gradients in the inputs' dtype and device
    acts = torch.tensor(w.actions, device=engine.device, requires_grad=True)
    obs_var = torch.tensor(w.S0, requires_grad=True)
    out = m.predict_trajectory_batch(acts, torch.tensor(w.mu0), obs_var)
    assert set(out) == set(eng)
    for k in eng:
        assert out[k].grad_fn is not None and torch.equal(out[k].detach(), eng[k]), k
    sd = _random_seeds(3, 6, 3, seed=9)
    loss = sum((out[k] * torch.tensor(sd[s], device=engine.device)).sum()
               for k, s in (("mu", "mu_bar"), ("Sig", "Sig_bar"), ("cost_mu", "cost_mu_bar"), ("cost_var", "cost_var_bar"), ("J", "J_bar")))
    loss.backward()
    assert acts.grad.device == acts.device and obs_var.grad.device == obs_var.device and obs_var.grad.dtype == torch.float64
    ref = engine.rollout_backward(w.actions, w.mu0, w.S0, **sd)
    assert torch.equal(acts.grad, ref["actions_bar"])
    assert torch.equal(obs_var.grad, ref["S0_bar"].sum(0).cpu())
    # double backward raises
    out = m.predict_trajectory_batch(acts, torch.tensor(w.mu0), torch.tensor(w.S0))
    g, = torch.autograd.grad(out["J"].sum(), acts, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    # shapes outside the gradient kernels raise at the forward, naming the chaining alternative
    w7 = synth.make_workload(40, 3, 7, 2, 2, seed=2)
    m7 = _model(engine, w7)
    with pytest.raises(GpmpcError) as ei:
        m7.predict_trajectory_batch(torch.tensor(w7.actions, requires_grad=True), w7.mu0, w7.S0)
    assert ei.value.code == -4 and "predict_next_state_change" in str(ei.value)


def test_candidate_alone_and_inside_a_batch(engine):
    w = _workload(60, 3, 1, 6, 8, False, seed=13)
    _load(engine, w)
    sd = _random_seeds(8, 6, 3, seed=2)
    one = {k: v[3:4] for k, v in sd.items()}
    alone = engine.rollout_backward(w.actions[3:4], w.mu0, w.S0, **one)
    pair = engine.rollout_backward(w.actions[2:4], w.mu0, w.S0, **{k: v[2:4] for k, v in sd.items()})
    for k in alone:                                       # 2 B H <= CUs for both: the same forms, the same bits
        assert torch.equal(alone[k][0], pair[k][1]), k
    many = engine.rollout_backward(w.actions, w.mu0, w.S0, **sd)
    for k in alone:                                       # past that the summation orders change
        assert rel_err(_np(many[k][3]), _np(alone[k][0])) < 1e-9, k
