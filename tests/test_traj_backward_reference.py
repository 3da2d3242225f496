"""Tier 1 (CPU): gradients of whole predicted trajectories, pinned to the reference's own autograd independently of autograd.

tests/golden/traj_grad_*.npz hold torch autograd through the reference's predict_trajectory + get_rewards_trajectory
(gp_model.py:60-110, setpoint_distance_reward_mapper.py:144-149) for three upstream sets per candidate
(tools/gen_golden_traj_grad.py): the raw gradients with respect to the actions, obs_mu and obs_var.  The numpy VJP of
tests/traj_vjp.py (oracle.adjoint's steps with general cotangents) must reproduce them, and must itself agree with longdouble
central differences of oracle.extended_precision.predict_trajectory.  Also: the C header declares gpmpc_rollout_backward and
the built library exports it.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import load, workload_of, factors_of, rel_err
from traj_vjp import traj_vjp, golden_seeds
from oracle import adjoint
from oracle import extended_precision as xp

GOLDENS = ["traj_c1", "traj_c4_time", "traj_constraints", "traj_c5class"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sym(G):
    return 0.5 * (G + np.swapaxes(G, -1, -2))


def _grad_name(name):
    return name.replace("traj_", "traj_grad_")


def _cost_args(g):
    kw = {}
    if bool(g["use_constraints"]):
        kw = dict(state_min=g["state_min"], state_max=g["state_max"])
    return kw


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_upstream_sets(name):
    g, gg = load(name), load(_grad_name(name))
    assert str(gg["source"]) == name
    C = int(gg["candidates"])
    B, H1, D = g["mu"].shape
    A = g["actions"].shape[2]
    assert C <= B and gg["mu_bar"].shape == (3, C, H1, D) and gg["actions_grad"].shape == (3, C, H1 - 1, A)
    # set 0: everything; set 1: the trajectory only; set 2: the rewards only
    assert np.all(gg["mu_bar"][:2] != 0) and np.all(gg["Sig_bar"][:2] != 0) and np.all(gg["mu_bar"][2] == 0)
    assert np.all(gg["rewards_bar"][1] == 0) and np.all(gg["reward_vars_bar"][1] == 0)
    assert np.all(gg["rewards_bar"][[0, 2]] != 0) and np.all(gg["reward_vars_bar"][[0, 2]] != 0)
    # the raw autograd gradient of obs_var is not symmetric: the reason the library returns its symmetric part
    G = gg["obs_var_grad"][0]
    assert np.abs(G - np.swapaxes(G, -1, -2)).max() > 1e-3 * np.abs(G).max()


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("s", [0, 1, 2])
def test_numpy_vjp_matches_reference_autograd(name, s):
    g, gg = load(name), load(_grad_name(name))
    w = workload_of(g)
    f = factors_of(w)
    for b in range(int(gg["candidates"])):
        ga, gm, gS = traj_vjp(f, w.actions[b], w.mu0, w.S0, w.target, w.W, w.W_T, w.kappa, **golden_seeds(gg, s, b),
                              include_time=w.include_time, time0=w.time0, **_cost_args(g))
        e = (rel_err(ga, gg["actions_grad"][s, b]), rel_err(gm, gg["obs_mu_grad"][s, b]), rel_err(gS, _sym(gg["obs_var_grad"][s, b])))
        assert max(e) < 1e-9, (name, s, b, e)


def test_numpy_vjp_with_objective_seed_is_the_lcb_gradient():
    g = load("traj_c1")
    w = workload_of(g)
    f = factors_of(w)
    ga, _, _ = traj_vjp(f, w.actions[0], w.mu0, w.S0, w.target, w.W, w.W_T, w.kappa, J_bar=1.0)
    _, g0, *_ = adjoint.lcb_and_gradient(f, w.actions[0], w.mu0, w.S0, w.target, w.W, w.W_T, w.kappa)
    assert rel_err(ga, g0) < 1e-12


def _xloss(fx, act, mu0, S0, mu_bar, Sig_bar, include_time, time0):
    mu, Sig = xp.predict_trajectory(fx, act, mu0, S0, include_time, time0)
    return (mu * xp._ld(mu_bar)).sum() + (Sig * xp._ld(Sig_bar)).sum()


@pytest.mark.parametrize("name", ["traj_c1", "traj_c4_time"])
def test_numpy_vjp_matches_longdouble_differences(name):
    g, gg = load(name), load(_grad_name(name))
    w = workload_of(g)
    f = factors_of(w)
    fx = xp.Factors(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    rng = np.random.default_rng(7)
    LD = np.longdouble
    mb, Sb = gg["mu_bar"][1, 0], gg["Sig_bar"][1, 0]
    ga, gm, gS = traj_vjp(f, w.actions[0], w.mu0, w.S0, w.target, w.W, w.W_T, w.kappa, mu_bar=mb, Sig_bar=Sb,
                          include_time=w.include_time, time0=w.time0)
    D = w.mu0.shape[0]
    h = 1e-6
    for _ in range(3):
        da = 0.1 * rng.standard_normal(w.actions[0].shape)
        dm = 0.01 * rng.standard_normal(D)
        R = rng.standard_normal((D, D))
        dS = 1e-4 * (R + R.T)
        a0, m0, S0 = xp._ld(w.actions[0]), xp._ld(w.mu0), xp._ld(w.S0)
        lp = _xloss(fx, a0 + LD(h) * xp._ld(da), m0 + LD(h) * xp._ld(dm), S0 + LD(h) * xp._ld(dS), mb, Sb, w.include_time, w.time0)
        lm = _xloss(fx, a0 - LD(h) * xp._ld(da), m0 - LD(h) * xp._ld(dm), S0 - LD(h) * xp._ld(dS), mb, Sb, w.include_time, w.time0)
        fd = float((lp - lm) / (2 * LD(h)))
        an = float((ga * da).sum() + gm @ dm + (gS * dS).sum())
        assert abs(an - fd) < 1e-7 * (abs(fd) + 1e-3), (an, fd)


def test_header_declares_and_library_exports_rollout_backward():
    hdr = open(os.path.join(ROOT, "include", "gpmpc.h")).read()
    assert re.search(r"\bint\s+gpmpc_rollout_backward\s*\(", hdr)
    import gp_mpc_amd
    lib = ctypes.CDLL(gp_mpc_amd.LIB_PATH)
    assert hasattr(lib, "gpmpc_rollout_backward")
    assert hasattr(gp_mpc_amd.HipEngine, "rollout_backward")
