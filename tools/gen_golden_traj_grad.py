#!/usr/bin/env python3
"""Generate tests/golden/traj_grad_*.npz by EXECUTING THE REFERENCE'S OWN CODE under torch autograd (this container only).

The reverse-mode product of predict_trajectory (gp_model.py:60-110) followed by get_rewards_trajectory
(setpoint_distance_reward_mapper.py:144-149) that gpmpc_rollout_backward computes.  This tool reuses gen_golden.py's placeholder
modules, reference model and reward mapper, rebuilds the workloads of the committed traj_*.npz and asserts that the rebuilt mu, Sig,
rewards and reward_vars equal them bit for bit (traj_c5class: to 1e-13 of scale, see main()).  Every candidate gets three seeded
upstream sets: 0 all of mu_bar, Sig_bar, rewards_bar, reward_vars_bar; 1 the trajectory only (mu_bar, Sig_bar); 2 the rewards only (rewards_bar, reward_vars_bar).  For
each it stores the RAW autograd gradients of <mu_bar, mu> + <Sig_bar, Sig> + <rewards_bar, rewards> + <reward_vars_bar,
reward_vars> with respect to the actions (H, A), obs_mu (D) and obs_var (D, D), obs_var's not symmetrised (the tests take the
symmetric part).  The reference's rewards are -cost_mu and its reward variances are cost_var: the tests convert the seeds.
Only data is written.  Re-run:  python tools/gen_golden_traj_grad.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (installs the placeholders and imports the reference)

torch = G.torch


def grad_case(name, fwd_name, w, n_cand, up_seed, use_constraints=False, state_min=None, state_max=None, exact=True):
    m = G.ref_model(w)
    N, D, A, E, H, B = w.dims
    rm, _ = G.ref_reward_mapper(w, False, use_constraints, state_min, state_max)
    ref = np.load(os.path.join(G.OUT, fwd_name + ".npz"))
    assert np.array_equal(ref["actions"], w.actions) and np.array_equal(ref["mu0"], w.mu0) and np.array_equal(ref["S0"], w.S0)
    rng = np.random.default_rng(up_seed)
    C = n_cand
    mu_bar = rng.standard_normal((3, C, H + 1, D))
    Sig_bar = rng.standard_normal((3, C, H + 1, D, D))
    rew_bar = rng.standard_normal((3, C, H + 1))
    rvar_bar = rng.standard_normal((3, C, H + 1))
    mu_bar[2] = 0.0
    Sig_bar[2] = 0.0
    rew_bar[1] = 0.0
    rvar_bar[1] = 0.0
    g_act = np.zeros((3, C, H, A))
    g_mu0 = np.zeros((3, C, D))
    g_S0 = np.zeros((3, C, D, D))
    for b in range(C):
        for s in range(3):
            act = torch.tensor(w.actions[b], requires_grad=True)
            x0 = torch.tensor(w.mu0, requires_grad=True)
            S0 = torch.tensor(w.S0, requires_grad=True)
            mu, Sig = m.predict_trajectory(act, x0, S0, H, int(w.time0))
            r, rv = rm.get_rewards_trajectory(mu, Sig, act)
            if s == 0:
                for k, v in (("mu", mu), ("Sig", Sig), ("rewards", r), ("reward_vars", rv)):
                    v = v.detach().numpy()
                    if exact:
                        assert np.array_equal(v, ref[k][b]), k
                    else:
                        assert np.abs(v - ref[k][b]).max() <= 1e-13 * np.abs(ref[k][b]).max(), k
            loss = (torch.tensor(mu_bar[s, b]) * mu).sum() + (torch.tensor(Sig_bar[s, b]) * Sig).sum() + \
                (torch.tensor(rew_bar[s, b]) * r).sum() + (torch.tensor(rvar_bar[s, b]) * rv).sum()
            loss.backward()
            g_act[s, b] = act.grad.numpy()
            g_mu0[s, b] = x0.grad.numpy()
            g_S0[s, b] = S0.grad.numpy()
    np.savez_compressed(os.path.join(G.OUT, name + ".npz"), source=np.array(fwd_name), candidates=np.array(C),
                        mu_bar=mu_bar, Sig_bar=Sig_bar, rewards_bar=rew_bar, reward_vars_bar=rvar_bar,
                        actions_grad=g_act, obs_mu_grad=g_mu0, obs_var_grad=g_S0)
    asym = np.abs(g_S0 - np.swapaxes(g_S0, -1, -2)).max() / np.abs(g_S0).max()
    print(f"{name}: D={D} A={A} E={E} H={H} candidates={C}  max|d/du|={np.abs(g_act).max():.3e}  "
          f"max|G - G^T| / max|G| = {asym:.2f}")


def main():
    mk = G.synth.make_workload
    grad_case("traj_grad_c1", "traj_c1", mk(50, 3, 1, 15, 8, seed=20), 3, up_seed=170)
    grad_case("traj_grad_c4_time", "traj_c4_time", mk(300, 4, 2, 30, 2, include_time=True, seed=24, time0=300.0), 2, up_seed=171)
    grad_case("traj_grad_constraints", "traj_constraints", mk(50, 3, 1, 10, 4, seed=27), 2, up_seed=172, use_constraints=True,
              state_min=[0.05, 0.05, 0.05], state_max=[0.95, 0.95, 0.925])
    # D = 16: the reference's own factorisation of this memory (LAPACK's Cholesky of a 128 x 128 K) differs from the one behind
    # traj_c5class.npz in the last bits (beta to 6e-15), so that rebuild is checked to 1e-13 of scale instead of bit for bit
    grad_case("traj_grad_c5class", "traj_c5class", mk(128, 16, 4, 5, 2, seed=25), 2, up_seed=173, exact=False)


if __name__ == "__main__":
    main()
