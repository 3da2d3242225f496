#!/usr/bin/env python3
"""Generate tests/golden/moments_grad_full_var*.npz by EXECUTING THE REFERENCE'S OWN CODE under torch autograd (this container only).

The reverse-mode product of predict_next_state_change (gp_model.py:112-180) that gpmpc_moments_backward computes.  This tool
reuses gen_golden.py's placeholder modules and reference model and gen_golden_moments.py's workloads and 24 input points, and
asserts that the rebuilt M, S, V equal the committed moments_full_var*.npz bit for bit (the model of each file is the one of the
matching forward golden).  Every input gets three seeded upstream sets: 0 all of M_bar, S_bar, V_bar; 1 M_bar and V_bar only;
2 S_bar only.  For each it stores the RAW autograd gradients: mu_bar (E,) and G (E, E) of <M_bar, M.t()> + <S_bar, S> +
<V_bar, V.t()>, G not symmetrised (the tests take its symmetric part).  Only data is written.
Re-run:  python tools/gen_golden_moments_grad.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (installs the placeholders and imports the reference)
import gen_golden_moments as GM  # noqa: E402

torch = G.torch


def grad_case(name, fwd_name, w, seed, up_seed):
    m = G.ref_model(w)
    N, D, A, E, H, B = w.dims
    mean, var, kind = GM.input_points(w, seed)
    ref = np.load(os.path.join(G.OUT, fwd_name + ".npz"))
    assert np.array_equal(ref["in_mean"], mean) and np.array_equal(ref["in_var"], var)
    rng = np.random.default_rng(up_seed)
    P = len(mean)
    Mb = rng.standard_normal((3, P, D))
    Sb = rng.standard_normal((3, P, D, D))
    Vb = rng.standard_normal((3, P, E, D))
    Mb[2] = 0.0
    Vb[2] = 0.0
    Sb[1] = 0.0
    mu_bar = np.zeros((3, P, E))
    G_ = np.zeros((3, P, E, E))
    for p in range(P):
        for s in range(3):
            x = torch.tensor(mean[p], requires_grad=True)
            v = torch.tensor(var[p], requires_grad=True)
            Mt, S, Vt = m.predict_next_state_change(x, v)
            if s == 0:
                assert np.array_equal(Mt.detach().numpy().reshape(D), ref["M"][p])
                assert np.array_equal(S.detach().numpy(), ref["S"][p]) and np.array_equal(Vt.detach().numpy(), ref["V"][p])
            loss = (torch.tensor(Mb[s, p]) * Mt.reshape(D)).sum()
            if s != 1:
                loss = loss + (torch.tensor(Sb[s, p]) * S).sum()
            if s != 2:
                loss = loss + (torch.tensor(Vb[s, p]) * Vt).sum()
            loss.backward()
            mu_bar[s, p] = x.grad.numpy()
            G_[s, p] = v.grad.numpy()
    np.savez_compressed(os.path.join(G.OUT, name + ".npz"), in_mean=mean, in_var=var, kind=kind, M_bar=Mb, S_bar=Sb, V_bar=Vb,
                        mu_bar=mu_bar, G=G_)
    asym = np.abs(G_ - np.swapaxes(G_, -1, -2)).max() / np.abs(G_).max()
    print(f"{name}: P={P} E={E}  max|mu_bar|={np.abs(mu_bar).max():.3e}  max|G - G^T| / max|G| = {asym:.2f}")


def main():
    mk = G.synth.make_workload
    grad_case("moments_grad_full_var", "moments_full_var", mk(200, 3, 2, 2, 1, seed=160), seed=161, up_seed=164)
    grad_case("moments_grad_full_var_time", "moments_full_var_time", mk(200, 3, 2, 2, 1, include_time=True, seed=162, time0=200.0),
              seed=163, up_seed=165)


if __name__ == "__main__":
    main()
