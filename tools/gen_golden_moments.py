#!/usr/bin/env python3
"""Generate tests/golden/moments_full_var*.npz by EXECUTING THE REFERENCE'S OWN CODE (this container only).

predict_next_state_change (gp_model.py:112-180) with a general input covariance, what gpmpc_moments computes.  This tool reuses
gen_golden.py's placeholder modules and reference model (its existing cases are untouched) and calls that function once per
point, for 24 points of a memory of N = 200 (D = 3, A = 2; the second file adds a time input):
  *  8 dense full-E Sigma (state, action and time inputs correlated),
  *  4 Sigma non-zero only in the action block,
  *  4 Sigma non-zero only on the time variance (on the last action's variance without a time input),
  *  4 Sigma = 0,
  *  4 Sigma several lengthscales wide.
The means are drawn in the box of the memory inputs.  Only data is written.  Re-run:  python tools/gen_golden_moments.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (installs the placeholders and imports the reference)

torch = G.torch


def input_points(w, seed):
    """(mean (24, E), covariance (24, E, E), kind (24,)): kind 0 dense, 1 action block, 2 time, 3 zero, 4 wide."""
    rng = np.random.default_rng(seed)
    N, D, A, E, H, B = w.dims
    lo, hi = w.X.min(axis=0), w.X.max(axis=0)
    mean = lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(24, E))
    var = np.zeros((24, E, E))
    kind = np.repeat(np.arange(5), [8, 4, 4, 4, 4])
    ls = w.lengthscales.min(axis=0)                 # the shortest lengthscale of every input dimension
    for p in range(24):
        k = kind[p]
        if k == 0:
            G_ = rng.standard_normal((E, E)) * (0.3 * ls)[:, None]
            var[p] = G_ @ G_.T + 1e-6 * np.diag(ls ** 2)
        elif k == 1:
            G_ = rng.standard_normal((A, A)) * 0.2
            var[p, D:D + A, D:D + A] = G_ @ G_.T + 1e-4 * np.eye(A)
        elif k == 2:
            var[p, E - 1, E - 1] = (rng.uniform(0.2, 1.0) * ls[E - 1]) ** 2
        elif k == 4:
            G_ = rng.standard_normal((E, E)) * (rng.uniform(2.0, 4.0) * ls)[:, None]
            var[p] = G_ @ G_.T + 0.5 * np.diag(ls ** 2)
    return mean, var, kind


def moments_case(name, w, seed):
    m = G.ref_model(w)
    N, D, A, E, H, B = w.dims
    mean, var, kind = input_points(w, seed)
    Ms, Ss, Vs = [], [], []
    for x, s in zip(mean, var):
        Mt, S, Vt = m.predict_next_state_change(torch.tensor(x), torch.tensor(s))
        Ms.append(Mt.numpy().reshape(D))
        Ss.append(S.numpy())
        Vs.append(Vt.numpy())
    d = G.inputs_dict(w)
    d.update(beta=m.beta.numpy(), iK=m.iK.numpy(), in_mean=mean, in_var=var, M=np.stack(Ms), S=np.stack(Ss), V=np.stack(Vs),
             kind=kind)
    np.savez_compressed(os.path.join(G.OUT, name + ".npz"), **d)
    print(f"{name}: N={N} D={D} E={E} M[0]={Ms[0]}  max|S|={np.abs(np.stack(Ss)).max():.3e}")


def main():
    os.makedirs(G.OUT, exist_ok=True)
    mk = G.synth.make_workload
    moments_case("moments_full_var", mk(200, 3, 2, 2, 1, seed=160), seed=161)
    moments_case("moments_full_var_time", mk(200, 3, 2, 2, 1, include_time=True, seed=162, time0=200.0), seed=163)


if __name__ == "__main__":
    main()
