#!/usr/bin/env python3
"""Generate tests/golden/predict_batch*.npz by EXECUTING THE REFERENCE'S OWN CODE (this container only).

The GP posterior at deterministic query inputs (what gpmpc_predict computes) is the reference's
predict_next_state_change (gp_model.py:112-180) at zero input variance: M = k^T beta and a diagonal
S with S_aa = sigma2_a - k_a^T iK_a k_a.  This tool reuses gen_golden.py's placeholder modules and
reference model (its existing cases are untouched) and calls that function once per query point, for
48 points of a memory of N = 200:
  * 16 memory points (the variance cancels down to about the noise level),
  * 16 points drawn uniformly in the box of the memory inputs,
  * 16 points far outside it (var -> sigma2, mean -> 0).
Only data is written.  Re-run:  python tools/gen_golden_predict.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (installs the placeholders and imports the reference)

torch = G.torch


def query_points(w, seed):
    rng = np.random.default_rng(seed)
    X = w.X
    lo, hi = X.min(axis=0), X.max(axis=0)
    mem = X[rng.choice(X.shape[0], 16, replace=False)]
    box = lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(16, X.shape[1]))
    # far: every coordinate 20-50 box widths beyond the upper corner (time columns included)
    far = hi + (hi - lo) * rng.uniform(20.0, 50.0, size=(16, X.shape[1]))
    return np.concatenate([mem, box, far])


def predict_case(name, w, seed):
    m = G.ref_model(w)
    N, D, A, E, H, B = w.dims
    Xq = query_points(w, seed)
    zero = torch.zeros((E, E))
    Ms, Ss = [], []
    for x in Xq:
        Mt, S, _ = m.predict_next_state_change(torch.tensor(x), zero)
        Ms.append(Mt.numpy().reshape(D))
        Ss.append(S.numpy())
    d = G.inputs_dict(w)
    d.update(beta=m.beta.numpy(), iK=m.iK.numpy(), Xq=Xq, M=np.stack(Ms), S=np.stack(Ss),
             kind=np.repeat(np.arange(3), 16))          # 0 memory point, 1 inside the box, 2 far outside
    np.savez_compressed(os.path.join(G.OUT, name + ".npz"), **d)
    far_var = np.stack(Ss)[32:, range(D), range(D)]
    print(f"{name}: N={N} D={D} E={E} M[0]={Ms[0]}  far var / sigma2 - 1 = {np.abs(far_var / w.outputscales - 1).max():.1e}")


def main():
    os.makedirs(G.OUT, exist_ok=True)
    mk = G.synth.make_workload
    predict_case("predict_batch", mk(200, 3, 1, 2, 1, seed=60), seed=61)
    predict_case("predict_batch_time", mk(200, 3, 1, 2, 1, include_time=True, seed=62, time0=200.0), seed=63)


if __name__ == "__main__":
    main()
