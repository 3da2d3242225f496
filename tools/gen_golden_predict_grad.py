#!/usr/bin/env python3
"""Generate tests/golden/predict_grad_batch*.npz by EXECUTING THE REFERENCE'S OWN CODE under torch autograd (this container only).

The reverse-mode product of the GP posterior at deterministic query inputs that gpmpc_predict_backward computes: the reference's
predict_next_state_change (gp_model.py:112-180) at zero input variance gives M = k^T beta and a diagonal S with
S_aa = sigma2_a - k_a^T iK_a k_a, and autograd through it with respect to the input mean is the gradient of the posterior.  This
tool reuses gen_golden.py's placeholder modules and reference model and gen_golden_predict.py's workloads and 48 query points
(memory points, points inside the input box, far points), and asserts that the rebuilt M and S equal the committed
predict_batch*.npz bit for bit (the model of each file is the one of the matching forward golden).  Every query gets three
seeded upstream sets: 0 mean_bar and var_bar; 1 mean_bar only; 2 var_bar only.  For each it stores the gradient of
<mean_bar, M> + sum_a var_bar_a S_aa with respect to the query.  Only the queries, the upstream vectors and the gradients are
written (the model is the forward golden's).  Re-run:  python tools/gen_golden_predict_grad.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (installs the placeholders and imports the reference)
import gen_golden_predict as GP  # noqa: E402

torch = G.torch


def grad_case(name, fwd_name, w, seed, up_seed):
    m = G.ref_model(w)
    N, D, A, E, H, B = w.dims
    Xq = GP.query_points(w, seed)
    ref = np.load(os.path.join(G.OUT, fwd_name + ".npz"))
    assert np.array_equal(ref["Xq"], Xq)
    rng = np.random.default_rng(up_seed)
    Mq = len(Xq)
    mean_bar = rng.standard_normal((3, Mq, D))
    var_bar = rng.standard_normal((3, Mq, D))
    var_bar[1] = 0.0
    mean_bar[2] = 0.0
    Xq_bar = np.zeros((3, Mq, E))
    zero = torch.zeros((E, E))
    for p in range(Mq):
        for s in range(3):
            x = torch.tensor(Xq[p], requires_grad=True)
            Mt, S, _ = m.predict_next_state_change(x, zero)
            if s == 0:
                assert np.array_equal(Mt.detach().numpy().reshape(D), ref["M"][p]) and np.array_equal(S.detach().numpy(), ref["S"][p])
            loss = (torch.tensor(mean_bar[s, p]) * Mt.reshape(D)).sum() + (torch.tensor(var_bar[s, p]) * torch.diagonal(S)).sum()
            loss.backward()
            Xq_bar[s, p] = x.grad.numpy()
    np.savez_compressed(os.path.join(G.OUT, name + ".npz"), Xq=Xq, kind=ref["kind"], mean_bar=mean_bar, var_bar=var_bar,
                        Xq_bar=Xq_bar)
    print(f"{name}: M={Mq} N={N} D={D} E={E}  max|Xq_bar| = {np.abs(Xq_bar).max():.3e}  far max = {np.abs(Xq_bar[:, 32:]).max():.1e}")


def main():
    mk = G.synth.make_workload
    grad_case("predict_grad_batch", "predict_batch", mk(200, 3, 1, 2, 1, seed=60), seed=61, up_seed=64)
    grad_case("predict_grad_batch_time", "predict_batch_time", mk(200, 3, 1, 2, 1, include_time=True, seed=62, time0=200.0),
              seed=63, up_seed=65)


if __name__ == "__main__":
    main()
