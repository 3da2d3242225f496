#!/usr/bin/env python3
"""Writes tests/golden/step_tail_costs.npz: the BITS of J, cost_mu and cost_var of the shapes in
tests/step_tail_cases.py::GOLDEN_CASES, as computed by the build the fixture is to pin.

The fixture was written ONCE, on an MI355X, by the build that preceded the register form of the cost kernel (every operand
a global load inside run-time loops): tests/test_gpu_step_tail.py::test_cost_bits_pinned asserts array_equal against it, so
any later form of traj_cost_body has to keep the operations and their order.  To regenerate it from another build:

  GPMPC_LIB=/path/to/that/libgpmpc_hip.so python tools/gen_step_tail_golden.py [--out DIR]

from a checkout whose Python binding matches that library's ABI (this script and tests/step_tail_cases.py use nothing but
prepare / set_cost / rollout, so they run unchanged in an older checkout).  Needs a GPU; never run by the test suite.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import step_tail_cases as cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    import gp_mpc_amd
    from gp_mpc_amd import _lib
    eng = gp_mpc_amd.HipEngine(0)
    data = {"cases": np.array([[int(v) for v in c] for c in cases.GOLDEN_CASES], dtype=np.int64),
            "build_id": np.array(_lib.lib().gpmpc_build_id().decode())}
    for k, (D, A, H, B, clip, cons, tim) in enumerate(cases.GOLDEN_CASES):
        w, _, _, out = cases.run_case(eng, D, A, H, B, clip, cons, tim)
        data[f"seed_{k}"] = np.array(cases.case_seed(D, A, H, B), dtype=np.int64)
        data[f"actions_sum_{k}"] = np.array(w.actions.sum())          # the inputs' checksum: same synthetic workload
        for name in ("J", "cost_mu", "cost_var"):
            data[f"{name}_{k}"] = out[name].cpu().numpy().copy()
        assert np.all(np.isfinite(data[f"J_{k}"])), (k, "non-finite objective: not a shape worth pinning")
        print(f"case {k} {(D, A, H, B, clip, cons, tim)}: J[0] = {data[f'J_{k}'][0]!r}")
    eng.close()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "step_tail_costs.npz")
    np.savez(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes; build", data["build_id"])


if __name__ == "__main__":
    main()
