#!/usr/bin/env python3
"""Writes tests/golden/step_chain_bits.npz: the BITS of mu, Sig and J of every run in tests/step_chain_cases.py::RUNS, as computed
by the build the fixture is to pin.

The fixture was written ONCE, on an MI355X, by the kernel that preceded the merge of a horizon step's serial chain (pair totals,
M and V, state update, the next step's small algebra) into one loop trip with fewer workgroup barriers -- the parent commit's
csrc/rollout_kernel.h, built together with the read-only query gpmpc_last_pair_groups the runs assert on (host code only).
tests/test_gpu_step_chain_bits.py asserts array_equal against it, so any later form of the chain has to keep every operation and
the order of every sum.  To regenerate it from another build:

  GPMPC_LIB=/path/to/that/libgpmpc_hip.so python tools/gen_step_chain_golden.py [--out DIR]

from a checkout whose Python binding matches that library's ABI.  Needs a GPU; never run by the test suite.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import step_chain_cases as cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    import gp_mpc_amd
    from gp_mpc_amd import _lib
    eng = gp_mpc_amd.HipEngine(0)
    res = cases.run_all(eng)
    eng.close()
    data = {"runs": np.array(cases.RUNS, dtype=np.int64), "build_id": np.array(_lib.lib().gpmpc_build_id().decode())}
    for case in cases.CASES:
        data["actions_sum_N%d_D%d_H%d_tm%d" % case] = np.array(cases.make_case(*case).actions.sum())      # the inputs' checksum
    for key, o in res.items():
        for name in ("mu", "Sig", "J"):
            assert np.all(np.isfinite(o[name])), (key, name, "non-finite: not a run worth pinning")
            data[f"{name}/{key}"] = o[name]
        print(f"{key}: groups {o['groups']} J[0] = {o['J'][0]!r}")
    for run in cases.MULTI_GROUP_RUNS:
        assert res[cases.run_key(run)]["groups"] > 1, (run, "meant to walk several pair groups")
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "step_chain_bits.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes; build", data["build_id"])


if __name__ == "__main__":
    main()
