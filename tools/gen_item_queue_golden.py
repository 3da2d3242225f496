#!/usr/bin/env python3
"""Writes tests/golden/item_queue_bits.npz: the BITS of mu, Sig and J of every run in tests/item_queue_cases.py::RUNS, as computed
by the build the fixture is to pin.

The fixture was written ONCE, on an MI355X, by the build that preceded the per-entry descriptors and the claim-ahead pull of the
pairwise work queue (csrc/rollout_kernel.h); its `build_id` names that build.  tests/test_gpu_item_queue_bits.py asserts
array_equal against it, so any later form of the queue has to keep every item's arithmetic, the slot of its result and the order
of every sum.  To regenerate it from another build:

  GPMPC_LIB=/path/to/that/libgpmpc_hip.so python tools/gen_item_queue_golden.py [--out DIR]

from a checkout whose Python binding matches that library's ABI (this script and tests/item_queue_cases.py use nothing but
prepare / set_cost / set_option / rollout and the last_* properties).  Every run has to be the fused-horizon kernel's
(last_rollout_path == 0) in the form and with the number of pair groups it names: cases.run_all asserts that.  Needs a GPU; never
run by the test suite.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import item_queue_cases as cases  # noqa: E402


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
    for (N, D, tm) in cases.CASES:
        data[f"actions_sum_N{N}_D{D}_tm{tm}"] = np.array(cases.make_case(N, D, tm).actions.sum())      # the inputs' checksum
    for key, o in res.items():
        for name in ("mu", "Sig", "J"):
            assert np.all(np.isfinite(o[name])), (key, name, "non-finite: not a run worth pinning")
            data[f"{name}/{key}"] = o[name]
        print(f"{key}: J[0] = {o['J'][0]!r}")
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "item_queue_bits.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes; build", data["build_id"])


if __name__ == "__main__":
    main()
