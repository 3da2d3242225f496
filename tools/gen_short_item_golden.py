#!/usr/bin/env python3
"""Writes tests/golden/short_item_bits.npz: the BITS of mu, Sig and J of every run in tests/short_item_cases.py::RUNS, as computed
by the build the fixture is to pin.

The fixture was written ONCE, on an MI355X, by the build that preceded the LDS-typed, scalar-argument separable items and the
one-pass mean sums (csrc/rollout_kernel.h); its `build_id` names that build.  (Its runs with X^T in global memory are there for
the per-point pass, whose X reads a dropped stage of that change had typed.)
tests/test_gpu_short_item_bits.py asserts array_equal against it, so any later form of these items has to keep every
floating-point operation, its order and the slot of every result.  To regenerate it from another build:

  GPMPC_LIB=/path/to/that/libgpmpc_hip.so python tools/gen_short_item_golden.py [--out DIR]

from a checkout whose Python binding matches that library's ABI (this script and tests/short_item_cases.py use nothing but
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
import short_item_cases as cases  # noqa: E402


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
        data["actions_sum_N%d_tm%d_s%d" % case] = np.array(cases.make_case(*case).actions.sum())      # the inputs' checksum
    for key, o in res.items():
        for name in ("mu", "Sig", "J"):
            assert np.all(np.isfinite(o[name])), (key, name, "non-finite: not a run worth pinning")
            data[f"{name}/{key}"] = o[name]
        print(f"{key}: J[0] = {o['J'][0]!r}")
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "short_item_bits.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes; build", data["build_id"])


if __name__ == "__main__":
    main()
