#!/usr/bin/env python3
"""Writes tests/golden/search_bits.npz: the BITS of every result in tests/search_bits_cases.py::run_all, as computed by the build
the fixture is to pin.

The fixture was written ONCE, on an MI355X, by the build of commit d975212 ("Controller: candidate searches behind one table and
one skeleton"): the last one with two copies of the bitonic sort, of the refit and of the action mapper, and with the CEM
mapper's parameters uploaded into its workspace.  tests/test_gpu_search_bits.py asserts array_equal against it, so any later form
of the searches' shared code has to keep every element's arithmetic and the order of every sum.  To regenerate it from another
build:

  GPMPC_LIB=/path/to/that/libgpmpc_hip.so python tools/gen_search_bits_golden.py [--out DIR]

from a checkout whose Python binding matches that library's ABI.  Needs a GPU; never run by the test suite.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import search_bits_cases as cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    import gp_mpc_amd
    from gp_mpc_amd import _lib
    eng = gp_mpc_amd.HipEngine(0)
    res = cases.run_all(eng)
    eng.close()
    data = {"keys": np.array(cases.KEYS), "build_id": np.array(_lib.lib().gpmpc_build_id().decode())}
    for (A, H) in cases.MODELS:
        data[f"actions_sum_A{A}_H{H}"] = np.array(cases.make_case(A, H).actions.sum())      # the inputs' checksum: same synthetic workload
    for key in cases.KEYS:
        for name, v in res[key].items():
            data[f"{key}/{name}"] = v
        o = res[key]            # the run's leading objective: best J, the winner record's first entry, or the merged state's last
        J = o["best_J"][0] if "best_J" in o else o["winner"].ravel()[0] if "winner" in o else o[f"state_it{cases.SHARD_ITERS - 1}"][-1]
        assert np.isfinite(J), (key, "non-finite: not a run worth pinning")
        print(f"{key}: J = {float(J)!r}")
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "search_bits.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes; build", data["build_id"])


if __name__ == "__main__":
    main()
