#!/usr/bin/env python3
"""Writes tests/golden/sparse_update_bits.npz: the BITS of beta_eff, of predict's mean and variance and the SHA-256 of iK_eff of
every run in tests/sparse_update_cases.py::RUNS, as computed by the build the fixture is to pin.

The fixture was written ONCE, on an MI355X, by the build that still had gpmpc_sparse_append and gpmpc_sparse_forget as two copies
of kernels, plan and driver: tests/test_gpu_sparse_update_bits.py asserts array_equal against it, so the one templated copy
(csrc/sparse_update.hip) and any later form of it has to keep every element's arithmetic and the order of every sum.
To regenerate it from another build:

  GPMPC_LIB=/path/to/that/libgpmpc_hip.so python tools/gen_sparse_update_golden.py [--out DIR]

from a checkout whose Python binding matches that library's ABI (this script and tests/sparse_update_cases.py use nothing but
prepare_sparse / sparse_append / sparse_forget / factors / predict).  Needs a GPU; never run by the test suite.

  python tools/gen_sparse_update_golden.py --check-inputs

needs no GPU: the float64 numpy restatement (tests/sparse_append_ref.py, tests/sparse_forget_ref.py) of the two large-M runs --
the build succeeds, the forget keeps its pivot, everything is finite.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sparse_update_cases as cases  # noqa: E402


def check_inputs():
    import sparse_append_ref as ar
    import sparse_forget_ref as fr
    import sparse_gp_ref as ref
    for name in cases.LARGE:
        c = cases.large_case(name)
        r = ar.build_record(c.X[:c.N - 1], c.Y[:c.N - 1], c.Z, c.ls, c.os, c.nz, ref.JITTER_REL)          # raises if not positive definite
        ar.append(r, c.X[c.N - 1:], c.Y[c.N - 1:])
        fr.forget(r, c.X[:1], c.Y[:1])                                                                     # raises LostPivot
        mean, var = ref.predict(c.Z, c.ls, c.os, r.iK, r.beta(), c.Xq)
        for v in (r.Yu, r.Yb, r.w, r.iK, mean, var):
            assert np.all(np.isfinite(v)), name
        floor = 1.0 / (2.0 * (1.0 + c.os[0] / c.nz[0]))
        print(f"{name}: M = {c.M}, tau of the forget {r.min_tau:.3e} (floor {floor:.3e}), max |Yu| {np.max(np.abs(r.Yu)):.3e}, "
              f"mean in [{mean.min():.3f}, {mean.max():.3f}], var in [{var.min():.3e}, {var.max():.3e}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--check-inputs", action="store_true")
    args = ap.parse_args()
    if args.check_inputs:
        return check_inputs()
    import gp_mpc_amd
    from gp_mpc_amd import _lib
    eng = gp_mpc_amd.HipEngine(0)
    t0 = time.perf_counter()
    res = cases.run_all(eng)
    print(f"run_all: {time.perf_counter() - t0:.1f} s (with the numpy references of the cases)")
    eng.close()
    data = {"runs": np.array(cases.RUNS), "build_id": np.array(_lib.lib().gpmpc_build_id().decode())}
    for name in cases.LARGE:
        data[f"X_sum/{name}"] = np.array(cases.large_case(name).X.sum())                 # the inputs' checksum: same synthetic memory
    for key, o in res.items():
        for f in ("beta", "mean", "var"):
            assert np.all(np.isfinite(o[f])), (key, f, "non-finite: not a run worth pinning")
        for f, v in o.items():
            data[f"{f}/{key}"] = v
        print(f"{key}: beta[0, 0] = {o['beta'][0, 0]!r}, iK_eff {str(o['iK_sha256'])[:16]}")
    print("lost pivot:", int(res["lost_pivot"]["code"]), str(res["lost_pivot"]["message"]))
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "sparse_update_bits.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes; build", data["build_id"])


if __name__ == "__main__":
    main()
