#!/usr/bin/env python3
"""Writes tests/golden/controller_search_traces.json: what every case of tests/controller_search_cases.py::CASES makes
GpMpcController._get_optimal_actions do -- the ordered engine and model calls with their arguments, the next draw of numpy's
global generator, the returned action, the attributes left on the controller -- as recorded from the checkout the fixture is
to pin.

The fixture was written ONCE, on the CPU, from the gp_mpc_controller.py of commit 60a19cf2e63da93e40081bfb387fe70e3bc5064e,
which still held the seven candidate searches inline, before any product file was edited:
tests/test_controller_search_traces.py compares against it, so control_objects/controllers/candidate_search.py and any later
form of the searches have to make the same calls, take the same draws and leave the same attributes.  To regenerate it from
another checkout:

  python tools/gen_controller_search_golden.py [--out DIR]

Needs no GPU and no built library; never run by the test suite.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import controller_search_cases as cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    res = cases.run_all()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "controller_search_traces.json")
    with open(path, "w") as fh:
        # one case per line
        fh.write("{\n" + ",\n".join(f"{json.dumps(cid)}: {json.dumps(res[cid], sort_keys=True)}" for cid in cases.IDS) + "\n}\n")
    print(f"wrote {path}: {len(res)} cases, {sum(len(r['calls']) for r in res.values())} calls, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
