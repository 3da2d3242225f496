#!/usr/bin/env python3
"""Writes tests/golden/engine_calls.json: what every case of tests/engine_call_cases.py::CASES makes engine.py hand to the C ABI
-- the function called, integers and floats by value, pointers by role, the returned keys, shapes and dtypes, the text of
every ValueError -- as recorded from the checkout the fixture is to pin.

The fixture was written ONCE, by the engine.py that still had one copy of each wrapper per entry point:
tests/test_engine_marshalling.py asserts equality against it, so the shared helpers behind `rollout*`, `moments*` and
`predict*` and any later form of them have to make the same calls.  To regenerate it from another checkout:

  python tools/gen_engine_calls_golden.py [--out DIR]

Needs no GPU (the library is loaded, never called); never run by the test suite.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import engine_call_cases as cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    res = cases.run_all()
    for cid, rec in res.items():
        assert '"?"' not in json.dumps(rec), (cid, "a pointer whose role the record cannot name")
    n_calls = sum(len(r["calls"]) for r in res.values())
    n_raise = sum("raises" in r for r in res.values())
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "engine_calls.json")
    with open(path, "w") as fh:
        # one case per line
        fh.write("{\n" + ",\n".join(f"{json.dumps(cid)}: {json.dumps(res[cid], sort_keys=True)}" for cid in sorted(res)) + "\n}\n")
    print(f"wrote {path}: {len(res)} cases, {n_calls} calls, {n_raise} ValueErrors, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
