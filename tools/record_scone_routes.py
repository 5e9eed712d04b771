#!/usr/bin/env python3
"""Writes the scone route table: which launches one training step of every case of tests/scone_route_cases.py makes and what the
forward's record says (one MI355X, seconds).

    python tools/record_scone_routes.py --out tests/golden/scone_routes.json

Run on the revision whose routes are to be pinned; tests/test_gpu_scone_routes.py then holds later trees to the table.  Two runs on one
revision must write the same bytes: a case that does not is no pin and leaves the case list."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.scone_route_cases import CASES, observe   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
a = ap.parse_args()
table = {}
for case in CASES:
    table[case["name"]] = observe(case)
    print("%-40s %s" % (case["name"], " | ".join("%s x%d" % (k, n) for k, (n, _) in table[case["name"]]["launches"].items())), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(table, f, indent=1, sort_keys=True)
    f.write("\n")
