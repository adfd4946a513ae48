#!/usr/bin/env python3
"""Record tests/golden/plan_shapes.json: what the host planner of a given
libmpc.so answers over the shape grid of tests/plan_shapes.py (plan info, the
parse tables as CRC-32, workspace bytes, offset and count of every MPC_BUF_*,
code and message of every error case).  Needs no GPU.  Run it on the commit
whose planner is the reference, BEFORE changing the planner:
  python3 scripts/make_plan_golden.py [--lib path/to/libmpc.so]"""
import argparse
import importlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import plan_shapes as ps  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", help="libmpc.so to record from (default: the in-tree build)")
a = ap.parse_args()
engine = importlib.import_module("minion-plasmid-consensus_amd.engine")
if a.lib:
    engine.set_library(os.path.abspath(a.lib))
limit = ps.bisect_lds_limit(engine)
fx = {"lds_limit": limit,
      "cases": {c["name"]: ps.record(engine, c) for c in ps.cases(limit)},
      "errors": {c["name"]: ps.record(engine, c) for c in ps.error_cases()}}
with open(ps.FIXTURE, "w") as f:
    json.dump(fx, f, indent=0, separators=(",", ":"), sort_keys=True)
    f.write("\n")
print("%s: %d cases, %d error cases, lds_limit %d" % (ps.FIXTURE, len(fx["cases"]), len(fx["errors"]), limit))
