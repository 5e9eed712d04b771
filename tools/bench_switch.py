#!/usr/bin/env python3
"""bench.py with a module switch of scone_gcn_amd.ops flipped first -- the step-level side of an A/B that bench.py has no flag for:

    python tools/bench_switch.py RECOMPUTE_FIRST=0 -- --gpus 1 --steps 10 --warmup 2

Everything after `--` goes to bench.py unchanged; the result line is bench.py's own."""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scone_gcn_amd import ops   # noqa: E402

sep = sys.argv.index("--") if "--" in sys.argv else len(sys.argv)
for spec in sys.argv[1:sep]:
    name, val = spec.split("=")
    assert isinstance(getattr(ops, name), bool), name
    setattr(ops, name, val not in ("0", "false", "False"))
    print("ops.%s = %s" % (name, getattr(ops, name)), file=sys.stderr, flush=True)
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[sep + 1:]
runpy.run_path(sys.argv[0], run_name="__main__")
