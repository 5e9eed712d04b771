#!/usr/bin/env python3
"""Same-process A/B of the LAST layer's forward with every row stored against the kept rows only (ops.KEEP_LAST: scn_keep_mask +
scn_conv_forward_keep / scn_conv_forward_from_y_keep), alternating round by round on ONE complex and ONE set of tensors.

    python tools/keep_last_ab.py --data dense,sparse --rounds 4 --reps 2 [--form plain,from_y] [--hidden 32]
                                 [--libs parent=tools/ab/lib_parent.so,new=scone_gcn_amd/libscone_hip.so]

|E| = 996 634 and 32 slabs by default (one micro-batch of bench.py), seeded random last nodes.  Prints per (data, form, path) the
forward's mean time, the mask's two launches (memset + kernel, one timer key), per-round values and their spread, the share of
(block, slab) items kept, and whether the kept blocks and the readout's log-probabilities agree bit for bit with the full store.
--libs: library builds to compare (tools/ab_build_rev.sh makes the one of an earlier revision), a plan per build as in tools/ab_run.py:
the "kept" path then runs once per build, all paths alternating, and each build's kept rows are checked against the first build's
full store.  (The step-level A/B flips ops.KEEP_LAST around bench.py: tools/bench_switch.py.)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scone_gcn_amd import _lib, ops, synthetic_data_gen as g, trajectory_experiments as te   # noqa: E402
from scone_gcn_amd.complex import SimplicialComplex                                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--edges", type=int, default=1_000_000)
ap.add_argument("--slabs", type=int, default=32)
ap.add_argument("--hidden", type=int, default=32)
ap.add_argument("--data", default="dense,sparse")
ap.add_argument("--form", default="plain,from_y")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--libs", default="", help="name=path,... (paths relative to the repo root); default: the library of this tree alone")
a = ap.parse_args()

cx = g.random_SC_graph(g.calibrate_n_points(a.edges))
sc = SimplicialComplex(cx)
shifts, readout, _ = te.setup_from_complex(sc, "scone")
dev = ops.default_device()
builds = {}                               # name -> (library, its plan, the plan's node -> blocks tables)
for spec in a.libs.split(",") if a.libs else ["this=" + _lib.LIB_PATH]:
    name, path = spec.split("=")
    _lib._lib = None
    _lib.LIB_PATH = path if os.path.isabs(path) else os.path.join(ROOT, path)
    lib = _lib.load()
    p = ops.SconePlan(shifts[0], shifts[1], readout, "tanh", dev)
    builds[name] = (lib, p, p.field_tables_dev())
    assert builds[name][2] is not None, "the plan has no node -> blocks table"
    print("build %s: %s" % (name, _lib.LIB_PATH), flush=True)
first = next(iter(builds))
_, plan, tabs = builds[first]
E, C, S = cx.n_edges, a.hidden, a.slabs
torch.manual_seed(0)
W = [torch.randn(C, C, device=dev) * 0.1 for _ in range(3)]
Wf = [torch.randn(1, C, device=dev) * 0.3 for _ in range(3)]
w_last = torch.randn(C, 1, device=dev) * 0.3
last = torch.as_tensor(np.random.RandomState(1).randint(0, plan.n_nodes, size=S * ops.NS).astype(np.int32), device=dev)
row0 = torch.as_tensor(np.asarray(plan.conv.plan_blocks(), np.int64), device=dev)
blk_of = torch.searchsorted(row0, torch.arange(E, device=dev), right=True) - 1            # plan block of every row
print("|E| = %d, %d plan blocks, %d slabs, hidden %d" % (E, tabs.n_blocks, S, C), flush=True)


def forward(build, form, src, keep, out):
    lib, p, t = builds[build]
    _lib._lib = lib                       # (a plan's handles belong to the library that made them)
    mask = p.conv.keep_mask(last, ops.NS, p.n_nodes, t) if keep else None
    if form == "from_y":
        return p.conv.forward_from_y(src, Wf, W, "tanh", keep=mask, out=out)
    return p.conv.forward([src], W, C, "tanh", out=out, keep=mask)


def path(build, keep):
    return lambda form, src, out: forward(build, form, src, keep, out)


# the full store of the first build, then the kept path of every build
PATHS = {"full": path(first, False)}
PATHS.update({("kept" if len(builds) == 1 else "kept/" + n): path(n, True) for n in builds})
for data in a.data.split(","):
    for form in a.form.split(","):
        if form == "from_y" and C != 32:
            continue
        x = torch.randn(S, E, 4, 1 if form == "from_y" else C, device=dev)
        if data == "sparse":      # like the benchmark's tensors: ~5 % of the 64-row groups of a slab carry values, the rest exact zeros
            live = (torch.rand(S, (E + 63) // 64, device=dev) < 0.05).repeat_interleave(64, dim=1)[:, :E]
            x *= live[:, :, None, None]
        _lib._lib = builds[first][0]
        src = plan.conv.shifted_input(x) if form == "from_y" else x
        out = {n: torch.empty(S, E, 4, C, device=dev) for n in PATHS}
        ref = PATHS["full"](form, src, out["full"])
        assert ref is not None, "form not served"
        mask = plan.conv.keep_mask(last, ops.NS, plan.n_nodes, tabs)
        bits = (mask[:, torch.arange(S, device=dev) >> 5] >> (torch.arange(S, device=dev) & 31)) & 1      # [n_blocks][S]
        rows = bits.bool()[blk_of].T                                                                       # [S][E]
        ri, lp_ref = ref.view(torch.int32), plan.readout(ref, w_last, last)[0]
        for n in PATHS:
            if n == "full":
                continue
            out[n].view(torch.int32).fill_(0x7FC0DEAD)
            got = PATHS[n](form, src, out[n])
            assert got is not None, "form not served"
            torch.cuda.synchronize()
            _lib._lib = builds[first][0]
            gi = got.view(torch.int32)
            same_kept = bool((gi[rows] == ri[rows]).all())
            untouched = bool((gi[~rows] == 0x7FC0DEAD).all())
            same_logp = torch.equal(lp_ref.view(torch.int32), plan.readout(got, w_last, last)[0].view(torch.int32))
            print("%-6s %-6s %-11s kept items %.3f %% of (block, slab), rows %.3f %%; kept blocks agree bit for bit: %s; other rows "
                  "untouched: %s; logp agrees bit for bit: %s" % (data, form, n, 100.0 * float(bits.float().mean()),
                                                                  100.0 * float(rows.float().mean()), same_kept, untouched, same_logp),
                  flush=True)
            del got, gi
        del ref, rows, ri
        times = {n: {} for n in PATHS}
        names = list(PATHS)
        for r in range(a.rounds):
            for n in names[r % len(names):] + names[:r % len(names)]:      # rotate: no path always runs behind the same one
                with ops.KernelTimer() as kt:
                    for _ in range(a.reps):
                        PATHS[n](form, src, out[n])
                for k, (cnt, ms) in kt.summary().items():
                    times[n].setdefault(k, []).append(ms)
        base = None
        for n in names:
            tot = [sum(v[r] for v in times[n].values()) for r in range(a.rounds)]
            for k, v in times[n].items():
                print("%-6s %-6s %-11s %-22s %8.3f ms  spread %.3f  rounds: %s" % (data, form, n, k, sum(v) / len(v), max(v) - min(v),
                                                                                " ".join("%.3f" % t for t in v)), flush=True)
            mean = sum(tot) / len(tot)
            base = mean if base is None else base
            print("%-6s %-6s %-11s %-22s %8.3f ms  (%+.2f %% vs full)  spread %.3f" % (data, form, n, "all launches", mean,
                                                                                     100.0 * (mean / base - 1.0), max(tot) - min(tot)), flush=True)
        del x, src, out
        torch.cuda.empty_cache()
