#!/usr/bin/env python3
"""Same-process A/B of the LAST layer's forward with every row stored against the kept rows only (ops.KEEP_LAST: scn_keep_mask +
scn_conv_forward_keep / scn_conv_forward_from_y_keep), alternating round by round on ONE complex and ONE set of tensors.

    python tools/keep_last_ab.py --data dense,sparse --rounds 4 --reps 2 [--form plain,from_y] [--hidden 32]

|E| = 996 634 and 32 slabs by default (one micro-batch of bench.py), seeded random last nodes.  Prints per (data, form, path) the
forward's mean time, the mask's two launches (memset + kernel, one timer key), per-round values and their spread, the share of
(block, slab) items kept, and whether the kept blocks and the readout's log-probabilities agree bit for bit with the full store.
(The step-level A/B flips ops.KEEP_LAST around bench.py: tools/bench_switch.py.)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scone_gcn_amd import ops, synthetic_data_gen as g, trajectory_experiments as te   # noqa: E402
from scone_gcn_amd.complex import SimplicialComplex                                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--edges", type=int, default=1_000_000)
ap.add_argument("--slabs", type=int, default=32)
ap.add_argument("--hidden", type=int, default=32)
ap.add_argument("--data", default="dense,sparse")
ap.add_argument("--form", default="plain,from_y")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--reps", type=int, default=2)
a = ap.parse_args()

cx = g.random_SC_graph(g.calibrate_n_points(a.edges))
sc = SimplicialComplex(cx)
shifts, readout, _ = te.setup_from_complex(sc, "scone")
dev = ops.default_device()
plan = ops.SconePlan(shifts[0], shifts[1], readout, "tanh", dev)
tabs = plan.field_tables_dev()
assert tabs is not None, "the plan has no node -> blocks table"
E, C, S = cx.n_edges, a.hidden, a.slabs
torch.manual_seed(0)
W = [torch.randn(C, C, device=dev) * 0.1 for _ in range(3)]
Wf = [torch.randn(1, C, device=dev) * 0.3 for _ in range(3)]
w_last = torch.randn(C, 1, device=dev) * 0.3
last = torch.as_tensor(np.random.RandomState(1).randint(0, plan.n_nodes, size=S * ops.NS).astype(np.int32), device=dev)
row0 = torch.as_tensor(np.asarray(plan.conv.plan_blocks(), np.int64), device=dev)
blk_of = torch.searchsorted(row0, torch.arange(E, device=dev), right=True) - 1            # plan block of every row
print("|E| = %d, %d plan blocks, %d slabs, hidden %d" % (E, tabs.n_blocks, S, C), flush=True)


def forward(form, src, keep, out):
    if form == "from_y":
        return plan.conv.forward_from_y(src, Wf, W, "tanh", keep=keep, out=out)
    return plan.conv.forward([src], W, C, "tanh", out=out, keep=keep)


def full(form, src, out):
    return forward(form, src, None, out)


def kept(form, src, out):
    return forward(form, src, plan.conv.keep_mask(last, ops.NS, plan.n_nodes, tabs), out)


PATHS = {"full": full, "kept": kept}
for data in a.data.split(","):
    for form in a.form.split(","):
        if form == "from_y" and C != 32:
            continue
        x = torch.randn(S, E, 4, 1 if form == "from_y" else C, device=dev)
        if data == "sparse":      # like the benchmark's tensors: ~5 % of the 64-row groups of a slab carry values, the rest exact zeros
            live = (torch.rand(S, (E + 63) // 64, device=dev) < 0.05).repeat_interleave(64, dim=1)[:, :E]
            x *= live[:, :, None, None]
        src = plan.conv.shifted_input(x) if form == "from_y" else x
        out = {n: torch.empty(S, E, 4, C, device=dev) for n in PATHS}
        out["kept"].view(torch.int32).fill_(0x7FC0DEAD)
        ref, got = full(form, src, out["full"]), kept(form, src, out["kept"])
        assert ref is not None and got is not None, "form not served"
        mask = plan.conv.keep_mask(last, ops.NS, plan.n_nodes, tabs)
        bits = (mask[:, torch.arange(S, device=dev) >> 5] >> (torch.arange(S, device=dev) & 31)) & 1      # [n_blocks][S]
        rows = bits.bool()[blk_of].T                                                                       # [S][E]
        torch.cuda.synchronize()
        gi, ri = got.view(torch.int32), ref.view(torch.int32)
        same_kept = bool((gi[rows] == ri[rows]).all())
        untouched = bool((gi[~rows] == 0x7FC0DEAD).all())
        lp_ref, lp_got = plan.readout(ref, w_last, last)[0], plan.readout(got, w_last, last)[0]
        same_logp = torch.equal(lp_ref.view(torch.int32), lp_got.view(torch.int32))
        print("%-6s %-6s kept items %.3f %% of (block, slab), rows %.3f %%; kept blocks agree bit for bit: %s; other rows untouched: %s; "
              "logp agrees bit for bit: %s" % (data, form, 100.0 * float(bits.float().mean()), 100.0 * float(rows.float().mean()),
                                               same_kept, untouched, same_logp), flush=True)
        del ref, got, rows, gi, ri
        times = {n: {} for n in PATHS}
        names = list(PATHS)
        for r in range(a.rounds):
            for n in names[r % 2:] + names[:r % 2]:
                with ops.KernelTimer() as kt:
                    for _ in range(a.reps):
                        PATHS[n](form, src, out[n])
                for k, (cnt, ms) in kt.summary().items():
                    times[n].setdefault(k, []).append(ms)
        base = None
        for n in names:
            tot = [sum(v[r] for v in times[n].values()) for r in range(a.rounds)]
            for k, v in times[n].items():
                print("%-6s %-6s %-5s %-22s %8.3f ms  spread %.3f  rounds: %s" % (data, form, n, k, sum(v) / len(v), max(v) - min(v),
                                                                                " ".join("%.3f" % t for t in v)), flush=True)
            mean = sum(tot) / len(tot)
            base = mean if base is None else base
            print("%-6s %-6s %-5s %-22s %8.3f ms  (%+.2f %% vs full)  spread %.3f" % (data, form, n, "all launches", mean,
                                                                                     100.0 * (mean / base - 1.0), max(tot) - min(tot)), flush=True)
        del x, src, out
        torch.cuda.empty_cache()
