#!/usr/bin/env python3
"""Same-process A/B of the three launches the first layer's output H1 touches -- layer 1, layer 2's forward, layer 2's fused-first
backward -- with H1 stored (forward_first + forward + backward_fused_first on aux) against H1 rebuilt from the shifted-input records
(shifted_input + forward_from_y + backward_fused_first without aux), alternating round by round on ONE complex and ONE set of tensors.

    python tools/recompute_first_ab.py --data dense,sparse --rounds 4 --reps 2

Prints per (data, path) every launch's mean time, the three-launch sum per round and its spread, and whether the outputs agree bit
for bit.  (The step-level A/B flips ops.RECOMPUTE_FIRST around bench.py: tools/bench_switch.py.)"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scone_gcn_amd import ops, synthetic_data_gen as g, trajectory_experiments as te   # noqa: E402
from scone_gcn_amd.complex import SimplicialComplex                                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--edges", type=int, default=1_000_000)
ap.add_argument("--slabs", type=int, default=32)
ap.add_argument("--data", default="dense,sparse")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--reps", type=int, default=2)
a = ap.parse_args()

cx = g.random_SC_graph(g.calibrate_n_points(a.edges))
sc = SimplicialComplex(cx)
shifts, readout, _ = te.setup_from_complex(sc, "scone")
dev = ops.default_device()
plan = ops.SconePlan(shifts[0], shifts[1], readout, "tanh", dev)
E, C, S = cx.n_edges, 32, a.slabs
torch.manual_seed(0)
W = [torch.randn(C, C, device=dev) * 0.1 for _ in range(3)]
Wf = [torch.randn(1, C, device=dev) * 0.3 for _ in range(3)]


def stored(x, dz):
    H1, y = plan.conv.forward_first(x, Wf, C, "tanh")
    H2 = plan.conv.forward([H1], W, C, "tanh")
    dW, dW1 = [torch.zeros_like(w) for w in W], [torch.zeros_like(w) for w in Wf]
    assert plan.conv_T.backward_fused_first(dz, W, H1, "tanh", y, dW, dW1)
    return [H2] + dW + dW1


def rebuilt(x, dz):
    y = plan.conv.shifted_input(x)
    H2 = plan.conv.forward_from_y(y, Wf, W, "tanh")
    dW, dW1 = [torch.zeros_like(w) for w in W], [torch.zeros_like(w) for w in Wf]
    assert plan.conv_T.backward_fused_first(dz, W, None, "tanh", y, dW, dW1, Ws_first=Wf)
    return [H2] + dW + dW1


PATHS = {"stored": stored, "rebuilt": rebuilt}
for data in a.data.split(","):
    x = torch.randn(S, E, 4, 1, device=dev)
    dz = torch.randn(S, E, 4, C, device=dev)
    if data == "sparse":      # like the benchmark's tensors: ~5 % of the 64-row groups of a slab carry values, the rest exact zeros
        keep = (torch.rand(S, (E + 63) // 64, device=dev) < 0.05).repeat_interleave(64, dim=1)[:, :E]
        x *= keep[:, :, None, None]
        keep = (torch.rand(S, (E + 63) // 64, device=dev) < 0.05).repeat_interleave(64, dim=1)[:, :E]
        dz *= keep[:, :, None, None]
    ref = stored(x, dz)
    got = rebuilt(x, dz)
    torch.cuda.synchronize()
    same = all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(ref, got))
    print("%-6s outputs of the two paths agree bit for bit: %s" % (data, same), flush=True)
    del ref, got
    torch.cuda.empty_cache()
    sums = {n: [] for n in PATHS}
    parts = {n: {} for n in PATHS}
    names = list(PATHS)
    for r in range(a.rounds):
        for n in names[r % 2:] + names[:r % 2]:
            with ops.KernelTimer() as kt:
                for _ in range(a.reps):
                    PATHS[n](x, dz)
            tot = 0.0
            for k, (cnt, ms) in kt.summary().items():
                parts[n].setdefault(k, []).append(ms)
                tot += ms
            sums[n].append(tot)
            torch.cuda.empty_cache()
    for n in names:
        for k, v in parts[n].items():
            print("%-6s %-8s %-34s %8.3f ms" % (data, n, k, sum(v) / len(v)), flush=True)
    base = sum(sums["stored"]) / len(sums["stored"])
    for n in names:
        t = sums[n]
        mean = sum(t) / len(t)
        print("%-6s %-8s three-launch sum %8.3f ms (%+.2f %% vs stored)  spread %.3f  rounds: %s"
              % (data, n, mean, 100.0 * (mean / base - 1.0), max(t) - min(t), " ".join("%.3f" % v for v in t)), flush=True)
    del x, dz
    torch.cuda.empty_cache()
