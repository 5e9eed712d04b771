#!/usr/bin/env python3
"""Same-process A/B of the TOP layer's backward with the readout gradient staged everywhere against staged only where the readout
wrote it (ops.TOP_DZ_MASK: scn_keep_mask + scn_mask_hop + scn_conv_backward_dzmask), alternating round by round on ONE complex and
ONE set of tensors.

    python tools/top_dz_mask_ab.py --data sparse,dense --rounds 4 --reps 2

|E| = 996 634 and 32 slabs by default (one micro-batch of bench.py), seeded random last nodes; dz is what scn_readout_backward
leaves in an all-zero buffer for them.  `data` is the aux tensor (the layer's input): sparse like the benchmark's, or dense random.
Times are HIP events around every launch (ops.KernelTimer).  Prints per (data, path) the backward's mean time, the mask's launches
(memset + mask kernel under one key, the hop under another), per-round values and their spread, the share of (block, slab) items in
M0 and in the hopped mask, and whether dx and the weight gradients agree bit for bit with the plain call.
(The step-level A/B flips ops.TOP_DZ_MASK around bench.py: tools/bench_switch.py.)"""
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
ap.add_argument("--data", default="sparse,dense")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--reps", type=int, default=2)
a = ap.parse_args()

cx = g.random_SC_graph(g.calibrate_n_points(a.edges))
sc = SimplicialComplex(cx)
shifts, readout, _ = te.setup_from_complex(sc, "scone")
dev = ops.default_device()
plan = ops.SconePlan(shifts[0], shifts[1], readout, "tanh", dev)
tabs = plan.field_tables_dev()
assert tabs is not None, "the plan has no block tables"
assert plan.conv_T is plan.conv, "the shifts are symmetric"
E, C, S = cx.n_edges, 32, a.slabs
torch.manual_seed(0)
W = [torch.randn(C, C, device=dev) * 0.1 for _ in range(3)]
w_last = torch.randn(C, 1, device=dev) * 0.3
last = torch.as_tensor(np.random.RandomState(1).randint(0, plan.n_nodes, size=S * ops.NS).astype(np.int32), device=dev)
print("|E| = %d, %d plan blocks, %d slabs, hidden %d" % (E, tabs.n_blocks, S, C), flush=True)


def share(mask):
    bits = (mask[:, torch.arange(S, device=dev) >> 5] >> (torch.arange(S, device=dev) & 31)) & 1      # [n_blocks][S]
    return 100.0 * float(bits.float().mean())


m0 = plan.conv.keep_mask(last, ops.NS, plan.n_nodes, tabs)
print("items in M0 %.3f %% of (block, slab), in the hopped mask %.3f %%" % (share(m0), share(plan.conv.mask_hop(m0, tabs))), flush=True)

# the readout gradient of these last nodes, into an all-zero buffer (SconePlan._readout_grad: the pooled path)
H = torch.tanh(torch.randn(S, E, 4, C, device=dev))
logp, bh = plan.readout(H, w_last, last)[:2]
dz = plan._readout_grad(H, bh, logp, torch.randn_like(logp), last, [w_last], [torch.zeros_like(w_last)])
del H
torch.cuda.synchronize()
print("dz: %.4f %% of the values are non-zero" % (100.0 * float((dz != 0).float().mean())), flush=True)


def plain(aux, dx, dW):
    return plan.conv_T.backward([dz], W, aux, "tanh", True, dW, dx=dx)


def masked(aux, dx, dW):
    mask = plan.conv.mask_hop(plan.conv.keep_mask(last, ops.NS, plan.n_nodes, tabs, key="dz_mask"), tabs)
    got = plan.conv_T.backward([dz], W, aux, "tanh", True, dW, dx=dx, dz_mask=mask)
    assert got is not False, "masked backward not served"
    return got


PATHS = {"plain": plain, "masked": masked}
for data in a.data.split(","):
    aux = torch.tanh(torch.randn(S, E, 4, C, device=dev))
    if data == "sparse":      # like the benchmark's tensors: ~5 % of the 64-row groups of a slab carry values, the rest exact zeros
        live = (torch.rand(S, (E + 63) // 64, device=dev) < 0.05).repeat_interleave(64, dim=1)[:, :E]
        aux *= live[:, :, None, None]
    dx = {n: torch.empty(S, E, 4, C, device=dev) for n in PATHS}
    dW = {n: [torch.zeros(C, C, device=dev) for _ in range(3)] for n in PATHS}
    for n in PATHS:
        PATHS[n](aux, dx[n], dW[n])
    torch.cuda.synchronize()
    same_dx = torch.equal(dx["plain"].view(torch.int32), dx["masked"].view(torch.int32))
    same_dw = all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(dW["plain"], dW["masked"]))
    print("%-6s dx agrees bit for bit: %s; dW agrees bit for bit: %s; |dW| max %.3g" % (data, same_dx, same_dw,
                                                                                      max(float(t.abs().max()) for t in dW["plain"])), flush=True)
    times = {n: {} for n in PATHS}
    names = list(PATHS)
    for r in range(a.rounds):
        for n in names[r % 2:] + names[:r % 2]:
            with ops.KernelTimer() as kt:
                for _ in range(a.reps):
                    PATHS[n](aux, dx[n], dW[n])
            for k, (cnt, ms) in kt.summary().items():
                times[n].setdefault(k, []).append(ms)
    base = None
    for n in names:
        tot = [sum(v[r] for v in times[n].values()) for r in range(a.rounds)]
        for k, v in times[n].items():
            print("%-6s %-6s %-22s %8.3f ms  spread %.3f  rounds: %s" % (data, n, k, sum(v) / len(v), max(v) - min(v),
                                                                          " ".join("%.3f" % t for t in v)), flush=True)
        mean = sum(tot) / len(tot)
        base = mean if base is None else base
        print("%-6s %-6s %-22s %8.3f ms  (%+.2f %% vs plain)  spread %.3f" % (data, n, "all launches", mean, 100.0 * (mean / base - 1.0),
                                                                               max(tot) - min(tot)), flush=True)
    del aux, dx
    torch.cuda.empty_cache()
