#!/usr/bin/env python3
"""What the six masked launches of a readout-cone step cost, and how much of it is the walk over the workgroups' mask windows.

    python tools/window_scan_floor.py [--libs parent=tools/ab/lib_parent.so,new=scone_gcn_amd/libscone_hip.so] [--rounds 4] [--reps 20]
                                      [--edges 1000000] [--slabs 32] [--masks zero,cone,bench]

|E| = 996 634, 32 slabs (one micro-batch of bench.py), hidden 32, tanh.  The launches and their masks (M0 = scn_keep_mask of the last
nodes, M_k = scn_mask_hop of M_{k-1}):
    bwd2_first_visit   layer-2 backward, fused-first from y, visiting M2   (+ its two reduce launches, ~5 us each)
    bwd3_visit         layer-3 backward, visiting M1                       (+ its reduce launch)
    fwd2_from_y_keep   layer-2 forward from y, kept on M1
    fwd3_keep          layer-3 forward, kept on M0
    y_keep             gather3_c1_keep_kernel on M2
    clear_mask         clear_mask_kernel on M1
with three sets of masks:
    zero   all-zero words: every block is left at the window test, so the time is launch + prologue + the walk and nothing else;
    cone   seeded random last nodes, the masks of tools/readout_cone_density.py;
    bench  the last nodes of 4 * slabs trajectories drawn as bench.py draws its batch (bench.dataset, seed 1030).
Timing: HIP events around `reps` back-to-back launches queued behind a ~3 ms sleep kernel, so the host's launch cost is off the clock;
"empty" is the same measurement of a one-element fill.  --libs: library builds to compare (tools/ab_build_rev.sh makes the one of
an earlier revision), a plan per build, the builds alternating round by round on the same tensors."""
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
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--masks", default="zero,cone,bench")
ap.add_argument("--libs", default="", help="name=path,... (paths relative to the repo root); default: the library of this tree alone")
a = ap.parse_args()

cx = g.random_SC_graph(g.calibrate_n_points(a.edges))
sc = SimplicialComplex(cx)
shifts, readout, _ = te.setup_from_complex(sc, "scone")
dev = ops.default_device()
_lib.AB_OLDER_LIBRARY = True
builds = {}                               # name -> (library, its plan, the plan's tables)
for spec in a.libs.split(",") if a.libs else ["this=" + _lib.LIB_PATH]:
    name, path = spec.split("=")
    _lib._lib = None
    _lib.LIB_PATH = path if os.path.isabs(path) else os.path.join(ROOT, path)
    lib = _lib.load()
    p = ops.SconePlan(shifts[0], shifts[1], readout, "tanh", dev)
    builds[name] = (lib, p, p.field_tables_dev())
    assert builds[name][2] is not None and p.conv_T is p.conv
    print("build %s: %s" % (name, _lib.LIB_PATH), flush=True)
first = next(iter(builds))
_lib._lib, plan, tabs = builds[first]
E, C, S = cx.n_edges, 32, a.slabs
print("|E| = %d, %d plan blocks, %d slabs, hidden %d, tanh; %d rounds x %d launches" % (E, tabs.n_blocks, S, C, a.rounds, a.reps), flush=True)


def cone(last_nodes):
    last = torch.as_tensor(np.asarray(last_nodes).astype(np.int32), device=dev)
    m = [plan.conv.keep_mask(last, ops.NS, plan.n_nodes, tabs)]
    for _ in range(2):
        m.append(plan.conv.mask_hop(m[-1], tabs))
    return m


MASKS = {}
for kind in a.masks.split(","):
    if kind == "zero":
        z = torch.zeros((tabs.n_blocks, (S + 31) // 32), device=dev, dtype=torch.int32)
        MASKS[kind] = [z, z, z]
    elif kind == "cone":
        MASKS[kind] = cone(np.random.RandomState(1).randint(0, plan.n_nodes, size=S * ops.NS))
    else:
        assert kind == "bench"
        import bench
        MASKS[kind] = cone(bench.dataset(cx, sc, S * ops.NS, 1030)[2])
    bits = [int(((m[:, torch.arange(S, device=dev) >> 5] >> (torch.arange(S, device=dev) & 31)) & 1).sum()) for m in MASKS[kind]]
    print("masks %-5s M0 %d, M1 %d, M2 %d items of %d" % (kind, bits[0], bits[1], bits[2], tabs.n_blocks * S), flush=True)

# one set of tensors for every build: a trajectory-like input (~5 % of the 64-row groups of a slab carry values), its records y, the
# layer-2 output h (aux of the layer-3 backward, input of the layer-3 forward, and a dense stand-in for the gradients), one output buffer
torch.manual_seed(0)
W = [torch.randn(C, C, device=dev) * 0.1 for _ in range(3)]
Wf = [torch.randn(1, C, device=dev) * 0.3 for _ in range(3)]
x = torch.randn(S, E, 4, 1, device=dev)
x *= (torch.rand(S, (E + 63) // 64, device=dev) < 0.05).repeat_interleave(64, dim=1)[:, :E][:, :, None, None]
y = plan.conv.shifted_input(x)
h = plan.conv.forward_from_y(y, Wf, W, "tanh")
assert y is not None and h is not None
buf = torch.zeros_like(h)
dW, dWf = [torch.zeros(C, C, device=dev) for _ in range(3)], [torch.zeros(1, C, device=dev) for _ in range(3)]
one = torch.zeros(1, device=dev)


def launches(p, m):
    return {
        "bwd2_first_visit": lambda: p.conv_T.backward_fused_first(h, W, None, "tanh", y, dW, dWf, Ws_first=Wf, visit=m[2]),
        "bwd3_visit": lambda: p.conv_T.backward([h], W, h, "tanh", True, dW, dx=buf, visit=m[1]),
        "fwd2_from_y_keep": lambda: p.conv.forward_from_y(y, Wf, W, "tanh", keep=m[1], out=buf),
        "fwd3_keep": lambda: p.conv.forward([h], W, C, "tanh", out=buf, keep=m[0]),
        "y_keep": lambda: p.conv.shifted_input(x, keep=m[2]),
        "clear_mask": lambda: p.conv.clear_mask(buf, m[1]),
        "empty": lambda: one.zero_(),
    }


e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
torch.cuda.synchronize()
e0.record()
torch.cuda._sleep(10_000_000)
e1.record()
torch.cuda.synchronize()
SLEEP = int(10_000_000 * 3.0 / max(e0.elapsed_time(e1), 1e-3))      # cycles of a ~3 ms sleep


def timed(fn, reps):
    """us per launch: `reps` launches queued behind a sleeping kernel, between two events"""
    fn()
    torch.cuda.synchronize()
    torch.cuda._sleep(SLEEP)
    e0.record()
    for _ in range(reps):
        r = fn()
        assert r is not False
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


times = {}
names = list(builds)
for r in range(a.rounds):
    for n in names[r % len(names):] + names[:r % len(names)]:          # rotate: no build always runs behind the same one
        lib, p, _ = builds[n]
        _lib._lib = lib                                                # (a plan's handles belong to the library that made them)
        for kind, m in MASKS.items():
            for key, fn in launches(p, m).items():
                times.setdefault((kind, key, n), []).append(timed(fn, a.reps))
for kind in MASKS:
    print("== masks: %s (us per launch: mean over rounds, spread, rounds)" % kind)
    for key in launches(plan, MASKS[kind]):
        for n in names:
            v = times[(kind, key, n)]
            print("   %-17s %-7s %8.1f  spread %5.1f   %s" % (key, n, sum(v) / len(v), max(v) - min(v), " ".join("%.1f" % t for t in v)), flush=True)
    for n in names:
        tot = sum(sum(times[(kind, key, n)]) / a.rounds for key in launches(plan, MASKS[kind]) if key != "empty")
        print("   %-17s %-7s %8.1f" % ("six launches", n, tot), flush=True)
