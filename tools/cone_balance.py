#!/usr/bin/env python3
"""How evenly the visits of a readout cone's three forward-side launches fall on the workgroups, and what taking the units from one
device-wide list (ops.CONE_UNIT_LIST, WindowWalk's list mode) does about it.

    python tools/cone_balance.py [--edges 1000000] [--slabs 32] [--rounds 4] [--reps 20] [--no-timing]

|E| = 996 634, 32 slabs (one micro-batch of bench.py).  Masks M0 = scn_keep_mask of the last nodes, M_k = scn_mask_hop of M_{k-1}, for
    cone   the seeded random last nodes of tools/readout_cone_density.py,
    bench  last nodes drawn as bench.py draws its batch (bench.dataset, seed 1030).
The launches and their grids (launch_grid of scn_blk_dispatch.inc, restated in tools/blocked_grid.py):
    fwd3_keep          layer-3 forward kept on M0                  256 x 1 workgroups
    fwd2_from_y_keep   layer-2 forward from y kept on M1           256 x 1
    y_keep             gather3_c1_keep_kernel on M2                512 x 1
1. Balance.  STATIC: every workgroup's sequence as scn_window_scan_probe writes it for the launch's grid -- units (non-empty blocks)
   and visits (set bits) per workgroup: mean, median, busiest.  LIST: workgroup g takes entries g, g + G, ... of the mask's unit list
   in the order the device wrote it (scn_keep_mask_units / scn_mask_hop_units): the same figures, and the bound ceil(units / G).
2. Timing (skipped with --no-timing): each launch with the static walk and with the list, on all-zero masks (the floor: launch +
   prologue + the walk) and on the two sets above; HIP events around `reps` back-to-back launches queued behind a ~3 ms sleep kernel,
   the two forms alternating round by round on one set of tensors (the method of tools/window_scan_floor.py, whose tensors these are).
   Beside it the time the balance predicts for the list form: floor + (busiest after) / (busiest before) x (static time - floor)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blocked_grid import launch_grid                                                   # noqa: E402
from scone_gcn_amd import ops, synthetic_data_gen as g, trajectory_experiments as te   # noqa: E402
from scone_gcn_amd.complex import SimplicialComplex                                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--edges", type=int, default=1_000_000)
ap.add_argument("--slabs", type=int, default=32)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--no-timing", action="store_true")
a = ap.parse_args()

cx = g.random_SC_graph(g.calibrate_n_points(a.edges))
sc = SimplicialComplex(cx)
shifts, readout, _ = te.setup_from_complex(sc, "scone")
dev = ops.default_device()
plan = ops.SconePlan(shifts[0], shifts[1], readout, "tanh", dev)
tabs = plan.field_tables_dev()
assert tabs is not None and plan.conv_T is plan.conv
E, C, S, nb = cx.n_edges, 32, a.slabs, tabs.n_blocks
assert S <= 64, "the list mode serves one slab range of at most 64 slabs"


LAUNCHES = [("fwd3_keep", 0, 1), ("fwd2_from_y_keep", 1, 1), ("y_keep", 2, 2)]      # name, mask index, workgroups per CU
GRIDS = {name: launch_grid(nb, S, per_cu) for name, _, per_cu in LAUNCHES}
print("|E| = %d, %d plan blocks, %d slabs; grids %s" % (E, nb, S, GRIDS), flush=True)
assert all(gy == 1 for _, gy in GRIDS.values()), "a grid splits the slabs: the launches would walk their static units"


def cone(last_nodes):
    """([M0, M1, M2], their unit lists)"""
    last = torch.as_tensor(np.asarray(last_nodes).astype(np.int32), device=dev)
    m, u, counters = plan.conv.keep_mask_units(last, ops.NS, plan.n_nodes, tabs)
    masks, units = [m], [u]
    for k in (1, 2):
        m, u = plan.conv.mask_hop_units(masks[-1], tabs, counters[k:k + 1])
        masks.append(m)
        units.append(u)
    return masks, units


def three(v):
    v = np.asarray(v, np.float64)
    return "mean %6.2f  median %4.0f  busiest %4d" % (v.mean(), np.median(v), int(v.max()))


popcount = np.vectorize(lambda w: bin(int(w)).count("1"))
SETS = {"cone": np.random.RandomState(1).randint(0, plan.n_nodes, size=S * ops.NS)}
import bench                                                                            # noqa: E402
SETS["bench"] = bench.dataset(cx, sc, S * ops.NS, 1030)[2]
MASKS, RATIO = {}, {}
for kind, last in SETS.items():
    masks, units = cone(last)
    MASKS[kind] = (masks, units)
    print("== balance, masks %s" % kind)
    for name, k, _ in LAUNCHES:
        G = GRIDS[name][0]
        seqs, _ = plan.conv.window_scan_probe(masks[k], S, G, 0, S)
        st_units = [len(s) for s in seqs]
        st_visits = [sum(bin(w).count("1") for _, w in s) for s in seqs]
        words = masks[k].cpu().numpy().view(np.uint32).reshape(-1)
        n = int(units[k].count.cpu()[0])
        ent = units[k].units.cpu().numpy()[:n].astype(np.int64)
        assert n == int((words != 0).sum()) and sorted(ent.tolist()) == np.flatnonzero(words).tolist(), "the list names every non-empty word once"
        assert n == sum(st_units) and int(popcount(words[ent]).sum()) == sum(st_visits)
        li_units = [len(ent[w::G]) for w in range(G)]
        li_visits = [int(popcount(words[ent[w::G]]).sum()) if len(ent[w::G]) else 0 for w in range(G)]
        RATIO[(kind, name)] = (max(st_visits), max(li_visits))
        print("   %-17s M%d  %5d units, %5d visits on %d workgroups; round-robin bound ceil(units / G) = %d units" %
              (name, k, n, sum(st_visits), G, -(-n // G)))
        print("      static  units  %s | visits %s" % (three(st_units), three(st_visits)))
        print("      list    units  %s | visits %s" % (three(li_units), three(li_visits)))
        print("      busiest visits: static %d = %.2f x mean, list %d = %.2f x mean; static / list %.2f" %
              (max(st_visits), max(st_visits) / np.mean(st_visits), max(li_visits), max(li_visits) / np.mean(li_visits),
               max(st_visits) / max(1, max(li_visits))), flush=True)
if a.no_timing:
    sys.exit(0)

z = torch.zeros((nb, (S + 31) // 32), device=dev, dtype=torch.int32)
zc = torch.zeros(1, device=dev, dtype=torch.int32)
zu = ops.UnitList(torch.zeros(z.numel(), device=dev, dtype=torch.int32), zc)
MASKS = dict([("zero", ([z, z, z], [zu, zu, zu]))] + list(MASKS.items()))
# the tensors of tools/window_scan_floor.py
torch.manual_seed(0)
W = [torch.randn(C, C, device=dev) * 0.1 for _ in range(3)]
Wf = [torch.randn(1, C, device=dev) * 0.3 for _ in range(3)]
x = torch.randn(S, E, 4, 1, device=dev)
x *= (torch.rand(S, (E + 63) // 64, device=dev) < 0.05).repeat_interleave(64, dim=1)[:, :E][:, :, None, None]
y = plan.conv.shifted_input(x)
h = plan.conv.forward_from_y(y, Wf, W, "tanh")
assert y is not None and h is not None
buf = torch.zeros_like(h)


def launches(m, u):
    return {
        "fwd3_keep": lambda: plan.conv.forward([h], W, C, "tanh", out=buf, keep=m[0], units=u[0]),
        "fwd2_from_y_keep": lambda: plan.conv.forward_from_y(y, Wf, W, "tanh", keep=m[1], out=buf, units=u[1]),
        "y_keep": lambda: plan.conv.shifted_input(x, keep=m[2], units=u[2]),
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
    assert fn() is not None
    torch.cuda.synchronize()
    torch.cuda._sleep(SLEEP)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


times = {}
forms = ["static", "list"]
for r in range(a.rounds):
    for form in forms[r % 2:] + forms[:r % 2]:
        for kind, (m, u) in MASKS.items():
            for key, fn in launches(m, u if form == "list" else [None] * 3).items():
                times.setdefault((kind, key, form), []).append(timed(fn, a.reps))
mean = lambda v: sum(v) / len(v)
for kind in MASKS:
    print("== masks: %s (us per launch: mean over %d rounds of %d launches, spread, rounds)" % (kind, a.rounds, a.reps))
    for key, _, _ in LAUNCHES:
        for form in forms:
            v = times[(kind, key, form)]
            print("   %-17s %-7s %8.1f  spread %5.1f   %s" % (key, form, mean(v), max(v) - min(v), " ".join("%.1f" % t for t in v)))
        if kind != "zero":
            floor, t = mean(times[("zero", key, "static")]), mean(times[(kind, key, "static")])
            before, after = RATIO[(kind, key)]
            print("   %-17s predicted for the list: %.1f + %d / %d x (%.1f - %.1f) = %.1f us; measured %.1f us" %
                  (key, floor, after, before, t, floor, floor + after / before * (t - floor), mean(times[(kind, key, "list")])), flush=True)
    for form in forms:
        print("   %-17s %-7s %8.1f" % ("three launches", form, sum(mean(times[(kind, key, form)]) for key, _, _ in LAUNCHES)), flush=True)
