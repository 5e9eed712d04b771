#!/usr/bin/env python3
"""What visiting only the blocks a written row can reach (ops.VISIT_ROWS) takes off the two visiting backwards of the cone step, counted
before anything is timed.

    python tools/visit_rows_count.py [--edges 1000000] [--micro-batches 4] [--slabs 32] [--times 103.1,165.8] [--floors 11.1,14.7]

The benchmark's complex, the plan's real blocks, last nodes drawn as bench.py draws its batch (bench.dataset, seed 1030), three layers.
Per micro-batch, from the step's own mask launch (ConvOp.cone_masks with the plan's visit tables; V_k is checked against
ops.visit_masks_host on the first micro-batch):
    items     set bits of M1, M2 (what the backwards of layers 3 and 2 visit today) against V1, V2;
    busiest   units (blocks with a visit) and visits of the busiest workgroup of each launch under its static shares -- every
              workgroup's sequence as scn_window_scan_probe writes it for the launch's grid (256 x 1; launch_grid as
              tools/blocked_grid.py restates it, shared with tools/cone_balance.py), for M_k and for V_k;
    predicted floor + (busiest visits after / before) x (time - floor) per launch, with the traced times and the floors given.
The decision rule of the change: go on if either launch loses at least a third of its busiest workgroup's visits.
Also printed: the host seconds of the table build and the tables' sizes."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                                            # noqa: E402
from blocked_grid import launch_grid                                                   # noqa: E402
from scone_gcn_amd import ops, synthetic_data_gen as g, trajectory_experiments as te   # noqa: E402
from scone_gcn_amd.complex import SimplicialComplex                                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--edges", type=int, default=1_000_000)
ap.add_argument("--micro-batches", type=int, default=4)
ap.add_argument("--slabs", type=int, default=32)
ap.add_argument("--times", default="103.1,165.8", help="traced us of the layer-3 and the layer-2 backward (profiles/cone_masks_ab.txt)")
ap.add_argument("--floors", default="11.1,14.7", help="their floors, us (an all-zero mask)")
a = ap.parse_args()
L = 3
TIMES, FLOORS = ([float(v) for v in s.split(",")] for s in (a.times, a.floors))

cx = g.random_SC_graph(g.calibrate_n_points(a.edges))
sc = SimplicialComplex(cx)
shifts, readout, _ = te.setup_from_complex(sc, "scone")
dev = ops.default_device()
plan = ops.SconePlan(shifts[0], shifts[1], readout, "tanh", dev)
tabs = plan.field_tables_dev()
assert tabs is not None and plan.conv_T is plan.conv
t0 = time.perf_counter()
vt = plan.visit_tables_dev(L - 1)
torch.cuda.synchronize()
print("|E| = %d, %d plan blocks; visit tables built in %.1f s on the host: %s entries (top: %d)" %
      (cx.n_edges, tabs.n_blocks, time.perf_counter() - t0, " / ".join(str(b.numel() - 1) for b in vt.blk), tabs.top_blk.numel() - 1), flush=True)

S, nb = a.slabs, tabs.n_blocks
n = S * ops.NS
last = np.asarray(bench.dataset(cx, sc, n * a.micro_batches, 1030)[2])
last_devs = [torch.as_tensor(last[i * n:(i + 1) * n].astype(np.int32), device=dev) for i in range(a.micro_batches)]
cones = plan.conv.cone_masks(last_devs, ops.NS, plan.n_nodes, tabs, L, visit_tabs=vt)
assert cones is not None
torch.cuda.synchronize()
host = ops.visit_masks_host(last[:n], ops.NS, [(p.cpu().numpy()[:-1], b.cpu().numpy()[:-1]) for p, b in zip(vt.ptr, vt.blk)], nb)
for k in (1, 2):
    assert np.array_equal(cones[0].visits[k].cpu().numpy().view(np.uint32), host[k - 1]), "V_%d of the launch is not the host's" % k


G, gy = launch_grid(nb, S, 1)                      # (a backward launch: one workgroup per CU)
assert gy == 1, "the grid splits the slabs"
bits = lambda m: int(np.unpackbits(m.cpu().numpy().view(np.uint8)).sum())


def busiest(mask):
    seqs, _ = plan.conv.window_scan_probe(mask, S, G, 0, S)
    return max(len(s) for s in seqs), max(sum(bin(w).count("1") for _, w in s) for s in seqs)


rows = {1: [], 2: []}
for i, c in enumerate(cones):
    for k in (1, 2):
        m, v = c[k], c.visits[k]
        assert not bool((v & ~m).any()), "V_%d is not inside M_%d" % (k, k)
        rows[k].append((bits(m), bits(v)) + busiest(m) + busiest(v))
        print("micro-batch %d  M%d %5d items, V%d %5d (%.2f x fewer); busiest workgroup of %d: %3d units / %3d visits -> %3d / %3d" %
              ((i, k, rows[k][-1][0], k, rows[k][-1][1], rows[k][-1][0] / max(1, rows[k][-1][1]), G) + rows[k][-1][2:]), flush=True)
go = False
for k, name in ((1, "layer-3 backward"), (2, "layer-2 backward (fused-first from y)")):
    r = np.asarray(rows[k], np.float64).mean(axis=0)
    t, f = TIMES[k - 1], FLOORS[k - 1]
    lost = 1 - r[5] / r[3]
    go |= lost >= 1 / 3
    print("%-38s mean items %7.1f -> %7.1f; busiest visits %5.1f -> %5.1f (-%.0f %%); predicted %.1f + %.3f x (%.1f - %.1f) = %.1f us" %
          (name, r[0], r[1], r[3], r[5], 100 * lost, f, r[5] / r[3], t, f, f + r[5] / r[3] * (t - f)), flush=True)
print("decision: %s" % ("go on (a launch loses at least a third of its busiest workgroup's visits)" if go else "stop"))
