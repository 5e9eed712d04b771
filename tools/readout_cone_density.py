#!/usr/bin/env python3
"""Share of the (plan block, slab) items in the masks M0 .. M_{L-1} of the readout's cone (ops.READOUT_CONE): M0 = scn_keep_mask of
the last nodes, M_k = scn_mask_hop of M_{k-1}.  |E| = 996 634 and 32 slabs by default (one micro-batch of bench.py), seeded random last
nodes as in tools/top_dz_mask_ab.py.

    python tools/readout_cone_density.py [--edges 1000000] [--slabs 32] [--layers 3]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scone_gcn_amd import ops, synthetic_data_gen as g, trajectory_experiments as te   # noqa: E402
from scone_gcn_amd.complex import SimplicialComplex                                            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--edges", type=int, default=1_000_000)
ap.add_argument("--slabs", type=int, default=32)
ap.add_argument("--layers", type=int, default=3)
a = ap.parse_args()

cx = g.random_SC_graph(g.calibrate_n_points(a.edges))
sc = SimplicialComplex(cx)
shifts, readout, _ = te.setup_from_complex(sc, "scone")
dev = ops.default_device()
plan = ops.SconePlan(shifts[0], shifts[1], readout, "tanh", dev)
tabs = plan.field_tables_dev()
assert tabs is not None and plan.conv_T is plan.conv
S = a.slabs
last = torch.as_tensor(np.random.RandomState(1).randint(0, plan.n_nodes, size=S * ops.NS).astype(np.int32), device=dev)
print("|E| = %d, %d plan blocks, %d slabs" % (cx.n_edges, tabs.n_blocks, S), flush=True)
mask = plan.conv.keep_mask(last, ops.NS, plan.n_nodes, tabs)
for k in range(a.layers):
    bits = (mask[:, torch.arange(S, device=dev) >> 5] >> (torch.arange(S, device=dev) & 31)) & 1      # [n_blocks][S]
    print("M%d: %d items, %.3f %% of (block, slab)" % (k, int(bits.sum()), 100.0 * float(bits.float().mean())), flush=True)
    mask = plan.conv.mask_hop(mask, tabs)
