#!/usr/bin/env python3
"""The cone masks of a step, timed with device events at the benchmark's geometry: bench.py's complex (|E| ~ 1M), its 4096
trajectories and their last nodes as bench.py draws and stages them (32 micro-batches of 128), three masks per micro-batch.

    python tools/cone_masks_time.py [--reps 200] [--edges 1000000] [--batch 4096]

  chain     today's launches for ONE micro-batch: scn_keep_mask_units (its memset included) + two scn_mask_hop_units
  one       scn_cone_masks for one micro-batch         (where the library has it)
  step      scn_cone_masks for all micro-batches of the step in one launch

The library's entries are called on buffers allocated once.  Each figure: sixteen calls (or chains) back to back between one pair of
events, queued while fills keep the device busy (so the device's time is measured, not the host's), divided by sixteen; `reps` / 16
such groups behind a warm-up over every micro-batch, cycling through the step's micro-batches; median, minimum and the 10th / 90th
percentile in microseconds.  Prints one JSON line at the end."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--edges", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--layers", type=int, default=3)
    args = ap.parse_args()
    import torch
    import bench
    from scone_gcn_amd import _lib, ops, synthetic_data_gen as g
    from scone_gcn_amd.complex import SimplicialComplex
    assert torch.cuda.is_available(), "needs a GPU"
    cx = g.random_SC_graph(g.calibrate_n_points(args.edges))
    sc = SimplicialComplex(cx)
    flows, choice, last, y = bench.dataset(cx, sc, args.batch, 1030)
    net, inputs = bench.make_net("scone", 32, sc, flows, last, y, args.batch)
    staged = net.stage(inputs, y, np.arange(args.batch))
    plan = net._plan(inputs)
    tabs = plan.field_tables_dev()
    lasts = [m[1] for m in staged]
    L = args.layers
    print("|E| = %d, %d plan blocks, %d micro-batches of %d last nodes, %d masks each" %
          (cx.n_edges, tabs.n_blocks, len(lasts), lasts[0].numel(), L), flush=True)

    # the library's entries on buffers allocated once: what is timed is the device's work, not the wrappers' allocations and views
    lib, i32 = _lib.load(), torch.int32
    st = ops._stream()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    n_words = tabs.n_blocks * ((-(-lasts[0].numel() // ops.NS) + 31) // 32)
    assert all(t.numel() == lasts[0].numel() for t in lasts)
    stride = -(-n_words // 128) * 128
    old_masks = [torch.empty(n_words + ops.UNIT_COUNTERS, device="cuda", dtype=i32)] + \
                [torch.empty(n_words, device="cuda", dtype=i32) for _ in range(L - 1)]
    old_units = [torch.empty(n_words, device="cuda", dtype=i32) for _ in range(L)]
    masks = torch.empty(len(lasts) * L * stride, device="cuda", dtype=i32)
    units = torch.empty_like(masks)
    counters = torch.empty(len(lasts) * ops.UNIT_COUNTERS, device="cuda", dtype=i32)
    new = hasattr(lib, "scn_cone_masks")
    if new:
        desc = (_lib.ConeMb * len(lasts))()
        for i, t in enumerate(lasts):
            d = desc[i]
            d.node, d.n, d.stride = t.data_ptr(), t.numel(), stride
            d.masks, d.units = masks.data_ptr() + 4 * i * L * stride, units.data_ptr() + 4 * i * L * stride
            d.counters = counters.data_ptr() + 4 * ops.UNIT_COUNTERS * i
    tp, tb, ap, ab = (ptr(t) for t in (tabs.top_ptr, tabs.top_blk, tabs.adj_ptr, tabs.adj_blk))

    def chain(i):
        t = lasts[i % len(lasts)]
        _lib.check(lib.scn_keep_mask_units(t.numel(), ops.NS, ptr(t), plan.n_nodes, tp, tb, tabs.n_blocks, ptr(old_masks[0]),
                                           ptr(old_units[0]), n_words, st), "scn_keep_mask_units")
        for k in range(1, L):
            _lib.check(lib.scn_mask_hop_units(tabs.n_blocks, n_words // tabs.n_blocks, ap, ab, ptr(old_masks[k - 1]), ptr(old_masks[k]),
                                              ptr(old_units[k]), ctypes.c_void_p(old_masks[0].data_ptr() + 4 * (n_words + k)), n_words, st),
                       "scn_mask_hop_units")

    def one(i):
        one_desc = (_lib.ConeMb * 1)(desc[i % len(lasts)])
        _lib.check(lib.scn_cone_masks(1, one_desc, ops.NS, plan.n_nodes, tabs.n_blocks, tp, tb, ap, ab, L, st), "scn_cone_masks")

    def step(i):
        _lib.check(lib.scn_cone_masks(len(lasts), desc, ops.NS, plan.n_nodes, tabs.n_blocks, tp, tb, ap, ab, L, st), "scn_cone_masks")

    plug = torch.empty(1 << 28, device="cuda", dtype=torch.float32)          # 1 GiB: a fill of it keeps the device busy for a while

    def timed(fn):
        """`group` calls back to back between one pair of events, behind fills that keep the device busy until the host has queued them
        all: the device's time per call with its launch gaps, not the host's."""
        group = 16
        for i in range(len(lasts)):
            fn(i)
        torch.cuda.synchronize()
        us = []
        for r in range(max(1, args.reps // group)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(4):
                plug.fill_(0.0)
            a.record()
            for i in range(group):
                fn(r * group + i)
            b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / group)
        us = np.sort(us)
        return {"median_us": float(np.median(us)), "min_us": float(us[0]), "p10_us": float(us[len(us) // 10]),
                "p90_us": float(us[(9 * len(us)) // 10])}

    res = {"n_edges": int(cx.n_edges), "n_blocks": int(tabs.n_blocks), "micro_batches": len(lasts), "masks": L, "reps": args.reps}
    res["chain (one micro-batch, today's %d launches and memset)" % L] = timed(chain)
    if new:
        res["scn_cone_masks, one micro-batch"] = timed(one)
        res["scn_cone_masks, the step's %d micro-batches" % len(lasts)] = timed(step)
    for k, v in res.items():
        if isinstance(v, dict):
            print("%-64s median %8.1f  min %8.1f  p10 %8.1f  p90 %8.1f us" % (k, v["median_us"], v["min_us"], v["p10_us"], v["p90_us"]),
                  flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
