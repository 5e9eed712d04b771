"""Timing of teacher-forced path scoring (Scone_GCN.path_step_log_probs; scone_gcn_amd/path_scores.py, csrc/scn_paths.hip).

  (a) the 400-point generated data set, 1000 walks, 3-layer SCoNe of hidden 16: seconds per call, items per second, and beside it
      the host route the call replaces -- one SparseFlows row per (path, prefix) from paths_to_flows, then Scone_GCN._predict on
      them -- measured once in the same run, and the ratio;
  (b) the |E| ~ 1M complex of bench.py's headline configuration (hidden 32) with --walks device-generated walks (Euclidean metric):
      seconds per call, items per second, and whether the forwards of a chunk take the cone route (SconePlan._route of the chunk's
      shape).  Nothing to compare with at this size.  --micro-batch sets Scone_GCN.multi_hop_micro_batch (0: the default rule; a
      comma list times one call per value); --max-items times a call on the walks' first items only (whole walks, as many as
      fit), since every item is one forward column.
Device-synchronised wall time (a call ends in its copy back); (a) is the median of --reps calls after a warm-up call, (b) one call
per chunk size after a warm-up call on four walks at that size.  Prints one JSON line per case and appends them to --out.

The kernel-time share of the three new kernels beside the forward's comes from a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/path_score_time.py --case b --out /dev/null

    python tools/path_score_time.py [--case a|b|ab] [--reps 5] [--edges 1000000] [--walks 256] [--micro-batch 0] [--max-items 0]
                                    [--out profiles/path_scores.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import scone_oracle as so                                     # noqa: E402
from scone_gcn_amd import ops, path_scores, synthetic_data_gen as g, trajectory_experiments as te   # noqa: E402
from scone_gcn_amd.complex import SimplicialComplex                        # noqa: E402
from scone_gcn_amd.scone_trajectory_model import Scone_GCN                # noqa: E402

T0 = time.perf_counter()


def _say(*a):
    print("[path_score_time %.0fs]" % (time.perf_counter() - T0), *a, file=sys.stderr, flush=True)


def _net(sc, hidden, seed=0):
    shifts, readout, _ = te.setup_from_complex(sc, "scone")
    inputs = [readout, np.zeros(1, np.int64), g.paths_to_flows(sc.cx, [[]])]
    net = Scone_GCN(1, 1e-3, 100, 0.0, verbose=False)
    net.setup(te.scone_func, [(3, hidden)] * 3, shifts, inputs, np.zeros((1, sc.max_degree, 1)), None, np.ones(1))
    rs = np.random.RandomState(seed)
    net._install([0.3 * rs.randn(*s) for s in so.weight_shapes(1, [(3, hidden)] * 3, 1)])
    return net, inputs


def _call(net, inputs, paths):
    t0 = time.perf_counter()
    sc = net.path_step_log_probs(inputs, paths)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, sc


def case_a(reps):
    cx = g.random_SC_graph(400)
    sc = SimplicialComplex(cx)
    paths = g.generate_random_walks(cx, m=1000)
    net, inputs = _net(sc, 16)
    _call(net, inputs, paths)
    times = []
    for _ in range(reps):
        dt, scores = _call(net, inputs, paths)
        times.append(dt)
    M = len(scores.logp)
    # the host route: every prefix a row of its own, then the model's forward over the rows
    t0 = time.perf_counter()
    ptr, nodes = path_scores.ragged(paths)
    _, item_path, item_len = path_scores.path_items(ptr, 2)
    prefixes = [paths[p][:k] for p, k in zip(item_path, item_len)]
    flows = g.paths_to_flows(cx, prefixes)
    last = np.asarray([p[-1] for p in prefixes])
    build_s = time.perf_counter() - t0
    host_in = [inputs[0], last, flows]
    net._predict(net.weights, host_in)                                   # (warm-up; the evaluation cache is keyed on the weights' version)
    net.invalidate_eval_cache()
    t1 = time.perf_counter()
    pred = net._predict(net.weights, host_in).cpu().numpy()
    predict_s = time.perf_counter() - t1
    nxt = nodes[ptr[item_path] + item_len]
    slot = np.asarray([list(sc.nbrhoods[v]).index(u) for v, u in zip(last, nxt)])
    diff = float(np.abs(pred[np.arange(M), slot, 0] - scores.logp).max())
    med = float(np.median(times))
    return [{"case": "a", "n_edges": int(cx.n_edges), "paths": len(paths), "path_nodes": int(ptr[-1]), "items": M, "hidden": 16,
             "call_s": med, "call_s_min_max": [float(min(times)), float(max(times))], "items_per_s": M / med,
             "host_route_s": build_s + predict_s, "host_route_build_flows_s": build_s, "host_route_predict_s": predict_s,
             "ratio_host_route_over_call": (build_s + predict_s) / med, "max_abs_difference_to_host_route": diff,
             "note": "the call includes the upload of the paths and the copy back; the host route's forward is the same kernels"}]


def case_b(edges, n_walks, micro_batches, max_items):
    _say("building the |E| ~ %d complex" % edges)
    cx = g.random_SC_graph(g.calibrate_n_points(edges))
    sc = SimplicialComplex(cx)
    _say("walks: %d on the device" % n_walks)
    t0 = time.perf_counter()
    walks = g.generate_random_walks_batched(cx, m=n_walks, metric="euclid", backend="device")
    gen_s = time.perf_counter() - t0
    if max_items:
        keep, total = 0, 0
        while keep < len(walks) and total + max(len(walks[keep]) - 2, 0) <= max_items:
            total += max(len(walks[keep]) - 2, 0)
            keep += 1
        walks = walks[:max(keep, 1)]
    net, inputs = _net(sc, 32)
    plan = net._plan(inputs)
    rows = []
    for micro_batch in micro_batches:
        net.multi_hop_micro_batch = micro_batch or None
        _say("warm-up on four walks")                                    # (per chunk size: a new launch shape builds its masks and buffers once)
        _call(net, inputs, walks[:4])
        _say("the timed call: %d walks, micro-batch %d" % (len(walks), micro_batch))
        dt, scores = _call(net, inputs, walks)
        M = len(scores.logp)
        mb = micro_batch or ops.forward_micro_batch(plan, net.weights, M)
        mb = min(max(ops.NS, ops.pad_count(int(mb))), ops.pad_count(M))
        route = plan._route(torch.empty((mb // ops.NS, plan.n_edges, ops.NS, 1), device="meta"), net.weights, None,
                            torch.empty((mb,), device="meta", dtype=torch.int32))
        rows.append({"case": "b", "n_edges": int(cx.n_edges), "n_nodes": int(cx.n_nodes), "walks_asked": n_walks, "walks": len(walks),
                     "walk_nodes": int(sum(map(len, walks))), "longest_walk": int(max(map(len, walks))), "generator_s": gen_s,
                     "items": M, "hidden": 32, "micro_batch_set": micro_batch, "items_per_forward": int(mb), "forwards": -(-M // int(mb)),
                     "call_s": dt, "items_per_s": M / dt, "cone_route": bool(route.cone), "keep_last": bool(route.keep_last),
                     "first": route.first, "mean_step_logp": float(scores.logp.mean()), "accuracy": float(np.mean(scores.rank == 0)),
                     "note": "one call after a warm-up call on four walks; includes the upload of the paths and the copy back"})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="ab")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--edges", type=int, default=1_000_000)
    ap.add_argument("--walks", type=int, default=256)
    ap.add_argument("--micro-batch", default="0", help="comma list: one timed call of case b per value (0: the default rule)")
    ap.add_argument("--max-items", type=int, default=0)
    ap.add_argument("--out", default=os.path.join("profiles", "path_scores.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "path_score_time needs a GPU: a time taken elsewhere says nothing"
    rows = []
    if "a" in a.case:
        rows += case_a(a.reps)
    if "b" in a.case:
        rows += case_b(a.edges, a.walks, [int(v) for v in a.micro_batch.split(",")], a.max_items)
    with open(a.out, "a") as f:
        f.write("# python tools/path_score_time.py --case %s --reps %d --edges %d --walks %d --micro-batch %s --max-items %d  (%s)\n"
                % (a.case, a.reps, a.edges, a.walks, a.micro_batch, a.max_items, torch.cuda.get_device_name(0)))
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
