"""Timing of training on whole paths (Scone_GCN.path_grad_step; scone_gcn_amd/path_train.py, scn_path_stage in csrc/scn_paths.hip).

  (a) the 400-point generated data set, 1000 walks, 3-layer SCoNe of hidden 16: one optimiser step on --items (4096) items drawn
      from all prefixes, milliseconds per step and items per second, and beside it the only route there was before -- one
      SparseFlows row per (path, prefix) from paths_to_flows on the host plus one-hot targets, then Scone_GCN.grad_step on them --
      measured in the same run, and the ratio.  That route is the yardstick.  The two gradients are compared once (apply=False).
  (b) the |E| ~ 1M complex of bench.py's headline configuration (hidden 32) with --walks device-generated walks (Euclidean metric):
      steps of --items items in micro-batches of --micro-batch (128), cycling through four item sets so that every restage finds
      other items in its buffer; ms per step and items per second with ops.PATH_STAGE_SPARSE_CLEAR on and off in the SAME call,
      --reps (3) windows of --steps steps per arm, alternating, after a warm-up window per arm; the spread of each arm and the
      ratio of the medians.  The gradients of one step under both settings are compared bitwise.
Device-synchronised host clock around each window.  Prints one JSON line per case and appends them to --out.

The kernel-time share of the staging kernels (path_reset_kernel / path_zero_kernel, path_stage_kernel) beside the step's comes
from a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/path_train_time.py --case b --out /dev/null

    python tools/path_train_time.py [--case a|b|ab] [--items 4096] [--reps 3] [--steps 20] [--edges 1000000] [--walks 32]
                                    [--micro-batch 128] [--out profiles/path_train.txt]
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
from scone_gcn_amd import ops, synthetic_data_gen as g, trajectory_experiments as te   # noqa: E402
from scone_gcn_amd.complex import SimplicialComplex                        # noqa: E402
from scone_gcn_amd.scone_trajectory_model import Scone_GCN                # noqa: E402

T0 = time.perf_counter()


def _say(*a):
    print("[path_train_time %.0fs]" % (time.perf_counter() - T0), *a, file=sys.stderr, flush=True)


def _net(sc, hidden, batch, seed=0):
    shifts, readout, _ = te.setup_from_complex(sc, "scone")
    inputs = [readout, np.zeros(1, np.int64), g.paths_to_flows(sc.cx, [[]])]
    net = Scone_GCN(1, 1e-3, batch, 0.0, verbose=False)
    net.setup(te.scone_func, [(3, hidden)] * 3, shifts, inputs, np.zeros((1, sc.max_degree, 1)), None, np.ones(1))
    rs = np.random.RandomState(seed)
    net._install([0.3 * rs.randn(*s) for s in so.weight_shapes(1, [(3, hidden)] * 3, 1)])
    return net, inputs


def _window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def case_a(n_items, reps, steps):
    cx = g.random_SC_graph(400)
    sc = SimplicialComplex(cx)
    paths = g.generate_random_walks(cx, m=1000)
    net, inputs = _net(sc, 16, n_items)
    ps = net.path_set(inputs, paths)
    item_ptr, item_path, item_len = ps.items(2)
    M = len(item_path)
    sel = np.sort(np.random.RandomState(1).choice(M, size=min(n_items, M), replace=False))
    step = lambda i: net.path_grad_step(inputs, ps, sel)
    _window(step, 3)
    times = [_window(step, steps) for _ in range(reps)]
    # the host route: every prefix a SparseFlows row and a one-hot target row of its own, then grad_step on them
    nb = np.asarray(sc.nbrhoods)

    def host_inputs():
        prefixes = [paths[p][:k] for p, k in zip(item_path[sel], item_len[sel])]
        flows = g.paths_to_flows(cx, prefixes)
        last = np.asarray([p[-1] for p in prefixes])
        y = np.zeros((len(sel), nb.shape[1], 1), np.float32)
        for i, (p, k) in enumerate(zip(item_path[sel], item_len[sel])):
            y[i, list(nb[paths[p][k - 1]]).index(paths[p][k]), 0] = 1.0
        return [inputs[0], last, flows], y
    mask = np.ones(len(sel), int)
    host_in, y = host_inputs()
    net.grad_step(host_in, y, mask)                                      # (warm-up)
    build, grad = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_in, y = host_inputs()
        t1 = time.perf_counter()
        net.grad_step(host_in, y, mask)
        torch.cuda.synchronize()
        build.append(t1 - t0)
        grad.append(time.perf_counter() - t1)
    net.grad_step(host_in, y, mask, apply=False)
    g_host = net._flat_g.clone()
    net.path_grad_step(inputs, ps, sel, apply=False)
    diff = float((net._flat_g - g_host).abs().max())
    med, host = float(np.median(times)), float(np.median(build) + np.median(grad))
    return [{"case": "a", "n_edges": int(cx.n_edges), "paths": len(paths), "items_in_set": M, "items_per_step": len(sel), "hidden": 16,
             "micro_batches": len(net._path_pool.bufs), "step_ms": 1e3 * med, "step_ms_min_max": [1e3 * min(times), 1e3 * max(times)],
             "items_per_s": len(sel) / med, "host_route_ms": 1e3 * host, "host_route_build_ms": 1e3 * float(np.median(build)),
             "host_route_grad_step_ms": 1e3 * float(np.median(grad)), "ratio_host_route_over_step": host / med,
             "max_abs_gradient_difference_to_host_route": diff,
             "note": "median of %d windows of %d steps; the host route is the median of %d single steps, flows rebuilt every step"
                     % (reps, steps, reps)}]


def case_b(edges, n_walks, n_items, micro_batch, reps, steps):
    _say("building the |E| ~ %d complex" % edges)
    cx = g.random_SC_graph(g.calibrate_n_points(edges))
    sc = SimplicialComplex(cx)
    _say("walks: %d on the device" % n_walks)
    walks = g.generate_random_walks_batched(cx, m=n_walks, metric="euclid", backend="device")
    net, inputs = _net(sc, 32, n_items)
    net.path_micro_batch = micro_batch
    ps = net.path_set(inputs, walks)
    _, item_path, item_len = ps.items(2)
    M = len(item_path)
    rs = np.random.RandomState(2)
    sets = [rs.choice(M, size=min(n_items, M), replace=False) for _ in range(4)]
    step = lambda i: net.path_grad_step(inputs, ps, sets[i % len(sets)])
    arms = {"sparse": True, "dense": False}
    grads = {}
    for name, flag in arms.items():                                      # one step per arm from the same state: the same bits
        ops.PATH_STAGE_SPARSE_CLEAR = flag
        net.path_grad_step(inputs, ps, sets[0], apply=False)
        net.path_grad_step(inputs, ps, sets[1], apply=False)
        grads[name] = net._flat_g.clone()
    same = bool(torch.equal(grads["sparse"].view(torch.int32), grads["dense"].view(torch.int32)))
    times = {name: [] for name in arms}
    for name, flag in arms.items():
        _say("warm-up window, %s" % name)
        ops.PATH_STAGE_SPARSE_CLEAR = flag
        _window(step, max(4, steps // 4))
    for r in range(reps):
        for name, flag in arms.items():
            ops.PATH_STAGE_SPARSE_CLEAR = flag
            times[name].append(_window(step, steps))
            _say("window %d, %s: %.3f ms/step" % (r, name, 1e3 * times[name][-1]))
    ops.PATH_STAGE_SPARSE_CLEAR = True
    med = {name: float(np.median(t)) for name, t in times.items()}
    spread = {name: (max(t) - min(t)) / med[name] for name, t in times.items()}
    n = len(sets[0])
    prefix_nodes = float(np.mean([item_len[s].mean() for s in sets]))
    return [{"case": "b", "n_edges": int(cx.n_edges), "n_nodes": int(cx.n_nodes), "walks": len(walks),
             "walk_nodes": int(sum(map(len, walks))), "items_in_set": M, "items_per_step": n, "mean_prefix_nodes": prefix_nodes,
             "hidden": 32, "micro_batch": micro_batch, "micro_batches": len(net._path_pool.bufs), "steps_per_window": steps,
             "sparse_ms_per_step": [1e3 * t for t in times["sparse"]], "dense_ms_per_step": [1e3 * t for t in times["dense"]],
             "sparse_ms_median": 1e3 * med["sparse"], "dense_ms_median": 1e3 * med["dense"],
             "sparse_items_per_s": n / med["sparse"], "dense_items_per_s": n / med["dense"],
             "spread_sparse": spread["sparse"], "spread_dense": spread["dense"], "ratio_dense_over_sparse": med["dense"] / med["sparse"],
             "gradients_bitwise_equal": same,
             "note": "windows alternate sparse, dense; spread = (max - min) / median of an arm's windows"}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="ab")
    ap.add_argument("--items", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--edges", type=int, default=1_000_000)
    ap.add_argument("--walks", type=int, default=32)
    ap.add_argument("--micro-batch", type=int, default=128)
    ap.add_argument("--out", default=os.path.join("profiles", "path_train.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "path_train_time needs a GPU: a time taken elsewhere says nothing"
    rows = []
    if "a" in a.case:
        rows += case_a(a.items, a.reps, a.steps)
    if "b" in a.case:
        rows += case_b(a.edges, a.walks, a.items, a.micro_batch, a.reps, a.steps)
    with open(a.out, "a") as f:
        f.write("# python tools/path_train_time.py --case %s --items %d --reps %d --steps %d --edges %d --walks %d --micro-batch %d  (%s)\n"
                % (a.case, a.items, a.reps, a.steps, a.edges, a.walks, a.micro_batch, torch.cuda.get_device_name(0)))
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
