"""Timing of the baselines' whole-path scores (Markov_Model.path_step_log_probs, Projection_Model.path_step_log_probs;
csrc/scn_markov.hip: markov_path_scores_kernel, csrc/scn_project.hip: project_path_scores_kernel).

  (a) the 400-point generated data set, 1000 walks: the Markov table at orders 1 and 2 (trained on the same walks, alpha = 1) and the
      projection on the embedded basis.  Per arm: seconds per call and items per second (a call includes the upload of the paths
      and the copy back), the kernel's share of that time (the same launch on resident buffers between two device events), and
      beside it the host route the call replaces -- one next_node_probs / predict_all call on host-built prefixes (paths_to_flows
      for the projection) -- timed ONCE, after a warm-up call on one walk and outside the alternating windows, on the first
      --host-walks walks and EXTRAPOLATED to all items by the item count: a single sample, to be read as an order of magnitude;
  (b) the |E| ~ 1M complex of bench.py's headline configuration with --walks device-generated walks (Euclidean metric), the basis
      from embed(): the same figures without a host route (nothing to compare with at this size).
The arms alternate: every round times one window of each arm (a window repeats the call until it lasts --window seconds), three
rounds after a warm-up call per arm; the median and the spread (min, max) of the three are reported.  Device-synchronised wall time.
Prints one JSON line per arm and appends them to --out.

    python tools/baseline_path_time.py [--case a|b|ab] [--rounds 3] [--window 0.3] [--edges 1000000] [--walks 512] [--host-walks 50]
                                       [--out profiles/baseline_path_scores.txt]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scone_gcn_amd import _lib, ops, path_scores, synthetic_data_gen as g  # noqa: E402
from scone_gcn_amd.complex import SimplicialComplex                        # noqa: E402
from scone_gcn_amd.markov_model import Markov_Model, ragged                # noqa: E402
from scone_gcn_amd.projection_model import Projection_Model                # noqa: E402

T0 = time.perf_counter()
ALPHA = 1.0


def _say(*a):
    print("[baseline_path_time %.0fs]" % (time.perf_counter() - T0), *a, file=sys.stderr, flush=True)


def _window(fn, window):
    """Seconds per call over one window of at least `window` seconds."""
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= window:
            return dt / n


def _alternate(arms, rounds, window):
    """{name: [seconds per call of each round]}: one warm-up call per arm, then `rounds` rounds of one window per arm, in turn."""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            times[name].append(_window(fn, window))
    return times


def _events(launch, reps=20):
    """Median milliseconds of one launch between two device events (after a warm-up launch)."""
    launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def _markov_launch(mm, ptr, nodes):
    """The launch of Markov_Model._path_records alone, on buffers that stay on the device."""
    lib, dev, T = _lib.load(), mm.device, len(nodes)
    d_ptr, d_nodes = torch.from_numpy(ptr).to(dev), torch.from_numpy(nodes).to(dev)
    prob = torch.empty((T,), dtype=torch.float64, device=dev)
    rank, total = (torch.empty((T,), dtype=torch.int32, device=dev) for _ in range(2))
    err = torch.full((1,), ops.INT32_MAX, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def launch():
        _lib.check(lib.scn_markov_path_scores(len(ptr) - 1, p(d_ptr), p(d_nodes), mm.order, ctypes.c_double(ALPHA), *mm._graph_args(),
                                              p(mm.counts), p(prob), p(rank), p(total), p(err), ops._stream()), "scn_markov_path_scores")
    return launch


def _project_launch(pm, ptr, nodes):
    lib, dev, T = _lib.load(), pm.device, len(nodes)
    d_ptr, d_nodes = torch.from_numpy(ptr).to(dev), torch.from_numpy(nodes).to(dev)
    logp, mass = (torch.empty((T,), dtype=torch.float64, device=dev) for _ in range(2))
    rank = torch.empty((T,), dtype=torch.int32, device=dev)
    err = torch.full((1,), ops.INT32_MAX, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
    t = pm._tab

    def launch():
        _lib.check(lib.scn_project_path_scores(len(ptr) - 1, p(d_ptr), p(d_nodes), pm.dim, pm.n_edges, p(pm._V), pm.n_nodes, p(t[0]),
                                               p(t[1]), p(t[2]), p(t[3]), pm.width, p(t[4]), p(t[5]), p(logp), p(rank), p(mass), None,
                                               p(err), ops._stream()), "scn_project_path_scores")
    return launch


def _rows(case, cx, paths, models, rounds, window, extra):
    ptr, nodes = ragged(paths)
    arms = {name: (lambda m=m: m.path_step_log_probs((ptr, nodes))) if name == "projection"
            else (lambda m=m: m.path_step_log_probs((ptr, nodes), alpha=ALPHA)) for name, m in models.items()}
    times = _alternate(arms, rounds, window)
    rows = []
    for name, m in models.items():
        sc = arms[name]()
        M, med = len(sc.logp), float(np.median(times[name]))
        kernel_ms = _events(_project_launch(m, ptr, nodes) if name == "projection" else _markov_launch(m, ptr, nodes))
        row = {"case": case, "arm": name, "n_nodes": int(cx.n_nodes), "n_edges": int(cx.n_edges), "paths": len(ptr) - 1,
               "path_nodes": int(len(nodes)), "longest_path": int(np.diff(ptr).max()), "items": M, "call_s": med,
               "call_s_min_max": [float(min(times[name])), float(max(times[name]))], "rounds": rounds, "items_per_s": M / med,
               "kernel_ms": kernel_ms, "kernel_share_of_call": kernel_ms * 1e-3 / med, "mean_step_logp": float(sc.logp.mean()),
               "perplexity": float(np.exp(-sc.logp.mean())), "accuracy": float(np.mean(sc.rank == 0))}
        if name == "projection":
            row.update(dim=m.dim)
        else:
            row.update(order=m.order, alpha=ALPHA, table_bytes=int(m.counts.numel() * 4), n_unseen=int((m.path_totals == 0).sum()))
        row.update(extra.get(name, {}))
        rows.append(row)
    return rows


def _host_route(cx, paths, models, host_walks, items_all):
    """The per-prefix calls on host-built prefixes of the first walks: seconds, and their extrapolation to all items."""
    sub = paths[:host_walks]
    ptr, nodes = path_scores.ragged(sub)
    _, item_path, item_len = path_scores.path_items(ptr, 2)
    out = {}
    for name, m in models.items():
        if name == "projection":                                     # warm-up: the calls' first launches and allocations are not the route's
            m.predict_all(g.paths_to_flows(cx, sub[:1]), np.asarray([sub[0][-1]]))
        else:
            m.next_node_probs(sub[:1])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prefixes = [sub[p][:k] for p, k in zip(item_path, item_len)]
        if name == "projection":
            m.predict_all(g.paths_to_flows(cx, prefixes), np.asarray([p[-1] for p in prefixes]))
        else:
            m.next_node_probs(prefixes)
        dt = time.perf_counter() - t0
        out[name] = {"host_route_walks": len(sub), "host_route_items": len(item_len), "host_route_s_measured": dt,
                     "host_route_s_extrapolated_to_all_items": dt * items_all / max(len(item_len), 1),
                     "host_route_note": "measured on the first walks only and scaled by the item count: an extrapolation"}
    return out


def case_a(rounds, window, host_walks):
    cx = g.random_SC_graph(400)
    sc = SimplicialComplex(cx)
    paths = g.generate_random_walks(cx, m=1000)
    nbr, _ = g.neighborhood_table(cx)
    models = {}
    for order in (1, 2):
        models["markov_order%d" % order] = Markov_Model(order)
        models["markov_order%d" % order].train(nbr, paths)
    models["projection"] = Projection_Model().embed(sc)
    items = int(np.maximum(np.asarray([len(p) for p in paths]) - 2, 0).sum())
    extra = _host_route(cx, paths, models, host_walks, items)
    rows = _rows("a", cx, paths, models, rounds, window, extra)
    for r in rows:
        r["ratio_host_route_extrapolated_over_call"] = r["host_route_s_extrapolated_to_all_items"] / r["call_s"]
    return rows


def case_b(rounds, window, edges, n_walks):
    _say("building the |E| ~ %d complex" % edges)
    cx = g.random_SC_graph(g.calibrate_n_points(edges))
    sc = SimplicialComplex(cx)
    _say("walks: %d on the device" % n_walks)
    t0 = time.perf_counter()
    paths = g.generate_random_walks_batched(cx, m=n_walks, metric="euclid", backend="device")
    gen_s = time.perf_counter() - t0
    nbr, _ = g.neighborhood_table(cx)
    models = {}
    for order in (1, 2):
        _say("Markov table of order %d" % order)
        models["markov_order%d" % order] = Markov_Model(order)
        models["markov_order%d" % order].train(nbr, paths)
    _say("embedding")
    t0 = time.perf_counter()
    models["projection"] = Projection_Model().embed(sc)
    embed_s = time.perf_counter() - t0
    _say("timing")
    rows = _rows("b", cx, paths, models, rounds, window, {"projection": {"embed_s": embed_s}})
    for r in rows:
        r.update(generator_s=gen_s, D=int(nbr.shape[1]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="ab")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--edges", type=int, default=1_000_000)
    ap.add_argument("--walks", type=int, default=512)
    ap.add_argument("--host-walks", type=int, default=50)
    ap.add_argument("--out", default=os.path.join("profiles", "baseline_path_scores.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "baseline_path_time needs a GPU: a time taken elsewhere says nothing"
    rows = []
    if "a" in a.case:
        rows += case_a(a.rounds, a.window, a.host_walks)
    if "b" in a.case:
        rows += case_b(a.rounds, a.window, a.edges, a.walks)
    with open(a.out, "a") as f:
        f.write("# python tools/baseline_path_time.py --case %s --rounds %d --window %g --edges %d --walks %d --host-walks %d  (%s)\n"
                % (a.case, a.rounds, a.window, a.edges, a.walks, a.host_walks, torch.cuda.get_device_name(0)))
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
