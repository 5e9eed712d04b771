"""Timing of the device walk generator (synthetic_data_gen.generate_random_walks_batched: scn_sssp_paths + scn_walk_assemble)
beside the host generator (generate_random_walks) with fresh waypoints per walk, i.e. WITHOUT a waypoint pool:

  (a) the 400-point complex, --small-walks walks, both metrics: both generators run to the end;
  (b) the |E| ~ 1M complex of bench.py's headline configuration, --walks walks, metric="euclid": the host generator cannot make
      them in any reasonable time (two scipy trees per attempt), so a probe of --probe walks sizes one call that lasts about
      --budget seconds and its walks per second are reported from what that call produced; the device generator makes them all.
Per case: seconds, walks and trees per second, rounds, acceptance rate, generations per tree, and the device time inside the two
kernels' calls (HIP events around each launch) as a share of the generator's wall time.  Prints one JSON line per case and writes
them all to --out.

    python tools/walks_time.py [--case a|b|ab] [--walks 4096] [--small-walks 1000] [--edges 1000000] [--budget 60] [--probe 4] [--out profiles/walks.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scone_gcn_amd import synthetic_data_gen as g                          # noqa: E402

T0 = time.perf_counter()


def _say(*a):
    print("[walks_time %.0fs]" % (time.perf_counter() - T0), *a, file=sys.stderr, flush=True)


class KernelClock:
    """HIP events around every call of the two device entry points the generator makes."""

    def __init__(self):
        self.spans = {"scn_sssp_paths": [], "scn_walk_assemble": []}
        self._real = (g.sssp_paths_device, g.walk_assemble_device)

    def _timed(self, name, fn):
        def run(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            self.spans[name].append((e0, e1))
            return out
        return run

    def __enter__(self):
        g.sssp_paths_device = self._timed("scn_sssp_paths", self._real[0])
        g.walk_assemble_device = self._timed("scn_walk_assemble", self._real[1])
        return self

    def __exit__(self, *exc):
        g.sssp_paths_device, g.walk_assemble_device = self._real

    def seconds(self):
        torch.cuda.synchronize()
        return {k: sum(a.elapsed_time(b) for a, b in v) / 1e3 for k, v in self.spans.items()}


def device_case(cx, m, metric, seed=1030):
    g.generate_random_walks_batched(cx, m=min(m, 64), seed=seed + 1, metric=metric)       # warm-up: library, upload of the graph
    torch.cuda.synchronize()
    stats = {}
    with KernelClock() as clock:
        t0 = time.perf_counter()
        walks, ways = g.generate_random_walks_batched(cx, m=m, seed=seed, metric=metric, stats=stats, return_waypoints=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ks = clock.seconds()
    lens = np.asarray([len(w) for w in walks])
    return {"device_s": dt, "device_walks_per_s": m / dt, "device_trees_per_s": stats["trees"] / dt, "rounds": stats["rounds"],
            "attempts": stats["attempts"], "acceptance": m / stats["attempts"], "generations_per_tree": stats["generations"] / stats["trees"],
            "sssp_paths_s": ks["scn_sssp_paths"], "walk_assemble_s": ks["scn_walk_assemble"],
            "sssp_paths_share": ks["scn_sssp_paths"] / dt, "walk_assemble_share": ks["scn_walk_assemble"] / dt,
            "mean_walk_nodes": float(lens.mean()), "longest_walk": int(lens.max()),
            "distinct_waypoints": int(len(np.unique(ways[:, 1:3])))}


def case_a(m):
    cx = g.random_SC_graph(400)
    out = []
    for metric in ("hops", "euclid"):
        t0 = time.perf_counter()
        g.generate_random_walks(cx, m=m, metric=metric)
        host_s = time.perf_counter() - t0
        row = {"case": "a", "metric": metric, "n_nodes": int(cx.n_nodes), "n_edges": int(cx.n_edges), "walks": m, "host_s": host_s,
               "host_walks_per_s": m / host_s}
        row.update(device_case(cx, m, metric))
        row["ratio_host_over_device"] = host_s / row["device_s"]
        out.append(row)
    return out


def case_b(m, edges, budget, probe):
    _say("building the |E| ~ %d complex" % edges)
    cx = g.random_SC_graph(g.calibrate_n_points(edges))
    _say("host generator: probe of %d walks" % probe)
    t0 = time.perf_counter()
    g.generate_random_walks(cx, m=probe, seed=1, metric="euclid")
    per_walk = (time.perf_counter() - t0) / probe
    m_host = int(max(probe, min(m, budget / per_walk)))
    _say("host generator: %d walks (%.2f s per walk in the probe)" % (m_host, per_walk))
    t0 = time.perf_counter()
    g.generate_random_walks(cx, m=m_host, seed=2, metric="euclid")
    host_s = time.perf_counter() - t0
    row = {"case": "b", "metric": "euclid", "n_nodes": int(cx.n_nodes), "n_edges": int(cx.n_edges), "walks": m,
           "host_budget_s": budget, "host_walks_made": m_host, "host_s": host_s, "host_walks_per_s": m_host / host_s,
           "host_s_for_all_walks_extrapolated": m * host_s / m_host}
    _say("device generator: %d walks" % m)
    row.update(device_case(cx, m, "euclid"))
    row["ratio_walks_per_s_device_over_host"] = row["device_walks_per_s"] / row["host_walks_per_s"]
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="ab")
    ap.add_argument("--walks", type=int, default=4096)
    ap.add_argument("--small-walks", type=int, default=1000)
    ap.add_argument("--edges", type=int, default=1_000_000)
    ap.add_argument("--budget", type=float, default=60.0)
    ap.add_argument("--probe", type=int, default=4)
    ap.add_argument("--out", default=os.path.join("profiles", "walks.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "walks_time needs a GPU: a time taken elsewhere says nothing"
    rows = []
    if "a" in a.case:
        rows += case_a(a.small_walks)
    if "b" in a.case:
        rows += case_b(a.walks, a.edges, a.budget, a.probe)
    with open(a.out, "w") as f:
        f.write("# python tools/walks_time.py --case %s --walks %d --small-walks %d --edges %d --budget %g --probe %d  (%s)\n"
                % (a.case, a.walks, a.small_walks, a.edges, a.budget, a.probe, torch.cuda.get_device_name(0)))
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
