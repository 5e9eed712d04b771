"""Timing of the device Markov baseline (scone_gcn_amd/markov_model.py): Markov_Model.train and Markov_Model.test(hops = 2).

  (a) the 400-point generated data set, 1000 walks (800 train the table, the 200 others are tested): the device calls beside a
      host dictionary loop that restates the reference's algorithm (markov_model.py: every walk of `order` nodes enumerated by a
      double loop over nodes x shorter walks, nested dictionaries of counts, one predict() per prefix and hop), and their ratio;
  (b) the |E| ~ 1M complex of bench.py's headline configuration with as many walks as the generator (generate_random_walks,
      Euclidean metric, pooled waypoints) yields in a minute -- two timed calls of --probe and 4 x --probe walks size the one call
      that is kept -- at orders 1 and 2: seconds, paths per second, table bytes and the largest D.  Nothing to compare with at this size.
Device-synchronised wall time (both calls end in a device-to-host copy), the median of --reps windows after a warm-up call; a
window repeats the call until it lasts --window seconds.  Prints one JSON line per case and writes them all to --out.

    python tools/markov_time.py [--case a|b|ab] [--reps 5] [--window 0.2] [--edges 1000000] [--minute 60] [--max-walks 50000] [--out profiles/markov.txt]

--backoff times the variable-order table (Markov_Backoff) on the walks of (b) instead: the direct order-2 table beside the hashed one
read without back-off at K = 2 (equal results are asserted; both times and their ratio), then back-off at K = 4 and 8 with the table's
states per order, capacity, bytes and mean probe length.  It writes profiles/markov_backoff.txt unless --out says otherwise.
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
from scone_gcn_amd.markov_model import Markov_Backoff, Markov_Model, hash_mix, ragged, table_rows    # noqa: E402

T0 = time.perf_counter()


def _say(*a):
    print("[markov_time %.0fs]" % (time.perf_counter() - T0), *a, file=sys.stderr, flush=True)


def _timed(fn, reps, window):
    """Median seconds per call over `reps` windows of at least `window` seconds each, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(reps):
        n, t0 = 0, time.perf_counter()
        while True:
            fn()
            n += 1
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= window:
                break
        per_call.append(dt / n)
    return float(np.median(per_call)), float(np.min(per_call)), float(np.max(per_call))


# ---- the host loop of case (a): the reference's algorithm on dictionaries ----

def host_train(nbrs, order, paths):
    walks = [[v] for v in range(len(nbrs))]
    for _ in range(order - 1):                                   # all walks of `order` nodes: nodes x shorter walks, an edge test each
        walks = [w + [v] for v in range(len(nbrs)) for w in walks if v in nbrs[w[-1]]]
    weights = {tuple(w): {u: 0 for u in nbrs[w[-1]]} for w in walks}
    for p in paths:
        for i in range(len(p) - order):
            weights[tuple(p[i:i + order])][p[i + order]] += 1
    for dist in weights.values():
        total = sum(dist.values())
        if total:
            for u in dist:
                dist[u] /= total
    return weights


def host_test(weights, order, prefixes, targets, hops, rs):
    cur = [list(p) for p in prefixes]
    for _ in range(hops):
        for i, p in enumerate(prefixes):
            if len(p) >= order:
                dist = weights[tuple(cur[i][-order:])]
                best = max(dist.values())
                tied = [u for u, pr in dist.items() if pr == best]
                cur[i].append(tied[0] if len(tied) == 1 else tied[rs.randint(len(tied))])
    return float(np.mean([c[-1] == t for c, t in zip(cur, targets)]))


def case_a(reps, window, orders=(1, 2)):
    cx = g.random_SC_graph(400)
    paths = g.generate_random_walks(cx, m=1000)
    rs = np.random.RandomState(0)
    prefixes, suffixes, _ = g.split_paths(paths, rs)
    mask = np.array([1] * 800 + [0] * 200)
    rs.shuffle(mask)
    full = [p + s for p, s in zip(prefixes, suffixes)]
    train = [full[i] for i in np.flatnonzero(mask == 1)]
    test_pre = [prefixes[i] for i in np.flatnonzero(mask == 0)]
    test_t2 = np.asarray([suffixes[i][1] for i in np.flatnonzero(mask == 0)])
    nbr, deg = g.neighborhood_table(cx)
    nbrs = [set(int(u) for u in row[row >= 0]) for row in nbr]
    out = []
    for order in orders:
        mm = Markov_Model(order)
        t_train = _timed(lambda: mm.train(nbr, train), reps, window)
        t_test = _timed(lambda: mm.test(test_pre, test_t2, 2), reps, window)
        acc = float(mm.test(test_pre, test_t2, 2))
        t0 = time.perf_counter()
        weights = host_train(nbrs, order, train)
        h_train = time.perf_counter() - t0
        t0 = time.perf_counter()
        h_acc = host_test(weights, order, test_pre, test_t2, 2, np.random.RandomState(0))
        h_test = time.perf_counter() - t0
        out.append({"case": "a", "order": order, "n_nodes": int(cx.n_nodes), "D": int(nbr.shape[1]), "train_paths": len(train),
                    "test_paths": len(test_pre), "table_bytes": int(mm.counts.numel() * 4),
                    "device_train_s": t_train[0], "device_train_s_min_max": t_train[1:], "device_test_hops2_s": t_test[0],
                    "device_test_hops2_s_min_max": t_test[1:], "host_loop_train_s": h_train, "host_loop_test_hops2_s": h_test,
                    "train_ratio_host_over_device": h_train / t_train[0], "test_ratio_host_over_device": h_test / t_test[0],
                    "device_acc_hops2": acc, "host_loop_acc_hops2": h_acc,
                    "note": "the device times include the upload of the paths (and, for train, of the graph) and the copy back"})
    return out


def walks_b(edges, minute, probe, max_walks):
    """The complex and the walks of case (b): (cx, nbr, train (ptr, nodes), test (pre_ptr, pre_nodes, targets), what to report)."""
    _say("building the |E| ~ %d complex" % edges)
    cx = g.random_SC_graph(g.calibrate_n_points(edges))
    nbr, deg = g.neighborhood_table(cx)
    gen = lambda m, seed: g.generate_random_walks(cx, m=m, seed=seed, waypoint_pool=8, metric="euclid")
    # two probes split the generator's time into its fixed part (the waypoints' shortest-path trees, built once per call) and
    # the time per walk; the call that is kept is sized to last `minute` seconds
    t = []
    for m in (probe, 4 * probe):
        _say("walks: probe of %d" % m)
        t0 = time.perf_counter()
        gen(m, 1)
        t.append(time.perf_counter() - t0)
    per_walk = max((t[1] - t[0]) / (3 * probe), 1e-7)
    fixed = max(t[0] - probe * per_walk, 0.0)
    m = max(probe, int((minute - fixed) / per_walk))
    capped, m = m > max_walks, min(m, max_walks)                 # host memory: a walk is a Python list of ~1000 nodes at |E| ~ 1M
    _say("walks: %d (fixed part %.1f s, %.2f ms per walk)" % (m, fixed, 1e3 * per_walk))
    t0 = time.perf_counter()
    walks = gen(m, 2)
    gen_s = time.perf_counter() - t0
    ptr, nodes = ragged(walks)
    n_test = max(1, len(walks) // 5)
    # the test's prefixes: the last fifth of the walks without their last two nodes, the target their last node
    pre_ptr = np.concatenate([[0], np.cumsum(np.diff(ptr)[-n_test:] - 2)]).astype(np.int32)
    pre_nodes = np.concatenate([nodes[ptr[i]:ptr[i + 1] - 2] for i in range(len(walks) - n_test, len(walks))]).astype(np.int32)
    targets = nodes[ptr[1:][-n_test:] - 1]
    n_train = len(walks) - n_test                                # the table is trained on the other four fifths
    ptr, nodes = ptr[:n_train + 1], nodes[:ptr[n_train]]
    _say("%d walks (%d of them train the table, %d nodes), generated in %.1f s" % (len(walks), n_train, len(nodes), gen_s))
    return cx, nbr, (ptr, nodes), (pre_ptr, pre_nodes, targets), {"n_train": n_train, "n_test": n_test, "gen_s": gen_s, "capped": capped}


def case_b(reps, window, edges, minute, probe, max_walks, orders=(1, 2)):
    cx, nbr, (ptr, nodes), (pre_ptr, pre_nodes, targets), meta = walks_b(edges, minute, probe, max_walks)
    n_train, n_test, gen_s, capped = meta["n_train"], meta["n_test"], meta["gen_s"], meta["capped"]
    out = []
    for order in orders:
        mm = Markov_Model(order)
        t_train = _timed(lambda: mm.train(nbr, (ptr, nodes)), reps, window)
        t_test = _timed(lambda: mm.test((pre_ptr, pre_nodes), targets, 2), reps, window)
        out.append({"case": "b", "order": order, "n_nodes": int(cx.n_nodes), "n_edges": int(cx.n_edges), "D": int(nbr.shape[1]),
                    "walks": n_train, "walk_nodes": int(len(nodes)), "longest_walk": int(np.diff(ptr).max()),
                    "generator_s": gen_s, "walks_capped_by_max_walks": bool(capped), "table_rows": int(table_rows(nbr.shape[0], nbr.shape[1], order)),
                    "table_bytes": int(mm.counts.numel() * 4), "train_s": t_train[0], "train_s_min_max": t_train[1:],
                    "train_paths_per_s": n_train / t_train[0], "train_windows_per_s": float(np.maximum(np.diff(ptr) - order, 0).sum()) / t_train[0],
                    "test_paths": n_test, "test_hops2_s": t_test[0], "test_hops2_s_min_max": t_test[1:],
                    "test_paths_per_s": n_test / t_test[0], "acc_hops2": float(mm.test((pre_ptr, pre_nodes), targets, 2)),
                    "note": "train and test include the upload of the graph table and of the paths and the copy back"})
    return out


def mean_probe_length(mb):
    """Slots read to find a key of the table, averaged over its keys: 1 + the distance of a key's slot from its home slot."""
    keys = mb.keys.cpu().numpy().view(np.uint64)
    at = np.flatnonzero(keys != np.uint64(2 ** 64 - 1))
    home = (hash_mix(keys[at]) & np.uint64(mb.capacity - 1)).astype(np.int64)
    return float(1.0 + ((at - home) & (mb.capacity - 1)).mean()) if len(at) else 0.0


def case_backoff(reps, window, edges, minute, probe, max_walks, orders=(4, 8)):
    """On the walks of case (b): train and test(hops = 2) of the direct order-2 table beside the hashed table read without back-off
    at K = 2 (equal results; both times and their ratio), then the hashed table with back-off at the given maximum orders (nothing
    to compare with: no other table holds these orders at this size)."""
    cx, nbr, (ptr, nodes), (pre_ptr, pre_nodes, targets), meta = walks_b(edges, minute, probe, max_walks)
    shape = {"case": "backoff", "n_nodes": int(cx.n_nodes), "n_edges": int(cx.n_edges), "D": int(nbr.shape[1]), "walks": meta["n_train"],
             "walk_nodes": int(len(nodes)), "test_paths": meta["n_test"], "walks_capped_by_max_walks": bool(meta["capped"])}

    def times(mm):
        t_train = _timed(lambda: mm.train(nbr, (ptr, nodes)), reps, window)
        t_test = _timed(lambda: mm.test((pre_ptr, pre_nodes), targets, 2), reps, window)
        return t_train, t_test

    def table(mb):
        return {"n_states": mb.n_states, "capacity": mb.capacity, "table_bytes": mb.table_bytes, "load": sum(mb.n_states) / mb.capacity,
                "mean_probe_length": mean_probe_length(mb)}

    direct, hashed = Markov_Model(2), Markov_Backoff(2, backoff=False)
    (d_train, d_test), (h_train, h_test) = times(direct), times(hashed)
    pred_d, tied_d = direct.predict_paths((pre_ptr, pre_nodes), 2)
    pred_h, tied_h = hashed.predict_paths((pre_ptr, pre_nodes), 2)
    equal = bool(np.array_equal(pred_d, pred_h) and np.array_equal(tied_d, tied_h)
                 and np.array_equal(direct.next_node_probs((pre_ptr, pre_nodes)), hashed.next_node_probs((pre_ptr, pre_nodes))))
    acc_d, acc_h = float(direct.test((pre_ptr, pre_nodes), targets, 2)), float(hashed.test((pre_ptr, pre_nodes), targets, 2))
    assert equal and acc_d == acc_h, "the hashed table without back-off differs from the direct order-2 table"
    out = [dict(shape, K=2, backoff=False, results_equal_direct_order_2=equal, acc_hops2=acc_h,
                direct_table_bytes=int(direct.counts.numel() * 4), direct_train_s=d_train[0], direct_train_s_min_max=d_train[1:],
                direct_test_hops2_s=d_test[0], direct_test_hops2_s_min_max=d_test[1:], hashed_train_s=h_train[0],
                hashed_train_s_min_max=h_train[1:], hashed_test_hops2_s=h_test[0], hashed_test_hops2_s_min_max=h_test[1:],
                train_ratio_hashed_over_direct=h_train[0] / d_train[0], test_ratio_hashed_over_direct=h_test[0] / d_test[0],
                **table(hashed))]
    del direct, hashed
    for K in orders:
        mb = Markov_Backoff(K)
        t_train, t_test = times(mb)
        acc = float(mb.test((pre_ptr, pre_nodes), targets, 2))
        out.append(dict(shape, K=K, backoff=True, min_count=1, train_s=t_train[0], train_s_min_max=t_train[1:], test_hops2_s=t_test[0],
                        test_hops2_s_min_max=t_test[1:], acc_hops2=acc, used_order_hist_last_hop=np.bincount(mb.used_orders[:, -1],
                                                                                                          minlength=K + 1).tolist(),
                        compared_with="nothing: no other table holds these orders at this size", **table(mb)))
        del mb
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="ab")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--edges", type=int, default=1_000_000)
    ap.add_argument("--minute", type=float, default=60.0)
    ap.add_argument("--probe", type=int, default=200)         # well above the 48 waypoints: both probes build every tree
    ap.add_argument("--max-walks", type=int, default=50000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--backoff", action="store_true",
                    help="time the hashed variable-order table (Markov_Backoff) on the walks of case (b) instead; --out profiles/markov_backoff.txt")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join("profiles", "markov_backoff.txt" if a.backoff else "markov.txt")
    assert torch.cuda.is_available(), "markov_time needs a GPU: a time taken elsewhere says nothing"
    rows = []
    if a.backoff:
        a.case = "b --backoff"
        rows += case_backoff(a.reps, a.window, a.edges, a.minute, a.probe, a.max_walks)
    else:
        if "a" in a.case:
            rows += case_a(a.reps, a.window)
        if "b" in a.case:
            rows += case_b(a.reps, a.window, a.edges, a.minute, a.probe, a.max_walks)
    with open(a.out, "w") as f:
        f.write("# python tools/markov_time.py --case %s --reps %d --window %g --edges %d --minute %g --probe %d  (%s)\n"
                % (a.case, a.reps, a.window, a.edges, a.minute, a.probe, torch.cuda.get_device_name(0)))
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
