"""Timing of the device multi-hop probability tree (Scone_GCN.multi_hop_accuracy_dist, STM:154-206), of the beam search
(Scone_GCN.predict_paths_beam) and of the sampled decoder (Scone_GCN.sample_paths).

  (a) the 400-point generated data set, 1000 paths, dist with hops = 2: the device pipeline against a host loop that calls
      scone_func once per tree leaf (what the reference does with model_single);
  (b) |E| ~ 1M, 4096 roots (8-step random walks), hops = 2: leaves per second;
  (c) the complex and roots of (b), beam search with hops = 4 and beam = 8: leaves per second (every entry a level pushes through
      the forward is a leaf), to be read against (b) of the same run.  The share of kernel time the forward kernels take comes from
      a run of `--case c` alone under `rocprofv3 --kernel-trace --stats`, whose kernel table `--kernel-stats FILE` sums up.
  (d) the complex and roots of (b), sampled paths with hops = 8 and 256 samples per root (--d-roots R: the first R of the roots):
      seconds per call, leaves evaluated (the distinct entries of every level that goes through the forward) and leaves per
      second, to be read against (b) and (c) of the same run, and per level the distinct entries against the live samples.  The
      share of kernel time of sample_draw_kernel / sample_expand_kernel comes from a run of `--case d` alone under
      `rocprofv3 --kernel-trace --stats`, summed by `--kernel-stats FILE`.
Device-synchronised wall time (torch.cuda.synchronize around the call), after warm-up calls.  Prints one JSON line per case and
writes them all to --out.

--skip dense|field|both runs cases (b) and (c) with Scone_GCN.multi_hop_skip set accordingly; `both` times the two in one process on
one set of tensors and reports their ratio, whether the results agree, and the per-level active fractions of the field lists.

    python tools/multihop_time.py [--case a|b|c|d|abcd] [--d-roots 4096] [--skip dense] [--reps 3] [--host-roots 40] [--out profiles/multihop_time.json]
    python tools/multihop_time.py --kernel-stats profiles/multihop_c_kernel_stats.csv
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import scone_oracle as so                                     # noqa: E402
from scone_gcn_amd import dataset_io, multihop, synthetic_data_gen as g, trajectory_experiments as te   # noqa: E402
from scone_gcn_amd.complex import SimplicialComplex                        # noqa: E402
from scone_gcn_amd.scone_trajectory_model import Scone_GCN                # noqa: E402
from scone_gcn_amd.synthetic_data_gen import SparseFlows                   # noqa: E402

HIDDEN = [(3, 16)] * 3


def _net(shifts, inputs, y, seed=0):
    net = Scone_GCN(1, 1e-3, 100, 0.0, verbose=False)
    net.setup(te.scone_func, HIDDEN, shifts, inputs, y, None, np.ones(len(y)))
    rs = np.random.RandomState(seed)
    net._install([0.3 * rs.randn(*s) for s in so.weight_shapes(1, HIDDEN, 1)])
    return net


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def host_loop_target_probs(net, shifts, readout, flows, targets, nbrhoods, E_lookup, last_nodes, hops):
    """The reference's loop structure (STM:163-204): one scone_func call per leaf, children built on the host."""
    nb = [n[n != -1] for n in np.asarray(nbrhoods)]
    out = np.zeros(len(last_nodes))
    for i in range(len(last_nodes)):
        leaves = [(int(last_nodes[i]), flows[i].copy(), 1.0)]
        for _ in range(hops):
            new = []
            for v, f, p in leaves:
                probs = np.exp(te.scone_func(net.weights, *shifts, readout, v, f).cpu().numpy()[:, 0])
                for j, u in enumerate(nb[v]):
                    f2 = f.copy()
                    f2[E_lookup[tuple(sorted((v, int(u))))]] = 1 if v < u else -1
                    new.append((int(u), f2, p * probs[j]))
            leaves = new
        hit = [p for v, _, p in leaves if v == targets[i]]
        out[i] = sum(hit) / len(hit) if hit else np.nan
    return out


def case_a(reps, host_roots):
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        os.chdir(d)
        try:
            dataset_io.generate_dataset(400, 1000, folder="mht", holes=True)
            hp = te.hyperparams(["prog"])
            inputs_all, y_all, train_mask, test_mask, shifts, _, E_lookup, nbrhoods, _, targets_all, prefixes = \
                te.data_setup(hops=(1, 2), folder_suffix="mht", hp=hp)
        finally:
            os.chdir(cwd)
    inputs, y = inputs_all[0], y_all[0]
    net = _net(shifts, inputs, y)
    N = len(y)
    args = (shifts, inputs, targets_all[1], [train_mask, test_mask], nbrhoods, E_lookup, inputs[1], prefixes, 2)
    t_dev = _timed(lambda: net.multi_hop_accuracy_dist(*args), reps)
    leaves = int(sum(len(nbrhoods[v][nbrhoods[v] >= 0]) for v in inputs[1]))
    k = min(host_roots, N)
    X = inputs[-1]
    sub = X.select(np.arange(k)) if isinstance(X, SparseFlows) else np.asarray(X)[:k]
    dense = sub.todense() if isinstance(sub, SparseFlows) else sub
    dev_tp = net.multi_hop_target_probs([inputs[0], inputs[1][:k], sub], targets_all[1][:k], nbrhoods, E_lookup, inputs[1][:k], 2)
    host_loop_target_probs(net, shifts, inputs[0], dense[:1], targets_all[1][:1], nbrhoods, E_lookup, inputs[1][:1], 2)   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_tp = host_loop_target_probs(net, shifts, inputs[0], dense, targets_all[1][:k], nbrhoods, E_lookup, inputs[1][:k], 2)
    torch.cuda.synchronize()
    t_host = (time.perf_counter() - t0) * N / k
    ok = ~np.isnan(host_tp)
    return {"case": "a", "n_edges": int(dense.shape[1]), "roots": N, "hops": 2, "level1_leaves": leaves,
            "device_s": t_dev, "device_traj_per_s": N / t_dev, "host_loop_s_extrapolated": t_host, "host_loop_roots_timed": k,
            "host_loop_traj_per_s": N / t_host, "speedup": t_host / t_dev,
            "max_abs_diff_vs_host_loop": float(np.abs(dev_tp[ok] - host_tp[ok]).max()) if ok.any() else None}


def _say(*a):
    print("[multihop_time %.0fs]" % (time.perf_counter() - T0), *a, file=sys.stderr, flush=True)


T0 = time.perf_counter()


_BIG = {}


def _big(roots=4096):
    """The |E| ~ 1M complex, its roots and the model of cases (b) and (c), built once per run."""
    if roots not in _BIG:
        _BIG[roots] = _build_big(roots)
    return _BIG[roots]


def _build_big(roots):
    _say("building the |E| ~ 1M complex")
    cx = g.random_SC_graph(g.calibrate_n_points(1_000_000))
    sc = SimplicialComplex(cx)
    _say("random walks")
    # uniform random walks of 8 steps from random nodes (generate_random_walks' waypoint paths take many minutes at this size): the
    # flow of a walk is +1 / -1 on every edge it crosses (SDG:327-344), the walk's end is the last node
    rs = np.random.RandomState(1)
    nb = np.asarray(sc.nbrhoods)
    deg = (nb >= 0).sum(axis=1)
    walk = [rs.randint(cx.n_nodes, size=roots)]
    for _ in range(8):
        v = walk[-1]
        walk.append(nb[v, (rs.rand(roots) * deg[v]).astype(np.int64)])
    a, b = np.stack(walk[:-1], 1).ravel(), np.stack(walk[1:], 1).ravel()
    M = cx.n_nodes
    code = cx.edges[:, 0].astype(np.int64) * M + cx.edges[:, 1]
    order = np.argsort(code)
    idx = order[np.searchsorted(code[order], np.minimum(a, b) * M + np.maximum(a, b))]
    flows = SparseFlows(np.arange(0, 8 * roots + 1, 8, dtype=np.int64), idx.astype(np.int64),
                        np.where(a < b, 1.0, -1.0).astype(np.float32), cx.n_edges)
    last = walk[-1]
    shifts, readout, _ = te.setup_from_complex(sc, "scone")
    E_lookup = {(int(p), int(q)): k for k, (p, q) in enumerate(cx.edges.tolist())}
    _say("data ready")
    first = [rs.choice(nb[v][nb[v] >= 0]) for v in last]
    targets = np.array([rs.choice(nb[b][nb[b] >= 0]) for b in first])
    y = np.zeros((len(last), sc.max_degree, 1))
    inputs = [readout, last, flows]
    return _net(shifts, inputs, y), inputs, targets, sc, E_lookup, last, nb, cx


def _modes(skip):
    return ["dense", "field"] if skip == "both" else [skip]


def _skip_runs(net, skip, reps, call, leaves):
    """call() under every mode of `skip`: {mode_s, mode_leaves_per_s, ...} plus, for "field", the active fractions (mean and
    maximum over the forwards of one call, per list: the input and every layer) and, for "both", the ratio.  Returns (record, the
    last result per mode)."""
    rec, last = {}, {}
    for mode in _modes(skip):
        net.multi_hop_skip = mode
        t_first = time.perf_counter()
        call()                                                               # (field: builds and uploads the block tables)
        torch.cuda.synchronize()
        rec[mode + "_first_call_s"] = time.perf_counter() - t_first
        out = []
        t = _timed(lambda: out.append(call()), reps)
        last[mode] = out[-1]
        rec[mode + "_s"], rec[mode + "_leaves_per_s"] = t, leaves / t
        if mode == "field":
            net._multi_hop_fractions = fr = []
            call()
            net._multi_hop_fractions = None
            per = np.array([[f["input"]] + list(f["fwd"]) for f in fr]) if fr else np.zeros((0, 1))
            rec["field_forwards_per_call"] = len(fr)
            rec["active_fraction_mean"] = per.mean(axis=0).tolist() if len(fr) else None      # [input, layer 1 .. L]
            rec["active_fraction_max"] = per.max(axis=0).tolist() if len(fr) else None
    net.multi_hop_skip = "dense"
    if skip == "both":
        rec["dense_over_field"] = rec["dense_s"] / rec["field_s"]
    rec["device_s"] = rec[_modes(skip)[-1] + "_s"]
    rec["leaves_per_s"] = leaves / rec["device_s"]
    return rec, last


def case_b(reps, roots=4096, skip="dense"):
    net, inputs, targets, sc, E_lookup, last, nb, cx = _big(roots)
    net.multi_hop_skip = _modes(skip)[0]                                               # (--skip field: no dense forward in the run)
    t_tab = time.perf_counter()
    net.multi_hop_target_probs(inputs, targets, sc.nbrhoods, E_lookup, last, 1)        # builds and caches the step tables
    t_tab = time.perf_counter() - t_tab
    _say("step tables %.1f s; timing" % t_tab)
    leaves = len(last) + int((nb[last] >= 0).sum())
    rec, res = _skip_runs(net, skip, reps, lambda: net.multi_hop_target_probs(inputs, targets, sc.nbrhoods, E_lookup, last, 2), leaves)
    if skip == "both":
        d, f = res["dense"], res["field"]
        ok = ~np.isnan(d)
        rec["nan_pattern_equal"] = bool(np.array_equal(np.isnan(d), np.isnan(f)))
        rec["max_rel_diff_field_vs_dense"] = float((np.abs(f[ok] - d[ok]) / np.maximum(np.abs(d[ok]), 1e-300)).max()) if ok.any() else None
    return {"case": "b", "skip": skip, "n_edges": int(cx.n_edges), "roots": len(last), "hops": 2, "leaves_evaluated": leaves,
            "first_call_hops1_incl_step_tables_s": t_tab, **rec}


def case_c(reps, roots=4096, hops=4, beam=8, skip="dense"):
    net, inputs, targets, sc, E_lookup, last, nb, cx = _big(roots)
    net.multi_hop_skip = _modes(skip)[0]
    t_tab = time.perf_counter()
    net.predict_paths_beam(inputs, 1, 1, sc.nbrhoods, E_lookup)                        # builds and caches the step tables
    t_tab = time.perf_counter() - t_tab
    _say("step tables %.1f s; timing the beam" % t_tab)
    widths = [1]
    for _ in range(hops - 1):
        widths.append(min(beam, widths[-1] * sc.max_degree))
    leaves = len(last) * int(sum(widths))
    rec, res = _skip_runs(net, skip, reps, lambda: net.predict_paths_beam(inputs, hops, beam, sc.nbrhoods, E_lookup), leaves)
    paths, logp = res[_modes(skip)[-1]]
    if skip == "both":
        rec["paths_equal"] = bool(np.array_equal(res["dense"][0], res["field"][0]))
        rec["max_abs_logp_diff_field_vs_dense"] = float(np.nanmax(np.abs(np.where(np.isfinite(res["dense"][1]),
                                                                                   res["field"][1] - res["dense"][1], 0.0))))
    return {"case": "c", "skip": skip, "n_edges": int(cx.n_edges), "roots": len(last), "hops": hops, "beam": beam,
            "level_widths": widths, "leaves_evaluated": leaves, "live_paths": int((paths[:, :, -1] >= 0).sum()),
            "mean_best_logp": float(logp[:, 0].mean()), "first_call_hops1_incl_step_tables_s": t_tab, **rec}


def case_d(reps, roots=4096, hops=8, samples=256, skip="dense", d_roots=None):
    net, inputs, targets, sc, E_lookup, last, nb, cx = _big(roots)
    R = len(last) if not d_roots else min(int(d_roots), len(last))
    if R < len(last):
        inputs = [inputs[0], np.asarray(last)[:R], inputs[2].select(np.arange(R))]
    net.multi_hop_skip = _modes(skip)[0]
    t_tab = time.perf_counter()
    net.sample_paths(inputs, 1, 1, nbrhoods=sc.nbrhoods, E_lookup=E_lookup)            # builds and caches the step tables
    t_tab = time.perf_counter() - t_tab
    _say("step tables %.1f s; counting the levels" % t_tab)
    levels = multihop.sample_levels(net, inputs, hops, samples, 0, 1.0, sc.nbrhoods, E_lookup)
    entries = [int(l.node.shape[0]) for l in levels]                                   # level 0 .. hops; the last one is not evaluated
    live = [int((l.entry_of >= 0).sum().item()) for l in levels]
    del levels
    leaves = int(sum(entries[:hops]))
    _say("entries per level %s; timing" % entries)
    rec, res = _skip_runs(net, skip, reps, lambda: net.sample_paths(inputs, hops, samples, nbrhoods=sc.nbrhoods, E_lookup=E_lookup),
                          leaves)
    paths, logp = res[_modes(skip)[-1]]
    if skip == "both":
        rec["paths_equal"] = bool(np.array_equal(res["dense"][0], res["field"][0]))
    return {"case": "d", "skip": skip, "n_edges": int(cx.n_edges), "roots": R, "hops": hops, "samples": samples,
            "level_entries": entries, "level_live_samples": live,
            "entries_per_sample": [e / max(s, 1) for e, s in zip(entries, live)], "leaves_evaluated": leaves,
            "leaves_if_unmerged": int(sum(live[:hops])), "live_paths": int((paths[:, :, -1] >= 0).sum()),
            "mean_logp": float(logp[np.isfinite(logp)].mean()), "first_call_hops1_incl_step_tables_s": t_tab, **rec}


def kernel_shares(path):
    """Shares of kernel time from a `rocprofv3 --kernel-trace --stats` kernel table (Name, Calls, TotalDurationNs, ...): the forward
    kernels (the fused layer kernels `scn::fwd_*` and the readout) and every multi-hop kernel of csrc/scn_hops.hip by name."""
    import csv
    with open(path, newline="") as f:
        rows = [(r["Name"], int(r["Calls"]), int(r["TotalDurationNs"])) for r in csv.DictReader(f)]
    total = sum(t for _, _, t in rows)
    fwd = sum(t for n, _, t in rows if "scn::fwd_" in n or "scn::readout_fwd" in n)
    hops = {}
    for n, c, t in rows:
        for k in ("sample_draw", "sample_expand", "beam_step", "hop_select", "tree_expand", "tree_copy_list", "tree_patch_list", "tree_copy", "tree_patch", "tree_target",
                  "field_mark", "field_hop", "field_count", "field_scan", "field_fill", "clear_list"):
            if k + "_kernel" in n:
                hops[k] = {"calls": c, "total_ns": t, "share": t / total}
                break
    field = sum(v["total_ns"] for k, v in hops.items() if k.startswith("field_"))
    slabs_list = sum(v["total_ns"] for k, v in hops.items() if k in ("tree_copy_list", "tree_patch_list"))
    return {"kernel_time_s": total / 1e9, "forward_share": fwd / total, "multihop_kernels": hops,
            "scn_field_lists_share": field / total, "scn_tree_slabs_list_share": slabs_list / total,
            "other_share": 1.0 - (fwd + sum(v["total_ns"] for v in hops.values())) / total}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="ab")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip", default="dense", choices=["dense", "field", "both"], help="multi_hop_skip of cases b and c")
    ap.add_argument("--host-roots", type=int, default=40)
    ap.add_argument("--d-roots", type=int, default=0, help="case d on the first R roots of case b's (0: all of them)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv: print the shares of kernel time and exit")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_shares(a.kernel_stats)))
        return
    torch.cuda.set_device(0)
    res = []
    if "a" in a.case:
        res.append(case_a(a.reps, a.host_roots))
        print(json.dumps(res[-1]), flush=True)
    if "b" in a.case:
        res.append(case_b(a.reps, skip=a.skip))
        print(json.dumps(res[-1]), flush=True)
    if "c" in a.case:
        res.append(case_c(a.reps, skip=a.skip))
        print(json.dumps(res[-1]), flush=True)
    if "d" in a.case:
        res.append(case_d(a.reps, skip=a.skip, d_roots=a.d_roots))
        print(json.dumps(res[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
