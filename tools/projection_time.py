"""Timing of the device projection baseline (scone_gcn_amd/projection_model.py): Projection_Model.embed and .predict.

  (a) the 400-point generated data set, 1000 walks: the device calls beside the host route the reference takes -- a dense
      scipy.linalg.null_space of the (E, E) matrix L1, then V V^T F and a loop over the rows (projection_model.py) -- and their ratio;
  (b) the |E| ~ 1M complex of bench.py's headline configuration with 4096 flows (prefixes of generated walks): seconds of embed (one
      call: it is the conjugate-gradient solve that takes the time), its iteration count, final relative residual, dimension and
      the eigenvalues of the probes' Gram matrix, and seconds of predict.  Nothing to compare with at this size; if embed does not
      converge within max_iter or the probes saturate, that is what the row says.
Device-synchronised wall time (every call ends in a device-to-host copy); predict is the median of --reps windows after a warm-up
call, a window repeating the call until it lasts --window seconds.  Prints one JSON line per case and writes them all to --out.

    python tools/projection_time.py [--case a|b|ab] [--reps 5] [--window 0.2] [--edges 1000000] [--flows 4096] [--max-iter 50000] [--out profiles/projection.txt]
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
from scone_gcn_amd.complex import SimplicialComplex                        # noqa: E402
from scone_gcn_amd.projection_model import Projection_Model                # noqa: E402

T0 = time.perf_counter()


def _say(*a):
    print("[projection_time %.0fs]" % (time.perf_counter() - T0), *a, file=sys.stderr, flush=True)


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


def _prefix_flows(cx, walks):
    prefixes = [w[:-2] for w in walks if len(w) >= 4]
    return g.paths_to_flows(cx, prefixes), np.asarray([p[-1] for p in prefixes], np.int64)


def host_route(cx, flows, last):
    """The reference's algorithm on the host: (seconds of null_space, seconds of the projection and the row loop, probabilities)."""
    from scipy.linalg import null_space
    B1, B2 = g.incidence_matrices(cx)
    t0 = time.perf_counter()
    V = null_space((B1.T @ B1 + B2 @ B2.T).toarray())
    t_embed = time.perf_counter() - t0
    nbr, deg = g.neighborhood_table(cx)
    F, B1d = flows.todense()[:, :, 0].T.astype(np.float64), B1.toarray()
    t0 = time.perf_counter()
    projs = V @ V.T @ F
    res = np.zeros((len(last), nbr.shape[1]))
    for i, v in enumerate(last):
        n0, e0 = nbr[v, :deg[v]], np.where(B1d[v] != 0)[0]
        res[i, :len(n0)] = B1d[n0][:, e0] @ projs[e0, i]
    ex = np.exp(res - res.max(axis=1, keepdims=True))
    probs = ex / ex.sum(axis=1, keepdims=True)
    return t_embed, time.perf_counter() - t0, probs, V.shape[1]


def case_a(reps, window):
    cx = g.random_SC_graph(400)
    flows, last = _prefix_flows(cx, g.generate_random_walks(cx, m=1000))
    sc = SimplicialComplex(cx)
    pm = Projection_Model()
    t_embed = _timed(lambda: pm.embed(sc), reps, window)
    t_pred = _timed(lambda: pm.predict(flows, last), reps, window)
    h_embed, h_pred, h_probs, h_dim = host_route(cx, flows, last)
    return [{"case": "a", "n_edges": int(cx.n_edges), "flows": len(last), "dim": pm.dim, "host_dim": int(h_dim), "n_probes_used": pm.n_probes_used,
             "iterations": pm.iterations, "residual": pm.residual, "gram_eigenvalues": [float(w) for w in pm.gram_eigenvalues],
             "device_embed_s": t_embed[0], "device_embed_s_min_max": t_embed[1:], "device_predict_s": t_pred[0],
             "device_predict_s_min_max": t_pred[1:], "host_null_space_s": h_embed, "host_predict_s": h_pred,
             "embed_ratio_host_over_device": h_embed / t_embed[0], "predict_ratio_host_over_device": h_pred / t_pred[0],
             "largest_probability_difference": float(np.abs(pm.predict(flows, last) - h_probs).max()),
             "note": "embed includes the upload of L1 and of the probes and the copy of the basis back; predict the upload of the flows"}]


def case_b(reps, window, edges, n_flows, max_iter):
    _say("building the |E| ~ %d complex" % edges)
    cx = g.random_SC_graph(g.calibrate_n_points(edges))
    _say("its layout")
    sc = SimplicialComplex(cx)
    _say("%d walks" % n_flows)
    flows, last = _prefix_flows(cx, g.generate_random_walks(cx, m=n_flows, seed=2, waypoint_pool=8, metric="euclid"))
    row = {"case": "b", "n_nodes": int(cx.n_nodes), "n_edges": int(cx.n_edges), "n_faces": int(cx.n_faces), "D": int(sc.max_degree),
           "flows": len(last), "flow_entries": int(flows.ptr[-1]), "max_iter": max_iter, "tol": 1e-12}
    pm = Projection_Model(max_iter=max_iter)
    _say("embed")
    t0 = time.perf_counter()
    try:
        pm.embed(sc)
        torch.cuda.synchronize()
        row.update({"embed_s": time.perf_counter() - t0, "dim": pm.dim, "n_probes_used": pm.n_probes_used, "iterations": pm.iterations,
                    "residual": pm.residual, "gram_eigenvalues": [float(w) for w in pm.gram_eigenvalues]})
    except (RuntimeError, ValueError) as e:                      # not converged within max_iter, or the probes saturated: reported, not hidden
        row.update({"embed_s": time.perf_counter() - t0, "embed_failed": "%s: %s" % (type(e).__name__, e), "iterations": pm.iterations,
                    "residual": pm.residual})
        return [row]
    _say("embed: %.1f s, %d iterations, dim %d" % (row["embed_s"], pm.iterations, pm.dim))
    t_pred = _timed(lambda: pm.predict(flows, last), reps, window)
    V = torch.from_numpy(pm.basis).cuda()
    L_lo, L_up = sc.hodge_laplacians()
    row.update({"L1_V_max": float(np.abs((L_lo + L_up) @ pm.basis).max()), "predict_s": t_pred[0], "predict_s_min_max": t_pred[1:], "predict_flows_per_s": len(last) / t_pred[0],
                "orthonormality_error": float((V.T @ V - torch.eye(pm.dim, dtype=V.dtype, device=V.device)).abs().max()) if pm.dim else 0.0,
                "note": "embed includes the upload of L1 and of the probes and the copy of the basis back; predict the upload of the flows"})
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="ab")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--edges", type=int, default=1_000_000)
    ap.add_argument("--flows", type=int, default=4096)
    ap.add_argument("--max-iter", type=int, default=50000)
    ap.add_argument("--out", default=os.path.join("profiles", "projection.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "projection_time needs a GPU: a time taken elsewhere says nothing"
    rows = []
    if "a" in a.case:
        rows += case_a(a.reps, a.window)
    if "b" in a.case:
        rows += case_b(a.reps, a.window, a.edges, a.flows, a.max_iter)
    with open(a.out, "w") as f:
        f.write("# python tools/projection_time.py --case %s --reps %d --window %g --edges %d --flows %d --max-iter %d  (%s)\n"
                % (a.case, a.reps, a.window, a.edges, a.flows, a.max_iter, torch.cuda.get_device_name(0)))
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
