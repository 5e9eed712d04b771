#!/usr/bin/env python3
"""Generate tests/golden/cfg1_projection.npz from the reference's own projection model.

Run only where a checkout of the reference project is at hand (no test needs it: the tests read the committed .npz), with the
directory that holds its trajectory_analysis/ as the argument, from a scratch working directory:

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_projection.py REFERENCE_DIR

What is executed of the reference (read-only, unmodified): the definitions of trajectory_analysis/projection_model.py (PM) above
its module-level data-set load (PM:200 on, which cannot run here: load_dataset reads a gpickle), i.e. build_flow, embed,
neighborhood, project_flows, loss, accuracy, accuracy_2target and eval_dataset -- the text up to the line that assigns `folder`
is compiled and executed at generation time; none of it is kept.  Its import of synthetic_data_gen needs the two aliases
SURVEY.md section 8(c) records (nx.OrderedDiGraph, np.float).

Inputs: the complex of cfg1_complex.npz (B1, B2 dense, as the reference holds them) and the 1-hop flows, last nodes and targets
of cfg1_paths.npz, forward and reversed.  Nothing random of the reference is run: the draw of accuracy_2target (np.random.choice,
PM:119) is replaced, for the duration of one call on one row, by each possible other neighbour in turn.

Output (all 1000 rows unless stated):
  dim                         : columns of the reference's null-space basis (2)
  proj8 (8, E)                : V V^T f of the first 8 walks (PM:84)
  prob_rows                   : the rows probs_fwd / probs_rev hold (all rows while the file stays below 256 KB, else the test
                                and transfer rows)
  probs_fwd, probs_rev (., D) : project_flows' probabilities of the forward and the reversed 1-hop flows (PM:80-96), transposed
  argmax_fwd, argmax_rev      : np.argmax of every row's probabilities over all D slots (PM:108)
  test / rev_test / transfer  : (loss, accuracy) of eval_dataset on the test rows, the reversed test rows and the rows i % 3 == 2
  all_fwd                     : (loss, accuracy) over all 1000 forward rows
  tt_ptr, tt_other, tt_score  : per row, for every other slot of the last node ascending, what accuracy_2target adds (1, 0.5, 0)
"""
import os
import sys

import numpy as np
import networkx as nx

if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "trajectory_analysis", "projection_model.py")):
    sys.exit("usage: make_golden_projection.py REFERENCE_DIR   (the directory that holds trajectory_analysis/projection_model.py)")
OUT = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(sys.argv[1], "trajectory_analysis")
LIMIT = 256 * 1024

if not hasattr(nx, "OrderedDiGraph"):
    nx.OrderedDiGraph = nx.DiGraph
if not hasattr(np, "float"):
    np.float = float
sys.path.insert(0, REF)
sys.dont_write_bytecode = True


def reference_definitions():
    """The names PM defines before it loads a data set."""
    lines = open(os.path.join(REF, "projection_model.py")).read().split("\n")
    stop = next(i for i, l in enumerate(lines) if l.startswith("folder = "))
    ns = {"__name__": "projection_model_definitions"}
    exec(compile("\n".join(lines[:stop]), "projection_model.py", "exec"), ns)
    return ns


def dense(z, name):
    M = np.zeros(tuple(z[name + "_shape"]))
    M[z[name + "_row"], z[name + "_col"]] = z[name + "_val"]
    return M


def flows_dense(p, name, E):
    ptr, idx, val = p[name + "_ptr"], p[name + "_idx"], p[name + "_val"]
    X = np.zeros((len(ptr) - 1, E))
    X[np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)), idx] = val
    return X


def main():
    pm = reference_definitions()
    c = np.load(os.path.join(OUT, "cfg1_complex.npz"))
    p = np.load(os.path.join(OUT, "cfg1_paths.npz"))
    B1, B2 = dense(c, "B1"), dense(c, "B2")
    E, D, N = B1.shape[1], int(p["max_degree"]), len(p["last1"])
    G = nx.Graph()
    G.add_nodes_from(range(int(c["n_nodes"])))
    G.add_edges_from((int(a), int(b)) for a, b in c["edges"])
    assert max(len(G[v]) for v in G.nodes) == D

    def onehot(t):
        y = np.zeros((len(t), D))
        y[np.arange(len(t)), t] = 1.0
        return y

    sets = {"fwd": (flows_dense(p, "flow1", E), p["last1"].astype(int), onehot(p["targets1"])),
            "rev": (flows_dense(p, "rev_flow1", E), p["rev_last1"].astype(int), onehot(p["rev_targets1"]))}
    V, _ = pm["embed"](B1, B2)
    out = {"dim": np.int32(V.shape[1]), "proj8": (V @ V.T @ sets["fwd"][0][:8].T).T}
    probs = {}
    for k, (X, last, y) in sets.items():
        nb = [pm["neighborhood"](G, n) for n in last]
        probs[k] = pm["project_flows"](V, B1, X.T, last, nb, D).T              # (N, D)
        out["argmax_" + k] = np.argmax(probs[k], axis=1).astype(np.int8)
    test, transfer = p["test_mask"] == 1, np.arange(N) % 3 == 2

    def ev(k, rows):
        X, last, y = sets[k]
        ce, acc = pm["eval_dataset"](G, None, last[rows], y[rows].T, None, None, None, B1, B2, D, flows=X[rows].T)
        # eval_dataset embeds again; what it returns must be what the stored probabilities give
        assert ce == pm["loss"](y[rows].T, probs[k][rows].T) and acc == pm["accuracy"](y[rows].T, probs[k][rows].T)
        return np.asarray([ce, acc], np.float64)

    out["test"], out["rev_test"], out["transfer"] = ev("fwd", test), ev("rev", test), ev("fwd", transfer)
    out["all_fwd"] = ev("fwd", np.ones(N, bool))
    # 2-target: every possible other neighbour in place of the reference's draw
    X, last, y = sets["fwd"]
    n_nbrs = np.asarray([len(G[n]) for n in last])
    ptr, others, scores = [0], [], []
    draw = np.random.choice
    try:
        for i in range(N):
            for o in range(n_nbrs[i]):
                if o == p["targets1"][i]:
                    continue

                def pick(choices, o=o):
                    assert o in choices and p["targets1"][i] not in choices
                    return o
                np.random.choice = pick
                others.append(o)
                scores.append(pm["accuracy_2target"](y[i:i + 1].T, probs["fwd"][i:i + 1].T, n_nbrs[i:i + 1]))
            ptr.append(len(others))
    finally:
        np.random.choice = draw
    out["tt_ptr"], out["tt_other"] = np.asarray(ptr, np.int32), np.asarray(others, np.int8)
    out["tt_score"] = np.asarray(scores, np.float64)
    path = os.path.join(OUT, "cfg1_projection.npz")
    for rows in (np.arange(N), np.flatnonzero(test | transfer)):
        out["prob_rows"] = rows.astype(np.int32)
        out["probs_fwd"], out["probs_rev"] = probs["fwd"][rows], probs["rev"][rows]
        np.savez_compressed(path, **out)
        if os.path.getsize(path) < LIMIT:
            break
    srt = np.sort(np.log(probs["fwd"]), axis=1)
    print("dim", V.shape[1], "rows kept", len(out["prob_rows"]), "bytes", os.path.getsize(path), "test", out["test"], "rev_test",
          out["rev_test"], "transfer", out["transfer"], "all", out["all_fwd"], "smallest top-two logit gap",
          float((srt[:, -1] - srt[:, -2]).min()))
    assert os.path.getsize(path) < LIMIT


if __name__ == "__main__":
    main()
