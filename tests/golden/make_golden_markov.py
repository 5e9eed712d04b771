#!/usr/bin/env python3
"""Generate tests/golden/cfg1_markov.npz from the reference's own Markov model.

Run only where a checkout of the reference project is at hand (no test needs it: the tests read the committed .npz), with the
directory that holds its trajectory_analysis/ as the argument:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_markov.py REFERENCE_DIR

What is imported from the reference (read-only, unmodified): trajectory_analysis/markov_model.py, Markov_Model (MM:9-112).  It needs
NumPy and networkx only, so -- unlike the model's forward values -- its outputs can be pinned.

Inputs: the graph of cfg1_complex.npz and the 1000 walks of cfg1_paths.npz, each cut where the data set cut it: prefix = the
first (entries of the row's flow1) + 1 nodes, then the two target nodes (checked against last1 / tnode1 / tnode2 below).  The
reference model is trained on the 800 training rows (MM:38-56) for orders 1, 2 and 3.  Nothing random of the reference is run:
its choices among ties are recorded as SETS.

Output, per order k (all rows = all 1000 walks, train and test):
  w{k}_state (n, k), w{k}_nbr (n,), w{k}_prob (n,) : every non-zero entry of Markov_Model.weights
  tie{k}_ptr / tie{k}_nodes   : per row, the tied maxima of predict() at hop 1 (MM:62-72: the best and the `others`), ascending
  end{k}_ptr / end{k}_nodes   : per row, the end nodes test(hops=2) can reach through any chain of tied choices, ascending
  branch_tie{k}               : per row, 1 when a tie occurs somewhere on such a 2-hop branch
  tt{k}_ptr / tt{k}_other / tt{k}_score : per row, for every possible "other" neighbour of test_2_target (MM:102-111), ascending,
                                          what the row adds to `correct` (1, 0.5 or 0) with the 1-hop target
"""
import os
import sys

import numpy as np
import networkx as nx

if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "trajectory_analysis", "markov_model.py")):
    sys.exit("usage: make_golden_markov.py REFERENCE_DIR   (the directory that holds trajectory_analysis/markov_model.py)")
OUT = os.path.dirname(os.path.abspath(__file__))

sys.path.insert(0, os.path.join(sys.argv[1], "trajectory_analysis"))
sys.dont_write_bytecode = True
from markov_model import Markov_Model       # noqa: E402


def tied_maxima(dist):
    """The nodes predict() chooses among (MM:62-72): every neighbour whose probability equals the maximum."""
    best = max(dist.values())
    assert best > -1
    return sorted(int(n) for n, p in dist.items() if p == best)


def rag(lists, dtype=np.int32):
    ptr = np.cumsum([0] + [len(l) for l in lists]).astype(np.int32)
    flat = np.asarray([x for l in lists for x in l], dtype)
    return ptr, flat


def main():
    c = np.load(os.path.join(OUT, "cfg1_complex.npz"))
    p = np.load(os.path.join(OUT, "cfg1_paths.npz"))
    G = nx.Graph()
    G.add_nodes_from(range(int(c["n_nodes"])))
    G.add_edges_from((int(a), int(b)) for a, b in c["edges"])
    ptr, nodes = p["path_ptr"], p["path_nodes"]
    n_flow = np.diff(p["flow1_ptr"])
    paths, prefixes = [], []
    for i in range(len(ptr) - 1):
        walk = [int(v) for v in nodes[ptr[i]:ptr[i + 1]]]
        cut = int(n_flow[i]) + 1
        assert len(walk) >= cut + 2
        assert walk[cut - 1] == p["last1"][i] and walk[cut] == p["tnode1"][i] and walk[cut + 1] == p["tnode2"][i]
        prefixes.append(walk[:cut])
        paths.append(walk[:cut + 2])
    train = p["train_mask"] == 1
    t1 = p["tnode1"]
    out = {}
    for k in (1, 2, 3):
        mm = Markov_Model(k)
        mm.train(G, [paths[i] for i in np.flatnonzero(train)])
        st, nb, pr = [], [], []
        for state in sorted(mm.weights):
            for n in sorted(mm.weights[state]):
                if mm.weights[state][n] != 0:
                    st.append(state)
                    nb.append(n)
                    pr.append(mm.weights[state][n])
        out["w%d_state" % k] = np.asarray(st, np.int32).reshape(len(st), k)
        out["w%d_nbr" % k] = np.asarray(nb, np.int32)
        out["w%d_prob" % k] = np.asarray(pr, np.float64)
        ties, ends, branch, tt_other, tt_score = [], [], [], [], []
        for i, pre in enumerate(prefixes):
            first = tied_maxima(mm.weights[tuple(pre[-k:])])
            ties.append(first)
            end, tie = set(), len(first) > 1
            for u in first:
                second = tied_maxima(mm.weights[tuple((pre + [u])[-k:])])
                tie = tie or len(second) > 1
                end.update(second)
            ends.append(sorted(end))
            branch.append(int(tie))
            dist = mm.weights[tuple(pre[-k:])]
            others = sorted(int(n) for n in dist if n != t1[i])
            assert len(others) == len(dist) - 1
            tt_other.append(others)
            tt_score.append([0.5 if dist[int(t1[i])] == dist[o] else (1.0 if dist[int(t1[i])] > dist[o] else 0.0) for o in others])
        out["tie%d_ptr" % k], out["tie%d_nodes" % k] = rag(ties)
        out["end%d_ptr" % k], out["end%d_nodes" % k] = rag(ends)
        out["branch_tie%d" % k] = np.asarray(branch, np.int8)
        out["tt%d_ptr" % k], out["tt%d_other" % k] = rag(tt_other)
        out["tt%d_score" % k] = rag(tt_score, np.float64)[1]
        print("order", k, "weights", len(pr), "test rows with a tie on a 2-hop branch",
              int(np.asarray(branch)[~train].sum()), "of", int((~train).sum()))
    np.savez_compressed(os.path.join(OUT, "cfg1_markov.npz"), **out)


if __name__ == "__main__":
    main()
