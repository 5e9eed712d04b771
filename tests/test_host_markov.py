"""The Markov baseline without a GPU: this file's NumPy restatement of the four scn_markov_* kernels (include/scone_hip.h), checked
against tests/golden/cfg1_markov.npz -- the outputs of the reference's own Markov_Model (tests/golden/make_golden_markov.py) --
plus the reference's quirks, the argument checks that need no device and the -markov_order switch.  tests/test_gpu_markov.py imports
the restatement."""
import ctypes
import os

import numpy as np
import pytest

from tests.test_host_sample import M32, philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
INT32_MAX = (1 << 31) - 1
MAX_ORDER = 4
ORDERS = (1, 2, 3)


# ------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------

def u24(seed, r, s, h):
    """The 24-bit integers behind scn_sample_uniform(seed, r, s, h) for the rows r = 0 .. n-1 (a list of Python ints)."""
    r = np.arange(r, dtype=np.int64)
    ctr = np.stack([r & M32, np.full_like(r, s & M32), np.full_like(r, h & M32), np.zeros_like(r)], axis=-1).astype(np.uint64)
    key = np.broadcast_to(np.array([int(seed) & M32, (int(seed) >> 32) & M32], np.uint64), r.shape + (2,))
    return [int(x) >> 8 for x in philox4x32_10(ctr, key)[..., 0]] if len(r) else []


def table_from_edges(n_nodes, edges):
    """(nbr (V, D) int32, deg (V,) int32): neighbours ascending, left-aligned, -1 behind them."""
    rows = [set() for _ in range(n_nodes)]
    for a, b in np.asarray(edges).tolist():
        rows[a].add(b)
        rows[b].add(a)
    D = max(1, max(len(r) for r in rows))
    nbr = np.full((n_nodes, D), -1, np.int32)
    for v, r in enumerate(rows):
        nbr[v, :len(r)] = sorted(r)
    return nbr, (nbr >= 0).sum(axis=1).astype(np.int32)


def ragged(lists):
    ptr = np.cumsum([0] + [len(p) for p in lists]).astype(np.int32)
    return ptr, np.asarray([v for p in lists for v in p], np.int32).reshape(-1)


def table_rows(n_nodes, d, order):
    """Rows of the table, or None where the library answers SCN_ERR_UNSUPPORTED."""
    if not 1 <= order <= MAX_ORDER:
        return None
    rows = n_nodes * d ** (order - 1)
    return rows if rows * d < INT32_MAX else None


def slot(nbr, deg, a, b):
    V = len(deg)
    if not (0 <= a < V and 0 <= b < V):
        return -1
    hit = np.flatnonzero(nbr[a, :deg[a]] == b)
    return int(hit[0]) if len(hit) else -1


def ref_count(ptr, nodes, order, nbr, deg, counts=None):
    """scn_markov_count: (counts, err); accumulates into counts when given."""
    V, D = nbr.shape
    if counts is None:
        counts = np.zeros((table_rows(V, D, order), D), np.int32)
    err = INT32_MAX
    for p in range(len(ptr) - 1):
        t0, L = int(ptr[p]), int(ptr[p + 1] - ptr[p])
        if L <= order:
            continue
        sl = [slot(nbr, deg, int(nodes[t0 + q]), int(nodes[t0 + q + 1])) for q in range(L - 1)]
        for q, s in enumerate(sl):
            if s < 0:
                err = min(err, t0 + q)
        for i in range(L - order):
            w = sl[i:i + order]
            if min(w) < 0:
                continue
            s = int(nodes[t0 + i])
            for x in w[:-1]:
                s = s * D + x
            counts[s, w[-1]] += 1
    return counts, err


def window(ptr, nodes, i, order, nbr, deg):
    """The last `order` nodes of prefix i: (w, slots, err) -- w None for a short prefix or an offending pair (then err < INT32_MAX)."""
    t0, L = int(ptr[i]), int(ptr[i + 1] - ptr[i])
    if L < order:
        return None, None, INT32_MAX
    base = t0 + L - order
    w = [int(v) for v in nodes[base:base + order]]
    if order == 1 and not 0 <= w[0] < len(deg):
        return None, None, base
    sl = []
    for k in range(order - 1):
        s = slot(nbr, deg, w[k], w[k + 1])
        if s < 0:
            return None, None, base + k
        sl.append(s)
    return w, sl, INT32_MAX


def state(w, sl, D):
    s = w[0]
    for x in sl:
        s = s * D + x
    return s


def ref_rollout(ptr, nodes, order, hops, seed, nbr, deg, counts):
    """scn_markov_rollout: (pred [n][hops], n_tied [n][hops], err)."""
    n, D = len(ptr) - 1, nbr.shape[1]
    pred = np.full((n, hops), -1, np.int32)
    tied = np.zeros((n, hops), np.int32)
    err = INT32_MAX
    U = [u24(seed, n, 0, h) for h in range(hops)]
    for i in range(n):
        w, sl, e = window(ptr, nodes, i, order, nbr, deg)
        err = min(err, e)
        if w is None:
            continue
        for h in range(hops):
            v = w[-1]
            dv = int(deg[v])
            if dv == 0:
                break
            row = counts[state(w, sl, D), :dv]
            maxima = np.flatnonzero(row == row.max())
            m = len(maxima)
            j = int(maxima[(U[h][i] * m) >> 24])
            pred[i, h], tied[i, h] = nbr[v, j], m
            w, sl = (w + [int(nbr[v, j])])[1:], (sl + [j])[1:] if order > 1 else []
    return pred, tied, err


def ref_two_target(ptr, nodes, order, seed, target, nbr, deg, counts):
    """scn_markov_two_target: (score, other, err, err_target)."""
    n, D = len(ptr) - 1, nbr.shape[1]
    score, other = np.zeros(n, np.float32), np.full(n, -1, np.int32)
    err = err_t = INT32_MAX
    U = u24(seed, n, 1, 0)
    for i in range(n):
        w, sl, e = window(ptr, nodes, i, order, nbr, deg)
        err = min(err, e)
        if w is None:
            continue
        v = w[-1]
        t = slot(nbr, deg, v, int(target[i]))
        if t < 0:
            err_t = min(err_t, i)
        elif deg[v] > 1:
            o = (U[i] * (int(deg[v]) - 1)) >> 24
            j = o + (o >= t)
            row = counts[state(w, sl, D)]
            score[i] = 0.5 if row[t] == row[j] else (1.0 if row[t] > row[j] else 0.0)
            other[i] = nbr[v, j]
    return score, other, err, err_t


def ref_probs(ptr, nodes, order, nbr, deg, counts):
    """scn_markov_probs: (probs [n][D] float64, err) -- Python's own division of the two integers."""
    n, D = len(ptr) - 1, nbr.shape[1]
    probs = np.zeros((n, D), np.float64)
    err = INT32_MAX
    for i in range(n):
        w, sl, e = window(ptr, nodes, i, order, nbr, deg)
        err = min(err, e)
        if w is None:
            continue
        dv = int(deg[w[-1]])
        row = [int(c) for c in counts[state(w, sl, D), :dv]]
        total = sum(row)
        if total > 0:
            probs[i, :dv] = [c / total for c in row]
    return probs, err


def ref_test(pred, ptr, nodes, order, target):
    """Markov_Model.test from a rollout: the last hop's node, a short prefix's own last node (MM:85, 92)."""
    last = pred[:, -1].astype(np.int64)
    for i in np.flatnonzero(np.diff(ptr) < order):
        last[i] = nodes[ptr[i + 1] - 1]
    return np.average(np.asarray(target, np.int64) == last)


# ------------------------------------------------------------------------------------------------------------------
# cfg1 and the reference's outputs on it
# ------------------------------------------------------------------------------------------------------------------

def load_cfg1():
    """The graph, the 1000 walks cut as the data set cut them, and the fixture."""
    c = np.load(os.path.join(GOLDEN, "cfg1_complex.npz"))
    p = np.load(os.path.join(GOLDEN, "cfg1_paths.npz"))
    nbr, deg = table_from_edges(int(c["n_nodes"]), c["edges"])
    ptr, nodes = p["path_ptr"], p["path_nodes"]
    cut = np.diff(p["flow1_ptr"]) + 1
    prefixes = [nodes[ptr[i]:ptr[i] + cut[i]].tolist() for i in range(len(cut))]
    paths = [nodes[ptr[i]:ptr[i] + cut[i] + 2].tolist() for i in range(len(cut))]
    return {"nbr": nbr, "deg": deg, "prefixes": prefixes, "paths": paths, "train": p["train_mask"] == 1, "test": p["test_mask"] == 1,
            "t1": p["tnode1"].astype(np.int64), "t2": p["tnode2"].astype(np.int64), "last1": p["last1"],
            "fix": dict(np.load(os.path.join(GOLDEN, "cfg1_markov.npz")))}          # read once: an NpzFile reads an array on every access


_CFG1 = {}


def cfg1_markov():
    if not _CFG1:
        _CFG1.update(load_cfg1())
        _CFG1["counts"] = {}
    return _CFG1


def cfg1_counts(order):
    d = cfg1_markov()
    if order not in d["counts"]:
        ptr, nodes = ragged([d["paths"][i] for i in np.flatnonzero(d["train"])])
        counts, err = ref_count(ptr, nodes, order, d["nbr"], d["deg"])
        assert err == INT32_MAX
        counts.setflags(write=False)
        d["counts"][order] = counts
    return d["counts"][order]


def rag_row(fix, name, k, i, field):
    ptr = fix["%s%d_ptr" % (name, k)]
    return fix["%s%d_%s" % (name, k, field)][ptr[i]:ptr[i + 1]]


def test_the_cut_reproduces_the_data_set():
    d = cfg1_markov()
    assert d["nbr"].shape == (400, 13) and len(d["paths"]) == 1000 and d["train"].sum() == 800 and d["test"].sum() == 200
    for i, p in enumerate(d["paths"]):
        assert p[-3] == d["last1"][i] and p[-2] == d["t1"][i] and p[-1] == d["t2"][i]
    assert [table_rows(400, 13, k) for k in (1, 2, 3)] == [400, 5200, 67600]


@pytest.mark.parametrize("order", ORDERS)
def test_counts_reproduce_every_reference_weight_bitwise(order):
    d = cfg1_markov()
    fix, counts, nbr, deg = d["fix"], cfg1_counts(order), d["nbr"], d["deg"]
    D = nbr.shape[1]
    states, nbrs, probs = fix["w%d_state" % order], fix["w%d_nbr" % order], fix["w%d_prob" % order]
    assert len(probs) == int((counts != 0).sum()) > 600          # every non-zero weight, and no count the reference does not have
    for st, u, pr in zip(states.tolist(), nbrs.tolist(), probs.tolist()):
        sl = [slot(nbr, deg, a, b) for a, b in zip(st[:-1], st[1:])]
        assert min(sl + [0]) >= 0
        row = counts[state(st, sl, D)]
        j = slot(nbr, deg, st[-1], u)
        assert j >= 0 and int(row[j]) / int(row.sum()) == pr     # float64, bit for bit (== on two finite doubles)
    # the same through the probs restatement, padding and unseen states included
    ptr, nodes = ragged(states.tolist())
    got, err = ref_probs(ptr, nodes, order, nbr, deg, counts)
    assert err == INT32_MAX
    for i, (st, u, pr) in enumerate(zip(states.tolist(), nbrs.tolist(), probs.tolist())):
        assert got[i, slot(nbr, deg, st[-1], u)] == pr and got[i, deg[st[-1]]:].sum() == 0


@pytest.mark.parametrize("order", ORDERS)
def test_every_prediction_lies_in_the_reference_tied_set(order):
    d = cfg1_markov()
    fix, counts = d["fix"], cfg1_counts(order)
    ptr, nodes = ragged(d["prefixes"])
    exact = 0
    for seed in (0, 20261019):
        pred, tied, err = ref_rollout(ptr, nodes, order, 2, seed, d["nbr"], d["deg"], counts)
        assert err == INT32_MAX and pred.shape == (1000, 2)
        for i in range(1000):                                    # no row is left out: a tie-free row is an exact match
            first = rag_row(fix, "tie", order, i, "nodes")
            assert pred[i, 0] in first and tied[i, 0] == len(first)
            assert pred[i, 1] in rag_row(fix, "end", order, i, "nodes")
            if not fix["branch_tie%d" % order][i]:
                assert len(first) == 1 and tied[i, 1] == 1 and len(rag_row(fix, "end", order, i, "nodes")) == 1
                exact += 1
    assert exact == 2 * (1000 - int(fix["branch_tie%d" % order].sum()))


@pytest.mark.parametrize("order", ORDERS)
def test_tie_share_of_the_test_rows(order):
    """Rows with a tie somewhere on a 2-hop branch are at most 20 % of the 200 test rows: at least 80 % of the test rows are
    exact matches of the reference whatever it draws."""
    d = cfg1_markov()
    share = d["fix"]["branch_tie%d" % order][d["test"]]
    assert len(share) == 200 and share.sum() <= 0.2 * 200


@pytest.mark.parametrize("order", ORDERS)
def test_two_target_outcome_is_the_reference_outcome_for_the_drawn_neighbour(order):
    d = cfg1_markov()
    fix, counts = d["fix"], cfg1_counts(order)
    ptr, nodes = ragged(d["prefixes"])
    seen = set()
    for seed in (0, 7):
        score, other, err, err_t = ref_two_target(ptr, nodes, order, seed, d["t1"], d["nbr"], d["deg"], counts)
        assert err == err_t == INT32_MAX
        for i in range(1000):
            others = rag_row(fix, "tt", order, i, "other").tolist()
            assert other[i] in others and other[i] != d["t1"][i]
            assert score[i] == rag_row(fix, "tt", order, i, "score")[others.index(other[i])]
            seen.add((i, int(other[i])))
    assert len(seen) > 1000                                      # more pairs than one seed can give: the draw moves with the seed


# ------------------------------------------------------------------------------------------------------------------
# the reference's quirks on the 4-node graph: 0-1, 0-2, 0-3, 1-2, 2-3
# ------------------------------------------------------------------------------------------------------------------

def tiny4():
    t = np.load(os.path.join(GOLDEN, "tiny4_complex.npz"))
    return table_from_edges(4, t["edges"])


TINY_WALKS = [[0, 1, 2, 3, 0], [1, 2, 0, 3], [3, 2, 1, 0, 2], [2, 0], [1]]


def test_tiny4_counts_by_hand():
    nbr, deg = tiny4()
    assert nbr.tolist() == [[1, 2, 3], [0, 2, -1], [0, 1, 3], [0, 2, -1]] and deg.tolist() == [3, 2, 3, 2]
    ptr, nodes = ragged(TINY_WALKS)
    c1, err = ref_count(ptr, nodes, 1, nbr, deg)
    assert err == INT32_MAX
    # transitions: 0>1 1>2 2>3 3>0 | 1>2 2>0 0>3 | 3>2 2>1 1>0 0>2 | 2>0
    assert c1.tolist() == [[1, 1, 1], [1, 2, 0], [2, 1, 1], [1, 1, 0]]
    c2, _ = ref_count(ptr, nodes, 2, nbr, deg)
    assert c2.shape == (12, 3) and c2.sum() == 3 + 2 + 3               # a walk of len <= order counts nothing
    assert c2[state([0, 1], [0], 3), 1] == 1 and c2[state([2, 0], [0], 3), 2] == 1     # (0,1)>2 and (2,0)>3


def test_short_prefix_predicts_nothing_and_compares_its_own_last_node():
    nbr, deg = tiny4()
    ptr, nodes = ragged(TINY_WALKS)
    c2, _ = ref_count(ptr, nodes, 2, nbr, deg)
    pptr, pnodes = ragged([[1], [0, 1], []])
    pred, tied, err = ref_rollout(pptr, pnodes, 2, 3, 0, nbr, deg, c2)
    assert err == INT32_MAX and pred[0].tolist() == [-1] * 3 and tied[0].tolist() == [0] * 3 and pred[2].tolist() == [-1] * 3
    assert pred[1, 0] == 2 and tied[1, 0] == 1                   # (0, 1) was followed by 2 once and by 0 never
    assert ref_test(pred[:2], pptr[:3], pnodes, 2, [1, int(pred[1, 2])]) == 1.0      # MM:92: the short prefix's own last node
    probs, _ = ref_probs(pptr, pnodes, 2, nbr, deg, c2)
    assert probs[0].tolist() == [0, 0, 0] and probs[1].tolist() == [0, 1, 0]


def test_unseen_state_ties_all_neighbours():
    nbr, deg = tiny4()
    ptr, nodes = ragged(TINY_WALKS)
    c2, _ = ref_count(ptr, nodes, 2, nbr, deg)
    pptr, pnodes = ragged([[3, 0]] * 64)                         # (3, 0) ends a walk and starts none
    assert c2[state([3, 0], [0], 3)].sum() == 0
    pred, tied, _ = ref_rollout(pptr, pnodes, 2, 1, 5, nbr, deg, c2)
    assert (tied == 3).all() and set(pred[:, 0].tolist()) == {1, 2, 3}
    probs, _ = ref_probs(pptr, pnodes, 2, nbr, deg, c2)
    assert not probs.any()


def test_degree_one_node_and_foreign_target_in_two_target():
    nbr, deg = table_from_edges(3, [(0, 1), (1, 2)])             # a path graph: node 0 has one neighbour
    ptr, nodes = ragged([[0, 1, 2, 1, 0]])
    c1, _ = ref_count(ptr, nodes, 1, nbr, deg)
    pptr, pnodes = ragged([[1, 0], [0, 1], [0, 1]])
    score, other, err, err_t = ref_two_target(pptr, pnodes, 1, 0, [1, 2, 1], nbr, deg, c1)
    assert err == INT32_MAX and score[0] == 0 and other[0] == -1          # np.random.choice([]) raises in the reference
    assert other[1] == 0 and score[1] == 0.5                              # 1>2 once, 1>0 once
    assert err_t == 2 and other[2] == -1                                  # 1 is no neighbour of 1


def test_offending_pairs_lower_err_and_count_nothing():
    nbr, deg = tiny4()
    walks = [[0, 1, 2], [0, 1, 3, 2, 0, 1], [2, 0, 7, 0, 1]]                # (1, 3) is no edge; 7 is no node
    ptr, nodes = ragged(walks)
    for order in (1, 2, 3):
        c, err = ref_count(ptr, nodes, order, nbr, deg)
        assert err == 3 + 1                                      # walk 1, position 1
        clean, e2 = ref_count(*ragged([[0, 1, 2], [0, 1], [3, 2, 0, 1], [2, 0], [0, 1]]), order, nbr, deg)
        assert e2 == INT32_MAX and np.array_equal(c, clean)      # what is left are the windows beside the offending pairs
    c, err = ref_count(*ragged(walks[2:]), 1, nbr, deg)
    assert err == 1
    pptr, pnodes = ragged([[0, 1, 2], [2, 0, 7], [1, 3]])
    c2, _ = ref_count(ptr, nodes, 2, nbr, deg)
    pred, tied, err = ref_rollout(pptr, pnodes, 2, 2, 0, nbr, deg, c2)
    assert err == 4 and pred[1].tolist() == [-1, -1] and pred[0, 0] >= 0
    assert ref_rollout(pptr, pnodes, 1, 1, 0, nbr, deg, c)[2] == 5          # order 1: the position of the foreign last node
    assert ref_rollout(pptr[1:] - 3, pnodes[3:], 2, 1, 0, nbr, deg, c2)[2] == 1


def test_rollout_does_not_depend_on_the_rest_of_the_batch_but_on_row_and_seed():
    d = cfg1_markov()
    counts = cfg1_counts(1)
    rows = [i for i in range(1000) if d["fix"]["tie1_ptr"][i + 1] - d["fix"]["tie1_ptr"][i] > 1][:8]
    assert len(rows) == 8
    pre = [d["prefixes"][i] for i in rows]
    a = ref_rollout(*ragged(pre), 1, 2, 3, d["nbr"], d["deg"], counts)[0]
    b = ref_rollout(*ragged(pre[:3] + [[0, 1]] * 5), 1, 2, 3, d["nbr"], d["deg"], counts)[0]
    assert np.array_equal(a[:3], b[:3])
    draws = {tuple(ref_rollout(*ragged(pre), 1, 1, s, d["nbr"], d["deg"], counts)[0][:, 0]) for s in range(8)}
    assert len(draws) > 1


# ------------------------------------------------------------------------------------------------------------------
# argument checks that never reach the device, and the driver's switch
# ------------------------------------------------------------------------------------------------------------------

def test_table_rows_and_limits():
    from scone_gcn_amd import _lib
    lib = _lib.load()
    assert _lib.SCN_MARKOV_MAX_ORDER == MAX_ORDER
    src = open(os.path.join(ROOT, "include", "scone_hip.h")).read()
    assert "#define SCN_MARKOV_MAX_ORDER 4" in src
    for V, D, k in [(400, 13, 1), (400, 13, 2), (400, 13, 3), (400, 13, 4), (71, 70, 2), (4, 3, 4), (1, 1, 4), (46340, 46340, 1),
                    (46341, 46341, 2), (2 ** 31 - 2, 1, 1), (2 ** 31 - 1, 1, 1), (1290, 1290, 3), (1291, 1291, 3), (1000000, 13, 2),
                    (1000000, 13, 3), (400, 13, 0), (400, 13, 5), (400, 13, -1)]:
        want = table_rows(V, D, k)
        assert lib.scn_markov_table_rows(V, D, k) == (_lib.SCN_ERR_UNSUPPORTED if want is None else want), (V, D, k)
    assert lib.scn_markov_table_rows(0, 3, 1) == -2 and lib.scn_markov_table_rows(3, 0, 1) == -2


def test_unsupported_and_empty_calls_return_before_any_launch():
    """Order 5, a table past 2^31 - 1 entries and n = 0 answer from the host: NULL arrays are never touched."""
    from scone_gcn_amd import _lib
    lib = _lib.load()
    U, seed = _lib.SCN_ERR_UNSUPPORTED, ctypes.c_uint64(0)
    for order, V, D in [(5, 400, 13), (0, 400, 13), (3, 1291, 1291), (4, 400, 200)]:
        assert lib.scn_markov_count(3, None, None, order, V, D, None, None, None, None, None) == U
        assert lib.scn_markov_rollout(3, None, None, order, 2, seed, V, D, None, None, None, None, None, None, None) == U
        assert lib.scn_markov_two_target(3, None, None, order, seed, None, V, D, None, None, None, None, None, None, None, None) == U
        assert lib.scn_markov_probs(3, None, None, order, V, D, None, None, None, None, None, None) == U
    assert lib.scn_markov_count(0, None, None, 2, 400, 13, None, None, None, None, None) == 0
    assert lib.scn_markov_rollout(0, None, None, 2, 2, seed, 400, 13, None, None, None, None, None, None, None) == 0
    assert lib.scn_markov_two_target(0, None, None, 2, seed, None, 400, 13, None, None, None, None, None, None, None, None) == 0
    assert lib.scn_markov_probs(0, None, None, 2, 400, 13, None, None, None, None, None, None) == 0
    assert lib.scn_markov_count(3, None, None, 2, 400, 13, None, None, None, None, None) == _lib.SCN_ERR_BAD_ARG
    assert lib.scn_markov_count(-1, None, None, 2, 400, 13, None, None, None, None, None) == -2
    assert lib.scn_markov_rollout(3, None, None, 2, 0, seed, 400, 13, None, None, None, None, None, None, None) == -2


def test_python_class_refuses_orders_and_tables_before_touching_a_device():
    from scone_gcn_amd.markov_model import Markov_Model, neighbour_table, ragged as py_ragged
    for order in (0, 5, 1.5):
        with pytest.raises(ValueError, match="order"):
            Markov_Model(order)
    wide = np.full((300, 300), -1, np.int64)
    wide[:, 0] = (np.arange(300) + 1) % 300
    with pytest.raises(ValueError, match="2\\^31"):
        Markov_Model(4).train(wide, [[0, 1, 2]])                 # 300^4 entries
    with pytest.raises(RuntimeError, match="train"):
        Markov_Model(1).predict_paths([[0, 1]], 1)
    # the three graph forms give one table; padding anywhere, neighbours in any order
    nbr, deg = tiny4()
    import networkx as nx
    G = nx.Graph()
    G.add_edges_from([(2, 3), (0, 3), (0, 1), (1, 2), (0, 2)])
    scrambled = np.array([[3, -1, 1, 2], [-1, 2, 0, -1], [3, 1, -1, 0], [-1, -1, 2, 0]])
    for form in (G, nbr, scrambled[:, :]):
        got_nbr, got_deg = neighbour_table(form)
        assert np.array_equal(got_nbr[:, :3], nbr) and np.array_equal(got_deg, deg) and (got_nbr[:, 3:] == -1).all()
    ptr, nodes = py_ragged(TINY_WALKS)
    assert np.array_equal(ptr, ragged(TINY_WALKS)[0]) and np.array_equal(nodes, ragged(TINY_WALKS)[1])
    assert all(np.array_equal(a, b) for a, b in zip(py_ragged((ptr, nodes)), (ptr, nodes)))
    with pytest.raises(ValueError, match="ptr"):
        py_ragged((np.array([0, 3]), np.array([1, 2])))


def test_hyperparams_parse_markov_order():
    from scone_gcn_amd import trajectory_experiments as te
    hp = te.hyperparams(["prog"])
    assert hp["markov"] == 0 and hp["markov_order"] == 1         # the reference's hard-coded order (TE:329)
    hp = te.hyperparams(["prog", "-markov", "1", "-markov_order", "3"])
    assert hp["markov"] == 1 and int(hp["markov_order"]) == 3
