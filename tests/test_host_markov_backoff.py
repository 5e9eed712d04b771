"""The variable-order Markov baseline without a GPU: a dictionary restatement of the scn_markov_hash_* kernels (include/scone_hip.h)
on the helpers of tests/test_host_markov.py.  Without back-off it is that file's restatement (which the reference's own weights pin
bitwise); with it, cfg1's integers and perplexities, the rule by hand on the 4-node graph, the argument checks that need no device
and the driver's two flags.  tests/test_gpu_markov_backoff.py imports the restatement."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests.test_host_baseline_paths import np_markov_path_scores, path_items
from tests.test_host_markov import (INT32_MAX, ORDERS, TINY_WALKS, cfg1_counts, cfg1_markov, ragged, ref_count, ref_probs, ref_rollout,
                                    ref_two_target, slot, state, tiny4, u24)

MAX_ORDER = 8
KEY_SHIFT = 59


# ------------------------------------------------------------------------------------------------------------------
# the restatement: the table is {(order k, state s): [D] counts}
# ------------------------------------------------------------------------------------------------------------------

def key_bound(ptr, K):
    lens = np.diff(ptr).astype(np.int64)
    return [int(np.maximum(lens - k, 0).sum()) for k in range(1, K + 1)]


def ref_backoff_train(ptr, nodes, K, nbr, deg):
    """scn_markov_hash_insert / _number / _count: (table, err)."""
    D = nbr.shape[1]
    table, err = {}, INT32_MAX
    for p in range(len(ptr) - 1):
        t0, L = int(ptr[p]), int(ptr[p + 1] - ptr[p])
        sl = [slot(nbr, deg, int(nodes[t0 + q]), int(nodes[t0 + q + 1])) for q in range(L - 1)]
        for q, s in enumerate(sl):
            if s < 0:
                err = min(err, t0 + q)
        for i in range(L - 1):
            s = int(nodes[t0 + i])
            for k in range(1, K + 1):
                if i + k >= L or sl[i + k - 1] < 0:                  # no node after the window, or an offending pair in or behind it
                    break
                table.setdefault((k, s), np.zeros(D, np.int64))[sl[i + k - 1]] += 1
                s = s * D + sl[i + k - 1]
    return table, err


def n_states(table, K):
    return [sum(1 for k, _ in table if k == o) for o in range(1, K + 1)]


def context(ptr, nodes, i, K, backoff, nbr, deg):
    """The last min(len, K) nodes of prefix i: (w, slots, err) -- w None for an empty prefix, for one shorter than K without back-off
    and for an offending pair (then err < INT32_MAX)."""
    t0, L = int(ptr[i]), int(ptr[i + 1] - ptr[i])
    m = min(L, K)
    if m == 0 or (not backoff and L < K):
        return None, None, INT32_MAX
    base = t0 + L - m
    w = [int(v) for v in nodes[base:base + m]]
    if m == 1 and not 0 <= w[0] < len(deg):
        return None, None, base
    sl = []
    for k in range(m - 1):
        s = slot(nbr, deg, w[k], w[k + 1])
        if s < 0:
            return None, None, base + k
        sl.append(s)
    return w, sl, INT32_MAX


def choose(table, w, sl, K, backoff, min_count, D, dv):
    """(used order, its row) of a context: the longest k <= min(K, len(w)) in the table with a row total >= min_count; (0, zeros)."""
    for k in range(min(len(w), K), (1 if backoff else K) - 1, -1):
        row = table.get((k, state(w[len(w) - k:], sl[len(sl) - (k - 1):], D)))
        if row is not None and int(row[:dv].sum()) >= min_count:
            return k, row
    return 0, np.zeros(D, np.int64)


def ref_backoff_rollout(ptr, nodes, K, backoff, min_count, hops, seed, nbr, deg, table):
    """scn_markov_hash_rollout: (pred, n_tied, used_order [n][hops], err, tied sets {(i, h): nodes} of the hops with a tie)."""
    n, D = len(ptr) - 1, nbr.shape[1]
    pred, tied, used = np.full((n, hops), -1, np.int32), np.zeros((n, hops), np.int32), np.zeros((n, hops), np.int32)
    err, ties = INT32_MAX, {}
    U = [u24(seed, n, 0, h) for h in range(hops)]
    for i in range(n):
        w, sl, e = context(ptr, nodes, i, K, backoff, nbr, deg)
        err = min(err, e)
        if w is None:
            continue
        for h in range(hops):
            v = w[-1]
            dv = int(deg[v])
            if dv == 0:
                break
            k, row = choose(table, w, sl, K, backoff, min_count, D, dv)
            maxima = np.flatnonzero(row[:dv] == row[:dv].max())
            m = len(maxima)
            j = int(maxima[(U[h][i] * m) >> 24])
            pred[i, h], tied[i, h], used[i, h] = nbr[v, j], m, k
            if m > 1:
                ties[(i, h)] = nbr[v, maxima].tolist()
            w, sl = (w + [int(nbr[v, j])])[-K:], (sl + [j])[-(K - 1):] if K > 1 else []
    return pred, tied, used, err, ties


def ref_backoff_two_target(ptr, nodes, K, backoff, min_count, seed, target, nbr, deg, table):
    """scn_markov_hash_two_target: (score, other, used_order, err, err_target)."""
    n, D = len(ptr) - 1, nbr.shape[1]
    score, other, used = np.zeros(n, np.float32), np.full(n, -1, np.int32), np.zeros(n, np.int32)
    err = err_t = INT32_MAX
    U = u24(seed, n, 1, 0)
    for i in range(n):
        w, sl, e = context(ptr, nodes, i, K, backoff, nbr, deg)
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
            used[i], row = choose(table, w, sl, K, backoff, min_count, D, int(deg[v]))
            score[i] = 0.5 if row[t] == row[j] else (1.0 if row[t] > row[j] else 0.0)
            other[i] = nbr[v, j]
    return score, other, used, err, err_t


def ref_backoff_probs(ptr, nodes, K, backoff, min_count, nbr, deg, table):
    """scn_markov_hash_probs: (probs [n][D] float64 -- Python's own division of the two integers --, used_order, err)."""
    n, D = len(ptr) - 1, nbr.shape[1]
    probs, used = np.zeros((n, D), np.float64), np.zeros(n, np.int32)
    err = INT32_MAX
    for i in range(n):
        w, sl, e = context(ptr, nodes, i, K, backoff, nbr, deg)
        err = min(err, e)
        if w is None or deg[w[-1]] == 0:
            continue
        dv = int(deg[w[-1]])
        used[i], row = choose(table, w, sl, K, backoff, min_count, D, dv)
        total = int(row[:dv].sum())
        if used[i]:
            probs[i, :dv] = [int(c) / total for c in row[:dv]]
    return probs, used, err


def ref_backoff_path_scores(ptr, nodes, K, backoff, min_count, alpha, nbr, deg, table):
    """scn_markov_hash_path_scores: (prob float64, rank, total, used_order [T], err)."""
    D, T = nbr.shape[1], len(nodes)
    prob, rank = np.zeros(T, np.float64), np.full(T, -1, np.int32)
    total, used = np.zeros(T, np.int32), np.zeros(T, np.int32)
    err, alpha = INT32_MAX, float(alpha)
    for p in range(len(ptr) - 1):
        t0, L = int(ptr[p]), int(ptr[p + 1] - ptr[p])
        sl = [slot(nbr, deg, int(nodes[t0 + r]), int(nodes[t0 + r + 1])) for r in range(L - 1)]
        for r, s in enumerate(sl):
            if s < 0:
                err = min(err, t0 + r)
        for q in range(1, L):
            t = t0 + q
            if min(sl[max(q - K, 0):q]) < 0:                         # the window holds an offending pair: predicts nothing
                continue
            v, j = int(nodes[t - 1]), sl[q - 1]
            dv, m = int(deg[v]), min(q, K)
            w = [int(x) for x in nodes[t - m:t]]
            used[t], row = choose(table, w, sl[q - m:q - 1], K, backoff, min_count, D, dv)      # q < K without back-off: (0, zeros)
            row = [int(c) for c in row[:dv]]
            tot = sum(row)
            den = float(tot) + alpha * float(dv)
            prob[t] = (float(row[j]) + alpha) / den if den > 0.0 else 0.0
            rank[t] = sum(1 for x in range(dv) if row[x] > row[j] or (row[x] == row[j] and x < j))
            total[t] = tot
    return prob, rank, total, used, err


def perplexity(prob, ptr, min_prefix=2):
    """exp(-mean log prob) over the items of the paths, and the items' flat positions."""
    at = np.asarray([t for _, _, t in path_items(ptr, min_prefix)], np.int64)
    return math.exp(-float(np.sum(np.log(prob[at])) / len(at))), at


# ------------------------------------------------------------------------------------------------------------------
# cfg1: the walks prefix + [target 1, target 2] under the data set's train and test masks
# ------------------------------------------------------------------------------------------------------------------

_CFG1 = {}


def cfg1_backoff():
    """cfg1_markov() plus the table of all 8 orders of the 800 train walks prefix + [target 1, target 2] (the walks the fixture of
    the reference's weights was made from), the 200 test walks and their prefixes.  Read-only."""
    if not _CFG1:
        d = cfg1_markov()
        _CFG1.update(d)
        tr, te = np.flatnonzero(d["train"]), np.flatnonzero(d["test"])
        _CFG1["train_walks"] = [d["paths"][i] for i in tr]
        _CFG1["table"], err = ref_backoff_train(*ragged(_CFG1["train_walks"]), MAX_ORDER, d["nbr"], d["deg"])
        assert err == INT32_MAX
        _CFG1["test_walks"] = [d["paths"][i] for i in te]
        _CFG1["test_prefixes"] = [d["prefixes"][i] for i in te]
    return _CFG1


# ------------------------------------------------------------------------------------------------------------------
# without back-off it is the restatement of tests/test_host_markov.py
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ORDERS)
def test_without_backoff_it_is_the_direct_restatement_on_cfg1(order):
    d = cfg1_backoff()
    nbr, deg, table, counts = d["nbr"], d["deg"], d["table"], cfg1_counts(order)
    rows = {s: row for (k, s), row in table.items() if k == order}
    assert sorted(rows) == np.flatnonzero(counts.sum(axis=1)).tolist()          # a row per visited state and no other
    assert all(np.array_equal(row, counts[s]) for s, row in rows.items())
    # shorter prefixes among them: the direct restatement serves them as short
    pre = d["prefixes"][::5] + [p[:k] for p in d["prefixes"][:40] for k in (0, 1, 2, 3)]
    ptr, nodes = ragged(pre)
    probs, used, err = ref_backoff_probs(ptr, nodes, order, False, 1, nbr, deg, table)
    want, werr = ref_probs(ptr, nodes, order, nbr, deg, counts)
    assert err == werr == INT32_MAX and np.array_equal(probs.view(np.uint64), want.view(np.uint64))
    assert set(used.tolist()) == {0, order} and np.array_equal(used > 0, want.sum(axis=1) > 0)
    pred, tied, used, err, _ = ref_backoff_rollout(ptr, nodes, order, False, 1, 2, 7, nbr, deg, table)
    want = ref_rollout(ptr, nodes, order, 2, 7, nbr, deg, counts)
    assert np.array_equal(pred, want[0]) and np.array_equal(tied, want[1]) and err == want[2]
    full = [i for i, p in enumerate(pre) if len(p) >= order]
    ptr, nodes = ragged([pre[i] for i in full])
    target = [int(nbr[p[-1], (3 * i) % deg[p[-1]]]) for i, p in enumerate(pre[i] for i in full)]
    got = ref_backoff_two_target(ptr, nodes, order, False, 1, 7, target, nbr, deg, table)
    want = ref_two_target(ptr, nodes, order, 7, target, nbr, deg, counts)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[3:] == want[2:]
    ptr, nodes = ragged(d["test_walks"][:60])
    for alpha in (0.0, 1.0):
        got = ref_backoff_path_scores(ptr, nodes, order, False, 1, alpha, nbr, deg, table)
        want = np_markov_path_scores(ptr, nodes, order, alpha, nbr, deg, counts)
        assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and np.array_equal(got[1], want[1])
        assert np.array_equal(got[2], want[2]) and got[4] == want[3] and np.array_equal(got[3] > 0, want[2] > 0)


# ------------------------------------------------------------------------------------------------------------------
# cfg1's integers and perplexities, derived with an independent dictionary model and recomputed here
# ------------------------------------------------------------------------------------------------------------------

def used_hist(d, K, min_count):
    ptr, nodes = ragged(d["test_prefixes"])
    _, used, err = ref_backoff_probs(ptr, nodes, K, True, min_count, d["nbr"], d["deg"], d["table"])
    assert err == INT32_MAX
    return {k: int(c) for k, c in enumerate(np.bincount(used, minlength=K + 1))}


def test_cfg1_states_bounds_and_order_histograms():
    d = cfg1_backoff()
    ptr, _ = ragged(d["train_walks"])
    assert len(d["train_walks"]) == 800 and len(d["test_walks"]) == 200
    assert n_states(d["table"], 8) == [307, 646, 945, 1270, 1612, 1878, 1995, 1947]
    assert key_bound(ptr, 8) == [8158, 7358, 6558, 5758, 4958, 4158, 3438, 2797]
    assert all(n <= b for n, b in zip(n_states(d["table"], 8), key_bound(ptr, 8)))
    assert used_hist(d, 4, 1) == {0: 1, 1: 5, 2: 8, 3: 4, 4: 182}
    assert used_hist(d, 4, 2) == {0: 4, 1: 10, 2: 14, 3: 13, 4: 159}
    h8 = used_hist(d, 8, 1)
    assert h8 == {0: 1, 1: 5, 2: 8, 3: 4, 4: 31, 5: 38, 6: 29, 7: 26, 8: 58}
    assert all(h8[k] >= 1 for k in range(9))                       # no branch of the back-off goes untested on this data


# K: (fixed order K, its items without a seen state, back-off from K), in full precision: the dictionary restatement's values on the
# CPU, which print as the four decimals derived independently (2.4778 / 2.3912 / 3.0156 / 3.7073 and 2.4778 / 2.3692 / 2.5566 / 2.7393)
PERPLEXITY = {1: (2.477841966211377, 7, 2.477841966211377), 2: (2.3911985629189716, 40, 2.369219098185178),
              3: (3.0156220153539497, 284, 2.5566288381627986), 4: (3.7073225013087137, 549, 2.7392913358285926)}
PRINTED = {1: (2.4778, 2.4778), 2: (2.3912, 2.3692), 3: (3.0156, 2.5566), 4: (3.7073, 2.7393)}


def test_cfg1_perplexities():
    """Test-mask perplexity at min_prefix 2, alpha 1 of the fixed order K (and its items without a seen state) and of the back-off
    from K, each to 1e-9 relative of the recorded value (a sum of 1899 logarithms in fp64 is good to about 1899 x 2^-53 = 2e-13
    relative; 1e-9 leaves room for another libm and another summation order, and a change of one item's order or smoothing moves a
    perplexity by 1e-5 or more).  The fixed orders 1-3 also agree to 1e-9 with the direct-table restatement: the same rule, other
    code."""
    d = cfg1_backoff()
    nbr, deg = d["nbr"], d["deg"]
    ptr, nodes = ragged(d["test_walks"])
    tptr, tnodes = ragged(d["train_walks"])
    fixed, back = {}, {}
    for K, (want_fixed, want_unseen, want_back) in PERPLEXITY.items():
        prob, _, _, used, err = ref_backoff_path_scores(ptr, nodes, K, False, 1, 1.0, nbr, deg, d["table"])
        fixed[K], at = perplexity(prob, ptr)
        assert err == INT32_MAX and len(at) == 1899 and int((used[at] == 0).sum()) == want_unseen
        if K <= 3:                                                   # the direct table's restatement: the same rule, other code
            counts, _ = ref_count(tptr, tnodes, K, nbr, deg)
            direct, _ = perplexity(np_markov_path_scores(ptr, nodes, K, 1.0, nbr, deg, counts)[0], ptr)
            assert abs(fixed[K] - direct) <= 1e-9 * direct
        prob, _, _, used, _ = ref_backoff_path_scores(ptr, nodes, K, True, 1, 1.0, nbr, deg, d["table"])
        back[K], _ = perplexity(prob, ptr)
        assert abs(fixed[K] - want_fixed) <= 1e-9 * want_fixed and abs(back[K] - want_back) <= 1e-9 * want_back
        assert (round(want_fixed, 4), round(want_back, 4)) == PRINTED[K]
        assert used[at].max() <= K and used[at].min() >= 0
    assert abs(back[1] - fixed[1]) <= 1e-9 * fixed[1]                # order 1 has nothing to back off to but "unseen"
    assert back[2] < fixed[2] < back[1]
    assert back[3] < fixed[3] and back[4] < fixed[4]


# ------------------------------------------------------------------------------------------------------------------
# by hand on the 4-node graph: 0-1, 0-2, 0-3, 1-2, 2-3
# ------------------------------------------------------------------------------------------------------------------

def test_tiny4_backoff_by_hand():
    nbr, deg = tiny4()
    table, err = ref_backoff_train(*ragged(TINY_WALKS), 3, nbr, deg)
    assert err == INT32_MAX
    # order 1 is the direct table's: 0>1 1>2 2>3 3>0 | 1>2 2>0 0>3 | 3>2 2>1 1>0 0>2 | 2>0
    assert [table[(1, v)][:3].tolist() for v in range(4)] == [[1, 1, 1], [1, 2, 0], [2, 1, 1], [1, 1, 0]]
    assert n_states(table, 3) == [4, 3 + 2 + 3 - 1, 2 + 1 + 2]       # (1, 2) starts a window in two walks
    # a prefix of one node uses order 1
    pptr, pnodes = ragged([[1], [0, 1], [2, 3, 0], [3, 0], [0, 2, 1]])
    probs, used, _ = ref_backoff_probs(pptr, pnodes, 3, True, 1, nbr, deg, table)
    assert used.tolist() == [1, 2, 1, 1, 2]                          # (0, 2, 1) was never seen, (2, 1) > 0 once
    assert probs[0].tolist() == [1 / 3, 2 / 3, 0] and probs[1].tolist() == [0, 1, 0]       # 1 > 0 once, 1 > 2 twice; (0, 1) > 2 once
    # (2, 3, 0) ends a walk and so does its (3, 0): neither has a node after it anywhere, on to order 1 at node 0
    assert (3, state([2, 3, 0], [2, 0], 3)) not in table and (2, state([3, 0], [0], 3)) not in table
    assert probs[2].tolist() == probs[3].tolist() == [1 / 3, 1 / 3, 1 / 3]
    # a state seen once backs off under min_count = 2: (0, 1) > 2 once, so node 1's own row serves
    probs2, used2, _ = ref_backoff_probs(pptr, pnodes, 3, True, 2, nbr, deg, table)
    assert used2.tolist() == [1, 1, 1, 1, 1] and probs2[1].tolist() == [1 / 3, 2 / 3, 0]
    # without back-off only order 3 is tried and the shorter prefixes are short
    probs3, used3, _ = ref_backoff_probs(pptr, pnodes, 3, False, 1, nbr, deg, table)
    assert used3.tolist() == [0, 0, 0, 0, 0] and not probs3.any()
    # no order qualifies (node 0 was left three times, min_count is 4): all neighbours tie, 0.5 in the 2-target test, uniform
    pred, tied, used, _, ties = ref_backoff_rollout(*ragged([[3, 0]] * 64), 3, True, 4, 1, 5, nbr, deg, table)
    assert (used == 0).all() and (tied == 3).all() and set(pred[:, 0].tolist()) == {1, 2, 3} and len(ties) == 64
    score, other, used, _, _ = ref_backoff_two_target(*ragged([[3, 0]]), 3, True, 4, 0, [1], nbr, deg, table)
    assert score[0] == 0.5 and used[0] == 0
    prob, rank, total, used, _ = ref_backoff_path_scores(*ragged([[3, 0, 2]]), 3, True, 4, 1.0, nbr, deg, table)
    assert prob.tolist() == [0, 0.5, 1 / 3] and total.tolist() == [0, 0, 0] and used.tolist() == [0, 0, 0] and rank.tolist() == [-1, 0, 1]


def test_rollout_chooses_the_order_again_at_every_hop():
    nbr, deg = tiny4()
    table, _ = ref_backoff_train(*ragged(TINY_WALKS), 3, nbr, deg)
    pred, tied, used, _, _ = ref_backoff_rollout(*ragged([[1]]), 3, True, 1, 3, 0, nbr, deg, table)
    # 1 -> 2 (order 1: 2 of 3), then (1, 2) > 3 and > 0 once each (order 2, a tie), then order 3 or a back-off from it
    assert pred[0, 0] == 2 and used[0, :2].tolist() == [1, 2] and tied[0].tolist()[:2] == [1, 2]
    # a longer window than the table ever saw still reaches its longest suffix: (1, 2, 3) > 0 once, (1, 2, 0) > 3 once
    assert used[0, 2] == 3 and tied[0, 2] == 1 and pred[0, 2] == {3: 0, 0: 3}[int(pred[0, 1])]
    ctx = [1, 2, int(pred[0, 1])]
    sl = [slot(nbr, deg, a, b) for a, b in zip(ctx[:-1], ctx[1:])]
    assert used[0, 2] == choose(table, ctx, sl, 3, True, 1, 3, int(deg[ctx[-1]]))[0] >= 1


def test_a_bad_pair_inserts_nothing_at_any_order():
    nbr, deg = tiny4()
    walks = [[0, 1, 2], [0, 1, 3, 2, 0, 1], [2, 0, 7, 0, 1]]                # (1, 3) is no edge; 7 is no node
    table, err = ref_backoff_train(*ragged(walks), 4, nbr, deg)
    assert err == 3 + 1                                              # walk 1, position 1
    clean, e2 = ref_backoff_train(*ragged([[0, 1, 2], [0, 1], [3, 2, 0, 1], [2, 0], [0, 1]]), 4, nbr, deg)
    assert e2 == INT32_MAX and sorted(table) == sorted(clean) and all(np.array_equal(table[k], clean[k]) for k in table)
    assert (1, 1) in table and table[(1, 1)].tolist() == [0, 1, 0]         # 1 > 2 of walk 0 alone: 1 > 3 counted nothing
    pptr, pnodes = ragged([[0, 1, 2], [2, 0, 7], [1, 3], [9]])
    for backoff in (True, False):
        pred, _, used, err, _ = ref_backoff_rollout(pptr, pnodes, 2, backoff, 1, 2, 0, nbr, deg, table)
        assert err == 4 and pred[1].tolist() == [-1, -1] and pred[0, 0] >= 0 and used[1].tolist() == [0, 0]
    assert ref_backoff_rollout(pptr, pnodes, 1, True, 1, 1, 0, nbr, deg, table)[3] == 5      # order 1: the foreign last node
    assert ref_backoff_probs(pptr[3:] - 8, pnodes[8:], 3, True, 1, nbr, deg, table)[2] == 0   # a window of one foreign node


# ------------------------------------------------------------------------------------------------------------------
# argument checks that never reach the device, and the driver's flags
# ------------------------------------------------------------------------------------------------------------------

def hash_calls(lib, n, K, V, D, cap, backoff=1, min_count=1, hops=2, alpha=1.0):
    """The status of every entry point on NULL arrays."""
    seed, N = ctypes.c_uint64(0), None
    return [lib.scn_markov_hash_insert(n, N, N, K, V, D, N, N, N, cap, N, N, N),
            lib.scn_markov_hash_count(n, N, N, K, V, D, N, N, N, N, cap, 5, N, N, N),
            lib.scn_markov_hash_rollout(n, N, N, K, backoff, min_count, hops, seed, V, D, N, N, N, N, cap, N, N, N, N, N, N),
            lib.scn_markov_hash_two_target(n, N, N, K, backoff, min_count, seed, N, V, D, N, N, N, N, cap, N, N, N, N, N, N, N),
            lib.scn_markov_hash_probs(n, N, N, K, backoff, min_count, V, D, N, N, N, N, cap, N, N, N, N, N),
            lib.scn_markov_hash_path_scores(n, N, N, K, backoff, min_count, ctypes.c_double(alpha), V, D, N, N, N, N, cap, N, N, N, N, N,
                                            N, N)]


def test_limits_and_calls_that_return_before_any_launch():
    from scone_gcn_amd import _lib
    lib = _lib.load()
    U, A, S = _lib.SCN_ERR_UNSUPPORTED, _lib.SCN_ERR_BAD_ARG, -2
    assert _lib.SCN_MARKOV_HASH_MAX_ORDER == MAX_ORDER
    assert "#define SCN_MARKOV_HASH_MAX_ORDER 8" in open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                      "include", "scone_hip.h")).read()
    # the key's 59 bits: V * D^(K-1) < 2^59
    for V, D, K in [(400, 13, 8), (369004, 19, 8), (4, 3, 1), (2 ** 31 - 1, 2 ** 27, 2), (2 ** 31 - 1, 2 ** 28, 2), (1, 2, 8),
                    (1, 169, 8), (1, 345, 8), (1, 346, 8), (2 ** 31 - 1, 2 ** 31 - 1, 1), (2 ** 31 - 1, 2 ** 31 - 1, 2), (400, 13, 0),
                    (400, 13, 9), (400, 13, -1),
                    # products at and past 2^64, which a 64-bit product would wrap below the limit
                    (2 ** 22, 64, 8), (2 ** 22, 64, 7), (2 ** 17, 64, 8), (2 ** 16, 64, 8), (2 ** 31 - 1, 2 ** 31 - 1, 8), (3, 2 ** 31 - 1, 3),
                    (2 ** 4, 2 ** 16, 5), (2 ** 4, 2 ** 16, 4), (2 ** 26, 2 ** 11, 4), (2 ** 26, 2 ** 11, 5), (2 ** 2, 2 ** 19, 4),
                    (2 ** 2, 2 ** 19, 8)] + [(V, 70, 8) for V in range(2240000, 4900000, 99991)] + \
                   [(V, 70, K) for V in (70, 4900, 2 ** 31 - 1) for K in range(1, 9)]:
        ok = 1 <= K <= MAX_ORDER and V * D ** (K - 1) < 2 ** KEY_SHIFT
        assert lib.scn_markov_hash_check(V, D, K, 1024) == (0 if ok else U), (V, D, K)
    assert lib.scn_markov_hash_check(0, 3, 1, 1024) == S and lib.scn_markov_hash_check(3, 0, 1, 1024) == S
    for cap in (0, -8, 3, 1000, 2 ** 20 + 1, 3 * 2 ** 40):
        assert lib.scn_markov_hash_check(400, 13, 2, cap) == A
    for cap in (1, 2, 1024, 2 ** 40):
        assert lib.scn_markov_hash_check(400, 13, 2, cap) == 0
    assert hash_calls(lib, 3, 0, 400, 13, 1024) == [U] * 6 and hash_calls(lib, 3, 9, 400, 13, 1024) == [U] * 6
    assert hash_calls(lib, 3, 3, 2 ** 31 - 1, 2 ** 20, 1024) == [U] * 6
    assert hash_calls(lib, 3, 2, 400, 13, 1000) == [A] * 6
    assert hash_calls(lib, 3, 2, 400, 13, 1024, min_count=0)[2:] == [A] * 4
    assert hash_calls(lib, 3, 2, 400, 13, 1024, backoff=2)[2:] == [A] * 4
    assert hash_calls(lib, 3, 2, 400, 13, 1024, alpha=-1.0)[5] == A and hash_calls(lib, 3, 2, 400, 13, 1024, hops=0)[2] == S
    assert hash_calls(lib, 0, 2, 400, 13, 1024) == [0] * 6          # empty calls
    assert hash_calls(lib, -1, 2, 400, 13, 1024) == [S] * 6
    assert hash_calls(lib, 3, 2, 400, 13, 1024) == [A] * 6           # NULL arrays of a call that would launch
    assert lib.scn_markov_hash_number(None, 1000, 2, None, None, None, None) == A
    assert lib.scn_markov_hash_number(None, 1024, 9, None, None, None, None) == U
    assert lib.scn_markov_hash_number(None, 2 ** 31, 2, None, None, None, None) == U
    assert lib.scn_markov_hash_number(None, 1024, 2, None, None, None, None) == A


def test_python_class_refuses_before_touching_a_device():
    from scone_gcn_amd import markov_model as mm
    for K in (0, 9, 1.5):
        with pytest.raises(ValueError, match="max_order"):
            mm.Markov_Backoff(K)
    for c in (0, -1, 1.5):
        with pytest.raises(ValueError, match="min_count"):
            mm.Markov_Backoff(2, min_count=c)
    for load in (0.0, 1.5):
        with pytest.raises(ValueError, match="load"):
            mm.Markov_Backoff(2, load=load)
    nbr, _ = tiny4()
    with pytest.raises(ValueError, match="power of two"):
        mm.Markov_Backoff(2).train(nbr, TINY_WALKS, capacity=1000)
    wide = np.full((8, 300), -1, np.int64)
    wide[:, 0] = (np.arange(8) + 1) % 8
    with pytest.raises(ValueError, match="2\\^59"):
        mm.Markov_Backoff(8).train(wide, [[0, 1, 2]])                # 8 x 300^7 = 1.7e18 >= 2^59 = 5.8e17
    with pytest.raises(ValueError, match="2\\^59"):
        mm.Markov_Backoff(8).train(np.concatenate([wide, wide], axis=1)[:, :512], [[0, 1, 2]])      # 8 x 512^7 = 2^66: past 64 bits
    with pytest.raises(RuntimeError, match="train"):
        mm.Markov_Backoff(3).predict_paths([[0, 1]], 1)
    m = mm.Markov_Backoff(4, seed=3, backoff=False, min_count=2)
    assert (m.max_order, m.order, m.seed, m.backoff, m.min_count, m.shortest) == (4, 4, 3, False, 2, 4)
    assert mm.Markov_Backoff(4).shortest == 1 and mm.Markov_Backoff(4).n_states == [] and mm.Markov_Backoff(4).capacity == 0
    # the sizing rule: the key bound of the walks, the next power of two >= bound / load
    ptr, _ = ragged(cfg1_backoff()["train_walks"])
    assert mm.key_bound(ptr, 8) == sum(key_bound(ptr, 8)) == 43183 and mm.key_bound(ptr, 1) == 8158
    assert [mm.hash_capacity(b, l) for b, l in ((43183, 0.5), (8158, 0.5), (8192, 0.5), (8192, 1.0), (8193, 1.0), (0, 0.5), (3, 0.75))] == \
        [131072, 16384, 16384, 8192, 16384, 1, 4]
    # the hash of the kernels, restated twice
    x = np.array([0, 1, 5, (7 << KEY_SHIFT) | 12345, 2 ** 64 - 2], np.uint64)
    assert [int(v) for v in mm.hash_mix(x)] == [mm.hash_mix(int(v)) for v in x] and mm.hash_mix(0) == 0
    assert mm.hash_mix(1) == 0x5692161d100b05e5                   # splitmix64's finaliser of 1


def test_hyperparams_parse_the_backoff_flags():
    from scone_gcn_amd import trajectory_experiments as te
    hp = te.hyperparams(["prog"])
    assert hp.get("markov_backoff", 0) == 0 and hp.get("markov_min_count", 1) == 1 and hp["markov_order"] == 1
    hp = te.hyperparams(["prog", "-markov", "1", "-markov_backoff", "1", "-markov_min_count", "2", "-markov_order", "8"])
    assert hp["markov_backoff"] == 1 and int(hp["markov_min_count"]) == 2 and int(hp["markov_order"]) == 8


class _Stop(Exception):
    pass


@pytest.mark.parametrize("flag", (0, 1))
def test_the_flag_picks_the_class_of_the_markov_block(flag, monkeypatch, tmp_path):
    """-markov_backoff 0 leaves train_model()'s Markov block calling Markov_Model with the order; 1 calls Markov_Backoff with the
    maximum order and the minimum count.  Both classes are replaced: nothing reaches a device."""
    from scone_gcn_amd import markov_model as mm, trajectory_experiments as te
    made = []

    class Direct:
        def __init__(self, *a, **k):
            made.append(("direct", a, k))
            raise _Stop()

    class Backoff:
        def __init__(self, *a, **k):
            made.append(("backoff", a, k))
            raise _Stop()

    monkeypatch.setattr(mm, "Markov_Model", Direct)
    monkeypatch.setattr(mm, "Markov_Backoff", Backoff)
    with pytest.raises(_Stop):
        te.markov_experiments(None, [[0, 1]], [[2], [3]], [1], [0], order=3, **({"backoff": True, "min_count": 2} if flag else {}))
    assert made == ([("backoff", (3,), {"seed": 0, "backoff": True, "min_count": 2})] if flag else [("direct", (3,), {"seed": 0})])


@pytest.mark.parametrize("flag", (0, 1))
def test_the_flags_reach_both_markov_blocks_of_train_model(flag, monkeypatch):
    """train_model() builds the baseline of its five experiments and of its path likelihood through markov_baseline(order,
    **markov_rule(hp)): with the flag off that is Markov_Model(order) as before, with it on Markov_Backoff(order, min_count)."""
    from scone_gcn_amd import markov_model as mm, trajectory_experiments as te
    made = []
    monkeypatch.setattr(mm, "Markov_Model", lambda *a, **k: made.append(("direct", a, k)))
    monkeypatch.setattr(mm, "Markov_Backoff", lambda *a, **k: made.append(("backoff", a, k)))
    hp = te.hyperparams(["prog", "-markov", "1", "-markov_order", "3"] + (["-markov_backoff", "1", "-markov_min_count", "2"] if flag else []))
    rule = te.markov_rule(hp)
    assert rule == ({"backoff": True, "min_count": 2} if flag else {})
    assert te.markov_rule(te.hyperparams(["prog", "-markov_min_count", "5"])) == {}          # a count without the flag changes nothing
    assert te.markov_rule(te.hyperparams(["prog", "-markov_backoff", "1"])) == {"backoff": True, "min_count": 1}
    te.markov_baseline(int(hp["markov_order"]), **rule)
    assert made == ([("backoff", (3,), {"seed": 0, "backoff": True, "min_count": 2})] if flag else [("direct", (3,), {"seed": 0})])
    # both blocks of train_model take the rule, and neither imports a class of its own
    import inspect
    src = inspect.getsource(te.train_model)
    assert src.count("markov_rule(hp)") == 1 and src.count("**rule") == 2 and "import Markov" not in src
