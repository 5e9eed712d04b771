"""Whole-path scores of the Markov and projection baselines without a GPU: this file's NumPy restatements of scn_markov_path_scores
and scn_project_path_scores (include/scone_hip.h) -- explicit loops in step order, built on the helpers of tests/test_host_markov.py
and tests/test_host_projection.py -- checked against what those files' restatements of the per-prefix calls (ref_probs, ref_predict)
give on every prefix, plus the records' conventions and the parts of the Python surface that need no device.
tests/test_gpu_baseline_paths.py imports the restatements."""
import ctypes

import numpy as np
import pytest

from tests.test_host_markov import INT32_MAX, TINY_WALKS, cfg1_counts, cfg1_markov, ragged, ref_count, ref_probs, slot, state
from tests.test_host_markov import tiny4 as markov_tiny4
from tests.test_host_projection import cycle4, fixture, ref_predict
from tests.test_host_projection import cfg1 as projection_cfg1
from tests.test_host_projection import tiny4 as projection_tiny4

U = 2.0 ** -53                # unit roundoff of fp64


# ------------------------------------------------------------------------------------------------------------------
# the restatements
# ------------------------------------------------------------------------------------------------------------------

def np_markov_path_scores(ptr, nodes, order, alpha, nbr, deg, counts):
    """scn_markov_path_scores: (prob float64 [T], rank int32 [T], total int32 [T], err)."""
    D, T = nbr.shape[1], len(nodes)
    prob, rank, total = np.zeros(T, np.float64), np.full(T, -1, np.int32), np.zeros(T, np.int32)
    err = INT32_MAX
    alpha = float(alpha)
    for p in range(len(ptr) - 1):
        t0, L = int(ptr[p]), int(ptr[p + 1] - ptr[p])
        sl = [slot(nbr, deg, int(nodes[t0 + r]), int(nodes[t0 + r + 1])) for r in range(L - 1)]
        for r, s in enumerate(sl):
            if s < 0:
                err = min(err, t0 + r)
        for q in range(1, L):
            t = t0 + q
            if min(sl[max(q - order, 0):q]) < 0:                     # the window holds an offending pair: predicts nothing
                continue
            v, j = int(nodes[t - 1]), sl[q - 1]
            dv = int(deg[v])
            row = [0] * dv                                           # a prefix shorter than the order: the all-zero row
            if q >= order:
                row = [int(c) for c in counts[state([int(nodes[t - order])], sl[q - order:q - 1], D), :dv]]
            tot = sum(row)
            den = float(tot) + alpha * float(dv)
            prob[t] = (float(row[j]) + alpha) / den if den > 0.0 else 0.0
            rank[t] = sum(1 for x in range(dv) if row[x] > row[j] or (row[x] == row[j] and x < j))
            total[t] = tot
    return prob, rank, total, err


def np_project_path_scores(cx, V, ptr, nodes, D=None):
    """scn_project_path_scores on the complex cx (a tests.test_host_projection.Cx) with the basis V (E, k): a dict of logp, mass
    (float64 [T]), rank (int32 [T]), coef (float64 [T][k]), err, and for the tests' error bounds logits ([T][D]), lse ([T]) and
    absdot ([T]): the largest sum_m |V[e, m]| sum_i |V[e_i, m]| over the edges e at the record's last node."""
    D = cx.D if D is None else D
    V = np.asarray(V, np.float64).reshape(cx.E, -1)
    k, T = V.shape[1], len(nodes)
    out = {"logp": np.zeros(T), "mass": np.zeros(T), "rank": np.full(T, -1, np.int32), "coef": np.zeros((T, k)), "err": INT32_MAX,
           "logits": np.zeros((T, D)), "lse": np.zeros(T), "absdot": np.zeros(T)}
    for p in range(len(ptr) - 1):
        t0, L = int(ptr[p]), int(ptr[p + 1] - ptr[p])
        c, mag = [0.0] * k, [0.0] * k                                # the running sum from +0, and that of the magnitudes
        for q in range(1, L):
            t = t0 + q
            a, b = int(nodes[t - 1]), int(nodes[t])
            inside = 0 <= a < cx.n_nodes and 0 <= b < cx.n_nodes
            e = cx.at.get((min(a, b), max(a, b))) if inside else None
            if e is None:                                            # this record and every later one of the path predict nothing
                out["err"] = min(out["err"], t - 1)
                break
            out["coef"][t] = c
            lg = np.zeros(D)
            for e2 in np.flatnonzero(cx.B1[a]).tolist():
                other = int(cx.edges[e2, 0] + cx.edges[e2, 1] - a)
                h, hm = 0.0, 0.0
                for m in range(k):
                    h += V[e2, m] * c[m]
                    hm += abs(V[e2, m]) * mag[m]
                lg[slot(cx.nbr, cx.deg, a, other)] = cx.B1[other, e2] * h
                out["absdot"][t] = max(out["absdot"][t], hm)
            dv, j = int(cx.deg[a]), slot(cx.nbr, cx.deg, a, b)
            mx = float(lg.max())
            s_all = 0.0
            for x in range(D):
                s_all += np.exp(lg[x] - mx)
            lse = mx + np.log(s_all)
            s_real = 0.0
            for x in range(dv):
                s_real += np.exp(lg[x] - lse)
            out["logits"][t], out["lse"][t] = lg, lse
            out["logp"][t] = lg[j] - lse
            out["mass"][t] = np.log(s_real)
            out["rank"][t] = sum(1 for x in range(dv) if lg[x] > lg[j] or (lg[x] == lg[j] and x < j))
            sign = cx.B1[b, e]
            for m in range(k):                                       # the step enters the sums of the records behind it
                c[m] += sign * V[e, m]
                mag[m] += abs(V[e, m])
    return out


def logit_bound(r, t, n_steps, k):
    """The standard forward bound of a record's logits: u times the term counts of the two nested sums times the sum of the
    magnitudes of their terms."""
    return (n_steps + k) * U * r["absdot"][t]


def softmax_bound(r, t, D, extra=4):
    """... and of the soft-max behind them: D additions of exponentials, the exponential, the logarithm and the two subtractions."""
    return (D + extra) * U * (1.0 + abs(r["lse"][t]))


def record_bound(r, t, n_steps, k, D):
    """... and of logp and mass: the taken logit's error, the logsumexp's (it moves by at most the largest logit error), the
    soft-max's own roundings."""
    return 2.0 * logit_bound(r, t, n_steps, k) + softmax_bound(r, t, D)


# The one safety factor on the bounds above: 2 because a test compares two computed values, each within the bound of the exact
# one, and 2 for libm's exp and log, which are within a few ulp where the bound assumes half an ulp.
SAFETY = 4.0


def path_items(ptr, min_prefix):
    """(path, prefix length k, flat position of the node predicted) of every item, path-major with k ascending."""
    k0 = max(int(min_prefix), 1)
    return [(p, k, int(ptr[p]) + k) for p in range(len(ptr) - 1) for k in range(k0, int(ptr[p + 1] - ptr[p]))]


def random_walks(nbr, deg, rs, lengths, start=None):
    """Walks with backtracking and loops: every next node a uniform neighbour."""
    out = []
    live = np.flatnonzero(np.asarray(deg) > 0)                       # (the 400-point complex has points without an edge: its holes)
    for n in lengths:
        v = int(live[rs.randint(len(live))]) if start is None else int(start)
        walk = [v] if n else []
        while len(walk) < n:
            v = int(nbr[v][rs.randint(deg[v])])
            walk.append(v)
        out.append(walk)
    return out


def prefix_flows(cx, prefixes):
    """(E, N) float64 flows of node prefixes through the project's own paths_to_flows."""
    from scone_gcn_amd.synthetic_data_gen import Complex, paths_to_flows
    full = Complex(n_nodes=cx.n_nodes, edges=cx.edges, faces=cx.faces)
    return paths_to_flows(full, prefixes).todense()[:, :, 0].T.astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------
# Markov
# ------------------------------------------------------------------------------------------------------------------

def check_alpha0_is_ref_probs(paths, order, nbr, deg, counts):
    ptr, nodes = ragged(paths)
    prob, rank, total, err = np_markov_path_scores(ptr, nodes, order, 0.0, nbr, deg, counts)
    assert err == INT32_MAX
    items = path_items(ptr, 1)
    prefixes = [paths[p][:k] for p, k, _ in items]
    want, e2 = ref_probs(*ragged(prefixes), order, nbr, deg, counts)
    assert e2 == INT32_MAX
    for i, (p, k, t) in enumerate(items):
        j = slot(nbr, deg, paths[p][k - 1], paths[p][k])
        assert prob[t] == want[i, j], (p, k)                         # float64, bit for bit
        assert rank[t] == sum(1 for x in range(deg[paths[p][k - 1]]) if want[i, x] > want[i, j] or (want[i, x] == want[i, j] and x < j))
    first = ptr[:-1][np.diff(ptr) > 0]
    assert not prob[first].any() and (rank[first] == -1).all() and not total[first].any()
    return len(items)


@pytest.mark.parametrize("order", (1, 2, 3))
def test_markov_alpha0_equals_ref_probs_of_every_prefix_on_tiny4(order):
    nbr, deg = markov_tiny4()
    counts, _ = ref_count(*ragged(TINY_WALKS), order, nbr, deg)
    walks = TINY_WALKS + random_walks(nbr, deg, np.random.RandomState(order), [9, 2, 1, 0, 7, order, order + 1])
    assert check_alpha0_is_ref_probs(walks, order, nbr, deg, counts) >= 28


@pytest.mark.parametrize("order", (1, 2, 3))
def test_markov_alpha0_equals_ref_probs_of_every_prefix_on_cfg1(order):
    d = cfg1_markov()
    counts = cfg1_counts(order)
    paths = d["paths"][::4]                                          # 250 of the 1000 walks, train and test rows alike
    assert check_alpha0_is_ref_probs(paths, order, d["nbr"], d["deg"], counts) > 1500
    # the counts are those of the reference's fixture (tests/test_host_markov.py checks every weight of it against them)
    assert int((counts != 0).sum()) == len(d["fix"]["w%d_prob" % order])


def test_markov_alpha_by_hand():
    nbr, deg = markov_tiny4()
    c1, _ = ref_count(*ragged(TINY_WALKS), 1, nbr, deg)
    assert c1[2].tolist() == [2, 1, 1]                               # node 2 went to 0 twice, to 1 and to 3 once
    ptr, nodes = ragged([[1, 2, 0], [1, 2, 1], [1, 2, 3]])
    prob, rank, total, _ = np_markov_path_scores(ptr, nodes, 1, 1.0, nbr, deg, c1)
    assert prob[[2, 5, 8]].tolist() == [3.0 / 7.0, 2.0 / 7.0, 2.0 / 7.0] and total[[2, 5, 8]].tolist() == [4, 4, 4]
    assert rank[[2, 5, 8]].tolist() == [0, 1, 2]                     # 1 and 3 tie on the count: the lower slot first
    prob, _, _, _ = np_markov_path_scores(ptr, nodes, 1, 0.25, nbr, deg, c1)
    assert prob[2] == 2.25 / 4.75 and prob[5] == 1.25 / 4.75


def test_markov_unseen_state_and_short_prefix_are_uniform_under_smoothing():
    nbr, deg = markov_tiny4()
    c2, _ = ref_count(*ragged(TINY_WALKS), 2, nbr, deg)
    assert c2[state([3, 0], [0], 3)].sum() == 0                      # (3, 0) ends a walk and starts none
    ptr, nodes = ragged([[3, 0, 2], [1, 0], [0, 1, 2]])
    for alpha in (0.25, 1.0, 0.1):
        prob, rank, total, err = np_markov_path_scores(ptr, nodes, 2, alpha, nbr, deg, c2)
        assert err == INT32_MAX
        assert prob[2] == alpha / (alpha * 3.0) and total[2] == 0 and rank[2] == 1       # unseen: 1 / deg, the slot taken
        assert prob[1] == alpha / (alpha * 2.0) and prob[4] == alpha / (alpha * 2.0)     # short prefixes at nodes 3 and 1
        assert rank[4] == 0 and total[7] == 1 and prob[7] == (1.0 + alpha) / (1.0 + alpha * 2.0)
    prob, _, total, _ = np_markov_path_scores(ptr, nodes, 2, 0.0, nbr, deg, c2)
    assert prob.tolist() == [0, 0, 0, 0, 0, 0, 0, 1.0] and total.tolist() == [0] * 7 + [1]


# ------------------------------------------------------------------------------------------------------------------
# projection
# ------------------------------------------------------------------------------------------------------------------

def check_projection_against_ref_predict(cx, V, paths):
    """Every record's logits, logp, rank and mass against ref_predict on paths_to_flows of its prefix.  The two routes add the same
    terms in different orders (V (V^T f) over the flow's edges there, the running sum over the steps here), so they are compared
    against SAFETY times the forward bound; the rank where the taken logit is further than that from every other neighbour's."""
    V = np.asarray(V, np.float64).reshape(cx.E, -1)
    ptr, nodes = ragged(paths)
    r = np_project_path_scores(cx, V, ptr, nodes)
    assert r["err"] == INT32_MAX
    items = path_items(ptr, 1)
    prefixes = [paths[p][:k] for p, k, _ in items]
    probs, logits = ref_predict(cx, V, prefix_flows(cx, prefixes), [pre[-1] for pre in prefixes])
    worst = 0.0
    for i, (p, k, t) in enumerate(items):
        a, b = paths[p][k - 1], paths[p][k]
        j, dv = slot(cx.nbr, cx.deg, a, b), int(cx.deg[a])
        tol = SAFETY * record_bound(r, t, k - 1, V.shape[1], cx.D)
        errs = (abs(r["logits"][t] - logits[i]).max(), abs(r["logp"][t] - np.log(probs[i, j])),
                abs(r["mass"][t] - np.log(probs[i, :dv].sum())))
        assert max(errs) <= tol, (p, k, errs, tol)
        worst = max(worst, max(errs) / tol)
        gap = np.abs(np.delete(logits[i, :dv], j) - logits[i, j]).min() if dv > 1 else np.inf
        if gap > tol:
            assert r["rank"][t] == sum(1 for x in range(dv) if logits[i, x] > logits[i, j] or (logits[i, x] == logits[i, j] and x < j))
    first = ptr[:-1][np.diff(ptr) > 0]
    assert not r["logp"][first].any() and (r["rank"][first] == -1).all() and not r["mass"][first].any()
    return r, items, worst


def test_projection_on_tiny4_has_no_hole():
    cx = projection_tiny4()
    paths = random_walks(cx.nbr, cx.deg, np.random.RandomState(2), [6, 3, 2, 1, 0, 9])
    r, items, _ = check_projection_against_ref_predict(cx, np.zeros((cx.E, 0)), paths)
    for p, k, t in items:                                            # dim = 0: every logit exactly 0, exact throughout
        assert r["logp"][t] == -np.log(3.0) and r["rank"][t] == slot(cx.nbr, cx.deg, paths[p][k - 1], paths[p][k])
        assert abs(r["mass"][t] - np.log(cx.deg[paths[p][k - 1]] / 3.0)) <= 8 * U
    # a Gaussian basis on the same graph: the kernel does not care whether V is harmonic
    check_projection_against_ref_predict(cx, np.random.RandomState(3).randn(cx.E, 3), paths)


def test_projection_on_the_four_cycle_backtrack_and_double_crossing():
    cx = cycle4()
    V = np.array([[1.0], [-1.0], [1.0], [1.0]]) / 2.0               # the cycle's sign vector (tests/test_host_projection.py)
    back, twice = [0, 1, 0, 1], [0, 1, 2, 3, 0, 1, 2]
    r, items, _ = check_projection_against_ref_predict(cx, V, [back, twice, [2, 3]])
    ptr, _ = ragged([back, twice, [2, 3]])
    assert r["coef"][:4, 0].tolist() == [0.0, 0.0, 0.5, 0.0]         # (0, 1) forth and back cancels
    assert r["coef"][4:11, 0].tolist() == [0.0, 0.0, 0.5, 1.0, 1.5, 2.0, 2.5]          # (0, 1) a second time the same way counts twice
    # once round the cycle the projection prefers to go on round it
    t = 4 + 5
    assert r["rank"][t] == 0 and r["logp"][t] > np.log(0.5)


def test_projection_on_cfg1_against_ref_predict_and_the_fixture():
    """The basis is the dense null space tests/test_host_projection.py checks against tests/golden/cfg1_projection.npz; the records
    of the data set's own cut are the fixture's probabilities at the target's slot (to that file's TOL)."""
    from tests.test_host_projection import TOL, cfg1_bases, cfg1_data
    cx, fx, d, pd = projection_cfg1(), fixture(), cfg1_markov(), cfg1_data()
    V = cfg1_bases()["null_space"]
    assert V.shape == (1001, 2)
    rows = list(range(0, 1000, 25))
    there_and_back = d["paths"][0] + d["paths"][0][-2::-1]
    paths = [d["paths"][i] for i in rows] + [there_and_back]        # 40 walks and one that walks back over itself
    r, items, worst = check_projection_against_ref_predict(cx, V, paths)
    assert len(items) > 300 and worst < 1.0
    ptr, _ = ragged(paths)
    for n, i in enumerate(rows):
        t = int(ptr[n + 1]) - 2                                      # the node after the data set's prefix
        assert abs(np.exp(r["logp"][t]) - fx["probs_fwd"][i, pd["target"][i]]) <= TOL
    # back at the start every step has been undone: the coefficients of the last record hold the first step alone
    first = cx.B1[there_and_back[1], cx.at[tuple(sorted(there_and_back[:2]))]] * V[cx.at[tuple(sorted(there_and_back[:2]))]]
    assert abs(r["coef"][int(ptr[-1]) - 1] - first).max() <= 64 * U * r["absdot"].max()


# ------------------------------------------------------------------------------------------------------------------
# conventions of the records: short paths, min_prefix, offending pairs
# ------------------------------------------------------------------------------------------------------------------

def test_short_paths_and_min_prefix():
    from scone_gcn_amd import path_scores
    nbr, deg = markov_tiny4()
    c1, _ = ref_count(*ragged(TINY_WALKS), 1, nbr, deg)
    paths = [[], [2], [2, 0], [0, 1, 2, 3, 0, 2, 1]]
    ptr, nodes = ragged(paths)
    prob, rank, total, err = np_markov_path_scores(ptr, nodes, 1, 1.0, nbr, deg, c1)
    assert err == INT32_MAX and len(prob) == 10 and rank[[0, 1, 3]].tolist() == [-1, -1, -1] and rank[2] >= 0
    r = np_project_path_scores(projection_tiny4(), np.zeros((5, 0)), ptr, nodes)
    assert r["rank"][[0, 1, 3]].tolist() == [-1, -1, -1] and r["rank"][2] == 0 and r["coef"].shape == (10, 0)
    for min_prefix, want in ((1, [0, 0, 1, 6]), (2, [0, 0, 0, 5]), (5, [0, 0, 0, 2]), (0, [0, 0, 1, 6])):
        item_ptr, item_path, item_len = path_scores.path_items(ptr, min_prefix)
        assert np.diff(item_ptr).tolist() == want
        at = path_scores.item_positions(ptr, item_path, item_len)
        assert at.tolist() == [t for _, _, t in path_items(ptr, min_prefix)]
        assert (rank[at] >= 0).all()                                 # an item never lands on a record that predicts nothing


def test_bad_pair_lowers_err_to_the_first_and_blanks_exactly_its_windows():
    nbr, deg = markov_tiny4()
    walks = [[0, 1, 2, 0], [0, 1, 2, 1, 3, 2, 0, 1, 2], [2, 0, 7, 0, 1]]            # (1, 3) is no edge; 7 is no node
    ptr, nodes = ragged(walks)
    for order in (1, 2, 3):
        counts, _ = ref_count(*ragged(TINY_WALKS), order, nbr, deg)
        prob, rank, total, err = np_markov_path_scores(ptr, nodes, order, 1.0, nbr, deg, counts)
        assert err == 4 + 3                                          # walk 1, position 3
        blank = np.flatnonzero(rank < 0).tolist()
        # position 0 of every walk; then the records whose last `order` pairs hold (1, 3) at 7, (0, 7) at 14 or (7, 0) at 15
        want = {0, 4, 13} | {t for bad in (7, 14, 15) for t in range(bad + 1, bad + 1 + order)}
        assert blank == sorted(t for t in want if t < 18), order
        assert not prob[blank].any() and not total[blank].any() and (np.delete(prob, blank) > 0).all()
    cx = projection_tiny4()
    r = np_project_path_scores(cx, np.random.RandomState(0).randn(5, 2), ptr, nodes)
    assert r["err"] == 7
    assert np.flatnonzero(r["rank"] < 0).tolist() == [0, 4, 8, 9, 10, 11, 12, 13, 15, 16, 17]   # from the bad step to the path's end
    assert not r["coef"][8:13].any() and not r["logp"][15:].any()


# ------------------------------------------------------------------------------------------------------------------
# the surface that needs no device
# ------------------------------------------------------------------------------------------------------------------

def test_api_without_a_device():
    from scone_gcn_amd import _lib, path_scores
    from scone_gcn_amd.markov_model import Markov_Model, select_paths
    from scone_gcn_amd.projection_model import Projection_Model
    assert {"scn_markov_path_scores", "scn_project_path_scores"} <= set(_lib.SIGNATURES)
    mm, pm = Markov_Model(2), Projection_Model()
    for name in ("path_step_log_probs", "path_log_likelihood", "score_paths"):
        with pytest.raises(RuntimeError, match="train"):
            getattr(mm, name)([[0, 1, 2]])
        with pytest.raises(RuntimeError, match="embed"):
            getattr(pm, name)([[0, 1, 2]])
    for alpha in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            mm.path_step_log_probs([[0, 1, 2]], alpha=alpha)
    ptr, nodes = select_paths([[0, 1], [2], [3, 4, 5], []], [1, 0, 1, 1])
    assert ptr.tolist() == [0, 2, 5, 5] and nodes.tolist() == [0, 1, 3, 4, 5]
    ptr, nodes = select_paths((np.array([0, 2, 3]), np.array([7, 8, 9])), None)
    assert ptr.tolist() == [0, 2, 3] and nodes.tolist() == [7, 8, 9]
    sc = path_scores.PathScores(np.array([0, 2, 3]), np.log([0.5, 0.25, 0.5]), np.array([0, 1, 0]), np.zeros(3), np.array([2, 3, 2]))
    s = path_scores.summary(sc)
    assert s["n_steps"] == 3 and s["accuracy"] == 2.0 / 3.0 and abs(s["perplexity"] - 16.0 ** (1.0 / 3.0)) < 1e-12
    assert np.isnan(path_scores.summary(path_scores.PathScores(np.array([0]), np.zeros(0), np.zeros(0, np.int64), np.zeros(0),
                                                               np.zeros(0, np.int64)))["mean_step_logp"])


def test_n_unseen_and_mass_from_the_records():
    """What Markov_Model.path_step_log_probs / score_paths derive on the host from the records, on the restatement's records."""
    from scone_gcn_amd import path_scores
    from scone_gcn_amd.markov_model import Markov_Model
    nbr, deg = markov_tiny4()
    c2, _ = ref_count(*ragged(TINY_WALKS), 2, nbr, deg)
    paths = [[3, 0, 2, 1], [0, 1, 2, 3], [1]]
    ptr, nodes = ragged(paths)
    mm = Markov_Model(2)
    mm.counts, mm.h_nbr, mm.h_deg = "resident", nbr, deg            # (the device table is not touched: the records are handed in)
    for alpha, unseen, inf_mass in ((0.0, 4, 4), (1.0, 4, 0)):   # a short prefix, (3, 0), (0, 2) and a short one again
        rec = np_markov_path_scores(ptr, nodes, 2, alpha, nbr, deg, c2)[:3]
        mm._path_records = lambda *a, rec=rec: rec
        got = mm.score_paths(paths, min_prefix=1, alpha=alpha)
        sc = mm.path_step_log_probs(paths, min_prefix=1, alpha=alpha)
        assert got["n_steps"] == 6 and got["n_unseen"] == unseen and int(np.isinf(sc.mass).sum()) == inf_mass
        assert mm.path_totals.tolist() == [0, 0, 0, 0, 1, 2] and sc.prefix_len.tolist() == [1, 2, 3, 1, 2, 3]
        assert np.isfinite(got["mean_step_logp"]) == (alpha > 0)
        ll, n = mm.path_log_likelihood(paths, min_prefix=2, alpha=alpha)
        assert n.tolist() == [2, 2, 0] and ll[2] == 0.0
    with np.errstate(all="raise"):                                  # the log of a zero probability raises no warning
        mm.path_step_log_probs(paths, alpha=0.0)


def test_markov_alpha_flag_parses_without_a_default():
    from scone_gcn_amd import trajectory_experiments as te
    assert te.hyperparams(["prog", "-markov_alpha", "0.5"])["markov_alpha"] == 0.5
    assert "markov_alpha" not in te.hyperparams(["prog"])


def test_calls_answer_before_any_launch():
    from scone_gcn_amd import _lib
    lib = _lib.load()
    a = ctypes.c_double
    mk = lambda n, order, alpha, V=400, D=13: lib.scn_markov_path_scores(n, None, None, order, a(alpha), V, D, None, None, None, None, None,
                                                                        None, None, None)
    assert mk(3, 5, 0.0) == mk(3, 0, 0.0) == mk(3, 4, 0.0, 400, 200) == _lib.SCN_ERR_UNSUPPORTED
    assert mk(0, 2, 0.0) == 0 and mk(-1, 2, 0.0) == -2 and mk(3, 2, 0.0) == _lib.SCN_ERR_BAD_ARG
    assert mk(3, 2, -1.0) == mk(3, 2, float("nan")) == mk(0, 2, -0.5) == _lib.SCN_ERR_BAD_ARG
    pj = lambda n, k: lib.scn_project_path_scores(n, None, None, k, 5, None, 4, None, None, None, None, 3, None, None, None, None, None, None,
                                                  None, None)
    assert pj(3, 33) == pj(3, -1) == _lib.SCN_ERR_UNSUPPORTED and pj(0, 2) == 0 and pj(-1, 2) == -2 and pj(3, 2) == _lib.SCN_ERR_BAD_ARG
