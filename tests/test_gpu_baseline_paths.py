"""Whole-path scores of the Markov and projection baselines on the device (scn_markov_path_scores, scn_project_path_scores through
Markov_Model and Projection_Model) against the NumPy restatements of tests/test_host_baseline_paths.py and against the per-prefix
calls they replace (next_node_probs, predict_all), on walks at the tile edges of both kernels -- 2, order, order + 1, 63, 64, 65, 66,
128 and 129 nodes, and one ragged batch -- on the four-node graph, the 400-point cfg1 complex and a wheel with a pendant node (a
neighbourhood wider than a wave, a node of degree 1); then the errors, the empty calls and the driver's switches.

What is compared how.  Markov: prob, rank and total bitwise -- the quotient's operations are rounded one by one on the device as in
NumPy, so this holds for every alpha; for a non-dyadic alpha (0.1), where a denominator fused into one multiply-add would differ
by an ulp, the contract allows 1 ulp: that is asserted, and then that the kernel meets it with 0.  Projection: coef bitwise (a
chain of additions of +-V entries in a fixed order); logp and mass within SAFETY times the forward bound computed from the data
(tests/test_host_baseline_paths.py: record_bound, SAFETY) -- the device fuses the products of the dot product, NumPy does not,
predict_all sums V^T f over the flow's edges, and exp / log are the device's; rank exactly wherever the taken logit is further than
SAFETY times the logits' bound from every other real neighbour's, and no item of these inputs is closer.  One kind of item has
all its logits tied and is still compared exactly: where the coefficients -- already checked bitwise -- are exactly 0 (no basis, no
step before it, or a walk that has just undone all its steps: a, b, a), every logit is a product with 0 on both sides and no
rounding can move the rank off the slot taken.  On the four-node graph that rank check runs on a basis rounded to 2^-20 and the
rounding checks run again on the unrounded one (gaussian_basis says why).  The records beside an offending pair, which the Python
classes never hand out (they raise), are read through the C-ABI, with the pair in the first, the second and a middle pass.  The
largest error / bound ratios are printed (profiles/baseline_path_scores.txt quotes them)."""
import functools

import numpy as np
import pytest

from tests.test_host_baseline_paths import (SAFETY, U, logit_bound, np_markov_path_scores, np_project_path_scores, path_items,
                                            random_walks, record_bound)
from tests.test_host_markov import INT32_MAX, ragged, slot, table_from_edges
from tests.test_host_projection import Cx, wheel70
from tests.test_host_projection import cfg1 as projection_cfg1
from tests.test_host_projection import tiny4 as projection_tiny4

pytestmark = pytest.mark.gpu

EDGE_LENGTHS = (2, 63, 64, 65, 66, 128, 129)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@functools.lru_cache(None)
def spiky():
    """tests/test_host_projection.py's wheel (hub 0 with 70 neighbours, two holes) with the pendant node 71 at rim node 1."""
    w = wheel70()
    return Cx(72, w.edges.tolist() + [(1, 71)], w.faces.tolist())


@functools.lru_cache(None)
def graph(name):
    """(Cx, nbr int32, deg int32) of the three test graphs."""
    cx = {"tiny4": projection_tiny4, "cfg1": projection_cfg1, "spiky": spiky}[name]()
    nbr, deg = table_from_edges(cx.n_nodes, cx.edges)
    assert np.array_equal(nbr, cx.nbr) and np.array_equal(deg, cx.deg)
    return cx, nbr, deg


@functools.lru_cache(None)
def walks_of(name, order):
    """Seeded walks with revisits at the tile edges, a ragged batch of one long walk among short ones, and the training walks."""
    cx, nbr, deg = graph(name)
    rs = np.random.RandomState(100 + order)
    edge = random_walks(nbr, deg, rs, EDGE_LENGTHS + (order, order + 1))
    ragged_batch = random_walks(nbr, deg, rs, [3] * 40 + [129] + [3] * 40 + [1, 0, 2])
    train = random_walks(nbr, deg, rs, [40] * 60) + edge[:4]
    return edge, ragged_batch, train


@functools.lru_cache(None)
def markov(name, order):
    from scone_gcn_amd.markov_model import Markov_Model
    _, nbr, deg = graph(name)
    mm = Markov_Model(order)
    mm.train(nbr, walks_of(name, order)[2])
    counts = mm.counts.cpu().numpy()
    counts.setflags(write=False)
    return mm, counts


MARKOV_CASES = [("tiny4", k) for k in (1, 2, 3, 4)] + [("cfg1", k) for k in (1, 2, 3)] + [("spiky", 1), ("spiky", 2)]


@pytest.mark.parametrize("name,order", MARKOV_CASES)
def test_markov_records_are_the_restatement_bitwise(name, order):
    _, nbr, deg = graph(name)
    mm, counts = markov(name, order)
    edge, ragged_batch, _ = walks_of(name, order)
    for paths in (edge, ragged_batch):
        ptr, nodes = ragged(paths)
        for alpha in (0.0, 0.25, 1.0, 0.1):
            want = np_markov_path_scores(ptr, nodes, order, alpha, nbr, deg, counts)
            assert want[3] == INT32_MAX
            prob, rank, total = mm._path_records(ptr, nodes, alpha)
            assert np.array_equal(rank, want[1]) and np.array_equal(total, want[2])
            off = np.abs(bits(prob) - bits(want[0])).max()
            # 0.1 is not dyadic: alpha * deg and the sums round, and a denominator formed by one fused multiply-add would differ from
            # NumPy's by an ulp, hence the allowance of 1 ulp there.  The kernel rounds every operation on its own.
            assert off <= (1 if alpha == 0.1 else 0), (alpha, off)
            assert off == 0
        if paths is edge:
            assert (want[2] > 0).sum() > 10                          # seen states among them, not only the uniform fallback


@pytest.mark.parametrize("name,order", [("tiny4", 1), ("tiny4", 4), ("cfg1", 2), ("cfg1", 3), ("spiky", 2)])
def test_markov_alpha0_is_next_node_probs_of_every_prefix(name, order):
    from scone_gcn_amd import path_scores
    _, nbr, deg = graph(name)
    mm, _ = markov(name, order)
    paths = list(walks_of(name, order)[0])
    ptr, nodes = ragged(paths)
    items = path_items(ptr, 1)
    probs = mm.next_node_probs([paths[p][:k] for p, k, _ in items])
    want = np.asarray([probs[i, slot(nbr, deg, paths[p][k - 1], paths[p][k])] for i, (p, k, _) in enumerate(items)])
    prob, _, total = mm._path_records(ptr, nodes, 0.0)
    at = [t for _, _, t in items]
    assert np.array_equal(bits(prob[at]), bits(want))
    sc = mm.path_step_log_probs(paths, min_prefix=1)
    assert isinstance(sc, path_scores.PathScores) and np.array_equal(sc.ptr, np.cumsum([0] + [max(len(p) - 1, 0) for p in paths]))
    with np.errstate(divide="ignore"):
        assert np.array_equal(bits(sc.logp), bits(np.log(want)))
    assert np.array_equal(np.isinf(sc.mass), total[at] == 0) and np.array_equal(mm.path_totals, total[at])
    got = mm.score_paths((ptr, nodes), min_prefix=2, alpha=0.5)
    sc2 = mm.path_step_log_probs(paths, min_prefix=2, alpha=0.5)
    assert got["n_steps"] == len(sc2.logp) == sum(max(len(p) - 2, 0) for p in paths) and np.isfinite(got["mean_step_logp"])
    assert got["n_unseen"] == int((mm.path_totals == 0).sum()) and got["accuracy"] == float(np.mean(sc2.rank == 0))
    ll, n = mm.path_log_likelihood(paths, min_prefix=2, alpha=0.5)
    assert np.array_equal(n, np.diff(sc2.ptr)) and abs(ll.sum() - sc2.logp.sum()) <= 1e-9 * abs(sc2.logp.sum())


# ------------------------------------------------------------------------------------------------------------------
# projection
# ------------------------------------------------------------------------------------------------------------------

def gaussian_basis(name, dim, rounded):
    """A seeded Gaussian V (the kernel does not care whether it is harmonic), as it is or rounded to multiples of 2^-20.  A long
    walk on the four-node graph's five edges undoes itself again and again (net flow 0); what an unrounded Gaussian sum leaves
    behind there -- coefficients of 1e-16 -- puts every logit of the item inside the rounding bound, whatever the walks' seed.
    Sums of the rounded entries are exact, so such an item has coefficients of exactly 0 and its rank is decided.  The rounded
    basis therefore carries the rank check on that graph; the unrounded one is checked there as well, for the order of the sums
    and the rounding of coef, logp and mass (test_projection_rounding_on_the_four_node_graph), and alone on the other graphs."""
    cx, _, _ = graph(name)
    V = np.random.RandomState(7 + dim).randn(cx.E, dim)
    return np.round(V * 2.0 ** 20) / 2.0 ** 20 if rounded else V


@functools.lru_cache(None)
def projection(name, dim, rounded):
    from scone_gcn_amd.projection_model import Projection_Model
    cx, _, _ = graph(name)
    V = gaussian_basis(name, dim, rounded)
    return Projection_Model.from_basis(V, cx.B1), V


RATIOS = {}


def check_projection(name, dim, paths, against_predict_all, rounded=None, every_rank_decided=True):
    cx, nbr, deg = graph(name)
    rounded = name == "tiny4" if rounded is None else rounded
    pm, V = projection(name, dim, rounded)
    ptr, nodes = ragged(paths)
    want = np_project_path_scores(cx, V, ptr, nodes)
    assert want["err"] == INT32_MAX
    _, _, logp, rank, mass, coef = pm.path_records(paths, with_coef=True)
    assert coef.shape == (len(nodes), dim) and np.array_equal(bits(coef), bits(want["coef"]))
    items = path_items(ptr, 1)
    if against_predict_all:
        from scone_gcn_amd.synthetic_data_gen import Complex, paths_to_flows
        prefixes = [paths[p][:k] for p, k, _ in items]
        flows = paths_to_flows(Complex(n_nodes=cx.n_nodes, edges=cx.edges, faces=cx.faces), prefixes)
        probs, logits, _ = pm.predict_all(flows, [pre[-1] for pre in prefixes])
    worst = {"restatement": 0.0, "predict_all": 0.0, "logits": 0.0}
    left_out = 0
    for i, (p, k, t) in enumerate(items):
        a, b = paths[p][k - 1], paths[p][k]
        j, dv = slot(nbr, deg, a, b), int(deg[a])
        tol = SAFETY * record_bound(want, t, k - 1, dim, cx.D)
        tol_logit = SAFETY * logit_bound(want, t, k - 1, dim)
        ratio = {"restatement": max(abs(logp[t] - want["logp"][t]), abs(mass[t] - want["mass"][t])) / tol}
        if against_predict_all:
            ratio["predict_all"] = max(abs(logp[t] - np.log(probs[i, j])), abs(mass[t] - np.log(probs[i, :dv].sum()))) / tol
            off = abs(logits[i] - want["logits"][t]).max()           # predict_all's logits: the only ones the device hands out
            assert off <= tol_logit, (p, k, off, tol_logit)
            ratio["logits"] = off / tol_logit if tol_logit else 0.0
        for key, e in ratio.items():
            worst[key] = max(worst[key], e)
        lg = want["logits"][t]
        gap = np.abs(np.delete(lg[:dv], j) - lg[j]).min() if dv > 1 else np.inf
        if gap > tol_logit or not want["coef"][t].any():             # (see the docstring: coefficients of exactly 0, both sides exact)
            assert rank[t] == want["rank"][t], (p, k)
        else:
            left_out += 1
        if dim == 0:
            assert rank[t] == j and abs(logp[t] + np.log(cx.D)) <= 4 * U * np.log(cx.D)
    print("projection %s dim %d%s: %d items, %d inside the rank bound, largest error / (SAFETY x bound): %s"
          % (name, dim, " (rounded basis)" if rounded else "", len(items), left_out, worst))
    RATIOS[(name, dim, rounded)] = worst
    assert max(worst.values()) <= 1.0, worst
    if every_rank_decided:
        assert left_out == 0                                         # no item of these inputs is inside the bound
    first = ptr[:-1][np.diff(ptr) > 0]
    assert not logp[first].any() and (rank[first] == -1).all() and not mass[first].any() and not coef[first].any()


@pytest.mark.parametrize("dim", (0, 1, 2, 32))
@pytest.mark.parametrize("name", ("tiny4", "cfg1"))
def test_projection_records_at_the_tile_edges(name, dim):
    edge, ragged_batch, _ = walks_of(name, 3)
    check_projection(name, dim, edge, against_predict_all=True)
    check_projection(name, dim, ragged_batch, against_predict_all=False)


@pytest.mark.parametrize("dim", (1, 2, 32))
def test_projection_rounding_on_the_four_node_graph(dim):
    """The unrounded Gaussian basis on the four-node graph: coef bitwise, logp and mass within the bound, through every
    cancellation of its long walks.  The ranks of the items whose walk has just cancelled are not decided here (see
    gaussian_basis); every other rank is compared."""
    edge, ragged_batch, _ = walks_of("tiny4", 3)
    check_projection("tiny4", dim, edge, against_predict_all=True, rounded=False, every_rank_decided=False)
    check_projection("tiny4", dim, ragged_batch, against_predict_all=False, rounded=False, every_rank_decided=False)


@pytest.mark.parametrize("dim", (0, 2))
def test_projection_at_the_widest_neighbourhood_and_at_degree_one(dim):
    cx, nbr, deg = graph("spiky")
    assert deg[0] == 70 == cx.D and deg[71] == 1
    paths = [[71, 1, 0, 5, 0, 70, 1, 71, 1, 2], [0, 33], [71, 1]] + random_walks(nbr, deg, np.random.RandomState(4), [66, 9], start=0)
    check_projection("spiky", dim, paths, against_predict_all=True)


def test_markov_at_the_widest_neighbourhood_and_at_degree_one():
    _, nbr, deg = graph("spiky")
    mm, counts = markov("spiky", 2)
    paths = [[71, 1, 0, 5, 0, 70, 1, 71, 1, 2], [0, 33], [71, 1]] + walks_of("spiky", 2)[2][:3]
    ptr, nodes = ragged(paths)
    want = np_markov_path_scores(ptr, nodes, 2, 1.0, nbr, deg, counts)
    prob, rank, total = mm._path_records(ptr, nodes, 1.0)
    assert np.array_equal(bits(prob), bits(want[0])) and np.array_equal(rank, want[1]) and np.array_equal(total, want[2])
    assert prob[1] == 1.0 and rank[1] == 0                           # out of the pendant node there is one way
    assert rank.max() > 40                                           # ranks past one wave's worth of slots at the hub


def test_projection_model_surface():
    from scone_gcn_amd import path_scores
    pm, _ = projection("cfg1", 2, False)
    paths = list(walks_of("cfg1", 3)[0])
    _, _, logp, rank, mass, coef = pm.path_records(paths)
    assert coef is None
    for min_prefix in (1, 2, 5):
        sc = pm.path_step_log_probs(paths, min_prefix=min_prefix)
        ptr, _ = ragged(paths)
        at = [t for _, _, t in path_items(ptr, min_prefix)]
        assert isinstance(sc, path_scores.PathScores) and np.array_equal(sc.logp, logp[at]) and np.array_equal(sc.rank, rank[at])
        assert np.array_equal(sc.prefix_len, [k for _, k, _ in path_items(ptr, min_prefix)])
        norm = pm.path_step_log_probs(paths, min_prefix=min_prefix, normalise=True)
        assert np.array_equal(norm.logp, logp[at] - mass[at]) and np.array_equal(norm.mass, mass[at])
    assert (mass < 0).any() and (mass <= 0).all()                    # the padding slots take probability wherever deg < D
    mask = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1])
    got = pm.score_paths(paths, mask)
    sub = pm.path_step_log_probs([p for p, m in zip(paths, mask) if m])
    assert got == path_scores.summary(sub) and got["n_steps"] == len(sub.logp) > 100
    ll, n = pm.path_log_likelihood(paths)
    full = pm.path_step_log_probs(paths)
    assert np.array_equal(n, np.diff(full.ptr)) and np.array_equal(ll, path_scores.segment_sums(full.logp, full.ptr))
    again = pm.path_records(ragged(paths), with_coef=True)           # the (ptr, nodes) form, and the same bytes on a second call
    assert np.array_equal(bits(again[2]), bits(logp)) and np.array_equal(again[3], rank)


# ------------------------------------------------------------------------------------------------------------------
# errors and limits
# ------------------------------------------------------------------------------------------------------------------

def raw_markov(mm, ptr, nodes, alpha):
    """scn_markov_path_scores through the C-ABI: the records as the kernel left them (Markov_Model raises instead), and err."""
    import ctypes
    import torch
    from scone_gcn_amd import _lib, ops
    T = len(nodes)
    d_ptr, d_nodes = torch.from_numpy(ptr).cuda(), torch.from_numpy(nodes).cuda()
    prob = torch.full((T,), -7.0, dtype=torch.float64, device="cuda")
    rank, total = (torch.full((T,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    err = torch.full((1,), INT32_MAX, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = _lib.load().scn_markov_path_scores(len(ptr) - 1, p(d_ptr), p(d_nodes), mm.order, ctypes.c_double(alpha), *mm._graph_args(),
                                            p(mm.counts), p(prob), p(rank), p(total), p(err), ops._stream())
    assert st == 0
    return prob.cpu().numpy(), rank.cpu().numpy(), total.cpu().numpy(), int(err.item())


def raw_project(pm, ptr, nodes):
    """scn_project_path_scores through the C-ABI: (logp, rank, mass, coef, err) as the kernel left them."""
    import ctypes
    import torch
    from scone_gcn_amd import _lib, ops
    T, k = len(nodes), pm.dim
    d_ptr, d_nodes = torch.from_numpy(ptr).cuda(), torch.from_numpy(nodes).cuda()
    logp, mass = (torch.full((T,), -7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    coef = torch.full((T, k), -7.0, dtype=torch.float64, device="cuda")
    rank = torch.full((T,), -7, dtype=torch.int32, device="cuda")
    err = torch.full((1,), INT32_MAX, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    t = pm._tab
    st = _lib.load().scn_project_path_scores(len(ptr) - 1, p(d_ptr), p(d_nodes), k, pm.n_edges, p(pm._V), pm.n_nodes, p(t[0]), p(t[1]),
                                             p(t[2]), p(t[3]), pm.width, p(t[4]), p(t[5]), p(logp), p(rank), p(mass), p(coef), p(err),
                                             ops._stream())
    assert st == 0
    return logp.cpu().numpy(), rank.cpu().numpy(), mass.cpu().numpy(), coef.cpu().numpy(), int(err.item())


def walks_with_late_bad_pairs():
    """Walks round the triangle 0, 1, 2 of the four-node graph that step from 1 to 3 -- no edge -- in their second pass of 64
    positions: at the pair 70 (inside the pass), at the pair 63 (the first pair the second pass owns) and at the pair 127 of a walk
    of 200 nodes (a third pass follows the offending one), a clean walk between them; and an id outside the graph."""
    def walk(start, n, bad_at):
        w = [(start + i) % 3 for i in range(n)]
        assert w[bad_at] == 1
        return w[:bad_at + 1] + [3] + [(2 + i) % 3 for i in range(n - bad_at - 2)]       # ... 1, 3, 2, 0, 1, ...
    return [walk(0, 140, 70), [0, 1, 2, 0, 3, 2], walk(1, 130, 63), walk(0, 200, 127), [2, 0, 9, 0, 1]]


@pytest.mark.parametrize("order", (1, 2, 3, 4))
def test_markov_records_beside_offending_pairs_in_every_pass(order):
    _, nbr, deg = graph("tiny4")
    mm, counts = markov("tiny4", order)
    paths = walks_with_late_bad_pairs()
    ptr, nodes = ragged(paths)
    want = np_markov_path_scores(ptr, nodes, order, 1.0, nbr, deg, counts)
    prob, rank, total, err = raw_markov(mm, ptr, nodes, 1.0)
    assert err == want[3] == 70
    assert np.array_equal(bits(prob), bits(want[0])) and np.array_equal(rank, want[1]) and np.array_equal(total, want[2])
    blank = set(np.flatnonzero(rank < 0).tolist())
    starts = ptr[:-1].tolist()
    bad = [70, starts[2] + 63, starts[3] + 127, starts[4] + 1, starts[4] + 2]
    assert blank == set(starts) | {t for r in bad for t in range(r + 1, r + 1 + order) if t < len(nodes)}
    assert not prob[sorted(blank)].any() and not total[sorted(blank)].any()
    # the first offending pair alone, when the earlier walks are left out
    assert raw_markov(mm, *ragged(paths[2:]), 1.0)[3] == 63 and raw_markov(mm, *ragged(paths[3:]), 1.0)[3] == 127


@pytest.mark.parametrize("dim", (0, 2, 32))
def test_projection_records_behind_a_step_that_is_no_edge_in_every_pass(dim):
    cx, _, _ = graph("tiny4")
    pm, V = projection("tiny4", dim, True)
    paths = walks_with_late_bad_pairs()
    ptr, nodes = ragged(paths)
    want = np_project_path_scores(cx, V, ptr, nodes)
    logp, rank, mass, coef, err = raw_project(pm, ptr, nodes)
    assert err == want["err"] == 70
    assert np.array_equal(rank, want["rank"]) and np.array_equal(bits(coef), bits(want["coef"]))
    starts = ptr.tolist()
    blank = set(starts[:-1])
    for p, r in ((0, 70), (2, 63), (3, 127), (4, 1)):                # from the step that is no edge to the end of its path
        blank |= set(range(starts[p] + r + 1, starts[p + 1]))
    assert set(np.flatnonzero(rank < 0).tolist()) == blank
    for a in (logp, mass, coef):
        assert not a[sorted(blank)].any()
    live = np.flatnonzero(rank >= 0)
    at = np.searchsorted(ptr, live, side="right") - 1             # the record at position q of its path has q - 1 steps behind it
    tol = np.asarray([SAFETY * record_bound(want, t, t - int(ptr[p]) - 1, dim, cx.D) for t, p in zip(live, at)])
    assert (np.abs(logp[live] - want["logp"][live]) <= tol).all() and (np.abs(mass[live] - want["mass"][live]) <= tol).all()


def test_bad_pairs_raise_and_change_nothing():
    _, nbr, deg = graph("tiny4")
    mm, counts = markov("tiny4", 2)
    pm, _ = projection("tiny4", 2, True)
    good = [[0, 1, 2, 0, 3], [2, 3]]
    before = (mm._path_records(*ragged(good), 1.0), pm.path_records(good, with_coef=True)[2:])
    late = walks_with_late_bad_pairs()
    for bad, where in (([[0, 1, 2], [0, 1, 3, 2], [1, 3]], "path 1, position 1"), ([[2, 0, 7, 0, 1]], "path 0, position 1"),
                       ([[0, 1], [3, -1, 0]], "path 1, position 0"), (late[1:], "path 1, position 63"),
                       ([late[1], late[3]], "path 1, position 127")):
        with pytest.raises(ValueError, match=where):
            mm.path_step_log_probs(bad, alpha=1.0)
        with pytest.raises(ValueError, match=where):
            pm.path_step_log_probs(bad)
    after = (mm._path_records(*ragged(good), 1.0), pm.path_records(good, with_coef=True)[2:])
    for a, b in zip(before[0] + before[1], after[0] + after[1]):
        assert np.array_equal(a, b)
    assert np.array_equal(mm.counts.cpu().numpy(), counts)


def test_empty_calls():
    mm, _ = markov("tiny4", 2)
    pm, _ = projection("tiny4", 2, True)
    for model in (mm, pm):
        for paths in ([], [[], []], [[2]], [[], [1], [3]]):
            sc = model.path_step_log_probs(paths, min_prefix=1)
            assert len(sc.ptr) == len(paths) + 1 and not sc.ptr.any() and len(sc.logp) == len(sc.rank) == len(sc.mass) == 0
            assert np.isnan(model.score_paths(paths)["mean_step_logp"])
            ll, n = model.path_log_likelihood(paths)
            assert not ll.any() and not n.any() and len(ll) == len(paths)
    with pytest.raises(ValueError, match="alpha"):
        mm.score_paths([[0, 1]], alpha=-1.0)


# ------------------------------------------------------------------------------------------------------------------
# the driver
# ------------------------------------------------------------------------------------------------------------------

def test_train_model_scores_the_baselines_beside_the_model(tmp_path, monkeypatch):
    """-path_likelihood 1 with and without -markov 1 -projection 1.  The Markov experiments draw one shuffle from the trainer's
    stream before the weights are initialised (as they always have), so the second run hands the stream back as it found it:
    both runs then train the same model, and what the baselines add must leave the model's own scores as they were."""
    from scone_gcn_amd import dataset_io, scone_trajectory_model as stm, trajectory_experiments as te
    monkeypatch.chdir(tmp_path)
    dataset_io.generate_dataset(150, 45, folder="drv", holes=True)
    argv = ["prog", "-epochs", "1", "-batch_size", "12", "-data_folder_suffix", "drv", "-describe", "0", "-path_likelihood", "1"]

    def run(extra):
        hp = te.hyperparams(argv + extra)
        hp["hidden_layers"] = [(3, 16)] * 3
        stm.reseed(1030)
        return te.train_model(hp)[0].experiment_results
    alone = run([])
    assert "path_likelihood_markov" not in alone and "path_likelihood_projection" not in alone
    experiments = te.markov_experiments

    def same_stream(*a, **k):
        state = stm._RNG.get_state()
        try:
            return experiments(*a, **k)
        finally:
            stm._RNG.set_state(state)
    monkeypatch.setattr(te, "markov_experiments", same_stream)
    both = run(["-markov", "1", "-projection", "1"])
    stm.reseed(1030)
    assert both["path_likelihood"] == alone["path_likelihood"] and set(both["path_likelihood"]) == {"train", "test"}
    for key in ("path_likelihood_markov", "path_likelihood_projection"):
        assert set(both[key]) == {"train", "test"}
        for name in ("train", "test"):
            r = both[key][name]
            assert np.isfinite(r["mean_step_logp"]) and r["mean_step_logp"] < 0 and 0 <= r["accuracy"] <= 1
            assert r["n_steps"] == both["path_likelihood"][name]["n_steps"] > 0          # the same items
    assert both["path_likelihood_markov"]["train"]["n_unseen"] == 0                       # order 1 on its own training paths
    assert "markov" in both and "projection" in both
    # the Markov figures are those of a table of the train mask's paths at the default alpha = 1, and -markov_alpha reaches it
    from scone_gcn_amd.markov_model import Markov_Model
    quarter = run(["-markov", "1", "-markov_alpha", "0.25"])
    stm.reseed(1030)
    assert "path_likelihood_projection" not in quarter and quarter["path_likelihood"] == alone["path_likelihood"]
    hp = te.hyperparams(argv)
    _, _, train_mask, test_mask, _, G, _, _, _, targets_all, prefixes = te.data_setup(hops=(1, 2), folder_suffix="drv", hp=hp)
    paths = [[int(v) for v in p] + [int(t)] for p, t in zip(prefixes, targets_all[0])]
    mm = Markov_Model(1)
    mm.train(G, [paths[i] for i in np.flatnonzero(np.asarray(train_mask) == 1)])
    for res, alpha in ((both, 1.0), (quarter, 0.25)):
        for name, mask in (("train", train_mask), ("test", test_mask)):
            assert res["path_likelihood_markov"][name] == mm.score_paths(paths, mask, alpha=alpha)
    assert both["path_likelihood_markov"]["test"]["mean_step_logp"] != quarter["path_likelihood_markov"]["test"]["mean_step_logp"]
