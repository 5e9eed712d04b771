"""Teacher-forced path scoring (Scone_GCN.path_step_log_probs) without a GPU: this file's numpy restatement of the contracts of
scn_path_steps / scn_path_slabs / scn_path_score (include/scone_hip.h; tests/test_gpu_path_scores.py imports it as the reference of
the kernels) checked against brute force -- every item's column must be paths_to_flows of its prefix, ranks and masses come from plain
Python loops -- on the 4-node graph and on the 150-point data set; hand-made paths (a backtrack, a loop, short paths, min_prefix,
flips); the "flow" step-table rule against a dict walk; the -path_likelihood switch and the refusals."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import scone_oracle as so
from tests.test_host_multihop import _tiny4

INT32_MAX = (1 << 31) - 1


# ------------------------------------------------------------------------------------------------------------------
# the three contracts in numpy
# ------------------------------------------------------------------------------------------------------------------

def np_path_steps(ptr, nodes, deg, step_node, step_edge, step_sign, n_rows):
    """scn_path_steps: dict(slot, row, run, next_same [T], err)."""
    ptr, nodes = np.asarray(ptr, np.int64), np.asarray(nodes, np.int64)
    T, (V, d) = len(nodes), step_node.shape
    out = dict(slot=np.full(T, -1, np.int32), row=np.full(T, -1, np.int32), run=np.zeros(T, np.float32),
               next_same=np.full(T, INT32_MAX, np.int32), err=INT32_MAX)
    for p in range(len(ptr) - 1):
        t0, t1 = int(ptr[p]), int(ptr[p + 1])
        sign = {}
        for t in range(t0, t1 - 1):
            v, u = int(nodes[t]), int(nodes[t + 1])
            j = r = -1
            if 0 <= v < V and 0 <= u < V:
                hit = [c for c in range(min(max(int(deg[v]), 0), d)) if step_node[v, c] == u]
                if hit:
                    j, r = hit[0], int(step_edge[v, hit[0]])
                if r < 0 or r >= n_rows:
                    j = r = -1
            if j < 0:
                out["err"] = min(out["err"], t)
                continue
            out["slot"][t], out["row"][t], sign[t] = j, r, np.float32(step_sign[v, j])
        for t in sign:
            same = [q for q in sign if out["row"][q] == out["row"][t]]
            s = np.float32(0)
            for q in same:
                if q <= t:
                    s = np.float32(s + sign[q])
            out["run"][t] = s
            later = [q for q in same if q > t]
            if later:
                out["next_same"][t] = min(later)
    return out


def np_path_slabs(n_slabs, item_path, item_len, ptr, row, run, next_same, n_rows):
    """scn_path_slabs: x [n_slabs][n_rows][4][1] float32, and the number of writers of every word (never above one)."""
    x = np.zeros((n_slabs, n_rows, 4, 1), np.float32)
    writers = np.zeros((n_slabs, n_rows, 4), np.int64)
    for i, (p, k) in enumerate(zip(item_path, item_len)):
        t0 = int(ptr[p])
        end = t0 + int(k) - 1
        for t in range(t0, end):
            if row[t] >= 0 and next_same[t] >= end:
                x[i // 4, row[t], i % 4, 0] = run[t]
                writers[i // 4, row[t], i % 4] += 1
    assert writers.max(initial=0) <= 1
    return x


def comes_before(a, j, b, jb):
    """The order of scn_beam_step / scn_hop_select: a NaN before every number, then the higher value, then the lower slot."""
    if np.isnan(a):
        return j < jb if np.isnan(b) else True
    if np.isnan(b):
        return False
    return bool(a > b or (a == b and j < jb))


def np_path_score(item_path, item_len, ptr, nodes, slot, deg, logp):
    """scn_path_score: (step_logp float32, step_rank int32, step_mass float64 -- the fp64 value the fp32 kernel is held to)."""
    n, d = len(item_path), logp.shape[1]
    lp_out, rank, mass = np.full(n, np.nan, np.float32), np.full(n, -1, np.int32), np.full(n, np.nan, np.float64)
    for i, (p, k) in enumerate(zip(item_path, item_len)):
        t = int(ptr[p]) + int(k) - 1
        v, js = int(nodes[t]), int(slot[t])
        lim = min(max(int(deg[v]), 0), d) if 0 <= v < len(deg) else 0
        if js < 0 or js >= lim:
            continue
        row = logp[i]
        lp_out[i] = row[js]
        rank[i] = sum(1 for j in range(lim) if j != js and comes_before(row[j], j, row[js], js))
        best = 0
        for j in range(1, lim):
            if comes_before(row[j], j, row[best], best):
                best = j
        m = np.float64(row[best])
        with np.errstate(over="ignore", invalid="ignore"):
            mass[i] = m if not np.isfinite(m) else m + np.log(np.sum(np.exp(row[:lim].astype(np.float64) - m)))
    return lp_out, rank, mass


def same_floats(a, b):
    return a.dtype == b.dtype and np.array_equal(a.view(np.int32 if a.dtype == np.float32 else np.int64),
                                                 b.view(np.int32 if b.dtype == np.float32 else np.int64))


# ------------------------------------------------------------------------------------------------------------------
# brute force: an item's column is paths_to_flows of its prefix
# ------------------------------------------------------------------------------------------------------------------

def flow_tables(cx, nbrhoods, perm, flips=None):
    from scone_gcn_amd import multihop
    E_lookup = {(int(a), int(b)): k for k, (a, b) in enumerate(np.asarray(cx.edges).tolist())}
    return multihop.StepTables(nbrhoods, E_lookup, perm, "flow", torch.device("cpu"), flips)


def tab_arrays(tab):
    return tab.deg.numpy(), tab.node.numpy(), tab.edge.numpy(), tab.sign.numpy()


def check_columns(cx, nbrhoods, perm, paths, min_prefix, flips=None):
    """Every item of `paths` through the restatement; returns (steps, items, x)."""
    from scone_gcn_amd import path_scores
    from scone_gcn_amd import synthetic_data_gen as g
    from scone_gcn_amd.trajectory_experiments import apply_flips
    E = cx.n_edges
    deg, node, edge, sign = tab_arrays(flow_tables(cx, nbrhoods, perm, flips))
    ptr, nodes = path_scores.ragged(paths)
    st = np_path_steps(ptr, nodes, deg, node, edge, sign, E)
    assert st["err"] == INT32_MAX
    item_ptr, item_path, item_len = path_scores.path_items(ptr, min_prefix)
    M = len(item_path)
    S = (M + 3) // 4
    x = np_path_slabs(S, item_path, item_len, ptr, st["row"], st["run"], st["next_same"], E)
    cols = x[:, :, :, 0].transpose(0, 2, 1).reshape(S * 4, E)
    for i in range(M):
        prefix = list(paths[item_path[i]])[:item_len[i]]
        want = apply_flips(g.paths_to_flows(cx, [prefix]), flips).todense()[0, :, 0]
        assert np.array_equal(cols[i][perm], want), (i, prefix)
    assert not cols[M:].any()
    return st, (item_ptr, item_path, item_len), x


def tiny_complex():
    from scone_gcn_amd.synthetic_data_gen import Complex
    t = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny4_complex.npz"))
    cx = Complex(n_nodes=4, edges=np.asarray(t["edges"], np.int64), faces=np.asarray(t["faces"], np.int64))
    nb, _ = so.neighborhoods(cx.edges, 4)
    return cx, np.asarray(nb)


def random_walks(nb, rs, n, max_len):
    """Walks with backtracking and loops: every next node a uniform neighbour."""
    deg = (nb >= 0).sum(axis=1)
    out = []
    for _ in range(n):
        v = int(rs.randint(len(nb)))
        walk = [v]
        for _ in range(int(rs.randint(0, max_len))):
            v = int(nb[v][rs.randint(deg[v])])
            walk.append(v)
        out.append(walk)
    return out


@pytest.mark.parametrize("flip", [False, True])
def test_restatement_matches_brute_force_on_the_four_node_graph(flip):
    cx, nb = tiny_complex()
    rs = np.random.RandomState(5)
    perm = rs.permutation(cx.n_edges)
    flips = np.array([1.0, -1.0, 1.0, -1.0, -1.0]) if flip else None
    paths = random_walks(nb, rs, 40, 12)
    for min_prefix in (1, 2, 3):
        check_columns(cx, nb, perm, paths, min_prefix, flips)


@pytest.fixture(scope="module")
def data150(tmp_path_factory):
    from scone_gcn_amd import dataset_io, trajectory_experiments as te
    d = tmp_path_factory.mktemp("pathscores")
    cwd = os.getcwd()
    os.chdir(d)
    try:
        dataset_io.generate_dataset(150, 45, folder="ps", holes=True)
        out = te.data_setup(hops=(1, 2), folder_suffix="ps", hp=te.hyperparams(["prog"]))
    finally:
        os.chdir(cwd)
    return out


def test_restatement_matches_brute_force_on_the_150_point_data_set(data150):
    inputs_all, _, _, _, _, G, E_lookup, nbrhoods, _, targets_all, prefixes = data150
    sc = G.complex
    assert sc.cx.n_edges == 370 and sc.max_degree == 11
    assert 4 == min(map(len, prefixes[:11])) and max(map(len, prefixes[:11])) == 10
    paths = [list(p) + [int(t)] for p, t in zip(prefixes, targets_all[0])]
    perm = sc.layout.perm[1]
    assert not sc.layout.is_identity(1)
    st, (item_ptr, item_path, item_len), _ = check_columns(sc.cx, sc.nbrhoods, perm, paths[:11], 2)
    assert len(item_path) == 59
    check_columns(sc.cx, sc.nbrhoods, perm, paths, 1, sc.flip_vector(1))
    # rank and mass by plain loops, on a 0.25 grid so that ranks tie
    from scone_gcn_amd import path_scores
    rs = np.random.RandomState(6)
    ptr, nodes = path_scores.ragged(paths[:11])
    deg = (np.asarray(sc.nbrhoods) >= 0).sum(axis=1)
    logp = (-0.25 * rs.randint(0, 8, size=(59, 11))).astype(np.float32)
    lp, rank, mass = np_path_score(item_path, item_len, ptr, nodes, st["slot"], deg, logp)
    for i in range(59):
        p, k = item_path[i], item_len[i]
        v, u = paths[p][k - 1], paths[p][k]
        j = list(sc.nbrhoods[v]).index(u)
        assert lp[i] == logp[i, j]
        better = 0
        for c in range(deg[v]):
            if logp[i, c] > logp[i, j] or (logp[i, c] == logp[i, j] and c < j):
                better += 1
        assert rank[i] == better
        assert abs(mass[i] - math.log(sum(math.exp(float(a)) for a in logp[i, :deg[v]]))) <= 1e-12


def test_rank_and_mass_with_nan_and_infinities():
    cx, nb = tiny_complex()
    deg = (nb >= 0).sum(axis=1)                                                  # node 0 and node 2 have three neighbours
    ptr, nodes = np.array([0, 2]), np.array([0, 2])                               # one step 0 -> 2: slot 1 of node 0
    slot = np.array([1, -1])
    f = np.float32
    cases = [([0.0, np.nan, -1.0], 0, np.nan), ([np.nan, np.nan, 0.0], 1, np.nan), ([np.nan, -1.0, -1.0], 1, np.nan),
             ([np.inf, -1.0, -1.0], 1, np.inf), ([-np.inf] * 3, 1, -np.inf), ([-1.0, -1.0, -1.0], 1, -1.0 + math.log(3.0)),
             ([-np.inf, -2.0, -np.inf], 0, -2.0), ([-0.0, 0.0, 0.0], 1, math.log(3.0))]
    logp = np.array([c[0] + [9.0] for c in cases], f)                             # the padded slot is never read
    lp, rank, mass = np_path_score([0] * len(cases), [1] * len(cases), ptr, nodes, slot, deg, logp)
    for i, (_, want_rank, want_mass) in enumerate(cases):
        assert rank[i] == want_rank, i
        assert (np.isnan(want_mass) and np.isnan(mass[i])) or mass[i] == pytest.approx(want_mass, abs=1e-12), i
    # a prefix that ends its path has no slot: NaN / -1 / NaN
    lp, rank, mass = np_path_score([0], [2], ptr, nodes, slot, deg, logp[:1])
    assert np.isnan(lp[0]) and rank[0] == -1 and np.isnan(mass[0])


# ------------------------------------------------------------------------------------------------------------------
# hand-made paths
# ------------------------------------------------------------------------------------------------------------------

def test_backtrack_writes_an_explicit_zero():
    cx, nb = tiny_complex()
    perm = np.arange(5)
    paths = [[0, 1, 0, 1, 2]]
    st, (_, item_path, item_len), x = check_columns(cx, nb, perm, paths, 1)
    e01, e12 = 0, 3
    assert st["row"].tolist() == [e01, e01, e01, e12, -1] and st["slot"].tolist()[:4] == [0, 0, 0, 1]
    assert st["run"].tolist() == [1.0, 0.0, 1.0, 1.0, 0.0]                          # 1 -> 0 -> 1 on the one edge
    assert st["next_same"].tolist() == [1, 2, INT32_MAX, INT32_MAX, INT32_MAX]
    assert item_len.tolist() == [1, 2, 3, 4]
    assert [float(x[0, e01, i, 0]) for i in range(4)] == [0.0, 1.0, 0.0, 1.0]
    # the prefix 0, 1, 0: its writer on the edge is step 1 with the value 0 -- written, not skipped
    end = 0 + 3 - 1
    writers = [t for t in range(0, end) if st["next_same"][t] >= end]
    assert writers == [1] and st["run"][1] == 0.0


def test_an_edge_crossed_twice_the_same_way_counts_twice():
    cx, nb = tiny_complex()
    paths = [[0, 1, 2, 0, 1, 2], [2, 1, 0, 2, 1, 0]]
    st, (_, item_path, item_len), x = check_columns(cx, nb, np.arange(5), paths, 2)
    assert st["run"][3] == 2.0 and st["next_same"][0] == 3
    assert (item_path[3], item_len[3]) == (0, 5) and x[0, 0, 3, 0] == 2.0        # the prefix 0, 1, 2, 0, 1 holds 2 on the edge (0, 1)
    assert st["run"][6 + 3] == -2.0                                              # 2 -> 1 twice, against the orientation


def test_short_paths_and_min_prefix():
    from scone_gcn_amd import path_scores
    cx, nb = tiny_complex()
    paths = [[], [2], [0, 1], [0, 1, 2], [0, 1, 2, 3]]
    ptr, _ = path_scores.ragged(paths)
    for min_prefix, counts in ((0, [0, 0, 1, 2, 3]), (1, [0, 0, 1, 2, 3]), (2, [0, 0, 0, 1, 2]), (3, [0, 0, 0, 0, 1])):
        item_ptr, item_path, item_len = path_scores.path_items(ptr, min_prefix)
        assert np.diff(item_ptr).tolist() == counts
        assert all(item_len[item_ptr[p]:item_ptr[p + 1]].tolist() == list(range(max(min_prefix, 1), len(paths[p])))
                   for p in range(len(paths)))
        check_columns(cx, nb, np.arange(5), paths, min_prefix)
    st, _, x = check_columns(cx, nb, np.arange(5), paths, 1)
    assert not x[0, :, 0, 0].any()                                               # min_prefix 1: the first item of [0, 1] is the zero flow
    # the last position of every path is no step; an empty path owns no position
    assert st["slot"][[0, 2, 5, 9]].tolist() == [-1] * 4 and st["next_same"][[0, 2, 5, 9]].tolist() == [INT32_MAX] * 4


def test_flips_multiply_the_step():
    cx, nb = tiny_complex()
    flips = np.array([-1.0, 1.0, 1.0, -1.0, 1.0])
    st, _, _ = check_columns(cx, nb, np.arange(5), [[0, 1, 2, 3, 0]], 1, flips)
    assert st["run"].tolist()[:4] == [-1.0, -1.0, 1.0, -1.0]                      # +1 -1(flip) ; +1 * -1 ; +1 ; 3 -> 0 against


def test_bad_steps_lower_err_to_the_first_and_change_nothing_else():
    cx, nb = tiny_complex()
    deg, node, edge, sign = tab_arrays(flow_tables(cx, nb, np.arange(5)))
    good = np_path_steps([0, 3, 6], [0, 1, 2, 2, 3, 0], deg, node, edge, sign, 5)
    bad = np_path_steps([0, 3, 6], [0, 1, 3, 2, 7, 0], deg, node, edge, sign, 5)      # 1 -> 3 is no edge; 7 is no node
    assert good["err"] == INT32_MAX and bad["err"] == 1
    assert bad["slot"].tolist() == [0, -1, -1, -1, -1, -1] and bad["row"][0] == good["row"][0]
    assert np_path_steps([0, 3], [0, 1, 2], deg, node, edge, sign, 3)["err"] == 1      # row 3 of edge (1, 2) lies outside 3 rows


# ------------------------------------------------------------------------------------------------------------------
# the "flow" rule of the step tables, the switch and the refusals
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flip", [False, True])
def test_flow_step_tables_match_a_dict_walk(flip):
    from scone_gcn_amd import multihop
    from scone_gcn_amd import synthetic_data_gen as g
    from scone_gcn_amd.complex import SimplicialComplex
    sc = SimplicialComplex(g.random_SC_graph(60))
    cx, perm = sc.cx, sc.layout.perm[1]
    assert not sc.layout.is_identity(1)
    flips = sc.flip_vector(1) if flip else None
    E_lookup = {(int(a), int(b)): k for k, (a, b) in enumerate(cx.edges.tolist())}
    c, d = (int(v) for v in cx.edges[7])
    del E_lookup[(c, d)]                                                         # a pair without an edge: the sentinel on both sides
    nb = np.asarray(sc.nbrhoods)
    tab = multihop.StepTables(nb, E_lookup, perm, "flow", torch.device("cpu"), flips)
    V, D = nb.shape
    for v in range(V):
        for j in range(D):
            u = int(nb[v, j])
            assert tab.h_node[v, j] == u                                         # slots as the readout numbers them
            k = E_lookup.get((min(v, u), max(v, u))) if u >= 0 else None
            if k is None:
                assert tab.edge[v, j] == -1 and tab.sign[v, j] == 0
            else:
                assert tab.edge[v, j] == perm[k]
                assert tab.sign[v, j] == (1.0 if v < u else -1.0) * (flips[k] if flip else 1.0)
    assert np.array_equal(tab.deg.numpy(), (nb >= 0).sum(axis=1))
    assert tab.edge[c, list(nb[c]).index(d)] == -1 and tab.edge[d, list(nb[d]).index(c)] == -1


def test_interior_padding_is_refused():
    from scone_gcn_amd import multihop
    cx, nb = tiny_complex()
    E_lookup = {(int(a), int(b)): k for k, (a, b) in enumerate(cx.edges.tolist())}
    holed = nb.copy()
    holed[0, 0], holed[0, 1] = -1, nb[0, 0]
    with pytest.raises(ValueError, match="left-aligned"):
        multihop.StepTables(holed, E_lookup, np.arange(5), "flow", torch.device("cpu"))
    multihop.StepTables(holed, E_lookup, np.arange(5), "dist", torch.device("cpu"))     # the tree's rule re-aligns such a table
    with pytest.raises(ValueError, match="rule"):
        multihop.StepTables(nb, E_lookup, np.arange(5), "flows", torch.device("cpu"))


def test_probed_closure_is_refused():
    from scone_gcn_amd.scone_trajectory_model import Scone_GCN
    net = Scone_GCN(1, 1e-3, 4, 0.0, verbose=False)
    net.model_type = "scone"
    B1, B2, edges, E_lookup = _tiny4()
    nb, _ = so.neighborhoods(edges, 4)
    inputs = [so.make_Bconds(B1, nb), np.array([1]), np.zeros((1, 5, 1))]
    for call in (net.path_step_log_probs, net.path_log_likelihood, net.score_paths):
        with pytest.raises(TypeError, match="Bconds"):
            call(inputs, [[0, 1, 2]])


def test_path_likelihood_switch_parses():
    from scone_gcn_amd import trajectory_experiments as te
    assert te.hyperparams(["prog"])["path_likelihood"] == 0
    assert te.hyperparams(["prog", "-path_likelihood", "1"])["path_likelihood"] == 1


def test_segment_sums_handle_empty_paths():
    from scone_gcn_amd import path_scores
    got = path_scores.segment_sums(np.array([1.0, 2.0, 4.0, 8.0]), np.array([0, 0, 2, 2, 3, 4, 4]))
    assert got.tolist() == [0.0, 3.0, 0.0, 4.0, 8.0, 0.0]
    assert path_scores.segment_sums(np.zeros(0), np.array([0, 0, 0])).tolist() == [0.0, 0.0]
