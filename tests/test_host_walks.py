"""The host statement of the batched shortest paths (synthetic_data_gen.shortest_path_tree_host) against scipy, the batched walk
generator on its host backend, and the flags that reach it.  No GPU."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import dijkstra

from scone_gcn_amd import dataset_io
from scone_gcn_amd import synthetic_data_gen as g
from scone_gcn_amd import trajectory_experiments as te

HERE = os.path.dirname(os.path.abspath(__file__))
METRICS = ["hops", "euclid"]


@pytest.fixture(scope="module")
def cx():
    d = np.load(os.path.join(HERE, "golden", "cfg1_complex.npz"))
    return g.Complex(n_nodes=int(d["n_nodes"]), edges=d["edges"].astype(np.int64), faces=d["faces"].astype(np.int64),
                     coords=d["coords"], valid_idxs=d["valid_idxs"].astype(np.int64))


def _scipy_graph(graph):
    adj_ptr, adj, adj_w = graph
    n = len(adj_ptr) - 1
    return sp.csr_matrix((np.ones(len(adj)) if adj_w is None else adj_w, adj.astype(np.int64), adj_ptr.astype(np.int64)), shape=(n, n))


def _sources(cx):
    """Nodes of the big component from both ends and the middle, one next to a hole, and an isolated node (inside a hole)."""
    valid = cx.valid_idxs
    isolated = np.setdiff1d(np.arange(cx.n_nodes), np.unique(cx.edges))
    assert len(isolated)
    near_hole = valid[np.argmin(np.linalg.norm(cx.coords[valid] - [1 / 4, 3 / 4], axis=1))]
    return [int(valid[0]), int(valid[len(valid) // 2]), int(valid[-1]), int(near_hole), int(isolated[0])]


def test_csr_adjacency_is_sorted_symmetric_and_weighted_like_the_host_generator(cx):
    adj_ptr, adj, adj_w = g.csr_adjacency(cx, "euclid")
    assert adj_ptr[-1] == len(adj) == 2 * cx.n_edges and g.csr_adjacency(cx, "hops")[2] is None
    rows = np.repeat(np.arange(cx.n_nodes), np.diff(adj_ptr))
    assert np.all((np.diff(adj) > 0) | (np.diff(rows) > 0))
    assert np.array_equal(adj_w, np.linalg.norm(cx.coords[np.minimum(rows, adj)] - cx.coords[np.maximum(rows, adj)], axis=1))
    M = _scipy_graph((adj_ptr, adj, adj_w))
    assert (M != M.T).nnz == 0
    g._checked_graph(adj_ptr, adj, adj_w)
    with pytest.raises(ValueError, match="ascend"):
        g._checked_graph([0, 2, 3, 4], [2, 1, 0, 0], None)


@pytest.mark.parametrize("metric", METRICS)
def test_tree_host_matches_scipy(cx, metric):
    graph = g.csr_adjacency(cx, metric)
    adj_ptr, adj, adj_w = graph
    w = np.ones(len(adj)) if adj_w is None else adj_w
    G = _scipy_graph(graph)
    for s in _sources(cx):
        dist, pred = g.shortest_path_tree_host(adj_ptr, adj, adj_w, s)
        ref_d, ref_p = dijkstra(G, directed=False, indices=s, return_predecessors=True)
        assert np.array_equal(dist, ref_d)                                   # bit-equal (inf == inf)
        unreachable = ~np.isfinite(ref_d)
        assert unreachable.any() and np.all(pred[unreachable] == -1) and pred[s] == -1
        for v in np.flatnonzero(~unreachable):
            if v == s:
                continue
            row = slice(adj_ptr[v], adj_ptr[v + 1])
            tight = adj[row][dist[adj[row]] + w[row] == dist[v]]
            assert len(tight) and pred[v] == tight.min()                     # a tight neighbour, and the smallest one
        if metric == "euclid":
            assert np.array_equal(pred, np.where(ref_p < 0, -1, ref_p))
    lone = _sources(cx)[-1]
    dist, pred = g.shortest_path_tree_host(adj_ptr, adj, adj_w, lone)
    assert dist[lone] == 0 and np.isinf(np.delete(dist, lone)).all() and np.all(pred == -1)


def test_tree_host_later_generation_lowers_a_label():
    # 0 - 2 direct costs 5, the detour over 1 costs 2: generation 2 repairs what generation 1 wrote
    graph = g._checked_graph([0, 2, 4, 6], [1, 2, 0, 2, 0, 1], [1.0, 5.0, 1.0, 1.0, 5.0, 1.0])
    dist, pred = g.shortest_path_tree_host(*graph, 0)
    assert dist.tolist() == [0.0, 1.0, 2.0] and pred.tolist() == [-1, 0, 1]


@pytest.fixture(scope="module")
def host_walks(cx):
    return {m: g.generate_random_walks_batched(cx, m=30, seed=7, metric=m, backend="host", return_waypoints=True) for m in METRICS}


@pytest.mark.parametrize("metric", METRICS)
def test_batched_host_walks(cx, host_walks, metric):
    walks, ways = host_walks[metric]
    again = g.generate_random_walks_batched(cx, m=30, seed=7, metric=metric, backend="host")
    other = g.generate_random_walks_batched(cx, m=30, seed=8, metric=metric, backend="host")
    assert again == walks and other != walks and len(walks) == 30 and ways.shape == (30, 4)
    BEGIN, END, A, B = g.walk_regions(cx)
    graph = g.csr_adjacency(cx, metric)
    G = _scipy_graph(graph)
    for j, (wk, (v_begin, v_1, v_2, v_end)) in enumerate(zip(walks, ways.tolist())):
        assert len(wk) == len(set(wk))                                       # simple
        cx.edge_index(wk[:-1], wk[1:])                                       # consecutive nodes are adjacent (KeyError otherwise)
        assert v_begin in BEGIN and v_1 in A[j % 3] and v_2 in B[j % 3] and v_end in END
        assert wk[0] == v_begin and wk[-1] == v_end
        i1, i2 = wk.index(v_1), wk.index(v_2)
        assert 0 < i1 < i2 < len(wk) - 1                                     # the four regions are disjoint
        d = dijkstra(G, directed=False, indices=[v_1, v_2])
        for lo, hi, want in ((0, i1, d[0, v_begin]), (i1, i2, d[0, v_2]), (i2, len(wk) - 1, d[1, v_end])):
            seg = np.asarray(wk[lo:hi + 1])
            got = float(np.sum(np.asarray(G[seg[:-1], seg[1:]]).ravel()))
            # each segment is a shortest path between its waypoints; the first is summed from the other end than the tree
            # was grown: fewer than 64 fp64 additions, 64 * 2^-53 < 1e-14 relative
            assert got == pytest.approx(want, rel=1e-14, abs=0)
        if metric == "euclid":                                               # unique shortest paths: scipy's trees give the same walk
            p = dijkstra(G, directed=False, indices=[v_1, v_2], return_predecessors=True)[1]
            p_a, p_b, p_c = g._tree_path(p[0], v_1, v_begin), g._tree_path(p[0], v_1, v_2), g._tree_path(p[1], v_2, v_end)
            assert p_a[::-1][:-1] + p_b[:-1] + p_c == wk


def test_batched_generator_gives_up_like_the_host_generator(cx):
    two = g.Complex(n_nodes=cx.n_nodes, edges=cx.edges[:1], faces=cx.faces[:0], coords=cx.coords, valid_idxs=cx.valid_idxs)
    with pytest.raises(RuntimeError, match="could not generate enough simple walks"):
        g.generate_random_walks_batched(two, m=2, seed=1, backend="host")
    with pytest.raises(ValueError, match="backend"):
        g.generate_random_walks_batched(cx, m=2, backend="cpu")


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    from scone_gcn_amd import _lib
    lib = _lib.load()
    assert lib.scn_sssp_slot_bytes(400) >= 400 * 20 and lib.scn_sssp_slot_bytes(400) % 16 == 0 and lib.scn_sssp_slot_bytes(0) == 0
    p = 4096                                                                 # stands for a device array: nothing is launched or read
    ok = dict(n_nodes=400, adj_ptr=p, adj=p, adj_w=None, n_jobs=3, source=p, target=p, n_targets=2, path_cap=64, path=p, path_len=p,
              dist_out=None, dist_all=None, pred_all=None, n_gen=None, ws=p, ws_bytes=2 * lib.scn_sssp_slot_bytes(400), n_slots=2,
              stream=None)

    def call(**k):
        return lib.scn_sssp_paths(*{**ok, **k}.values())
    assert call(n_jobs=0) == 0                                               # nothing to do: no launch
    assert call(n_nodes=0) == -2 and call(n_jobs=-1) == -2                   # SCN_ERR_BAD_SHAPE
    for bad in (dict(n_targets=0), dict(n_targets=3), dict(path_cap=0), dict(n_slots=0), dict(adj_ptr=None), dict(adj=None),
                dict(source=None), dict(target=None), dict(path=None), dict(path_len=None), dict(ws=None), dict(ws=p + 4)):
        assert call(**bad) == _lib.SCN_ERR_BAD_ARG, bad
    assert call(n_slots=3) == -6 and call(ws_bytes=0) == -6                  # SCN_ERR_WORKSPACE: fewer than n_slots slots
    asm = lambda **k: lib.scn_walk_assemble(*{**dict(n=2, path=p, path_len=p, path_cap=8, walk=p, walk_len=p, walk_cap=16, stream=None),
                                              **k}.values())
    assert asm(n=0) == 0 and asm(n=-1) == -2
    for bad in (dict(path=None), dict(path_len=None), dict(walk=None), dict(walk_len=None), dict(path_cap=0), dict(walk_cap=0)):
        assert asm(**bad) == _lib.SCN_ERR_BAD_ARG, bad
    assert asm(walk_cap=_lib.SCN_WALK_MAX + 1) == _lib.SCN_ERR_UNSUPPORTED


def test_flags_parse_and_defaults_reproduce_the_present_call(monkeypatch):
    hp = te.hyperparams(["prog"])
    assert (hp["n_points"], hp["n_walks"], hp["walks"], hp["walk_metric"]) == (400, 1000, "host", "hops")
    hp2 = te.hyperparams(["prog", "-n_points", "900", "-n_walks", "50", "-walks", "device", "-walk_metric", "euclid", "-load_data", "0"])
    assert (hp2["n_points"], hp2["n_walks"], hp2["walks"], hp2["walk_metric"], hp2["load_data"]) == (900, 50, "device", "euclid", 0)
    calls = []
    monkeypatch.setattr(dataset_io, "generate_dataset", lambda *a, **k: calls.append((a, k)))
    for h in (hp, hp2):
        with pytest.raises(Exception, match="Data generation done"):
            te.data_setup(load=False, folder_suffix="w", hp=h)
    (a0, k0), (a1, k1) = calls
    assert a0 == (400, 1000) and all(type(x) is int for x in a0)
    assert k0 == {"folder": "w", "holes": True, "walks": "host", "metric": "hops"}
    assert a1 == (900, 50) and k1 == {"folder": "w", "holes": True, "walks": "device", "metric": "euclid"}


def test_generate_dataset_default_still_calls_the_host_generator(monkeypatch, tmp_path):
    seen = {}
    real = g.generate_random_walks

    def spy(cx, **k):
        seen.update(k)
        return real(cx, **k)
    monkeypatch.setattr(g, "generate_random_walks", spy)
    monkeypatch.setattr(g, "generate_random_walks_batched", lambda *a, **k: pytest.fail("the default must not take the batched path"))
    monkeypatch.chdir(tmp_path)
    dataset_io.generate_dataset(150, 12, folder="dflt", holes=True)
    assert seen["m"] == 12 and seen["metric"] == "hops" and "waypoint_pool" not in seen
    with pytest.raises(ValueError, match="walks"):
        dataset_io.generate_dataset(150, 12, folder="dflt", holes=True, walks="gpu")
