"""Batched shortest paths and walk assembly on the device (csrc/scn_walks.hip): scn_sssp_paths against the host statement
synthetic_data_gen.shortest_path_tree_host -- dist bit for bit, pred, paths and path_len equal -- on the smallest graphs that can
break the kernel, scn_walk_assemble on hand-made segments, and the batched walk generator device against host."""
import os

import numpy as np
import pytest
import torch

from scone_gcn_amd import dataset_io
from scone_gcn_amd import synthetic_data_gen as g

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def csr(n, edges, w=None):
    """The checked (adj_ptr, adj, adj_w) triple of an undirected edge list (and one weight per edge)."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    rows, cols = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
    order = np.lexsort((cols, rows))
    adj_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    adj_w = None if w is None else np.concatenate([w, w]).astype(np.float64)[order]
    return g._checked_graph(adj_ptr, cols[order], adj_w)


def chain(n):
    return csr(n, [(i, i + 1) for i in range(n - 1)])


def ring_with_chords(n, weighted, seed=0):
    rs = np.random.RandomState(seed)
    edges = {(i, (i + 1) % n) if i < (i + 1) % n else ((i + 1) % n, i) for i in range(n)} if n > 2 else {(i, i + 1) for i in range(n - 1)}
    for _ in range(n // 2):
        a, b = sorted(rs.randint(0, n, 2).tolist())
        if a != b:
            edges.add((a, b))
    edges = sorted(edges)
    return csr(n, edges, rs.rand(len(edges)) + 0.05 if weighted else None)


def host(graph, sources, targets, path_cap):
    """What scn_sssp_paths must return, from shortest_path_tree_host: path (-1 where nothing is written), path_len, dist, trees."""
    src = np.asarray(sources).ravel()
    tgt = np.asarray(targets).reshape(len(src), -1)
    n = len(graph[0]) - 1
    path = np.full(tgt.shape + (path_cap,), -1, np.int32)
    path_len = np.zeros(tgt.shape, np.int32)
    dist = np.full(tgt.shape, np.inf)
    dist_all, pred_all = np.zeros((len(src), n)), np.zeros((len(src), n), np.int32)
    for j, s in enumerate(src):
        dist_all[j], pred_all[j] = g.shortest_path_tree_host(*graph, int(s))
        for t, v in enumerate(tgt[j]):
            if v < 0:
                continue
            p = g._tree_path(pred_all[j], int(s), int(v))
            if p is None:
                path_len[j, t] = -1
            elif len(p) > path_cap:
                path_len[j, t], dist[j, t] = -2, dist_all[j, v]
            else:
                path_len[j, t], dist[j, t] = len(p), dist_all[j, v]
                path[j, t, :len(p)] = p
    return {"path": path, "path_len": path_len, "dist": dist, "dist_all": dist_all, "pred_all": pred_all}


def device(graph, sources, targets, path_cap, n_slots=None, want_tree=True, want_gen=False):
    dg = g.device_graph(graph)
    out = g.sssp_paths_device(dg, sources, targets, path_cap, n_slots=n_slots, want_tree=want_tree, want_gen=want_gen)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(got, want):
    for k, w in want.items():
        if k in got:
            assert got[k].shape == w.shape, k
            assert np.array_equal(got[k], w), k                              # distances bit for bit (inf == inf)


def check(graph, sources, targets, path_cap, n_slots=None):
    """The jobs with full trees and, paths only, with the early end: both equal the host statement."""
    want = host(graph, sources, targets, path_cap)
    got = device(graph, sources, targets, path_cap, n_slots=n_slots)
    same(got, want)
    same(device(graph, sources, targets, path_cap, n_slots=n_slots, want_tree=False), want)
    return got, want


def test_source_is_target():
    got, _ = check(chain(5), [2, 0], [2, 0], 4)
    assert got["path_len"].ravel().tolist() == [1, 1] and got["path"][:, 0, 0].tolist() == [2, 0]


def test_two_components():
    graph = csr(5, [(0, 1), (1, 2), (3, 4)])
    got, _ = check(graph, [0, 3], [[2, 4], [4, -1]], 8)
    assert got["path_len"].tolist() == [[3, -1], [2, 0]]
    assert np.isinf(got["dist"][0, 1]) and np.isinf(got["dist_all"][0, 3:]).all() and (got["pred_all"][0, 3:] == -1).all()
    assert got["path"][1, 0, :2].tolist() == [3, 4]


def test_chain_of_600_and_the_path_cap():
    graph = chain(600)
    got, _ = check(graph, [0, 599], [599, 300], 600)                         # fits exactly
    assert got["path_len"].ravel().tolist() == [600, 300] and got["path"][0, 0].tolist() == list(range(600))
    gens = device(graph, [0], [599], 600, want_gen=True)["n_gen"]
    assert gens.tolist() == [600]                                            # every generation the cap allows, and not capped
    got, _ = check(graph, [0, 599], [599, 300], 599)                         # one less
    assert got["path_len"].ravel().tolist() == [-2, 300] and (got["path"][0] == -1).all()


def test_star_of_300_leaves():
    graph = csr(301, [(0, i) for i in range(1, 301)])
    got, _ = check(graph, [0, 5, 300], [[300, 1], [299, 0], [1, -1]], 3)
    assert got["path_len"].tolist() == [[2, 2], [3, 2], [3, 0]]


def test_weighted_fan_where_a_later_generation_lowers_a_label():
    k = 20
    edges = [(0, i) for i in range(1, k + 1)] + [(i, i + 1) for i in range(1, k)]
    w = [float(i) for i in range(1, k + 1)] + [0.1] * (k - 1)                # the spoke to i costs i, the rim 0.1 a step
    got, want = check(csr(k + 1, edges, w), [0, k], [[k, 2], [0, 1]], k + 1)
    assert got["path"][0, 0, :k + 1].tolist() == list(range(k + 1))          # all the way along the rim
    assert want["dist_all"][0, k] < 3.0


@pytest.mark.parametrize("n", [1, 63, 65, 257])
@pytest.mark.parametrize("weighted", [False, True])
def test_sizes_around_the_wave_and_the_workgroup(n, weighted):
    graph = ring_with_chords(n, weighted) if n > 1 else g._checked_graph([0, 0], [], np.zeros(0) if weighted else None)
    src = sorted({0, n // 3, n // 2, n - 1})
    check(graph, src, [[n - 1 - s, (s + n // 2) % n] for s in src], n)


@pytest.mark.parametrize("weighted", [False, True])
def test_seven_jobs_on_two_slots(weighted):
    graph = ring_with_chords(257, weighted, seed=3)
    src = [0, 40, 80, 120, 160, 200, 256]
    tgt = [[(s + 100) % 257, (s + 201) % 257] for s in src]
    got, _ = check(graph, src, tgt, 257, n_slots=2)
    for j in range(7):                                                       # a slot's later job sees nothing of its earlier ones
        alone = device(graph, src[j:j + 1], tgt[j:j + 1], 257, n_slots=1)
        same(alone, {k: v[j:j + 1] for k, v in got.items()})


def test_one_target_and_an_absent_target():
    graph = ring_with_chords(65, True, seed=5)
    check(graph, [1, 2, 3], [10, 20, 30], 65)                                # n_targets = 1
    got, _ = check(graph, [1, 2, 3], [[-1, 10], [20, -1], [-1, -1]], 65)
    assert (got["path_len"] > 0).tolist() == [[False, True], [True, False], [False, False]]
    assert got["path_len"][2].tolist() == [0, 0]


@pytest.fixture(scope="module")
def cx():
    d = np.load(os.path.join(HERE, "golden", "cfg1_complex.npz"))
    return g.Complex(n_nodes=int(d["n_nodes"]), edges=d["edges"].astype(np.int64), faces=d["faces"].astype(np.int64),
                     coords=d["coords"], valid_idxs=d["valid_idxs"].astype(np.int64))


@pytest.mark.parametrize("metric", ["hops", "euclid"])
def test_cfg1_trees(cx, metric):
    graph = g.csr_adjacency(cx, metric)
    valid = cx.valid_idxs
    src = valid[np.linspace(0, len(valid) - 1, 15).astype(int)].tolist() + [int(np.setdiff1d(np.arange(400), valid)[0])]
    tgt = [[int(valid[-1 - i]), int(valid[7 * i])] for i in range(16)]
    check(graph, src, tgt, 400)
    (ptr, nodes), path_len, dist = g.shortest_paths_device(cx, src, tgt, metric=metric)
    want = host(graph, src, tgt, 400)
    assert np.array_equal(path_len, want["path_len"]) and np.array_equal(dist, want["dist"])
    for i, (j, t) in enumerate(np.ndindex(16, 2)):
        assert nodes[ptr[i]:ptr[i + 1]].tolist() == want["path"][j, t, :max(want["path_len"][j, t], 0)].tolist()


@pytest.mark.parametrize("metric", ["hops", "euclid"])
def test_full_size_paths_against_scipy(big_complex, metric):
    """|V| = 369 004: thousands of generations, queues and paths far beyond one pass of the workgroup, the early end.  scipy is the
    reference here (one host-statement tree at this size takes seconds): distances bit-equal, every step of a path the smallest tight
    neighbour."""
    from scipy.sparse.csgraph import dijkstra
    import scipy.sparse as sp
    cx = big_complex[0]
    adj_ptr, adj, adj_w = g.csr_adjacency(cx, metric)
    w = np.ones(len(adj)) if adj_w is None else adj_w
    G = sp.csr_matrix((w, adj.astype(np.int64), adj_ptr.astype(np.int64)), shape=(cx.n_nodes, cx.n_nodes))
    valid = cx.valid_idxs
    src = [int(valid[len(valid) // 3]), int(valid[5])]
    tgt = [[int(valid[-1]), int(valid[0])], [int(valid[2 * len(valid) // 3]), -1]]
    (ptr, nodes), path_len, dist = g.shortest_paths_device(cx, src, tgt, metric=metric)
    ref = dijkstra(G, directed=False, indices=src)
    for i, (j, t) in enumerate(np.ndindex(2, 2)):
        p = nodes[ptr[i]:ptr[i + 1]]
        if tgt[j][t] < 0:
            assert path_len[j, t] == 0 and len(p) == 0
            continue
        assert path_len[j, t] == len(p) and p[0] == src[j] and p[-1] == tgt[j][t]
        assert dist[j, t] == ref[j, tgt[j][t]]
        # hops: the paths jump along the long hull edges (a few dozen nodes); Euclidean ones cross the complex step by step
        assert len(p) == ref[j, tgt[j][t]] + 1 if metric == "hops" else len(p) > 100
        for u, v in zip(p[:-1].tolist(), p[1:].tolist()):
            row = slice(adj_ptr[v], adj_ptr[v + 1])
            tight = adj[row][ref[j, adj[row]] + w[row] == ref[j, v]]
            assert u == tight.min()


def test_shortest_paths_device_doubles_the_cap():
    assert g.initial_path_cap(600) == 200
    (ptr, nodes), path_len, dist, (dist_all, pred_all) = g.shortest_paths_device(chain(600), [0, 0, 599], [599, 10, 150], want_tree=True)
    assert path_len.ravel().tolist() == [600, 11, 450] and dist.ravel().tolist() == [599.0, 10.0, 449.0]
    assert nodes[ptr[0]:ptr[1]].tolist() == list(range(600)) and nodes[ptr[2]:ptr[3]].tolist() == list(range(599, 149, -1))
    assert dist_all[0].tolist() == list(range(600)) and pred_all[2].tolist() == list(range(1, 600)) + [-1]


def _assemble(segments, path_cap, walk_cap):
    """segments: per attempt the three node lists (or a negative path_len code) of v_1 -> v_begin, v_1 -> v_2, v_2 -> v_end."""
    n = len(segments)
    path = np.full((2 * n, 2, path_cap), -1, np.int32)
    path_len = np.zeros((2 * n, 2), np.int32)
    for a, seg in enumerate(segments):
        for (j, t), s in zip(((2 * a, 0), (2 * a, 1), (2 * a + 1, 0)), seg):
            if isinstance(s, int):
                path_len[j, t] = s
            else:
                path_len[j, t] = len(s)
                path[j, t, :len(s)] = s
    walk, walk_len = g.walk_assemble_device(torch.from_numpy(path).cuda(), torch.from_numpy(path_len).cuda(), walk_cap)
    torch.cuda.synchronize()
    return walk.cpu().numpy(), walk_len.cpu().numpy()


def test_walk_assemble():
    ok = ([5, 4, 3], [5, 6, 7, 8], [8, 9, 10])                               # 3 4 | 5 6 7 | 8 9 10
    shared = ([5, 4, 9], [5, 6, 7, 8], [8, 9, 10])                           # 9 in the first and the third segment
    unreachable = ([5, 4, 3], -1, [8, 9, 10])
    too_long = ([5, 4, 3], [5, 6, 7, 8], -2)
    long_one = (list(range(300, -1, -1)), list(range(300, 600)), list(range(599, 1000)))   # 0 .. 999: more than one pass of the workgroup
    walk, walk_len = _assemble([ok, shared, unreachable, too_long, long_one], 401, 1000)
    assert walk_len.tolist() == [8, 0, 0, 0, 1000]
    assert walk[0, :8].tolist() == [3, 4, 5, 6, 7, 8, 9, 10] and (walk[0, 8:] == -1).all()
    assert walk[4].tolist() == list(range(1000)) and (walk[2:4] == -1).all()
    walk, walk_len = _assemble([ok, long_one], 401, 999)                     # one node more than walk_cap: nothing is written
    assert walk_len.tolist() == [8, 0] and (walk[1] == -1).all()
    walk, walk_len = _assemble([ok], 4, 8)                                   # exactly walk_cap
    assert walk_len.tolist() == [8] and walk[0].tolist() == [3, 4, 5, 6, 7, 8, 9, 10]
    walk, walk_len = _assemble([ok], 4, 7)
    assert walk_len.tolist() == [0] and (walk == -1).all()


@pytest.mark.parametrize("metric", ["hops", "euclid"])
def test_batched_walks_device_equals_host(cx, metric):
    st = {}
    dev, ways_d = g.generate_random_walks_batched(cx, m=30, seed=7, metric=metric, backend="device", return_waypoints=True, stats=st)
    hst, ways_h = g.generate_random_walks_batched(cx, m=30, seed=7, metric=metric, backend="host", return_waypoints=True)
    assert dev == hst and np.array_equal(ways_d, ways_h)
    assert st["accepted"] == 30 and st["attempts"] >= 30 and st["trees"] == 2 * st["attempts"] and st["generations"] > 0


def test_generate_dataset_with_device_walks(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cxd = dataset_io.generate_dataset(150, 12, folder="dw", holes=True, walks="device", metric="euclid")
    for hop in (1, 2):
        X, (B1, B2), y, train_mask, test_mask, coords, last, tnodes = dataset_io.load_dataset("trajectory_data_%dhop_dw" % hop)
        assert X.shape[:2] == (12, cxd.n_edges) and B1.shape == (150, cxd.n_edges) and len(last) == len(tnodes) == 12
        assert y.shape[0] == 12 and np.all(y.sum(axis=(1, 2)) == 1) and np.array_equal(train_mask + test_mask, np.ones(11))
        cxd.edge_index(last, tnodes)                                         # every target is a neighbour of its last node
