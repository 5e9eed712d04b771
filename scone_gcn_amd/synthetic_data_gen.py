"""Sparse, scalable synthetic complexes and trajectories (host side, NumPy/scipy).

Follows the recipe of the reference generator -- trajectory_analysis/synthetic_data_gen.py (SDG):
  random_SC_graph      SDG:82-137   points under seed 1, sorted along x+y, Delaunay, two holes
  incidence_matrices   SDG:139-161  B1 (-1 tail / +1 head, tail < head), B2 (+1,+1,-1 for (a,b),(b,c),(a,c))
  generate_random_walks SDG:178-243 BEGIN -> A_r -> B_r -> END by concatenated shortest paths, r = i % 3
  split_paths / path_to_flow / path_dataset  SDG:245-258, 327-373
but never materialises a dense V x E or E x F matrix, so it reaches |E| ~ 1M (the reference's dense
B1/B2 stop at ~1e4 edges).  For n = 400 the complex is bit-identical to the reference's
(tests/golden/cfg1_complex.npz); the walks use our own BFS tie-breaking, so they follow the reference's
distribution, not its exact node sequences (the exact ones are in tests/golden/cfg1_paths.npz).

The second half of the module is the walk generator without a waypoint pool on the device: batched shortest paths
(shortest_paths_device, scn_sssp_paths), their host statement (shortest_path_tree_host) and generate_random_walks_batched.
"""
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import breadth_first_order, dijkstra
from scipy.spatial import Delaunay


@dataclass
class Complex:
    """A 2-dimensional simplicial complex: nodes 0..n_nodes-1, sorted edges (a<b), sorted faces (a<b<c)."""
    n_nodes: int
    edges: np.ndarray          # (E, 2) int64, lexicographically sorted, a < b
    faces: np.ndarray          # (F, 3) int64, sorted rows, lexicographically sorted
    coords: np.ndarray = None  # (V, 2) float64 or None
    valid_idxs: np.ndarray = None

    @property
    def n_edges(self):
        return int(self.edges.shape[0])

    @property
    def n_faces(self):
        return int(self.faces.shape[0])

    def edge_index(self, a, b):
        """Index of edge (min,max) for arrays a, b (vectorised binary search on the sorted edge list)."""
        a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        key = lo * self.n_nodes + hi
        keys = self.edges[:, 0] * self.n_nodes + self.edges[:, 1]
        idx = np.searchsorted(keys, key)
        if np.any(idx >= len(keys)) or np.any(keys[np.minimum(idx, len(keys) - 1)] != key):
            raise KeyError("edge not in complex")
        return idx


def random_SC_graph(n, holes=True):
    """SDG:82-137 without networkx.  Returns a Complex (edges/faces as arrays)."""
    rs = np.random.RandomState(1)                                        # SDG:98
    coords = rs.rand(n, 2)
    coords = coords[np.argsort(np.sum(coords, axis=1))]                  # SDG:102-104
    tri = Delaunay(coords)                                               # SDG:107 (qhull is deterministic)
    if holes:
        valid = (np.linalg.norm(coords - [1 / 4, 3 / 4], axis=1) > 1 / 8) \
            & (np.linalg.norm(coords - [3 / 4, 1 / 4], axis=1) > 1 / 8)  # SDG:109-110
    else:
        valid = np.ones(n, dtype=bool)
    simp = np.sort(tri.simplices.astype(np.int64), axis=1)
    simp = simp[valid[simp].all(axis=1)]                                 # SDG:114
    faces = np.unique(simp, axis=0)                                      # sorted, like sorted([...])
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [0, 2]]])   # SDG:120-124
    edges = np.unique(e, axis=0)                                         # SDG:127
    return Complex(n_nodes=n, edges=edges, faces=faces, coords=coords,
                   valid_idxs=np.nonzero(valid)[0])


def incidence_matrices(cx):
    """Sparse B1 (V x E) and B2 (E x F) with the reference's sign conventions (SDG:139-161)."""
    E, F = cx.n_edges, cx.n_faces
    ar = np.arange(E)
    B1 = sp.csr_matrix((np.concatenate([-np.ones(E), np.ones(E)]),
                        (np.concatenate([cx.edges[:, 0], cx.edges[:, 1]]), np.concatenate([ar, ar]))),
                       shape=(cx.n_nodes, E))
    if F:
        f = cx.faces
        e_ab = cx.edge_index(f[:, 0], f[:, 1])
        e_bc = cx.edge_index(f[:, 1], f[:, 2])
        e_ac = cx.edge_index(f[:, 0], f[:, 2])
        fr = np.arange(F)
        B2 = sp.csr_matrix((np.concatenate([np.ones(F), np.ones(F), -np.ones(F)]),
                            (np.concatenate([e_ab, e_bc, e_ac]), np.concatenate([fr, fr, fr]))),
                           shape=(E, F))
    else:
        B2 = sp.csr_matrix((E, 0))
    return B1, B2


def complex_from_incidence(B1, B2):
    """Recover (edges, faces) from incidence matrices given dense or sparse (the dataset folder format)."""
    B1 = sp.csc_matrix(B1)
    V, E = B1.shape
    edges = np.zeros((E, 2), np.int64)
    for e in range(E):
        rows = B1.indices[B1.indptr[e]:B1.indptr[e + 1]]
        vals = B1.data[B1.indptr[e]:B1.indptr[e + 1]]
        edges[e, 0] = rows[np.argmin(vals)]       # -1 = tail
        edges[e, 1] = rows[np.argmax(vals)]       # +1 = head
    B2c = sp.csc_matrix(B2)
    F = B2c.shape[1]
    faces = np.zeros((F, 3), np.int64)
    for f in range(F):
        es = B2c.indices[B2c.indptr[f]:B2c.indptr[f + 1]]
        faces[f] = np.unique(edges[es].ravel())
    return edges, faces


def adjacency(cx):
    a, b = cx.edges[:, 0], cx.edges[:, 1]
    n = cx.n_nodes
    return sp.csr_matrix((np.ones(2 * len(a)), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(n, n))


def _tree_path(pred, root, v):
    """Nodes from root to v along a BFS predecessor tree (inclusive)."""
    out = [int(v)]
    while out[-1] != root:
        p = pred[out[-1]]
        if p < 0:
            return None
        out.append(int(p))
    return out[::-1]


def generate_random_walks(cx, m=1000, seed=1030, waypoint_pool=None, metric="hops"):
    """SDG:178-243.  `waypoint_pool=k` draws the A_r / B_r waypoints from k candidates per region so that
    only 6k shortest-path trees are built however many walks are requested (needed at |V| ~ 4e5); None = fresh
    draw per walk as the reference does.  metric="hops" is the reference's BFS shortest path; "euclid" weights
    edges by length (Dijkstra): on very large Delaunay complexes the hop-count paths all detour along the long
    convex-hull edges, overlap there and fail the reference's simple-path test (SDG:239) almost always."""
    rs = np.random.RandomState(seed)
    pts, valid = cx.coords, cx.valid_idxs
    s = np.sum(pts[valid], axis=1)
    BEGIN, END = valid[s < 1 / 4], valid[s > 7 / 4]                      # SDG:207-208
    A012 = valid[(s > 1 / 4) & (s < 1)]
    B012 = valid[(s < 7 / 4) & (s > 1)]

    def regions(X):
        d = pts[X, 1] - pts[X, 0]
        return [X[(d < 1 / 2) & (d > -1 / 2)], X[d > 1 / 2], X[d < -1 / 2]]   # SDG:211-218
    A, B = regions(A012), regions(B012)
    if waypoint_pool:
        A = [rs.choice(a, size=min(waypoint_pool, len(a)), replace=False) for a in A]
        B = [rs.choice(b, size=min(waypoint_pool, len(b)), replace=False) for b in B]
    G = adjacency(cx)
    if metric == "euclid":
        a, b = cx.edges[:, 0], cx.edges[:, 1]
        w = np.linalg.norm(pts[a] - pts[b], axis=1)
        G = sp.csr_matrix((np.concatenate([w, w]), (np.concatenate([a, b]), np.concatenate([b, a]))),
                          shape=(cx.n_nodes, cx.n_nodes))
    trees = {}

    def tree(v):
        if v not in trees:
            if metric == "euclid":
                trees[v] = dijkstra(G, directed=False, indices=v, return_predecessors=True)[1]
            else:
                trees[v] = breadth_first_order(G, v, directed=False, return_predecessors=True)[1]
        return trees[v]

    paths, i, tries = [], 0, 0
    while len(paths) < m:
        tries += 1
        if tries > 50 * m + 1000:
            raise RuntimeError("could not generate enough simple walks")
        r = i % 3
        v_begin = int(rs.choice(BEGIN))
        v_1, v_2 = int(rs.choice(A[r])), int(rs.choice(B[r]))
        v_end = int(rs.choice(END))
        t1, t2 = tree(v_1), tree(v_2)
        p_a = _tree_path(t1, v_1, v_begin)
        p_b = _tree_path(t1, v_1, v_2)
        p_c = _tree_path(t2, v_2, v_end)
        if p_a is None or p_b is None or p_c is None:
            continue
        path = p_a[::-1][:-1] + p_b[:-1] + p_c                            # SDG:236-238
        if len(path) == len(set(path)):                                   # SDG:239
            paths.append(path)
            i += 1
        if not waypoint_pool and len(trees) > 64:
            trees.clear()
    return paths


def split_paths(paths, rs, truncate_paths=True, suffix_size=2):
    """SDG:245-258."""
    if truncate_paths:
        paths = [p[:4 + rs.choice(range(2, len(p) - 4))] for p in paths]
    prefixes = [p[:-suffix_size] for p in paths]
    suffixes = [p[-suffix_size:] for p in paths]
    return prefixes, suffixes, [p[-1] for p in prefixes]


@dataclass
class SparseFlows:
    """Edge flows of N trajectories as ragged (edge index, value) lists: the sparse form of flows_in (N, E, 1)."""
    ptr: np.ndarray      # (N+1,) int64
    idx: np.ndarray      # (nnz,) int64 edge ids
    val: np.ndarray      # (nnz,) float32
    n_edges: int

    def __len__(self):
        return len(self.ptr) - 1

    def select(self, sel):
        sel = np.asarray(sel)
        lens = self.ptr[sel + 1] - self.ptr[sel]
        ptr = np.concatenate([[0], np.cumsum(lens)])
        take = np.concatenate([np.arange(self.ptr[i], self.ptr[i + 1]) for i in sel]) if len(sel) else np.zeros(0, np.int64)
        return SparseFlows(ptr.astype(np.int64), self.idx[take], self.val[take], self.n_edges)

    def todense(self):
        X = np.zeros((len(self), self.n_edges, 1), np.float32)
        rows = np.repeat(np.arange(len(self)), np.diff(self.ptr))
        np.add.at(X[:, :, 0], (rows, self.idx), self.val)
        return X

    @staticmethod
    def fromdense(X):
        X = np.asarray(X)
        X2 = X.reshape(X.shape[0], X.shape[1])
        rows, cols = np.nonzero(X2)
        ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=X2.shape[0]))])
        return SparseFlows(ptr.astype(np.int64), cols.astype(np.int64), X2[rows, cols].astype(np.float32), X2.shape[1])


def paths_to_flows(cx, paths):
    """path_to_flow (SDG:327-344) for a list of node paths -> SparseFlows (+1 along a<b, -1 against)."""
    ptr, idx, val = [0], [], []
    for p in paths:
        p = np.asarray(p, np.int64)
        if len(p) > 1:
            a, b = p[:-1], p[1:]
            e = cx.edge_index(a, b)
            sgn = np.where(a < b, 1.0, -1.0)
            ue, inv = np.unique(e, return_inverse=True)
            v = np.zeros(len(ue))
            np.add.at(v, inv, sgn)
            idx.append(ue)
            val.append(v)
            ptr.append(ptr[-1] + len(ue))
        else:
            ptr.append(ptr[-1])
    idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    val = np.concatenate(val) if val else np.zeros(0)
    return SparseFlows(np.asarray(ptr, np.int64), idx.astype(np.int64), val.astype(np.float32), cx.n_edges)


def flow_to_path(flow, edges, last_node):
    """Node path of a +-1 edge flow that ends in last_node (SDG:299-325): walk backwards along the oriented edges."""
    flow = np.asarray(flow).reshape(-1)
    into = {}
    for i in np.flatnonzero(flow):
        a, b = (int(edges[i][0]), int(edges[i][1])) if flow[i] > 0 else (int(edges[i][1]), int(edges[i][0]))
        into.setdefault(b, []).append(a)                       # oriented edge a -> b
    path, cur, left = [int(last_node)], int(last_node), int(np.count_nonzero(flow))
    while left:
        if not into.get(cur):
            raise ValueError("flow is not a path ending in last_node")
        cur = into[cur].pop()
        path.append(cur)
        left -= 1
    return path[::-1]


def neighborhood_table(cx):
    """nbrhoods (V, D): sorted neighbours, -1 padded (TE:273-279); also degrees."""
    G = adjacency(cx)
    deg = np.diff(G.indptr)
    D = int(deg.max())
    tab = -np.ones((cx.n_nodes, D), np.int64)
    G.sort_indices()
    rows = np.repeat(np.arange(cx.n_nodes), deg)
    pos = np.arange(len(G.indices)) - np.repeat(G.indptr[:-1], deg)
    tab[rows, pos] = G.indices
    return tab, deg


def path_dataset(cx, paths, seed=None, truncate_paths=True, rs=None):
    """1-hop part of SDG:346-361: prefix flows, one-hot target index among the sorted neighbours, last nodes."""
    rs = rs if rs is not None else np.random.RandomState(seed)
    prefixes, suffixes, last_nodes = split_paths(paths, rs, truncate_paths)
    nbr, _ = neighborhood_table(cx)
    target_nodes = np.asarray([s[0] for s in suffixes], np.int64)
    last_nodes = np.asarray(last_nodes, np.int64)
    choice = np.argmax(nbr[last_nodes] == target_nodes[:, None], axis=1)
    return paths_to_flows(cx, prefixes), choice.astype(np.int64), last_nodes, target_nodes, prefixes


def calibrate_n_points(target_edges, holes=True):
    """Number of points whose complex has ~target_edges edges (E ~ 2.7 V with the two holes cut out)."""
    return max(16, int(round(target_edges / (2.71 if holes else 2.98))))


# ----------------------------------------------------------------------------------------------
# Batched shortest paths and the walk generator without a waypoint pool (csrc/scn_walks.hip)
#
# The definition, shared by the host statement below and the device kernel: dist is THE fixed point of
#     dist[v] = min over neighbours u of fl(dist[u] + w(u, v))        (fp64; one solution for weights >= 0)
# and pred[v] is the smallest-index neighbour u with fl(dist[u] + w(u, v)) == dist[v] exactly -- not whichever relaxation
# happened to win.  Trees, paths and walks therefore depend on the graph alone, and the two backends agree node for node.
# ----------------------------------------------------------------------------------------------

SSSP_SLOTS_PER_CU = 4          # workgroups (= workspace slots) per compute unit of a scn_sssp_paths launch
SSSP_MEMORY_SHARE = 0.25       # of the device's free memory the slots may take


def csr_adjacency(cx, metric="hops"):
    """(adj_ptr (V + 1,) int32, adj int32, adj_w float64 or None) of the complex: both directions of every edge, the columns
    of a row ascending; adj_w = the edge lengths np.linalg.norm(pts[a] - pts[b]) as generate_random_walks forms them
    (metric="euclid"), None for metric="hops"."""
    if metric not in ("hops", "euclid"):
        raise ValueError("metric must be 'hops' or 'euclid', got %r" % (metric,))
    a, b = cx.edges[:, 0], cx.edges[:, 1]
    rows, cols = np.concatenate([a, b]), np.concatenate([b, a])
    order = np.lexsort((cols, rows))
    adj_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=cx.n_nodes))])
    adj_w = None
    if metric == "euclid":
        w = np.linalg.norm(cx.coords[a] - cx.coords[b], axis=1)
        adj_w = np.ascontiguousarray(np.concatenate([w, w])[order], np.float64)
    return np.ascontiguousarray(adj_ptr, np.int32), np.ascontiguousarray(cols[order], np.int32), adj_w


def _checked_graph(adj_ptr, adj, adj_w):
    """The three arrays as the kernels need them, after the checks only the host can make: ValueError otherwise."""
    adj_ptr, adj = np.asarray(adj_ptr, np.int64).ravel(), np.asarray(adj, np.int64).ravel()
    n = len(adj_ptr) - 1
    if n < 1 or adj_ptr[0] != 0 or np.any(np.diff(adj_ptr) < 0) or adj_ptr[-1] != len(adj):
        raise ValueError("adj_ptr must rise from 0 to len(adj) over at least one node")
    if len(adj) >= (1 << 31) - 1 or n >= (1 << 31) - 1:
        raise ValueError("the graph does not fit 32-bit indices")
    if len(adj) and (adj.min() < 0 or adj.max() >= n):
        raise ValueError("adj names a node outside the graph's %d nodes" % n)
    rows = np.repeat(np.arange(n), np.diff(adj_ptr))
    if len(adj) > 1 and np.any((np.diff(adj) <= 0) & (np.diff(rows) == 0)):
        raise ValueError("the columns of a row must ascend strictly")
    if adj_w is not None:
        adj_w = np.ascontiguousarray(adj_w, np.float64).ravel()
        if len(adj_w) != len(adj) or not np.all(adj_w >= 0):
            raise ValueError("adj_w must hold one weight >= 0 per entry of adj")
    return np.ascontiguousarray(adj_ptr, np.int32), np.ascontiguousarray(adj, np.int32), adj_w


def shortest_path_tree_host(adj_ptr, adj, adj_w, source):
    """(dist (V,) float64, pred (V,) int64) from `source` by the definition above, in NumPy: the frontier is relaxed generation
    by generation with np.minimum.at until nothing drops (at most V generations), then every reached node takes its smallest
    tight neighbour.  Unreachable: inf and -1; pred[source] = -1.  adj_w None = unit weights.  The statement the device kernel
    (scn_sssp_paths) is tested against."""
    adj_ptr, adj = np.asarray(adj_ptr, np.int64), np.asarray(adj, np.int64)
    n = len(adj_ptr) - 1
    w = np.ones(len(adj)) if adj_w is None else np.asarray(adj_w, np.float64)
    deg = np.diff(adj_ptr)
    dist = np.full(n, np.inf)
    dist[source] = 0.0
    frontier, gen = np.asarray([source], np.int64), 0
    while len(frontier):
        gen += 1
        if gen > n:
            raise RuntimeError("the frontier is not empty after %d generations" % n)
        cnt = deg[frontier]
        k = np.repeat(adj_ptr[frontier] - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(int(cnt.sum()))
        new = dist.copy()
        np.minimum.at(new, adj[k], np.repeat(dist[frontier], cnt) + w[k])
        frontier = np.flatnonzero(new < dist)
        dist = new
    rows = np.repeat(np.arange(n), deg)
    tight = np.isfinite(dist[rows]) & (dist[adj] + w == dist[rows]) & (rows != source)
    pred = np.full(n, n, np.int64)
    np.minimum.at(pred, rows[tight], adj[tight])
    pred[pred == n] = -1
    return dist, pred


class _DeviceGraph:
    """The adjacency (and weights) of one complex and metric on one device: uploaded once, kept on the Complex."""

    def __init__(self, graph, device):
        import torch
        self.adj_ptr_h, self.adj_h, self.adj_w_h = graph
        self.n_nodes, self.device = len(graph[0]) - 1, device
        pad = lambda a: a if len(a) else np.zeros(1, a.dtype)             # a graph without edges still hands the library an array
        self.adj_ptr, self.adj = torch.from_numpy(graph[0]).to(device), torch.from_numpy(pad(graph[1])).to(device)
        self.adj_w = None if graph[2] is None else torch.from_numpy(pad(graph[2])).to(device)

    def n_slots(self, n_jobs):
        """Slots of a launch: SSSP_SLOTS_PER_CU workgroups per compute unit, no more than the jobs, and no more than fit
        SSSP_MEMORY_SHARE of the memory that is free now."""
        import torch
        from . import _lib, ops
        free, _ = torch.cuda.mem_get_info(self.device)
        per_slot = int(_lib.load().scn_sssp_slot_bytes(self.n_nodes))
        return max(1, min(int(n_jobs), SSSP_SLOTS_PER_CU * ops.device_cus(self.device), int(SSSP_MEMORY_SHARE * free) // per_slot))


def device_graph(cx, metric="hops", device=None):
    """The _DeviceGraph of a Complex (cached on it per metric and device) or of an (adj_ptr, adj, adj_w) triple."""
    import torch
    from . import ops
    device = torch.device(ops.default_device() if device is None else device)
    if isinstance(cx, _DeviceGraph):
        return cx
    if isinstance(cx, tuple):
        return _DeviceGraph(_checked_graph(*cx), device)
    cache = cx.__dict__.setdefault("_device_graphs", {})
    key = (metric, str(device))
    if key not in cache:
        cache[key] = _DeviceGraph(csr_adjacency(cx, metric), device)
    return cache[key]


def sssp_paths_device(graph, sources, targets, path_cap, n_slots=None, want_tree=False, want_gen=False):
    """One scn_sssp_paths launch on a _DeviceGraph: sources (n_jobs,), targets (n_jobs, n_targets) with -1 = none.  Returns a
    dict of device tensors: path (n_jobs, n_targets, path_cap) int32 (-1 where not written), path_len, dist, and dist_all /
    pred_all (want_tree) and n_gen (want_gen)."""
    import torch
    from . import _lib, ops
    src = np.ascontiguousarray(sources, np.int32).ravel()
    tgt = np.ascontiguousarray(targets, np.int32).reshape(len(src), -1)
    n_jobs, n_t, n, dev = len(src), tgt.shape[1], graph.n_nodes, graph.device
    if not 1 <= n_t <= _lib.SCN_SSSP_MAX_TARGETS:
        raise ValueError("1 .. %d targets per job, got %d" % (_lib.SCN_SSSP_MAX_TARGETS, n_t))
    if n_jobs and (src.min() < 0 or src.max() >= n or tgt.min() < -1 or tgt.max() >= n):
        raise ValueError("a source or target lies outside the graph's %d nodes" % n)
    path_cap = int(path_cap)
    if path_cap < 1:
        raise ValueError("path_cap must be at least 1")
    lib = _lib.load()
    n_slots = graph.n_slots(n_jobs) if n_slots is None else int(n_slots)
    out = {"path": torch.full((n_jobs, n_t, path_cap), -1, dtype=torch.int32, device=dev),
           "path_len": torch.zeros((n_jobs, n_t), dtype=torch.int32, device=dev),
           "dist": torch.empty((n_jobs, n_t), dtype=torch.float64, device=dev)}
    if want_tree:
        out["dist_all"] = torch.empty((n_jobs, n), dtype=torch.float64, device=dev)
        out["pred_all"] = torch.empty((n_jobs, n), dtype=torch.int32, device=dev)
    if want_gen:
        out["n_gen"] = torch.zeros((n_jobs,), dtype=torch.int32, device=dev)
    if n_jobs == 0:
        return out
    d_src, d_tgt = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    ws, ws_bytes = ops._workspace(int(lib.scn_sssp_slot_bytes(n)) * n_slots, dev)
    opt = lambda name, dtype: ops._dev(out[name], dtype) if name in out else None      # an optional array: NULL when not asked for
    with torch.cuda.device(dev):
        _lib.check(lib.scn_sssp_paths(
            n, ops._dev(graph.adj_ptr, torch.int32), ops._dev(graph.adj, torch.int32),
            None if graph.adj_w is None else ops._dev(graph.adj_w, torch.float64), n_jobs, ops._dev(d_src, torch.int32),
            ops._dev(d_tgt, torch.int32), n_t, path_cap, ops._dev(out["path"], torch.int32), ops._dev(out["path_len"], torch.int32),
            ops._dev(out["dist"], torch.float64), opt("dist_all", torch.float64), opt("pred_all", torch.int32), opt("n_gen", torch.int32),
            ws, ws_bytes, n_slots, ops._stream()), "scn_sssp_paths")
    return out


def walk_assemble_device(path, path_len, walk_cap):
    """scn_walk_assemble on the (2 n, 2, path_cap) paths and (2 n, 2) lengths of n attempts (device tensors): (walk (n,
    walk_cap) int32, -1 where not written, walk_len (n,) int32) on the device."""
    import torch
    from . import _lib, ops
    n, path_cap, dev = path.shape[0] // 2, int(path.shape[2]), path.device
    if path.shape[0] != 2 * n or path.shape[1] != 2 or tuple(path_len.shape) != (2 * n, 2):
        raise ValueError("two jobs of two targets per attempt")
    if not 1 <= int(walk_cap) <= _lib.SCN_WALK_MAX:
        raise ValueError("walk_cap must lie in 1 .. %d, got %d" % (_lib.SCN_WALK_MAX, walk_cap))
    walk = torch.full((n, int(walk_cap)), -1, dtype=torch.int32, device=dev)
    walk_len = torch.zeros((n,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().scn_walk_assemble(n, ops._dev(path, torch.int32), ops._dev(path_len, torch.int32), path_cap,
                                                 ops._dev(walk, torch.int32), ops._dev(walk_len, torch.int32), int(walk_cap),
                                                 ops._stream()), "scn_walk_assemble")
    return walk, walk_len


def initial_path_cap(n_nodes):
    """Where path_cap starts: min(V, max(64, 8 ceil(sqrt(V)))) -- a shortest path of a planar Delaunay complex has O(sqrt V) nodes."""
    return int(min(n_nodes, max(64, 8 * int(np.ceil(np.sqrt(n_nodes))))))


def shortest_paths_device(cx, sources, targets, metric="hops", device=None, want_tree=False):
    """Shortest paths from sources[j] to targets[j] (one target per job, or a row of up to two with -1 = none) on the device.
    cx: a Complex, or an (adj_ptr, adj, adj_w) triple.  Returns ((ptr, nodes), path_len, dist[, (dist_all, pred_all)]) as NumPy
    arrays: path j * n_targets + t is nodes[ptr[..] : ptr[.. + 1]], source to target inclusive (empty where path_len, shaped
    (n_jobs, n_targets), is 0 = no target or -1 = unreachable); dist is inf there.  path_cap starts at initial_path_cap(V);
    the jobs that report -2 are run again with the cap doubled, up to V."""
    graph = device_graph(cx, metric, device)
    src = np.asarray(sources, np.int64).ravel()
    tgt = np.asarray(targets, np.int64).reshape(len(src), -1)
    n_jobs, n_t, n = len(src), tgt.shape[1], graph.n_nodes
    cap = initial_path_cap(n)
    out = sssp_paths_device(graph, src, tgt, cap, want_tree=want_tree)
    path_len, dist = out["path_len"].cpu().numpy(), out["dist"].cpu().numpy()
    lens = np.maximum(path_len, 0).ravel()
    used = int(lens.max()) if lens.size else 0
    flat = out["path"].reshape(n_jobs * n_t, cap)[:, :max(used, 1)].cpu().numpy()
    segs = {i: flat[i, :lens[i]].astype(np.int64) for i in np.flatnonzero(lens)}
    redo = np.flatnonzero((path_len == -2).any(axis=1))
    while len(redo):
        if cap >= n:
            raise RuntimeError("a path does not fit %d nodes" % n)       # a simple path cannot be longer
        cap = min(2 * cap, n)
        again = sssp_paths_device(graph, src[redo], tgt[redo], cap)
        pl, pa, di = again["path_len"].cpu().numpy(), again["path"].cpu().numpy(), again["dist"].cpu().numpy()
        path_len[redo], dist[redo] = pl, di
        for r, j in enumerate(redo):
            for t in range(n_t):
                if pl[r, t] > 0:
                    segs[j * n_t + t] = pa[r, t, :pl[r, t]].astype(np.int64)
        redo = redo[(pl == -2).any(axis=1)]
    if np.any(path_len == -3):
        raise RuntimeError("a job's frontier was not empty after %d generations" % n)
    lens = np.maximum(path_len, 0).ravel()
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nodes = np.concatenate([segs[i] for i in np.flatnonzero(lens)]) if lens.any() else np.zeros(0, np.int64)
    res = ((ptr, nodes), path_len, dist)
    if want_tree:
        res += ((out["dist_all"].cpu().numpy(), out["pred_all"].cpu().numpy().astype(np.int64)),)
    return res


def walk_regions(cx):
    """(BEGIN, END, [A_0, A_1, A_2], [B_0, B_1, B_2]): the node sets the waypoints of a walk are drawn from (SDG:207-218), as
    generate_random_walks forms them inline (that function is left as it was)."""
    pts, valid = cx.coords, cx.valid_idxs
    s = np.sum(pts[valid], axis=1)
    BEGIN, END = valid[s < 1 / 4], valid[s > 7 / 4]
    A012 = valid[(s > 1 / 4) & (s < 1)]
    B012 = valid[(s < 7 / 4) & (s > 1)]

    def regions(X):
        d = pts[X, 1] - pts[X, 0]
        return [X[(d < 1 / 2) & (d > -1 / 2)], X[d > 1 / 2], X[d < -1 / 2]]
    return BEGIN, END, regions(A012), regions(B012)


def _attempts_host(graph, way):
    """The walks of the attempts way (n, 4) = (v_begin, v_1, v_2, v_end) on shortest_path_tree_host: a node list, or None where
    a segment is unreachable or the walk repeats a node."""
    trees, out = {}, []

    def tree(v):
        if v not in trees:
            trees[v] = shortest_path_tree_host(*graph, v)[1]
        return trees[v]
    for v_begin, v_1, v_2, v_end in way.tolist():
        t1, t2 = tree(v_1), tree(v_2)
        p_a, p_b, p_c = _tree_path(t1, v_1, v_begin), _tree_path(t1, v_1, v_2), _tree_path(t2, v_2, v_end)
        walk = None
        if p_a is not None and p_b is not None and p_c is not None:
            walk = p_a[::-1][:-1] + p_b[:-1] + p_c                        # SDG:236-238
            if len(walk) != len(set(walk)):                               # SDG:239
                walk = None
        out.append(walk)
    return out


def _attempts_device(graph, way, stats=None):
    """The same on the device: two scn_sssp_paths jobs per attempt, then scn_walk_assemble."""
    from . import _lib
    n = len(way)
    src = way[:, [1, 2]].reshape(-1)
    tgt = np.stack([way[:, [0, 2]], np.stack([way[:, 3], np.full(n, -1)], axis=1)], axis=1).reshape(2 * n, 2)
    cap = initial_path_cap(graph.n_nodes)
    while True:
        out = sssp_paths_device(graph, src, tgt, cap, want_gen=stats is not None)
        path_len = out["path_len"].cpu().numpy().astype(np.int64)
        if stats is not None:
            stats["trees"] = stats.get("trees", 0) + 2 * n
            stats["generations"] = stats.get("generations", 0) + int(out["n_gen"].sum().item())
        if np.any(path_len == -3):
            raise RuntimeError("a job's frontier was not empty after %d generations" % graph.n_nodes)
        if not np.any(path_len == -2):
            break
        if cap >= graph.n_nodes:
            raise RuntimeError("a path does not fit %d nodes" % graph.n_nodes)
        cap = min(2 * cap, graph.n_nodes)                                 # the whole round again: rare, and it keeps one layout
    seg = path_len.reshape(n, 4)[:, :3]
    total = np.where((seg > 0).all(axis=1), seg.sum(axis=1) - 2, 0)
    longest = int(total.max()) if n else 0
    if longest > _lib.SCN_WALK_MAX:
        raise RuntimeError("a walk of %d nodes is longer than the %d the repeat test holds" % (longest, _lib.SCN_WALK_MAX))
    walk, walk_len = walk_assemble_device(out["path"], out["path_len"], max(longest, 1))
    walk, walk_len = walk.cpu().numpy(), walk_len.cpu().numpy()
    return [walk[i, :walk_len[i]].tolist() if walk_len[i] > 0 else None for i in range(n)]


def generate_random_walks_batched(cx, m=1000, seed=1030, metric="hops", backend="device", device=None, return_waypoints=False,
                                  stats=None):
    """SDG:178-243 without a waypoint pool, in rounds: walk slot j has the region r = j % 3 (the reference's i % 3 over accepted
    walks gives the same assignment).  A round draws (v_begin, v_1, v_2, v_end) for every unfilled slot from ONE
    RandomState(seed) on the host, in slot order and in the reference's order of calls, builds all of their walks at once --
    backend="device": scn_sssp_paths + scn_walk_assemble; backend="host": the same round logic on shortest_path_tree_host --
    and keeps the accepted ones; the next round retries the slots still empty.  Both backends give identical walks for a seed.
    RuntimeError once the attempts pass generate_random_walks' limit of 50 m + 1000.  Returns the list of node lists (and the
    (m, 4) waypoints with return_waypoints); `stats`, a dict, receives rounds, attempts, accepted (and trees, generations on
    the device)."""
    if backend not in ("device", "host"):
        raise ValueError("backend must be 'device' or 'host', got %r" % (backend,))
    rs = np.random.RandomState(seed)
    BEGIN, END, A, B = walk_regions(cx)
    graph = device_graph(cx, metric, device) if backend == "device" else csr_adjacency(cx, metric)
    walks, ways = [None] * m, np.zeros((m, 4), np.int64)
    tries, rounds = 0, 0
    while True:
        todo = [j for j in range(m) if walks[j] is None]
        if not todo:
            break
        tries += len(todo)
        if tries > 50 * m + 1000:
            raise RuntimeError("could not generate enough simple walks")
        rounds += 1
        way = np.zeros((len(todo), 4), np.int64)
        for i, j in enumerate(todo):
            r = j % 3
            way[i, 0] = rs.choice(BEGIN)
            way[i, 1], way[i, 2] = rs.choice(A[r]), rs.choice(B[r])
            way[i, 3] = rs.choice(END)
        got = _attempts_device(graph, way, stats) if backend == "device" else _attempts_host(graph, way)
        for i, j in enumerate(todo):
            if got[i] is not None:
                walks[j], ways[j] = got[i], way[i]
    if stats is not None:
        stats.update(rounds=rounds, attempts=tries, accepted=m)
    return (walks, ways) if return_waypoints else walks
