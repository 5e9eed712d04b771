"""Field-of-view work lists of multi-hop prediction without a GPU: the two block tables (ops.field_tables) against dense-matrix
brute force, the closure property they exist for on the fp64 oracle's layers (whatever lies outside the lists may hold NaN and the
leaf's log-probabilities do not move by a bit), this file's numpy restatement of scn_field_lists (tests/test_gpu_field.py compares
the kernel with it), and the new exports and keyword."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import scone_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "scone_gcn_amd", "libscone_hip.so")


# ------------------------------------------------------------------------------------------------------------------
# numpy restatement of scn_field_lists (include/scone_hip.h)
# ------------------------------------------------------------------------------------------------------------------

def np_field_lists(n, ns, node, n_nodes, top, adj, n_blocks, n_levels, cap):
    """Per level l < n_levels (level n_levels - 1 = top, level 0 = input) a dict: counts = (n_work, items) and -- unless the level
    is empty or items > cap, when nothing but the counts is written -- block [n_work], ptr [n_work + 1], slab [items] in canonical
    order: blocks ascending, blocks without a slab left out, each block's slabs ascending.  Leaf i belongs to slab i // ns; a node
    outside [0, n_nodes) contributes nothing."""
    (top_ptr, top_blk), (adj_ptr, adj_blk) = top, adj
    n_slabs = max(1, -(-n // ns))
    mark = np.zeros((n_levels, n_blocks, n_slabs), bool)
    for i in range(n):
        v = int(node[i])
        if 0 <= v < n_nodes:
            mark[n_levels - 1, top_blk[top_ptr[v]:top_ptr[v + 1]], i // ns] = True
    for l in range(n_levels - 2, -1, -1):
        for b in np.flatnonzero(mark[l + 1].any(axis=1)):
            mark[l, adj_blk[adj_ptr[b]:adj_ptr[b + 1]]] |= mark[l + 1, b]
    out = []
    for l in range(n_levels):
        cnt = mark[l].sum(axis=1)
        blocks = np.flatnonzero(cnt > 0)
        lvl = {"counts": (len(blocks), int(cnt.sum()))}
        if len(blocks) and cnt.sum() <= cap:
            lvl["block"] = blocks.astype(np.int32)
            lvl["ptr"] = np.concatenate([[0], np.cumsum(cnt[blocks])]).astype(np.int32)
            lvl["slab"] = np.concatenate([np.flatnonzero(mark[l, b]) for b in blocks]).astype(np.int32)
        out.append(lvl)
    return out


def random_tables(rs, n_nodes, n_blocks, top_max=4, adj_max=3):
    """Random CSR tables in the form of ops.field_tables: ascending blocks per row, A with self; T(0) holds the last block."""
    def csr(rows, pick):
        ptr, idx = [0], []
        for r in range(rows):
            idx += sorted(pick(r))
            ptr.append(len(idx))
        return np.asarray(ptr, np.int32), np.asarray(idx, np.int32)
    top = csr(n_nodes, lambda v: set(rs.randint(0, n_blocks, size=rs.randint(0, top_max + 1)).tolist()) | ({n_blocks - 1} if v == 0 else set()))
    adj = csr(n_blocks, lambda b: set(rs.randint(0, n_blocks, size=rs.randint(0, adj_max + 1)).tolist()) | {b})
    return top, adj


# ------------------------------------------------------------------------------------------------------------------
# the tables
# ------------------------------------------------------------------------------------------------------------------

def _complex(one_sided=False):
    from scone_gcn_amd import synthetic_data_gen as g
    cx = g.random_SC_graph(300)
    B1, B2 = (m.toarray() for m in g.incidence_matrices(cx))
    L_lo, L_up = so.scone_shifts(B1, B2)
    if one_sided:                                       # strictly upper triangular: not symmetric, and no diagonal entry
        L_lo, L_up = np.triu(L_lo, 1), np.triu(L_up, 1)
    E = B1.shape[1]
    row0 = np.append(np.arange(0, E, 16), E)            # a synthetic plan: a block every 16 rows, the last one short
    nbr, D = so.neighborhoods(cx.edges, cx.n_nodes)
    inc_ptr, inc_edge, inc_sign, _ = so.incidence_csr(cx.edges, cx.n_nodes)
    return cx, B1, L_lo, L_up, row0, nbr, (inc_ptr, inc_edge, inc_sign)


def _rows_of(ptr, idx, r):
    return idx[ptr[r]:ptr[r + 1]]


@pytest.mark.parametrize("one_sided", [False, True])
def test_field_tables_match_dense_brute_force(one_sided):
    from scone_gcn_amd import ops
    cx, B1, L_lo, L_up, row0, nbr, inc = _complex(one_sided)
    E, V, nb = B1.shape[1], cx.n_nodes, len(row0) - 1
    assert E % 16 != 0 and nb > 20
    pattern = (abs(sp.csr_matrix(L_lo)) + abs(sp.csr_matrix(L_up))).tocsr()
    (top_ptr, top_blk), (adj_ptr, adj_blk) = ops.field_tables(row0, pattern, nbr, inc[0], inc[1])
    assert all(a.dtype == np.int32 for a in (top_ptr, top_blk, adj_ptr, adj_blk))
    in_blk = np.zeros((E, nb))
    in_blk[np.arange(E), np.arange(E) // 16] = 1
    P = ((np.abs(L_lo) + np.abs(L_up)) != 0).astype(float)
    A = (in_blk.T @ P @ in_blk + np.eye(nb)) > 0                              # rows of b read columns in b', b itself included
    N = np.zeros((V, V))
    for v in range(V):
        N[v, nbr[v][nbr[v] >= 0]] = 1
    T = (N @ (B1 != 0).astype(float) @ in_blk) > 0                            # edges incident to a neighbour of v
    assert len(adj_ptr) == nb + 1 and len(top_ptr) == V + 1
    for b in range(nb):
        assert np.array_equal(_rows_of(adj_ptr, adj_blk, b), np.flatnonzero(A[b])), b
    for v in range(V):
        assert np.array_equal(_rows_of(top_ptr, top_blk, v), np.flatnonzero(T[v])), v
    if one_sided:
        assert not np.array_equal(A, A.T)
    # (rowptr, cols) is taken like a scipy matrix, and an explicitly stored zero is part of the pattern
    again = ops.field_tables(row0, (pattern.indptr, pattern.indices), nbr, inc[0], inc[1])
    assert all(np.array_equal(x, y) for p, q in zip(again, ((top_ptr, top_blk), (adj_ptr, adj_blk))) for x, y in zip(p, q))
    far = int(np.flatnonzero(~A[0])[-1])
    coo = pattern.tocoo()
    stored = sp.csr_matrix((np.append(coo.data, 0.0), (np.append(coo.row, 0), np.append(coo.col, far * 16))), shape=pattern.shape)
    assert stored.nnz == pattern.nnz + 1
    _, (p2, b2) = ops.field_tables(row0, stored, nbr, inc[0], inc[1])
    assert far in _rows_of(p2, b2, 0)


# ------------------------------------------------------------------------------------------------------------------
# the closure property on the oracle's layers
# ------------------------------------------------------------------------------------------------------------------

def _sparse_readout(Bconds, v, H, w_last):
    """The oracle's readout (logits = Bcond(v) @ H @ W_last, log-softmax over all D slots) with Bcond(v) as a sparse matrix, so
    that only the rows it has entries in are read."""
    logits = (sp.csr_matrix(Bconds(v)) @ H) @ w_last
    return logits - so.logsumexp(logits, axis=0)


@pytest.mark.parametrize("one_sided", [False, True])
def test_nothing_outside_the_lists_is_read(one_sided):
    """3 layers; after every layer each block NOT in that layer's list is overwritten with NaN, and so is x outside list_0: the
    leaf's log-probabilities stay finite and equal the unrestricted run bit for bit.  Sparse shifts and a sparse readout operand,
    so that a product touches stored entries only -- as the kernels do."""
    from scone_gcn_amd import ops
    cx, B1, L_lo, L_up, row0, nbr, inc = _complex(one_sided)
    E, nb, L = B1.shape[1], len(row0) - 1, 3
    S_lo, S_up = sp.csr_matrix(L_lo), sp.csr_matrix(L_up)
    top, adj = ops.field_tables(row0, (abs(S_lo) + abs(S_up)).tocsr(), nbr, inc[0], inc[1])
    Bconds = so.make_Bconds(B1, nbr)
    rs = np.random.RandomState(5)
    w = [0.5 * rs.randn(*s) for s in so.weight_shapes(1, [(3, 8)] * L, 1)]
    layer = lambda l, H: so.conv_forward(w[3 * l:3 * l + 3] + [None], S_lo, S_up, H)
    blk_of = np.arange(E) // 16
    nodes = rs.choice(cx.n_nodes, size=20, replace=False)
    smallest, top_most = 1.0, 0.0
    for v in nodes:
        lists = np_field_lists(1, 1, [v], cx.n_nodes, top, adj, nb, L + 1, nb)
        keep = [np.isin(blk_of, lv.get("block", [])) for lv in lists]                # rows of the listed blocks, per level
        smallest, top_most = min(smallest, keep[0].mean()), max(top_most, keep[L].mean())
        x = rs.randn(1, E, 1)                                                # every edge non-zero: no exact zero hides a read
        H, Hr = x, np.where(keep[0][None, :, None], x, np.nan)
        for l in range(L):
            H, Hr = layer(l, H), layer(l, Hr)
            Hr = np.where(keep[l + 1][None, :, None], Hr, np.nan)
            assert np.array_equal(H[0][keep[l + 1]], Hr[0][keep[l + 1]])     # the listed items hold the dense values
        want, got = _sparse_readout(Bconds, v, H[0], w[-1]), _sparse_readout(Bconds, v, Hr[0], w[-1])
        assert np.isfinite(got).all() and np.array_equal(want, got), v
    assert smallest < 0.8 and top_most < 0.5                                 # the lists do leave something out, at every level


# ------------------------------------------------------------------------------------------------------------------
# the restatement itself
# ------------------------------------------------------------------------------------------------------------------

def test_restatement_is_canonical_and_matches_set_arithmetic():
    rs = np.random.RandomState(11)
    n_nodes, nb, ns, n_levels = 9, 23, 4, 4
    top, adj = random_tables(rs, n_nodes, nb)
    node = rs.randint(-1, n_nodes, size=13)
    node[5] = n_nodes + 3                                                    # out of range: contributes nothing
    got = np_field_lists(len(node), ns, node, n_nodes, top, adj, nb, n_levels, 10 ** 6)
    for s in range(-(-len(node) // ns)):
        cur = set()
        for i in range(ns * s, min(ns * s + ns, len(node))):
            if 0 <= node[i] < n_nodes:
                cur |= set(_rows_of(*top, node[i]).tolist())
        for l in range(n_levels - 1, -1, -1):
            lv = got[l]
            listed = {int(b) for u, b in enumerate(lv.get("block", [])) if s in lv["slab"][lv["ptr"][u]:lv["ptr"][u + 1]]}
            assert listed == cur, (s, l)
            cur = set().union(*[set(_rows_of(*adj, b).tolist()) for b in cur]) if cur else set()
    for lv in got:
        if "block" in lv:
            assert np.all(np.diff(lv["block"]) > 0) and np.all(np.diff(lv["ptr"]) > 0)
            assert all(np.all(np.diff(lv["slab"][a:b]) > 0) for a, b in zip(lv["ptr"][:-1], lv["ptr"][1:]))
            assert lv["counts"] == (len(lv["block"]), len(lv["slab"])) and lv["ptr"][-1] == len(lv["slab"])
    # a level over cap and an empty level keep their counts and nothing else
    items = got[0]["counts"][1]
    short = np_field_lists(len(node), ns, node, n_nodes, top, adj, nb, n_levels, items - 1)
    assert short[0] == {"counts": got[0]["counts"]}
    dead = np_field_lists(4, ns, [-1] * 4, n_nodes, top, adj, nb, 2, 100)
    assert dead == [{"counts": (0, 0)}] * 2


# ------------------------------------------------------------------------------------------------------------------
# exports, keyword, switch
# ------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported():
    if not os.path.exists(LIB):
        subprocess.check_call(["bash", os.path.join(ROOT, "scone_gcn_amd", "csrc", "build.sh")])
    lib = ctypes.CDLL(LIB)
    for name in ("scn_field_lists_workspace", "scn_field_lists", "scn_tree_slabs_list"):
        assert hasattr(lib, name), "missing export " + name
    lib.scn_field_lists_workspace.restype = ctypes.c_size_t
    assert lib.scn_field_lists_workspace(0, 1, 1) == 0 and lib.scn_field_lists_workspace(1 << 20, 1 << 10, 4) == 0
    need = lib.scn_field_lists_workspace(65, 3, 4)
    assert need >= 65 * 3 * 4 + 2 * 4 * 65 * 4
    # argument checks come before anything touches a device
    assert lib.scn_field_lists(4, 4, None, 1, None, None, 1, None, None, 2, None, None, None, ctypes.c_int64(0), None, None,
                               ctypes.c_size_t(0), None) == -1
    assert lib.scn_field_lists(-1, 4, None, 1, None, None, 1, None, None, 2, None, None, None, ctypes.c_int64(0), None, None,
                               ctypes.c_size_t(0), None) == -2
    assert lib.scn_tree_slabs_list(None, 0, 1, 0, None, None, None, 1, None, 1, 4, None, None, None) == -1


def test_multi_hop_skip_keyword_and_switch():
    from scone_gcn_amd import trajectory_experiments as te
    from scone_gcn_amd.scone_trajectory_model import Scone_GCN
    assert Scone_GCN(1, 1e-3, 4, 0.0, verbose=False).multi_hop_skip == "dense"
    assert Scone_GCN(1, 1e-3, 4, 0.0, verbose=False, multi_hop_skip="field").multi_hop_skip == "field"
    for bad in ("zeros", "Field", None, 1):
        with pytest.raises(ValueError, match="multi_hop_skip"):
            Scone_GCN(1, 1e-3, 4, 0.0, verbose=False, multi_hop_skip=bad)
    assert te.hyperparams(["prog"])["multi_hop_skip"] == "dense"
    assert te.hyperparams(["prog", "-multi_hop_skip", "field", "-beam", "4"])["multi_hop_skip"] == "field"
