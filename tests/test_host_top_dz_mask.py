"""The source mask of the top layer's backward (ops.TOP_DZ_MASK) without a GPU: ops.mask_hop_host -- the NumPy restatement of
scn_mask_hop that tests/test_gpu_top_dz_mask.py compares the kernel with -- against brute force over ROWS.  Block b of the backward
stages the blocks holding a column of one of its rows (the row itself included: the identity shift); the readout's gradient lives on
the readout rows of each trajectory (the edges incident to a neighbour of its last node).  So bit (b, s) must be set wherever some
pattern column of a row of b is a readout row of a trajectory of slab s -- a superset is all correctness needs -- and it must equal
the OR of the keep mask over A(b), which is what the kernel computes.  Plus the new exports and the switch."""
import numpy as np
import pytest

from oracle import scone_oracle as so
from scone_gcn_amd import _lib, ops

NS = 4
_TABLES = {}


def _tables(n_points, rows_per_block):
    """random_SC_graph(n_points) in its natural edge order under a synthetic plan (a block every rows_per_block rows, the last one
    short), the stored pattern of the two scone shifts (B1^T B1 and B2 B2^T, sparse), and both block tables."""
    key = (n_points, rows_per_block)
    if key not in _TABLES:
        from scone_gcn_amd import synthetic_data_gen as g
        cx = g.random_SC_graph(n_points)
        E = len(cx.edges)
        row0 = np.append(np.arange(0, E, rows_per_block), E)
        assert 0 < row0[-1] - row0[-2] < rows_per_block, "the plan is meant to end in a short block"
        B1, B2 = g.incidence_matrices(cx)
        pat = ((abs(B1.T @ B1) + abs(B2 @ B2.T)) != 0).tocsr()
        pat.sort_indices()
        nbr, _ = so.neighborhoods(cx.edges, cx.n_nodes)
        inc_ptr, inc_edge, _, _ = so.incidence_csr(cx.edges, cx.n_nodes)
        (top_ptr, top_blk), (adj_ptr, adj_blk) = ops.field_tables(row0, pat, nbr, inc_ptr, inc_edge)
        _TABLES[key] = dict(cx=cx, E=E, row0=row0, pat=pat, nbr=np.asarray(nbr), inc_ptr=np.asarray(inc_ptr),
                            inc_edge=np.asarray(inc_edge), top=(top_ptr, top_blk), adj=(adj_ptr, adj_blk))
    return _TABLES[key]


def _unpack(mask, n_slabs):
    return ((mask[:, np.arange(n_slabs) >> 5] >> (np.arange(n_slabs) & 31).astype(np.uint32)) & 1).astype(bool)


def _readout_rows(t, nodes):
    """bool [n_slabs][E]: the rows the readout of some leaf of the slab touches; a node outside the table has none."""
    n_slabs = -(-len(nodes) // NS)
    rows = np.zeros((n_slabs, t["E"]), bool)
    for i, v in enumerate(nodes):
        if 0 <= v < t["cx"].n_nodes:
            for u in t["nbr"][v]:
                if u >= 0:
                    rows[i // NS, t["inc_edge"][t["inc_ptr"][u]:t["inc_ptr"][u + 1]]] = True
    return rows


def _check(t, nodes):
    row0, pat = t["row0"], t["pat"]
    nb, n_slabs = len(row0) - 1, -(-len(nodes) // NS)
    m0 = ops.keep_mask_host(nodes, NS, *t["top"], nb)
    got = ops.mask_hop_host(m0, *t["adj"])
    assert got.dtype == np.uint32 and got.shape == m0.shape == (nb, (n_slabs + 31) // 32)
    bits = _unpack(got, n_slabs)
    assert not _unpack(got, 32 * got.shape[1])[:, n_slabs:].any(), "no bit beyond the last slab"
    blk_of = np.searchsorted(row0, np.arange(t["E"]), side="right") - 1
    rows = _readout_rows(t, nodes)
    # rows: bit (b, s) wherever a column of a row of b (or the row itself) is a readout row of slab s
    need = np.zeros((nb, n_slabs), bool)
    for r in range(t["E"]):
        cols = np.append(pat.indices[pat.indptr[r]:pat.indptr[r + 1]], r)
        need[blk_of[r]] |= rows[:, cols].any(axis=1)
    assert not (need & ~bits).any(), "an item with a non-zero source is outside the mask"
    # blocks: exactly the OR of the keep mask over A(b), with A(b) rebuilt here from the rows
    k0 = _unpack(m0, n_slabs)
    want = np.zeros((nb, n_slabs), bool)
    for r in range(t["E"]):
        for c in np.append(pat.indices[pat.indptr[r]:pat.indptr[r + 1]], r):
            want[blk_of[r]] |= k0[blk_of[c]]
    assert np.array_equal(bits, want)
    return k0, bits


@pytest.mark.parametrize("n_points,rows_per_block", [(400, 16), (2000, 64)])
def test_hopped_mask_covers_every_source_and_equals_the_or_over_the_adjacency(n_points, rows_per_block):
    t = _tables(n_points, rows_per_block)
    rs = np.random.RandomState(n_points)
    for n in (4, 128, 132, 131):                        # 1, 32 and 33 slabs (a second word), and a last slab that is not full
        k0, bits = _check(t, rs.randint(0, t["cx"].n_nodes, size=n))
        assert k0.any() and not bits.all()
        assert not (k0 & ~bits).any() and (bits & ~k0).any(), "one hop out: the keep mask and more"


def test_a_node_outside_the_table_contributes_nothing():
    t = _tables(400, 16)
    V = t["cx"].n_nodes
    _, a = _check(t, np.array([3, -1, V, 9, 2 ** 31 - 1, V + 5, -(2 ** 31), 11]))
    _, b = _check(t, np.array([3, 9, 11]))
    assert np.array_equal(a[:, 0] | a[:, 1], b[:, 0])


def test_a_block_outside_the_mask_contributes_nothing():
    m = np.array([[1], [2], [4]], np.uint32)
    adj_ptr, adj_blk = np.array([0, 2, 5, 6]), np.array([0, 7, 1, -1, 2, 3])
    assert np.array_equal(ops.mask_hop_host(m, adj_ptr, adj_blk), np.array([[1], [6], [0]], np.uint32))


def test_switch_and_signatures_exist():
    assert isinstance(ops.TOP_DZ_MASK, bool), "a bool, so that tools/bench_switch.py TOP_DZ_MASK=0 can set it"
    for name in ("scn_mask_hop", "scn_conv_backward_dzmask"):
        assert name in _lib.SIGNATURES
