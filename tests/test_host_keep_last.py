"""The keep mask of the last layer's forward (ops.KEEP_LAST) without a GPU: ops.keep_mask_host -- the NumPy restatement of
scn_keep_mask that tests/test_gpu_keep_last.py compares the kernel with -- against brute force over the readout's own tables: the rows
a leaf's readout reads are the edges incident to a neighbour of its node, a row belongs to the plan block whose row range holds it,
and bit (block, slab) is set iff some leaf of the slab reads a row of the block.  Plus the new exports."""
import numpy as np

from oracle import scone_oracle as so
from scone_gcn_amd import _lib, ops

NS = 4


def _tables():
    from scone_gcn_amd import synthetic_data_gen as g
    cx = g.random_SC_graph(300)
    E = len(cx.edges)
    row0 = np.append(np.arange(0, E, 16), E)            # a synthetic plan: a block every 16 rows, the last one short
    assert 0 < row0[-1] - row0[-2] < 16
    nbr, _ = so.neighborhoods(cx.edges, cx.n_nodes)
    inc_ptr, inc_edge, _, _ = so.incidence_csr(cx.edges, cx.n_nodes)
    # (the pattern only feeds the block adjacency, which the mask does not use: an empty one will do)
    (top_ptr, top_blk), _ = ops.field_tables(row0, (np.zeros(E + 1, np.int64), np.zeros(0, np.int64)), nbr, inc_ptr, inc_edge)
    return cx, row0, np.asarray(nbr), np.asarray(inc_ptr), np.asarray(inc_edge), top_ptr, top_blk


def _brute(nodes, row0, nbr, inc_ptr, inc_edge):
    n_blocks, n_slabs = len(row0) - 1, -(-len(nodes) // NS)
    bits = np.zeros((n_blocks, n_slabs), bool)
    for i, v in enumerate(nodes):
        for u in nbr[v]:
            if u >= 0:
                for e in inc_edge[inc_ptr[u]:inc_ptr[u + 1]]:
                    bits[np.searchsorted(row0, e, side="right") - 1, i // NS] = True
    return bits


def _unpack(mask, n_slabs):
    return ((mask[:, np.arange(n_slabs) >> 5] >> (np.arange(n_slabs) & 31).astype(np.uint32)) & 1).astype(bool)


def _check(nodes, tabs):
    cx, row0, nbr, inc_ptr, inc_edge, top_ptr, top_blk = tabs
    n_slabs = -(-len(nodes) // NS)
    mask = ops.keep_mask_host(nodes, NS, top_ptr, top_blk, len(row0) - 1)
    assert mask.dtype == np.uint32 and mask.shape == (len(row0) - 1, (n_slabs + 31) // 32)
    want = _brute(nodes, row0, nbr, inc_ptr, inc_edge)
    assert np.array_equal(_unpack(mask, n_slabs), want)
    # no bit beyond the last slab
    full = _unpack(mask, 32 * mask.shape[1])
    assert not full[:, n_slabs:].any()
    return want


def test_mask_of_random_nodes_equals_brute_force():
    tabs = _tables()
    rs = np.random.RandomState(0)
    for n in (4, 128, 132, 131):                        # 1, 32 and 33 slabs (a second word), and a last slab that is not full
        want = _check(rs.randint(0, tabs[0].n_nodes, size=n), tabs)
        assert want.any() and not want.all()


def test_a_node_repeated_inside_a_slab_sets_its_bits_once():
    tabs = _tables()
    v = int(np.argmax((tabs[2] >= 0).sum(axis=1)))      # a node of maximal degree
    one = _check(np.array([v, 5, 5, 7]), tabs)
    rep = _check(np.array([v, v, v, v, 5, 5, 7, 7]), tabs)
    assert np.array_equal(rep[:, 0], _check(np.array([v]), tabs)[:, 0])
    assert np.array_equal(rep[:, 0] | rep[:, 1], one[:, 0])


def test_slabs_whose_four_leaves_share_no_block():
    """Four leaves far apart in each of two slabs: their block sets are pairwise disjoint and the slab's bits are their disjoint union."""
    tabs = _tables()
    cx, row0, nbr, inc_ptr, inc_edge, top_ptr, top_blk = tabs
    T = [set(top_blk[top_ptr[v]:top_ptr[v + 1]].tolist()) for v in range(cx.n_nodes)]

    def disjoint4(order):                               # greedy: four nodes whose block sets are pairwise disjoint
        got = []
        for v in order:
            if T[v] and all(not (T[v] & T[u]) for u in got):
                got.append(v)
            if len(got) == 4:
                return got
        raise AssertionError("the complex has four nodes with pairwise disjoint block sets")
    pick = disjoint4(range(cx.n_nodes)) + disjoint4(range(cx.n_nodes - 1, -1, -1))
    want = _check(np.array(pick), tabs)
    for s in range(2):
        assert want[:, s].sum() == sum(len(T[v]) for v in pick[4 * s:4 * s + 4])


def test_a_node_outside_the_table_contributes_nothing():
    tabs = _tables()
    top_ptr, top_blk = tabs[5], tabs[6]
    nb = len(tabs[1]) - 1
    a = ops.keep_mask_host(np.array([3, -1, tabs[0].n_nodes, 9]), NS, top_ptr, top_blk, nb)
    b = ops.keep_mask_host(np.array([3, 9]), NS, top_ptr, top_blk, nb)
    assert np.array_equal(a, b)


def test_switch_threshold_and_signatures_exist():
    assert ops.KEEP_LAST is True
    assert ops.SconePlan.KEEP_LAST_MIN_BYTES == ops.SconePlan.SMALL_DZ_BYTES
    for name in ("scn_keep_mask", "scn_conv_forward_keep", "scn_conv_forward_from_y_keep"):
        assert name in _lib.SIGNATURES
