"""The visit tables and masks of the cone step's backwards without a GPU (ops.visit_tables, ops.visit_masks_host).

dZ_L is non-zero only on the rows R0 the readout's backward writes, so the backward k layers down gathers a non-zero only on R_k =
P^k R0 (P: the operator's stored pattern with the diagonal, rows read columns) and the items it has to visit are V_k = the (block, slab)
items holding a row of R_k.  Here, against brute force over rows -- dense P, explicit R_k per last node:
  * the tables T_k(v) = blocks(P^k rows(v));
  * visit_masks_host: V_k holds exactly the items with a row in R_k of a leaf of the slab;
  * V_k is a subset of M_k, word for word (ops.cone_masks_host on ops.field_tables), also for a pattern that is not symmetric.
Shapes: two small generator complexes on a synthetic plan (a block every 16 rows, the last one short) and a hand-built operator with a
hub row that every other row reads (P^2 is dense there: V_2 is everything some leaf's slab reaches)."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import scone_oracle as so

NS = 4


def _complex_case(n_points, one_sided=False):
    from scone_gcn_amd import synthetic_data_gen as g
    cx = g.random_SC_graph(n_points)
    B1, B2 = (m.toarray() for m in g.incidence_matrices(cx))
    L_lo, L_up = so.scone_shifts(B1, B2)
    if one_sided:                                       # strictly upper triangular: not symmetric, no diagonal entry
        L_lo, L_up = np.triu(L_lo, 1), np.triu(L_up, 1)
    E = B1.shape[1]
    row0 = np.append(np.arange(0, E, 16), E)
    nbr, _ = so.neighborhoods(cx.edges, cx.n_nodes)
    inc_ptr, inc_edge, _, _ = so.incidence_csr(cx.edges, cx.n_nodes)
    pattern = sp.csr_matrix((L_lo != 0) | (L_up != 0))
    return dict(E=E, row0=row0, nbr=np.asarray(nbr), inc_ptr=np.asarray(inc_ptr), inc_edge=np.asarray(inc_edge), pattern=pattern)


def _hub_case():
    """97 rows in blocks of 1 .. 9 rows: a ring, plus row 40, which reads every row and is read by every row.  Nodes: 30, node v with
    the incident `edges` 3 v .. 3 v + 2 (row 40 is node 13's) and the neighbours v - 1, v, v + 1."""
    E, V = 97, 30
    i = np.arange(E)
    r, c = np.r_[i, i, i, np.full(E, 40)], np.r_[(i + 1) % E, (i - 1) % E, np.full(E, 40), i]
    pattern = sp.csr_matrix((np.ones(len(r), np.int8), (r, c)), shape=(E, E))
    pattern.sum_duplicates()
    rs = np.random.RandomState(5)
    cuts = [0]
    while cuts[-1] < E:
        cuts.append(min(E, cuts[-1] + int(rs.randint(1, 10))))
    nbr = -np.ones((V, 4), np.int64)
    for v in range(V):
        nb = [u for u in (v - 1, v, v + 1) if 0 <= u < V]
        nbr[v, :len(nb)] = nb
    inc_ptr = 3 * np.arange(V + 1)
    return dict(E=E, row0=np.asarray(cuts), nbr=nbr, inc_ptr=inc_ptr, inc_edge=np.arange(3 * V), pattern=pattern)


CASES = {"complex300": lambda: _complex_case(300), "complex120_one_sided": lambda: _complex_case(120, True), "hub": _hub_case}
_BUILT = {}


def _case(name):
    """The case's arrays, its tables for three hops and the brute-force row sets R_k(v), k = 0 .. 3, built once."""
    if name not in _BUILT:
        from scone_gcn_amd import ops
        c = CASES[name]()
        E, V = c["E"], c["nbr"].shape[0]
        c["V"], c["nb"] = V, len(c["row0"]) - 1
        c["blk_of"] = np.searchsorted(c["row0"], np.arange(E), side="right") - 1
        args = (c["row0"], c["pattern"], c["nbr"], c["inc_ptr"], c["inc_edge"])
        c["field"] = ops.field_tables(*args)
        c["tables"] = ops.visit_tables(*args, 3)
        P = c["pattern"].toarray() != 0
        P |= np.eye(E, dtype=bool)
        R = np.zeros((4, V, E), bool)
        for v in range(V):
            for u in c["nbr"][v][c["nbr"][v] >= 0]:
                R[0, v, c["inc_edge"][c["inc_ptr"][u]:c["inc_ptr"][u + 1]]] = True
        for k in range(1, 4):
            R[k] = (R[k - 1].astype(np.int32) @ P.T.astype(np.int32)) > 0      # row r is in R_k iff it reads a column of R_{k-1}
        c["R"] = R
        _BUILT[name] = c
    return _BUILT[name]


def _nodes(c, n, rs, repeat=False):
    nodes = rs.randint(0, c["V"], size=n).astype(np.int32)
    if repeat:                                             # two nodes, each in many slabs
        nodes[:n // 2], nodes[n // 2:] = nodes[0], nodes[-1]
    return nodes


@pytest.mark.parametrize("name", sorted(CASES))
def test_tables_against_brute_force_over_rows(name):
    c = _case(name)
    assert len(c["tables"]) == 3
    some_growth = False
    for k, (ptr, blk) in enumerate(c["tables"], start=1):
        assert ptr.dtype == np.int32 and blk.dtype == np.int32 and len(ptr) == c["V"] + 1 and ptr[-1] == len(blk)
        for v in range(c["V"]):
            want = np.unique(c["blk_of"][c["R"][k, v]])
            got = blk[ptr[v]:ptr[v + 1]]
            assert got.tolist() == want.tolist(), "T_%d(%d): ascending, every block once" % (k, v)
            some_growth |= len(want) > len(np.unique(c["blk_of"][c["R"][0, v]]))
    # the `top` table is the same construction at k = 0
    tp, tb = c["field"][0]
    for v in range(c["V"]):
        assert tb[tp[v]:tp[v + 1]].tolist() == np.unique(c["blk_of"][c["R"][0, v]]).tolist()
    assert some_growth


def test_the_hub_row_makes_the_second_table_dense():
    c = _case("hub")
    ptr, blk = c["tables"][1]
    assert all(ptr[v + 1] - ptr[v] == c["nb"] for v in range(c["V"])), "two hops through row 40 reach every row"
    ptr, blk = c["tables"][0]
    assert min(np.diff(ptr)) < c["nb"], "one hop does not"


def test_tables_are_refused_where_a_product_would_pass_the_work_bound():
    """The hub's second hop multiplies every node's first-hop rows by the hub row's 97 entries: bounded before it is formed."""
    from scone_gcn_amd import ops
    c = _case("hub")
    args = (c["row0"], c["pattern"], c["nbr"], c["inc_ptr"], c["inc_edge"])
    one = ops.visit_tables(*args, 1, max_work=2000)
    assert one is not None and all(np.array_equal(a, b) for a, b in zip(one[0], c["tables"][0])), "one hop fits the bound"
    assert ops.visit_tables(*args, 2, max_work=2000) is None
    assert ops.visit_tables(*args, 1, max_work=10) is None
    assert ops.VISIT_TABLES_MAX_WORK < 2 ** 31, "a table's entries stay below the bound: ptr fits int32"


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("n,repeat", [(3, False), (4 * 5, False), (4 * 33 - 2, False), (4 * 64, True)])
def test_visit_masks_hold_the_items_with_a_row_in_r_k_and_lie_inside_the_cone(name, n, repeat):
    from scone_gcn_amd import ops
    c = _case(name)
    rs = np.random.RandomState(n)
    nodes = _nodes(c, n, rs, repeat)
    if not repeat and n > 4:
        nodes[1], nodes[2] = -1, c["V"]                    # out of range: skipped
    n_slabs = -(-n // NS)
    words = (n_slabs + 31) // 32
    L = 4
    got = ops.visit_masks_host(nodes, NS, c["tables"], c["nb"])
    (masks, _, _), = ops.cone_masks_host([nodes], NS, *c["field"][0], *c["field"][1], c["nb"], L)
    assert len(got) == L - 1
    proper = False
    for k in range(1, L):
        want = np.zeros((c["nb"], words), np.uint32)
        for i, v in enumerate(nodes):
            if 0 <= v < c["V"]:
                s = i // NS
                want[np.unique(c["blk_of"][c["R"][k, v]]), s >> 5] |= np.uint32(1 << (s & 31))
        assert got[k - 1].dtype == np.uint32 and got[k - 1].shape == (c["nb"], words)
        assert np.array_equal(got[k - 1], want), "V_%d = the items holding a row of R_%d" % (k, k)
        assert not (got[k - 1] & ~masks[k]).any(), "V_%d lies inside M_%d, word for word" % (k, k)
        proper |= bool((masks[k] & ~got[k - 1]).any())
    assert proper or name != "complex300", "on the larger complex the cone's masks are strictly larger somewhere"
