"""ops.cone_masks_host -- the NumPy restatement of scn_cone_masks (include/scone_hip.h) -- against brute force over bits on small random
`top` / `adj` tables: non-symmetric adjacency, empty rows, nodes and blocks outside their ranges, two mask words.  No GPU."""
import numpy as np
import pytest

from scone_gcn_amd import ops

NS = 4


def _csr(rows, rs, n_cols, density, bad=0.0):
    """(ptr, idx) int32 of a random table with `rows` rows over [0, n_cols); every third row empty; bad: the share of entries replaced
    by an index outside the range (-1, n_cols, n_cols + 7)."""
    ptr, idx = [0], []
    for r in range(rows):
        if r % 3 != 2:
            cols = np.flatnonzero(rs.rand(n_cols) < density)
            cols = [int(rs.choice([-1, n_cols, n_cols + 7])) if rs.rand() < bad else int(c) for c in cols]
            idx += cols
        ptr.append(len(idx))
    return np.asarray(ptr, np.int32), np.asarray(idx, np.int32)


def _brute(nodes, ns, top, adj, n_nodes, n_blocks, L):
    """Sets of (block, slab) pairs per level, one bit at a time."""
    top_ptr, top_blk = top
    adj_ptr, adj_blk = adj
    cur = set()
    for i, v in enumerate(nodes):
        if 0 <= v < n_nodes:
            for b in top_blk[top_ptr[v]:top_ptr[v + 1]]:
                if 0 <= b < n_blocks:
                    cur.add((int(b), i // ns))
    levels = [cur]
    for _ in range(1, L):
        nxt = set()
        for b in range(n_blocks):
            for b2 in adj_blk[adj_ptr[b]:adj_ptr[b + 1]]:
                if 0 <= b2 < n_blocks:
                    nxt |= {(b, s) for (bb, s) in cur if bb == b2}
        levels.append(nxt)
        cur = nxt
    return levels


def _unpack(mask):
    return {(b, 32 * w + k) for b in range(mask.shape[0]) for w in range(mask.shape[1]) for k in range(32) if mask[b, w] >> np.uint32(k) & 1}


@pytest.mark.parametrize("n,L,bad", [(12, 1, 0.0), (13, 3, 0.0), (4 * 33 + 1, 4, 0.0), (4 * 64, 2, 0.2), (30, 4, 0.3)])
def test_against_brute_force(n, L, bad):
    rs = np.random.RandomState(n * 7 + L)
    n_nodes, n_blocks = 17, 23
    top = _csr(n_nodes, rs, n_blocks, 0.15, bad)
    adj = _csr(n_blocks, rs, n_blocks, 0.12, bad)          # (random rows: not symmetric, no diagonal)
    lists = [rs.randint(-1, n_nodes + 1, size=n).astype(np.int32), rs.randint(0, n_nodes, size=max(1, n // 2)).astype(np.int32)]
    got = ops.cone_masks_host(lists, NS, *top, *adj, n_blocks, L)
    assert len(got) == 2
    for nodes, (masks, units, counters) in zip(lists, got):
        words = (-(-len(nodes) // NS) + 31) // 32
        assert words == (2 if len(nodes) > 4 * 32 else 1)
        want = _brute(nodes, NS, top, adj, n_nodes, n_blocks, L)
        assert len(masks) == len(units) == L and counters.shape == (ops.UNIT_COUNTERS,) and counters.dtype == np.uint32
        for k in range(L):
            assert masks[k].shape == (n_blocks, words) and masks[k].dtype == np.uint32
            assert _unpack(masks[k]) == want[k], "level %d" % k
            flat = masks[k].reshape(-1)
            assert units[k].tolist() == [i for i in range(flat.size) if flat[i]], "ascending, every non-empty word once"
            assert counters[k] == len(units[k])
        assert not counters[L:].any()
    assert any(len(u) for _, us, _ in got for u in us), "the case sets something"


def test_second_word_and_the_guards():
    """Slab 40 lies in word 1; a node of -1 and one of n_nodes set nothing; a block of -1 or n_blocks in either table is passed over."""
    n_nodes, n_blocks = 3, 4
    top = (np.asarray([0, 2, 4, 4], np.int32), np.asarray([1, -1, n_blocks, 2], np.int32))       # node 2: empty row
    adj = (np.asarray([0, 2, 3, 5, 5], np.int32), np.asarray([0, 1, n_blocks, -1, 2], np.int32))   # block 3: empty row; 0 <- 1, not 1 <- 0
    nodes = np.full(4 * 41, 2, np.int32)
    nodes[0], nodes[1], nodes[4 * 40], nodes[4 * 40 + 1] = 0, -1, 1, n_nodes
    (masks, units, counters), = ops.cone_masks_host([nodes], NS, *top, *adj, n_blocks, 3)
    m0 = np.zeros((4, 2), np.uint32)
    m0[1, 0] = 1                       # node 0 at slab 0 -> block 1 (the -1 beside it is passed over)
    m0[2, 1] = 1 << 8                  # node 1 at slab 40 -> block 2 (n_blocks beside it is passed over)
    assert (masks[0] == m0).all()
    m1 = np.zeros((4, 2), np.uint32)
    m1[0, 0] = 1                       # block 0 stages 0 and 1
    m1[2, 1] = 1 << 8                  # block 2 stages -1 (passed over) and 2; block 1 stages only n_blocks
    assert (masks[1] == m1).all()
    m2 = np.zeros((4, 2), np.uint32)
    m2[0, 0] = 1
    m2[2, 1] = 1 << 8
    assert (masks[2] == m2).all()
    assert [u.tolist() for u in units] == [[2, 5], [0, 5], [0, 5]] and counters.tolist() == [2, 2, 2, 0]
