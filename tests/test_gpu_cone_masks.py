"""scn_cone_masks -- the masks, unit lists and counts of several micro-batches in one launch -- on hand-built `top` / `adj` tables,
BITWISE against ops.cone_masks_host and against today's chain (scn_keep_mask_units + scn_mask_hop_units: masks equal, each list equal
to the old list sorted, counts equal).

Every output buffer is filled with a poison word first, and has poisoned words between one mask (list) and the next: every mask word
and all SCN_UNIT_COUNTERS counters are written, list entries at or past the count and the words between the masks are not.

Shapes: one block; 1023 / 1024 / 1025 words (the thread count's edge; 1023 and 1025 are no multiples of four, and a destination that
starts off a 16-byte boundary takes the 16-byte stores' head and tail, an adjacency table off one is read entry by entry); two words with 33 and with 64 slabs; a last partial slab;
L = 1 .. 4; 1, 2, 3 and 65 micro-batches with different last nodes and a shorter last one; nodes -1 and n_nodes, a node with an empty
row, blocks -1 and n_blocks in each table, a hub block adjacent to all; a mask exactly at the limit the library exports; the
benchmark's geometry (16 557 blocks, one word, 128 nodes, a band of about ten); the two refusals with every buffer's poison intact."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_keep_last import _need_gpu

pytestmark = pytest.mark.gpu

NS = 4
POISON = np.uint32(0xDEADBEEF).view(np.int32).item()
GAP = 5                 # poisoned words between one mask (list) and the next


def _tables(n_nodes, n_blocks, seed, band=5, hub=None, bad=False):
    """((top_ptr, top_blk), (adj_ptr, adj_blk)) int32: node v reads one to four blocks around v * n_blocks / n_nodes (every seventh node
    none); block b stages the blocks within `band` of it, itself included, less a random one (so the table is not symmetric; every
    fifth block beyond the first stages nothing).  hub: that block stages all blocks and all stage it.  bad: entries of -1 and
    n_blocks are mixed into both tables."""
    rs = np.random.RandomState(seed)
    tp, tb = [0], []
    for v in range(n_nodes):
        if v % 7 != 6:
            c = v * n_blocks // n_nodes
            blk = sorted({min(n_blocks - 1, max(0, c + int(d))) for d in rs.randint(-2, 3, size=rs.randint(1, 5))})
            if bad:
                blk = [-1] + blk + [n_blocks]
            tb += blk
        tp.append(len(tb))
    b = np.arange(n_blocks)
    lo, hi = np.maximum(b - band, 0), np.minimum(b + band, n_blocks - 1)
    deg = hi - lo + 1
    start = np.cumsum(deg) - deg
    cols = np.arange(int(deg.sum())) - np.repeat(start, deg) + np.repeat(lo, deg)
    rows = np.repeat(b, deg)
    keep = np.ones(len(cols), bool)
    keep[start + rs.randint(0, 1 << 30, size=n_blocks) % deg] = n_blocks < 3            # drop one entry per row
    keep[(rows % 5 == 4)] = False                                                        # empty rows
    if bad:
        cols = cols.copy()
        cols[rs.rand(len(cols)) < 0.1] = -1
        cols[rs.rand(len(cols)) < 0.1] = n_blocks
    rows, cols = rows[keep], cols[keep]
    if hub is not None:
        rows = np.concatenate([rows, np.full(n_blocks, hub), b])
        cols = np.concatenate([cols, b, np.full(n_blocks, hub)])
        order = np.argsort(rows, kind="stable")
        rows, cols = rows[order], cols[order]
    ap = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_blocks))])
    return (np.asarray(tp, np.int32), np.asarray(tb, np.int32)), (ap.astype(np.int32), cols.astype(np.int32))


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(np.append(a, 0), np.int32)).cuda()     # (a pad word: an empty table still has a pointer)


def _call(lists, n_nodes, n_blocks, top, adj, L, misalign=0):
    """Runs scn_cone_masks on poisoned buffers: (status, per micro-batch (masks [L][n_words], lists [L][n_words], counters), the checks
    of the untouched words done).  misalign: words the first mask and list, and the adjacency's entries, start past a 512-byte
    boundary (the entries are fetched in 16-byte loads only from a table that lies on a 16-byte boundary)."""
    from scone_gcn_amd import _lib, ops
    lib = _lib.load()
    dev = [torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in lists]
    words = [(-(-len(a) // NS) + 31) // 32 for a in lists]
    n_words = [n_blocks * w for w in words]
    stride = [nw + GAP for nw in n_words]
    total = misalign + ops.UNIT_COUNTERS * sum(stride) + GAP
    masks = torch.full((total,), POISON, dtype=torch.int32, device="cuda")
    units = torch.full((total,), POISON, dtype=torch.int32, device="cuda")
    counters = torch.full((len(lists) * ops.UNIT_COUNTERS + 1,), POISON, dtype=torch.int32, device="cuda")
    desc = (_lib.ConeMb * len(lists))()
    off, offs = misalign, []
    for i, t in enumerate(dev):
        d = desc[i]
        d.node, d.n, d.stride = t.data_ptr(), t.numel(), stride[i]
        d.masks, d.units, d.counters = masks.data_ptr() + 4 * off, units.data_ptr() + 4 * off, counters.data_ptr() + 16 * i
        offs.append(off)
        off += ops.UNIT_COUNTERS * stride[i]
    tabs = [_up(a) for a in (*top, adj[0], np.concatenate([np.full(misalign, n_blocks - 1, np.int32), adj[1]]))]
    ptrs = [t.data_ptr() for t in tabs]
    ptrs[3] += 4 * misalign
    status = lib.scn_cone_masks(len(lists), desc, NS, n_nodes, n_blocks, *(ctypes.c_void_p(q) for q in ptrs), L, ops._stream())
    torch.cuda.synchronize()
    m, u, c = masks.cpu().numpy(), units.cpu().numpy(), counters.cpu().numpy()
    if status != 0:
        assert (m == POISON).all() and (u == POISON).all() and (c == POISON).all(), "a declined call writes nothing"
        return status, None
    assert c[-1] == POISON
    out, written = [], np.zeros(total, bool)
    for i in range(len(lists)):
        cnt = c[4 * i:4 * i + 4].view(np.uint32)
        ms, us = [], []
        for k in range(L):
            a = offs[i] + k * stride[i]
            written[a:a + n_words[i]] = True
            ms.append(m[a:a + n_words[i]].view(np.uint32).reshape(n_blocks, words[i]))
            assert cnt[k] <= n_words[i]
            us.append(u[a:a + cnt[k]].view(np.uint32))
            assert (u[a + cnt[k]:a + stride[i]] == POISON).all(), "list entries at or past the count are not written"
        assert (u[offs[i] + L * stride[i]:offs[i] + ops.UNIT_COUNTERS * stride[i]] == POISON).all()
        out.append((ms, us, cnt))
    assert (m[~written] == POISON).all(), "nothing but the masks' own words is written"
    return status, out


def _check(lists, n_nodes, n_blocks, top, adj, L, misalign=0, chain=True):
    from scone_gcn_amd import ops
    status, got = _call(lists, n_nodes, n_blocks, top, adj, L, misalign)
    assert status == 0
    want = ops.cone_masks_host(lists, NS, *top, *adj, n_blocks, L)
    for i, ((ms, us, cnt), (hm, hu, hc)) in enumerate(zip(got, want)):
        assert (cnt == hc).all(), "counters of micro-batch %d: %s, host %s" % (i, cnt, hc)
        for k in range(L):
            assert (ms[k] == hm[k]).all(), "mask %d of micro-batch %d" % (k, i)
            assert us[k].tolist() == hu[k].tolist(), "list %d of micro-batch %d (ascending)" % (k, i)
    if chain:                                   # today's launches on the same tables
        tabs = ops.FieldTables(n_blocks, *(_up(a) for a in (*top, *adj)))
        for i, nodes in enumerate(lists):
            t = torch.from_numpy(np.ascontiguousarray(nodes, np.int32)).cuda()
            m, u, counters = ops.ConvOp.keep_mask_units(None, t, NS, n_nodes, tabs)
            old = [(m, u)]
            for k in range(1, L):
                old.append(ops.ConvOp.mask_hop_units(None, old[-1][0], tabs, counters[k:k + 1]))
            torch.cuda.synchronize()
            for k, (m, u) in enumerate(old):
                assert (m.cpu().numpy().view(np.uint32) == got[i][0][k]).all(), "mask %d against today's chain" % k
                n = int(u.count.cpu().numpy().view(np.uint32)[0])
                assert n == got[i][2][k]
                assert np.sort(u.units.cpu().numpy().view(np.uint32)[:n]).tolist() == got[i][1][k].tolist()
    return got


def _nodes(n, n_nodes, seed):
    return np.random.RandomState(seed).randint(0, n_nodes, size=n).astype(np.int32)


def test_one_block():
    _need_gpu()
    top = (np.asarray([0, 1, 1], np.int32), np.asarray([0], np.int32))
    adj = (np.asarray([0, 1], np.int32), np.asarray([0], np.int32))
    got = _check([np.asarray([1, 1, 1, 1, 0, 1], np.int32)], 2, 1, top, adj, 3)
    assert got[0][0][0].tolist() == [[2]] and got[0][2].tolist() == [1, 1, 1, 0]


@pytest.mark.parametrize("misalign", [0, 1, 3])
@pytest.mark.parametrize("n_blocks", [1023, 1024, 1025])
def test_the_thread_counts_edge_and_the_16_byte_stores_tail(n_blocks, misalign):
    _need_gpu()
    top, adj = _tables(200, n_blocks, n_blocks)
    got = _check([_nodes(24, 200, 3)], 200, n_blocks, top, adj, 3, misalign=misalign)
    assert 0 < got[0][2][0] < got[0][2][1] < got[0][2][2]
    # the last word itself: a node whose row names the last block
    top = (np.asarray([0, 2], np.int32), np.asarray([0, n_blocks - 1], np.int32))
    got = _check([np.zeros(5, np.int32)], 1, n_blocks, top, adj, 2, misalign=misalign)
    assert got[0][1][0].tolist() == [0, n_blocks - 1]


@pytest.mark.parametrize("slabs", [33, 64])
def test_two_words(slabs):
    _need_gpu()
    n_nodes, n_blocks = 90, 300
    top, adj = _tables(n_nodes, n_blocks, slabs)
    nodes = np.full(NS * slabs, 6, np.int32)                 # (node 6 has an empty row)
    nodes[NS * (slabs - 1):] = _nodes(NS, n_nodes, 5)        # bits of the last slab only: word 1, bit (slabs - 1) & 31
    got = _check([nodes], n_nodes, n_blocks, top, adj, 3)
    m0 = got[0][0][0]
    assert not m0[:, 0].any() and m0[:, 1].any() and set(np.unique(m0[:, 1])) <= {0, 1 << ((slabs - 1) & 31)}
    assert (got[0][1][0] % 2 == 1).all(), "every entry of M0's list is a second word"
    _check([_nodes(NS * slabs, n_nodes, 9)], n_nodes, n_blocks, top, adj, 3)


@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_levels_and_a_last_partial_slab(L):
    _need_gpu()
    n_nodes, n_blocks = 64, 2500
    top, adj = _tables(n_nodes, n_blocks, 11 + L)
    got = _check([_nodes(13, n_nodes, L)], n_nodes, n_blocks, top, adj, L)     # 13 leaves: three slabs and a quarter
    assert got[0][2][:L].all() and not got[0][2][L:].any()


@pytest.mark.parametrize("n_mb", [1, 2, 3, 65])
def test_micro_batches_and_the_chunking(n_mb):
    _need_gpu()
    n_nodes, n_blocks = 150, 1500
    top, adj = _tables(n_nodes, n_blocks, 31)
    lists = [_nodes(16, n_nodes, 100 + i) for i in range(n_mb - 1)] + [_nodes(7, n_nodes, 99)]        # a shorter last one
    got = _check(lists, n_nodes, n_blocks, top, adj, 3, chain=n_mb <= 3)
    assert len({tuple(g[1][0].tolist()) for g in got}) > min(n_mb, 2) - 1, "different last nodes give different masks"
    if n_mb == 65:          # a mix of one and two words, the 65th beyond the first launch's table
        lists = [_nodes(16 if i % 2 else NS * 40, n_nodes, 200 + i) for i in range(n_mb)]
        _check(lists, n_nodes, n_blocks, top, adj, 2, chain=False)


def test_the_guards_and_a_hub():
    _need_gpu()
    n_nodes, n_blocks = 40, 700
    top, adj = _tables(n_nodes, n_blocks, 77, hub=350, bad=True)
    nodes = _nodes(32, n_nodes, 8)
    nodes[0], nodes[1], nodes[2] = -1, n_nodes, 6               # outside on either side; node 6: an empty row
    got = _check([nodes, np.asarray([-1, n_nodes, 6, 6], np.int32)], n_nodes, n_blocks, top, adj, 4)
    assert got[0][2][2] > 600, "two hops through the hub reach nearly every block"
    assert not got[1][2].any() and not any(m.any() for m in got[1][0]), "nodes that contribute nothing: all-zero masks, written"


def test_a_mask_exactly_at_the_limit():
    _need_gpu()
    from scone_gcn_amd import _lib, ops
    limit = ops.cone_masks_limit()
    assert limit == int(_lib.load().scn_cone_masks_max_words()) and limit % 2 == 0
    top, adj = _tables(64, limit, 5)
    top[1][-1] = limit - 1                                       # the last word is set: the last entry of node 63's row
    nodes = _nodes(16, 64, 1)
    nodes[0] = 63
    got = _check([nodes], 64, limit, top, adj, 2)
    assert got[0][1][0][-1] == limit - 1
    top, adj = _tables(64, limit // 2, 6)                        # ... and as two words per block
    _check([_nodes(NS * 33, 64, 2)], 64, limit // 2, top, adj, 2)


def test_the_benchmarks_geometry():
    _need_gpu()
    n_nodes, n_blocks = 4000, 16557
    top, adj = _tables(n_nodes, n_blocks, 1030, band=5)
    got = _check([_nodes(128, n_nodes, 1030 + i) for i in range(2)], n_nodes, n_blocks, top, adj, 3)
    assert 100 < got[0][2][0] < got[0][2][1] < got[0][2][2] < n_blocks


def test_refusals_leave_every_buffer_untouched():
    _need_gpu()
    from scone_gcn_amd import _lib, ops
    limit = ops.cone_masks_limit()
    top, adj = _tables(8, limit + 1, 3)
    assert _call([_nodes(8, 8, 1)], 8, limit + 1, top, adj, 2)[0] == _lib.SCN_ERR_UNSUPPORTED
    top, adj = _tables(8, limit // 2 + 1, 3)
    assert _call([_nodes(8, 8, 1), _nodes(NS * 33, 8, 2)], 8, limit // 2 + 1, top, adj, 2)[0] == _lib.SCN_ERR_UNSUPPORTED, \
        "the second micro-batch's two words are over the limit: nothing is launched for the first either"
    top, adj = _tables(8, 50, 3)
    assert _call([_nodes(8, 8, 1)], 8, 50, top, adj, ops.UNIT_COUNTERS + 1)[0] == _lib.SCN_ERR_UNSUPPORTED
    assert _call([_nodes(8, 8, 1)], 8, 50, top, adj, ops.UNIT_COUNTERS)[0] == 0
