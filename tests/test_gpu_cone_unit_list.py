"""GPU tests of the unit lists of a readout cone's forward-side launches (ops.CONE_UNIT_LIST; include/scone_hip.h, "Unit lists";
WindowWalk's list mode, scn_window_scan.inc; DESIGN.md sections 3 and 7).

The three forward-side masked launches (gather3_c1_keep_kernel, fwd_c32_w16_kernel<FROMY, KEEP>, fwd_c32_w16_kernel<KEEP>) may take
their units from one device-wide list of the mask's non-empty words -- workgroup g of G takes entries g, g + G, ... -- instead of
walking a fixed share of the blocks.  Pinned here:

1. The lists the mask kernels write (scn_keep_mask_units, scn_mask_hop_units) against ops.keep_mask_host / ops.mask_hop_host: the set
   of entries is the set of non-zero (block, word), the count is exact, no entry twice, the masks are the bits of the calls without a
   list; 5, 32, 33 and 64 slabs (one and two words per block); an all-zero mask, all last nodes equal, every block non-empty; a
   capacity one short is refused before any launch (nothing written).
2. The three kernels with a list against the same masked launch on its static walk, on sentinel-filled outputs, bit for bit (kept
   items equal, every other row untouched), and the static one against the launch without a mask: count 0, exactly one entry, fewer
   entries than workgroups, entries only in word 1, blocks with bits in both words (two entries, each item once), a host-shuffled
   list (the order is free), tanh and relu.  The operator is tridiagonal with 1024 two-row blocks: its launch grids (256 x 1 and
   512 x 1, restated and asserted) have ONE slab range at every slab count used here, so the list is what the kernels walk -- on the
   suite's small complexes the grids split the slabs and a launch would fall back.  More than one scan per workgroup: 131 080 two-row
   blocks, all ones at two slabs -- 512 or 513 entries per workgroup of the 256-workgroup grid (three scans), 256 or 257 of the
   512-workgroup grid (two).
3. Fallback: a grid that splits the slabs (517 blocks at 64 slabs) or has more than 64 slabs (130) walks its static units: served,
   equal results.
4. Plan steps with ops.CONE_UNIT_LIST on against off: loss and every weight gradient bit for bit at three and four layers -- on one
   slab, where every grid has one slab range and the list is walked, and on the four slabs of tests/test_gpu_readout_cone.py; two
   forwards interleaved on one plan and their backwards in reverse order equal fresh plans; the pooled buffers come back all zero.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import scone_oracle as so
from tests import test_gpu_readout_cone as rc
from tests import test_gpu_window_scan as ws
from tests.test_gpu_keep_last import _expected, _need_gpu, _pack, _same_bits, _sentinel

pytestmark = pytest.mark.gpu


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------------------------
# 1. the lists the mask kernels write
# ------------------------------------------------------------------------------------------------------------------

FILL = 0x5A5A5A5A


def _check_list(words, units, count, what):
    """The first `count` entries of `units` are the indices of the non-zero words of `words` (uint32 [nb][w]), each once."""
    want = np.flatnonzero(words.reshape(-1))
    assert count == len(want), "%s: count %d, %d non-zero words" % (what, count, len(want))
    got = units[:count].astype(np.int64)
    assert len(set(got.tolist())) == count, what + ": an entry twice"
    assert sorted(got.tolist()) == want.tolist(), what + ": the entries are not the non-zero words"
    assert (units[count:] == FILL).all(), what + ": written past the count"


def _nodes(env, case, S, rs):
    plan, tabs = env["plan"](), env["tabs"]
    n = 4 * S
    if case == "none":                                    # no leaf stands on a node of the table: an all-zero mask
        return np.full(n, -1)
    if case == "equal":
        return np.full(n, int(np.argmax((plan._h_nbr >= 0).sum(axis=1))))
    if case == "every_block":                             # for every block a node whose readout reads it
        top_ptr, top_blk = tabs.top_ptr.cpu().numpy()[:plan.n_nodes + 1], tabs.top_blk.cpu().numpy()[:-1]
        node_of = {}
        for v in range(plan.n_nodes):
            for b in top_blk[top_ptr[v]:top_ptr[v + 1]]:
                node_of.setdefault(int(b), v)
        assert len(node_of) == tabs.n_blocks and (tabs.n_blocks <= n or S < 32), "a node for every block, and from 32 slabs on a leaf for each"
        picks = [node_of[b] for b in range(tabs.n_blocks)][:n]
        return np.array((picks * (n // len(picks) + 1))[:n])
    return rs.randint(0, plan.n_nodes, size=n)


@pytest.mark.parametrize("case", ["random", "none", "equal", "every_block"])
@pytest.mark.parametrize("S", [5, 32, 33, 64])
def test_keep_mask_units_lists_the_non_zero_words_once(S, case):
    _need_gpu()
    from scone_gcn_amd import _lib, ops
    env = rc._env()
    plan, tabs = env["plan"](), env["tabs"]
    top = (tabs.top_ptr.cpu().numpy()[:plan.n_nodes + 1], tabs.top_blk.cpu().numpy()[:-1])
    nodes = _nodes(env, case, S, np.random.RandomState(S))
    words = (S + 31) // 32
    n_words = tabs.n_blocks * words
    nd = torch.as_tensor(nodes.astype(np.int32), device="cuda")
    buf = torch.full((n_words + ops.UNIT_COUNTERS + 1,), FILL, device="cuda", dtype=torch.int32)     # (one guard word behind)
    units = torch.full((n_words + 1,), FILL, device="cuda", dtype=torch.int32)
    _lib.check(_lib.load().scn_keep_mask_units(len(nodes), 4, _p(nd), plan.n_nodes, _p(tabs.top_ptr), _p(tabs.top_blk), tabs.n_blocks,
                                               _p(buf), _p(units), n_words, _stream()), "scn_keep_mask_units")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert out[-1] == FILL, "the word behind the counters was written"
    mask = out[:n_words].view(np.uint32).reshape(tabs.n_blocks, words)
    want = ops.keep_mask_host(nodes, 4, *top, tabs.n_blocks)
    assert np.array_equal(mask, want), "the mask is not the restatement's"
    plain = torch.full((n_words,), FILL, device="cuda", dtype=torch.int32)
    _lib.check(_lib.load().scn_keep_mask(len(nodes), 4, _p(nd), plan.n_nodes, _p(tabs.top_ptr), _p(tabs.top_blk), tabs.n_blocks, _p(plain),
                                         _stream()), "scn_keep_mask")
    assert np.array_equal(plain.cpu().numpy().view(np.uint32), mask.reshape(-1)), "the mask differs from the call without a list"
    counters = out[n_words:n_words + ops.UNIT_COUNTERS]
    assert (counters[1:] == 0).all(), "the other counters are left zero"
    _check_list(want, units.cpu().numpy(), int(counters[0]), "%d slabs, %s" % (S, case))
    assert (int(counters[0]) == 0) == (case == "none")
    if case == "every_block" and S >= 32:                 # (5 slabs: as many blocks as there are leaves)
        assert want.any(axis=1).all()
    # ... and through the operator's wrapper
    m, u, c = plan.conv.keep_mask_units(nd, 4, plan.n_nodes, tabs)
    torch.cuda.synchronize()
    assert np.array_equal(m.cpu().numpy().view(np.uint32), want) and int(u.count.cpu()[0]) == int(counters[0]) and not bool(c[1:].any())


@pytest.mark.parametrize("case", ["random", "zero", "ones", "one_block"])
@pytest.mark.parametrize("S", [5, 32, 33, 64])
def test_mask_hop_units_lists_the_non_zero_words_once(S, case):
    _need_gpu()
    from scone_gcn_amd import _lib, ops
    env = rc._env()
    tabs, nb = env["tabs"], env["nb"]
    rs = np.random.RandomState(100 + S)
    k = np.zeros((nb, S), bool)
    if case == "random":
        k[:] = rs.rand(nb, S) < 0.02
        k[rs.randint(nb), S - 1] = True
    elif case == "ones":                                  # every block, every word non-empty
        k[:] = True
    elif case == "one_block":
        k[nb // 2, S - 1] = True
    src = _pack(k)
    want = ops.mask_hop_host(src.cpu().numpy().view(np.uint32), *env["adj"])
    n_words = want.size
    out = torch.full((n_words + 1,), FILL, device="cuda", dtype=torch.int32)
    units = torch.full((n_words + 1,), FILL, device="cuda", dtype=torch.int32)
    count = torch.zeros(2, device="cuda", dtype=torch.int32)
    _lib.check(_lib.load().scn_mask_hop_units(nb, want.shape[1], _p(tabs.adj_ptr), _p(tabs.adj_blk), _p(src), _p(out), _p(units), _p(count),
                                              n_words, _stream()), "scn_mask_hop_units")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[-1] == FILL and int(count[1]) == 0
    assert np.array_equal(got[:-1].view(np.uint32).reshape(want.shape), want), "the mask is not the restatement's"
    plain = env["plan"]().conv.mask_hop(src, tabs)
    assert np.array_equal(plain.cpu().numpy().view(np.uint32), want), "the mask differs from the call without a list"
    _check_list(want, units.cpu().numpy(), int(count[0]), "%d slabs, %s" % (S, case))
    assert (int(count[0]) == 0) == (case == "zero")
    if case == "ones":
        assert int(count[0]) == n_words


def test_a_capacity_one_short_is_refused_before_any_launch():
    _need_gpu()
    from scone_gcn_amd import _lib, ops
    env = rc._env()
    plan, tabs = env["plan"](), env["tabs"]
    S = 33
    n_words = tabs.n_blocks * 2
    nd = torch.as_tensor(np.random.RandomState(0).randint(0, plan.n_nodes, size=4 * S).astype(np.int32), device="cuda")
    buf = torch.full((n_words + ops.UNIT_COUNTERS,), FILL, device="cuda", dtype=torch.int32)
    units = torch.full((n_words,), FILL, device="cuda", dtype=torch.int32)
    count = torch.full((1,), FILL, device="cuda", dtype=torch.int32)
    lib = _lib.load()
    st = lib.scn_keep_mask_units(4 * S, 4, _p(nd), plan.n_nodes, _p(tabs.top_ptr), _p(tabs.top_blk), tabs.n_blocks, _p(buf), _p(units),
                                 n_words - 1, _stream())
    assert st == _lib.SCN_ERR_WORKSPACE
    src = _pack(np.ones((tabs.n_blocks, S), bool))
    st = lib.scn_mask_hop_units(tabs.n_blocks, 2, _p(tabs.adj_ptr), _p(tabs.adj_blk), _p(src), _p(buf), _p(units), _p(count), n_words - 1,
                                _stream())
    assert st == _lib.SCN_ERR_WORKSPACE
    st = lib.scn_mask_hop_units(tabs.n_blocks, 2, _p(tabs.adj_ptr), _p(tabs.adj_blk), _p(src), _p(buf), _p(units), None, n_words, _stream())
    assert st == _lib.SCN_ERR_BAD_ARG                      # a list without its counter
    torch.cuda.synchronize()
    assert all(bool((t == FILL).all()) for t in (buf, units, count)), "a refused call wrote something"


# ------------------------------------------------------------------------------------------------------------------
# 2. the three kernels on a list
# ------------------------------------------------------------------------------------------------------------------

NB = 1024                                                 # two-row blocks: 128 per XCD, 4 per workgroup of 256, 2 of 512
SLABS = [5, 33, 64]
ROW0 = np.arange(0, 2 * NB + 1, 2)
_IN = {}


def _inputs(S):
    """Inputs, weights and the outputs of the launches without a mask at S slabs: computed once, one slab count held at a time."""
    if S not in _IN:
        _IN.clear()
        # one slab range on both grids: the list is walked, not the fallback
        assert ws._launch_grid(NB, S, 1) == (256, 1) and ws._launch_grid(NB, S, 2) == (512, 1)
        op = ws._op(NB)
        g = torch.Generator(device="cuda")
        g.manual_seed(S)
        c = dict(op=op, W=[torch.randn(32, 32, device="cuda", generator=g) * 0.3 for _ in range(3)],
                 Wf=[torch.randn(1, 32, device="cuda", generator=g) * 0.3 for _ in range(3)],
                 x1=torch.randn(S, 2 * NB, 4, 1, device="cuda", generator=g), x=torch.randn(S, 2 * NB, 4, 32, device="cuda", generator=g))
        c["y"] = op.shifted_input(c["x1"])
        assert c["y"] is not None
        c["full"] = {("y", None): c["y"]}
        for act in ("tanh", "relu"):
            c["full"][("plain", act)] = op.forward([c["x"]], c["W"], 32, act)
            c["full"][("from_y", act)] = op.forward_from_y(c["y"], c["Wf"], c["W"], act)
        assert all(t is not None for t in c["full"].values())
        _IN[S] = c
    return _IN[S]


def _host_list(k, order=None):
    """The unit list of bool [nb][S] made on the host: the indices of the non-zero words, ascending or in `order`."""
    from scone_gcn_amd import ops
    words = _pack(k).cpu().numpy().view(np.uint32).reshape(-1)
    ent = np.flatnonzero(words)
    if order is not None:
        ent = ent[order.permutation(len(ent))]
    units = torch.full((max(1, len(words)),), -1, device="cuda", dtype=torch.int32)       # (past the count: a block no plan has)
    units[:len(ent)] = torch.as_tensor(ent.astype(np.int32), device="cuda")
    return ops.UnitList(units, torch.tensor([len(ent)], device="cuda", dtype=torch.int32))


def _launch(c, form, act, k, units, op=None, full=None):
    """The masked launch of `form` into a sentinel-filled output, on the list `units` or (None) on the static walk."""
    from scone_gcn_amd import _lib, ops
    op = c["op"] if op is None else op
    full = c["full"][(form, act)] if full is None else full
    out, keep = _sentinel(full.shape), _pack(k)
    if form == "y":
        lib, S = _lib.load(), c["x1"].shape[0]
        if units is None:
            st = lib.scn_conv_shifted_input_keep(op.handle, S, 4, ops._dev(c["x1"]), ops._dev(out), ops._dev(keep, torch.int32), ops._stream())
        else:
            st = lib.scn_conv_shifted_input_keep_units(op.handle, S, 4, ops._dev(c["x1"]), ops._dev(out), ops._dev(keep, torch.int32),
                                                       *ops._unit_ptrs(units), ops._stream())
        _lib.check(st, "scn_conv_shifted_input_keep")
        got = out
    elif form == "plain":
        got = op.forward([c["x"]], c["W"], 32, act, out=out, keep=keep, units=units)
    else:
        got = op.forward_from_y(c["y"], c["Wf"], c["W"], act, keep=keep, out=out, units=units)
    assert got is not None, "masked launch not served"
    torch.cuda.synchronize()
    return got


def _mask(name, S, rs):
    k = np.zeros((NB, S), bool)
    if name == "one":                                     # exactly one entry
        k[NB // 3, S - 1] = True
    elif name == "few":                                   # fewer entries than workgroups: most workgroups get none
        k[rs.choice(NB, 100, replace=False), rs.randint(min(S, 32))] = True
        k[NB - 1, 0] = True
    elif name == "word1":                                 # entries only in word 1 (slabs from 32 on)
        k[:, 32:] = rs.rand(NB, S - 32) < 0.1
    elif name == "both":                                  # blocks with bits in both words: two entries each, each item once;
        k[0::3, 1] = True                                 # others in one word only, others empty
        k[0::3, S - 1] = True
        k[1::6, 31] = True
        k[1::6, 32] = True
        k[4::6] = rs.rand(len(k[4::6]), S) < 0.05
    elif name == "ones":                                  # every word: 4 (8 at two words) entries per workgroup of 256
        k[:] = True
    else:
        assert name == "count0"
    return k


CASES = [(S, m) for S in SLABS for m in ["count0", "one", "few", "ones"] + (["word1", "both"] if S > 32 else [])]


@pytest.mark.parametrize("S,mask", CASES)                 # (innermost: a slab count's tensors are shared)
@pytest.mark.parametrize("form,act", [("y", None), ("plain", "tanh"), ("plain", "relu"), ("from_y", "tanh"), ("from_y", "relu")])
def test_list_form_equals_the_static_walk_bit_for_bit(form, act, S, mask):
    _need_gpu()
    c = _inputs(S)
    rs = np.random.RandomState(S + len(mask))
    k = _mask(mask, S, rs)
    what = "%s %s, %d slabs, mask %s" % (form, act, S, mask)
    static = _launch(c, form, act, k, None)
    _same_bits(static.view(torch.int32), _expected(c["full"][(form, act)], k, ROW0), what + ": static walk against the launch without a mask")
    ul = _host_list(k)
    n = int(ul.count.cpu()[0])
    assert {"count0": n == 0, "one": n == 1, "few": 0 < n < 256, "ones": n == NB * ((S + 31) // 32)}.get(mask, n > 0)
    if mask == "both":
        w = _pack(k).cpu().numpy().view(np.uint32)
        assert ((w[:, 0] != 0) & (w[:, 1] != 0)).sum() > 100 and ((w[:, 0] != 0) ^ (w[:, 1] != 0)).any()
    if mask == "word1":
        assert not _pack(k).cpu().numpy()[:, 0].any()
    got = _launch(c, form, act, k, ul)
    _same_bits(got.view(torch.int32), static.view(torch.int32), what + ": list against static walk")
    if mask == "count0":
        assert rc._untouched(got)                         # the launch writes nothing
    if mask in ("few", "both", "ones", "word1"):          # the order of the entries is free
        shuffled = _launch(c, form, act, k, _host_list(k, order=np.random.RandomState(7)))
        _same_bits(shuffled.view(torch.int32), static.view(torch.int32), what + ": shuffled list against static walk")


def test_a_list_of_every_word_in_device_order_is_served_too():
    """The list as scn_mask_hop_units writes it (identity-free: a real hop over the operator's adjacency), handed to the launches."""
    _need_gpu()
    from scone_gcn_amd import _lib, ops
    S = 33
    c = _inputs(S)
    k = _mask("both", S, np.random.RandomState(1))
    v = ws._hop1(k)                                       # A(b) = {b - 1, b, b + 1}
    adj_ptr = torch.as_tensor(np.concatenate([[0], np.cumsum([3 - (b in (0, NB - 1)) for b in range(NB)])]).astype(np.int32), device="cuda")
    adj_blk = torch.as_tensor(np.concatenate([[x for x in (b - 1, b, b + 1) if 0 <= x < NB] for b in range(NB)]).astype(np.int32), device="cuda")
    out = torch.empty((NB, 2), device="cuda", dtype=torch.int32)
    units = torch.empty(2 * NB, device="cuda", dtype=torch.int32)
    count = torch.zeros(1, device="cuda", dtype=torch.int32)
    _lib.check(_lib.load().scn_mask_hop_units(NB, 2, _p(adj_ptr), _p(adj_blk), _p(_pack(k)), _p(out), _p(units), _p(count), 2 * NB,
                                              _stream()), "scn_mask_hop_units")
    torch.cuda.synchronize()
    assert torch.equal(out, _pack(v)) and int(count[0]) == int((out != 0).sum())
    for form, act in (("y", None), ("from_y", "tanh"), ("plain", "relu")):
        got = _launch(c, form, act, v, ops.UnitList(units, count))
        _same_bits(got.view(torch.int32), _expected(c["full"][(form, act)], v, ROW0), "%s on the device's list" % form)


def test_more_than_one_scan_per_workgroup():
    """131 080 two-row blocks, all ones at two slabs: 512 or 513 entries per workgroup of the 256-workgroup grid (three scans, the
    third of one entry at the most), 256 or 257 of the 512-workgroup grid (two scans) -- with every item kept the output is the launch
    without a mask, everywhere."""
    _need_gpu()
    nb, S = ws.BIG_NB, 2
    assert ws._launch_grid(nb, S, 1) == (256, 1) and ws._launch_grid(nb, S, 2) == (512, 1)
    assert -(-nb // 256) == 513 and -(-nb // 512) == 257
    op = ws._op(nb)
    k = np.ones((nb, S), bool)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    c = dict(op=op, W=[torch.randn(32, 32, device="cuda", generator=g) * 0.3 for _ in range(3)],
             Wf=[torch.randn(1, 32, device="cuda", generator=g) * 0.3 for _ in range(3)],
             x1=torch.randn(S, 2 * nb, 4, 1, device="cuda", generator=g))
    c["y"] = op.shifted_input(c["x1"])
    ul = _host_list(k, order=np.random.RandomState(3))
    assert int(ul.count.cpu()[0]) == nb
    got = _launch(c, "y", None, k, ul, full=c["y"])
    _same_bits(got.view(torch.int32), c["y"].view(torch.int32), "y, big")
    del got
    full = op.forward_from_y(c["y"], c["Wf"], c["W"], "tanh")
    got = _launch(c, "from_y", "tanh", k, ul, full=full)
    _same_bits(got.view(torch.int32), full.view(torch.int32), "from-y forward, big")
    del got
    c["x"] = full                                         # (the from-y layer's output as the plain layer's input)
    full = op.forward([c["x"]], c["W"], 32, "tanh")
    got = _launch(c, "plain", "tanh", k, ul, full=full)
    _same_bits(got.view(torch.int32), full.view(torch.int32), "plain forward, big")


# ------------------------------------------------------------------------------------------------------------------
# 3. fallback
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [64, 130])
def test_a_grid_with_more_than_one_slab_range_walks_its_static_units(S):
    _need_gpu()
    nb = 517
    assert ws._launch_grid(nb, S, 1)[1] > 1 and ws._launch_grid(nb, S, 2)[1] > 1, "the grids split the slabs"
    op = ws._op(nb)
    rs = np.random.RandomState(S)
    g = torch.Generator(device="cuda")
    g.manual_seed(S)
    c = dict(op=op, W=[torch.randn(32, 32, device="cuda", generator=g) * 0.3 for _ in range(3)],
             Wf=[torch.randn(1, 32, device="cuda", generator=g) * 0.3 for _ in range(3)],
             x1=torch.randn(S, 2 * nb, 4, 1, device="cuda", generator=g), x=torch.randn(S, 2 * nb, 4, 32, device="cuda", generator=g))
    c["y"] = op.shifted_input(c["x1"])
    k = rs.rand(nb, S) < 0.05
    k[0, 0] = k[nb - 1, S - 1] = True
    ul = _host_list(k, order=rs)
    row0 = np.arange(0, 2 * nb + 1, 2)
    for form, full in (("y", c["y"]), ("from_y", op.forward_from_y(c["y"], c["Wf"], c["W"], "tanh")), ("plain", op.forward([c["x"]], c["W"], 32, "tanh"))):
        got = _launch(c, form, "tanh", k, ul, full=full)
        _same_bits(got.view(torch.int32), _expected(full, k, row0), "%s, %d slabs on %d blocks" % (form, S, nb))


# ------------------------------------------------------------------------------------------------------------------
# 4. plan steps
# ------------------------------------------------------------------------------------------------------------------

def _batch(slabs):
    """The batch of tests/test_gpu_readout_cone.py, or its first slab (four trajectories: every launch grid has one slab range)."""
    d = rc._data()
    if slabs == 1:
        return dict(x=d["x"][:1].contiguous(), last=d["last_dev"][:4].contiguous(), y=d["y_dev"][:4].contiguous(), N=4)
    assert d["x"].shape[0] == slabs
    return dict(x=d["x"], last=d["last_dev"], y=d["y_dev"], N=d["N"])


def _step(plan, w, b, listed, monkeypatch):
    from scone_gcn_amd import ops
    monkeypatch.setattr(ops, "READOUT_CONE", True)
    monkeypatch.setattr(ops, "CONE_UNIT_LIST", listed)
    wt = [torch.tensor(a, dtype=torch.float32, device="cuda") for a in w]
    logp, saved = plan.forward(b["x"], b["last"], wt)
    loss = -(logp * b["y"]).sum() / b["N"]
    grads = [torch.zeros_like(a) for a in wt]
    plan.backward(saved, logp, -b["y"] / b["N"], b["last"], wt, grads)
    torch.cuda.synchronize()
    return logp.clone(), loss.reshape(1), grads, saved


@pytest.mark.parametrize("slabs", [1, 4])
@pytest.mark.parametrize("act,layers", [("tanh", 3), ("relu", 3), ("tanh", 4)])
def test_plan_step_with_and_without_the_unit_lists(act, layers, slabs, monkeypatch):
    _need_gpu()
    env = rc._env()
    rc._thresholds(monkeypatch)
    plan, b = env["plan"](act), _batch(slabs)
    rs = np.random.RandomState(41)
    w = [0.3 * rs.randn(*s) for s in so.weight_shapes(1, [(3, 32)] * layers, 1)]
    on = _step(plan, w, b, True, monkeypatch)
    assert rc._pools_all_zero(plan)
    off = _step(plan, w, b, False, monkeypatch)
    assert rc._pools_all_zero(plan)
    cone = on[3].cone
    assert cone is not None and off[3].cone is not None and off[3].cone.units is None
    assert cone.units is not None and len(cone.units) == layers and all(u is not None for u in cone.units)
    for m, u in zip(cone, cone.units):                    # the lists of this forward's masks
        assert int(u.count.cpu()[0]) == int((m != 0).sum()) > 0
    for m_on, m_off in zip(cone, off[3].cone):
        assert torch.equal(m_on, m_off)
    what = "%d layers of 32, %s, %d slabs" % (layers, act, slabs)
    _same_bits(on[0], off[0], what + ": logp")
    _same_bits(on[1], off[1], what + ": loss")
    for i, (a, c) in enumerate(zip(on[2], off[2])):
        _same_bits(a, c, what + ": gradient of weight %d" % i)
    assert max(float(g.abs().max()) for g in on[2]) > 0


def test_two_forwards_interleaved_on_one_plan_then_both_backwards(monkeypatch):
    """Two forwards with different last nodes on one plan with the lists on, the backwards in reverse order, then the first batch
    again: each equals a fresh plan's run with the lists off, bit for bit -- a forward's lists and counters are its own."""
    _need_gpu()
    from scone_gcn_amd import ops
    env, b = rc._env(), _batch(1)
    rc._thresholds(monkeypatch)
    monkeypatch.setattr(ops, "READOUT_CONE", True)
    rs = np.random.RandomState(23)
    w = [torch.tensor(0.3 * rs.randn(*s), dtype=torch.float32, device="cuda") for s in so.weight_shapes(1, [(3, 32)] * 3, 1)]
    x = b["x"]
    plan = env["plan"](fresh=True)
    lasts = [b["last"], torch.as_tensor(rs.randint(0, plan.n_nodes, size=4).astype(np.int32), device="cuda")]
    d_logps = [rc._randn(rs, 4, plan.max_deg) for _ in lasts]

    def backward(pl, logp, saved, last, d_logp, listed):
        assert saved.cone is not None and (saved.cone.units is not None) == listed
        grads = [torch.zeros_like(a) for a in w]
        pl.backward(saved, logp, d_logp, last, w, grads)
        return logp.clone(), grads

    monkeypatch.setattr(ops, "CONE_UNIT_LIST", False)
    alone = []
    for last, dl in zip(lasts, d_logps):
        pl = env["plan"](fresh=True)
        alone.append(backward(pl, *pl.forward(x, last, w), last, dl, False))
    monkeypatch.setattr(ops, "CONE_UNIT_LIST", True)
    fwd = [plan.forward(x, last, w) for last in lasts]
    assert fwd[0][1].cone.units[0].units.data_ptr() != fwd[1][1].cone.units[0].units.data_ptr()
    assert fwd[0][1].cone.units[0].count.data_ptr() != fwd[1][1].cone.units[0].count.data_ptr()
    mixed = [None, None]
    for j in (1, 0):
        mixed[j] = backward(plan, *fwd[j], lasts[j], d_logps[j], True)
    again = backward(plan, *plan.forward(x, lasts[0], w), lasts[0], d_logps[0], True)
    torch.cuda.synchronize()
    assert not torch.equal(alone[0][0], alone[1][0]) and rc._pools_all_zero(plan)
    for j in range(2):
        _same_bits(mixed[j][0], alone[j][0], "logp of batch %d" % j)
        for i, (a, c) in enumerate(zip(mixed[j][1], alone[j][1])):
            _same_bits(a, c, "batch %d, gradient of weight %d" % (j, i))
        assert max(float(g.abs().max()) for g in alone[j][1]) > 0
    for i, (a, c) in enumerate(zip(again[1], alone[0][1])):
        _same_bits(a, c, "third use of the pooled buffers, gradient of weight %d" % i)
