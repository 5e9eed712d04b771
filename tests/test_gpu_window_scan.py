"""GPU tests of the batched window scan of the masked blocked kernels (scn_window_scan.inc, DESIGN.md sections 3 and 7).

A masked launch no longer walks a workgroup's units one at a time; ahead of its block loop the workgroup fetches the blocks and the mask
windows of up to 256 units at once (four chunks of 64, one lane per unit), cuts the windows to its slab range and keeps, in order, the
units whose window is non-zero.  Three things are pinned here.

1. scn_window_scan_probe runs that device helper on a caller-chosen grid and writes every workgroup's sequence; it is compared, entry
   by entry, with a NumPy restatement (per workgroup: its units in order, their windows from the mask words, cut, zeros dropped).  The
   operators are tridiagonal with forced block cuts every two rows, so the block count is exact: 517 blocks give 64 or 65 units per
   workgroup of an 8-workgroup grid (one chunk; two chunks, the last of one unit), 1032 give 129 (three chunks, the last of one unit),
   and 520 workgroups on 517 blocks give one unit or none.  A scan takes 256 units; a workgroup with more comes back for the next 256
   behind its block loop: 2056 blocks give 257 units (two scans, the second of one unit), 4104 give 513 (three scans).  Masks: all
   zero, all ones, alternating, exactly one non-empty unit at positions 0 / 63 / 64 / 255 / 256 / 511 / 512 / last, non-empty units
   only in the second chunk, only in the second scan, only in the third, random ones at 1, 32, 33, 64, 65 and 130 slabs (one to five
   mask words) with slab ranges that start inside a word, and bits at or above n_it, which must be cut.
2. The five masked kernels and clear_mask_kernel on sentinel-filled buffers, against the launch without a mask restricted to the mask:
   kept rows and weight gradients bit for bit, every other byte untouched -- the mask patterns of tests/test_gpu_keep_visits.py and
   tests/test_gpu_readout_cone.py (first and last block empty, runs of skipped blocks, a single kept item), whose helpers are reused.
3. The same kernels with MORE THAN ONE SCAN per workgroup: 131 080 two-row blocks, which the launch grids (256 x 1 for the MFMA
   kernels, 512 x 1 for gather3_c1_keep_kernel: restated and asserted here) hand out as up to 513 and 257 units per workgroup, on two
   slabs (0.27 GB per tensor).  No other test reaches that path: the full-size complex has 64 or 65 units per workgroup.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import test_gpu_keep_visits as kv
from tests import test_gpu_readout_cone as rc
from tests.test_gpu_keep_last import _env as _kl_env, _expected, _need_gpu, _pack, _same_bits, _sentinel

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------------------------
# 1. the probe against its restatement
# ------------------------------------------------------------------------------------------------------------------

_OPS = {}


def _op(nb):
    """A tridiagonal operator of 2 * nb rows whose plan is cut every two rows: exactly nb blocks."""
    if nb not in _OPS:
        import scipy.sparse as sp
        from scone_gcn_amd import ops
        n = 2 * nb
        lo = sp.diags([np.full(n - 1, 0.5), np.full(n - 1, -0.25)], [-1, 1], format="csr", dtype=np.float32)
        up = sp.diags([np.full(n - 1, 0.125)], [1], format="csr", dtype=np.float32)
        start = np.zeros(n, np.uint8)
        start[0::2] = 1
        op = ops.ConvOp(n, [{"mats": [lo, up], "identity": True, "n_cols": n}], block_start=start)
        assert op.plan_info()[0] == nb, "the plan follows the forced cuts"
        _OPS[nb] = op
    return _OPS[nb]


def _words(k):
    """uint32 [nb][ceil(S / 32)] of bool [nb][S]"""
    return _pack(k).cpu().numpy().view(np.uint32)


def _restatement(words, unit_block, gx, slab0, n_it):
    """Per workgroup: its units first, first + stride, ... < last in order, the 64-bit window of each unit's block from slab0 on
    (a bit past the block's words is no slab), cut to n_it bits, the zero windows dropped."""
    nb, nw = words.shape
    row = [sum(int(words[b, w]) << (32 * w) for w in range(nw)) for b in range(nb)]
    cut = (1 << n_it) - 1
    seqs = []
    for g in range(gx):
        xcd, j, stride = g & 7, g >> 3, gx >> 3
        first, last = nb * xcd // 8 + j, nb * (xcd + 1) // 8
        seq = []
        for u in range(first, last, stride):
            b = int(unit_block[u])
            win = (row[b] >> slab0) & ((1 << 64) - 1) & cut
            if win:
                seq.append((b, win))
        seqs.append(seq)
    return seqs


def _units(nb, gx, g):
    xcd, j, stride = g & 7, g >> 3, gx >> 3
    return list(range(nb * xcd // 8 + j, nb * (xcd + 1) // 8, stride))


def _check(nb, k_or_words, S, gx, slab0, n_it, what):
    op = _op(nb)
    words = k_or_words if k_or_words.dtype == np.uint32 else _words(k_or_words)
    mask = torch.as_tensor(words.view(np.int32), device="cuda")
    got, ub = op.window_scan_probe(mask, S, gx, slab0, n_it)
    for x in range(8):                                                  # the table is a permutation inside every XCD range
        lo, hi = nb * x // 8, nb * (x + 1) // 8
        assert sorted(ub[lo:hi].tolist()) == list(range(lo, hi)), what
    want = _restatement(words, ub, gx, slab0, n_it)
    assert len(got) == gx
    for g in range(gx):
        assert got[g] == want[g], "%s: workgroup %d of %d" % (what, g, gx)
    return got, ub


def _unit_table(nb, gx):
    """unit -> block of a grid (a probe with an empty mask)."""
    _, ub = _op(nb).window_scan_probe(torch.zeros((nb, 1), device="cuda", dtype=torch.int32), 1, gx, 0, 1)
    return ub


GRIDS = [(517, 8), (1032, 8), (517, 520), (517, 16), (1032, 24), (2056, 8), (4104, 8)]


@pytest.mark.parametrize("nb,gx", GRIDS)
def test_units_per_workgroup_are_what_the_cases_need(nb, gx):
    _need_gpu()
    _op(nb)
    n = [len(_units(nb, gx, g)) for g in range(gx)]
    if (nb, gx) == (517, 8):
        assert sorted(set(n)) == [64, 65]                               # one full chunk; two chunks, the last of one unit
    if (nb, gx) == (1032, 8):
        assert set(n) == {129}                                          # three chunks, the last of one unit
    if (nb, gx) == (517, 520):
        assert sorted(set(n)) == [0, 1]
    if (nb, gx) == (2056, 8):
        assert set(n) == {257}                                          # two scans, the second of one unit
    if (nb, gx) == (4104, 8):
        assert set(n) == {513}                                          # three scans, the third of one unit
    ub = _unit_table(nb, gx)
    if gx >= nb:
        assert ub.tolist() == list(range(nb))                           # no assignment table for a grid that covers the blocks


@pytest.mark.parametrize("pattern", ["zero", "ones", "alternating", "alternating_units"])
@pytest.mark.parametrize("nb,gx", GRIDS)
def test_probe_on_uniform_masks(nb, gx, pattern):
    _need_gpu()
    S = 33
    k = np.zeros((nb, S), bool)
    if pattern == "ones":
        k[:] = True
    elif pattern == "alternating":                                      # every other block, every other slab
        k[0::2, 0::2] = True
    elif pattern == "alternating_units":                                # every other UNIT of every workgroup
        ub = _unit_table(nb, gx)
        for g in range(gx):
            k[ub[_units(nb, gx, g)[1::2]]] = True
    got, _ = _check(nb, k, S, gx, 0, 33, "%s, %d blocks" % (pattern, nb))
    n = sum(len(s) for s in got)
    assert n == {"zero": 0, "ones": nb}.get(pattern, n)
    if pattern == "ones":
        assert all(w == (1 << 33) - 1 for s in got for _, w in s)


@pytest.mark.parametrize("nb", [517, 1032, 2056, 4104])
def test_exactly_one_non_empty_unit(nb):
    """At positions 0, 63, 64, 255, 256, 511, 512 and the last of a workgroup's units (8 workgroups: 64 / 65 / 129 / 257 / 513 units):
    the last entry of a scan and the first of the next one."""
    _need_gpu()
    gx, S = 8, 5
    ub = _unit_table(nb, gx)
    for g in (0, 7, int(np.argmax([len(_units(nb, gx, g)) for g in range(gx)]))):
        units = _units(nb, gx, g)
        for pos in sorted({0, 63, 64, 255, 256, 511, 512, len(units) - 1} & set(range(len(units)))):
            k = np.zeros((nb, S), bool)
            k[ub[units[pos]], 3] = True
            got, _ = _check(nb, k, S, gx, 0, S, "one unit at position %d of workgroup %d, %d blocks" % (pos, g, nb))
            assert [len(s) for s in got] == [int(i == g) for i in range(gx)] and got[g] == [(int(ub[units[pos]]), 8)]


def test_non_empty_units_only_in_the_second_chunk():
    _need_gpu()
    nb, gx, S = 1032, 8, 40
    ub = _unit_table(nb, gx)
    rs = np.random.RandomState(2)
    k = np.zeros((nb, S), bool)
    for g in range(gx):
        for u in _units(nb, gx, g)[64:128]:
            k[ub[u]] = rs.rand(S) < 0.2
    got, _ = _check(nb, k, S, gx, 0, S, "second chunk only")
    assert all(0 < len(s) <= 64 for s in got)


@pytest.mark.parametrize("nb,lo,hi", [(2056, 256, 257), (4104, 256, 512), (4104, 512, 513), (4104, 255, 257)])
def test_non_empty_units_only_in_a_later_scan(nb, lo, hi):
    """Units [lo, hi) of every workgroup only: the second scan alone (its one unit; all 256 of it), the third alone, and the pair
    255 / 256 on either side of the first scan's end."""
    _need_gpu()
    gx, S = 8, 40
    ub = _unit_table(nb, gx)
    rs = np.random.RandomState(nb + lo)
    k = np.zeros((nb, S), bool)
    for g in range(gx):
        for u in _units(nb, gx, g)[lo:hi]:
            k[ub[u]] = rs.rand(S) < 0.2
            k[ub[u], rs.randint(S)] = True
    got, _ = _check(nb, k, S, gx, 0, S, "units %d..%d only, %d blocks" % (lo, hi, nb))
    assert all(len(s) == hi - lo for s in got)


@pytest.mark.parametrize("S,slab0,n_it", [(1, 0, 1), (32, 0, 32), (32, 5, 27), (33, 0, 33), (33, 31, 2), (64, 0, 64), (64, 33, 31),
                                          (65, 0, 64), (65, 7, 58), (65, 64, 1), (130, 0, 64), (130, 70, 60), (130, 97, 33)])
@pytest.mark.parametrize("nb,gx", [(517, 8), (1032, 8), (517, 520), (1032, 24), (2056, 8), (4104, 8)])
def test_probe_on_random_masks_at_every_word_count(nb, gx, S, slab0, n_it):
    """1 - 5 mask words per block; slab ranges that start inside a word (shifts 5, 31, 1, 7, 6, 1) and reach over two or three words."""
    _need_gpu()
    rs = np.random.RandomState(S + 131 * slab0 + nb)
    k = rs.rand(nb, S) < (0.5 / n_it)                                   # about 40 % of the windows are empty
    k[rs.randint(nb, size=8)] = True
    got, _ = _check(nb, k, S, gx, slab0, n_it, "%d slabs from %d, %d of them" % (S, slab0, n_it))
    assert 0 < sum(len(s) for s in got) < nb


@pytest.mark.parametrize("S,slab0,n_it", [(33, 0, 7), (64, 10, 20), (65, 40, 3), (130, 70, 1)])
def test_bits_at_or_above_n_it_are_cut(S, slab0, n_it):
    """Every word all ones (the bits past n_slabs in the last word included): the window is exactly n_it ones; and with only the bits
    from slab0 + n_it on set, no unit is left."""
    _need_gpu()
    nb, gx = 517, 8
    words = np.full((nb, (S + 31) // 32), 0xFFFFFFFF, np.uint32)
    got, _ = _check(nb, words, S, gx, slab0, n_it, "all ones, cut to %d" % n_it)
    assert sum(len(s) for s in got) == nb and all(w == (1 << n_it) - 1 for s in got for _, w in s)
    k = np.zeros((nb, S), bool)
    k[:, slab0 + n_it:] = True
    k[:, :slab0] = True
    got, _ = _check(nb, k, S, gx, slab0, n_it, "only bits outside the range")
    assert sum(len(s) for s in got) == 0


def test_probe_refuses_bad_grids_and_ranges():
    _need_gpu()
    from scone_gcn_amd import _lib
    op = _op(517)
    mask = torch.zeros((517, 2), device="cuda", dtype=torch.int32)
    for gx, slab0, n_it in [(0, 0, 1), (12, 0, 1), (8, 40, 1), (8, 0, 0), (8, 0, 65), (8, -1, 1)]:
        with pytest.raises(_lib.SconeHipError):
            op.window_scan_probe(mask, 40, gx, slab0, n_it)


# ------------------------------------------------------------------------------------------------------------------
# 2. the masked kernels on the new walk
# ------------------------------------------------------------------------------------------------------------------

PATTERNS = ["empty", "first", "last", "runs", "ends_empty", "random"]     # tests/test_gpu_readout_cone.py: _mask
KEEP_MASKS = ["one_first", "one_last", "one_middle", "one_two_three", "islands"]   # tests/test_gpu_keep_visits.py: _bits


@pytest.mark.parametrize("S", [5, 64])
@pytest.mark.parametrize("form", ["plain", "from_y"])
def test_kept_forward_writes_the_kept_rows_and_nothing_else(form, S):
    _need_gpu()
    env = _kl_env()
    nb = len(env["row0"]) - 1
    c = kv._case(form, "tanh", S)
    rs = np.random.RandomState(S)
    masks = [(m, kv._bits(m, nb, S)) for m in KEEP_MASKS] + [(p, rc._mask(p, nb, S, rs)) for p in PATTERNS]
    for name, k in masks:
        got = kv._kept(c, k)
        _same_bits(got.view(torch.int32), _expected(c["full"], k, env["row0"]), "%s, %d slabs, mask %s" % (form, S, name))


@pytest.mark.parametrize("S", [5, 64])
def test_kept_y_writes_the_kept_records_and_nothing_else(S):
    _need_gpu()
    from scone_gcn_amd import _lib
    env = rc._env()
    rs = np.random.RandomState(S + 1)
    x = rc._randn(rs, S, env["E"], 4, 1)
    full = env["plan"]().conv.shifted_input(x)
    assert full is not None
    for pattern in PATTERNS:
        k = rc._mask(pattern, env["nb"], S, rs)
        out = _sentinel(full.shape)
        _lib.check(rc._kept_y(env, x, _pack(k), out), "scn_conv_shifted_input_keep")
        _same_bits(out.view(torch.int32), _expected(full, k, env["row0"]), "y, %d slabs, mask %s" % (S, pattern))


@pytest.mark.parametrize("S", [5, 64])
def test_visiting_backward_gives_the_plain_dx_on_the_visited_items_and_the_plain_dw(S):
    _need_gpu()
    env = rc._env()
    rs = np.random.RandomState(300 + S)
    for pattern in PATTERNS:
        c = rc._bwd_case(env, "tanh", S, pattern, rs)
        dx, dW = rc._visit(c, "tanh")
        what = "%d slabs, M %s" % (S, pattern)
        _same_bits(dx.view(torch.int32), _expected(c["dx"], c["v"], env["row0"]), "dx, " + what)
        for g in range(3):
            _same_bits(dW[g], c["dW"][g], "dW[%d], %s" % (g, what))


@pytest.mark.parametrize("S", [5, 64])
def test_visiting_fused_first_backward_gives_the_plain_gradients(S):
    _need_gpu()
    env = rc._env()
    rs = np.random.RandomState(400 + S)
    for pattern in PATTERNS:
        c = rc._first_case(env, "tanh", S, pattern, rs)
        dW, dWf = rc._first_visit(c, "tanh")
        for g in range(3):
            _same_bits(dW[g], c["dW"][g], "dW[%d], %d slabs, M %s" % (g, S, pattern))
            _same_bits(dWf[g], c["dWf"][g], "dW_first[%d], %d slabs, M %s" % (g, S, pattern))


@pytest.mark.parametrize("S,C", [(5, 32), (64, 32), (37, 4)])
def test_masked_clear_zeroes_the_listed_items_and_nothing_else(S, C):
    _need_gpu()
    env = rc._env()
    rs = np.random.RandomState(S + C)
    n = S * env["E"] * 4 * C
    for pattern in PATTERNS + ["all"]:
        k = rc._mask(pattern, env["nb"], S, rs)
        buf = _sentinel((n + 4,))                                           # (four guard words behind the tensor)
        t = buf[:n].view(S, env["E"], 4, C)
        env["plan"]().conv.clear_mask(t, _pack(k))
        torch.cuda.synchronize()
        want = torch.where(rc._rows(k, env["row0"])[:, :, None, None], torch.zeros_like(t.view(torch.int32)),
                           torch.full_like(t.view(torch.int32), rc.SENTINEL))
        _same_bits(t.view(torch.int32), want, "%d slabs, %d channels, mask %s" % (S, C, pattern))
        assert rc._untouched(buf[n:])


def test_masked_clear_with_several_blocks_per_workgroup():
    """The clear runs on min(n_blocks, 2048) workgroups: 4200 two-row blocks give every workgroup two or three blocks, so several
    threads test their blocks at once and a workgroup walks a list of more than one (8 rows of 4 x 4 floats per block and slab)."""
    _need_gpu()
    nb, S, C = 4200, 3, 4
    op = _op(nb)
    rs = np.random.RandomState(5)
    k = rs.rand(nb, S) < 0.5
    k[0:2048:7] = False                                                     # some workgroups: an empty block ahead of a listed one
    for b in (0, 2048, 4096):                                               # workgroup 0: all three of its blocks listed
        k[b, 1] = True
    assert all(k[b::2048].any(axis=1).sum() >= 2 for b in (0, 1, 5)), "workgroups with more than one listed block"
    t = _sentinel((S, 2 * nb, 4, C))
    op.clear_mask(t, _pack(k))
    torch.cuda.synchronize()
    rows = torch.as_tensor(np.repeat(k, 2, axis=0).T, device="cuda")[:, :, None, None]
    want = torch.where(rows, torch.zeros_like(t.view(torch.int32)), torch.full_like(t.view(torch.int32), rc.SENTINEL))
    _same_bits(t.view(torch.int32), want, "clear on %d blocks" % nb)


# ------------------------------------------------------------------------------------------------------------------
# 3. more than one scan per workgroup inside the masked kernels
# ------------------------------------------------------------------------------------------------------------------

BIG_NB = 8 * (256 * 64 + 1)                                                 # 131 080 blocks, 16 385 per XCD


def _launch_grid(nb, n_slabs, per_cu):
    """The library's choice of (grid.x, grid.y) for a blocked launch (launch_grid, scn_blk_dispatch.inc), restated."""
    cap, nb_xcd, best = 256 * per_cu, (nb + 7) // 8, None
    gy = 1
    while gy <= 32 and gy <= max(1, n_slabs):
        gx = max(8, min(cap // gy, (nb + 7) // 8 * 8) // 8 * 8)
        cost = ((nb_xcd + gx // 8 - 1) // (gx // 8)) * (2 * ((n_slabs + gy - 1) // gy) + 1) * 64 + gy
        if best is None or cost < best[0]:
            best = (cost, gx, gy)
        gy *= 2
    return best[1], best[2]


_BIG = {}


def _big():
    """The operator, its unit tables on the two grids, and two masks on 2 slabs: `edges` = a few random items plus, in every XCD, the
    units at positions 255 / 256 (and 511 / 512) of the workgroup that has 513 (257) units; `later` = items only in units past the
    first scan of the 256-workgroup grid."""
    if not _BIG:
        S = 2
        assert _launch_grid(BIG_NB, S, 1) == (256, 1) and _launch_grid(BIG_NB, S, 2) == (512, 1)
        op = _op(BIG_NB)
        ub = {gx: _unit_table(BIG_NB, gx) for gx in (256, 512)}
        assert max(len(_units(BIG_NB, 256, g)) for g in range(256)) == 513      # three scans, the third of one unit
        assert max(len(_units(BIG_NB, 512, g)) for g in range(512)) == 257      # two scans, the second of one unit
        rs = np.random.RandomState(11)
        edges = rs.rand(BIG_NB, S) < 0.002
        later = np.zeros((BIG_NB, S), bool)
        for x in range(8):
            for gx, at in ((256, (255, 256, 511, 512)), (512, (255, 256))):
                u = _units(BIG_NB, gx, x)                                   # workgroup j = 0 of XCD x: the longest
                edges[ub[gx][[u[i] for i in at]], rs.randint(S)] = True
            for g in (x, x + 8, x + 248):
                u = _units(BIG_NB, 256, g)
                later[ub[256][u[256::5]], 1] = True
        _BIG.update(op=op, S=S, E=2 * BIG_NB, row0=np.arange(0, 2 * BIG_NB + 1, 2), masks={"edges": edges, "later": later})
        for name, k in _BIG["masks"].items():                               # what the kernels are to walk, pinned on the probe as well
            for gx in (256, 512):
                got, _ = _check(BIG_NB, k, S, gx, 0, S, "big, %s, grid %d" % (name, gx))
                assert sum(len(s) for s in got) == int(k.any(axis=1).sum())
                assert name != "later" or gx != 256 or any(len(s) > 0 for s in got)
    return _BIG


def _hop1(k):
    """One hop over the tridiagonal operator's block adjacency A(b) = {b - 1, b, b + 1}."""
    v = k.copy()
    v[1:] |= k[:-1]
    v[:-1] |= k[1:]
    return v


def _big_rows(k):
    return torch.as_tensor(np.repeat(k, 2, axis=0).T, device="cuda")[:, :, None, None]


@pytest.mark.parametrize("mask", ["edges", "later"])
def test_kept_forwards_and_y_past_one_scan(mask):
    _need_gpu()
    b = _big()
    op, S, E, k = b["op"], b["S"], b["E"], b["masks"][mask]
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    W = [torch.randn(32, 32, device="cuda", generator=g) * 0.3 for _ in range(3)]
    Wf = [torch.randn(1, 32, device="cuda", generator=g) * 0.3 for _ in range(3)]
    x1 = torch.randn(S, E, 4, 1, device="cuda", generator=g)
    y = op.shifted_input(x1)
    assert y is not None
    got = op.shifted_input(x1, keep=_pack(k))
    assert got is not None
    rows = _big_rows(k).expand_as(y)
    assert torch.equal(got.view(torch.int32)[rows], y.view(torch.int32)[rows]), "y on the kept items"
    from scone_gcn_amd import _lib, ops
    out = _sentinel(y.shape)
    _lib.check(_lib.load().scn_conv_shifted_input_keep(op.handle, S, 4, ops._dev(x1), ops._dev(out), ops._dev(_pack(k), torch.int32),
                                                       ops._stream()), "scn_conv_shifted_input_keep")
    torch.cuda.synchronize()
    _same_bits(out.view(torch.int32), _expected(y, k, b["row0"]), "y, big, mask " + mask)
    x = torch.randn(S, E, 4, 32, device="cuda", generator=g)
    for form, full, kept in (("plain", lambda: op.forward([x], W, 32, "tanh"),
                              lambda o: op.forward([x], W, 32, "tanh", out=o, keep=_pack(k))),
                             ("from_y", lambda: op.forward_from_y(y, Wf, W, "tanh"),
                              lambda o: op.forward_from_y(y, Wf, W, "tanh", keep=_pack(k), out=o))):
        ref = full()
        assert ref is not None
        got = kept(_sentinel(ref.shape))
        assert got is not None, "kept forward not served"
        torch.cuda.synchronize()
        _same_bits(got.view(torch.int32), _expected(ref, k, b["row0"]), "%s forward, big, mask %s" % (form, mask))


@pytest.mark.parametrize("mask", ["edges", "later"])
def test_visiting_backwards_past_one_scan(mask):
    _need_gpu()
    b = _big()
    op, S, E, m = b["op"], b["S"], b["E"], b["masks"][mask]
    v = _hop1(m)
    g = torch.Generator(device="cuda")
    g.manual_seed(4)
    W = [torch.randn(32, 32, device="cuda", generator=g) * 0.3 for _ in range(3)]
    Wf = [torch.randn(1, 32, device="cuda", generator=g) * 0.3 for _ in range(3)]
    dz = torch.randn(S, E, 4, 32, device="cuda", generator=g) * _big_rows(m)
    aux = torch.tanh(torch.randn(S, E, 4, 32, device="cuda", generator=g))
    dW0 = [torch.randn(32, 32, device="cuda", generator=g) for _ in range(3)]
    ref = [t.clone() for t in dW0]
    dx = op.backward([dz], W, aux, "tanh", True, ref)
    dW = [t.clone() for t in dW0]
    got = op.backward([dz], W, aux, "tanh", True, dW, dx=_sentinel(dx.shape), visit=_pack(v))
    assert got is not False, "visiting backward not served"
    torch.cuda.synchronize()
    _same_bits(got.view(torch.int32), _expected(dx, v, b["row0"]), "dx, big, mask " + mask)
    for i in range(3):
        _same_bits(dW[i], ref[i], "dW[%d], big, mask %s" % (i, mask))
    del dx, got, aux
    y = op.shifted_input(torch.randn(S, E, 4, 1, device="cuda", generator=g))
    dWf0 = [torch.randn(1, 32, device="cuda", generator=g) for _ in range(3)]
    ref, ref_f = [t.clone() for t in dW0], [t.clone() for t in dWf0]
    assert op.backward_fused_first(dz, W, None, "tanh", y, ref, ref_f, Ws_first=Wf)
    dW, dWf = [t.clone() for t in dW0], [t.clone() for t in dWf0]
    assert op.backward_fused_first(dz, W, None, "tanh", y, dW, dWf, Ws_first=Wf, visit=_pack(v)), "not served"
    torch.cuda.synchronize()
    for i in range(3):
        _same_bits(dW[i], ref[i], "fused first dW[%d], big, mask %s" % (i, mask))
        _same_bits(dWf[i], ref_f[i], "dW_first[%d], big, mask %s" % (i, mask))
