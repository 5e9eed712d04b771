"""Host tests of the block plan AT ITS LIMITS (csrc/scn_blk_plan.inc: grow_block / build_block_plan; csrc/scn_blk_layout.inc), and
the builders of the hand-made operators that tests/test_gpu_block_plan_limits.py runs the blocked kernels on.

A plan block is closed by one of four limits -- 64 rows, 128 distinct staged sources, 1152 padded ELL entries, a padded width above
254 -- or by a `block_start` hint; a row that fits no block leaves the operator without a plan.  Three things are pinned here, all on
the CPU:

1. `restate_cut`: a NumPy / set restatement of the greedy cut that also names WHY every block was closed.  The library's own
   block count (scn_plan_gather_stats, which lays every block out and runs the layout's entry-by-entry self-check) must equal it
   on every operator below and on a seeded family of heavy-tailed random patterns with four markings of the second operator and
   three hint settings; a pattern with a row that fits no block must give a non-zero status and the restatement's "no plan".
2. The operators are built from hinted ROW GROUPS, each made to meet one limit (GROUP_ROWS).  That they really do is asserted from
   the restatement's reasons: a block closed by each of rows / sources / ELL cap / hint, one with exactly 128 sources, one with
   rows * width == 1152, one of width 128, one without entries.
3. The group sequence of the large operator is a seeded shuffle, not a cycle (a workgroup's consecutive blocks lie a fixed stride
   apart, and a cycle would hand it the same kind again).
"""
import ctypes

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")

BK_R, BK_SRC, BK_ELL_CAP, W_MAX = 64, 128, 1152, 254

# ------------------------------------------------------------------------------------------------------------------
# the greedy cut, restated
# ------------------------------------------------------------------------------------------------------------------


def restate_cut(rowptr, col, identity, hint=None):
    """The plan's blocks as [(row0, rows, sources, padded width, reason)], reason in rows / sources / ELL / width / hint / end (what
    stopped the block from taking its next row), or None: "no plan" (a row fits no block).  identity: the rows themselves are staged."""
    n = len(rowptr) - 1
    blocks, r0 = [], 0
    while r0 < n:
        r_limit, hinted = n, False
        if hint is not None:
            for r in range(r0 + 1, min(n, r0 + BK_R + 1)):
                if hint[r]:
                    r_limit, hinted = r, True
                    break
        seen, rows, w, reason = set(), 0, 0, None
        while True:
            if rows == BK_R:
                reason = "rows"
                break
            if r0 + rows == r_limit:
                reason = "hint" if hinted else "end"
                break
            r = r0 + rows
            cols = col[rowptr[r]:rowptr[r + 1]]
            new = set(int(c) for c in cols) - seen
            if identity:
                new.add(r)
                new -= seen
            nw = max(w, (len(cols) + 1) & ~1)
            if len(seen) + len(new) > BK_SRC:
                reason = "sources"
            elif nw * (rows + 1) > BK_ELL_CAP:
                reason = "ELL"
            elif nw > W_MAX:
                reason = "width"
            if reason:
                break
            seen |= new
            w = nw
            rows += 1
        if rows == 0:
            return None
        blocks.append((r0, rows, len(seen), w, reason))
        r0 += rows
    return blocks


def gather_stats(rowptr, col, val1, identity, hint):
    """(status, blocks) of scn_plan_gather_stats: the library's cut with every block laid out and self-checked."""
    from scone_gcn_amd import _lib
    lib = _lib.load()
    rowptr, col = np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(col, np.int32)
    val1 = None if val1 is None else np.ascontiguousarray(val1, np.float32)
    hint = None if hint is None else np.ascontiguousarray(hint, np.uint8)
    out = np.full(4, -1, np.int64)
    as_p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    st = lib.scn_plan_gather_stats(len(rowptr) - 1, as_p(rowptr), as_p(col), None if val1 is None or not len(val1) else val1.ctypes.data,
                                   int(identity), None if hint is None else hint.ctypes.data, out.ctypes.data)
    return int(st), int(out[3])


# ------------------------------------------------------------------------------------------------------------------
# the operators: hinted row groups, each made for one limit
# ------------------------------------------------------------------------------------------------------------------

GROUP_ROWS = {
    "r64": 64,        # 1..7 entries per row inside a 104-column window: closed by the row limit
    "wide": 1,        # 127 off-diagonal entries from anywhere: with the row itself 128 sources, width 128, one row
    "ell": 40,        # 36 entries in a sliding window: 32 rows x 36 = 1152 = the ELL cap, 8 rows left
    "hub11": 11,      # row 4 has 100 entries, rows 1 / 2 / 7 (its quad) have 0 / 1 / 2, the others 0..3
    "empty5": 5,      # no entries: identity reads only
    "g1": 1, "g2": 2, "g7": 7, "g8": 8, "g9": 9, "g63": 63,   # 1..3 entries: the edges of a wave's eight rows and of the last wave
    "second12": 12,   # 1..5 entries; every other row has val0 == 0 on all of them (it feeds the second operator only)
    "over": 1,        # 128 off-diagonal entries: 129 sources, fits no block (the fallback operator only)
}
KINDS = tuple(k for k in GROUP_ROWS if k != "over")
TAIL_ROWS = 150       # unhinted, 4 entries per row in the tail's own columns: the greedy cut closes these blocks on the source cap
WINDOW = 104          # columns a local group draws from: its own rows and 40 more (<= 128 sources with the rows themselves)
MIXED_REPEATS, MIXED_SEED = 70, 0


def _pick(rs, lo, hi, k, row):
    """k distinct columns of [lo, hi) without the diagonal, ascending"""
    c = lo + rs.choice(hi - lo, size=min(hi - lo, k + 1), replace=False)
    return np.sort(c[c != row][:k])


def build_operator(kinds, tail_rows, seed, n_cols=None, hinted=True):
    """The operator of a group sequence: dict with n, n_cols, the union pattern (rowptr, col), val0 / val1 on it (float32; an entry
    has val0 != 0 unless its row feeds the second operator only, and val1 != 0 on about 40 % of the entries), the hint, and
    groups = [(kind, first row)].  n_cols: a rectangular operator over that many columns (the windows are scaled)."""
    rs = np.random.RandomState(seed)
    n = sum(GROUP_ROWS[k] for k in kinds) + tail_rows
    nc = n if n_cols is None else n_cols
    assert nc >= 130 and n - tail_rows >= 0
    cols, v0, v1, hint, groups = [], [], [], np.zeros(n, np.uint8), []

    def window(g0):
        start = min(max(g0 * nc // n - 20, 0), nc - WINDOW)
        return start, start + WINDOW

    def row(r, c, second_only=False):
        a = rs.randn(len(c)).astype(np.float32)
        b = rs.randn(len(c)).astype(np.float32)
        cols.append(c)
        v0.append(a * 0 if second_only else a)
        v1.append(b if second_only else b * (rs.rand(len(c)) < 0.4))

    r = 0
    for kind in kinds:
        g0, m = r, GROUP_ROWS[kind]
        hint[g0] = 1
        groups.append((kind, g0))
        lo, hi = window(g0)
        for i in range(m):
            if kind == "r64":
                row(r, _pick(rs, lo, hi, rs.randint(1, 8), r))
            elif kind in ("wide", "over"):
                row(r, _pick(rs, 0, nc, 127 if kind == "wide" else 128, r))
            elif kind == "ell":
                base = min(lo + i // 2, nc - 36)
                row(r, np.arange(base, base + 36))
            elif kind == "hub11":
                k = {4: 100, 1: 0, 2: 1, 7: 2}.get(i, rs.randint(0, 4))
                row(r, _pick(rs, lo, hi, k, r))
            elif kind == "empty5":
                row(r, np.zeros(0, np.int64))
            elif kind == "second12":
                row(r, _pick(rs, lo, hi, rs.randint(1, 6), r), second_only=i % 2 == 1)
            else:
                row(r, _pick(rs, lo, hi, rs.randint(1, 4), r))
            r += 1
    if tail_rows:
        hint[r] = 1
        t0 = r * nc // n
        for i in range(tail_rows):
            row(r, _pick(rs, t0, nc, 4, r))
            r += 1
    rowptr = np.zeros(n + 1, np.int32)
    rowptr[1:] = np.cumsum([len(c) for c in cols])
    op = dict(n=n, n_cols=nc, rowptr=rowptr, col=np.concatenate(cols).astype(np.int32), val0=np.concatenate(v0), val1=np.concatenate(v1),
              hint=hint if hinted else None, groups=groups, identity=n_cols is None)
    assert ((op["val0"] != 0) | (op["val1"] != 0)).all(), "every entry of the union pattern carries a value"
    return op


def matrices(op):
    """[lo, up] (or [lo] for one value array): the value arrays as float32 CSR without explicit zeros (their union is the
    operator's pattern)."""
    out = []
    for v in (op["val0"], op["val1"]):
        if v is None:
            continue
        m = sp.csr_matrix((v, op["col"], op["rowptr"]), shape=(op["n"], op["n_cols"]), copy=True)
        m.eliminate_zeros()
        m.sort_indices()
        out.append(m)
    return out


def from_matrices(lo, up, hint, identity=True):
    """The operator dict of two CSR matrices (their union pattern; no groups)."""
    from scone_gcn_amd.complex import union_pattern
    rowptr, col, vals = union_pattern([lo, up] if up is not None else [lo])
    return dict(n=lo.shape[0], n_cols=lo.shape[1], rowptr=rowptr, col=col, val0=vals[0], val1=vals[1] if up is not None else None,
                hint=hint, groups=[], identity=identity)


def mixed_kinds(repeats=MIXED_REPEATS, seed=MIXED_SEED):
    """Every kind `repeats` times in a seeded shuffled order."""
    seq = [k for k in KINDS for _ in range(repeats)]
    np.random.RandomState(seed).shuffle(seq)
    return seq


_CACHE = {}


def operator(name):
    """small: each group once, then the tail.  mixed: the groups 70 times over, shuffled, then the tail.  unhinted: small without
    hints.  nonsym / nonsym_T: small with a third of the entries below the diagonal dropped, and its transpose (same hints).
    power / mixed_power: identity + ONE value array on small's / mixed's pattern.  rect: one value array, no identity, the same groups over n / 2 columns.
    noplan: small plus one row of 128 off-diagonal entries (129 sources)."""
    if name in _CACHE:
        return _CACHE[name]
    if name == "small":
        op = build_operator(KINDS, TAIL_ROWS, 1)
    elif name == "mixed":
        op = build_operator(mixed_kinds(), TAIL_ROWS, 2)
    elif name == "unhinted":
        op = dict(operator("small"), hint=None)
    elif name in ("nonsym", "nonsym_T"):
        s = operator("small")
        lo, up = (m.tocoo() for m in matrices(s))
        drop = np.random.RandomState(3).rand(s["n"], s["n"]) < 1.0 / 3
        mats = []
        for m in (lo, up):
            keep = ~((m.col < m.row) & drop[m.row, m.col])
            m = sp.csr_matrix((m.data[keep], (m.row[keep], m.col[keep])), shape=m.shape)
            mats.append(m.T.tocsr() if name == "nonsym_T" else m)
        for m in mats:
            m.sort_indices()
        op = from_matrices(mats[0], mats[1], s["hint"])
    elif name in ("power", "mixed_power"):
        s = operator("small" if name == "power" else "mixed")
        op = dict(s, val0=np.where(s["val0"] != 0, s["val0"], s["val1"]), val1=None)
    elif name == "rect":
        s = operator("small")
        op = build_operator(KINDS, TAIL_ROWS, 4, n_cols=s["n"] // 2)
        op = dict(op, val0=np.where(op["val0"] != 0, op["val0"], op["val1"]), val1=None)
    elif name == "noplan":
        op = build_operator(KINDS + ("over",), TAIL_ROWS, 1)
    else:
        raise KeyError(name)
    _CACHE[name] = op
    return op


def cut_of(name):
    key = ("cut", name)
    if key not in _CACHE:
        op = operator(name)
        _CACHE[key] = restate_cut(op["rowptr"], op["col"], op["identity"], op["hint"])
    return _CACHE[key]


WITH_PLAN = ["small", "mixed", "unhinted", "nonsym", "nonsym_T", "power", "rect"]

# ------------------------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", WITH_PLAN)
def test_library_cut_and_layout_on_the_operators(name):
    op, cut = operator(name), cut_of(name)
    assert cut is not None
    st, blocks = gather_stats(op["rowptr"], op["col"], op["val1"], op["identity"], op["hint"])
    assert st == 0, "status %d: -7 is a block whose layout lost or moved an entry" % st
    assert blocks == len(cut)
    assert sum(b[1] for b in cut) == op["n"] and all(b[1] <= BK_R and b[2] <= BK_SRC and b[1] * b[3] <= BK_ELL_CAP for b in cut)


def test_operator_without_a_plan():
    op = operator("noplan")
    assert cut_of("noplan") is None
    st, _ = gather_stats(op["rowptr"], op["col"], op["val1"], 1, op["hint"])
    assert st != 0
    # without the identity read the same row has 128 sources and a width of 128: it fits
    assert restate_cut(op["rowptr"], op["col"], False, op["hint"]) is not None
    assert gather_stats(op["rowptr"], op["col"], op["val1"], 0, op["hint"])[0] == 0


def _block_of(cut, row):
    return next(b for b in cut if b[0] <= row < b[0] + b[1])


def test_small_meets_every_limit_it_is_built_for():
    op, cut = operator("small"), cut_of("small")
    first = {k: g0 for k, g0 in op["groups"]}
    assert 350 <= op["n"] <= 400 and 14 <= len(cut) <= 24
    reasons = {b[4] for b in cut}
    assert {"rows", "sources", "ELL", "hint", "end"} <= reasons
    assert _block_of(cut, first["r64"]) == (first["r64"], 64, _block_of(cut, first["r64"])[2], 8, "rows")
    assert _block_of(cut, first["wide"]) == (first["wide"], 1, 128, 128, "hint")          # exactly 128 sources, width 128, one row
    assert _block_of(cut, first["ell"])[:2] + _block_of(cut, first["ell"])[3:] == (first["ell"], 32, 36, "ELL")   # 32 x 36 == 1152
    assert _block_of(cut, first["ell"] + 32)[:2] == (first["ell"] + 32, 8)
    assert any(b[1] * b[3] == BK_ELL_CAP for b in cut)
    hub = _block_of(cut, first["hub11"])
    assert hub[:2] == (first["hub11"], 11) and hub[3] == 100 and hub[4] == "hint"
    nnz = np.diff(op["rowptr"])[first["hub11"]:first["hub11"] + 11]
    assert [int(nnz[i]) for i in (1, 2, 4, 7)] == [0, 1, 100, 2]                           # the quad {1, 2, 4, 7} of the first wave
    assert _block_of(cut, first["empty5"]) == (first["empty5"], 5, 5, 0, "hint")          # no entries: width 0, the rows themselves
    for k in ("g1", "g2", "g7", "g8", "g9", "g63", "second12"):
        b = _block_of(cut, first[k])
        assert b[:2] == (first[k], GROUP_ROWS[k]) and b[4] == "hint" and 2 <= b[3] <= 6
    s0 = first["second12"]
    for i in range(12):
        v = op["val0"][op["rowptr"][s0 + i]:op["rowptr"][s0 + i + 1]]
        assert len(v) >= 1 and (v == 0).all() == (i % 2 == 1)
    assert {int(x) for x in np.diff(op["rowptr"])[s0:s0 + 12]} & {1, 3, 5}, "odd entry counts occur"
    tail = [b for b in cut if b[0] >= op["n"] - TAIL_ROWS]
    assert len(tail) >= 3 and all(b[4] == "sources" for b in tail[:-1]) and tail[-1][4] == "end" and all(b[3] == 4 for b in tail)


def test_the_other_operators_are_what_they_are_meant_to_be():
    small, un = cut_of("small"), cut_of("unhinted")
    assert [b[0] for b in un] != [b[0] for b in small]
    assert not any(b[4] == "hint" for b in un) and len(un) < len(small)
    assert sum(b[4] == "sources" for b in un) >= 3 and any(b[4] == "ELL" for b in un) and any(b[4] == "rows" for b in un)
    ns, nt = operator("nonsym"), operator("nonsym_T")
    assert ns["rowptr"][-1] < operator("small")["rowptr"][-1] and ns["rowptr"][-1] == nt["rowptr"][-1]
    lo, up = matrices(ns)
    lt, ut = matrices(nt)
    assert abs(lo.T - lt).nnz == 0 and abs(up.T - ut).nnz == 0 and abs(lo - lo.T).nnz > 0
    rect = operator("rect")
    assert rect["n_cols"] == operator("small")["n"] // 2 and not rect["identity"] and rect["val1"] is None
    assert any(b[1:4] == (1, 127, 128) for b in cut_of("rect")), "the one-row block of width 128 (127 sources without the identity)"
    assert any(b[2] == 0 and b[3] == 0 for b in cut_of("rect")), "a block that stages nothing"
    assert operator("power")["val1"] is None and (operator("power")["val0"] != 0).all()


def test_mixed_is_large_shuffled_and_repeats_every_limit():
    op, cut = operator("mixed"), cut_of("mixed")
    assert len(cut) > 768, "more blocks than the largest grid has workgroups per slab range"
    assert 15000 <= op["n"] <= 17000
    kinds = [k for k, _ in op["groups"]]
    assert sorted(kinds) == sorted(KINDS * MIXED_REPEATS)
    assert len({tuple(kinds[i:i + len(KINDS)]) for i in range(0, len(kinds), len(KINDS))}) > MIXED_REPEATS // 2, "not a cycle"
    assert sum(b[1:4] == (1, 128, 128) for b in cut) == MIXED_REPEATS
    assert sum(b[4] == "ELL" and b[1] * b[3] == BK_ELL_CAP for b in cut) == MIXED_REPEATS
    assert sum(b[4] == "rows" for b in cut) >= MIXED_REPEATS
    assert sum(b[3] == 0 for b in cut) == MIXED_REPEATS
    assert any(b[4] == "sources" for b in cut)


def _heavy_tailed(rs, n):
    """rows of 0..126 entries (Pareto counts), columns anywhere"""
    rows = []
    for r in range(n):
        k = int(min(126, rs.pareto(1.2) * 2))
        c = rs.choice(n, size=k, replace=False) if k else np.zeros(0, np.int64)
        rows.append(np.sort(c))
    rowptr = np.zeros(n + 1, np.int32)
    rowptr[1:] = np.cumsum([len(c) for c in rows])
    return rowptr, np.concatenate(rows).astype(np.int32)


def _star(rs, n, hub_entries):
    """a band with one hub row of `hub_entries` off-diagonal entries"""
    rows = [np.array([c for c in (r - 1, r + 1) if 0 <= c < n], np.int64) for r in range(n)]
    h = n // 2
    c = rs.choice(n - 1, size=hub_entries, replace=False)
    rows[h] = np.sort(c + (c >= h))
    rowptr = np.zeros(n + 1, np.int32)
    rowptr[1:] = np.cumsum([len(c) for c in rows])
    return rowptr, np.concatenate(rows).astype(np.int32)


def test_seeded_random_patterns_against_the_restatement():
    """Heavy-tailed rows and hub rows at and past the source cap; second-operator markings none / random / all / all-zero val1;
    hints none / every row / random."""
    rs = np.random.RandomState(7)
    pats = [("heavy %d" % i, _heavy_tailed(rs, 260 + 13 * i)) for i in range(20)]
    pats += [("hub %d" % k, _star(rs, 300, k)) for k in (126, 127, 128, 140)]
    no_plan = 0
    for name, (rowptr, col) in pats:
        n, nnz = len(rowptr) - 1, len(col)
        for marking in ("none", "random", "all", "zero"):
            val1 = {"none": None, "random": (rs.rand(nnz) < 0.4).astype(np.float32), "all": np.ones(nnz, np.float32),
                    "zero": np.zeros(nnz, np.float32)}[marking]
            for hints in ("none", "every", "random"):
                hint = {"none": None, "every": np.ones(n, np.uint8), "random": (rs.rand(n) < 0.1).astype(np.uint8)}[hints]
                cut = restate_cut(rowptr, col, True, hint)
                st, blocks = gather_stats(rowptr, col, val1, 1, hint)
                what = "%s, val1 %s, hints %s" % (name, marking, hints)
                if cut is None:
                    assert st != 0, what
                    no_plan += 1
                else:
                    assert st == 0 and blocks == len(cut), what
                    if hints == "every":
                        assert blocks == n
    assert no_plan == 2 * 12, "the hub rows with 129 and 141 sources, and nothing else, fit no block"
