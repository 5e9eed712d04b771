"""GPU tests of the unit pipeline of the two visiting backwards (csrc/scn_blk_bwd.inc, ops.VISIT_PREFETCH): a unit's prologue fetches
the next unit's source rows, its last visit stages the next unit's first slab, and the staging parity runs over the workgroup's whole
visit sequence.  No arithmetic changes, so everything is compared BIT FOR BIT (int32 views):

  * against the same call with the switch off (the unit loop without the pipeline), and
  * against the plain (non-visiting) backward on a dz that is exactly zero outside the rows of a set M with V = hop(M) visited,

with aux / y outside V and dz outside what V stages pre-filled with NaN, dx pre-filled with a sentinel no kernel produces (nothing
outside the visited items may be written), tanh and relu, the plain and the fused-first from-y form.

The operators are hand-built with block hints, so that one workgroup of the launch runs MANY units (the golden complexes of the
other cone tests give every workgroup one block at the most: no unit there has a successor):

  * `tri`: 1 024 two-row blocks of a tridiagonal operator, 4 units per workgroup of the 256 x 1 grid, at 5, 33 and 64 slabs;
  * `mixed`: 2 048 blocks of three kinds in a seeded order -- 64 rows on 128 sources, 2 rows on their own 2 sources, one row
    without any entry -- so that a wide block hands over to a narrow one and back, a tall one to a short one, an entry-less one to a
    filled one;
  * `long`: 131 080 one-row blocks, 513 units per workgroup = three table scans, every unit visited: a visit in the last entry of
    one scan and in the first of the next.

Each back-to-back pattern is asserted on the launch's own unit sequences (scn_window_scan_probe), so that no case passes by never
meeting it.  Then one plan step (three layers of 32, tanh) with the switch on against off."""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")

from tests.test_gpu_keep_last import _expected, _need_gpu, _pack, _same_bits, _sentinel
from tests.test_gpu_top_dz_mask import _rows

pytestmark = pytest.mark.gpu

_OPS = {}


def _block_adjacency(mat, row0):
    """bool [nb][nb]: A[b, b'] = block b stages a row of block b' (an entry of its rows, or the identity)."""
    nb = len(row0) - 1
    blk = np.repeat(np.arange(nb), np.diff(row0))
    coo = mat.tocoo()
    A = sp.csr_matrix((np.ones(coo.nnz + len(blk)), (np.r_[blk[coo.row], blk], np.r_[blk[coo.col], blk])), shape=(nb, nb))
    return A.tocsr() > 0


def _operator(name):
    """dict(op, row0, adj, kinds): the ConvOp (identity + two value arrays on one pattern), its block starts, block adjacency and, for
    `mixed`, the kind of every block."""
    if name in _OPS:
        return _OPS[name]
    from scone_gcn_amd import ops
    rs = np.random.RandomState(7)
    kinds = None
    if name in ("tri", "long"):
        rows_per, nb = (2, 1024) if name == "tri" else (1, 131080)
        n = nb * rows_per
        i = np.arange(n - 1)
        r, c = np.r_[i, i + 1], np.r_[i + 1, i]
        sizes = np.full(nb, rows_per)
    else:
        assert name == "mixed"
        kinds = rs.randint(0, 3, size=2048)                   # 0: 64 rows on 128 sources, 1: 2 rows on 2 sources, 2: one row, no entry
        kinds[-3:] = 1                                          # (a wide block's 64 extra sources lie behind it)
        sizes = np.array([64, 2, 1])[kinds]
        starts = np.r_[0, np.cumsum(sizes)]
        n = int(starts[-1])
        r, c = [], []
        for b, k in enumerate(kinds):
            s = int(starts[b])
            if k == 0:                                          # row j: its neighbour in the block and two of the 64 rows behind the block
                j = np.arange(64)
                r += [s + j, s + j, s + j]
                c += [s + (j + 1) % 64, np.minimum(s + 64 + j, n - 1), np.minimum(s + 64 + (j + 7) % 64, n - 1)]
            elif k == 1:
                r += [np.array([s, s + 1])]
                c += [np.array([s + 1, s])]
        r, c = np.concatenate(r), np.concatenate(c)
    lo = sp.csr_matrix((rs.uniform(0.2, 1.0, len(r)).astype(np.float32), (r, c)), shape=(n, n))
    lo.sum_duplicates()
    up = lo.copy()
    up.data = np.where(rs.rand(len(up.data)) < 0.5, rs.uniform(-1.0, -0.2, len(up.data)), 0.0).astype(np.float32)
    up.eliminate_zeros()
    hint = np.zeros(n, np.uint8)
    hint[np.r_[0, np.cumsum(sizes)[:-1]]] = 1
    op = ops.ConvOp(n, [{"mats": [lo, up], "identity": True, "n_cols": n}], block_start=hint)
    row0 = np.asarray(op.plan_blocks(), np.int64)
    assert row0.tolist() == np.r_[0, np.cumsum(sizes)].tolist(), "the plan keeps the hinted cuts"
    _OPS[name] = dict(op=op, row0=row0, adj=_block_adjacency(lo, row0), kinds=kinds, n=n, nb=len(sizes))
    return _OPS[name]


def _grid(nb, n_slabs):
    """(grid.x, grid.y) of a backward launch (one workgroup per CU, 256 CUs; launch_grid of csrc/scn_blk_dispatch.inc restated)."""
    best = None
    gy = 1
    while gy <= 32 and gy <= max(1, n_slabs):
        gx = max(8, min(256 // gy, (nb + 7) // 8 * 8) // 8 * 8)
        cost = (((nb + 7) // 8 + gx // 8 - 1) // (gx // 8)) * (2 * ((n_slabs + gy - 1) // gy) + 1) * 64 + gy
        if best is None or cost < best[0]:
            best = (cost, gx, gy)
        gy *= 2
    return best[1], best[2]


def _sequences(o, v, S):
    """every workgroup's [(block, visits), ...] in visiting order, from the launch's own walk; dense grids of one slab range here"""
    gx, gy = _grid(o["nb"], S)
    assert gy == 1, "the cases are sized for one slab range"
    seqs, _ = o["op"].window_scan_probe(_pack(v), S, gx, 0, S)
    out = [[(b, bin(w).count("1")) for b, w in s] for s in seqs]
    for s in out:
        for b, k in s:
            assert k == int(v[b].sum())
    return out


def _case(name, act, S, m, seed):
    """dz = 0 outside the rows of M, V = hop(M); the plain backward's results of both forms, computed once per case."""
    o = _operator(name)
    rs = np.random.RandomState(seed)
    v = np.asarray((o["adj"] @ m.astype(np.float64)) > 0)                     # every block that stages a row of M
    staged = np.asarray((o["adj"].T @ v.astype(np.float64)) > 0)             # the items some visited item stages
    n = o["n"]
    t = lambda *shape: torch.as_tensor(rs.randn(*shape).astype(np.float32), device="cuda")   # noqa: E731
    dz = t(S, n, 4, 32) * _rows(m, o["row0"])[:, :, None, None]
    W = [0.3 * t(32, 32) for _ in range(3)]
    Wf = [0.3 * t(1, 32) for _ in range(3)]
    h = t(S, n, 4, 32)
    aux = torch.tanh(h) if act == "tanh" else torch.relu(h)
    y = t(S, n, 4, 4)
    dW0, dWf0 = [t(32, 32) for _ in range(3)], [t(1, 32) for _ in range(3)]
    nan = torch.full((), float("nan"), device="cuda")
    out_v = _rows(~v, o["row0"])[:, :, None, None]
    c = dict(o=o, S=S, act=act, m=m, v=v, mask=_pack(v), W=W, Wf=Wf, dW0=dW0, dWf0=dWf0, dz=dz, aux=aux, y=y,
             dz_p=torch.where(_rows(~staged, o["row0"])[:, :, None, None], nan, dz), aux_p=torch.where(out_v, nan, aux),
             y_p=torch.where(out_v, nan, y))
    dW = [a.clone() for a in dW0]
    c["dx"] = o["op"].backward([dz], W, aux, act, True, dW)
    c["dW"] = dW
    dW2, dWf = [a.clone() for a in dW0], [a.clone() for a in dWf0]
    assert o["op"].backward_fused_first(dz, W, None, act, y, dW2, dWf, Ws_first=Wf) is not False
    c["dW2"], c["dWf"] = dW2, dWf
    torch.cuda.synchronize()
    return c


def _run_visits(c, on, monkeypatch):
    """both visiting forms on the poisoned tensors with the switch set: (dx, dW, dW of the fused form, dW_first)"""
    from scone_gcn_amd import ops
    monkeypatch.setattr(ops, "VISIT_PREFETCH", on)
    op = c["o"]["op"]
    dW = [a.clone() for a in c["dW0"]]
    dx = op.backward([c["dz_p"]], c["W"], c["aux_p"], c["act"], True, dW, dx=_sentinel(c["dz"].shape), visit=c["mask"])
    assert dx is not False, "visiting backward not served"
    dW2, dWf = [a.clone() for a in c["dW0"]], [a.clone() for a in c["dWf0"]]
    assert op.backward_fused_first(c["dz_p"], c["W"], None, c["act"], c["y_p"], dW2, dWf, Ws_first=c["Wf"], visit=c["mask"]) is not False
    torch.cuda.synchronize()
    return dx, dW, dW2, dWf


def _check(c, what, monkeypatch):
    on, off = _run_visits(c, True, monkeypatch), _run_visits(c, False, monkeypatch)
    want_dx = _expected(c["dx"], c["v"], c["o"]["row0"])
    for tag, got in (("pipeline", on), ("switch off", off)):
        _same_bits(got[0].view(torch.int32), want_dx, "dx on the visited items, sentinel elsewhere (%s), %s" % (tag, what))
        for g in range(3):
            _same_bits(got[1][g], c["dW"][g], "dW[%d] against the plain backward (%s), %s" % (g, tag, what))
            _same_bits(got[2][g], c["dW2"][g], "fused form's dW[%d] against the plain one (%s), %s" % (g, tag, what))
            _same_bits(got[3][g], c["dWf"][g], "dW_first[%d] against the plain fused backward (%s), %s" % (g, tag, what))
    for a, b in zip(on, off):
        for x, z in zip(a, b) if isinstance(a, list) else [(a, b)]:
            _same_bits(x, z, "pipeline against the switch off, " + what)
    assert float(c["dx"].abs().max()) > 0 and max(float((a - b).abs().max()) for a, b in zip(c["dW"], c["dW0"])) > 0, "the case contracts nothing"


def _pairs(seqs):
    """the (visits of a unit, visits of the next unit) pairs that occur back to back in some workgroup"""
    return {(a[1], b[1]) for s in seqs for a, b in zip(s, s[1:])}


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("S", [5, 33, 64])
def test_tridiagonal_units_of_one_two_and_three_visits_in_every_order(S, act, monkeypatch):
    """M: a seeded third of the blocks with 1 .. 3 slabs each, plus a zero slab: dz of slab S - 1 is all zero, so every visit there is
    the zero-tile early-out -- as a unit's last visit it still has to stage the next unit."""
    _need_gpu()
    o = _operator("tri")
    rs = np.random.RandomState(S)
    m = np.zeros((o["nb"], S), bool)
    for b in np.flatnonzero(rs.rand(o["nb"]) < 0.3):
        m[b, rs.choice(S, size=rs.randint(1, 4), replace=False)] = True
    c = _case("tri", act, S, m, 10 * S + (act == "relu"))
    c["dz"][S - 1].zero_()
    c.update(_case_refresh(c))
    seqs = _sequences(o, c["v"], S)
    want = {(a, b) for a in (1, 2, 3) for b in (1, 2, 3)}
    assert want <= _pairs(seqs), "a back-to-back pair of unit lengths is missing: %s" % sorted(want - _pairs(seqs))
    lens = {len(s) for s in seqs}
    assert 0 in lens and 1 in lens and max(lens) >= 3, "workgroups without a unit, with exactly one, and with several: %s" % sorted(lens)
    # a unit whose LAST visit is the zero slab, followed by a unit whose first visit is not
    last_zero = [1 for s in seqs for a, b in zip(s, s[1:]) if c["v"][a[0], S - 1] and int(np.flatnonzero(c["v"][b[0]])[0]) != S - 1]
    assert last_zero, "no unit ends on the all-zero slab ahead of a live one"
    _check(c, "tri, %d slabs, %s" % (S, act), monkeypatch)


def _case_refresh(c):
    """the poisoned dz and the plain references again after dz was edited in place"""
    o, act = c["o"], c["act"]
    staged = np.asarray((o["adj"].T @ c["v"].astype(np.float64)) > 0)
    nan = torch.full((), float("nan"), device="cuda")
    dz_p = torch.where(_rows(~staged, o["row0"])[:, :, None, None], nan, c["dz"])
    dW = [a.clone() for a in c["dW0"]]
    dx = o["op"].backward([c["dz"]], c["W"], c["aux"], act, True, dW)
    dW2, dWf = [a.clone() for a in c["dW0"]], [a.clone() for a in c["dWf0"]]
    assert o["op"].backward_fused_first(c["dz"], c["W"], None, act, c["y"], dW2, dWf, Ws_first=c["Wf"]) is not False
    torch.cuda.synchronize()
    return dict(dz_p=dz_p, dx=dx, dW=dW, dW2=dW2, dWf=dWf)


@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_mixed_blocks_hand_over_between_wide_and_narrow_tall_and_short_empty_and_filled(act, monkeypatch):
    _need_gpu()
    o = _operator("mixed")
    S = 5
    rs = np.random.RandomState(3)
    m = rs.rand(o["nb"], S) < 0.15
    c = _case("mixed", act, S, m, 50 + (act == "relu"))
    seqs = _sequences(o, c["v"], S)
    kind = o["kinds"]
    got = {(int(kind[a[0]]), int(kind[b[0]])) for s in seqs for a, b in zip(s, s[1:])}
    # 0: 64 rows / 128 sources, 1: 2 rows / 2 sources, 2: one row without an entry
    want = {(0, 1), (1, 0), (0, 2), (2, 0), (2, 1), (1, 2), (0, 0)}
    assert want <= got, "a hand-over between block kinds is missing: %s" % sorted(want - got)
    info = o["op"].plan_info()
    assert info[0] == o["nb"]
    _check(c, "mixed, %s" % act, monkeypatch)


def test_three_scans_per_workgroup_with_visits_on_both_sides_of_a_scan_boundary(monkeypatch):
    """131 080 one-row blocks on 256 workgroups: 513 units for the first workgroups of an XCD, 256 per scan, every one visited (one
    slab), so entries 255 | 256 and 511 | 512 of a workgroup's sequence sit on the two sides of a table refill."""
    _need_gpu()
    o = _operator("long")
    S = 1
    m = np.ones((o["nb"], S), bool)
    c = _case("long", "tanh", S, m, 77)
    seqs = _sequences(o, c["v"], S)
    assert max(len(s) for s in seqs) == 513 and min(len(s) for s in seqs) >= 512
    _check(c, "long", monkeypatch)


def test_plan_step_with_the_switch_on_against_off(monkeypatch):
    """Three layers of 32, tanh, 128 trajectories on a complex of ~40 000 edges (several units per workgroup): loss and every weight
    gradient bit for bit; some workgroup of the M2 launch runs two units back to back."""
    _need_gpu()
    from oracle import scone_oracle as so
    from scone_gcn_amd import ops, synthetic_data_gen as g, trajectory_experiments as te
    from scone_gcn_amd.complex import SimplicialComplex
    for name in ("KEEP_LAST_MIN_BYTES", "SMALL_DZ_BYTES", "READOUT_CONE_MIN_BYTES"):
        monkeypatch.setattr(ops.SconePlan, name, 0)
    cx = g.random_SC_graph(g.calibrate_n_points(40000))
    sc = SimplicialComplex(cx)
    shifts, readout, _ = te.setup_from_complex(sc, "scone")
    dev = ops.default_device()
    plan = ops.SconePlan(shifts[0], shifts[1], readout, "tanh", dev)
    N = 128
    paths = g.generate_random_walks(cx, m=N, seed=3)
    flows, choice, last, _, _ = g.path_dataset(cx, paths, seed=4)
    x, _ = ops.flows_to_slabs(flows, sc.layout, dev)
    n_pad = x.shape[0] * ops.NS
    yp = np.zeros((n_pad, sc.max_degree), np.float32)
    yp[:N] = np.asarray(so.onehot_targets(choice, sc.max_degree)).reshape(N, sc.max_degree)
    y_dev, last_dev = torch.as_tensor(yp, device=dev), ops._last_nodes_dev(np.asarray(last), n_pad, dev)
    rs = np.random.RandomState(41)
    w = [torch.tensor(0.3 * rs.randn(*s), dtype=torch.float32, device="cuda") for s in so.weight_shapes(1, [(3, 32)] * 3, 1)]

    def step(on):
        monkeypatch.setattr(ops, "VISIT_PREFETCH", on)
        logp, saved = plan.forward(x, last_dev, w)
        loss = -(logp * y_dev).sum() / N
        grads = [torch.zeros_like(a) for a in w]
        plan.backward(saved, logp, -y_dev / N, last_dev, w, grads)
        torch.cuda.synchronize()
        assert getattr(saved, "cone", None) is not None, "the step did not run on the readout's cone"
        return loss.reshape(1), grads

    on, off = step(True), step(False)
    _same_bits(on[0], off[0], "loss")
    for i, (a, b) in enumerate(zip(on[1], off[1])):
        _same_bits(a, b, "gradient %d" % i)
    assert max(float(a.abs().max()) for a in on[1]) > 0
    tabs = plan.field_tables_dev()
    m2 = plan.conv.keep_mask(last_dev, ops.NS, plan.n_nodes, tabs)
    for _ in range(2):
        m2 = plan.conv.mask_hop(m2, tabs)
    S = x.shape[0]
    gx, gy = _grid(tabs.n_blocks, S)
    lens = [len(s) for r in range(gy) for s in plan.conv.window_scan_probe(m2, S, gx, r * S // gy, (r + 1) * S // gy - r * S // gy)[0]]
    assert max(lens) >= 2, "no workgroup of the M2 launch has a unit with a successor"
