"""GPU tests of the packed block records in the two visiting backwards (csrc/scn_blk_record.h, scn_window_scan.inc, scn_blk_bwd.inc;
ops.VISIT_RECORDS): the window scan leaves the records of its first scn_conv_visit_records_cap() live entries in LDS, a unit's top reads its
header, its tile widths and the next unit's source range from there (an entry past the cap: from one 32-byte load), and every load
of the unit's top goes out under one wait.  Which tiles are computed, their order and their arithmetic do not change, so everything
is compared BIT FOR BIT:

  * the switch on against the switch off (the unit loop as it was), and
  * both against the plain (non-visiting) backward on a dz that is exactly zero outside the rows of a set M with V = hop(M) visited,

in dx, the reduced dW of both forms and dW_first, with aux / y outside V and dz outside what V stages pre-filled with NaN and dx
pre-filled with a sentinel.  The shapes and operators are those of tests/test_gpu_visit_prefetch.py (the smallest at which a unit has
a successor): `tri` at 5 / 33 / 64 slabs with every ordered pair of 1-, 2- and 3-visit units, that file's `mixed` with every hand-over
between its block kinds (all of width <= 4), the `mixed` LIMIT operator of tests/test_host_block_plan_limits.py (width-128 block ->
width <= 4, 64 rows -> <= 2, entry-less -> filled, units on the 32 x 36 ELL-cap block: ELL tiles of one, two and three pieces per
thread), `long` with 513 units per workgroup over three scans -- units past the cap and a table refilled per scan, asserted on
the launch's own sequences (scn_window_scan_probe) -- and one plan step on ~40 000 edges."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_keep_last import _expected, _need_gpu, _same_bits, _sentinel
from tests.test_gpu_visit_prefetch import _case, _case_refresh, _grid, _operator, _pairs, _sequences

pytestmark = pytest.mark.gpu


def _run_visits(c, on, monkeypatch):
    """both visiting forms on the poisoned tensors with the records switch set: (dx, dW, dW of the fused form, dW_first)"""
    from scone_gcn_amd import ops
    monkeypatch.setattr(ops, "VISIT_RECORDS", on)
    op = c["o"]["op"]
    dW = [a.clone() for a in c["dW0"]]
    dx = op.backward([c["dz_p"]], c["W"], c["aux_p"], c["act"], True, dW, dx=_sentinel(c["dz"].shape), visit=c["mask"])
    assert dx is not False, "visiting backward not served"
    dW2, dWf = [a.clone() for a in c["dW0"]], [a.clone() for a in c["dWf0"]]
    assert op.backward_fused_first(c["dz_p"], c["W"], None, c["act"], c["y_p"], dW2, dWf, Ws_first=c["Wf"], visit=c["mask"]) is not False
    torch.cuda.synchronize()
    from scone_gcn_amd import _lib
    assert _lib.load().scn_conv_visit_records(-1) == (1 if on else 0), "the launches did not run with the switch as set"
    return dx, dW, dW2, dWf


def _check(c, what, monkeypatch):
    on, off = _run_visits(c, True, monkeypatch), _run_visits(c, False, monkeypatch)
    want_dx = _expected(c["dx"], c["v"], c["o"]["row0"])
    for tag, got in (("records", on), ("switch off", off)):
        _same_bits(got[0].view(torch.int32), want_dx, "dx on the visited items, sentinel elsewhere (%s), %s" % (tag, what))
        for g in range(3):
            _same_bits(got[1][g], c["dW"][g], "dW[%d] against the plain backward (%s), %s" % (g, tag, what))
            _same_bits(got[2][g], c["dW2"][g], "fused form's dW[%d] against the plain one (%s), %s" % (g, tag, what))
            _same_bits(got[3][g], c["dWf"][g], "dW_first[%d] against the plain fused backward (%s), %s" % (g, tag, what))
    for a, b in zip(on, off):
        for x, z in zip(a, b) if isinstance(a, list) else [(a, b)]:
            _same_bits(x, z, "records against the switch off, " + what)
    assert float(c["dx"].abs().max()) > 0 and max(float((a - b).abs().max()) for a, b in zip(c["dW"], c["dW0"])) > 0, "the case contracts nothing"


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("S", [5, 33, 64])
def test_tridiagonal_units_of_one_two_and_three_visits_in_every_order(S, act, monkeypatch):
    """M: a seeded third of the blocks with 1 .. 3 slabs each; dz of slab S - 1 is all zero (a unit's last visit an early-out)."""
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
    _check(c, "tri, %d slabs, %s" % (S, act), monkeypatch)


@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_mixed_blocks_hand_over_between_wide_and_narrow_tall_and_short_empty_and_filled(act, monkeypatch):
    _need_gpu()
    o = _operator("mixed")
    S = 5
    m = np.random.RandomState(3).rand(o["nb"], S) < 0.15
    c = _case("mixed", act, S, m, 50 + (act == "relu"))
    seqs = _sequences(o, c["v"], S)
    kind = o["kinds"]
    got = {(int(kind[a[0]]), int(kind[b[0]])) for s in seqs for a, b in zip(s, s[1:])}
    # 0: 64 rows / 128 sources (width 4), 1: 2 rows / 2 sources (width 2), 2: one row without an entry
    want = {(0, 1), (1, 0), (0, 2), (2, 0), (2, 1), (1, 2), (0, 0)}
    assert want <= got, "a hand-over between block kinds is missing: %s" % sorted(want - got)
    _check(c, "mixed, %s" % act, monkeypatch)


def _limit_operator():
    """The `mixed` LIMIT operator of tests/test_host_block_plan_limits.py (the ConvOp of tests/test_gpu_block_plan_limits.py) in the form
    _case takes: a one-row block of width 128 on 128 sources, the 32 x 36 ELL-cap block, 64-row blocks, entry-less blocks and the 1 .. 63
    row groups, 70 times over in a seeded shuffle -- blocks whose ELL tile needs the second and third piece of load_block_c32_rec."""
    from tests import test_gpu_block_plan_limits as gl
    from tests import test_gpu_visit_prefetch as vp
    if "limit_mixed" not in vp._OPS:
        e = gl._env("mixed")
        row0 = np.asarray(e["op"].plan_blocks(), np.int64)
        pattern = abs(e["mats"][0]) + abs(e["mats"][1])
        vp._OPS["limit_mixed"] = dict(op=e["op"], row0=row0, adj=vp._block_adjacency(pattern, row0), kinds=None, n=e["n"], nb=len(row0) - 1,
                                      cut=e["cut"])
    return vp._OPS["limit_mixed"]


@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_limit_operator_hands_over_from_width_128_from_64_rows_and_from_an_entry_less_block(act, monkeypatch):
    """Units on the block plan's limits, each hand-over asserted on the launch's own sequences: a width-128 block -> a block of width
    <= 4, a 64-row block -> one of <= 2 rows, an entry-less block -> a filled one; a unit on the ELL-cap block (32 x 36 = 1152 entries:
    all three ELL pieces of a thread carry elements) with a successor and one as a successor."""
    _need_gpu()
    o = _limit_operator()
    S = 3
    m = np.random.RandomState(5).rand(o["nb"], S) < 0.5
    c = _case("limit_mixed", act, S, m, 90 + (act == "relu"))
    seqs = _sequences(o, c["v"], S)
    cut = o["cut"]                                                # (row0, rows, sources, width, reason) per block
    pairs = [(cut[a[0]], cut[b[0]]) for s in seqs for a, b in zip(s, s[1:])]
    assert any(a[3] == 128 and b[3] <= 4 for a, b in pairs), "no width-128 unit ahead of one of width <= 4"
    assert any(a[1] == 64 and b[1] <= 2 for a, b in pairs), "no 64-row unit ahead of one of <= 2 rows"
    assert any(a[3] == 0 and b[3] > 0 for a, b in pairs), "no entry-less unit ahead of a filled one"
    assert any(a[1] * a[3] == 1152 for a, b in pairs) and any(b[1] * b[3] == 1152 for a, b in pairs), "no unit on the ELL-cap block"
    assert any(1024 < a[1] * a[3] < 1152 for a, b in pairs), "no unit whose ELL tile ends inside a thread's third piece (11 rows x 100)"
    assert any(a[1] * a[3] == 512 for a, b in pairs), "no unit whose ELL tile is exactly a thread's first piece (64 rows x 8)"
    _check(c, "limit operator mixed, %s" % act, monkeypatch)


def test_units_past_the_cap_and_a_table_refilled_per_scan(monkeypatch):
    """131 080 one-row blocks on 256 workgroups, every one visited: 256 live entries per scan, so entries CAP .. 255 of every scan take
    the one-load fallback, entry CAP - 1 reads its successor's record from global memory, and the table is refilled for the second and
    the third scan (whose single entry has no successor)."""
    _need_gpu()
    from scone_gcn_amd import _lib
    o = _operator("long")
    S = 1
    c = _case("long", "tanh", S, np.ones((o["nb"], S), bool), 77)
    seqs = _sequences(o, c["v"], S)
    cap = _lib.load().scn_conv_visit_records_cap()           # the library's own figure
    assert max(len(s) for s in seqs) == 513 and min(len(s) for s in seqs) >= 512
    assert all(len(s) > 256 + cap for s in seqs) and 0 < cap < 256, "every workgroup: entries on both sides of the cap, in two full scans"
    _check(c, "long", monkeypatch)


def test_plan_step_with_the_switch_on_against_off(monkeypatch):
    """Three layers of 32, tanh, 128 trajectories on a complex of ~40 000 edges: loss and every weight gradient bit for bit."""
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
        monkeypatch.setattr(ops, "VISIT_RECORDS", on)
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
