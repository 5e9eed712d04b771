"""GPU tests of the LDS-blocked kernels on hand-built operators AT THE LIMITS OF THE BLOCK PLAN.

Every other small-shape kernel test runs on triangulated complexes, whose blocks all look alike (about 64 rows, 11 entries per row,
130 staged rows).  The operators here (tests/test_host_block_plan_limits.py builds them and proves on the CPU what each of their
blocks is) are made of hinted row groups that each meet one limit of the plan: a 64-row block, a ONE-ROW block with 128 sources and
an ELL width of 128, a block cut exactly at the ELL cap (32 x 36 = 1152) and its 8-row rest, an 11-row block whose quad {1, 2, 4, 7}
has the widths 0 / 1 / 100 / 2, a block without entries (identity reads only), blocks of 1 / 2 / 7 / 8 / 9 / 63 rows (the edges of a
wave's eight rows and of the last wave), rows whose entries feed the second operator only, and an unhinted tail that the greedy cut
closes on the source cap.

  small     every group once (373 rows, 16 blocks: one block per workgroup)
  mixed     the groups 70 times over in a seeded shuffled order (15 760 rows, 913 blocks): every grid the launch can pick has workgroups
            that walk several blocks, and on the 256-workgroup grid of the MFMA kernels some workgroup goes, back to back, from the
            width-128 block to one of width <= 4, from a 64-row block to one of <= 2 rows, and from the entry-less block to one with
            entries (asserted on the launch's own unit table), so ELL tile, source list and staging buffers still hold the earlier
            block's data
  unhinted  small without hints (another cut: rows / sources / ELL only)
  nonsym    small with a third of the entries below the diagonal dropped; nonsym_T, its transpose, is the backward's operator
  power     identity + one value array (forward_power / backward_power);   rect: one value array over n / 2 columns, no identity
  noplan    small plus a row of 128 off-diagonal entries = 129 sources: NO plan, the generic kernels of scn_conv.hip serve it

Each kernel runs against an fp64 scipy CSR evaluation of the same formula on the same dense randn slabs, every row of every block
compared.  Bars: outputs, dx, y and the SpMM REL_TERMS = 4e-6 of each output's own sum of |terms| (tests/test_gpu_fullsize_dense.py),
weight gradients 8e-6 of each entry's own sum of |terms| over all points; the buffer the gradient is
accumulated into starts from 0.25, which is one more term.  A missing or doubled entry, a wrong pad slot or a stale tile moves an
output by a whole term, orders of magnitude above either bar.  The plan's row0 list is compared with the restated cut first, so a
wrong cut is reported as such and not as a numeric error.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import test_host_block_plan_limits as hb
from tests.test_gpu_fullsize_dense import REL_TERMS, _assert_close, _layer_reference, _t
from tests.test_gpu_nonfinite import ACTS, _shift
from tests.test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu

REL_DW_TERMS = 8e-6
FILL = 0.25
DACT = {"tanh": lambda a: 1.0 - a ** 2, "relu": lambda a: (a > 0).astype(np.float64)}      # act' through the OUTPUT value

_ENV = {}


def _env(name):
    """dict(op: ConvOp, mats: the value arrays as fp64 CSR, n, n_cols, cut: the restated blocks or None)."""
    _need_gpu()
    if name not in _ENV:
        from scone_gcn_amd import ops
        o = hb.operator(name)
        mats = hb.matrices(o)
        op = ops.ConvOp(o["n"], [{"mats": mats, "identity": o["identity"], "n_cols": o["n_cols"]}], block_start=o["hint"])
        cut = hb.cut_of(name)
        if cut is None:
            assert op.plan_info()[0] == 0, "an operator with a row that fits no block has no plan"
        else:
            assert op.plan_blocks().tolist() == [b[0] for b in cut] + [o["n"]], "%s: the plan's cut is not the restated one" % name
        _ENV[name] = dict(op=op, mats=[m.astype(np.float64) for m in mats], n=o["n"], n_cols=o["n_cols"], cut=cut)
    return _ENV[name]


def _randn(rs, *shape):
    return rs.randn(*shape).astype(np.float32)


def _weights(rs, c_in, c_out, scale=0.1):
    return [(scale * rs.randn(c_in, c_out)).astype(np.float32) for _ in range(3)]


def _terms(mats, x):
    """[x, A0 x, A1 x] and the same of |.| in fp64 for slabs x [S, cols, ns, C]"""
    x = x.astype(np.float64)
    return [x] + [_shift(m, x) for m in mats], [np.abs(x)] + [_shift(abs(m), np.abs(x)) for m in mats]


def _fwd_ref(gk, ga, W):
    Wd = [w.astype(np.float64) for w in W]
    return sum(g @ w for g, w in zip(gk, Wd)), sum(g @ np.abs(w) for g, w in zip(ga, Wd))


def _bwd_ref(gk, ga, W, aux, act):
    """dx = (sum_k g_k W_k^T) act'(aux), dW_k = aux^T g_k, with their sums of |terms|"""
    a = aux.astype(np.float64)
    Wd = [w.astype(np.float64) for w in W]
    dx = sum(g @ w.T for g, w in zip(gk, Wd)) * DACT[act](a)
    sdx = sum(g @ np.abs(w).T for g, w in zip(ga, Wd))
    A = a.reshape(-1, a.shape[-1])
    dW = [A.T @ g.reshape(-1, g.shape[-1]) for g in gk]
    sdW = [np.abs(A).T @ g.reshape(-1, g.shape[-1]) for g in ga]
    return dx, sdx, dW, sdW


def _close(got, ref, scale, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == ref.shape, what
    print("%s: worst %.3g of its terms' sum (bar %.1e)" % (what, float((np.abs(got - ref) / np.maximum(scale, 1e-3)).max()), REL_TERMS))
    _assert_close(got, ref, scale, what)


def _close_dw(got, ref, scale, what):
    """weight gradients accumulated into a buffer that held FILL"""
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, what
    err = np.abs(got - FILL - ref) / (scale + FILL)
    print("%s: worst %.3g of its terms' sum (bar %.1e)" % (what, float(err.max()), REL_DW_TERMS))
    assert (err <= REL_DW_TERMS).all(), "%s: %d entries off, worst %.3e of its terms' sum" % (what, int((err > REL_DW_TERMS).sum()), float(err.max()))
    assert float(np.abs(ref).max()) > 0.1, what + ": reference is trivially small"


def _fill(*shape):
    return torch.full(shape, FILL, device="cuda")


def _dz(rs, S, n, C):
    """dense randn with ONE all-zero slab among non-zero ones (S >= 2): the zero-tile early-out and the running dW exponent"""
    dz = _randn(rs, S, n, 4, C)
    if S >= 2:
        dz[S // 2] = 0.0
    return dz


def _aux(rs, act, *shape):
    a = _randn(rs, *shape)
    return np.tanh(a).astype(np.float32) if act == "tanh" else a


def _launch_grid(nb, n_slabs, per_cu):
    """The library's choice of (grid.x, grid.y) for a blocked launch (launch_grid, scn_blk_dispatch.inc), restated; per_cu: the
    workgroups per CU the kernel's LDS footprint allows (1, 2 or 3)."""
    cap, nb_xcd, best = 256 * per_cu, (nb + 7) // 8, None
    gy = 1
    while gy <= 32 and gy <= max(1, n_slabs):
        gx = max(8, min(cap // gy, (nb + 7) // 8 * 8) // 8 * 8)
        cost = ((nb_xcd + gx // 8 - 1) // (gx // 8)) * (2 * ((n_slabs + gy - 1) // gy) + 1) * 64 + gy
        if best is None or cost < best[0]:
            best = (cost, gx, gy)
        gy *= 2
    return best[1], best[2]


def _units(nb, gx, g):
    """the units (positions of the unit -> block table) of workgroup g, in visiting order"""
    xcd, j, stride = g & 7, g >> 3, gx >> 3
    return list(range(nb * xcd // 8 + j, nb * (xcd + 1) // 8, stride))


FWD_OPS = ["small", "unhinted", "nonsym"]
BWD_OPS = ["small", "unhinted", "nonsym_T"]

# ------------------------------------------------------------------------------------------------------------------
# the plans and the walk
# ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", hb.WITH_PLAN + ["mixed_power", "noplan"])
def test_plan_blocks_are_the_restated_cut(name):
    e = _env(name)
    if name != "noplan":
        assert e["op"].plan_info()[0] == len(e["cut"]) > 0


def test_small_gives_every_workgroup_one_block_and_splits_32_slabs():
    nb = len(_env("small")["cut"])
    for per_cu in (1, 2, 3):
        for S in (1, 2, 3, 5):
            assert _launch_grid(nb, S, per_cu)[0] >= nb
        assert _launch_grid(nb, 32, per_cu)[1] in (16, 32)


def test_mixed_workgroups_walk_from_wide_to_narrow_from_tall_to_short_and_from_empty_to_filled():
    """On the launch's own unit -> block table (window_scan_probe on an empty mask).  The MFMA kernels and the K = 128 ring SpMM run
    one workgroup per CU: 256 workgroups, three to four blocks each -- all three transitions.  The 512- and 768-workgroup grids
    (K = 64 ring SpMM, the y-only gather; the one-channel forward) have one or two blocks per workgroup."""
    e = _env("mixed")
    op, cut = e["op"], e["cut"]
    nb = len(cut)
    assert nb > 768
    for S in (1, 3):                                                     # the slab counts of the mixed cases below: no slab split
        assert [_launch_grid(nb, S, p) for p in (1, 2, 3)] == [(256, 1), (512, 1), (768, 1)]
    found = {}
    for gx in (256, 512, 768):
        _, ub = op.window_scan_probe(torch.zeros((nb, 1), device="cuda", dtype=torch.int32), 1, gx, 0, 1)
        assert sorted(ub.tolist()) == list(range(nb))
        t = dict(wide_narrow=0, tall_short=0, empty_filled=0, several=0)
        for g in range(gx):
            blocks = [cut[ub[u]] for u in _units(nb, gx, g)]
            t["several"] += len(blocks) >= 2
            for a, b in zip(blocks, blocks[1:]):
                t["wide_narrow"] += a[3] == 128 and b[3] <= 4
                t["tall_short"] += a[1] == 64 and b[1] <= 2
                t["empty_filled"] += a[3] == 0 and b[3] > 0
        found[gx] = t
    print(found)
    assert all(found[gx]["several"] > 0 for gx in found)
    assert found[256]["wide_narrow"] and found[256]["tall_short"] and found[256]["empty_filled"]
    assert found[512]["wide_narrow"] and found[768]["wide_narrow"]


# ------------------------------------------------------------------------------------------------------------------
# SpMM
# ------------------------------------------------------------------------------------------------------------------

def _spmm_case(name, K, S, seed):
    e = _env(name)
    rs = np.random.RandomState(seed)
    x = _randn(rs, S, e["n_cols"], K)
    dual = len(e["mats"]) == 2
    ya, yb = e["op"].spmm_dual(_t(x), dual=dual)
    ya1, none = e["op"].spmm_dual(_t(x), dual=False)
    assert none is None
    for s in range(S):
        xs = x[s].astype(np.float64)
        _close(ya1[s], e["mats"][0] @ xs, abs(e["mats"][0]) @ np.abs(xs), "%s single K=%d slab %d/%d" % (name, K, s, S))
        if dual:
            _close(ya[s], e["mats"][0] @ xs, abs(e["mats"][0]) @ np.abs(xs), "%s dual a K=%d slab %d/%d" % (name, K, s, S))
            _close(yb[s], e["mats"][1] @ xs, abs(e["mats"][1]) @ np.abs(xs), "%s dual b K=%d slab %d/%d" % (name, K, s, S))


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("K", [128, 64, 100, 4])
def test_spmm_dual_and_single(K, S):
    """K = 128 / 64: the ring kernel, 100: the two-buffer one, 4: slabs folded into one staged piece.  rect: blocks that stage nothing."""
    for name in FWD_OPS + ["nonsym_T", "power", "rect"]:
        _spmm_case(name, K, S, 10 * K + S)


@pytest.mark.parametrize("K,S", [(128, 1), (64, 3), (100, 1)])
def test_spmm_on_mixed(K, S):
    _spmm_case("mixed", K, S, K)


# ------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------

def _forward_case(name, C, S, acts, seed, partial=False):
    e = _env(name)
    rs = np.random.RandomState(seed)
    x, W = _randn(rs, S, e["n"], 4, C), _weights(rs, C, C)
    z, scale, _ = _layer_reference(e["mats"][0], e["mats"][1], x, W)
    part = _randn(rs, S, e["n"], 4, C) if partial else None
    for act in acts:
        what = "%s forward C=%d S=%d %s%s" % (name, C, S, act, " + partial" if partial else "")
        if partial:
            out = e["op"].forward([_t(x)], [_t(w) for w in W], C, act, partial=_t(part))
            _close(out, ACTS[act](z + part), scale + np.abs(part), what)
        else:
            _close(e["op"].forward([_t(x)], [_t(w) for w in W], C, act), ACTS[act](z), scale, what)


@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("C", [32, 16])
@pytest.mark.parametrize("name", FWD_OPS)
def test_forward(name, C, S):
    """fwd_c32_w16_kernel / fwd_c16_w16_kernel (slab pairs; S odd: the pair form's tail)"""
    _forward_case(name, C, S, ("tanh", "relu"), 100 + C + S)


@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("name", FWD_OPS)
def test_forward_accumulate(name, S):
    _forward_case(name, 32, S, ("tanh", "relu"), 200 + S, partial=True)


@pytest.mark.parametrize("C,S,partial", [(32, 3, False), (16, 3, False), (32, 1, True)])
def test_forward_on_mixed(C, S, partial):
    _forward_case("mixed", C, S, ("tanh", "relu") if C == 32 and not partial else ("tanh",), 300 + C, partial)


def _first_case(name, S, seed, acts=("tanh", "relu")):
    """forward_first 1 -> 32 and 1 -> 16 with y, shifted_input, and forward_from_y on the device's own H1 (held to fp64 here first)"""
    e = _env(name)
    op = e["op"]
    rs = np.random.RandomState(seed)
    x = _randn(rs, S, e["n"], 4, 1)
    gk, ga = _terms(e["mats"], x)
    yref, yscale = np.concatenate(gk, axis=3), np.concatenate(ga, axis=3)
    y2 = op.shifted_input(_t(x))
    assert y2 is not None, "y-only launch not served"
    _close(y2[..., :3], yref, yscale, "%s shifted_input S=%d" % (name, S))
    assert not bool(y2[..., 3].any())
    for C in (32, 16):
        Wf = _weights(rs, 1, C, 0.5)
        z, scale = _fwd_ref(gk, ga, Wf)
        for act in acts:
            res = op.forward_first(_t(x), [_t(w) for w in Wf], C, act)
            assert res is not None, "first layer not served"
            H1, y = res
            _close(H1, ACTS[act](z), scale, "%s forward_first c_out=%d S=%d %s" % (name, C, S, act))
            assert torch.equal(y, y2), "y of forward_first and of the y-only launch"
            if C == 32:
                W = _weights(rs, 32, 32)
                out = op.forward_from_y(y, [_t(w) for w in Wf], [_t(w) for w in W], act)
                assert out is not None, "from-y forward not served"
                z2, s2, _ = _layer_reference(e["mats"][0], e["mats"][1], H1.cpu().numpy(), W)
                _close(out, ACTS[act](z2), s2, "%s forward_from_y S=%d %s" % (name, S, act))


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("name", FWD_OPS)
def test_first_layer_and_from_y(name, S):
    """fwd_c1_kernel, gather3_c1_kernel and the from-y forward"""
    _first_case(name, S, 400 + S)


def test_first_layer_and_from_y_on_mixed():
    _first_case("mixed", 1, 401, acts=("tanh",))


# ------------------------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------------------------

def _backward_case(name, C, S, acts, seed, forms=("dx", "dw_only", "partial")):
    e = _env(name)
    op = e["op"]
    rs = np.random.RandomState(seed)
    dz, W = _dz(rs, S, e["n"], C), _weights(rs, C, C)
    gk, ga = _terms(e["mats"], dz)
    for act in acts:
        aux = _aux(rs, act, S, e["n"], 4, C)
        rdx, sdx, rdW, sdW = _bwd_ref(gk, ga, W, aux, act)
        for form in forms:
            if form == "partial" and C != 32:
                continue
            what = "%s backward C=%d S=%d %s %s" % (name, C, S, act, form)
            dWs = [_fill(C, C) for _ in range(3)]
            if form == "partial":
                dxp = _randn(rs, S, e["n"], 4, C)
                dx = op.backward([_t(dz)], [_t(w) for w in W], _t(aux), act, True, dWs, dx_partial=_t(dxp))
                _close(dx, rdx + dxp, sdx + np.abs(dxp), what + " dx")
            else:
                dx = op.backward([_t(dz)], [_t(w) for w in W], _t(aux), act, form == "dx", dWs)
                if form == "dx":
                    _close(dx, rdx, sdx, what + " dx")
                else:
                    assert dx is None
            for k in range(3):
                _close_dw(dWs[k], rdW[k], sdW[k], what + " dW%d" % k)


@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("C", [32, 16])
@pytest.mark.parametrize("name", BWD_OPS)
def test_backward(name, C, S):
    """bwd_c32_bf16_kernel plain (need_dx on and off), PAIR (16 channels) and ACCUM (dx_partial=)"""
    _backward_case(name, C, S, ("tanh", "relu"), 500 + C + S)


@pytest.mark.parametrize("C,S,forms", [(32, 3, ("dx",)), (16, 3, ("dx",)), (32, 1, ("dw_only", "partial"))])
def test_backward_on_mixed(C, S, forms):
    _backward_case("mixed", C, S, ("tanh",), 600 + C + S, forms)


def test_forward_and_backward_on_small_at_32_slabs():
    """the restated grid splits the slabs 16 or 32 ways (asserted above): one or two slabs per workgroup"""
    _forward_case("small", 32, 32, ("tanh",), 700)
    _backward_case("small", 32, 32, ("tanh",), 701, ("dx",))


def _first_ref(y, rdx, sdx):
    """dW_first[g][c] = sum_p y[p][g] dx[p][c]"""
    Y = y.astype(np.float64)[..., :3].reshape(-1, 3)
    return Y.T @ rdx.reshape(-1, rdx.shape[-1]), np.abs(Y).T @ sdx.reshape(-1, sdx.shape[-1])


def _fused_first_case(name, fwd_name, S, seed, acts=("tanh", "relu")):
    """backward_fused_first with aux (32 and 16 channels) and from y (32, Ws_first); the from-y form takes y and H1 from the FORWARD
    operator's first layer, as a training step does"""
    e = _env(name)
    op = e["op"]
    rs = np.random.RandomState(seed)
    for C in (32, 16):
        dz, W = _dz(rs, S, e["n"], C), _weights(rs, C, C)
        gk, ga = _terms(e["mats"], dz)
        y = _randn(rs, S, e["n"], 4, 4)
        y[..., 3] = 0.0
        for act in acts:
            aux = _aux(rs, act, S, e["n"], 4, C)
            dWs, dWf = [_fill(C, C) for _ in range(3)], [_fill(1, C) for _ in range(3)]
            assert op.backward_fused_first(_t(dz), [_t(w) for w in W], _t(aux), act, _t(y), dWs, dWf), "not served"
            rdx, sdx, rdW, sdW = _bwd_ref(gk, ga, W, aux, act)
            rf, sf = _first_ref(y, rdx, sdx)
            what = "%s backward_fused_first C=%d S=%d %s" % (name, C, S, act)
            for k in range(3):
                _close_dw(dWs[k], rdW[k], sdW[k], what + " dW%d" % k)
                _close_dw(dWf[k], rf[k][None], sf[k][None], what + " dW_first%d" % k)
            if C != 32:
                continue
            Wf = _weights(rs, 1, 32, 0.5)
            H1, yd = _env(fwd_name)["op"].forward_first(_t(_randn(rs, S, e["n"], 4, 1)), [_t(w) for w in Wf], 32, act)
            dWs, dWf = [_fill(C, C) for _ in range(3)], [_fill(1, C) for _ in range(3)]
            assert op.backward_fused_first(_t(dz), [_t(w) for w in W], None, act, yd, dWs, dWf, Ws_first=[_t(w) for w in Wf]), "not served"
            rdx, sdx, rdW, sdW = _bwd_ref(gk, ga, W, H1.cpu().numpy(), act)
            rf, sf = _first_ref(yd.cpu().numpy(), rdx, sdx)
            for k in range(3):
                _close_dw(dWs[k], rdW[k], sdW[k], what + " from y dW%d" % k)
                _close_dw(dWf[k], rf[k][None], sf[k][None], what + " from y dW_first%d" % k)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("name,fwd_name", [("small", "small"), ("unhinted", "unhinted"), ("nonsym_T", "nonsym")])
def test_backward_fused_first(name, fwd_name, S):
    """bwd_c32_bf16_kernel FIRST, its pair form and the from-y form"""
    _fused_first_case(name, fwd_name, S, 800 + S)


def test_backward_fused_first_on_mixed():
    _fused_first_case("mixed", "mixed", 3, 803, acts=("tanh",))


def _dw_first_case(name, S, seed):
    e = _env(name)
    op = e["op"]
    rs = np.random.RandomState(seed)
    x = _randn(rs, S, e["n"], 4, 1)
    gk, ga = _terms(e["mats"], x)
    yref, yabs = np.concatenate(gk, axis=3).reshape(-1, 3), np.concatenate(ga, axis=3).reshape(-1, 3)
    y = op.shifted_input(_t(x))
    for C in (32, 16):
        dz = _dz(rs, S, e["n"], C)
        D = dz.astype(np.float64).reshape(-1, C)
        ref, scale = yref.T @ D, yabs.T @ np.abs(D)
        assert op.dw_first_served(_t(dz))
        for yy in (None, y):
            dWs = [_fill(1, C) for _ in range(3)]
            assert op.dw_first(_t(x), yy, _t(dz), dWs)
            for k in range(3):
                _close_dw(dWs[k], ref[k][None], scale[k][None], "%s dw_first C=%d S=%d%s dW%d" % (name, C, S, "" if yy is None else " from y", k))


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("name", FWD_OPS)
def test_dw_first(name, S):
    _dw_first_case(name, S, 900 + S)


def test_dw_first_on_mixed():
    _dw_first_case("mixed", 1, 901)


# ------------------------------------------------------------------------------------------------------------------
# power forms: identity + one value array
# ------------------------------------------------------------------------------------------------------------------

def _power_case(name, C, S, seed, acts=("tanh", "relu")):
    """out = act(x0 W0 + x W1 + (A x) W2); backward with dz := x0, g1 := x: dx = (dz W0^T + g1 W1^T + (A g1) W2^T) act'(aux),
    dW = aux^T [dz, g1, A g1]"""
    e = _env(name)
    op, A = e["op"], e["mats"][0]
    rs = np.random.RandomState(seed)
    x0, x, W = _dz(rs, S, e["n"], C), _randn(rs, S, e["n"], 4, C), _weights(rs, C, C)
    a0, a1 = x0.astype(np.float64), x.astype(np.float64)
    gk = [a0, a1, _shift(A, a1)]
    ga = [np.abs(a0), np.abs(a1), _shift(abs(A), np.abs(a1))]
    z, scale = _fwd_ref(gk, ga, W)
    for act in acts:
        what = "%s power C=%d S=%d %s" % (name, C, S, act)
        out = op.forward_power(_t(x0), _t(x), [_t(w) for w in W], act)
        assert out is not None, "power forward not served"
        _close(out, ACTS[act](z), scale, what + " forward")
        aux = _aux(rs, act, S, e["n"], 4, C)
        dWs = [_fill(C, C) for _ in range(3)]
        served, dx = op.backward_power(_t(x0), _t(x), [_t(w) for w in W], _t(aux), act, True, dWs)
        assert served, "power backward not served"
        rdx, sdx, rdW, sdW = _bwd_ref(gk, ga, W, aux, act)
        _close(dx, rdx, sdx, what + " dx")
        for k in range(3):
            _close_dw(dWs[k], rdW[k], sdW[k], what + " dW%d" % k)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("C", [32, 16])
def test_power_forward_and_backward(C, S):
    _power_case("power", C, S, 1000 + C + S)


def test_power_forward_and_backward_on_mixed():
    _power_case("mixed_power", 32, 3, 1001, acts=("tanh",))


# ------------------------------------------------------------------------------------------------------------------
# no plan: the generic kernels, or "not served" -- never a wrong number
# ------------------------------------------------------------------------------------------------------------------

def test_operator_without_a_plan_runs_the_generic_kernels_or_is_not_served():
    """forward / backward (32 and 16 channels): served by the generic kernels of scn_conv.hip, held to the same bars.
    forward_first / shifted_input: None ("not served": these entry points exist on a blocked plan only, and the caller falls back to
    forward).  forward_from_y: None; backward_fused_first and dw_first: False.  spmm_dual: status SCN_OK (0) -- its contract has no
    "not served" for a shape the generic SpMM takes -- with the right product from spmm_dual_generic."""
    e = _env("noplan")
    op = e["op"]
    assert e["cut"] is None and op.plan_info()[0] == 0
    S = 2
    for C in (32, 16):
        _forward_case("noplan", C, S, ("tanh",), 1100 + C)
        _backward_case("noplan", C, S, ("tanh",), 1200 + C, ("dx", "dw_only"))
    rs = np.random.RandomState(12)
    x1 = _t(_randn(rs, S, e["n"], 4, 1))
    Wf, W = [_t(w) for w in _weights(rs, 1, 32, 0.5)], [_t(w) for w in _weights(rs, 32, 32)]
    assert op.forward_first(x1, Wf, 32, "tanh") is None
    assert op.shifted_input(x1) is None
    y = torch.zeros(S, e["n"], 4, 4, device="cuda")
    assert op.forward_from_y(y, Wf, W, "tanh") is None
    dz = _t(_randn(rs, S, e["n"], 4, 32))
    dWs, dWf = [_fill(32, 32) for _ in range(3)], [_fill(1, 32) for _ in range(3)]
    assert op.backward_fused_first(dz, W, dz, "tanh", y, dWs, dWf) is False
    assert op.dw_first_served(dz) is False and op.dw_first(x1, None, dz, dWf) is False
    assert all(bool((t == FILL).all()) for t in dWs + dWf), "a call that is not served leaves the gradients alone"
    # the generic first layer through forward, against the same reference
    gk, ga = _terms(e["mats"], x1.cpu().numpy())
    z, scale = _fwd_ref(gk, ga, [w.cpu().numpy() for w in Wf])
    _close(op.forward([x1], Wf, 32, "tanh"), np.tanh(z), scale, "noplan forward 1 -> 32")
    for K in (128, 100):
        x = _randn(rs, S, e["n"], K)
        ya, yb = op.spmm_dual(_t(x))                                     # (raises on any status but SCN_OK)
        for s in range(S):
            _close(ya[s], e["mats"][0] @ x[s].astype(np.float64), abs(e["mats"][0]) @ np.abs(x[s].astype(np.float64)), "noplan spmm a K=%d" % K)
            _close(yb[s], e["mats"][1] @ x[s].astype(np.float64), abs(e["mats"][1]) @ np.abs(x[s].astype(np.float64)), "noplan spmm b K=%d" % K)
