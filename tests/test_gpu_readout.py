"""csrc/scn_readout.hip through its C-ABI, against the fp64 restatement at the same layout (oracle/scone_oracle.py slab_readout_*,
pinned on the CPU by tests/test_host_readout.py): the readout forward and backward on the fast item-list, serial and wide forms
and their boundaries, every dz_is_zero mode, scn_readout_clear_dz, the node readout, scn_logits_sum_log_softmax and
scn_masked_ce / _begin.  Tables are built from edge lists, not through complex.py.  Each output is held to a bar relative to
the sum of |terms| it is made of; the worst ratio is in the assert message.  Last, one SconePlan large enough for the pooled
readout-gradient buffer runs two batches back to back that end at different nodes."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import scone_oracle as so
from tests.test_host_readout import COMPLEXES, random_H

pytestmark = pytest.mark.gpu

C_LIST = [1, 3, 8, 16, 32, 40, 64, 96]
REL = 4e-6
SENTINEL = np.uint32(0x7FC0BEEF)               # a quiet NaN with a payload: "never written"
SCN_ERR_BAD_SHAPE, SCN_ERR_UNSUPPORTED = -2, -4


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from scone_gcn_amd import _lib
    return _lib.load()


def _t(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))
    return torch.from_numpy(a).cuda()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    from scone_gcn_amd import ops
    return ops._stream()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _filled(shape, kind, rs):
    if kind == "sentinel":
        return _t(np.full(shape, SENTINEL, np.uint32).view(np.int32)).view(torch.float32)
    return _t((rs.randn(*shape) * 1e3).astype(np.float32))                           # garbage


def _worst(got, ref, bar, rel=REL):
    """max |got - ref| / (rel * bar); an entry with bar 0 must be exact."""
    got, ref, bar = (np.asarray(x, np.float64) for x in (got, ref, bar))
    err = np.abs(got - ref)
    r = np.where(bar > 0, err / np.where(bar > 0, rel * bar, 1.0), np.where(err > 0, np.inf, 0.0))
    r[~np.isfinite(got)] = np.inf
    return float(r.max()) if r.size else 0.0


def _check(what, got, ref, bar, rel=REL):
    w = _worst(got, ref, bar, rel)
    assert w <= 1.0, "%s: worst |err| / (%g x sum|terms|) = %.3g" % (what, rel, w)


_TABLES = {}


def _tables(name):
    if name not in _TABLES:
        cx = COMPLEXES[name]()
        dev = {k: _t(cx[k], np.int32) for k in ("nbr", "last", "inc_ptr", "inc_edge", "edge_nodes")}
        dev["inc_sign"] = _t(cx["inc_sign"], np.float32)
        _TABLES[name] = (cx, dev)
    return _TABLES[name]


def _fwd(lib, cx, dv, H, w, c):
    S, ns, D = cx["S"], cx["ns"], cx["D"]
    N = S * ns
    bh = torch.empty((N, D, c), device="cuda")
    logits = torch.empty((N, D), device="cuda")
    logp = torch.empty((N, D), device="cuda")
    st = lib.scn_readout_forward(S, ns, len(cx["edges"]), c, _p(H), _p(w), _p(dv["nbr"]), cx["n_nodes"], D, _p(dv["last"]),
                                 _p(dv["inc_ptr"]), _p(dv["inc_edge"]), _p(dv["inc_sign"]), _p(bh), _p(logits), _p(logp), _stream())
    assert st == 0
    torch.cuda.synchronize()
    return bh, logits, logp


def _bwd(lib, cx, dv, H, w, bh, d_logp, logp, act, dz, mode, d_w):
    S, ns, D = cx["S"], cx["ns"], cx["D"]
    d_logits = torch.empty((S * ns, D), device="cuda")
    st = lib.scn_readout_backward(S, ns, len(cx["edges"]), H.shape[-1], _p(H), _p(w), _p(dv["nbr"]), cx["n_nodes"], D,
                                  _p(dv["last"]), _p(dv["inc_ptr"]), _p(dv["inc_edge"]), _p(dv["inc_sign"]), _p(dv["edge_nodes"]),
                                  _p(bh), _p(d_logp), _p(logp), act, _p(d_logits), _p(dz), mode, _p(d_w), _stream())
    assert st == 0
    torch.cuda.synchronize()
    return d_logits


def _clear(lib, cx, dv, c, dz):
    S, ns = cx["S"], cx["ns"]
    st = lib.scn_readout_clear_dz(S, ns, len(cx["edges"]), c, _p(dv["nbr"]), cx["n_nodes"], cx["D"], _p(dv["last"]),
                                  _p(dv["inc_ptr"]), _p(dv["inc_edge"]), _p(dv["edge_nodes"]), _p(dz), _stream())
    assert st == 0
    torch.cuda.synchronize()


def _d_logp(rs, cx):
    g = rs.randn(cx["S"] * cx["ns"], cx["D"])
    g[cx["n_real"]:] = 0.0                                                             # padding trajectories carry no loss
    return g.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------
# scn_readout_forward / _backward / _clear_dz
# ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("c", C_LIST)
@pytest.mark.parametrize("name", sorted(COMPLEXES))
def test_readout_matches_fp64_on_every_path(lib, name, c):
    cx, dv = _tables(name)
    rs = np.random.RandomState(100 * sorted(COMPLEXES).index(name) + c)
    S, ns, E, D = cx["S"], cx["ns"], len(cx["edges"]), cx["D"]
    tab = (cx["nbr"], cx["last"], cx["inc_ptr"], cx["inc_edge"], cx["inc_sign"])
    H = random_H(rs, S, E, ns, c)
    w = (rs.randn(c) / math.sqrt(c)).astype(np.float32)
    Hd, wd = _t(H), _t(w)
    tag = "%s c=%d" % (name, c)

    # forward
    ref = so.slab_readout_forward(H, w, *tab)
    bh, logits, logp = _fwd(lib, cx, dv, Hd, wd, c)
    _check(tag + " bh", bh.cpu().numpy(), ref["bh"], ref["bh_abs"])
    _check(tag + " logits", logits.cpu().numpy(), ref["logits"], ref["logits_abs"])
    _check(tag + " logp", logp.cpu().numpy(), ref["logp"], ref["logp_abs"])
    again = _fwd(lib, cx, dv, Hd, wd, c)
    for a, b in zip((bh, logits, logp), again):
        assert np.array_equal(_bits(a), _bits(b)), tag + ": two forward launches differ"

    # backward: inputs fixed in fp32, independent of the forward launch
    g = _d_logp(rs, cx)
    logp_in = ref["logp"].astype(np.float32)
    bh_in = ref["bh"].astype(np.float32)
    gd, lpd, bhd = _t(g), _t(logp_in), _t(bh_in)
    w0 = rs.randn(c).astype(np.float32)
    for act in range(4):
        r = so.slab_readout_backward(H, w, *tab, bh_in, g, logp_in, act)
        sup = np.broadcast_to(r["support"][..., None], (S, E, ns, c))
        for mode, fill in ((0, "garbage"), (1, "sentinel"), (2, "garbage")):
            t = "%s act=%d dz_is_zero=%d" % (tag, act, mode)
            dz = _filled((S, E, ns, c), fill, rs)
            d_w = _t(w0)
            dl = _bwd(lib, cx, dv, Hd, wd, bhd, gd, lpd, act, dz, mode, d_w)
            _check(t + " d_logits", dl.cpu().numpy(), r["d_logits"], r["d_logits_abs"])
            _check(t + " d_w_last", d_w.cpu().numpy(), w0 + r["d_w"], np.abs(w0) + r["d_w_abs"], 2 * REL)
            got = dz.cpu().numpy()
            _check(t + " dz", got[sup], r["dz"][sup], r["dz_abs"][sup])
            if mode == 1:
                written = got.view(np.uint32) != SENTINEL
                assert np.array_equal(written, sup), t + ": %d entries off the support written, %d of it not" % (
                    int((written & ~sup).sum()), int((sup & ~written).sum()))
            else:
                assert np.all(got[~sup] == 0.0), t + ": non-zero off the support"
            if mode == 0 and act == 1:
                dz2, d_w2 = _filled((S, E, ns, c), fill, rs), _t(w0)
                dl2 = _bwd(lib, cx, dv, Hd, wd, bhd, gd, lpd, act, dz2, mode, d_w2)
                for a, b in ((dz, dz2), (dl, dl2), (d_w, d_w2)):
                    assert np.array_equal(_bits(a), _bits(b)), t + ": two backward launches differ"

    # scn_readout_clear_dz zeroes exactly what the backward writes
    dz = _filled((S, E, ns, c), "sentinel", rs)
    _clear(lib, cx, dv, c, dz)
    got = dz.cpu().numpy()
    sup = np.broadcast_to(r["support"][..., None], (S, E, ns, c))
    kept = got.view(np.uint32) == SENTINEL
    assert np.array_equal(~kept, sup), tag + ": clear_dz wrote %d entries off the support and missed %d" % (
        int((~kept & ~sup).sum()), int((sup & kept).sum()))
    assert np.all(got[sup] == 0.0)


def test_readout_rejects_more_than_1024_slots_before_launching(lib):
    """max_deg 1025: SCN_ERR_UNSUPPORTED from every readout entry point, a host check (nothing is launched)."""
    buf = torch.zeros(64, device="cuda")
    ib = torch.zeros(64, device="cuda", dtype=torch.int32)
    P, I, s = _p(buf), _p(ib), _stream()
    assert lib.scn_readout_forward(1, 1, 2, 1, P, P, I, 2, 1025, I, I, I, P, P, P, P, s) == SCN_ERR_UNSUPPORTED
    assert lib.scn_readout_backward(1, 1, 2, 1, P, P, I, 2, 1025, I, I, I, P, I, P, P, P, 0, P, P, 1, P, s) == SCN_ERR_UNSUPPORTED
    assert lib.scn_readout_clear_dz(1, 1, 2, 1, I, 2, 1025, I, I, I, I, P, s) == SCN_ERR_UNSUPPORTED
    assert lib.scn_node_readout_forward(1, 1, 2, P, I, 1025, I, P, P, s) == SCN_ERR_UNSUPPORTED
    assert lib.scn_node_readout_backward(1, 1, 2, P, I, 1025, I, P, P, 0, P, s) == SCN_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert np.all(buf.cpu().numpy() == 0.0)


# ------------------------------------------------------------------------------------------------------------------
# node readout (Bunch, TE:198-203)
# ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["mixed", "wide", "deg1024"])
def test_node_readout_matches_fp64_with_wrapped_slots(lib, name, act):
    cx, dv = _tables(name)
    rs = np.random.RandomState(31 + act)
    S, ns, V, D = cx["S"], cx["ns"], cx["n_nodes"], cx["D"]
    N = S * ns
    rows = cx["nbr"][cx["last"][:cx["n_real"]]]
    if name != "deg1024":                                   # a real neighbour V - 1 and wrapped -1 slots in one trajectory
        assert ((rows == V - 1).any(axis=1) & (rows < 0).any(axis=1)).any()
    X = rs.uniform(-2, 2, (S, V, ns))
    X[rs.rand(*X.shape) < 0.1] = 0.0
    X = X.astype(np.float32)
    Xd = _t(X)
    ref = so.slab_node_readout_forward(X, cx["nbr"], cx["last"])
    logits, logp = torch.empty((N, D), device="cuda"), torch.empty((N, D), device="cuda")
    args = (S, ns, V, _p(Xd), _p(dv["nbr"]), D, _p(dv["last"]))
    assert lib.scn_node_readout_forward(*args, _p(logits), _p(logp), _stream()) == 0
    torch.cuda.synchronize()
    tag = "%s act=%d" % (name, act)
    assert np.array_equal(logits.cpu().numpy(), ref["logits"].astype(np.float32)), tag + ": logits are not the gathered values"
    _check(tag + " logp", logp.cpu().numpy(), ref["logp"], ref["logp_abs"])

    g = _d_logp(rs, cx)
    lp_in = ref["logp"].astype(np.float32)
    gd, lpd = _t(g), _t(lp_in)
    r = so.slab_node_readout_backward(X, cx["nbr"], cx["last"], g, lp_in, act)
    outs = []
    for _ in range(2):
        dz = _filled((S, V, ns), "garbage", rs)
        assert lib.scn_node_readout_backward(*args, _p(gd), _p(lpd), act, _p(dz), _stream()) == 0
        torch.cuda.synchronize()
        outs.append(dz)
    _check(tag + " dz", outs[0].cpu().numpy(), r["dz"], r["dz_abs"])
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])), tag + ": two backward launches differ"


# ------------------------------------------------------------------------------------------------------------------
# scn_logits_sum_log_softmax
# ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_parts", [1, 2, 3, 4])
@pytest.mark.parametrize("max_deg", [1, 13, 64, 65, 200])
def test_logits_sum_log_softmax_with_logits_aliased_to_the_first_part(lib, max_deg, n_parts):
    from scone_gcn_amd._lib import ptr_array
    rs = np.random.RandomState(max_deg * 10 + n_parts)
    N = 37
    parts = rs.uniform(-80, 80, (n_parts, N, max_deg)).astype(np.float32)
    parts[:, 0], parts[:, 1] = 80.0, -80.0                  # sums of up to +-320: exp overflows / underflows without the max
    pd = [_t(p) for p in parts]
    logp = torch.empty((N, max_deg), device="cuda")
    assert lib.scn_logits_sum_log_softmax(N, max_deg, n_parts, ptr_array([p.data_ptr() for p in pd]), _p(pd[0]), _p(logp),
                                          _stream()) == 0
    torch.cuda.synchronize()
    P = parts.astype(np.float64)
    z, z_abs = P.sum(axis=0), np.abs(P).sum(axis=0)
    ref_lp, lp_abs = so._log_softmax_bars(z, z_abs)
    tag = "max_deg=%d n_parts=%d" % (max_deg, n_parts)
    _check(tag + " logits", pd[0].cpu().numpy(), z, z_abs)
    _check(tag + " logp", logp.cpu().numpy(), ref_lp, lp_abs)


def test_logits_sum_log_softmax_rejects_0_and_5_parts(lib):
    from scone_gcn_amd._lib import ptr_array
    buf = torch.zeros(8, device="cuda")
    ptrs = ptr_array([buf.data_ptr()] * 5)
    for n_parts in (0, 5):
        assert lib.scn_logits_sum_log_softmax(2, 4, n_parts, ptrs, _p(buf), _p(buf), _stream()) == SCN_ERR_BAD_SHAPE


# ------------------------------------------------------------------------------------------------------------------
# scn_masked_ce / scn_masked_ce_begin
# ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,zero_n", [(1, 0), (1023, 1), (1024, 1023), (1025, 1024), (3 * 1024 + 7, 1025), (10 ** 6, 5003)])
def test_masked_ce(lib, n, zero_n):
    rs = np.random.RandomState(n % 1000 + 41)
    logp = (-rs.uniform(0, 20, n)).astype(np.float32)
    y = (rs.rand(n) < 0.1).astype(np.float32) * rs.uniform(0.5, 1.5, n).astype(np.float32)
    scale = np.float32(-1.0 / 123.0)
    want_d = y * scale                                                                 # one fp32 multiply
    want = math.fsum((logp.astype(np.float64) * want_d.astype(np.float64)).tolist())
    lpd, yd = _t(logp), _t(y)

    def run(start, overwrite=None, zero=None):
        d = torch.full((n,), 7.0, device="cuda")
        loss = torch.full((1,), start, device="cuda", dtype=torch.float64)
        if overwrite is None:
            st = lib.scn_masked_ce(n, _p(lpd), _p(yd), float(scale), _p(d), _p(loss), _stream())
        else:
            st = lib.scn_masked_ce_begin(n, _p(lpd), _p(yd), float(scale), _p(d), _p(loss), overwrite,
                                         _p(zero) if zero is not None else None, zero_n if zero is not None else 0, _stream())
        assert st == 0
        torch.cuda.synchronize()
        return d.cpu().numpy(), float(loss.item())

    d, loss = run(2.5)
    assert np.array_equal(d.view(np.uint32), want_d.view(np.uint32)), "d_logp is not fp32(y * scale)"
    assert abs((loss - 2.5) - want) <= 1e-12 * abs(want) + 1e-15
    _, loss2 = run(2.5)
    assert loss2 == loss                                                               # bitwise repeatable
    zero = _filled((zero_n + 16,), "sentinel", rs)
    d, loss = run(7.0, overwrite=1, zero=zero if zero_n else None)
    assert np.array_equal(d.view(np.uint32), want_d.view(np.uint32))
    assert abs(loss - want) <= 1e-12 * abs(want) + 1e-15, "overwrite must set the loss"
    z = zero.cpu().numpy()
    assert np.all(z[:zero_n] == 0.0) and np.all(z[zero_n:].view(np.uint32) == SENTINEL), "zero_buf: not exactly zero_n floats"
    _, loss_acc = run(7.0, overwrite=0)
    assert abs((loss_acc - 7.0) - want) <= 1e-12 * abs(want) + 1e-15


# ------------------------------------------------------------------------------------------------------------------
# the pooled readout-gradient buffer of one SconePlan (dz_is_zero = 1 + scn_readout_clear_dz between batches)
# ------------------------------------------------------------------------------------------------------------------


def _plan_case():
    from scone_gcn_amd import synthetic_data_gen as g
    from scone_gcn_amd.complex import SimplicialComplex
    cx0 = COMPLEXES["mixed"]()
    edges = np.unique(np.sort(cx0["edges"], axis=1), axis=0)
    cx = g.Complex(n_nodes=cx0["n_nodes"], edges=edges, faces=np.zeros((0, 3), np.int64))
    return cx, SimplicialComplex(cx)


def test_pooled_readout_gradient_is_clean_for_the_next_batch(lib):
    """Two batches back to back on one plan, ending at disjoint node sets (hub-B side, then the serial hub-A side, and the
    reverse): the second batch's gradients equal a fresh plan's bit for bit and the fp64 oracle's.  Once with the Bconds
    object, once with a plain Bcond_func closure (ProbedBconds tables: pseudo-node ids, -2 endpoints)."""
    from scone_gcn_amd import ops, trajectory_experiments as te
    cx, sc = _plan_case()
    E, V = cx.n_edges, cx.n_nodes
    B1 = sc.B1.toarray()
    nb, D = so.neighborhoods(cx.edges, V)
    L_lo, L_up = so.scone_shifts(B1, np.zeros((E, 0)))
    rs = np.random.RandomState(51)
    # (scale 0.1: the hubs of degree 40-48 amplify larger weights until a plain fp32 evaluation is itself off by > 1e-5)
    w = [0.1 * a for a in (rs.randn(*s) for s in so.weight_shapes(1, [(3, 16)] * 3, 1))]
    N = 320
    assert (N // ops.NS) * E * ops.NS * 16 * 4 > ops.SconePlan.SMALL_DZ_BYTES          # the pooled form, not the self-zeroing one
    side_b = np.arange(13, 63)                                                         # hub B, its leaves, the isolated node
    side_a = np.array([0] + list(range(1, 13)) + list(range(63, 103)))                 # hub A, satellites, u_i: serial item lists
    batches = {}
    for key, pool in (("b", side_b), ("a", side_a)):
        last = rs.choice(pool, N)
        X = np.zeros((N, E, 1))
        for n in range(N):
            X[n, rs.choice(E, 6, replace=False), 0] = rs.choice([-1.0, 1.0], 6)
        y = so.onehot_targets(rs.randint(0, np.maximum((nb[last] >= 0).sum(1), 1)), D)
        batches[key] = (last, X, y)

    def grads(shifts, readout, key):
        last, X, y = batches[key]
        wt = [torch.tensor(a, dtype=torch.float32, device="cuda", requires_grad=True) for a in w]
        out = te.scone_func(wt, *shifts, readout, last, X)
        loss = -(out * torch.as_tensor(y, dtype=torch.float32, device="cuda")).sum() / N
        loss.backward()
        torch.cuda.synchronize()
        return [t.grad.cpu().numpy() for t in wt]

    ref = {k: so.scone_loss_and_grad(w, L_lo, L_up, so.make_Bconds(B1, nb), *batches[k], np.ones(N, int), 0.0)[1] for k in batches}
    for closure in (False, True):
        for first, second in (("b", "a"), ("a", "b")):
            tag = "%s, %s then %s" % ("closure" if closure else "Bconds", first, second)
            shifts, readout, _ = te.setup_from_complex(sc, "scone")
            if closure:
                readout = so.make_Bconds(B1, nb)
            grads(shifts, readout, first)
            plan = next(iter(shifts[0]._cache.values()))
            pooled = [k for k, v in plan._dz_zero.items() if v and v[0].numel() * 4 > plan.SMALL_DZ_BYTES]
            assert pooled, tag + ": the pooled readout-gradient buffer was not used"
            g2 = grads(shifts, readout, second)
            shifts_f, readout_f, _ = te.setup_from_complex(sc, "scone")
            if closure:
                readout_f = so.make_Bconds(B1, nb)
            fresh = grads(shifts_f, readout_f, second)
            for k, (a, b) in enumerate(zip(g2, fresh)):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: weight %d differs from a fresh plan" % (tag, k)
            for k, (a, b) in enumerate(zip(g2, ref[second])):
                err = float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))
                assert err <= 1e-5, "%s: weight %d off the oracle by %.3g" % (tag, k, err)
