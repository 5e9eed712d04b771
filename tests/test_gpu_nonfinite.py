"""GPU tests of NaN, +-Inf and fp32-extreme data through the fused layer kernels ("Non-finite data").

Every kernel output is held against a plain fp64 CSR evaluation of the same operation (scipy CSR with explicit zeros removed, so a
NaN spreads only along stored entries):
(1) lower bound: an output the CSR evaluation makes non-finite is non-finite in the kernel's output (NaN may stand for +-Inf);
(2) upper bound (forward outputs): a trajectory whose input is finite gets a finite output -- trajectories are independent samples;
(3) everything finite on both sides matches to the usual bar, 8e-6 of each output's sum of |terms| (plus 1e-6 absolute where an
    activation is applied: fast tanh is good to ~3e-7).
The cases put a NaN into an otherwise all-zero slab (the zero-tile early-outs decide on a NaN-ignoring max), onto a sparse finite
background (early-out tiles and full tiles side by side), +Inf / -Inf / NaN into different trajectories of one slab, and a NaN into
one weight matrix with an all-zero input (0 * NaN is NaN everywhere in its column).  A second group runs finite data at both ends of
fp32 (rows below the split's scale clamp, rows of 1e30 .. 1e37, pre-activations that must overflow)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import scone_oracle as so

pytestmark = pytest.mark.gpu

ACTS = {"none": lambda z: z, "tanh": np.tanh, "relu": lambda z: np.where(z > 0, z, np.where(np.isnan(z), z, 0.0)),
        "leaky_relu": lambda z: np.where(z >= 0, z, 0.01 * z)}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_ENV = {}


def _scone_env():
    """random_SC_graph(2000) with its scone plan and the device-order fp64 CSR shifts (explicit zeros removed)."""
    if "scone" not in _ENV:
        from scone_gcn_amd import ops, synthetic_data_gen as g, trajectory_experiments as te
        from scone_gcn_amd.complex import SimplicialComplex
        cx = g.random_SC_graph(2000)
        sc = SimplicialComplex(cx)
        shifts, readout, _ = te.setup_from_complex(sc, "scone")
        plan = ops.get_scone_plan(shifts[0], shifts[1], readout, "tanh", ops.default_device())
        ops_ = []
        for s in shifts:
            m = s.device_csr().astype(np.float64).tocsr()
            m.eliminate_zeros()
            ops_.append(m)
        _ENV["scone"] = (cx.n_edges, plan, ops_[0], ops_[1])
    return _ENV["scone"]


def _mm(a, w):
    """a @ w over the last axis without BLAS (a BLAS may skip zero operands: 0 * NaN must be NaN here)."""
    return np.einsum("...i,ij->...j", a, w, optimize=False)


def _shift(m, x):
    """CSR (rows x rows_src) applied to [S, rows_src, ns, C] in fp64."""
    S, R, ns, C = x.shape
    y = m @ x.transpose(1, 0, 2, 3).reshape(R, -1)
    return y.reshape(m.shape[0], S, ns, C).transpose(1, 0, 2, 3)


def _layer_ref(x, W, lo, up):
    """pre-activation sum_k (S_k x) W_k and each output's sum of |terms| (S_0 = identity), fp64."""
    x = x.astype(np.float64)
    W = [w.astype(np.float64) for w in W]
    gk = [x, _shift(lo, x), _shift(up, x)]
    with np.errstate(invalid="ignore", over="ignore"):
        ga = [np.abs(x), _shift(abs(lo), np.abs(x)), _shift(abs(up), np.abs(x))]
        z = sum(_mm(a, w) for a, w in zip(gk, W))
        s = sum(_mm(a, np.abs(w)) for a, w in zip(ga, W))
    return z, s, gk, ga


def _check(got, ref, scale, bad_traj=None, absolute=0.0, what="", bar=True):
    """(1) lower bound, (2) the per-trajectory upper bound (bad_traj: [S, ns] bool of trajectories with a non-finite input; None:
    no upper bound), (3) the bar on everything finite on both sides."""
    got = np.asarray(got, np.float64)
    ref_nf, got_nf = ~np.isfinite(ref), ~np.isfinite(got)
    assert got_nf[ref_nf].all(), "%s: %d non-finite reference outputs came out finite" % (what, int((ref_nf & ~got_nf).sum()))
    if bad_traj is not None:
        clean = ~bad_traj                                         # [S, ns]
        assert np.isfinite(got.transpose(0, 2, 1, 3)[clean]).all(), "%s: a non-finite value reached another trajectory" % what
    if not bar:
        return
    both = ~ref_nf & ~got_nf
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(got - ref)[both]
        sc = scale[both] if scale is not None else np.full(err.shape, np.inf)
        tol = np.where(np.isfinite(sc), 8e-6 * sc + absolute, 1e-5 * np.maximum(1.0, np.abs(ref[both])))
    assert (err <= tol).all(), "%s: max excess %g" % (what, float((err - tol).max()) if err.size else 0.0)


def _bad(x):
    return ~np.isfinite(x).all(axis=(1, 3))                      # [S, ns]


def _case(case, S, E, C, rs):
    """Input slabs [S, E, 4, C] with a few non-finite values placed on purpose."""
    x = np.zeros((S, E, 4, C), np.float32)
    if case == "sparse":                                          # trajectory-like support: ~3 % of the rows, every trajectory
        for s in range(S):
            for n in range(4):
                rows = rs.choice(E, E // 32, replace=False)
                x[s, rows, n] = rs.randn(len(rows), C)
    if case in ("zero", "sparse"):                                # ONE NaN: on the zero background the only non-zero of its tile
        x[S - 1, E // 3, 1, C // 2] = np.nan
    elif case == "infs":                                          # +Inf, -Inf, NaN in three trajectories of one slab
        x[S - 1] = rs.randn(E, 4, C) * 0.5
        x[S - 1, E // 5, 0, 0] = np.inf
        x[S - 1, E // 2, 1, C - 1] = -np.inf
        x[S - 1, (4 * E) // 5, 2, C // 3] = np.nan
    return x


def _weights(C_in, C_out, rs, scale=0.3):
    return [(scale * rs.randn(C_in, C_out)).astype(np.float32) for _ in range(3)]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------------------
# one layer: forward (C = 32, the C = 16 slab-pair form with its odd tail, the generic widths), accumulate form, backward
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,S", [(32, 1), (32, 3), (16, 1), (16, 2), (16, 3), (8, 2), (40, 2)])
@pytest.mark.parametrize("case", ["zero", "sparse", "infs"])
def test_layer_forward_propagates_nonfinite_values_along_the_operator(C, S, case):
    _need_gpu()
    E, plan, lo, up = _scone_env()
    rs = np.random.RandomState(C * 10 + S)
    x = _case(case, S, E, C, rs)
    W = _weights(C, C, rs)
    z, scale, _, _ = _layer_ref(x, W, lo, up)
    for act in ("none", "tanh", "relu", "leaky_relu"):
        out = plan.conv.forward([_t(x)], [_t(w) for w in W], C, act).cpu().numpy()
        with np.errstate(invalid="ignore"):
            ref = ACTS[act](z)
        _check(out, ref, scale, _bad(x), 0.0 if act == "none" else 1e-6, "C=%d S=%d %s %s" % (C, S, case, act))


@pytest.mark.parametrize("C", [32, 16, 8])
def test_nan_weight_reaches_every_row_of_its_column_on_zero_input(C):
    """A NaN in W_1 with an all-zero input: the CSR evaluation is NaN in that output column everywhere (0 * NaN), the rest 0."""
    _need_gpu()
    E, plan, lo, up = _scone_env()
    rs = np.random.RandomState(5)
    S = 2
    x = np.zeros((S, E, 4, C), np.float32)
    W = _weights(C, C, rs)
    W[1][C // 4, C // 2] = np.nan
    z, scale, _, _ = _layer_ref(x, W, lo, up)
    assert np.isnan(z[..., C // 2]).all()
    for act in ("none", "relu", "tanh"):
        out = plan.conv.forward([_t(x)], [_t(w) for w in W], C, act).cpu().numpy()
        with np.errstate(invalid="ignore"):
            _check(out, ACTS[act](z), scale, None, 1e-6, "C=%d %s" % (C, act))
    # backward: dx = (sum_k S_k^T dz W_k^T) act'(aux) is NaN in row C // 4 everywhere
    aux = np.tanh(rs.randn(S, E, 4, C)).astype(np.float32)
    dWs = [torch.zeros(C, C, device="cuda") for _ in range(3)]
    dx = plan.conv.backward([_t(x)], [_t(w) for w in W], _t(aux), "tanh", True, dWs)
    if dx is not None:
        assert np.isnan(dx.cpu().numpy()[..., C // 4]).all()


def test_accumulate_form_at_hidden_64():
    """act(partial + sum_k (S_k x) W_k) (hidden widths above 32 add their 32-channel blocks through `partial=`): a NaN in x on a zero
    slab and a NaN in the partial on a zero tile both reach the output."""
    _need_gpu()
    E, plan, lo, up = _scone_env()
    rs = np.random.RandomState(64)
    S, C = 2, 32
    x = _case("zero", S, E, C, rs)
    part = np.zeros((S, E, 4, C), np.float32)
    part[0, E // 2, 3, 7] = np.nan
    part[0, : E // 4] = rs.randn(E // 4, 4, C)
    W = _weights(C, C, rs)
    z, scale, _, _ = _layer_ref(x, W, lo, up)
    z = z + part
    scale = scale + np.abs(part)
    for act in ("none", "tanh", "relu", "leaky_relu"):
        out = plan.conv.forward([_t(x)], [_t(w) for w in W], C, act, partial=_t(part)).cpu().numpy()
        with np.errstate(invalid="ignore"):
            _check(out, ACTS[act](z), scale, _bad(x) | _bad(part), 0.0 if act == "none" else 1e-6, "accumulate %s" % act)


def _bwd_ref(dz, aux, W, lo, up, act):
    z, _, gk, ga = _layer_ref(dz, [w.T for w in W], lo.T.tocsr(), up.T.tocsr())
    with np.errstate(invalid="ignore", over="ignore"):
        sdx = sum(_mm(a, np.abs(w.astype(np.float64)).T) for a, w in zip(ga, W))
        a64 = aux.astype(np.float64)
        dact = (1.0 - a64 ** 2) if act == "tanh" else (a64 > 0).astype(np.float64)
        dx = z * dact
        dW = [np.einsum("srnc,srnd->cd", a64, g, optimize=False) for g in gk]
        sdW = [np.einsum("srnc,srnd->cd", np.abs(a64), g, optimize=False) for g in ga]
    return dx, sdx, dW, sdW


@pytest.mark.parametrize("C", [32, 16])
@pytest.mark.parametrize("case", ["zero", "sparse", "infs"])
def test_layer_backward_propagates_nonfinite_gradients(C, case):
    """scn_conv_backward with need_dx and the weight gradients: a NaN gradient alone in its tile must not be dropped by the
    early-out (dx there, and the whole dW column it feeds).  dx has no per-trajectory upper bound.  An Inf in the
    gradient sets its whole tile's scale (and the wave's running dW units) to the largest one, which flushes the tile's other values
    and the dW accumulated so far: with Infs only the lower bound is asserted ("Non-finite data")."""
    _need_gpu()
    E, plan, lo, up = _scone_env()
    rs = np.random.RandomState(7 + C)
    S = 3
    dz = _case(case, S, E, C, rs)
    W = _weights(C, C, rs)
    for act in ("tanh", "relu"):
        aux = (np.tanh(rs.randn(S, E, 4, C)) if act == "tanh" else np.maximum(rs.randn(S, E, 4, C), 0.0)).astype(np.float32)
        dWs = [torch.zeros(C, C, device="cuda") for _ in range(3)]
        dx = plan.conv.backward([_t(dz)], [_t(w) for w in W], _t(aux), act, True, dWs).cpu().numpy()
        rdx, sdx, rdW, sdW = _bwd_ref(dz, aux, W, lo, up, act)
        _check(dx, rdx, sdx, None, 0.0, "dx C=%d %s %s" % (C, case, act), bar=case != "infs")
        for k in range(3):
            got = dWs[k].cpu().numpy().astype(np.float64)
            ref_nf = ~np.isfinite(rdW[k])
            assert (~np.isfinite(got))[ref_nf].all(), "dW%d C=%d %s %s" % (k, C, case, act)
            if case != "infs":
                both = np.isfinite(rdW[k]) & np.isfinite(got)
                assert (np.abs(got - rdW[k])[both] <= 1e-4 * sdW[k][both] + 1e-30).all(), "dW%d C=%d %s %s" % (k, C, case, act)


def test_dual_spmm_lower_and_per_trajectory_upper_bound():
    """scn_spmm_dual: its ELL pads are zero-valued entries that read a real row, so only the lower bound and the upper bound apply
    (here per slab: the finite slab 0 stays finite), with the bar on what is finite on both sides."""
    _need_gpu()
    E, plan, lo, up = _scone_env()
    rs = np.random.RandomState(3)
    for k in (4, 64, 128):
        x = np.zeros((3, E, k), np.float32)
        x[0] = rs.randn(E, k)
        x[1, E // 2, k // 2] = np.nan
        x[2, E // 3, 0] = np.inf
        ya, yb = plan.conv.spmm_dual(_t(x))
        for y, m in ((ya, lo), (yb, up)):
            got = y.cpu().numpy()
            for s in range(3):
                with np.errstate(invalid="ignore"):
                    ref = m @ x[s].astype(np.float64)
                assert (~np.isfinite(got[s]))[~np.isfinite(ref)].all()
                if s == 0:
                    assert np.isfinite(got[s]).all()
                both = np.isfinite(ref) & np.isfinite(got[s])
                with np.errstate(invalid="ignore"):
                    assert (np.abs(got[s] - ref)[both] <= 2e-5 * max(1.0, np.abs(ref[both]).max())).all()


# ------------------------------------------------------------------------------------------------------------------
# the fused Bunch layer (terms kernels)
# ------------------------------------------------------------------------------------------------------------------

def test_fused_bunch_layer_keeps_a_nan_in_a_zero_tile():
    _need_gpu()
    from scone_gcn_amd import ops, synthetic_data_gen as g, trajectory_experiments as te
    from scone_gcn_amd.complex import SimplicialComplex
    cx = g.random_SC_graph(1500)
    sc = SimplicialComplex(cx)
    shifts, nbr, _ = te.setup_from_complex(sc, "bunch")
    plan = ops.get_bunch_plan(shifts, nbr, ops.default_device())
    fwd, bwd = plan._terms_ops()
    S, sizes = 2, plan.sizes
    rs = np.random.RandomState(4)
    dev = []
    for s in shifts:
        m = s.device_csr().astype(np.float64).tocsr()
        m.eliminate_zeros()
        dev.append(m)
    SRC, DST = ops.BUNCH_SRC, ops.BUNCH_DST
    xs = [np.zeros((S, n, 4, 32), np.float32) for n in sizes]
    xs[1][1, sizes[1] // 2, 2, 5] = np.nan                       # an edge-level NaN, everything else zero
    xs[0][0, : sizes[0] // 3] = rs.randn(sizes[0] // 3, 4, 32)  # and a finite node-level background in the other slab
    Wk = [(0.2 * rs.randn(32, 32)).astype(np.float32) for _ in range(7)]
    Ws = [[None] * 3 for _ in range(3)]
    for k in range(7):
        Ws[DST[k]][SRC[k]] = _t(Wk[k])
    outs = fwd.forward([_t(x) for x in xs], Ws, "relu", [True] * 3)
    bad = _bad(xs[0]) | _bad(xs[1]) | _bad(xs[2])
    for l in range(3):
        with np.errstate(invalid="ignore", over="ignore"):
            z = sum(_mm(_shift(dev[k], xs[SRC[k]].astype(np.float64)), Wk[k].astype(np.float64)) for k in range(7) if DST[k] == l)
            sc_ = sum(_mm(_shift(abs(dev[k]), np.abs(xs[SRC[k]].astype(np.float64))), np.abs(Wk[k].astype(np.float64)))
                      for k in range(7) if DST[k] == l)
        assert (~np.isfinite(z)).any() or l == 0
        _check(outs[l].cpu().numpy(), ACTS["relu"](z), sc_, bad, 1e-6, "terms fwd level %d" % l)
    # backward on the transposed operator with the same kind of input as the gradient
    dzs = [x.copy() for x in xs]
    auxs = [np.maximum(rs.randn(S, n, 4, 32), 0).astype(np.float32) for n in sizes]
    Wb = [[None] * 3 for _ in range(3)]
    dWb = [[None] * 3 for _ in range(3)]
    for k in range(7):
        a, b = SRC[k], DST[k]
        Wb[a][b], dWb[a][b] = _t(Wk[k]), torch.zeros(32, 32, device="cuda")
    dxs = ops._terms_backward(bwd, [_t(d) for d in dzs], Wb, [_t(a) for a in auxs], "relu", [True] * 3, dWb)
    for a in range(3):
        with np.errstate(invalid="ignore", over="ignore"):
            gk = {k: _shift(dev[k].T.tocsr(), dzs[DST[k]].astype(np.float64)) for k in range(7) if SRC[k] == a}
            ref = sum(_mm(gk[k], Wk[k].astype(np.float64).T) for k in gk) * (auxs[a] > 0)
            sdx = sum(_mm(np.abs(gk[k]), np.abs(Wk[k].astype(np.float64)).T) for k in gk)
        got = dxs[a].cpu().numpy()
        assert (~np.isfinite(got))[~np.isfinite(ref)].all(), "terms dx level %d" % a
        for k in gk:
            with np.errstate(invalid="ignore", over="ignore"):
                refw = np.einsum("srnc,srnd->cd", auxs[a].astype(np.float64), gk[k], optimize=False)
            gw = dWb[a][DST[k]].cpu().numpy()
            assert (~np.isfinite(gw))[~np.isfinite(refw)].all(), "terms dW %d" % k
            both = np.isfinite(refw) & np.isfinite(gw)
            assert (np.abs(gw - refw)[both] <= 2e-5 * max(1.0, np.abs(refw[both]).max() if both.any() else 1.0)).all()


# ------------------------------------------------------------------------------------------------------------------
# finite data at the ends of fp32
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [32, 16])
@pytest.mark.parametrize("lo_exp,hi_exp,wscale", [(-37, -34, 0.3), (30, 37, 1e-3)])
def test_rows_at_the_ends_of_fp32_hold_the_bar(C, lo_exp, hi_exp, wscale):
    """Rows whose largest magnitude lies under the split's scale clamp (2^-112) and rows of 1e30 .. 1e37: forward, dx and dW to the
    usual bar relative to each output's sum of |terms| (dW: 1e-4, fp32 accumulation over S * E * 4 terms)."""
    _need_gpu()
    E, plan, lo, up = _scone_env()
    rs = np.random.RandomState(C + abs(hi_exp))
    S = 3
    mag = 10.0 ** rs.uniform(lo_exp, hi_exp, size=(S, E, 4, C))
    x = (mag * rs.choice([-1.0, 1.0], size=mag.shape)).astype(np.float32)
    x[1] = 0.0                                                    # and a zero slab in between
    W = _weights(C, C, rs, wscale)
    z, scale, _, _ = _layer_ref(x, W, lo, up)
    out = plan.conv.forward([_t(x)], [_t(w) for w in W], C, "none").cpu().numpy()
    assert np.isfinite(out).all()
    _check(out, z, scale, None, 0.0, "fwd C=%d 1e%d..1e%d" % (C, lo_exp, hi_exp))
    # backward: the same rows as the incoming gradient (up to 1e34 so that dW stays inside fp32)
    dz = np.where(np.abs(x) > 1e34, np.sign(x) * 1e34, x).astype(np.float32)
    aux = np.tanh(rs.randn(S, E, 4, C)).astype(np.float32)
    dWs = [torch.zeros(C, C, device="cuda") for _ in range(3)]
    dx = plan.conv.backward([_t(dz)], [_t(w) for w in W], _t(aux), "tanh", True, dWs).cpu().numpy()
    rdx, sdx, rdW, sdW = _bwd_ref(dz, aux, W, lo, up, "tanh")
    assert np.isfinite(dx).all()
    # (below the clamp the input gradient is held to 1e-35 absolute on top of the bar: it misses the bar there)
    _check(dx, rdx, sdx, None, 1e-35 if hi_exp < 0 else 0.0, "dx C=%d" % C)
    for k in range(3):
        got = dWs[k].cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all() and (np.abs(got - rdW[k]) <= 1e-4 * sdW[k]).all(), (C, k)


@pytest.mark.parametrize("C", [32, 16])
def test_pre_activations_that_overflow_fp32(C):
    """act none: an fp64 pre-activation above 4e38 comes out +-Inf or NaN, never finite; one below 1e38 is finite and on the bar."""
    _need_gpu()
    E, plan, lo, up = _scone_env()
    rs = np.random.RandomState(9)
    S = 2
    x = np.zeros((S, E, 4, C), np.float32)
    x[0] = (rs.randn(E, 4, C) * 0.1).astype(np.float32)
    p = E // 2
    x[1, p, 2, 0] = 1e38                                          # (its shifts S x stay inside fp32: they are fp32 intermediates)
    W = _weights(C, C, rs, 0.1)
    W[1][:] = 0.0
    W[2][:] = 0.0
    W[0][0, :] = 0.0
    W[0][0, 0], W[0][0, 1], W[0][0, 2] = 6.0, 0.5, -6.0
    z, scale, _, _ = _layer_ref(x, W, lo, up)
    out = plan.conv.forward([_t(x)], [_t(w) for w in W], C, "none").cpu().numpy()
    assert abs(z[1, p, 2, 0]) > 4e38 and abs(z[1, p, 2, 2]) > 4e38 and abs(z[1, p, 2, 1]) < 1e38
    assert not np.isfinite(out[1, p, 2, 0]) and not np.isfinite(out[1, p, 2, 2])
    big = np.abs(z) > 4e38
    assert not np.isfinite(out[big]).any()
    ok = np.abs(z) < 1e38
    assert np.isfinite(out[ok]).all()
    assert (np.abs(out[ok] - z[ok]) <= 8e-6 * scale[ok]).all()
    assert np.isfinite(out[0]).all()                              # the other slab's trajectories


# ------------------------------------------------------------------------------------------------------------------
# end to end: loss and gradients, readout
# ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sc1(cfg1):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from scone_gcn_amd.complex import SimplicialComplex
    from scone_gcn_amd.synthetic_data_gen import Complex
    cx = Complex(n_nodes=cfg1["n_nodes"], edges=cfg1["edges"].astype(np.int64), faces=cfg1["faces"].astype(np.int64),
                 coords=cfg1["coords"])
    return SimplicialComplex(cx)


def _nan_flows(cfg1, sel):
    """The selected trajectories' flows with ONE NaN: trajectory `bad` on an edge at its last node (in its support)."""
    X = np.array(cfg1["flows"][sel], np.float64)
    B1 = cfg1["B1"]
    for t in range(len(sel)):
        last = cfg1["last_nodes"][sel[t]]
        cand = np.nonzero((X[t] != 0) & (B1[last] != 0))[0]
        if len(cand):
            X[t, cand[0]] = np.nan
            return X, t
    raise AssertionError("no trajectory with flow on an edge at its last node")


def _run(net, inputs, y, sel):
    staged = net.stage(inputs, y, sel)
    loss = float(net.grad_step_staged(inputs, staged, len(sel), apply=False))
    return loss, [t.detach().cpu().numpy().astype(np.float64) for t in net._grads]


@pytest.mark.parametrize("model,act,small,pairing", [("scone", "tanh", False, 0), ("scone", "relu", False, 0),
                                                     ("ebli", "leaky_relu", False, 0), ("bunch", "relu", False, 0),
                                                     ("scone", "tanh", True, 0), ("scone", "tanh", True, 1),
                                                     ("scone", "relu", True, 0), ("scone", "relu", True, 1)])
def test_nan_flow_reaches_the_loss_and_every_gradient_the_oracle_makes_nonfinite(cfg1, sc1, model, act, small, pairing):
    """One NaN in one trajectory's flow on an edge at its last node: the CSR oracle's loss is NaN; the loss and every gradient entry the
    oracle makes non-finite must be non-finite, on the layer path (dense mode) and the one-launch step (one workgroup per trajectory
    and paired).  On the layer path the readout's log-probabilities of every OTHER trajectory equal the clean run's bit for bit."""
    _need_gpu()
    import scipy.sparse as sp
    from scone_gcn_amd import _lib, ops, scone_trajectory_model as stm, trajectory_experiments as te
    sel = np.arange(3, 12)
    N = len(sel)
    X, bad = _nan_flows(cfg1, sel)
    y = cfg1["targets"][sel]
    B1, B2 = sp.csr_matrix(cfg1["B1"]), sp.csr_matrix(cfg1["B2"])
    nb, _ = so.neighborhoods(cfg1["edges"], cfg1["n_nodes"])
    mask = np.ones(N, int)
    layers = [(3, 16)] * 3 if model != "bunch" else [(7, 32)] * 3
    shifts, readout, _ = te.setup_from_complex(sc1, model)
    old = (ops.SMALL_STEP, ops.SMALL_STEP_MAX_EDGES)
    lib = _lib.load()
    plan = old_act = None
    try:
        ops.SMALL_STEP, ops.SMALL_STEP_MAX_EDGES = small, (1 << 30) if small else old[1]
        if small:
            assert lib.scn_small_step_pairing(pairing) == 0
        res = {}
        for name, flows in (("nan", X), ("clean", np.array(cfg1["flows"][sel], np.float64))):
            inputs = [readout, cfg1["last_nodes"][sel], flows]
            stm.reseed(1030)
            net = stm.Scone_GCN(1, 1e-3, N, 0.0, verbose=False)
            net.setup(te.MODEL_FUNCS[model], layers, shifts, inputs, y, None, mask, model_type=model)
            if model != "bunch":
                plan = net._plan(inputs)
                old_act = plan.act if old_act is None else old_act
                plan.act = act
            with ops.KernelTimer() as kt:
                res[name] = _run(net, inputs, y, np.arange(N))
            assert any(k.startswith("small_step") for k in kt.table()) == small
            w = [a.detach().cpu().numpy().astype(np.float64) for a in net.weights]
            if not small:
                res[name + "_logp"] = te.MODEL_FUNCS[model](net.weights, *shifts, readout, cfg1["last_nodes"][sel], flows)
                res[name + "_logp"] = res[name + "_logp"].detach().cpu().numpy()
    finally:
        ops.SMALL_STEP, ops.SMALL_STEP_MAX_EDGES = old
        if small:
            lib.scn_small_step_pairing(0)
        if plan is not None:
            plan.act = old_act
    if model == "bunch":
        shifts_o = []
        for m in so.bunch_shifts(cfg1["B1"], cfg1["B2"]):
            m = sp.csr_matrix(m)
            m.eliminate_zeros()
            shifts_o.append(m)
        ref_loss, ref_g = so.bunch_loss_and_grad(w, shifts_o, nb, cfg1["last_nodes"][sel], X, y, mask, 0.0)
    else:
        L_lo, L_up = (B1.T @ B1).tocsr(), (B2 @ B2.T).tocsr()
        if model == "ebli":
            L1 = (L_lo + L_up).tocsr()
            L_lo, L_up = L1, (L1 @ L1).tocsr()
        L_lo.eliminate_zeros()
        L_up.eliminate_zeros()
        B1x = sp.vstack([B1, sp.csr_matrix((1, B1.shape[1]))]).tocsr()
        Bc = lambda n: B1x[nb[n]].toarray()
        with np.errstate(invalid="ignore", over="ignore"):
            ref_loss, ref_g = so.scone_loss_and_grad(w, L_lo, L_up, Bc, cfg1["last_nodes"][sel], X, y, mask, 0.0, act=act)
    loss, grads = res["nan"]
    assert not np.isfinite(ref_loss)
    assert not np.isfinite(loss), "loss %r" % loss
    for k, (a, b) in enumerate(zip(grads, ref_g)):
        if model == "bunch":
            break                              # Bunch: the loss only -- some whole weight gradients stay finite
        a = a.reshape(b.shape)
        assert (~np.isfinite(a))[~np.isfinite(b)].all(), "gradient %d: %d oracle-non-finite entries came out finite" % (
            k, int((np.isfinite(a) & ~np.isfinite(b)).sum()))
    if not small:
        lp, lc = res["nan_logp"], res["clean_logp"]
        assert np.isnan(lp[bad]).all()
        others = np.arange(N) != bad
        assert np.array_equal(lp[others], lc[others])
