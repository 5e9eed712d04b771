"""GPU wiring test of the host launch layer: every launch site of the blocked, terms and dense kernels once per activation.

The kernels themselves are tested elsewhere (parity, fuzz, boundary, non-finite data); this file guards what sits between the C-ABI
and the launch -- which kernel form a call picks, which activation it is instantiated with, and which pointer goes into which
argument.  Every output is held against the fp64 CSR evaluation of tests/test_gpu_nonfinite.py (_layer_ref, _shift, _mm) with that
file's bar: 8e-6 of each output's sum of |terms|, plus 1e-6 absolute where an activation is applied (fast tanh is good to ~3e-7).
Data are finite and free of zeros, so no tile takes a zero early-out; S = 3 slabs (odd: the C = 16 slab-pair forms run their tail),
four trajectories per slab.  The complex is the 400-point synthetic one when its blocked plan is built, otherwise the 2000-point
one of test_gpu_nonfinite.py; the terms operator runs on the config-1 complex of the golden fixtures."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_nonfinite import ACTS, _layer_ref, _mm, _need_gpu, _scone_env, _shift, _t

pytestmark = pytest.mark.gpu

ACT_NAMES = ("none", "tanh", "relu", "leaky_relu")
DACT = {"none": lambda a: np.ones_like(a), "tanh": lambda a: 1.0 - a ** 2, "relu": lambda a: (a > 0).astype(np.float64),
        "leaky_relu": lambda a: np.where(a >= 0, 1.0, 0.01)}      # act' through the OUTPUT value, as the kernels have it
S = 3

_ENV = {}


def _fp64_csr(shift):
    m = shift.device_csr().astype(np.float64).tocsr()
    m.eliminate_zeros()
    return m


def _env():
    """(E, scone plan, S_lower, S_upper as fp64 CSR in device order)."""
    _need_gpu()
    if "scone" not in _ENV:
        from scone_gcn_amd import ops, synthetic_data_gen as g, trajectory_experiments as te
        from scone_gcn_amd.complex import SimplicialComplex
        cx = g.random_SC_graph(400)
        shifts, readout, _ = te.setup_from_complex(SimplicialComplex(cx), "scone")
        plan = ops.get_scone_plan(shifts[0], shifts[1], readout, "tanh", ops.default_device())
        if plan.conv.plan_info()[0] > 0:
            _ENV["scone"] = (cx.n_edges, plan, _fp64_csr(shifts[0]), _fp64_csr(shifts[1]))
        else:
            _ENV["scone"] = _scone_env()
    return _ENV["scone"]


def _bunch_env(cfg1):
    """(level sizes, forward terms operator, transposed terms operator, the seven shifts as fp64 CSR) of the config-1 complex."""
    _need_gpu()
    if "bunch" not in _ENV:
        from scone_gcn_amd import ops, trajectory_experiments as te
        from scone_gcn_amd.complex import SimplicialComplex
        from scone_gcn_amd.synthetic_data_gen import Complex
        cx = Complex(n_nodes=cfg1["n_nodes"], edges=cfg1["edges"].astype(np.int64), faces=cfg1["faces"].astype(np.int64),
                     coords=cfg1["coords"])
        shifts, nbr, _ = te.setup_from_complex(SimplicialComplex(cx), "bunch")
        plan = ops.get_bunch_plan(shifts, nbr, ops.default_device())
        terms = plan._terms_ops()
        assert terms is not None, "the fused Bunch operators were not built"
        _ENV["bunch"] = (plan.sizes, terms[0], terms[1], [_fp64_csr(s) for s in shifts], plan)
    return _ENV["bunch"][:4]


def _rand(rs, *shape):
    """finite, no zeros, nothing below 1e-3 in magnitude"""
    a = rs.randn(*shape)
    return (a + np.sign(a) * 1e-3).astype(np.float32)


def _aux(rs, act, *shape):
    """a saved layer output that act could have produced (tanh: inside (-1, 1); relu: positive or zero-free negative stand-ins)"""
    a = _rand(rs, *shape)
    return np.tanh(a).astype(np.float32) if act == "tanh" else a


def _weights(rs, c_in, c_out, scale=0.3):
    return [(scale * _rand(rs, c_in, c_out)).astype(np.float32) for _ in range(3)]


def _close(got, ref, scale, absolute, what):
    got = (got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)).astype(np.float64)
    assert got.shape == ref.shape, "%s: shape %s against %s" % (what, got.shape, ref.shape)
    tol = 8e-6 * scale + absolute
    err = np.abs(got - ref)
    print("%s: worst error %.3g of its bar" % (what, float((err / tol).max())))
    assert np.isfinite(got).all(), "%s: non-finite output" % what
    assert float(np.abs(ref).max()) > 1e-3, "%s: the reference is trivially small" % what
    assert (err <= tol).all(), "%s: %d outputs over the bar, worst %.3g of it" % (what, int((err > tol).sum()), float((err / tol).max()))


def _fwd_abs(act):
    return 0.0 if act == "none" else 1e-6


def _bwd_ref(gk, ga, W, aux, act):
    """dx = (sum_k g_k W_k^T) act'(aux), dW_k = aux^T g_k from the gathered gradient terms g_k (ga: of |.|), with their sums of |terms|."""
    a = aux.astype(np.float64)
    Wd = [w.astype(np.float64) for w in W]
    dx = sum(_mm(g, w.T) for g, w in zip(gk, Wd)) * DACT[act](a)
    sdx = sum(_mm(g, np.abs(w).T) for g, w in zip(ga, Wd))
    dW = [np.einsum("srnc,srnd->cd", a, g, optimize=False) for g in gk]
    sdW = [np.einsum("srnc,srnd->cd", np.abs(a), g, optimize=False) for g in ga]
    return dx, sdx, dW, sdW


def _conv_terms(dz, lo, up):
    """the three gathered terms of a layer's backward, [dz, S_lo^T dz, S_up^T dz], and the same of |.|"""
    _, _, gk, ga = _layer_ref(dz, [np.zeros((dz.shape[3], 1), np.float32)] * 3, lo.T.tocsr(), up.T.tocsr())
    return gk, ga


def _zeros(*shape):
    return torch.zeros(*shape, device="cuda")


# ------------------------------------------------------------------------------------------------------------------
# one layer on the fused operator (identity + S_lower + S_upper)
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [32, 16])
def test_forward(C):
    E, plan, lo, up = _env()
    rs = np.random.RandomState(C)
    x, W = _rand(rs, S, E, 4, C), _weights(rs, C, C)
    z, scale, _, _ = _layer_ref(x, W, lo, up)
    for act in ACT_NAMES:
        out = plan.conv.forward([_t(x)], [_t(w) for w in W], C, act)
        _close(out, ACTS[act](z), scale, _fwd_abs(act), "forward C=%d %s" % (C, act))


def test_forward_with_partial():
    E, plan, lo, up = _env()
    rs = np.random.RandomState(2)
    x, part, W = _rand(rs, S, E, 4, 32), _rand(rs, S, E, 4, 32), _weights(rs, 32, 32)
    z, scale, _, _ = _layer_ref(x, W, lo, up)
    for act in ACT_NAMES:
        out = plan.conv.forward([_t(x)], [_t(w) for w in W], 32, act, partial=_t(part))
        _close(out, ACTS[act](z + part), scale + np.abs(part), _fwd_abs(act), "forward + partial %s" % act)


@pytest.mark.parametrize("C", [16, 32])
def test_forward_first(C):
    E, plan, lo, up = _env()
    rs = np.random.RandomState(100 + C)
    x, Wf = _rand(rs, S, E, 4, 1), _weights(rs, 1, C, 0.5)
    z, scale, gk, ga = _layer_ref(x, Wf, lo, up)
    for act in ACT_NAMES:
        res = plan.conv.forward_first(_t(x), [_t(w) for w in Wf], C, act)
        assert res is not None, "first layer not served"
        _close(res[0], ACTS[act](z), scale, _fwd_abs(act), "forward_first c_out=%d %s" % (C, act))
        y = res[1].cpu().numpy()
        assert not y[..., 3].any()
        _close(y[..., :3], np.concatenate(gk, axis=3), np.concatenate(ga, axis=3), 0.0, "forward_first y, c_out=%d %s" % (C, act))


def _first_layer(plan, rs, E, act):
    """the first layer's output H1 and shifted-input records y as the device made them (held to fp64 in test_forward_first)"""
    x, Wf = _rand(rs, S, E, 4, 1), _weights(rs, 1, 32, 0.5)
    H1, y = plan.conv.forward_first(_t(x), [_t(w) for w in Wf], 32, act)
    return Wf, H1, y


def test_forward_from_y():
    E, plan, lo, up = _env()
    rs = np.random.RandomState(3)
    W = _weights(rs, 32, 32)
    for act in ACT_NAMES:
        Wf, H1, y = _first_layer(plan, rs, E, act)
        out = plan.conv.forward_from_y(y, [_t(w) for w in Wf], [_t(w) for w in W], act)
        assert out is not None, "from-y forward not served"
        z, scale, _, _ = _layer_ref(H1.cpu().numpy(), W, lo, up)
        _close(out, ACTS[act](z), scale, _fwd_abs(act), "forward_from_y %s" % act)


@pytest.mark.parametrize("need_dx", [True, False])
@pytest.mark.parametrize("C", [32, 16])
def test_backward(C, need_dx):
    E, plan, lo, up = _env()
    rs = np.random.RandomState(200 + C)
    dz, W = _rand(rs, S, E, 4, C), _weights(rs, C, C)
    gk, ga = _conv_terms(dz, lo, up)
    for act in ACT_NAMES:
        aux = _aux(rs, act, S, E, 4, C)
        dWs = [_zeros(C, C) for _ in range(3)]
        dx = plan.conv_T.backward([_t(dz)], [_t(w) for w in W], _t(aux), act, need_dx, dWs)
        rdx, sdx, rdW, sdW = _bwd_ref(gk, ga, W, aux, act)
        what = "backward C=%d %s%s" % (C, act, "" if need_dx else " (dW only)")
        if need_dx:
            _close(dx, rdx, sdx, 0.0, what + " dx")
        else:
            assert dx is None
        for k in range(3):
            _close(dWs[k], rdW[k], sdW[k], 0.0, what + " dW%d" % k)


def test_backward_with_dx_partial():
    E, plan, lo, up = _env()
    rs = np.random.RandomState(4)
    dz, dxp, W = _rand(rs, S, E, 4, 32), _rand(rs, S, E, 4, 32), _weights(rs, 32, 32)
    gk, ga = _conv_terms(dz, lo, up)
    for act in ACT_NAMES:
        aux = _aux(rs, act, S, E, 4, 32)
        dWs = [_zeros(32, 32) for _ in range(3)]
        dx = plan.conv_T.backward([_t(dz)], [_t(w) for w in W], _t(aux), act, True, dWs, dx_partial=_t(dxp))
        rdx, sdx, rdW, sdW = _bwd_ref(gk, ga, W, aux, act)
        _close(dx, rdx + dxp, sdx + np.abs(dxp), 0.0, "backward + dx_partial %s dx" % act)
        for k in range(3):
            _close(dWs[k], rdW[k], sdW[k], 0.0, "backward + dx_partial %s dW%d" % (act, k))


def _first_ref(y, rdx, sdx):
    """dW_first[g][c] = sum_p y[p][g] dx[p][c]"""
    y = y.astype(np.float64)
    return (np.einsum("srng,srnc->gc", y[..., :3], rdx, optimize=False),
            np.einsum("srng,srnc->gc", np.abs(y[..., :3]), sdx, optimize=False))


def _check_fused_first(dWs, dWf, rdW, sdW, rf, sf, what):
    for k in range(3):
        _close(dWs[k], rdW[k], sdW[k], 0.0, what + " dW%d" % k)
        _close(dWf[k], rf[k][None], sf[k][None], 0.0, what + " dW_first%d" % k)


@pytest.mark.parametrize("C", [32, 16])
def test_backward_fused_first_with_aux(C):
    E, plan, lo, up = _env()
    rs = np.random.RandomState(300 + C)
    dz, W = _rand(rs, S, E, 4, C), _weights(rs, C, C)
    y = _rand(rs, S, E, 4, 4)
    y[..., 3] = 0.0
    gk, ga = _conv_terms(dz, lo, up)
    for act in ACT_NAMES:
        aux = _aux(rs, act, S, E, 4, C)
        dWs, dWf = [_zeros(C, C) for _ in range(3)], [_zeros(1, C) for _ in range(3)]
        assert plan.conv_T.backward_fused_first(_t(dz), [_t(w) for w in W], _t(aux), act, _t(y), dWs, dWf), "not served"
        rdx, sdx, rdW, sdW = _bwd_ref(gk, ga, W, aux, act)
        _check_fused_first(dWs, dWf, rdW, sdW, *_first_ref(y, rdx, sdx), "backward_fused_first C=%d %s" % (C, act))


def test_backward_fused_first_from_y():
    E, plan, lo, up = _env()
    rs = np.random.RandomState(5)
    dz, W = _rand(rs, S, E, 4, 32), _weights(rs, 32, 32)
    gk, ga = _conv_terms(dz, lo, up)
    for act in ACT_NAMES:
        Wf, H1, y = _first_layer(plan, rs, E, act)
        dWs, dWf = [_zeros(32, 32) for _ in range(3)], [_zeros(1, 32) for _ in range(3)]
        assert plan.conv_T.backward_fused_first(_t(dz), [_t(w) for w in W], None, act, y, dWs, dWf,
                                                Ws_first=[_t(w) for w in Wf]), "not served"
        rdx, sdx, rdW, sdW = _bwd_ref(gk, ga, W, H1.cpu().numpy(), act)
        _check_fused_first(dWs, dWf, rdW, sdW, *_first_ref(y.cpu().numpy(), rdx, sdx), "backward_fused_first from y, %s" % act)


# ------------------------------------------------------------------------------------------------------------------
# "power" layers: identity + one value array, act(x0 W0 + x W1 + (S x) W2)
# ------------------------------------------------------------------------------------------------------------------

def _power_op(E, lo):
    if "power" not in _ENV:
        from scone_gcn_amd import ops
        _ENV["power"] = ops.ConvOp(E, [{"mats": [lo], "identity": True, "n_cols": E}])       # S_lower is symmetric: its own transpose
        assert abs(lo - lo.T).nnz == 0
    return _ENV["power"]


@pytest.mark.parametrize("C", [32, 16])
def test_forward_and_backward_power(C):
    E, plan, lo, up = _env()
    op = _power_op(E, lo)
    rs = np.random.RandomState(400 + C)
    x0, x, W = _rand(rs, S, E, 4, C), _rand(rs, S, E, 4, C), _weights(rs, C, C)
    a0, a1 = x0.astype(np.float64), x.astype(np.float64)
    gk = [a0, a1, _shift(lo, a1)]
    ga = [np.abs(a0), np.abs(a1), _shift(abs(lo), np.abs(a1))]
    Wd = [w.astype(np.float64) for w in W]
    z = sum(_mm(g, w) for g, w in zip(gk, Wd))
    scale = sum(_mm(g, np.abs(w)) for g, w in zip(ga, Wd))
    for act in ACT_NAMES:
        out = op.forward_power(_t(x0), _t(x), [_t(w) for w in W], act)
        assert out is not None, "power forward not served"
        _close(out, ACTS[act](z), scale, _fwd_abs(act), "forward_power C=%d %s" % (C, act))
        # backward with dz := x0 and g1 := x: dx = (dz W0^T + g1 W1^T + (S g1) W2^T) act'(aux), dW = aux^T [dz, g1, S g1]
        aux = _aux(rs, act, S, E, 4, C)
        dWs = [_zeros(C, C) for _ in range(3)]
        served, dx = op.backward_power(_t(x0), _t(x), [_t(w) for w in W], _t(aux), act, True, dWs)
        assert served, "power backward not served"
        rdx, sdx, rdW, sdW = _bwd_ref(gk, ga, W, aux, act)
        _close(dx, rdx, sdx, 0.0, "backward_power C=%d %s dx" % (C, act))
        for k in range(3):
            _close(dWs[k], rdW[k], sdW[k], 0.0, "backward_power C=%d %s dW%d" % (C, act, k))


# ------------------------------------------------------------------------------------------------------------------
# the fused Bunch layer (terms kernels)
# ------------------------------------------------------------------------------------------------------------------

def _bunch_weights(rs):
    return [(0.2 * _rand(rs, 32, 32)).astype(np.float32) for _ in range(7)]


def test_terms_forward(cfg1):
    from scone_gcn_amd import ops
    sizes, fwd, _, dev = _bunch_env(cfg1)
    SRC, DST = ops.BUNCH_SRC, ops.BUNCH_DST
    rs = np.random.RandomState(6)
    xs, Wk = [_rand(rs, S, n, 4, 32) for n in sizes], _bunch_weights(rs)
    Ws = [[None] * 3 for _ in range(3)]
    for k in range(7):
        Ws[DST[k]][SRC[k]] = _t(Wk[k])
    z = [sum(_mm(_shift(dev[k], xs[SRC[k]].astype(np.float64)), Wk[k].astype(np.float64)) for k in range(7) if DST[k] == l)
         for l in range(3)]
    sc = [sum(_mm(_shift(abs(dev[k]), np.abs(xs[SRC[k]].astype(np.float64))), np.abs(Wk[k].astype(np.float64)))
              for k in range(7) if DST[k] == l) for l in range(3)]
    for act in ACT_NAMES:
        outs = fwd.forward([_t(x) for x in xs], Ws, act, [True] * 3)
        for l in range(3):
            _close(outs[l], ACTS[act](z[l]), sc[l], _fwd_abs(act), "terms forward level %d %s" % (l, act))


@pytest.mark.parametrize("first", [False, True])
def test_terms_backward(cfg1, first):
    """_terms_backward (input gradients written) and _terms_backward_first (contracted with the first layer's shifted input)."""
    from scone_gcn_amd import ops
    sizes, _, bwd, dev = _bunch_env(cfg1)
    SRC, DST = ops.BUNCH_SRC, ops.BUNCH_DST
    rs = np.random.RandomState(7)
    dzs, Wk = [_rand(rs, S, n, 4, 32) for n in sizes], _bunch_weights(rs)
    ys = [_rand(rs, S, n, 4, 1) for n in sizes]
    gk = {k: _shift(dev[k].T.tocsr(), dzs[DST[k]].astype(np.float64)) for k in range(7)}
    ga = {k: _shift(abs(dev[k]).T.tocsr(), np.abs(dzs[DST[k]].astype(np.float64))) for k in range(7)}
    for act in ACT_NAMES:
        auxs = [_aux(rs, act, S, n, 4, 32) for n in sizes]
        Wb = [[None] * 3 for _ in range(3)]
        dWb = [[None] * 3 for _ in range(3)]
        for k in range(7):
            Wb[SRC[k]][DST[k]], dWb[SRC[k]][DST[k]] = _t(Wk[k]), _zeros(32, 32)
        args = ([_t(d) for d in dzs], Wb, [_t(a) for a in auxs], act)
        what = "terms backward%s %s" % (" first" if first else "", act)
        if first:
            dWf = [_zeros(1, 32) for _ in range(3)]
            ops._terms_backward_first(bwd, *args, [_t(y) for y in ys], dWb, dWf)
        else:
            dxs = ops._terms_backward(bwd, *args, [True] * 3, dWb)
        for a in range(3):
            ks = [k for k in range(7) if SRC[k] == a]
            rdx, sdx, rdW, sdW = _bwd_ref([gk[k] for k in ks], [ga[k] for k in ks], [Wk[k] for k in ks], auxs[a], act)
            if first:
                y = ys[a].astype(np.float64)
                _close(dWf[a], np.einsum("srng,srnc->gc", y, rdx, optimize=False),
                       np.einsum("srng,srnc->gc", np.abs(y), sdx, optimize=False), 0.0, what + " dW_first level %d" % a)
            else:
                _close(dxs[a], rdx, sdx, 0.0, what + " dx level %d" % a)
            for i, k in enumerate(ks):
                _close(dWb[a][DST[k]], rdW[i], sdW[i], 0.0, what + " dW%d" % k)


# ------------------------------------------------------------------------------------------------------------------
# dense term kernels and the elementwise sum
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c_term,c", [(32, 32), (1, 16), (1, 32), (1, 64)])
def test_dense_terms_forward_and_backward(c_term, c):
    """three 32-wide terms: the MFMA kernels; three one-channel terms: the rank-one kernels at their three widths"""
    _need_gpu()
    from scone_gcn_amd import ops
    rs = np.random.RandomState(500 + c_term + c)
    R = 157
    Gs = [_rand(rs, S, R, 4, c_term) for _ in range(3)]
    Gd, Ga = [g.astype(np.float64) for g in Gs], [np.abs(g.astype(np.float64)) for g in Gs]
    W = _weights(rs, c_term, c)
    z = sum(_mm(g, w.astype(np.float64)) for g, w in zip(Gd, W))
    scale = sum(_mm(g, np.abs(w.astype(np.float64))) for g, w in zip(Ga, W))
    Wb = _weights(rs, c, c_term)                                                   # backward: W_k is (c_aux, c_k)
    for act in ACT_NAMES:
        what = "dense terms 3 x %d, width %d, %s" % (c_term, c, act)
        with ops.KernelTimer() as kt:
            out = ops.dense_terms_forward([_t(g) for g in Gs], [_t(w) for w in W], c, act)
            aux = _aux(rs, act, S, R, 4, c)
            dWs = [_zeros(c, c_term) for _ in range(3)]
            dx = ops.dense_terms_backward([_t(g) for g in Gs], [_t(w) for w in Wb], _t(aux), act, True, dWs)
        assert set(kt.summary()) == {"dense_fwd x3 ->%d" % c, "dense_bwd x3"}      # one launch each: no block decomposition
        _close(out, ACTS[act](z), scale, _fwd_abs(act), what + " forward")
        rdx, sdx, rdW, sdW = _bwd_ref(Gd, Ga, Wb, aux, act)
        _close(dx, rdx, sdx, 0.0, what + " dx")
        for k in range(3):
            _close(dWs[k], rdW[k], sdW[k], 0.0, what + " dW%d" % k)


def test_sum_act():
    _need_gpu()
    from scone_gcn_amd import ops
    rs = np.random.RandomState(8)
    terms = [_rand(rs, S, 157, 4, 32) for _ in range(3)]
    z = sum(t.astype(np.float64) for t in terms)
    scale = sum(np.abs(t.astype(np.float64)) for t in terms)
    for act in ACT_NAMES:
        out = torch.empty(S, 157, 4, 32, device="cuda")
        assert ops.sum_act([_t(t) for t in terms], act, out=out) is out
        _close(out, ACTS[act](z), scale, _fwd_abs(act), "sum_act %s" % act)


@pytest.mark.parametrize("act", [-1, 4, 7])
def test_sum_act_rejects_an_activation_code_out_of_range(act):
    """SCN_ERR_BAD_ARG straight from the entry point (every other argument valid), the output untouched."""
    _need_gpu()
    from scone_gcn_amd import _lib
    lib = _lib.load()
    t, out = torch.ones(64, device="cuda"), torch.full((64,), 5.0, device="cuda")
    st = lib.scn_sum_act(64, 1, _lib.ptr_array([t.data_ptr()]), act, ctypes.c_void_p(out.data_ptr()),
                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == _lib.SCN_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
