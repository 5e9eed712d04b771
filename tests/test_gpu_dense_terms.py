"""GPU tests of csrc/scn_dense.hip on its own: tile edges, grid caps, idle blocks, entry-point limits and non-finite data.

Every kernel of that file -- the generic VALU forward and backward, the fp32-MFMA pair, dense_fwd_out1, dense_fwd_in1, dense_bwd_g1,
dense_dw_reduce, sum_act, split_sign and the two folds -- is held against the fp64 references of tests/test_host_dense_terms.py with the
project's bar (tests/test_gpu_dispatch.py: _close; tests/test_gpu_nonfinite.py: _check): 8e-6 of each output's sum of |terms|, plus
1e-6 absolute where an activation is applied; weight gradients on their own sum of |terms| (their starting value included: the kernels
accumulate).  scn_split_sign, and scn_sum_act with none / relu over at most two terms, are compared bit for bit with float32 NumPy.
The dense-term calls go through ops.dense_terms_* on tensors [1, n_points, 1, c] (one trajectory per slab: no pairing of widths 16);
what the wrapper would reroute -- widths above 32, the LDS limit, the rejections -- goes to the C-ABI directly.
The sizes are the points at which the kernels change their path: one point, one short of / exactly / one past a tile of 32 and of 64
and a block of 128, and for every launch form one size past its grid cap, so that the grid-stride loop takes a full trip and part of
a second one (for the unrolled kernels: a later slot partly in range).  The caps below mirror scn_dense.hip.
Each message starts with the launch form; the worst error of a form is the largest fraction of the bar its lines print."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_dispatch import ACT_NAMES, _close, _fwd_abs
from tests.test_gpu_nonfinite import ACTS, _check, _need_gpu, _t
from tests.test_host_dense_terms import dense_terms_bwd_ref, dense_terms_ref, fold1_backward_ref, fold1_forward_ref, split_sign_ref

pytestmark = pytest.mark.gpu

# launch geometry of scn_dense.hip (each cap there carries a comment that points here)
THREADS = 256          # DN_THREADS, and the block of every streaming kernel
CAP_STREAM = 8192      # blocks: generic forward, out1, in1, sum_act
CAP_SPLIT = 4096       # blocks: split_sign
CAP_TILES = 2048       # blocks: generic backward (dense_blocks), MFMA forward and backward
CAP_G1 = 1024          # blocks: g1
DN_TILE = 64           # points per tile of the generic backward
DM_WAVES, DM_TILE = 4, 32   # waves per MFMA block, points per wave tile
IN1_U, G1_U = 4, 2     # items per thread and trip of in1 / g1

BAD_ARG, BAD_SHAPE, UNSUPPORTED, WORKSPACE = -1, -2, -4, -6        # include/scone_hip.h

EDGES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
ALL_ACTS_AT = (33, 129)                                            # every activation here, relu at the other sizes
CHUNK = 1 << 16                                                    # points per piece of an fp64 reference


def _rand(rng, *shape):
    """data of tests/test_gpu_dispatch.py's _rand kind (finite, no zeros, nothing below 1e-3 in magnitude), drawn in float32"""
    a = rng.standard_normal(shape, dtype=np.float32)
    return a + np.copysign(np.float32(1e-3), a)


def _aux(rng, act, *shape):
    a = _rand(rng, *shape)
    return np.tanh(a).astype(np.float32) if act == "tanh" else a


def _wts(rng, rows, cols):
    return (np.float32(0.3) * _rand(rng, rows, cols)).astype(np.float32)


def _slab(a):
    return _t(a).view(1, a.shape[0], 1, a.shape[1])


def _fwd_ref(Gs, Ws, act):
    parts = [dense_terms_ref([g[i:i + CHUNK] for g in Gs], Ws, act) for i in range(0, Gs[0].shape[0], CHUNK)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _bwd_ref(Gs, Ws, aux, act):
    parts = [dense_terms_bwd_ref([g[i:i + CHUNK] for g in Gs], Ws, aux[i:i + CHUNK], act) for i in range(0, aux.shape[0], CHUNK)]
    K = range(len(Gs))
    return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
            [sum(p[2][k] for p in parts) for k in K], [sum(p[3][k] for p in parts) for k in K])


def _hold(got, ref, scale, absolute, what):
    """_close; an output whose sum of |terms| is zero (a fold over weights of one sign) has to be exact"""
    got = got.detach().cpu().numpy().astype(np.float64)
    live = (scale > 0) | (absolute > 0)
    assert (got[~live] == ref[~live]).all(), "%s: an output without terms is not exact" % what
    _close(got[live], ref[live], scale[live], absolute, what)


# ------------------------------------------------------------------------------------------------------------------
# the calls
# ------------------------------------------------------------------------------------------------------------------

def _libs():
    from scone_gcn_amd import _lib
    return _lib, _lib.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptrs(ts):
    from scone_gcn_amd import _lib
    return _lib.ptr_array([t.data_ptr() for t in ts])


def _abi_forward(Gs, Ws, c_out, act, out):
    _lib, lib = _libs()
    return lib.scn_dense_terms_forward(Gs[0].shape[0], len(Gs), _ptrs(Gs), _lib.i32_array([g.shape[1] for g in Gs]), _ptrs(Ws), c_out,
                                       _lib.ACT[act], _p(out), _stream())


def _abi_workspace(n, cs, c_aux):
    _lib, lib = _libs()
    return int(lib.scn_dense_terms_backward_workspace(n, len(cs), _lib.i32_array(cs), c_aux))


def _abi_backward(Gs, Ws, aux, act, dx, dWs, ws, ws_bytes):
    _lib, lib = _libs()
    return lib.scn_dense_terms_backward(aux.shape[0], len(Gs), _ptrs(Gs), _lib.i32_array([g.shape[1] for g in Gs]), _ptrs(Ws), _p(aux),
                                        aux.shape[1], _lib.ACT[act], _p(dx), _ptrs(dWs), _p(ws), ws_bytes, _stream())


def _forward_case(form, rng, n, cs, c_out, act):
    from scone_gcn_amd import ops
    Gs = [_rand(rng, n, c) for c in cs]
    Ws = [_wts(rng, c, c_out) for c in cs]
    if sum(float(g[0].astype(np.float64) @ w[:, 0].astype(np.float64)) for g, w in zip(Gs, Ws)) < 0:
        Gs = [-g for g in Gs]                                       # point 0, channel 0 is positive: relu leaves something at n = 1
    what = "%s forward | %s -> %d, %d points, %s" % (form, cs, c_out, n, act)
    out = ops.dense_terms_forward([_slab(g) for g in Gs], [_t(w) for w in Ws], c_out, act)
    assert tuple(out.shape) == (1, n, 1, c_out), what
    ref, scale = _fwd_ref(Gs, Ws, act)
    _close(out.view(n, c_out), ref, scale, _fwd_abs(act), what)


def _backward_case(form, rng, n, cs, c_aux, act, need_dx, fold=False):
    """dW starts from non-zero tensors; fold: BunchPlan._fold_backward's call, the dW tensors passed as W too (W is not read for dW)"""
    from scone_gcn_amd import ops
    Gs = [_rand(rng, n, c) for c in cs]
    Ws = [_wts(rng, c_aux, c) for c in cs]
    aux = _aux(rng, act, n, c_aux)
    aux[0, 0] = abs(aux[0, 0])                                      # relu' leaves something at n = 1
    D0 = [_rand(rng, c_aux, c) for c in cs]
    dWs = [_t(d) for d in D0]
    what = "%s backward | %s, aux %d, %d points, %s%s" % (form, cs, c_aux, n, act, "" if need_dx else ", no dx")
    dx = ops.dense_terms_backward([_slab(g) for g in Gs], dWs if fold else [_t(w) for w in Ws], _slab(aux), act, need_dx, dWs)
    rdx, sdx, rdW, sdW = _bwd_ref(Gs, D0 if fold else Ws, aux, act)
    if need_dx:
        _close(dx.view(n, c_aux), rdx, sdx, 0.0, what + " dx")
    else:
        assert dx is None
    for k in range(len(cs)):
        _close(dWs[k], D0[k] + rdW[k], np.abs(D0[k].astype(np.float64)) + sdW[k], 0.0, what + " dW%d" % k)


def _acts(n):
    return ACT_NAMES if n in ALL_ACTS_AT else ("relu",)


# ------------------------------------------------------------------------------------------------------------------
# (a) tile edges, every launch form
# ------------------------------------------------------------------------------------------------------------------

FWD_FORMS = ([("generic", [5, 3], 7), ("generic", [3], 2), ("generic", [32, 16], 32)] +
             [("mfma", [32] * k, 32) for k in (1, 2, 3)] +
             [("out1", [c] * k, 1) for c in (16, 32) for k in (1, 2, 3)] +
             [("in1", [1] * k, c) for c in (16, 32, 64) for k in (1, 2, 6)] + [("in1", [1] * k, 32) for k in (3, 4, 5)])
BWD_FORMS = ([("generic", [5, 3], 5, True), ("generic", [3], 2, True), ("generic", [32, 16], 32, True)] +      # 32 x 32: the 4th dW slot
             [("mfma", [32] * k, 32, True) for k in (1, 2, 3)] + [("mfma", [32] * 3, 32, False)] +
             [("g1", [1] * k, c, dx) for c in (16, 32, 64) for k in (1, 3, 6) for dx in (True, False)])


def _id(f):
    return "%s-%s-%d%s" % (f[0], "x".join(map(str, f[1])), f[2], "" if len(f) < 4 or f[3] else "-nodx")


@pytest.mark.parametrize("form", FWD_FORMS, ids=_id)
def test_forward_at_tile_edges(form):
    _need_gpu()
    name, cs, c_out = form
    rng = np.random.default_rng(1000 + 7 * len(cs) + c_out + cs[0])
    for n in EDGES:
        for act in _acts(n):
            _forward_case(name, rng, n, cs, c_out, act)


@pytest.mark.parametrize("form", BWD_FORMS, ids=_id)
def test_backward_at_tile_edges(form):
    _need_gpu()
    name, cs, c_aux, need_dx = form
    rng = np.random.default_rng(2000 + 7 * len(cs) + c_aux + cs[0])
    for n in EDGES:
        for act in _acts(n):
            _backward_case(name, rng, n, cs, c_aux, act, need_dx)


def test_backward_as_the_fold_calls_it():
    """six one-channel terms, no activation, no dx, dW also in the place of W (BunchPlan._fold_backward)"""
    _need_gpu()
    rng = np.random.default_rng(77)
    for n in EDGES:
        _backward_case("g1", rng, n, [1] * 6, 32, "none", False, fold=True)


# ------------------------------------------------------------------------------------------------------------------
# (b) blocks without a tile still write their partial; the workspace is the size the query states
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [65, 128])
@pytest.mark.parametrize("form", [("mfma", [32] * 3, 32), ("g1", [1] * 3, 32), ("generic", [5, 3], 5)], ids=_id)
def test_backward_in_an_exact_workspace_of_ones_bits(form, n):
    """dense_blocks counts 64-point tiles, an MFMA block covers 128 points: at 65 .. 128 points block 1 has no tile and must write
    a zero partial.  The workspace holds 0xFF bytes (NaN) beforehand, with 64 guard words behind it."""
    _need_gpu()
    name, cs, c_aux = form
    rng = np.random.default_rng(300 + n + c_aux + cs[0])
    Gs, Ws, aux = [_rand(rng, n, c) for c in cs], [_wts(rng, c_aux, c) for c in cs], _aux(rng, "relu", n, c_aux)
    aux[0, 0] = abs(aux[0, 0])
    D0 = [_rand(rng, c_aux, c) for c in cs]
    dWs, dx = [_t(d) for d in D0], torch.empty(n, c_aux, device="cuda")
    nbytes = _abi_workspace(n, cs, c_aux)
    assert nbytes > 0 and nbytes % 4 == 0
    buf = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    st = _abi_backward([_t(g) for g in Gs], [_t(w) for w in Ws], _t(aux), "relu", dx, dWs, buf, nbytes)
    assert st == 0
    what = "%s backward | %s, aux %d, %d points, exact workspace" % (name, cs, c_aux, n)
    rdx, sdx, rdW, sdW = _bwd_ref(Gs, Ws, aux, "relu")
    _close(dx, rdx, sdx, 0.0, what + " dx")
    for k in range(len(cs)):
        _close(dWs[k], D0[k] + rdW[k], np.abs(D0[k].astype(np.float64)) + sdW[k], 0.0, what + " dW%d" % k)
    assert bool((buf[nbytes:] == 0xFF).all()), what + ": the words behind the workspace were written"


# ------------------------------------------------------------------------------------------------------------------
# (c) grid caps: one full trip of the grid-stride loop and part of a second
# ------------------------------------------------------------------------------------------------------------------

CAPS = [
    ("generic-forward", lambda rng: _forward_case("generic", rng, CAP_STREAM * THREADS // 2 + 37, [5, 3], 7, "relu")),   # 2 groups / point
    ("generic-backward", lambda rng: _backward_case("generic", rng, CAP_TILES * DN_TILE + 65, [5, 3], 5, "relu", True)),
    ("mfma-forward", lambda rng: _forward_case("mfma", rng, CAP_TILES * DM_WAVES * DM_TILE + 33, [32] * 3, 32, "relu")),
    ("mfma-backward", lambda rng: _backward_case("mfma", rng, CAP_TILES * DM_WAVES * DM_TILE + 33, [32] * 3, 32, "relu", True)),
    ("out1", lambda rng: _forward_case("out1", rng, CAP_STREAM * THREADS // 4 + 5, [16] * 3, 1, "relu")),               # 4 chunks / point
    # 16 channel groups per point; slot u = 1 partly in range, then the outer loop's second trip
    ("in1-slot", lambda rng: _forward_case("in1", rng, CAP_STREAM * THREADS // 16 + 37, [1] * 6, 64, "relu")),
    ("in1-trip", lambda rng: _forward_case("in1", rng, IN1_U * CAP_STREAM * THREADS // 16 + 37, [1] * 6, 64, "relu")),
    ("g1-slot", lambda rng: _backward_case("g1", rng, CAP_G1 * THREADS // 16 + 37, [1] * 6, 64, "relu", True)),
    ("g1-trip", lambda rng: _backward_case("g1", rng, G1_U * CAP_G1 * THREADS // 16 + 37, [1] * 6, 64, "relu", True)),
]


@pytest.mark.parametrize("case", CAPS, ids=[c[0] for c in CAPS])
def test_past_the_grid_cap(case):
    _need_gpu()
    case[1](np.random.default_rng(4000 + len(case[0])))


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float32)
    return a.view(np.uint32)


def _sum_f32(terms, act):
    """act(t0 + t1 + ...) in float32, term order, relu as the kernel has it (z <= 0 gives +0.0)"""
    v = terms[0].copy()
    for t in terms[1:]:
        v = v + t
    return np.where(v <= 0, np.float32(0.0), v).astype(np.float32) if act == "relu" else v


def test_sum_act_in_place_past_the_grid_cap():
    _need_gpu()
    from scone_gcn_amd import ops
    n = 4 * (CAP_STREAM * THREADS + 3)                              # 16 bytes per thread and trip
    rng = np.random.default_rng(41)
    terms = [_rand(rng, n), _rand(rng, n)]
    dev = [_t(t) for t in terms]
    assert ops.sum_act(dev, "relu") is dev[0]
    want = _sum_f32(terms, "relu")
    assert float(np.abs(want).max()) > 1e-3
    assert (_bits(dev[0]) == _bits(want)).all(), "sum_act | in place past the cap: %d words differ" % int((_bits(dev[0]) != _bits(want)).sum())
    assert (_bits(dev[1]) == _bits(terms[1])).all()


# ------------------------------------------------------------------------------------------------------------------
# (d) scn_sum_act
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n_terms", [1, 2, 4])
def test_sum_act_terms_and_placement(n_terms, in_place):
    _need_gpu()
    from scone_gcn_amd import ops
    n = 4 * (2 * THREADS + 3)
    rng = np.random.default_rng(50 + n_terms)
    for act in ACT_NAMES:
        terms = [_rand(rng, n) for _ in range(n_terms)]
        dev = [_t(t) for t in terms]
        out = dev[0] if in_place else torch.full((n,), 9.0, device="cuda")
        assert ops.sum_act(dev, act, out=None if in_place else out) is out
        what = "sum_act | %d terms, %s, %s" % (n_terms, act, "in place" if in_place else "out of place")
        for k in range(0 if not in_place else 1, n_terms):
            assert (_bits(dev[k]) == _bits(terms[k])).all(), what + ": an input term changed"
        if n_terms <= 2 and act in ("none", "relu"):
            want = _sum_f32(terms, act)
            assert float(np.abs(want).max()) > 1e-3
            assert (_bits(out) == _bits(want)).all(), what + ": not bit for bit"
        _close(out, ACTS[act](sum(t.astype(np.float64) for t in terms)), sum(np.abs(t.astype(np.float64)) for t in terms),
               _fwd_abs(act), what)


def test_sum_act_rejections():
    """the documented status, before any launch: the output keeps its fill value"""
    _need_gpu()
    _lib, lib = _libs()
    ts = [torch.ones(72, device="cuda") for _ in range(5)]
    out = torch.full((72,), 5.0, device="cuda")
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 4)              # 4 bytes off a 16-byte boundary
    call = lambda n, k, terms, o: lib.scn_sum_act(n, k, _lib.ptr_array([p if isinstance(p, int) else p.value for p in terms]),
                                                  _lib.ACT["relu"], o, _stream())
    base = [t.data_ptr() for t in ts]
    assert all(p % 16 == 0 for p in base) and out.data_ptr() % 16 == 0
    assert call(64, 2, base[:2], _p(out)) == 0                      # the same call, valid
    torch.cuda.synchronize()
    assert bool((out[:64] == 2.0).all()) and bool((out[64:] == 5.0).all())
    out.fill_(5.0)
    assert call(62, 2, base[:2], _p(out)) == BAD_SHAPE              # n % 4 != 0
    assert call(64, 0, base[:1], _p(out)) == BAD_SHAPE
    assert call(64, 5, base, _p(out)) == BAD_SHAPE
    assert call(64, 2, [base[0], off(ts[1])], _p(out)) == BAD_ARG
    assert call(64, 2, base[:2], off(out)) == BAD_ARG
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())


# ------------------------------------------------------------------------------------------------------------------
# (e) scn_split_sign
# ------------------------------------------------------------------------------------------------------------------

def _specials():
    big = np.finfo(np.float32).max
    nan = np.array([0x7FC00000, 0xFFC00001, 0x7FC00123], np.uint32).view(np.float32)      # quiet NaNs, two with a payload
    return np.concatenate([np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, big, -big, np.inf, -np.inf], np.float32), nan])


def _split_sign(v):
    _, lib = _libs()
    g = _t(v)
    gp, gm = torch.full_like(g, 7.0), torch.full_like(g, 7.0)
    assert lib.scn_split_sign(g.numel(), _p(g), _p(gp), _p(gm), _stream()) == 0
    torch.cuda.synchronize()
    rp, rm = split_sign_ref(v)
    assert (_bits(gp) == _bits(rp)).all() and (_bits(gm) == _bits(rm)).all(), "split_sign | %d values: not bit for bit" % v.size
    with np.errstate(invalid="ignore"):
        body = np.isfinite(v) & (v != 0)
    vb, pb, mb = _bits(v)[body], _bits(gp)[body], _bits(gm)[body]   # finite and non-zero: one part is the value, the other +0.0
    assert (((pb == vb) & (mb == 0)) | ((mb == vb) & (pb == 0))).all()
    assert (_bits(g) == _bits(v)).all()


@pytest.mark.parametrize("n", [1, 255, 256, 257, CAP_SPLIT * THREADS + 3])
def test_split_sign_bit_for_bit(n):
    _need_gpu()
    rng = np.random.default_rng(60 + n % 1000)
    sp = _specials()
    if n == 1:
        for x in list(sp) + [np.float32(1.5), np.float32(-2.5)]:
            _split_sign(np.array([x], np.float32))
        return
    v = _rand(rng, n)
    at = rng.choice(n - 2, 4 * len(sp), replace=False) + 1
    v[at] = np.tile(sp, 4)
    v[0], v[-1] = sp[1], sp[-1]                                     # -0.0 first, a NaN last
    assert float(np.nanmax(np.abs(v[np.isfinite(v)]))) > 1e-3
    _split_sign(v)


# ------------------------------------------------------------------------------------------------------------------
# (f) the folds: one workgroup, a thread per channel, += into dW2 and dw1
# ------------------------------------------------------------------------------------------------------------------

FOLD_C = (1, 7, 32, 63, 64, 65)


def _fold_w1(rng, c1):
    """positive, negative and exactly zero entries (c1 = 1: a positive one)"""
    w1 = _wts(rng, 1, c1)[0]
    w1[2::3] = 0.0
    if c1 >= 2:
        w1[0], w1[1] = abs(w1[0]), -abs(w1[1])
    else:
        w1[0] = abs(w1[0])
    return w1


def _fold_forward(w1, W2, fill=3.0):
    _, lib = _libs()
    c1, c2 = W2.shape
    ap, am = torch.full((c2,), fill, device="cuda"), torch.full((c2,), fill, device="cuda")
    a1, a2 = _t(w1), _t(W2)                                        # (named: they live until the synchronize below)
    st = lib.scn_fold1_forward(_p(a1), _p(a2), c1, c2, _p(ap), _p(am), _stream())
    torch.cuda.synchronize()
    return st, ap, am


def _fold_backward(w1, W2, up, um, D2, d1):
    _, lib = _libs()
    c1, c2 = W2.shape
    dW2, dw1 = _t(D2), _t(d1)
    ins = [_t(a) for a in (w1, W2, up, um)]                        # (named: they live until the synchronize below)
    st = lib.scn_fold1_backward(*[_p(t) for t in ins], c1, c2, _p(dW2), _p(dw1), _stream())
    torch.cuda.synchronize()
    return st, dW2, dw1


def _fold_pair(rng, c1, c2):
    w1, W2 = _fold_w1(rng, c1), _wts(rng, c1, c2)
    what = "fold1 | %d x %d" % (c1, c2)
    st, ap, am = _fold_forward(w1, W2)
    assert st == 0
    (Ap, Am), (sp, sm) = fold1_forward_ref(w1, W2)
    _hold(torch.cat([ap, am]), np.concatenate([Ap, Am]), np.concatenate([sp, sm]), 0.0, what + " Ap|Am")
    up, um, D2, d1 = _rand(rng, c2), _rand(rng, c2), _rand(rng, c1, c2), _rand(rng, c1)
    st, dW2, dw1 = _fold_backward(w1, W2, up, um, D2, d1)
    assert st == 0
    (rW2, rw1), (sW2, sw1) = fold1_backward_ref(w1, W2, up, um)
    _close(dW2, D2 + rW2, np.abs(D2.astype(np.float64)) + sW2, 0.0, what + " dW2")
    _close(dw1, d1 + rw1, np.abs(d1.astype(np.float64)) + sw1, 0.0, what + " dw1")
    zero = w1 == 0                                                  # relu'(0) = 0: a zero weight's row and entry keep their values
    assert (_bits(dW2)[zero] == _bits(D2)[zero]).all() and (_bits(dw1)[zero] == _bits(d1)[zero]).all(), what


@pytest.mark.parametrize("c1", FOLD_C)
def test_folds_at_wave_edges(c1):
    _need_gpu()
    rng = np.random.default_rng(700 + c1)
    for c2 in FOLD_C:
        _fold_pair(rng, c1, c2)


def test_folds_at_the_thread_limit():
    _need_gpu()
    rng = np.random.default_rng(701)
    w1, W2 = _fold_w1(rng, 32), _wts(rng, 32, 1024)
    st, ap, am = _fold_forward(w1, W2)
    assert st == 0
    (Ap, Am), (sp, sm) = fold1_forward_ref(w1, W2)
    _close(torch.cat([ap, am]), np.concatenate([Ap, Am]), np.concatenate([sp, sm]), 0.0, "fold1 | 32 x 1024 Ap|Am")
    w1, W2 = _fold_w1(rng, 1024), _wts(rng, 1024, 32)
    up, um, D2, d1 = _rand(rng, 32), _rand(rng, 32), _rand(rng, 1024, 32), _rand(rng, 1024)
    st, dW2, dw1 = _fold_backward(w1, W2, up, um, D2, d1)
    assert st == 0
    (rW2, rw1), (sW2, sw1) = fold1_backward_ref(w1, W2, up, um)
    _close(dW2, D2 + rW2, np.abs(D2.astype(np.float64)) + sW2, 0.0, "fold1 | 1024 x 32 dW2")
    _close(dw1, d1 + rw1, np.abs(d1.astype(np.float64)) + sw1, 0.0, "fold1 | 1024 x 32 dw1")


def test_fold_rejections():
    _need_gpu()
    _, lib = _libs()
    rng = np.random.default_rng(702)
    st, ap, am = _fold_forward(_fold_w1(rng, 4), _wts(rng, 4, 1025))
    assert st == BAD_SHAPE and bool((ap == 3.0).all()) and bool((am == 3.0).all())
    D2, d1 = _rand(rng, 1025, 4), _rand(rng, 1025)
    st, dW2, dw1 = _fold_backward(_fold_w1(rng, 1025), _wts(rng, 1025, 4), _rand(rng, 4), _rand(rng, 4), D2, d1)
    assert st == BAD_SHAPE and (_bits(dW2) == _bits(D2)).all() and (_bits(dw1) == _bits(d1)).all()
    w1, W2 = _t(_fold_w1(rng, 4)), _t(_wts(rng, 4, 8))             # c1 = 0 with valid pointers
    ap, am = torch.full((8,), 3.0, device="cuda"), torch.full((8,), 3.0, device="cuda")
    assert lib.scn_fold1_forward(_p(w1), _p(W2), 0, 8, _p(ap), _p(am), _stream()) == BAD_SHAPE
    dW2, dw1, u = torch.full((4, 8), 3.0, device="cuda"), torch.full((4,), 3.0, device="cuda"), torch.ones(8, device="cuda")
    assert lib.scn_fold1_backward(_p(w1), _p(W2), _p(u), _p(u), 0, 8, _p(dW2), _p(dw1), _stream()) == BAD_SHAPE
    torch.cuda.synchronize()
    assert all(bool((t == 3.0).all()) for t in (ap, am, dW2, dw1))


# ------------------------------------------------------------------------------------------------------------------
# (g) entry-point limits of scn_dense_terms_*
# ------------------------------------------------------------------------------------------------------------------

def test_forward_with_exactly_64_kb_of_weights():
    _need_gpu()
    rng = np.random.default_rng(800)
    n, cs, c_out = 257, [128, 128], 64
    assert 4 * c_out * sum(cs) == 64 * 1024
    Gs, Ws = [_rand(rng, n, c) for c in cs], [_wts(rng, c, c_out) for c in cs]
    out = torch.full((n, c_out), 7.0, device="cuda")
    assert _abi_forward([_t(g) for g in Gs], [_t(w) for w in Ws], c_out, "relu", out) == 0
    ref, scale = _fwd_ref(Gs, Ws, "relu")
    _close(out, ref, scale, _fwd_abs("relu"), "generic forward | %s -> %d at the LDS limit, %d points" % (cs, c_out, n))


def test_dense_terms_rejections():
    """every status comes back before a launch: the outputs keep their fill value"""
    _need_gpu()
    n = 40
    ones = lambda *s: torch.ones(*s, device="cuda")
    fill = lambda *s: torch.full(s, 7.0, device="cuda")
    kept = lambda *ts: all(bool((t == 7.0).all()) for t in ts)

    out = fill(n, 48)                                               # 72 KB of weights
    assert _abi_forward([ones(n, 128)] * 3, [ones(128, 48)] * 3, 48, "relu", out) == UNSUPPORTED
    out4 = fill(n, 32)                                              # four terms, one of them two channels wide
    cs4 = [1, 1, 2, 1]
    assert _abi_forward([ones(n, c) for c in cs4], [ones(c, 32) for c in cs4], 32, "relu", out4) == BAD_SHAPE

    def backward(cs, c_aux, short=0):
        nbytes = _abi_workspace(n, cs, c_aux)
        assert nbytes > 0
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        dx, dWs = fill(n, c_aux), [fill(c_aux, c) for c in cs]
        st = _abi_backward([ones(n, c) for c in cs], [ones(c_aux, c) for c in cs], ones(n, c_aux), "relu", dx, dWs, ws, nbytes - short)
        torch.cuda.synchronize()
        return st, kept(dx, *dWs)

    assert backward([32], 33) == (UNSUPPORTED, True)                # c_aux * c_k = 1056 > 1024
    assert backward([32], 32, short=1) == (WORKSPACE, True)
    assert backward([1] * 3, 32, short=1) == (WORKSPACE, True)
    assert backward(cs4, 32) == (BAD_SHAPE, True)
    torch.cuda.synchronize()
    assert kept(out, out4)


# ------------------------------------------------------------------------------------------------------------------
# (h) non-finite data: the three rules of tests/test_gpu_nonfinite.py
# ------------------------------------------------------------------------------------------------------------------

NF_POINTS = 32 * 9 + 1                                              # a one-point tail: clamp lanes and fallbacks re-read the last point
NF_FWD = [("generic", [5, 3], 7), ("mfma", [32] * 3, 32), ("out1", [16] * 3, 1), ("out1", [32] * 3, 1), ("in1", [1] * 6, 32)]
NF_BWD = [("generic", [5, 3], 5), ("mfma", [32] * 3, 32), ("g1", [1] * 3, 32)]


def _check_points(got, ref, scale, bad, absolute, what):
    """points are independent: rule (2) per point (bad: [points] bool, points with a non-finite input)"""
    n, c = ref.shape
    got = got.detach().cpu().numpy().astype(np.float64).reshape(n, 1, 1, c)
    _check(got, ref.reshape(n, 1, 1, c), scale.reshape(n, 1, 1, c), bad.reshape(n, 1), absolute, what)


def _check_entries(got, ref, scale, what):
    """a weight gradient: rule (2) per entry -- what the reference keeps finite is finite"""
    r, c = ref.shape
    got = got.detach().cpu().numpy().astype(np.float64).reshape(r, 1, c, 1)
    _check(got, ref.reshape(r, 1, c, 1), scale.reshape(r, 1, c, 1), ~np.isfinite(ref), 0.0, what)
    fin = np.isfinite(ref)
    assert not fin.any() or float(np.abs(ref[fin]).max()) > 1e-3, what + ": the finite part of the reference is trivially small"


def _place(Gs):
    """+Inf in G_0 at point 0, -Inf in the last term at a middle point, NaN at the last point; returns the bad points"""
    n = Gs[0].shape[0]
    Gs[0][0, 0] = np.inf
    Gs[-1][n // 2, -1] = -np.inf
    Gs[0][n - 1, Gs[0].shape[1] // 2] = np.nan
    bad = np.zeros(n, bool)
    bad[[0, n // 2, n - 1]] = True
    return bad


@pytest.mark.parametrize("form", NF_FWD, ids=_id)
def test_forward_with_nonfinite_points(form):
    _need_gpu()
    from scone_gcn_amd import ops
    name, cs, c_out = form
    n = NF_POINTS
    rng = np.random.default_rng(900 + c_out + cs[0])
    Gs, Ws = [_rand(rng, n, c) for c in cs], [_wts(rng, c, c_out) for c in cs]
    bad = _place(Gs)
    for act in ACT_NAMES:
        what = "%s forward | %s -> %d, non-finite points, %s" % (name, cs, c_out, act)
        out = ops.dense_terms_forward([_slab(g) for g in Gs], [_t(w) for w in Ws], c_out, act)
        ref, scale = _fwd_ref(Gs, Ws, act)
        assert np.isfinite(ref[~bad]).all() and float(np.abs(ref[~bad]).max()) > 1e-3
        if act == "none":
            assert all((~np.isfinite(ref[p])).any() for p in (0, n // 2, n - 1)), what + ": the reference is finite"
        _check_points(out.view(n, c_out), ref, scale, bad, _fwd_abs(act), what)


@pytest.mark.parametrize("form", NF_FWD, ids=_id)
def test_forward_with_a_nan_weight_on_zero_input(form):
    """0 * NaN is NaN down the weight's whole column and nowhere else"""
    _need_gpu()
    from scone_gcn_amd import ops
    name, cs, c_out = form
    n = NF_POINTS
    rng = np.random.default_rng(950 + c_out + cs[0])
    Gs, Ws = [np.zeros((n, c), np.float32) for c in cs], [_wts(rng, c, c_out) for c in cs]
    col = c_out // 2
    Ws[-1][min(1, cs[-1] - 1), col] = np.nan
    for act in ACT_NAMES:
        what = "%s forward | %s -> %d, NaN weight, %s" % (name, cs, c_out, act)
        got = ops.dense_terms_forward([_slab(g) for g in Gs], [_t(w) for w in Ws], c_out, act).view(n, c_out).cpu().numpy()
        ref, _ = _fwd_ref(Gs, Ws, act)
        assert np.isnan(ref[:, col]).all() and (np.delete(ref, col, axis=1) == 0).all()
        assert np.isnan(got[:, col]).all(), what + ": %d outputs of the column are not NaN" % int((~np.isnan(got[:, col])).sum())
        assert (np.delete(got, col, axis=1) == 0).all(), what + ": the NaN left its column"


@pytest.mark.parametrize("case", ["terms", "aux"])
@pytest.mark.parametrize("form", NF_BWD, ids=_id)
def test_backward_with_nonfinite_points(form, case):
    """terms: +Inf / -Inf / NaN in the gathered gradients; aux: one NaN in channel ca0 of aux at one point -- row ca0 of every dW_k
    is NaN, every other row stays finite and inside the bar"""
    _need_gpu()
    from scone_gcn_amd import ops
    name, cs, c_aux = form
    n = NF_POINTS
    rng = np.random.default_rng(970 + c_aux + cs[0])
    Gs, Ws = [_rand(rng, n, c) for c in cs], [_wts(rng, c_aux, c) for c in cs]
    ca0, pt = c_aux // 2, n - 1
    for act in ACT_NAMES:
        what = "%s backward | %s, aux %d, non-finite %s, %s" % (name, cs, c_aux, case, act)
        G = [g.copy() for g in Gs]
        aux = _aux(rng, act, n, c_aux)
        if case == "terms":
            bad = _place(G)
        else:
            aux[pt, ca0] = np.nan
            bad = np.zeros(n, bool)
            bad[pt] = True
        D0 = [_rand(rng, c_aux, c) for c in cs]
        dWs = [_t(d) for d in D0]
        dx = ops.dense_terms_backward([_slab(g) for g in G], [_t(w) for w in Ws], _slab(aux), act, True, dWs)
        rdx, sdx, rdW, sdW = _bwd_ref(G, Ws, aux, act)
        assert np.isfinite(rdx[~bad]).all() and float(np.abs(rdx[~bad]).max()) > 1e-3
        if case == "terms":
            if act == "none":
                assert all((~np.isfinite(rdx[p])).any() for p in (0, n // 2, n - 1)), what + ": the reference dx is finite"
            assert not np.isfinite(rdW[0]).all() and not np.isfinite(rdW[-1]).all(), what + ": the reference dW is finite"
        else:
            assert all(np.isnan(r[ca0]).all() and np.isfinite(np.delete(r, ca0, axis=0)).all() for r in rdW), what
        assert any(np.isfinite(r).any() for r in rdW), what + ": no finite weight gradient left to compare"
        _check_points(dx.view(n, c_aux), rdx, sdx, bad, 0.0, what + " dx")
        for k in range(len(cs)):
            _check_entries(dWs[k], D0[k] + rdW[k], np.abs(D0[k].astype(np.float64)) + sdW[k], what + " dW%d" % k)


def test_folds_with_a_nan_weight():
    _need_gpu()
    rng = np.random.default_rng(990)
    c1, c2, a = 33, 65, 5
    w1, W2 = _fold_w1(rng, c1), _wts(rng, c1, c2)
    w1[a] = np.nan
    st, ap, am = _fold_forward(w1, W2)
    (Ap, Am), _ = fold1_forward_ref(w1, W2)
    assert st == 0 and np.isnan(Ap).all() and np.isnan(Am).all()
    assert bool(torch.isnan(ap).all()) and bool(torch.isnan(am).all()), "fold1 | a NaN weight did not reach every Ap, Am"
    up, um, D2, d1 = _rand(rng, c2), _rand(rng, c2), _rand(rng, c1, c2), _rand(rng, c1)
    st, dW2, dw1 = _fold_backward(w1, W2, up, um, D2, d1)
    (rW2, rw1), (sW2, sw1) = fold1_backward_ref(w1, W2, up, um)
    assert st == 0 and np.isnan(rW2[a]).all() and np.isfinite(np.delete(rW2, a, axis=0)).all() and np.isfinite(rw1).all()
    _check_entries(dW2, D2 + rW2, np.abs(D2.astype(np.float64)) + sW2, "fold1 | NaN weight dW2")
    _close(dw1, d1 + rw1, np.abs(d1.astype(np.float64)) + sw1, 0.0, "fold1 | NaN weight dw1")
