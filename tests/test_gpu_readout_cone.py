"""GPU tests of the layers below the top running on the readout's cone (DESIGN.md sections 3 and 7, ops.READOUT_CONE).

The readout reads H_L on the items M0 of the keep mask; nothing reads H_l outside M_{L-l} = hop^{L-l}(M0) and dZ_l is zero outside it.
Three native pieces serve that and are tested here directly, BIT FOR BIT (int32 views) against the plain entry points on buffers
pre-filled with a NaN pattern no kernel produces:
  * scn_conv_shifted_input_keep: y on the kept items, every other row untouched;
  * scn_conv_backward_visit / scn_conv_backward_fused_first_from_y_visit: only the items of V = hop(M) are visited, dz being zero outside
    M -- dx on V and the weight gradients (accumulated into non-zero values) are the plain call's, every other row of dx untouched,
    and aux / y outside V and dz no item of V stages may hold NaN;
  * scn_clear_mask: +0 on the listed items, nothing else.
Then plan steps with the switch on against off (loss and every weight gradient bit for bit, three and four layers; against the fp64
oracle to the suite's 1e-5 of max(1, |reference|)), the pooled gradient buffers all-zero afterwards, two batches through one plan, and
the shapes the path refuses.

Shapes: the complex of tests/golden/cfg1_complex.npz (|E| = 1001: 17 plan blocks or so, the last one short) and tiny4_complex.npz (one
block); 5 slabs (one mask word), 64 (two words, a full window) and 130 (five words, several slab ranges of the launch grid, bits
only above slab 64); tanh and relu.  The three size thresholds of the plan are set to 0 the way tests/test_gpu_keep_last.py does.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import scone_oracle as so
from tests.test_gpu_keep_last import SENTINEL, _assert_equal_steps, _expected, _need_gpu, _pack, _same_bits, _sentinel
from tests.test_gpu_top_dz_mask import _rows, _unpack

pytestmark = pytest.mark.gpu
TOL = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_ENVS = {}


def _env(name="cfg1"):
    """The complex of a golden file, its scone plans by activation (built on demand), block starts and block adjacency."""
    if name not in _ENVS:
        from scone_gcn_amd import ops, synthetic_data_gen as g, trajectory_experiments as te
        from scone_gcn_amd.complex import SimplicialComplex
        d = np.load(os.path.join(GOLDEN, name + "_complex.npz"))
        if name == "cfg1":
            cx = g.Complex(n_nodes=int(d["n_nodes"]), edges=d["edges"].astype(np.int64), faces=d["faces"].astype(np.int64),
                           coords=d["coords"], valid_idxs=d["valid_idxs"].astype(np.int64))
        else:
            cx = g.Complex(n_nodes=int(d["edges"].max()) + 1, edges=d["edges"].astype(np.int64), faces=d["faces"].astype(np.int64))
        sc = SimplicialComplex(cx)
        env = dict(cx=cx, sc=sc, te=te, plans={})

        def plan(act="tanh", fresh=False):
            if fresh or act not in env["plans"]:
                shifts, readout, _ = te.setup_from_complex(sc, "scone")
                p = ops.SconePlan(shifts[0], shifts[1], readout, act, ops.default_device())
                if fresh:
                    return p
                env["plans"][act] = p
            return env["plans"][act]

        env["plan"] = plan
        p = plan()
        assert p.conv_T is p.conv
        tabs = p.field_tables_dev()
        env["row0"] = np.asarray(p.conv.plan_blocks(), np.int64)
        assert tabs is not None and tabs.n_blocks == len(env["row0"]) - 1
        env["tabs"] = tabs
        env["adj"] = (tabs.adj_ptr.cpu().numpy()[:tabs.n_blocks + 1], tabs.adj_blk.cpu().numpy()[:-1])   # (without the upload's pad word)
        env["nb"], env["E"] = tabs.n_blocks, cx.n_edges
        _ENVS[name] = env
    return _ENVS[name]


PATTERNS = ["empty", "all", "first", "last", "runs", "ends_empty", "random", "high"]


def _mask(name, nb, S, rs):
    """bool [nb][S]: a set of (block, slab) items."""
    k = np.zeros((nb, S), bool)
    if name == "all":
        k[:] = True
    elif name == "first":                    # the first slab of block 0
        k[0, 0] = True
    elif name == "last":                     # the last slab of the short last block
        k[nb - 1, S - 1] = True
    elif name == "runs":                     # runs of slabs in every third block, the blocks between them empty
        k[0::3, 1:3] = True
        k[0::3, S // 2:S // 2 + 3] = True
    elif name == "ends_empty":               # the first and the last block empty
        k[1:nb - 1] = rs.rand(max(nb - 2, 0), S) < 0.3
    elif name == "random":
        k[:] = rs.rand(nb, S) < 0.1
    elif name == "high":                     # bits only from slab 64 on (130 slabs); fewer slabs: the upper half
        k[:, min(64, S // 2):] = rs.rand(nb, S - min(64, S // 2)) < 0.2
    else:
        assert name == "empty"
    return k


def _hop(env, k):
    from scone_gcn_amd import ops
    return _unpack(ops.mask_hop_host(_pack(k).cpu().numpy().view(np.uint32), *env["adj"]), k.shape[1])


def _staged(env, v):
    """The dz items (b', s) some item (b, s) of v stages: b' in A(b)."""
    adj_ptr, adj_blk = env["adj"]
    st = np.zeros_like(v)
    for b in range(v.shape[0]):
        st[adj_blk[adj_ptr[b]:adj_ptr[b + 1]]] |= v[b]
    return st


def _randn(rs, *shape):
    return torch.as_tensor(rs.randn(*shape).astype(np.float32), device="cuda")


def _weights(rs, c_in=32):
    return [torch.as_tensor((0.3 * rs.randn(c_in, 32)).astype(np.float32), device="cuda") for _ in range(3)]


def _nan_where(rows, t):
    return torch.where(rows[:, :, None, None], torch.full((), float("nan"), device="cuda"), t)


SHAPES = [("tanh", 5), ("relu", 5), ("tanh", 64), ("tanh", 130), ("relu", 130)]


# ------------------------------------------------------------------------------------------------------------------
# y on the kept items
# ------------------------------------------------------------------------------------------------------------------

def _kept_y(env, x, keep, out):
    from scone_gcn_amd import _lib, ops
    op = env["plan"]().conv
    st = _lib.load().scn_conv_shifted_input_keep(op.handle, x.shape[0], 4, ops._dev(x), ops._dev(out), ops._dev(keep, torch.int32),
                                                 ops._stream())
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("S", [5, 64, 130])
def test_kept_y_holds_the_plain_records_on_the_kept_items_and_nothing_else(S):
    _need_gpu()
    from scone_gcn_amd import _lib
    env = _env()
    rs = np.random.RandomState(S)
    x = _randn(rs, S, env["E"], 4, 1)
    full = env["plan"]().conv.shifted_input(x)
    assert full is not None
    for pattern in PATTERNS:
        k = _mask(pattern, env["nb"], S, rs)
        out = _sentinel(full.shape)
        _lib.check(_kept_y(env, x, _pack(k), out), "scn_conv_shifted_input_keep")
        _same_bits(out.view(torch.int32), _expected(full, k, env["row0"]), "y, %d slabs, mask %s" % (S, pattern))
    # the plan's own call
    k = _mask("random", env["nb"], S, rs)
    got = env["plan"]().conv.shifted_input(x, keep=_pack(k))
    rows = _rows(k, env["row0"])[:, :, None, None].expand_as(full)
    assert got is not None and torch.equal(got.view(torch.int32)[rows], full.view(torch.int32)[rows])


# ------------------------------------------------------------------------------------------------------------------
# the visiting backward, plain form
# ------------------------------------------------------------------------------------------------------------------

def _bwd_case(env, act, S, pattern, rs):
    """dz zero outside the rows of M (random on them), V = hop(M), and the plain backward's dx and weight gradients."""
    plan = env["plan"](act)
    m = _mask(pattern, env["nb"], S, rs)
    v = _hop(env, m)
    assert not (m & ~v).any()
    dz = _randn(rs, S, env["E"], 4, 32) * _rows(m, env["row0"])[:, :, None, None]
    h = rs.randn(S, env["E"], 4, 32).astype(np.float32)
    aux = torch.as_tensor(np.tanh(h) if act == "tanh" else np.maximum(h, 0), device="cuda")
    W = _weights(rs)
    dW0 = [_randn(rs, 32, 32) for _ in range(3)]
    dW = [t.clone() for t in dW0]
    dx = plan.conv_T.backward([dz], W, aux, act, True, dW)
    torch.cuda.synchronize()
    return dict(plan=plan, m=m, v=v, dz=dz, aux=aux, W=W, dW0=dW0, dW=dW, dx=dx, mask=_pack(v))


def _visit(c, act, dz=None, aux=None, need_dx=True, W=None):
    dW = [t.clone() for t in c["dW0"]]
    out = _sentinel(c["dx"].shape) if need_dx else None
    dx = c["plan"].conv_T.backward([c["dz"] if dz is None else dz], c["W"] if W is None else W, c["aux"] if aux is None else aux, act,
                                   need_dx, dW, dx=out, visit=c["mask"])
    assert dx is not False, "visiting backward not served"
    torch.cuda.synchronize()
    return dx, dW


@pytest.mark.parametrize("act,S", SHAPES)
def test_visiting_backward_equals_the_plain_backward_on_the_visited_items(act, S):
    """Clean tensors first; then NaN over every aux item outside V and every dz item no item of V stages: the same bits again."""
    _need_gpu()
    env = _env()
    rs = np.random.RandomState(100 * S + (act == "relu"))
    for pattern in PATTERNS:
        c = _bwd_case(env, act, S, pattern, rs)
        what = "%s, %d slabs, M %s" % (act, S, pattern)
        assert pattern == "empty" or float(c["dx"].abs().max()) > 0
        want = _expected(c["dx"], c["v"], env["row0"])
        aux_p = _nan_where(_rows(~c["v"], env["row0"]), c["aux"])
        dz_p = _nan_where(_rows(~_staged(env, c["v"]), env["row0"]), c["dz"])
        assert pattern == "all" or (bool(torch.isnan(aux_p).any()) and bool(torch.isnan(dz_p).any()))
        for tag, kw in (("", {}), (" with poisoned tensors", dict(dz=dz_p, aux=aux_p))):
            dx, dW = _visit(c, act, **kw)
            _same_bits(dx.view(torch.int32), want, "dx" + tag + ", " + what)
            for g in range(3):
                _same_bits(dW[g], c["dW"][g], "dW[%d]%s, %s" % (g, tag, what))
        if pattern == "random":                                             # dx = NULL: the weight gradients alone
            none, dW = _visit(c, act, need_dx=False)
            assert none is None
            for g in range(3):
                _same_bits(dW[g], c["dW"][g], "dW[%d], dx = NULL, %s" % (g, what))


def test_visiting_backward_on_a_single_block():
    """tiny4: one plan block of five rows -- the window is one bit per slab and hop(M) = M."""
    _need_gpu()
    env = _env("tiny4")
    assert env["nb"] == 1
    rs = np.random.RandomState(4)
    for pattern in ("empty", "all", "first", "random"):
        c = _bwd_case(env, "tanh", 5, pattern, rs)
        assert np.array_equal(c["v"], c["m"])
        dx, dW = _visit(c, "tanh")
        _same_bits(dx.view(torch.int32), _expected(c["dx"], c["v"], env["row0"]), "dx, tiny4, M " + pattern)
        for g in range(3):
            _same_bits(dW[g], c["dW"][g], "dW[%d], tiny4, M %s" % (g, pattern))


def _untouched(*tensors):
    return all(bool((t.view(torch.int32) == SENTINEL).all()) for t in tensors)


def test_unserved_shapes_are_refused_before_any_launch():
    """C = 16 (the slab-pair form has no visit mask), two groups, and a slab count that leaves a workgroup of every launch grid more
    than 64 slabs: SCN_ERR_UNSUPPORTED with dx, y and the weight gradients untouched; no mask at all is a bad argument."""
    _need_gpu()
    from scone_gcn_amd import _lib, ops
    env = _env()
    plan, nb, E = env["plan"](), env["nb"], env["E"]
    rs = np.random.RandomState(0)
    S = 4
    ones = _pack(np.ones((nb, S), bool))
    t16 = _randn(rs, S, E, 4, 16)
    W16 = [torch.as_tensor((0.3 * rs.randn(16, 16)).astype(np.float32), device="cuda") for _ in range(3)]
    dW, dx = [_sentinel((16, 16)) for _ in range(3)], _sentinel(t16.shape)
    assert plan.conv_T.backward([t16], W16, t16, "tanh", True, dW, dx=dx, visit=ones) is False
    y = _randn(rs, S, E, 4, 4)
    dWf = [_sentinel((1, 16)) for _ in range(3)]
    W16f = [torch.as_tensor((0.3 * rs.randn(1, 16)).astype(np.float32), device="cuda") for _ in range(3)]
    assert plan.conv_T.backward_fused_first(t16, W16, None, "tanh", y, dW, dWf, Ws_first=W16f, visit=ones) is False
    torch.cuda.synchronize()
    assert _untouched(dx, *dW, *dWf)
    # two groups
    lo, up = (s.device_csr() for s in plan._shift_pair)
    two = ops.ConvOp(E, [{"mats": [lo], "identity": True, "n_cols": E}, {"mats": [up], "identity": False, "n_cols": E}])
    t32, W32 = _randn(rs, S, E, 4, 32), _weights(rs)
    dW, dx = [_sentinel((32, 32)) for _ in range(3)], _sentinel(t32.shape)
    assert two.backward([t32, t32], W32, t32, "tanh", True, dW, dx=dx, visit=ones) is False
    torch.cuda.synchronize()
    assert _untouched(dx, *dW)
    # 32 slab ranges at the most: 2080 slabs leave every workgroup 65 or more (the one-block complex keeps the tensors small)
    tiny = _env("tiny4")
    tp, S = tiny["plan"](), 2080
    big = _pack(np.ones((1, S), bool))
    t = torch.zeros((S, tiny["E"], 4, 32), device="cuda")
    dW, dx = [_sentinel((32, 32)) for _ in range(3)], _sentinel(t.shape)
    assert tp.conv_T.backward([t], W32, t, "tanh", True, dW, dx=dx, visit=big) is False
    dWf, yb = [_sentinel((1, 32)) for _ in range(3)], torch.zeros((S, tiny["E"], 4, 4), device="cuda")
    assert tp.conv_T.backward_fused_first(t, W32, None, "tanh", yb, dW, dWf, Ws_first=_weights(rs, 1), visit=big) is False
    ys = _sentinel(yb.shape)
    st = _lib.load().scn_conv_shifted_input_keep(tp.conv.handle, S, 4, ops._dev(torch.zeros((S, tiny["E"], 4, 1), device="cuda")),
                                                 ops._dev(ys), ops._dev(big, torch.int32), ops._stream())
    torch.cuda.synchronize()
    assert st == _lib.SCN_ERR_UNSUPPORTED
    assert _untouched(dx, ys, *dW, *dWf)
    # visit = NULL
    lib, cdz = _lib.load(), ops.i32_array([32])
    ws = ops._workspace(lib.scn_conv_backward_workspace(plan.conv_T.handle, 4, 4, cdz, 32), "cuda", 256)
    dW, dx = [_sentinel((32, 32)) for _ in range(3)], _sentinel(t32.shape)
    st = lib.scn_conv_backward_visit(plan.conv_T.handle, 4, 4, ops._ptrs([t32]), cdz, ops._ptrs(W32), ops._dev(t32), 32, ops.ACT["tanh"],
                                     ops._dev(dx), ops._ptrs(dW), *ws, None, ops._stream())
    torch.cuda.synchronize()
    assert st == _lib.SCN_ERR_BAD_ARG and _untouched(dx, *dW)


# ------------------------------------------------------------------------------------------------------------------
# the visiting backward, fused-first from-y form
# ------------------------------------------------------------------------------------------------------------------

def _first_case(env, act, S, pattern, rs):
    plan = env["plan"](act)
    m = _mask(pattern, env["nb"], S, rs)
    v = _hop(env, m)
    dz = _randn(rs, S, env["E"], 4, 32) * _rows(m, env["row0"])[:, :, None, None]
    y = plan.conv.shifted_input(_randn(rs, S, env["E"], 4, 1))
    W, Wf = _weights(rs), _weights(rs, 1)
    dW0, dWf0 = [_randn(rs, 32, 32) for _ in range(3)], [_randn(rs, 1, 32) for _ in range(3)]
    dW, dWf = [t.clone() for t in dW0], [t.clone() for t in dWf0]
    assert plan.conv_T.backward_fused_first(dz, W, None, act, y, dW, dWf, Ws_first=Wf)
    torch.cuda.synchronize()
    return dict(plan=plan, m=m, v=v, dz=dz, y=y, W=W, Wf=Wf, dW0=dW0, dWf0=dWf0, dW=dW, dWf=dWf, mask=_pack(v))


def _first_visit(c, act, dz=None, y=None, W=None):
    dW, dWf = [t.clone() for t in c["dW0"]], [t.clone() for t in c["dWf0"]]
    assert c["plan"].conv_T.backward_fused_first(c["dz"] if dz is None else dz, c["W"] if W is None else W, None, act,
                                                 c["y"] if y is None else y, dW, dWf, Ws_first=c["Wf"], visit=c["mask"]), "not served"
    torch.cuda.synchronize()
    return dW, dWf


@pytest.mark.parametrize("act,S", SHAPES)
def test_visiting_fused_first_backward_equals_the_plain_one(act, S):
    """dW and dW_first; then NaN over y outside V and over the dz no item of V stages."""
    _need_gpu()
    env = _env()
    rs = np.random.RandomState(200 * S + (act == "relu"))
    for pattern in PATTERNS:
        c = _first_case(env, act, S, pattern, rs)
        what = "%s, %d slabs, M %s" % (act, S, pattern)
        y_p = _nan_where(_rows(~c["v"], env["row0"]), c["y"])
        dz_p = _nan_where(_rows(~_staged(env, c["v"]), env["row0"]), c["dz"])
        assert pattern == "all" or (bool(torch.isnan(y_p).any()) and bool(torch.isnan(dz_p).any()))
        for tag, kw in (("", {}), (" with poisoned tensors", dict(dz=dz_p, y=y_p))):
            dW, dWf = _first_visit(c, act, **kw)
            for g in range(3):
                _same_bits(dW[g], c["dW"][g], "dW[%d]%s, %s" % (g, tag, what))
                _same_bits(dWf[g], c["dWf"][g], "dW_first[%d]%s, %s" % (g, tag, what))
        if pattern == "random":
            assert max(float((a - b).abs().max()) for a, b in zip(c["dWf"], c["dWf0"])) > 0


@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_one_inf_weight_every_entry_the_plain_call_makes_non_finite_is_non_finite(act):
    """The visiting forms visit V whatever the weights are (no widening to all ones): with V non-empty every gradient entry that the
    plain call makes non-finite is non-finite here too."""
    _need_gpu()
    env = _env()
    rs = np.random.RandomState(9)
    bad = lambda ts: torch.cat([~torch.isfinite(t).reshape(-1) for t in ts])
    c = _bwd_case(env, act, 5, "random", rs)
    assert c["v"].any()
    W = [w.clone() for w in c["W"]]
    W[1][3, 7] = float("inf")
    ref = [t.clone() for t in c["dW0"]]
    c["plan"].conv_T.backward([c["dz"]], W, c["aux"], act, True, ref)
    _, dW = _visit(c, act, W=W)
    assert not bool((bad(ref) & ~bad(dW)).any()), "plain form"
    f = _first_case(env, act, 5, "random", rs)
    assert f["v"].any()
    W = [w.clone() for w in f["W"]]
    W[1][3, 7] = float("inf")
    ref, ref_f = [t.clone() for t in f["dW0"]], [t.clone() for t in f["dWf0"]]
    assert f["plan"].conv_T.backward_fused_first(f["dz"], W, None, act, f["y"], ref, ref_f, Ws_first=f["Wf"])
    dW, dWf = _first_visit(f, act, W=W)
    assert bool(bad(ref_f).any()), "the plain call's dW_first has a non-finite entry"
    assert not bool((bad(ref + ref_f) & ~bad(dW + dWf)).any()), "fused-first form"


# ------------------------------------------------------------------------------------------------------------------
# the masked clear
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,C", [(5, 32), (64, 32), (130, 32), (5, 4)])
def test_masked_clear_zeroes_the_listed_items_and_nothing_else(S, C):
    _need_gpu()
    env = _env()
    rs = np.random.RandomState(S + C)
    n = S * env["E"] * 4 * C
    for pattern in PATTERNS:
        k = _mask(pattern, env["nb"], S, rs)
        buf = _sentinel((n + 4,))                                            # (four guard words behind the tensor)
        t = buf[:n].view(S, env["E"], 4, C)
        env["plan"]().conv.clear_mask(t, _pack(k))
        torch.cuda.synchronize()
        want = torch.where(_rows(k, env["row0"])[:, :, None, None], torch.zeros_like(t.view(torch.int32)),
                           torch.full_like(t.view(torch.int32), SENTINEL))
        _same_bits(t.view(torch.int32), want, "%d slabs, %d channels, mask %s" % (S, C, pattern))
        assert _untouched(buf[n:])


# ------------------------------------------------------------------------------------------------------------------
# end to end on the plan
# ------------------------------------------------------------------------------------------------------------------

_DATA = {}


def _data():
    """Twelve trajectories on the cfg1 complex plus a slab of padding, the first ending on a node of maximal degree; fp64 oracle
    inputs (the batch of tests/test_gpu_keep_last.py, on the golden complex)."""
    if not _DATA:
        from scone_gcn_amd import ops, synthetic_data_gen as g
        env = _env()
        cx, sc, N = env["cx"], env["sc"], 12
        paths = g.generate_random_walks(cx, m=N, seed=3)
        flows, choice, last, _, _ = g.path_dataset(cx, paths, seed=4)
        nb, _ = so.neighborhoods(cx.edges, cx.n_nodes)
        last, choice = np.asarray(last).copy(), np.asarray(choice).copy()
        last[0] = int(np.argmax((np.asarray(nb) >= 0).sum(axis=1)))
        choice[0] = 0
        y = so.onehot_targets(choice, sc.max_degree)
        B1, B2 = (m.toarray() for m in g.incidence_matrices(cx))
        dev = ops.default_device()
        x, _ = ops.flows_to_slabs(flows, sc.layout, dev)
        x = torch.cat([x, torch.zeros_like(x[:1])]).contiguous()
        n_pad = x.shape[0] * ops.NS
        yp = np.zeros((n_pad, sc.max_degree), np.float32)
        yp[:N] = np.asarray(y).reshape(N, sc.max_degree)
        _DATA.update(N=N, flows=flows, last=last, y=y, B1=B1, B2=B2, nb=nb, x=x, last_dev=ops._last_nodes_dev(last, n_pad, dev),
                     y_dev=torch.as_tensor(yp, device=dev))
    return _DATA


def _thresholds(monkeypatch, value=0):
    from scone_gcn_amd import ops
    for name in ("KEEP_LAST_MIN_BYTES", "SMALL_DZ_BYTES", "READOUT_CONE_MIN_BYTES"):
        monkeypatch.setattr(ops.SconePlan, name, value)


def _step(plan, w, on, monkeypatch, activity=None, last_dev=None):
    """(logp, loss, grads, timer keys, the forward ran on the cone) of one step with the switch set."""
    from scone_gcn_amd import ops
    d = _data()
    monkeypatch.setattr(ops, "READOUT_CONE", on)
    wt = [torch.tensor(a, dtype=torch.float32, device="cuda") for a in w]
    last_dev = d["last_dev"] if last_dev is None else last_dev
    with ops.KernelTimer() as kt:
        logp, saved = plan.forward(d["x"], last_dev, wt, activity) if activity is not None else plan.forward(d["x"], last_dev, wt)
        loss = -(logp * d["y_dev"]).sum() / d["N"]
        grads = [torch.zeros_like(a) for a in wt]
        plan.backward(saved, logp, -d["y_dev"] / d["N"], last_dev, wt, grads)
    torch.cuda.synchronize()
    return logp.clone(), loss.reshape(1), grads, set(kt.table()), getattr(saved, "cone", None) is not None


def _pools_all_zero(plan):
    pools = [t for pool in plan._dz_zero.values() for t in pool]
    assert pools, "no pooled gradient buffer"
    return all(not bool(t.view(torch.int32).any()) for t in pools)


@pytest.mark.parametrize("act,layers", [("tanh", 3), ("relu", 3), ("tanh", 4)])
def test_plan_step_with_and_without_the_cone(act, layers, monkeypatch):
    """Loss and every weight gradient with READOUT_CONE on against off bit for bit; the path ran (the record carries the masks, the
    masked clear ran) and the masks grow strictly from M0 to M1; the pooled gradient buffers hold no non-zero bit afterwards; the tanh
    steps against the fp64 oracle."""
    _need_gpu()
    from scone_gcn_amd import ops
    env, d = _env(), _data()
    _thresholds(monkeypatch)
    plan = env["plan"](act)
    rs = np.random.RandomState(41)             # (the draw of the suite's other oracle steps on this stack: tests/test_gpu_top_dz_mask.py)
    w = [0.3 * rs.randn(*s) for s in so.weight_shapes(1, [(3, 32)] * layers, 1)]
    on = _step(plan, w, True, monkeypatch)
    assert _pools_all_zero(plan)
    off = _step(plan, w, False, monkeypatch)
    assert on[4] and not off[4]
    assert "clear_mask" in on[3] and "clear_mask" not in off[3]
    _assert_equal_steps(on, off, "%d layers of 32, %s" % (layers, act))
    assert max(float(g.abs().max()) for g in on[2]) > 0
    # the cone of this batch: M0 is a proper subset of M1, and every mask contains the one before
    tabs = env["tabs"]
    m = [ops.keep_mask_host(d["last_dev"].cpu().numpy(), ops.NS, tabs.top_ptr.cpu().numpy()[:plan.n_nodes + 1],
                            tabs.top_blk.cpu().numpy()[:-1], tabs.n_blocks)]
    for _ in range(layers - 1):
        m.append(ops.mask_hop_host(m[-1], *env["adj"]))
    bits = [_unpack(a, d["x"].shape[0]) for a in m]
    print("items per mask of %d: %s" % (bits[0].size, [int(b.sum()) for b in bits]))
    assert bits[0].any() and all(not (a & ~b).any() for a, b in zip(bits, bits[1:])) and (bits[1] & ~bits[0]).any()
    if act == "tanh":
        L_lo, L_up = so.scone_shifts(d["B1"], d["B2"])
        ref_loss, ref_g = so.scone_loss_and_grad(w, L_lo, L_up, so.make_Bconds(d["B1"], d["nb"]), d["last"],
                                                 d["flows"].todense().astype(float), d["y"], np.ones(d["N"], int), 0.0)
        errs = [abs(float(on[1]) - ref_loss) / max(1.0, abs(ref_loss))] + \
               [float(np.abs(a.cpu().numpy() - b).max()) / max(1.0, float(np.abs(b).max())) for a, b in zip(on[2], ref_g)]
        print("%d layers: error of the loss and of every gradient against the oracle: %s" % (layers, " ".join("%.2e" % e for e in errs)))
        assert max(errs) <= TOL


def test_two_batches_with_different_last_nodes_through_one_plan(monkeypatch):
    """Two forwards with different last nodes, then both backwards in reverse order, then the first batch again: each equals the run
    of a fresh plan bit for bit -- the masks belong to their forward, and the pooled buffers come back all-zero."""
    _need_gpu()
    from scone_gcn_amd import ops
    env, d = _env(), _data()
    _thresholds(monkeypatch)
    monkeypatch.setattr(ops, "READOUT_CONE", True)
    rs = np.random.RandomState(23)
    w = [torch.tensor(0.3 * rs.randn(*s), dtype=torch.float32, device="cuda") for s in so.weight_shapes(1, [(3, 32)] * 3, 1)]
    x, n_pad = d["x"], d["x"].shape[0] * ops.NS
    plan = env["plan"](fresh=True)
    lasts = [d["last_dev"], torch.as_tensor(rs.randint(0, plan.n_nodes, size=n_pad).astype(np.int32), device="cuda")]
    d_logps = [_randn(rs, n_pad, plan.max_deg) for _ in lasts]

    def backward(pl, logp, saved, last, d_logp):
        assert saved.cone is not None
        grads = [torch.zeros_like(a) for a in w]
        pl.backward(saved, logp, d_logp, last, w, grads)
        return logp.clone(), grads

    alone = []
    for last, dl in zip(lasts, d_logps):
        pl = env["plan"](fresh=True)
        alone.append(backward(pl, *pl.forward(x, last, w), last, dl))
    fwd = [plan.forward(x, last, w) for last in lasts]
    mixed = [None, None]
    for j in (1, 0):
        mixed[j] = backward(plan, *fwd[j], lasts[j], d_logps[j])
    again = backward(plan, *plan.forward(x, lasts[0], w), lasts[0], d_logps[0])
    torch.cuda.synchronize()
    assert not torch.equal(alone[0][0], alone[1][0]) and _pools_all_zero(plan)
    for j in range(2):
        _same_bits(mixed[j][0], alone[j][0], "logp of batch %d" % j)
        for k, (a, b) in enumerate(zip(mixed[j][1], alone[j][1])):
            _same_bits(a, b, "batch %d, gradient of weight %d" % (j, k))
        assert max(float(g.abs().max()) for g in alone[j][1]) > 0
    for k, (a, b) in enumerate(zip(again[1], alone[0][1])):
        _same_bits(a, b, "third use of the pooled buffers, gradient of weight %d" % k)


@pytest.mark.parametrize("case", ["hidden16", "separate_conv_T", "zeros", "field", "two_layers", "keep_last_off", "top_dz_mask_off",
                                  "below_threshold"])
def test_refused_cases_give_todays_results(case, monkeypatch):
    """The path is not taken (no masks in the record, no masked clear) and the switch moves no bit."""
    _need_gpu()
    from scone_gcn_amd import ops
    env, d = _env(), _data()
    _thresholds(monkeypatch, ops.SconePlan.READOUT_CONE_MIN_BYTES if case == "below_threshold" else 0)
    rs = np.random.RandomState(17)
    hidden = 16 if case == "hidden16" else 32
    layers = 2 if case == "two_layers" else 3
    w = [0.3 * rs.randn(*s) for s in so.weight_shapes(1, [(3, hidden)] * layers, 1)]
    plan = env["plan"](fresh=case == "below_threshold")     # (below the bound the pooled gradient buffers are not kept all-zero: a plan of its own)
    if case == "separate_conv_T":              # the shifts are symmetric, so a second operator of the transposes computes the same: it
        plan = env["plan"](fresh=True)          # stands for non-symmetric shifts, whose block adjacency is not the forward operator's
        lo, up = (s.device_csr() for s in plan._shift_pair)
        E = lo.shape[0]
        plan.conv_T = ops.ConvOp(E, [{"mats": [lo.T.tocsr(), up.T.tocsr()], "identity": True, "n_cols": E}],
                                 plan.layout.block_starts[plan._shift_pair[0].row_level])
    if case == "keep_last_off":
        monkeypatch.setattr(ops, "KEEP_LAST", False)
    if case == "top_dz_mask_off":
        monkeypatch.setattr(ops, "TOP_DZ_MASK", False)
    activity = plan.activity(d["flows"], d["last"], 3, hidden, case) if case in ("zeros", "field") else None
    assert case not in ("zeros", "field") or activity is not None
    on = _step(plan, w, True, monkeypatch, activity=activity)
    off = _step(plan, w, False, monkeypatch, activity=activity)
    assert not on[4] and not off[4] and "clear_mask" not in (on[3] | off[3])
    _assert_equal_steps(on, off, case)
    assert max(float(g.abs().max()) for g in on[2]) > 0
