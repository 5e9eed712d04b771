"""GPU tests of the top layer's backward that stages the readout gradient only where it was written (DESIGN.md sections 2 and 3,
ops.TOP_DZ_MASK).

The readout's backward writes dZ_L on the rows its forward reads: the keep mask M0 of the last layer's forward (scn_keep_mask) is
also where dZ_L can be non-zero.  scn_mask_hop takes it one hop out over the block adjacency -- bit (b, s) set wherever a block that
b's rows stage has its bit in M0 -- and scn_conv_backward_dzmask stages, gathers and reads aux only for the (block, slab) items of
that source mask; every other item gets the zero tile the plain call's early-out writes.  So every comparison here is BIT FOR BIT
(int32 views) against scn_conv_backward on the same tensors: dx on every row, the three weight gradients accumulated into non-zero
starting values; and at plan level log-probabilities, loss and all weight gradients with the switch on against off, and against
the fp64 oracle to the suite's 1e-5 of max(1, |reference|).  The complex is random_SC_graph(2000) (dozens of plan blocks, the last one
cut short), as in tests/test_gpu_keep_last.py, whose environment and small plan this file shares.

What "not read" means: aux of an item whose bit is clear is never requested; an item (b', s) of dz is staged by the items (b, s) with
b' in A(b), so it is never read when none of those has its bit set.  The poison test writes NaN on exactly those items.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import scone_oracle as so
from tests.test_gpu_keep_last import SENTINEL, _assert_equal_steps, _env, _need_gpu, _pack, _same_bits, _sentinel, _small, _small_plan

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _adj(env):
    if "adj" not in env:
        tabs = env["tabs"]
        env["adj"] = (tabs.adj_ptr.cpu().numpy()[:tabs.n_blocks + 1], tabs.adj_blk.cpu().numpy()[:-1])   # (without the upload's pad word)
    return env["adj"]


def _unpack(mask, S):
    return ((mask[:, np.arange(S) >> 5] >> (np.arange(S) & 31).astype(np.uint32)) & 1).astype(bool)


def _pack_host(k):
    return _pack(k).cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------
# the hop kernel against its NumPy restatement (ops.mask_hop_host; tests/test_host_top_dz_mask.py checks that one by brute force)
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fill", [0, -1, 0x5A5A5A5A])
@pytest.mark.parametrize("n_leaves", [3, 4, 128, 132])
def test_hop_kernel_equals_the_restatement(n_leaves, fill):
    """1, 32 and 33 slabs (33: a second word per block), a last slab that is not full; clean and dirty output buffers (every word is
    written), one guard word behind the output."""
    _need_gpu()
    from scone_gcn_amd import _lib, ops
    env = _env()
    tabs, nb = env["tabs"], env["tabs"].n_blocks
    rs = np.random.RandomState(n_leaves)
    nodes = rs.randint(0, env["plan"].n_nodes, size=n_leaves)
    m0 = ops.keep_mask_host(nodes, 4, *env["top"], nb)
    words = m0.shape[1]
    src = torch.as_tensor(m0.view(np.int32), device="cuda")
    buf = torch.full((nb * words + 1,), fill, device="cuda", dtype=torch.int32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(_lib.load().scn_mask_hop(nb, words, p(tabs.adj_ptr), p(tabs.adj_blk), p(src), p(buf),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "scn_mask_hop")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert out[-1] == fill, "the word behind the mask was written"
    want = ops.mask_hop_host(m0, *_adj(env))
    assert want.any() and not np.array_equal(want, m0)
    assert np.array_equal(out[:-1].view(np.uint32).reshape(nb, words), want)
    # the plan's own call
    got = env["plan"].conv.mask_hop(src, tabs)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want)


# ------------------------------------------------------------------------------------------------------------------
# the masked backward against the plain backward
# ------------------------------------------------------------------------------------------------------------------

PATTERNS = ["none", "all", "alternating", "random", "last_block", "slab0", "last_slab", "set_but_zero"]


def _m0(name, nb, S, rs):
    """bool [nb][S]: the (block, slab) items that carry the readout gradient."""
    k = np.zeros((nb, S), bool)
    if name == "all":
        k[:] = True
    elif name == "alternating":              # a block written in the even slabs, its neighbour in the odd ones: staged and unstaged visits
        k[nb // 2, 0::2] = True              # alternate in the blocks around them, with both buffer parities
        k[nb // 2 + 1, 1::2] = True
    elif name in ("random", "set_but_zero"):
        k[:] = rs.rand(nb, S) < 0.05
    elif name == "last_block":               # only the short last block
        k[nb - 1, :] = True
    elif name == "slab0":
        k[:, 0] = rs.rand(nb) < 0.3
    elif name == "last_slab":
        k[:, S - 1] = rs.rand(nb) < 0.3
    else:
        assert name == "none"
    return k


def _rows(k, row0):
    """bool [S][E] on the device: the rows of the set (block, slab) items."""
    return torch.as_tensor(np.repeat(k, np.diff(row0), axis=0).T.copy(), device="cuda")


_CASES = {}


def _case(act, S, pattern):
    """Tensors of one case and the plain backward's dx and weight gradients, computed once: dz is zero except random dense values on
    the rows of the items of M0 (pattern set_but_zero: zero there too), the source mask is hop(M0)."""
    key = (act, S, pattern)
    if key not in _CASES:
        from scone_gcn_amd import ops
        env = _env()
        plan, row0, nb, E = env["plan"], env["row0"], len(env["row0"]) - 1, env["cx"].n_edges
        rs = np.random.RandomState(1000 * S + 10 * PATTERNS.index(pattern) + (act == "relu"))
        k0 = _m0(pattern, nb, S, rs)
        hop = _unpack(ops.mask_hop_host(_pack_host(k0), *_adj(env)), S)
        assert not (k0 & ~hop).any()
        dz = torch.as_tensor(rs.randn(S, E, 4, 32).astype(np.float32), device="cuda")
        dz = dz * _rows(k0, row0)[:, :, None, None] * (0.0 if pattern == "set_but_zero" else 1.0)
        h = rs.randn(S, E, 4, 32).astype(np.float32)
        aux = torch.as_tensor(np.tanh(h) if act == "tanh" else np.maximum(h, 0), device="cuda")
        W = [torch.as_tensor((0.3 * rs.randn(32, 32)).astype(np.float32), device="cuda") for _ in range(3)]
        dW0 = [torch.as_tensor(rs.randn(32, 32).astype(np.float32), device="cuda") for _ in range(3)]
        dW = [t.clone() for t in dW0]
        dx = plan.conv_T.backward([dz], W, aux, act, True, dW)
        torch.cuda.synchronize()
        _CASES.clear()                                                   # (one case's tensors at a time: S = 37 is 0.1 GB each)
        _CASES[key] = dict(k0=k0, hop=hop, dz=dz, aux=aux, W=W, dW0=dW0, dx=dx, dW=dW, mask=_pack(hop))
    return _CASES[key]


def _masked(c, act, dz=None, aux=None, need_dx=True, W=None):
    env = _env()
    dW = [t.clone() for t in c["dW0"]]
    dx = env["plan"].conv_T.backward([c["dz"] if dz is None else dz], c["W"] if W is None else W, c["aux"] if aux is None else aux, act,
                                     need_dx, dW, dz_mask=c["mask"])
    assert dx is not False, "masked backward not served"
    torch.cuda.synchronize()
    return dx, dW


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("act,S", [("tanh", 5), ("relu", 5), ("tanh", 37), ("relu", 37)])
def test_masked_backward_equals_the_plain_backward_and_makes_no_pass_outside_the_mask(act, S, pattern):
    """S = 5: one mask word; 37: two, and slab ranges of the launch grid that start inside a word.  Clean tensors first; then every
    item of aux whose bit is clear and every item of dz that no set item stages overwritten with NaN: the same bits again, and the
    dx rows of the clear items are +0.0."""
    _need_gpu()
    env = _env()
    c = _case(act, S, pattern)
    what = "%s, %d slabs, M0 %s" % (act, S, pattern)
    assert pattern in ("none", "set_but_zero") or float(c["dx"].abs().max()) > 0
    dx, dW = _masked(c, act)
    _same_bits(dx, c["dx"], "dx, " + what)
    for g in range(3):
        _same_bits(dW[g], c["dW"][g], "dW[%d], %s" % (g, what))
    # poison
    hop, row0 = c["hop"], env["row0"]
    adj_ptr, adj_blk = _adj(env)
    staged = np.zeros_like(hop)                                          # dz item (b', s) is staged by (b, s), b' in A(b), bit (b, s) set
    for b in range(hop.shape[0]):
        staged[adj_blk[adj_ptr[b]:adj_ptr[b + 1]]] |= hop[b]
    nan = torch.full((), float("nan"), device="cuda")
    aux_p = torch.where(_rows(~hop, row0)[:, :, None, None], nan, c["aux"])
    dz_p = torch.where(_rows(~staged, row0)[:, :, None, None], nan, c["dz"])
    assert pattern == "all" or (bool(torch.isnan(aux_p).any()) and bool(torch.isnan(dz_p).any()))
    dx, dW = _masked(c, act, dz=dz_p, aux=aux_p)
    _same_bits(dx, c["dx"], "dx with poisoned tensors, " + what)
    for g in range(3):
        _same_bits(dW[g], c["dW"][g], "dW[%d] with poisoned tensors, %s" % (g, what))
    clear = _rows(~hop, row0)[:, :, None, None].expand_as(dx)
    assert int((dx.view(torch.int32)[clear] != 0).sum()) == 0, "a row outside the mask is not +0.0"


@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_one_inf_weight_takes_the_plain_path(act):
    """With a NaN / Inf weight the plain kernel has no zero-tile early-out (0 * Inf): the masked form ignores its mask and gives the
    same bits, NaNs included."""
    _need_gpu()
    env = _env()
    c = _case(act, 5, "random")
    W = [w.clone() for w in c["W"]]
    W[1][3, 7] = float("inf")
    dW_ref = [t.clone() for t in c["dW0"]]
    dx_ref = env["plan"].conv_T.backward([c["dz"]], W, c["aux"], act, True, dW_ref)
    dx, dW = _masked(c, act, W=W)
    assert bool(torch.isnan(dx_ref).any())
    _same_bits(dx, dx_ref, "dx, one Inf weight")
    for g in range(3):
        _same_bits(dW[g], dW_ref[g], "dW[%d], one Inf weight" % g)


def _raw(env, c, act, dx, dW, mask):
    """scn_conv_backward_dzmask itself (dx and mask may be None)."""
    from scone_gcn_amd import _lib, ops
    lib, op = _lib.load(), env["plan"].conv_T
    S = c["dz"].shape[0]
    cdz = ops.i32_array([32])
    ws = ops._workspace(lib.scn_conv_backward_workspace(op.handle, S, 4, cdz, 32), "cuda", 256)
    st = lib.scn_conv_backward_dzmask(op.handle, S, 4, ops._ptrs([c["dz"]]), cdz, ops._ptrs(c["W"]), ops._dev(c["aux"]), 32, ops.ACT[act],
                                      ops._dev(dx) if dx is not None else None, ops._ptrs(dW), *ws,
                                      ops._dev(mask, torch.int32) if mask is not None else None, ops._stream())
    torch.cuda.synchronize()
    return st


def test_dw_only_form_and_the_call_without_a_mask():
    _need_gpu()
    from scone_gcn_amd import _lib
    env = _env()
    c = _case("tanh", 5, "random")
    # dx = NULL: the weight gradients alone
    dW_ref = [t.clone() for t in c["dW0"]]
    assert env["plan"].conv_T.backward([c["dz"]], c["W"], c["aux"], "tanh", False, dW_ref) is None
    none, dW = _masked(c, "tanh", need_dx=False)
    assert none is None
    for g in range(3):
        _same_bits(dW[g], dW_ref[g], "dW[%d], dx = NULL" % g)
        _same_bits(dW[g], c["dW"][g], "dW[%d], dx = NULL against the call with dx" % g)
    # dzmask = NULL: the plain call
    dW = [t.clone() for t in c["dW0"]]
    dx = _sentinel(c["dx"].shape)
    _lib.check(_raw(env, c, "tanh", dx, dW, None), "scn_conv_backward_dzmask")
    _same_bits(dx, c["dx"], "dx, dzmask = NULL")
    for g in range(3):
        _same_bits(dW[g], c["dW"][g], "dW[%d], dzmask = NULL" % g)


def _untouched(*tensors):
    return all(bool((t.view(torch.int32) == SENTINEL).all()) for t in tensors)


def test_unserved_shapes_are_refused_before_any_launch():
    """C = 16, two groups, and a slab count that leaves a workgroup of every launch grid more than 64 slabs: SCN_ERR_UNSUPPORTED with
    dx and the weight gradients untouched."""
    _need_gpu()
    from scone_gcn_amd import _lib, ops
    env = _env()
    plan, nb, E = env["plan"], len(env["row0"]) - 1, env["cx"].n_edges
    rs = np.random.RandomState(0)
    # C = 16 (the slab-pair form has no mask)
    S = 4
    t16 = torch.as_tensor(rs.randn(S, E, 4, 16).astype(np.float32), device="cuda")
    W16 = [torch.as_tensor((0.3 * rs.randn(16, 16)).astype(np.float32), device="cuda") for _ in range(3)]
    dW = [_sentinel((16, 16)) for _ in range(3)]
    dx = _sentinel(t16.shape)
    assert plan.conv_T.backward([t16], W16, t16, "tanh", True, dW, dx=dx, dz_mask=_pack(np.ones((nb, S), bool))) is False
    torch.cuda.synchronize()
    assert _untouched(dx, *dW)
    # two groups
    sm = _small()
    sp = _small_plan()
    lo, up = (s.device_csr() for s in sp._shift_pair)
    Es = lo.shape[0]
    two = ops.ConvOp(Es, [{"mats": [lo], "identity": True, "n_cols": Es}, {"mats": [up], "identity": False, "n_cols": Es}])
    assert two.n_groups == 2 and two.n_slots == 3
    t32 = torch.as_tensor(rs.randn(S, Es, 4, 32).astype(np.float32), device="cuda")
    W32 = [torch.as_tensor((0.3 * rs.randn(32, 32)).astype(np.float32), device="cuda") for _ in range(3)]
    dW = [_sentinel((32, 32)) for _ in range(3)]
    dx = _sentinel(t32.shape)
    nbs = sp.field_tables_dev().n_blocks
    assert two.backward([t32, t32], W32, t32, "tanh", True, dW, dx=dx, dz_mask=_pack(np.ones((nbs, S), bool))) is False
    torch.cuda.synchronize()
    assert _untouched(dx, *dW)
    # 32 slab ranges at the most: 2080 slabs leave every workgroup 65 or more
    S = 2080
    t = torch.empty((S, Es, 4, 32), device="cuda", dtype=torch.float32)
    dx = _sentinel(t.shape)
    dW = [_sentinel((32, 32)) for _ in range(3)]
    assert sp.conv_T.backward([t], W32, t, "tanh", True, dW, dx=dx, dz_mask=_pack(np.ones((nbs, S), bool))) is False
    torch.cuda.synchronize()
    assert _untouched(dx, *dW)
    del sm


# ------------------------------------------------------------------------------------------------------------------
# end to end on the plan
# ------------------------------------------------------------------------------------------------------------------

def _step(plan, w, on, monkeypatch, activity=None, small_dz=0):
    """(logp, loss, grads, timer keys) of one step of the small complex with the switch set; small_dz: SconePlan.SMALL_DZ_BYTES."""
    from scone_gcn_amd import ops
    sm = _small()
    monkeypatch.setattr(ops, "TOP_DZ_MASK", on)
    monkeypatch.setattr(ops.SconePlan, "SMALL_DZ_BYTES", small_dz)
    monkeypatch.setattr(ops.SconePlan, "KEEP_LAST_MIN_BYTES", 0)
    wt = [torch.tensor(a, dtype=torch.float32, device="cuda") for a in w]
    with ops.KernelTimer() as kt:
        if activity is not None:
            logp, saved = plan.forward(sm["x"], sm["last_dev"], wt, activity)
        else:
            logp, saved = plan.forward(sm["x"], sm["last_dev"], wt)
        loss = -(logp * sm["y_dev"]).sum() / sm["N"]
        grads = [torch.zeros_like(a) for a in wt]
        plan.backward(saved, logp, -sm["y_dev"] / sm["N"], sm["last_dev"], wt, grads)
    torch.cuda.synchronize()
    return logp.clone(), loss.reshape(1), grads, set(kt.table())


@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_plan_step_with_and_without_the_source_mask(act, monkeypatch):
    """Three layers of 32: logp, loss and every weight gradient with TOP_DZ_MASK on against off bit for bit, the two mask launches
    ran, and (tanh) the step against the fp64 oracle."""
    _need_gpu()
    from scone_gcn_amd import ops
    sm = _small()
    if act == "tanh":
        plan = _small_plan()
    else:
        shifts, readout, _ = sm["te"].setup_from_complex(sm["sc"], "scone")
        plan = ops.SconePlan(shifts[0], shifts[1], readout, "relu", ops.default_device())
    rs = np.random.RandomState(41)
    w = [0.3 * rs.randn(*s) for s in so.weight_shapes(1, [(3, 32)] * 3, 1)]
    on = _step(plan, w, True, monkeypatch)
    off = _step(plan, w, False, monkeypatch)
    assert {"dz_mask", "dz_mask_hop"} <= on[3] and not ({"dz_mask", "dz_mask_hop"} & off[3])
    _assert_equal_steps(on, off, "three layers of 32, " + act)
    assert max(float(g.abs().max()) for g in on[2]) > 0
    if act == "tanh":
        L_lo, L_up = so.scone_shifts(sm["B1"], sm["B2"])
        ref_loss, ref_g = so.scone_loss_and_grad(w, L_lo, L_up, so.make_Bconds(sm["B1"], sm["nb"]), sm["last"],
                                                 sm["flows"].todense().astype(float), sm["y"], np.ones(sm["N"], int), 0.0)
        assert abs(float(on[1]) - ref_loss) <= TOL * max(1.0, abs(ref_loss))
        for a, b in zip(on[2], ref_g):
            assert float(np.abs(a.cpu().numpy() - b).max()) <= TOL * max(1.0, float(np.abs(b).max()))


def test_two_forwards_with_different_last_nodes_then_both_backwards(monkeypatch):
    """One plan, two forwards with different last nodes, then both backwards in reverse order: each equals the run of a fresh plan
    bit for bit -- the mask is built from the backward's own last nodes, and the pooled all-zero buffer comes back all-zero."""
    _need_gpu()
    from scone_gcn_amd import ops
    sm = _small()
    monkeypatch.setattr(ops, "TOP_DZ_MASK", True)
    monkeypatch.setattr(ops.SconePlan, "SMALL_DZ_BYTES", 0)
    monkeypatch.setattr(ops.SconePlan, "KEEP_LAST_MIN_BYTES", 0)
    shifts, readout, _ = sm["te"].setup_from_complex(sm["sc"], "scone")
    fresh = lambda: ops.SconePlan(shifts[0], shifts[1], readout, "tanh", ops.default_device())
    rs = np.random.RandomState(23)
    w = [torch.tensor(0.3 * rs.randn(*s), dtype=torch.float32, device="cuda") for s in so.weight_shapes(1, [(3, 32)] * 3, 1)]
    x, n_pad = sm["x"], sm["x"].shape[0] * ops.NS
    plan = fresh()
    lasts = [sm["last_dev"], torch.as_tensor(rs.randint(0, plan.n_nodes, size=n_pad).astype(np.int32), device="cuda")]
    d_logps = [torch.tensor(rs.randn(n_pad, plan.max_deg).astype(np.float32), device="cuda") for _ in lasts]

    def backward(pl, saved, logp, last, d_logp):
        grads = [torch.zeros_like(a) for a in w]
        with ops.KernelTimer() as kt:
            pl.backward(saved, logp, d_logp, last, w, grads)
        assert "dz_mask_hop" in set(kt.table())
        return logp.clone(), grads

    alone = []
    for last, d in zip(lasts, d_logps):
        pl = fresh()
        logp, saved = pl.forward(x, last, w)
        alone.append(backward(pl, saved, logp, last, d))
    fwd = [plan.forward(x, last, w) for last in lasts]
    mixed = [None, None]
    for j in (1, 0):
        mixed[j] = backward(plan, fwd[j][1], fwd[j][0], lasts[j], d_logps[j])
    again = backward(plan, *plan.forward(x, lasts[0], w)[::-1], lasts[0], d_logps[0])     # the pooled buffer a third time
    torch.cuda.synchronize()
    assert not torch.equal(alone[0][0], alone[1][0])
    for j in range(2):
        _same_bits(mixed[j][0], alone[j][0], "logp of forward %d" % j)
        for k, (a, b) in enumerate(zip(mixed[j][1], alone[j][1])):
            _same_bits(a, b, "forward %d, gradient of weight %d" % (j, k))
        assert max(float(g.abs().max()) for g in alone[j][1]) > 0
    for k, (a, b) in enumerate(zip(again[1], alone[0][1])):
        _same_bits(a, b, "third use of the pooled buffer, gradient of weight %d" % k)


@pytest.mark.parametrize("case", ["two_layers", "hidden16", "wide", "power", "zeros", "field", "separate_conv_T", "below_threshold"])
def test_refused_cases_run_the_plain_backward_with_equal_results(case, monkeypatch):
    """No mask launch, and the same bits as with the switch off."""
    _need_gpu()
    from scone_gcn_amd import ops
    sm = _small()
    rs = np.random.RandomState(17)
    hidden = {"wide": 64, "hidden16": 16}.get(case, 32)
    layers = 2 if case == "two_layers" else 3
    scale = 0.05 if case == "power" else 0.3
    w = [scale * rs.randn(*s) for s in so.weight_shapes(1, [(3, hidden)] * layers, 1)]
    plan = _small_plan("ebli", power=True) if case == "power" else _small_plan()
    if case == "separate_conv_T":           # the shifts are symmetric, so a second operator of the transposes computes the same
        shifts, readout, _ = sm["te"].setup_from_complex(sm["sc"], "scone")
        plan = ops.SconePlan(shifts[0], shifts[1], readout, "tanh", ops.default_device())
        lo, up = (s.device_csr() for s in plan._shift_pair)
        E = lo.shape[0]
        plan.conv_T = ops.ConvOp(E, [{"mats": [lo.T.tocsr(), up.T.tocsr()], "identity": True, "n_cols": E}],
                                 plan.layout.block_starts[plan._shift_pair[0].row_level])
        assert plan.conv_T is not plan.conv
    activity = None
    if case in ("zeros", "field"):
        activity = plan.activity(sm["flows"], sm["last"], 3, hidden, case)
        assert activity is not None
    small_dz = ops.SconePlan.SMALL_DZ_BYTES if case == "below_threshold" else 0
    assert case != "below_threshold" or sm["x"].shape[0] * sm["x"].shape[1] * 4 * hidden * 4 <= small_dz
    on = _step(plan, w, True, monkeypatch, activity=activity, small_dz=small_dz)
    off = _step(plan, w, False, monkeypatch, activity=activity, small_dz=small_dz)
    assert not ({"dz_mask", "dz_mask_hop"} & (on[3] | off[3]))
    _assert_equal_steps(on, off, case)
    assert max(float(g.abs().max()) for g in on[2]) > 0
