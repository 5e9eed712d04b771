"""GPU tests of the last layer's forward that stores only what the readout reads (DESIGN.md sections 2 and 3, ops.KEEP_LAST).

Nothing reads H_L except the readout, on the edges incident to a neighbour of each trajectory's last node.  scn_keep_mask turns the
last nodes into a bit per (plan block, slab); the *_keep forwards stage, gather and contract every tile as the plain calls do and
store a finished tile only where its bit is set.  So every comparison here is BIT FOR BIT (int32 views): a kept row holds the bits
the plain forward writes, any other row still holds the NaN pattern the buffer was filled with, and log-probabilities, loss and all
weight gradients of a plan do not move by a bit when the switch is flipped; against the fp64 oracle the suite's 1e-5 of
max(1, |reference|).  The complex is random_SC_graph(2000) (dozens of plan blocks, the last one cut short); the path's size
threshold (SconePlan.KEEP_LAST_MIN_BYTES) is set to 0 where a test wants it on a small complex.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import scone_oracle as so

pytestmark = pytest.mark.gpu
TOL = 1e-5
SENTINEL = 0x7FC0DEAD                                    # a quiet NaN no kernel produces


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _same_bits(a, b, what):
    a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    assert a.shape == b.shape, what
    n = int((a != b).sum())
    assert n == 0, "%s: %d of %d values differ in their bits" % (what, n, a.numel())


_ENV = {}


def _env():
    """random_SC_graph(2000), its scone plan (tanh), the plan's block starts and node -> blocks table."""
    if not _ENV:
        from scone_gcn_amd import ops, synthetic_data_gen as g, trajectory_experiments as te
        from scone_gcn_amd.complex import SimplicialComplex
        cx = g.random_SC_graph(2000)
        sc = SimplicialComplex(cx)
        shifts, readout, _ = te.setup_from_complex(sc, "scone")
        plan = ops.get_scone_plan(shifts[0], shifts[1], readout, "tanh", ops.default_device())
        assert type(plan) is ops.SconePlan
        row0 = plan.conv.plan_blocks()
        assert len(row0) - 1 >= 24, "dozens of plan blocks"
        assert 0 < row0[-1] - row0[-2] < 64, "the complex is meant to end in a short block"
        tabs = plan.field_tables_dev()
        assert tabs is not None and tabs.n_blocks == len(row0) - 1
        _ENV.update(cx=cx, sc=sc, plan=plan, row0=np.asarray(row0, np.int64), tabs=tabs,
                    top=(tabs.top_ptr.cpu().numpy()[:plan.n_nodes + 1], tabs.top_blk.cpu().numpy()[:-1]))   # (without the upload's pad word)
    return _ENV


# ------------------------------------------------------------------------------------------------------------------
# the mask kernel against its NumPy restatement (ops.keep_mask_host; tests/test_host_keep_last.py checks that one by brute force)
# ------------------------------------------------------------------------------------------------------------------

def _mask_kernel(env, nodes, fill):
    """scn_keep_mask into a buffer pre-filled with `fill`, one guard word behind it."""
    from scone_gcn_amd import _lib
    plan, tabs = env["plan"], env["tabs"]
    n = len(nodes)
    words = (-(-n // 4) + 31) // 32
    buf = torch.full((tabs.n_blocks * words + 1,), fill, device="cuda", dtype=torch.int32)
    nd = torch.as_tensor(np.asarray(nodes, np.int32), device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(_lib.load().scn_keep_mask(n, 4, p(nd), plan.n_nodes, p(tabs.top_ptr), p(tabs.top_blk), tabs.n_blocks, p(buf),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "scn_keep_mask")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert out[-1] == fill, "the word behind the mask was written"
    return out[:-1].view(np.uint32).reshape(tabs.n_blocks, words)


@pytest.mark.parametrize("n_leaves,fill", [(4, 0), (3, -1), (128, 0), (132, 0), (130, -1), (132, 0x5A5A5A5A)])
def test_mask_kernel_equals_the_restatement(n_leaves, fill):
    """1, 32 and 33 slabs (33: a second word per block), last slabs that are not full, clean and dirty buffers (the launch zeroes)."""
    _need_gpu()
    from scone_gcn_amd import ops
    env = _env()
    rs = np.random.RandomState(n_leaves + (fill & 7))
    nodes = rs.randint(0, env["plan"].n_nodes, size=n_leaves)
    nodes[0] = int(np.argmax((env["plan"]._h_nbr >= 0).sum(axis=1)))        # a node of maximal degree
    if n_leaves > 8:
        nodes[5] = nodes[4]                                                   # a node repeated inside a slab
    got = _mask_kernel(env, nodes, fill)
    want = ops.keep_mask_host(nodes, 4, *env["top"], env["tabs"].n_blocks)
    assert want.any()
    assert np.array_equal(got, want)


def test_mask_kernel_reads_nothing_through_a_node_outside_the_table():
    _need_gpu()
    from scone_gcn_amd import ops
    env = _env()
    V = env["plan"].n_nodes
    nodes = np.array([7, -1, V, 2 ** 31 - 1, V + 5, 11, -(2 ** 31), 3])
    got = _mask_kernel(env, nodes, -1)
    want = ops.keep_mask_host(nodes, 4, *env["top"], env["tabs"].n_blocks)
    assert np.array_equal(got, want) and want.any()


def test_plan_mask_is_the_restatement_of_its_last_nodes():
    _need_gpu()
    from scone_gcn_amd import ops
    env = _env()
    nodes = np.random.RandomState(3).randint(0, env["plan"].n_nodes, size=20)
    m = env["plan"].conv.keep_mask(torch.as_tensor(nodes.astype(np.int32), device="cuda"), 4, env["plan"].n_nodes, env["tabs"])
    assert np.array_equal(m.cpu().numpy().view(np.uint32), ops.keep_mask_host(nodes, 4, *env["top"], env["tabs"].n_blocks))


# ------------------------------------------------------------------------------------------------------------------
# the kept forward against the full-store forward
# ------------------------------------------------------------------------------------------------------------------

def _input(env, S, C, rs):
    """[S, E, 4, C]: trajectory-like support (a third of the 64-row groups of a slab carry values, the rest exact zeros), slab 1 dense."""
    E = env["cx"].n_edges
    x = rs.randn(S, E, 4, C).astype(np.float32)
    live = (rs.rand(S, (E + 63) // 64) < 0.33).repeat(64, axis=1)[:, :E]
    if S > 1:
        live[1] = True
    return torch.as_tensor(x * live[:, :, None, None], device="cuda")


def _weights(C, rs, c_in=None):
    return [torch.as_tensor((0.3 * rs.randn(c_in or C, C)).astype(np.float32), device="cuda") for _ in range(3)]


def _bits(S, nb, name, rs):
    """bool [nb][S]: the kept (block, slab) items of a case."""
    k = np.zeros((nb, S), bool)
    if name == "ones":
        k[:] = True
    elif name == "alternating":          # one block kept in the even slabs and dropped in the odd ones, its neighbour the other way round;
        k[nb // 2, 0::2] = True          # every other block dropped (the deferred store of a kept tile rides in a dropped visit and
        k[nb // 2 + 1, 1::2] = True      # vice versa; C = 16: only slab A / only slab B of every pair)
    elif name == "last_of_last":         # only the last slab of the last, short block: the store after the loop
        k[nb - 1, S - 1] = True
    elif name == "random":
        k[:] = rs.rand(nb, S) < 0.3
    else:
        assert name == "zero"
    return k


def _pack(k):
    nb, S = k.shape
    m = np.zeros((nb, (S + 31) // 32), np.uint32)
    for s in range(S):
        m[:, s >> 5] |= k[:, s].astype(np.uint32) << np.uint32(s & 31)
    return torch.as_tensor(m.view(np.int32), device="cuda")


def _expected(full, k, row0):
    """`full` on the rows of kept (block, slab) items, the sentinel elsewhere (int32 views)."""
    rows = np.repeat(k, np.diff(row0), axis=0).T                      # [S][E]
    keep = torch.as_tensor(rows, device="cuda")[:, :, None, None]
    return torch.where(keep, full.view(torch.int32), torch.full_like(full.view(torch.int32), SENTINEL))


def _sentinel(shape):
    return torch.full(shape, SENTINEL, device="cuda", dtype=torch.int32).view(torch.float32)


MASKS = ["zero", "ones", "alternating", "last_of_last", "random"]
_FULL = {}


def _full_forward(env, C, act, S):
    """The inputs of a (C, act, S) case and the plain forward's output, computed once."""
    key = (C, act, S)
    if key not in _FULL:
        rs = np.random.RandomState(100 * C + S)
        x, W = _input(env, S, C, rs), _weights(C, rs)
        full = env["plan"].conv.forward([x], W, C, act)
        torch.cuda.synchronize()
        _FULL[key] = (x, W, full)
    return _FULL[key]


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("C,act,S", [(32, "tanh", 5), (16, "tanh", 5), (32, "relu", 5), (16, "tanh", 6), (32, "tanh", 37), (16, "tanh", 35)])
def test_kept_forward_writes_the_kept_rows_and_nothing_else(C, act, S, mask):
    """S = 5: an odd slab count (C = 16: the last pair has slab A only); 6: every pair complete; 37 / 35: a second mask word per block
    and slab ranges of the launch grid that start inside a word."""
    _need_gpu()
    env = _env()
    x, W, full = _full_forward(env, C, act, S)
    nb = len(env["row0"]) - 1
    k = _bits(S, nb, mask, np.random.RandomState(S + C))
    out = _sentinel(full.shape)
    got = env["plan"].conv.forward([x], W, C, act, out=out, keep=_pack(k))
    assert got is not None, "kept forward not served"
    torch.cuda.synchronize()
    _same_bits(got.view(torch.int32), _expected(full, k, env["row0"]), "C = %d, %s, %d slabs, mask %s" % (C, act, S, mask))
    if mask == "ones":
        _same_bits(got, full, "all ones = the full forward")


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("act,S", [("tanh", 5), ("relu", 3), ("tanh", 37)])
def test_kept_from_y_forward_writes_the_kept_rows_and_nothing_else(act, S, mask):
    """The from-y form (the last layer of a 2-layer hidden-32 stack)."""
    _need_gpu()
    env = _env()
    key = ("y", act, S)
    if key not in _FULL:
        rs = np.random.RandomState(7 + S)
        x = _input(env, S, 1, rs)
        Wf, W = _weights(32, rs, c_in=1), _weights(32, rs)
        y = env["plan"].conv.shifted_input(x)
        full = env["plan"].conv.forward_from_y(y, Wf, W, act)
        assert full is not None
        torch.cuda.synchronize()
        _FULL[key] = (y, Wf, W, full)
    y, Wf, W, full = _FULL[key]
    nb = len(env["row0"]) - 1
    k = _bits(S, nb, mask, np.random.RandomState(S))
    got = env["plan"].conv.forward_from_y(y, Wf, W, act, keep=_pack(k), out=_sentinel(full.shape))
    assert got is not None, "kept from-y forward not served"
    torch.cuda.synchronize()
    _same_bits(got.view(torch.int32), _expected(full, k, env["row0"]), "from y, %s, %d slabs, mask %s" % (act, S, mask))


def test_unserved_shapes_are_refused_before_any_launch():
    _need_gpu()
    env = _env()
    rs = np.random.RandomState(0)
    nb = len(env["row0"]) - 1
    x = _input(env, 2, 32, rs)
    out = _sentinel((2, env["cx"].n_edges, 4, 16))
    # 32 -> 16 channels has no kept form
    got = env["plan"].conv.forward([x], _weights(16, rs, c_in=32), 16, "tanh", out=out, keep=_pack(np.ones((nb, 2), bool)))
    torch.cuda.synchronize()
    assert got is None
    assert bool((out.view(torch.int32) == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------
# end to end on the plan
# ------------------------------------------------------------------------------------------------------------------

_SMALL = {}


def _small():
    """random_SC_graph(400), 12 trajectories plus padding (a fourth slab of four padding trajectories: no flow, last node 0), the first
    trajectory ending on a node of maximal degree; fp64 oracle inputs."""
    if not _SMALL:
        from scone_gcn_amd import ops, synthetic_data_gen as g, trajectory_experiments as te
        from scone_gcn_amd.complex import SimplicialComplex
        cx = g.random_SC_graph(400)
        sc = SimplicialComplex(cx)
        N = 12
        paths = g.generate_random_walks(cx, m=N, seed=3)
        flows, choice, last, _, _ = g.path_dataset(cx, paths, seed=4)
        nb, D = so.neighborhoods(cx.edges, cx.n_nodes)
        last = np.asarray(last).copy()
        choice = np.asarray(choice).copy()
        last[0] = int(np.argmax((np.asarray(nb) >= 0).sum(axis=1)))
        choice[0] = 0
        assert (np.asarray(nb)[last[0]] >= 0).sum() == sc.max_degree
        y = so.onehot_targets(choice, sc.max_degree)
        B1, B2 = (m.toarray() for m in g.incidence_matrices(cx))
        dev = ops.default_device()
        x, _ = ops.flows_to_slabs(flows, sc.layout, dev)
        x = torch.cat([x, torch.zeros_like(x[:1])]).contiguous()
        n_pad = x.shape[0] * ops.NS
        assert n_pad == 16
        yp = np.zeros((n_pad, sc.max_degree), np.float32)
        yp[:N] = np.asarray(y).reshape(N, sc.max_degree)
        _SMALL.update(cx=cx, sc=sc, N=N, flows=flows, last=last, y=y, B1=B1, B2=B2, nb=nb, x=x,
                      last_dev=ops._last_nodes_dev(last, n_pad, dev), y_dev=torch.as_tensor(yp, device=dev), shifts={}, te=te)
    return _SMALL


def _small_plan(model="scone", power=False):
    from scone_gcn_amd import ops
    sm = _small()
    key = (model, power)
    if key not in sm["shifts"]:
        shifts, readout, _ = sm["te"].setup_from_complex(sm["sc"], model)
        dev = ops.default_device()
        if power:
            plan = ops.PowerPlan(shifts[0], shifts[1], readout, "tanh", dev)
            assert plan.op.plan_info()[0] > 0
        else:
            plan = ops.SconePlan(shifts[0], shifts[1], readout, "tanh", dev)   # a plan of this file's own: its threshold is set below
        sm["shifts"][key] = plan
    return sm["shifts"][key]


def _step(plan, w, on, monkeypatch, threshold=0, activity=None, fill=True):
    """(logp, loss, grads, timer keys, H_L as the forward left it in a sentinel-filled buffer or None) with the switch set."""
    from scone_gcn_amd import ops
    sm = _small()
    monkeypatch.setattr(ops, "KEEP_LAST", on)
    monkeypatch.setattr(ops.SconePlan, "KEEP_LAST_MIN_BYTES", threshold)
    wt = [torch.tensor(a, dtype=torch.float32, device="cuda") for a in w]
    x = sm["x"]
    buf = None
    if fill and activity is None and plan.fused_conv:
        width = plan.layer_widths(wt)[-1]
        if width <= 32:
            buf = _sentinel((x.shape[0], x.shape[1], ops.NS, width))
    with ops.KernelTimer() as kt:
        if activity is not None:
            logp, saved = plan.forward(x, sm["last_dev"], wt, activity)
        else:
            logp, saved = plan.forward(x, sm["last_dev"], wt, out_last=buf)
        torch.cuda.synchronize()
        left = saved.hs[-1].clone() if buf is not None else None
        assert buf is None or saved.hs[-1].data_ptr() == buf.data_ptr()
        loss = -(logp * sm["y_dev"]).sum() / sm["N"]
        grads = [torch.zeros_like(a) for a in wt]
        plan.backward(saved, logp, -sm["y_dev"] / sm["N"], sm["last_dev"], wt, grads)
    torch.cuda.synchronize()
    return logp.clone(), loss.reshape(1), grads, set(kt.table()), left


def _assert_equal_steps(a, b, what):
    _same_bits(a[0], b[0], "log-probabilities, " + what)
    _same_bits(a[1], b[1], "loss, " + what)
    assert len(a[2]) == len(b[2])
    for k, (p, q) in enumerate(zip(a[2], b[2])):
        _same_bits(p, q, "gradient of weight %d, %s" % (k, what))


STACKS = {"3x32": [(3, 32)] * 3, "2x32": [(3, 32)] * 2, "mixed_32_16": [(3, 32), (3, 16)], "3x16": [(3, 16)] * 3, "2x16": [(3, 16)] * 2}


@pytest.mark.parametrize("stack", list(STACKS))
def test_plan_step_with_and_without_the_keep_mask(stack, monkeypatch):
    """logp, loss and every weight gradient: KEEP_LAST on against off bit for bit, and against the fp64 oracle; the mask launch ran,
    and H_L of the "on" run holds the sentinel outside the kept blocks and the "off" run's bits inside."""
    _need_gpu()
    from scone_gcn_amd import ops
    sm = _small()
    plan = _small_plan()
    layers = STACKS[stack]
    rs = np.random.RandomState(len(stack) + layers[-1][1])
    w = [0.3 * rs.randn(*s) for s in so.weight_shapes(1, layers, 1)]
    on = _step(plan, w, True, monkeypatch)
    off = _step(plan, w, False, monkeypatch)
    assert "keep_mask" in on[3] and "keep_mask" not in off[3]
    _assert_equal_steps(on, off, stack)
    # H_L: the "off" run wrote every row, the "on" run exactly the rows of the kept (block, slab) items
    row0 = np.asarray(plan.conv.plan_blocks(), np.int64)
    tabs = plan.field_tables_dev()
    mask = ops.keep_mask_host(sm["last_dev"].cpu().numpy(), ops.NS, tabs.top_ptr.cpu().numpy()[:plan.n_nodes + 1],
                              tabs.top_blk.cpu().numpy()[:-1], tabs.n_blocks)
    S = sm["x"].shape[0]
    k = ((mask[:, np.arange(S) >> 5] >> (np.arange(S) & 31).astype(np.uint32)) & 1).astype(bool)
    assert k.any() and not k.all(), "the last nodes' blocks are some of the plan's, not all"
    assert not bool((off[4].view(torch.int32) == SENTINEL).any())
    _same_bits(on[4].view(torch.int32), _expected(off[4], k, row0), "H_L, " + stack)
    # the oracle
    L_lo, L_up = so.scone_shifts(sm["B1"], sm["B2"])
    ref_loss, ref_g = so.scone_loss_and_grad(w, L_lo, L_up, so.make_Bconds(sm["B1"], sm["nb"]), sm["last"],
                                             sm["flows"].todense().astype(float), sm["y"], np.ones(sm["N"], int), 0.0)
    assert abs(float(on[1]) - ref_loss) <= TOL * max(1.0, abs(ref_loss))
    for a, b in zip(on[2], ref_g):
        assert float(np.abs(a.cpu().numpy() - b).max()) <= TOL * max(1.0, float(np.abs(b).max()))


def test_relu_plan_step_with_and_without_the_keep_mask(monkeypatch):
    _need_gpu()
    from scone_gcn_amd import ops
    sm = _small()
    shifts, readout, _ = sm["te"].setup_from_complex(sm["sc"], "scone")
    plan = ops.SconePlan(shifts[0], shifts[1], readout, "relu", ops.default_device())
    rs = np.random.RandomState(5)
    w = [0.3 * rs.randn(*s) for s in so.weight_shapes(1, [(3, 32)] * 3, 1)]
    on = _step(plan, w, True, monkeypatch)
    off = _step(plan, w, False, monkeypatch)
    assert "keep_mask" in on[3] and "keep_mask" not in off[3]
    _assert_equal_steps(on, off, "relu")
    assert bool((on[4].view(torch.int32) == SENTINEL).any()) and max(float(g.abs().max()) for g in on[2]) > 0


@pytest.mark.parametrize("case", ["wide", "power", "zeros", "field", "below_threshold"])
def test_refused_cases_run_the_full_store_path_with_equal_results(case, monkeypatch):
    """The wide stack, the composed Ebli plan, the work-list modes and a tensor below the threshold: no mask launch, H_L written
    everywhere, the same bits as with the switch off."""
    _need_gpu()
    from scone_gcn_amd import ops
    sm = _small()
    rs = np.random.RandomState(17)
    hidden = 64 if case == "wide" else 32
    scale = 0.05 if case == "power" else 0.3
    w = [scale * rs.randn(*s) for s in so.weight_shapes(1, [(3, hidden)] * 3, 1)]
    plan = _small_plan("ebli", power=True) if case == "power" else _small_plan()
    activity = None
    if case in ("zeros", "field"):
        activity = plan.activity(sm["flows"], sm["last"], 3, hidden, case)
        assert activity is not None
    threshold = ops.SconePlan.SMALL_DZ_BYTES if case == "below_threshold" else 0
    assert case != "below_threshold" or sm["x"].shape[0] * sm["x"].shape[1] * 4 * hidden * 4 <= threshold
    on = _step(plan, w, True, monkeypatch, threshold=threshold, activity=activity)
    off = _step(plan, w, False, monkeypatch, threshold=threshold, activity=activity)
    assert "keep_mask" not in on[3] and "keep_mask" not in off[3]
    _assert_equal_steps(on, off, case)
    assert max(float(g.abs().max()) for g in on[2]) > 0
    if on[4] is not None:
        assert not bool((on[4].view(torch.int32) == SENTINEL).any()), "H_L was not written everywhere"


def test_two_forwards_with_different_last_nodes_then_both_backwards(monkeypatch):
    """One plan, two forwards with different last nodes (different masks, different kept rows), then both backwards in reverse order:
    each equals its stand-alone run bit for bit -- the mask belongs to its forward alone."""
    _need_gpu()
    from scone_gcn_amd import ops
    sm = _small()
    plan = _small_plan()
    monkeypatch.setattr(ops, "KEEP_LAST", True)
    monkeypatch.setattr(ops.SconePlan, "KEEP_LAST_MIN_BYTES", 0)
    rs = np.random.RandomState(23)
    w = [torch.tensor(0.3 * rs.randn(*s), dtype=torch.float32, device="cuda") for s in so.weight_shapes(1, [(3, 32)] * 3, 1)]
    x, n_pad = sm["x"], sm["x"].shape[0] * ops.NS
    lasts = [sm["last_dev"], torch.as_tensor(rs.randint(0, plan.n_nodes, size=n_pad).astype(np.int32), device="cuda")]
    d_logps = [torch.tensor(rs.randn(n_pad, plan.max_deg).astype(np.float32), device="cuda") for _ in lasts]

    def backward(saved, logp, last, d_logp):
        grads = [torch.zeros_like(a) for a in w]
        plan.backward(saved, logp, d_logp, last, w, grads)
        return logp.clone(), grads

    alone = []
    for last, d in zip(lasts, d_logps):
        logp, saved = plan.forward(x, last, w)
        alone.append(backward(saved, logp, last, d))
    fwd = [plan.forward(x, last, w) for last in lasts]
    mixed = [None, None]
    for j in (1, 0):
        mixed[j] = backward(fwd[j][1], fwd[j][0], lasts[j], d_logps[j])
    torch.cuda.synchronize()
    assert not torch.equal(alone[0][0], alone[1][0])
    for j in range(2):
        _same_bits(mixed[j][0], alone[j][0], "logp of forward %d" % j)
        for k, (a, b) in enumerate(zip(mixed[j][1], alone[j][1])):
            _same_bits(a, b, "forward %d, gradient of weight %d" % (j, k))
        assert max(float(g.abs().max()) for g in alone[j][1]) > 0


def test_default_threshold_takes_the_path_from_8_mib_on(monkeypatch):
    """No override: on random_SC_graph(2000) sixteen trajectories give an H_L of 10.3 MiB at hidden 32 (the path is taken) and half
    that at hidden 16 (it is not); either way the switch moves no bit of the log-probabilities or of a weight gradient."""
    _need_gpu()
    from scone_gcn_amd import ops, synthetic_data_gen as g
    env = _env()
    plan, cx, sc = env["plan"], env["cx"], env["sc"]
    paths = g.generate_random_walks(cx, m=16, seed=5)
    flows, _, last, _, _ = g.path_dataset(cx, paths, seed=6)
    dev = ops.default_device()
    x, _ = ops.flows_to_slabs(flows, sc.layout, dev)
    last_dev = ops._last_nodes_dev(last, x.shape[0] * ops.NS, dev)
    rs = np.random.RandomState(31)
    d_logp = torch.tensor(rs.randn(x.shape[0] * ops.NS, plan.max_deg).astype(np.float32), device="cuda")
    assert x.numel() * 16 * 4 <= ops.SconePlan.KEEP_LAST_MIN_BYTES < x.numel() * 32 * 4
    for hidden in (32, 16):
        w = [torch.tensor(0.3 * rs.randn(*s), dtype=torch.float32, device="cuda") for s in so.weight_shapes(1, [(3, hidden)] * 3, 1)]
        res = {}
        for on in (True, False):
            monkeypatch.setattr(ops, "KEEP_LAST", on)
            with ops.KernelTimer() as kt:
                logp, saved = plan.forward(x, last_dev, w)
                grads = [torch.zeros_like(a) for a in w]
                plan.backward(saved, logp, d_logp, last_dev, w, grads)
            res[on] = (logp.clone(), grads, set(kt.table()))
        assert ("keep_mask" in res[True][2]) == (hidden == 32) and "keep_mask" not in res[False][2]
        _same_bits(res[True][0], res[False][0], "logp, hidden %d" % hidden)
        for k, (a, b) in enumerate(zip(res[True][1], res[False][1])):
            _same_bits(a, b, "gradient of weight %d, hidden %d" % (k, hidden))
        assert max(float(t.abs().max()) for t in res[True][1]) > 0
