"""GPU tests of the visit masks of the cone step's backwards (ops.VISIT_ROWS, scn_cone_masks_visits).

dZ_L is non-zero only on the rows R0 the readout's backward writes, so the backward k layers down gathers a non-zero only on R_k = P^k R0
and needs to visit only V_k, the (block, slab) items holding a row of R_k -- a subset of the cone's M_k.  Three parts, BIT FOR BIT:

  * the entry: V_k against ops.visit_masks_host and the same call's masks, lists and counters against scn_cone_masks's, on the hand-built
    tables of tests/test_gpu_cone_masks.py with two more node -> blocks tables per level; 1, 5, 33 and 64 slabs (one and two mask
    words), L = 3 and 4, three micro-batches per call: a leaf count that is no multiple of four, last nodes that repeat, nodes outside
    the range; every buffer poisoned first (every word of every V_k is written, nothing else); the refusals write nothing;
  * the kernels: scn_conv_backward_visit and the fused-first from-y visiting form with visit = V_k against visit = M_k and against the
    plain call, on the 400-point generator complex (33 slabs) and on the ~40 000-edge complex of tests/test_gpu_visit_prefetch.py (5
    slabs), tanh and relu, k = 1 and 2, dz random on the rows of R_{k-1} and +0 elsewhere: dW and dW_first accumulated into non-zero
    values, dx into an all-zero buffer (the plain call's bits on V_k, +0 outside), and again with NaN over every aux / y item outside
    M_k and every dz item no item of V_k stages.  V_k is first asserted to be a PROPER subset of M_k;
  * plan steps with VISIT_ROWS on against off and against READOUT_CONE off: loss and every weight gradient, 3 and 4 layers, tanh and
    relu, the tanh steps against the fp64 oracle at the suite's 1e-5; two steps with different last nodes on one plan, the pooled
    buffers all-zero after each; the trainer's loop over two micro-batches into a garbage gradient buffer; one Inf weight in the top
    layer.  The golden complex and batch of tests/test_gpu_readout_cone.py, the plan's size bounds set to 0 as there."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")

from oracle import scone_oracle as so
from tests.test_gpu_cone_masks import GAP, NS, POISON, _call, _nodes, _tables, _up
from tests.test_gpu_keep_last import _need_gpu, _same_bits
from tests.test_gpu_readout_cone import TOL, _data, _env, _pools_all_zero, _thresholds
from tests.test_gpu_step_tail import _batch, _weights
from tests.test_gpu_top_dz_mask import _rows, _unpack

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------
# the entry
# ------------------------------------------------------------------------------------------------------------------

def _call_visits(lists, n_nodes, n_blocks, top, adj, vtabs, L, visits_null=False):
    """scn_cone_masks_visits on poisoned buffers: (status, per micro-batch (masks, lists, counters) as _call of
    tests/test_gpu_cone_masks.py returns them, per micro-batch [V_1 .. V_{L-1}]).  The untouched words are checked here."""
    from scone_gcn_amd import _lib, ops
    lib = _lib.load()
    dev = [torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in lists]
    words = [(-(-len(a) // NS) + 31) // 32 for a in lists]
    n_words = [n_blocks * w for w in words]
    stride = [nw + GAP for nw in n_words]
    total = ops.UNIT_COUNTERS * sum(stride) + GAP
    masks, units, visits = (torch.full((total,), POISON, dtype=torch.int32, device="cuda") for _ in range(3))
    counters = torch.full((len(lists) * ops.UNIT_COUNTERS + 1,), POISON, dtype=torch.int32, device="cuda")
    desc = (_lib.ConeMb * len(lists))()
    off, offs = 0, []
    for i, t in enumerate(dev):
        d = desc[i]
        d.node, d.n, d.stride = t.data_ptr(), t.numel(), stride[i]
        d.masks, d.units, d.counters = masks.data_ptr() + 4 * off, units.data_ptr() + 4 * off, counters.data_ptr() + 16 * i
        offs.append(off)
        off += ops.UNIT_COUNTERS * stride[i]
    tabs = [_up(a) for a in (*top, *adj)]
    vdev = [(_up(p), _up(b)) for p, b in vtabs]
    status = lib.scn_cone_masks_visits(len(lists), desc, None if visits_null else ops.ptr_array([visits.data_ptr() + 4 * o for o in offs]), NS,
                                       n_nodes, n_blocks, *(ctypes.c_void_p(t.data_ptr()) for t in tabs), L,
                                       ops.ptr_array([p.data_ptr() for p, _ in vdev]), ops.ptr_array([b.data_ptr() for _, b in vdev]),
                                       ops._stream())
    torch.cuda.synchronize()
    m, u, c, v = masks.cpu().numpy(), units.cpu().numpy(), counters.cpu().numpy(), visits.cpu().numpy()
    if status != 0:
        assert all((a == POISON).all() for a in (m, u, c, v)), "a declined call writes nothing"
        return status, None, None
    assert c[-1] == POISON
    out, vis, written, v_written = [], [], np.zeros(total, bool), np.zeros(total, bool)
    for i in range(len(lists)):
        cnt = c[4 * i:4 * i + 4].view(np.uint32)
        ms, us = [], []
        for k in range(L):
            a = offs[i] + k * stride[i]
            written[a:a + n_words[i]] = True
            ms.append(m[a:a + n_words[i]].view(np.uint32).reshape(n_blocks, words[i]))
            us.append(u[a:a + cnt[k]].view(np.uint32))
            assert (u[a + cnt[k]:a + stride[i]] == POISON).all(), "list entries at or past the count are not written"
        out.append((ms, us, cnt))
        vs = []
        for k in range(L - 1):
            a = offs[i] + k * stride[i]
            v_written[a:a + n_words[i]] = True
            vs.append(v[a:a + n_words[i]].view(np.uint32).reshape(n_blocks, words[i]))
        vis.append(vs)
    assert (m[~written] == POISON).all() and (v[~v_written] == POISON).all(), "nothing but the masks' own words is written"
    return status, out, vis


def _visit_tabs(n_nodes, n_blocks, L, seed, bad=False):
    """L - 1 more node -> blocks tables, each of its own draw (the entry takes any table)."""
    return [_tables(n_nodes, n_blocks, seed + 17 * k, bad=bad)[0] for k in range(1, L)]


@pytest.mark.parametrize("L", [3, 4])
@pytest.mark.parametrize("slabs", [1, 5, 33, 64])
def test_entry_against_the_host_and_against_scn_cone_masks(slabs, L):
    _need_gpu()
    from scone_gcn_amd import ops
    n_nodes, n_blocks = 90, 1300                                   # (1300 and 2600 words: more than one trip of the 1024 threads)
    top, adj = _tables(n_nodes, n_blocks, 10 * slabs + L, bad=True)
    vtabs = _visit_tabs(n_nodes, n_blocks, L, slabs, bad=True)
    n = NS * slabs
    short = _nodes(n - 1, n_nodes, slabs)                          # a leaf count that is no multiple of four
    repeat = np.repeat(_nodes(2, n_nodes, slabs + 1), [n // 2, n - n // 2]).astype(np.int32)
    outside = _nodes(n, n_nodes, slabs + 2)
    outside[::3] = -1
    outside[1::5] = n_nodes
    lists = [short, repeat, outside]
    status, got, vis = _call_visits(lists, n_nodes, n_blocks, top, adj, vtabs, L)
    assert status == 0
    status, ref = _call(lists, n_nodes, n_blocks, top, adj, L)
    assert status == 0
    for i, nodes in enumerate(lists):
        want = ops.visit_masks_host(nodes, NS, vtabs, n_blocks)
        assert len(vis[i]) == L - 1
        for k in range(L - 1):
            assert vis[i][k].shape == want[k].shape == (n_blocks, 2 if slabs > 32 else 1)
            assert (vis[i][k] == want[k]).all(), "V_%d of micro-batch %d" % (k + 1, i)
        assert any(v.any() for v in vis[i]), "the case sets something"
        for k in range(L):
            assert (got[i][0][k] == ref[i][0][k]).all(), "M_%d of micro-batch %d against scn_cone_masks" % (k, i)
            assert got[i][1][k].tolist() == ref[i][1][k].tolist(), "list %d of micro-batch %d" % (k, i)
        assert (got[i][2] == ref[i][2]).all(), "counters of micro-batch %d" % i


def test_entry_refusals_leave_every_buffer_untouched():
    _need_gpu()
    from scone_gcn_amd import _lib, ops
    limit = ops.cone_masks_limit()
    for n_blocks, lists, L in ((limit + 1, [_nodes(8, 8, 1)], 3), (limit // 2 + 1, [_nodes(8, 8, 1), _nodes(NS * 33, 8, 2)], 3),
                               (50, [_nodes(8, 8, 1)], ops.UNIT_COUNTERS + 1)):
        top, adj = _tables(8, n_blocks, 3)
        vtabs = _visit_tabs(8, n_blocks, min(L, ops.UNIT_COUNTERS) + 1, 3)[:L - 1]
        assert _call_visits(lists, 8, n_blocks, top, adj, vtabs, L)[0] == _lib.SCN_ERR_UNSUPPORTED
    top, adj = _tables(8, 50, 3)
    vtabs = _visit_tabs(8, 50, 3, 3)
    assert _call_visits([_nodes(8, 8, 1)], 8, 50, top, adj, vtabs, 3, visits_null=True)[0] == _lib.SCN_ERR_BAD_ARG
    assert _call_visits([_nodes(8, 8, 1)], 8, 50, top, adj, vtabs, 3)[0] == 0


# ------------------------------------------------------------------------------------------------------------------
# the two visiting backwards on V_k
# ------------------------------------------------------------------------------------------------------------------

_GEN = {}


def _gen(name):
    """A generator complex, its scone plan, field and visit tables, block starts, block adjacency and the pattern P (rows read
    columns, diagonal included) the visit tables hop over."""
    if name not in _GEN:
        from scone_gcn_amd import ops, synthetic_data_gen as g, trajectory_experiments as te
        from scone_gcn_amd.complex import SimplicialComplex
        cx = g.random_SC_graph(400 if name == "gen400" else g.calibrate_n_points(40000))
        sc = SimplicialComplex(cx)
        shifts, readout, _ = te.setup_from_complex(sc, "scone")
        plan = ops.SconePlan(shifts[0], shifts[1], readout, "tanh", ops.default_device())
        assert plan.conv_T is plan.conv
        tabs, vt = plan.field_tables_dev(), plan.visit_tables_dev(2)
        assert tabs is not None and vt is not None and len(vt.ptr) == 2
        E = cx.n_edges
        rowptr, cols, _ = ops.union_pattern([s.device_csr() for s in plan._shift_pair])
        rows = np.repeat(np.arange(E), np.diff(rowptr))
        PT = sp.csr_matrix((np.ones(len(rows) + E, np.int32), (np.r_[cols, np.arange(E)], np.r_[rows, np.arange(E)])), shape=(E, E))
        nb = tabs.n_blocks
        adj = (tabs.adj_ptr.cpu().numpy()[:nb + 1], tabs.adj_blk.cpu().numpy()[:-1])
        _GEN[name] = dict(plan=plan, tabs=tabs, vt=vt, E=E, nb=nb, PT=PT, adj=adj, row0=np.asarray(plan.conv.plan_blocks(), np.int64))
    return _GEN[name]


def _row_sets(env, last, S):
    """bool [3][S][E]: R_0, R_1, R_2 of every slab's leaves, by brute force over rows."""
    plan, E = env["plan"], env["E"]
    R0 = np.zeros((S, E), bool)
    for i, v in enumerate(last):
        for u in plan._h_nbr[v][plan._h_nbr[v] >= 0]:
            R0[i // NS, plan._h_inc_edge[plan._h_inc_ptr[u]:plan._h_inc_ptr[u + 1]]] = True
    out = [R0]
    for _ in range(2):
        out.append(np.asarray((sp.csr_matrix(out[-1].astype(np.int32)) @ env["PT"]).todense()) > 0)
    return out


def _staged(env, v):
    """The dz items (b', s) some item (b, s) of v stages: b' in A(b)."""
    adj_ptr, adj_blk = env["adj"]
    st = np.zeros_like(v)
    for b in np.flatnonzero(v.any(axis=1)):
        st[adj_blk[adj_ptr[b]:adj_ptr[b + 1]]] |= v[b]
    return st


def _nan_where(rows, t):
    return torch.where(rows[:, :, None, None], torch.full((), float("nan"), device="cuda"), t)


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("name,S", [("gen400", 33), ("gen40k", 5)])
def test_visiting_backwards_on_v_against_m_and_against_the_plain_call(name, S, act):
    _need_gpu()
    from scone_gcn_amd import ops
    env = _gen(name)
    plan, tabs, E, nb, row0 = env["plan"], env["tabs"], env["E"], env["nb"], env["row0"]
    rs = np.random.RandomState(S)
    last = rs.randint(0, plan.n_nodes, size=NS * S).astype(np.int32)
    cone, = plan.conv.cone_masks([torch.as_tensor(last, device="cuda")], NS, plan.n_nodes, tabs, 3, visit_tabs=env["vt"])
    torch.cuda.synchronize()
    R = _row_sets(env, last, S)
    torch.manual_seed(S)
    t = lambda *shape: torch.randn(*shape, device="cuda")         # noqa: E731
    W, Wf = [0.3 * t(32, 32) for _ in range(3)], [0.3 * t(1, 32) for _ in range(3)]
    dW0, dWf0 = [t(32, 32) for _ in range(3)], [t(1, 32) for _ in range(3)]
    h = t(S, E, 4, 32)
    aux = torch.tanh(h) if act == "tanh" else torch.relu(h)
    y = plan.conv.shifted_input(t(S, E, 4, 1))
    op = plan.conv_T
    for k in (1, 2):
        what = "%s, %s, level %d" % (name, act, k)
        m, v = _unpack(cone[k].cpu().numpy().view(np.uint32), S), _unpack(cone.visits[k].cpu().numpy().view(np.uint32), S)
        print("%s: M_%d %d items, V_%d %d" % (what, k, m.sum(), k, v.sum()))
        assert not (v & ~m).any() and (m & ~v).any(), "V_%d is a proper subset of M_%d" % (k, k)
        in_v = np.repeat(v, np.diff(row0), axis=0).T
        assert not (R[k] & ~in_v).any(), "V_%d holds every item with a row in R_%d" % (k, k)
        dz = t(S, E, 4, 32) * torch.as_tensor(R[k - 1], device="cuda")[:, :, None, None]
        # the plain calls
        dW_p = [a.clone() for a in dW0]
        dx_p = op.backward([dz], W, aux, act, True, dW_p)
        dW2_p, dWf_p = [a.clone() for a in dW0], [a.clone() for a in dWf0]
        assert op.backward_fused_first(dz, W, None, act, y, dW2_p, dWf_p, Ws_first=Wf) is not False
        assert float(dx_p.abs().max()) > 0 and not bool((dx_p != 0)[~torch.as_tensor(in_v, device="cuda")].any()), \
            "the plain call's dx is zero outside V_%d" % k
        want_dx = torch.where(_rows(v, row0)[:, :, None, None], dx_p.view(torch.int32), torch.zeros_like(dx_p.view(torch.int32)))
        aux_x = _nan_where(_rows(~m, row0), aux)
        y_x = _nan_where(_rows(~m, row0), y)
        dz_x = _nan_where(_rows(~_staged(env, v), row0), dz)
        assert bool(torch.isnan(aux_x).any()) and bool(torch.isnan(dz_x).any())
        for tag, mask, dz_, aux_, y_ in (("visit = M", cone[k], dz, aux, y), ("visit = V", cone.visits[k], dz, aux, y),
                                         ("visit = V, poisoned", cone.visits[k], dz_x, aux_x, y_x)):
            dW = [a.clone() for a in dW0]
            dx = op.backward([dz_], W, aux_, act, True, dW, dx=torch.zeros_like(dz), visit=mask)
            assert dx is not False, "visiting backward not served"
            dW2, dWf = [a.clone() for a in dW0], [a.clone() for a in dWf0]
            assert op.backward_fused_first(dz_, W, None, act, y_, dW2, dWf, Ws_first=Wf, visit=mask) is not False
            torch.cuda.synchronize()
            if mask is not cone[k]:
                _same_bits(dx.view(torch.int32), want_dx, "dx: the plain call's on V, +0 outside (%s), %s" % (tag, what))
            else:
                _same_bits(dx.view(torch.int32)[_rows(v, row0)], dx_p.view(torch.int32)[_rows(v, row0)], "dx on V (%s), %s" % (tag, what))
            for g in range(3):
                _same_bits(dW[g], dW_p[g], "dW[%d] (%s), %s" % (g, tag, what))
                _same_bits(dW2[g], dW2_p[g], "the fused form's dW[%d] (%s), %s" % (g, tag, what))
                _same_bits(dWf[g], dWf_p[g], "dW_first[%d] (%s), %s" % (g, tag, what))
        assert max(float((a - b).abs().max()) for a, b in zip(dW_p + dWf_p, dW0 + dWf0)) > 0, "the case contracts nothing"


# ------------------------------------------------------------------------------------------------------------------
# plan steps
# ------------------------------------------------------------------------------------------------------------------

def _bounds(monkeypatch):
    from scone_gcn_amd import ops
    _thresholds(monkeypatch)
    monkeypatch.setattr(ops.SconePlan, "VISIT_ROWS_MIN_BYTES", 0)
    monkeypatch.setattr(ops, "SMALL_STEP", False)
    monkeypatch.setattr(ops, "STEP_TAIL", True)
    monkeypatch.setattr(ops, "STEP_MASKS", True)


def _micro(plan, w, mode, monkeypatch, batch, last_dev=None):
    """One micro-batch the way the trainer runs it.  mode "visits": VISIT_ROWS on; "masks": off; "no_cone": READOUT_CONE off (the step
    declines, the separate calls run).  (loss [1] fp64, grads, the cone the step ran on or None)."""
    from scone_gcn_amd import _lib, ops
    monkeypatch.setattr(ops, "VISIT_ROWS", mode == "visits")
    monkeypatch.setattr(ops, "READOUT_CONE", mode != "no_cone")
    x, last, yt, n = batch
    last = last if last_dev is None else last_dev
    part = torch.full((1,), 7.0, device="cuda", dtype=torch.float64)
    grads = [torch.zeros_like(a) for a in w]
    cones = plan.step_cones([(x, last, yt, None)], w)
    assert (cones is None) == (mode == "no_cone")
    cone = cones[0] if cones is not None else None
    assert cone is None or (cone.visits is not None) == (mode == "visits")
    ran = plan.step(x, last, yt, -1.0 / n, w, grads, part, overwrite=True, cone=cone)
    assert bool(ran) == (mode != "no_cone")
    if not ran:
        logp, saved = plan.forward(x, last, w)
        d_logp = torch.empty_like(logp)
        _lib.check(_lib.load().scn_masked_ce_begin(logp.numel(), ops._dev(logp), ops._dev(yt), -1.0 / n, ops._dev(d_logp),
                                                   ctypes.c_void_p(part.data_ptr()), 1, None, 0, ops._stream()), "scn_masked_ce_begin")
        plan.backward(saved, logp, d_logp, last, w, grads)
    torch.cuda.synchronize()
    return part, grads, cone


def _assert_same(a, b, what):
    _same_bits(a[0].view(torch.int32), b[0].view(torch.int32), "loss, " + what)
    for k, (p, q) in enumerate(zip(a[1], b[1])):
        _same_bits(p, q, "gradient of weight %d, %s" % (k, what))
    assert max(float(g.abs().max()) for g in a[1]) > 0 and float(a[0]) != 7.0


def _inside(cone, S):
    """V_k inside M_k for every level; the items of each as a string"""
    sizes = []
    for k in range(1, len(cone)):
        m, v = (_unpack(t.cpu().numpy().view(np.uint32), S) for t in (cone[k], cone.visits[k]))
        assert not (v & ~m).any()
        sizes.append("M_%d %d / V_%d %d" % (k, m.sum(), k, v.sum()))
    return ", ".join(sizes)


@pytest.mark.parametrize("act,layers,slabs", [("tanh", 3, 4), ("relu", 3, 4), ("tanh", 4, 4), ("relu", 4, 33)])
def test_plan_step_on_against_off_and_against_no_cone(act, layers, slabs, monkeypatch):
    _need_gpu()
    _bounds(monkeypatch)
    env, d = _env(), _data()
    w, batch = _weights(layers), _batch(slabs)
    res = {}
    for mode in ("visits", "masks", "no_cone"):
        plan = env["plan"](act, fresh=True)
        res[mode] = _micro(plan, w, mode, monkeypatch, batch)
        assert mode == "no_cone" or _pools_all_zero(plan)
    print("%d layers, %s, %d slabs: %s" % (layers, act, slabs, _inside(res["visits"][2], slabs)))
    _assert_same(res["visits"], res["masks"], "VISIT_ROWS on against off, %d layers, %s" % (layers, act))
    _assert_same(res["visits"], res["no_cone"], "VISIT_ROWS on against READOUT_CONE off, %d layers, %s" % (layers, act))
    if act == "tanh":
        wn = [a.cpu().numpy().astype(np.float64) for a in w]
        L_lo, L_up = so.scone_shifts(d["B1"], d["B2"])
        ref_loss, ref_g = so.scone_loss_and_grad(wn, L_lo, L_up, so.make_Bconds(d["B1"], d["nb"]), d["last"],
                                                 d["flows"].todense().astype(float), d["y"], np.ones(d["N"], int), 0.0)
        loss, grads, _ = res["visits"]
        errs = [abs(float(loss) - ref_loss) / max(1.0, abs(ref_loss))] + \
               [float(np.abs(a.cpu().numpy() - b).max()) / max(1.0, float(np.abs(b).max())) for a, b in zip(grads, ref_g)]
        print("%d layers: error of the loss and of every gradient against the oracle: %s" % (layers, " ".join("%.2e" % e for e in errs)))
        assert max(errs) <= TOL


def test_two_steps_with_different_last_nodes_on_one_plan(monkeypatch):
    _need_gpu()
    _bounds(monkeypatch)
    env, batch = _env(), _batch()
    w = _weights(4, seed=23)
    rs = np.random.RandomState(23)
    other = torch.as_tensor(rs.randint(0, env["plan"]().n_nodes, size=batch[1].numel()).astype(np.int32), device="cuda")
    plans = {mode: env["plan"](fresh=True) for mode in ("visits", "masks")}
    for k, last in enumerate((batch[1], other, batch[1])):
        res = {mode: _micro(plans[mode], w, mode, monkeypatch, batch, last_dev=last) for mode in plans}
        assert all(_pools_all_zero(p) for p in plans.values())
        _assert_same(res["visits"], res["masks"], "step %d" % k)
        assert sum(len(v) for v in plans["visits"]._dz_zero.values()) == sum(len(v) for v in plans["masks"]._dz_zero.values())


def test_the_trainers_loop_over_two_micro_batches_into_a_garbage_gradient_buffer(monkeypatch):
    _need_gpu()
    from scone_gcn_amd import ops, scone_trajectory_model as stm
    _bounds(monkeypatch)
    env, d = _env(), _data()
    te, N = env["te"], d["N"]
    shifts, readout, _ = te.setup_from_complex(env["sc"], "scone")
    inputs = [readout, d["last"], d["flows"]]
    y = np.asarray(d["y"])
    stm.reseed(1030)
    net = stm.Scone_GCN(1, 1e-3, N, 0.0, verbose=False)
    net.setup(te.scone_func, [(3, 32)] * 3, shifts, inputs, y, None, np.ones(N, int), model_type="scone")
    plan = net._plan(inputs)
    staged = net.stage(inputs, y, np.arange(0, 8)) + net.stage(inputs, y, np.arange(8, N))
    assert type(plan) is ops.SconePlan and len(staged) == 2
    cones = []
    real = ops.SconePlan.step
    monkeypatch.setattr(ops.SconePlan, "step", lambda self, *a, **k: cones.append(k.get("cone")) or real(self, *a, **k))
    res = {}
    for on in (True, False, True):
        monkeypatch.setattr(ops, "VISIT_ROWS", on)
        del cones[:]
        net._flat_g.copy_(torch.as_tensor(np.random.RandomState(5).randn(net._flat_g.numel()).astype(np.float32) * 1e3))
        loss = net._accumulate_staged(plan, staged, N, fresh=True)
        torch.cuda.synchronize()
        assert len(cones) == 2 and all(c is not None and (c.visits is not None) == on for c in cones)
        assert _pools_all_zero(plan)
        got = (loss.detach().clone().reshape(1), [net._flat_g.detach().clone()])
        if on in res:
            _assert_same(got, res[on], "VISIT_ROWS on, a second call")
        res[on] = got
    _assert_same(res[True], res[False], "the trainer's loop, VISIT_ROWS on against off")
    assert bool(torch.isfinite(res[True][1][0]).all())


@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_one_inf_weight_in_the_top_layer(act, monkeypatch):
    """Every gradient entry that is non-finite in the VISIT_ROWS-off step is non-finite in the on step."""
    _need_gpu()
    _bounds(monkeypatch)
    env = _env()
    w = _weights(3, seed=9)
    w[7][3, 7] = float("inf")                                       # (weights 6 .. 8: the top layer's three)
    res = {mode: _micro(env["plan"](act, fresh=True), w, mode, monkeypatch, _batch()) for mode in ("visits", "masks")}
    bad = lambda ts: torch.cat([~torch.isfinite(t).reshape(-1) for t in ts])        # noqa: E731
    assert bool(bad(res["masks"][1]).any()), "the off step has a non-finite entry"
    assert not bool((bad(res["masks"][1]) & ~bad(res["visits"][1])).any())
