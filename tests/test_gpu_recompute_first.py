"""GPU tests of the scone path that never stores the first layer's output H1 (ops.RECOMPUTE_FIRST).

H1[p][c] = act(y[p] . W_first[:, c]) follows from the 16-byte shifted-input record y[p] = (x, S_lo x, S_up x, 0); layer 1 writes y
only (ConvOp.shifted_input), layer 2's forward expands y into its LDS image (ConvOp.forward_from_y) and the fused-first backward
rebuilds its aux values in registers (ConvOp.backward_fused_first with aux = None).  All three sites and fwd_c1_kernel call ONE
function (first_layer_value, csrc/scn_internal.h), so every comparison against the materialised path here is BIT FOR BIT
(int32 views: a NaN must equal the same NaN, -0 is not +0); the oracle comparison is the suite's 1e-5 of max(1, |reference|).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import scone_oracle as so

pytestmark = pytest.mark.gpu
TOL = 1e-5
C = 32


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
    """random_SC_graph(2000) and its scone plan; the plan's last block is cut short by the row count (asserted)."""
    if not _ENV:
        from scone_gcn_amd import ops, synthetic_data_gen as g, trajectory_experiments as te
        from scone_gcn_amd.complex import SimplicialComplex
        cx = g.random_SC_graph(2000)
        sc = SimplicialComplex(cx)
        shifts, readout, _ = te.setup_from_complex(sc, "scone")
        plan = ops.get_scone_plan(shifts[0], shifts[1], readout, "tanh", ops.default_device())
        row0 = plan.conv.plan_blocks()
        assert 0 < row0[-1] - row0[-2] < 64, "the complex is meant to end in a short block"
        _ENV.update(E=cx.n_edges, plan=plan)
    return _ENV["E"], _ENV["plan"]


CASES = ["dense_S3", "sparse_S1", "zero_slabs", "nonfinite", "decades"]


def _flow(case, E, rs):
    """1-channel input slabs [S, E, 4, 1]."""
    S = 1 if case == "sparse_S1" else 3                           # S = 1 and an odd number of slabs
    x = np.zeros((S, E, 4, 1), np.float32)
    if case == "dense_S3":
        x[:] = rs.randn(S, E, 4, 1)
    else:                                                         # trajectory-like support: ~3 % of the rows
        for s in range(S):
            if case == "zero_slabs" and s != 1:
                continue                                          # slabs 0 and 2 stay all-zero
            for n in range(4):
                rows = rs.choice(E, E // 32, replace=False)
                x[s, rows, n, 0] = rs.randn(len(rows))
    if case == "nonfinite":                                       # one NaN and one Inf in the flow, different trajectories
        x[0, E // 3, 1, 0] = np.nan
        x[S - 1, E // 2, 2, 0] = np.inf
    if case == "decades":                                         # the four trajectories of every slab three decades apart
        x *= np.array([1.0, 1e1, 1e2, 1e3], np.float32)[None, None, :, None]
    return x


def _weights(rs):
    Wf = [(0.5 * rs.randn(1, C)).astype(np.float32) for _ in range(3)]
    W = [(0.3 * rs.randn(C, C)).astype(np.float32) for _ in range(3)]
    return Wf, W


def _dev(arrs):
    return [torch.as_tensor(a, device="cuda") for a in arrs]


@pytest.mark.parametrize("act", ["tanh", "relu", "leaky_relu"])
@pytest.mark.parametrize("case", CASES)
def test_forward_from_y_equals_the_materialised_two_layers_bit_for_bit(case, act):
    _need_gpu()
    E, plan = _env()
    rs = np.random.RandomState(11)
    x = torch.as_tensor(_flow(case, E, rs), device="cuda")
    Wf, W = (_dev(w) for w in _weights(rs))
    H1, y = plan.conv.forward_first(x, Wf, C, act)
    H2 = plan.conv.forward([H1], W, C, act)
    y2 = plan.conv.shifted_input(x)
    assert y2 is not None
    _same_bits(y2, y, "y of the y-only launch")
    got = plan.conv.forward_from_y(y2, Wf, W, act)
    assert got is not None, "from-y forward not served"
    torch.cuda.synchronize()
    _same_bits(got, H2, "layer 2 from y (%s, %s)" % (case, act))
    if case == "nonfinite":                                       # the NaN / Inf reach the output on both paths (same bits, checked above)
        assert not bool(torch.isfinite(got).all())


@pytest.mark.parametrize("act", ["tanh", "relu", "leaky_relu"])
@pytest.mark.parametrize("case", CASES)
def test_aux_free_fused_first_backward_equals_the_one_reading_h1_bit_for_bit(case, act):
    _need_gpu()
    E, plan = _env()
    rs = np.random.RandomState(13)
    xh = _flow(case, E, rs)
    x = torch.as_tensor(xh, device="cuda")
    Wf, W = (_dev(w) for w in _weights(rs))
    H1, y = plan.conv.forward_first(x, Wf, C, act)
    S = x.shape[0]
    dz = np.zeros((S, E, 4, C), np.float32)                       # gradient on ~6 % of the rows (and dense for the dense case)
    if case == "dense_S3":
        dz[:] = rs.randn(S, E, 4, C)
    else:
        for s in range(S):
            rows = rs.choice(E, E // 16, replace=False)
            dz[s, rows] = rs.randn(len(rows), 4, C)
    dz = torch.as_tensor(dz, device="cuda")
    out = []
    for aux in (H1, None):
        dW = [torch.zeros(C, C, device="cuda") for _ in range(3)]
        dW1 = [torch.zeros(1, C, device="cuda") for _ in range(3)]
        assert plan.conv_T.backward_fused_first(dz, W, aux, act, y, dW, dW1, Ws_first=None if aux is not None else Wf)
        out.append((dW, dW1))
    torch.cuda.synchronize()
    for k in range(3):
        _same_bits(out[1][0][k], out[0][0][k], "dW[%d] of layer 2 (%s, %s)" % (k, case, act))
        _same_bits(out[1][1][k], out[0][1][k], "dW_first[%d] (%s, %s)" % (k, case, act))
    if case != "nonfinite":
        assert all(bool(torch.isfinite(t).all()) for t in out[1][0] + out[1][1])
        assert any(float(t.abs().max()) > 0 for t in out[1][1])


def _small_problem(n_layers, N=8):
    from scone_gcn_amd import synthetic_data_gen as g
    from scone_gcn_amd.complex import SimplicialComplex
    cx = g.random_SC_graph(400)
    sc = SimplicialComplex(cx)
    paths = g.generate_random_walks(cx, m=N, seed=3)
    flows, choice, last, _, _ = g.path_dataset(cx, paths, seed=4)
    y = so.onehot_targets(choice, sc.max_degree)
    rs = np.random.RandomState(n_layers)
    w = [0.3 * rs.randn(*s) for s in so.weight_shapes(1, [(3, C)] * n_layers, 1)]
    return cx, sc, flows, last, y, w


def _run(sc, flows, last, y, w, on, monkeypatch):
    """(logp, loss, grads, timer keys) of te.scone_func + autograd with the switch set."""
    from scone_gcn_amd import ops, trajectory_experiments as te
    monkeypatch.setattr(ops, "RECOMPUTE_FIRST", on)
    shifts, readout, _ = te.setup_from_complex(sc, "scone")
    wt = [torch.tensor(a, dtype=torch.float32, device="cuda", requires_grad=True) for a in w]
    with ops.KernelTimer() as kt:
        out = te.scone_func(wt, *shifts, readout, last, flows)
        loss = -(out * torch.as_tensor(y, dtype=torch.float32, device="cuda").reshape(out.shape)).sum() / len(last)
        loss.backward()
    torch.cuda.synchronize()
    return out.detach(), loss.detach(), [t.grad for t in wt], set(kt.table())


@pytest.mark.parametrize("n_layers", [2, 3, 4])
def test_plan_forward_backward_with_and_without_a_stored_h1(n_layers, monkeypatch):
    """SconePlan.forward / backward with RECOMPUTE_FIRST on and off: identical log-probabilities, loss and every weight gradient
    (bit for bit), the new launches are the ones that ran, and both against the fp64 oracle at 1e-5 of max(1, |reference|)."""
    _need_gpu()
    from scone_gcn_amd import synthetic_data_gen as g
    cx, sc, flows, last, y, w = _small_problem(n_layers)
    on = _run(sc, flows, last, y, w, True, monkeypatch)
    off = _run(sc, flows, last, y, w, False, monkeypatch)
    assert "conv_fwd c1->y" in on[3] and "conv_fwd c1->32" not in on[3]          # layer 1 wrote y only
    assert "conv_fwd c1->32" in off[3] and "conv_fwd c1->y" not in off[3]
    _same_bits(on[0], off[0], "log-probabilities, %d layers" % n_layers)
    _same_bits(on[1].reshape(1), off[1].reshape(1), "loss, %d layers" % n_layers)
    for k, (a, b) in enumerate(zip(on[2], off[2])):
        _same_bits(a, b, "gradient of weight %d, %d layers" % (k, n_layers))
    B1, B2 = (m.toarray() for m in g.incidence_matrices(cx))
    L_lo, L_up = so.scone_shifts(B1, B2)
    nb, D = so.neighborhoods(cx.edges, cx.n_nodes)
    ref_loss, ref_g = so.scone_loss_and_grad(w, L_lo, L_up, so.make_Bconds(B1, nb), last, flows.todense().astype(float), y,
                                             np.ones(len(last), int), 0.0)
    assert abs(float(on[1]) - ref_loss) <= TOL * max(1.0, abs(ref_loss))
    for a, b in zip(on[2], ref_g):
        assert float(np.abs(a.cpu().numpy() - b).max()) <= TOL * max(1.0, float(np.abs(b).max()))


def test_headline_launch_shape_with_and_without_a_stored_h1(big_complex, monkeypatch):
    """|E| = 996 634, hidden 32, ONE launch of 128 trajectories = 32 slabs (what bench.py times 32 times per step): loss and all ten
    weight gradients with RECOMPUTE_FIRST on against off, bit for bit."""
    from scone_gcn_amd import ops, scone_trajectory_model as stm, synthetic_data_gen as g, trajectory_experiments as te
    cx, sc = big_complex
    N = 128
    paths = g.generate_random_walks(cx, m=N, seed=63, waypoint_pool=8, metric="euclid")
    flows, choice, last, _, _ = g.path_dataset(cx, paths, seed=64)
    y = so.onehot_targets(choice, sc.max_degree)
    rs = np.random.RandomState(13)
    w = [0.12 * rs.randn(*s) for s in so.weight_shapes(1, [(3, C)] * 3, 1)]
    shifts, readout, _ = te.setup_from_complex(sc, "scone")
    inputs = [readout, last, flows]
    stm.reseed(1030)
    net = stm.Scone_GCN(1, 1e-3, N, 0.0, verbose=False)
    net.setup(te.scone_func, [(3, C)] * 3, shifts, inputs, y, None, np.ones(N, int), model_type="scone")
    for a, b in zip(net.weights, w):
        a.copy_(torch.as_tensor(b, dtype=torch.float32))
    res = {}
    for on in (True, False):
        monkeypatch.setattr(ops, "RECOMPUTE_FIRST", on)
        staged = net.stage(inputs, y, np.arange(N))
        assert len(staged) == 1 and staged[0][0].shape[0] == 32
        with ops.KernelTimer() as kt:
            loss = net.grad_step_staged(inputs, staged, N, apply=False)
        res[on] = (torch.as_tensor(float(loss)).reshape(1), [t.detach().clone() for t in net._grads], set(kt.table()))
        del staged
        torch.cuda.empty_cache()
    assert "conv_fwd c1->y" in res[True][2] and "conv_fwd c1->y" not in res[False][2]
    assert float(res[True][0]) == float(res[False][0])
    for k, (a, b) in enumerate(zip(res[True][1], res[False][1])):
        _same_bits(a, b, "gradient of weight %d at |E| = %d" % (k, cx.n_edges))
    assert all(float(t.abs().max()) > 0 for t in res[True][1])
