"""Training on whole paths on the MI355X (scn_path_stage in csrc/scn_paths.hip; Scone_GCN.path_grad_step / train_paths in
scone_gcn_amd/path_train.py): the staging kernel through the C-ABI against the numpy restatement of tests/test_host_path_train.py,
bitwise, through a sequence of restages of ONE buffer (dense fill, sparse resets, fewer items, none, weights); its refusals; then
end to end on the generated data set of tests/test_gpu_path_scores.py -- the gradient of the sequence loss against the fp64 oracle
on host-built prefix flows for scone, ebli, bunch and scone under -flip_edges 1, the pool's sparse reset against a dense fill, the
same bits as grad_step on every path's last item, train_paths beside the oracle's Adam, and the driver's -train_paths switch."""
import os

import numpy as np
import pytest
import torch

from oracle import scone_oracle as so
from scone_gcn_amd.synthetic_data_gen import SparseFlows
from tests.test_gpu_beam import HIDDEN, _close
from tests.test_gpu_parity import TOL, _maxdiff
from tests.test_gpu_path_scores import N_PATHS, _prefix_flows, _setup, case, data, run_steps    # noqa: F401  (data: the fixture)
from tests.test_host_path_scores import INT32_MAX, np_path_steps, same_floats
from tests.test_host_path_train import np_path_stage

pytestmark = pytest.mark.gpu

JUNK_F, JUNK_I = 7.5, -7


def _dev():
    return torch.device("cuda")


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(_dev())


def _p(x):
    from scone_gcn_amd import ops
    return None if x is None else ops._dev(x, x.dtype)


# ------------------------------------------------------------------------------------------------------------------
# 1. the kernel through the C-ABI: one buffer, five restages
# ------------------------------------------------------------------------------------------------------------------

def stage_calls(c):
    """The five chunks of the sequence: lists of (path, k) and the weights of the last.  Path 6 is the 70-node walk, path 2 has two
    nodes, path 7 does not exist."""
    lens = np.diff(c["ptr"])
    assert lens.tolist() == [0, 1, 2, 5, 9, 9, 70]
    a = [(2, 1), (3, 5), (6, 70), (6, 40), (6, 40), (7, 3), (4, 4), (6, 69), (5, 9), (3, 2), (6, 23)]     # k = 1, k = len, a twin, a guard
    b = [(6, 55), (6, 12), (-1, 2), (4, 8), (4, 2), (6, 64), (5, 3), (6, 31), (3, 4), (2, 2), (6, 47)]
    cc = [(6, 70), (5, 5), (6, 9)]
    e = [(6, 18), (3, 3), (6, 66), (2, 1), (5, 9), (6, 66), (4, 6), (1, 1), (6, 37)]
    w = (0.125 * (1 + np.arange(len(e)))).astype(np.float32)
    return [(a, None), (b, None), (cc, None), ([], None), (e, w)]


def run_sequence(c, st_dev, calls, sparse):
    """The calls on one buffer of S + 1 slabs (the last one is not the calls'): [(x, last, y) on the host after every call]."""
    from scone_gcn_amd import _lib, ops
    lib = _lib.load()
    d, n_rows, P = c["d"], c["n_rows"], len(c["ptr"]) - 1
    S = 3
    x = torch.full((S + 1, n_rows, 4, 1), JUNK_F, device=_dev())
    last = torch.full((4 * S + 4,), JUNK_I, device=_dev(), dtype=torch.int32)
    y = torch.full((4 * S + 4, d), JUNK_F, device=_dev())
    ptr_d, nodes_d = _t(c["ptr"], np.int32), _t(c["nodes"], np.int32)
    prev, out = None, []
    for items, w in calls:
        ip = _t([p for p, _ in items], np.int32) if items else None
        il = _t([k for _, k in items], np.int32) if items else None
        wd = None if w is None else _t(w, np.float32)
        n_prev = len(prev[2]) if (sparse and prev is not None) else -1
        use_prev = n_prev > 0
        status = lib.scn_path_stage(len(items), S, _p(ip), _p(il), _p(wd), n_prev, _p(prev[0]) if use_prev else None,
                                    _p(prev[1]) if use_prev else None, P, _p(ptr_d), _p(nodes_d), _p(st_dev["slot"]), _p(st_dev["row"]),
                                    _p(st_dev["run"]), _p(st_dev["next_same"]), n_rows, 4, d, _p(x), _p(last), _p(y), ops._stream())
        assert status == 0
        torch.cuda.synchronize()
        prev = (ip, il, items)
        out.append((x.cpu().numpy(), last.cpu().numpy(), y.cpu().numpy()))
    return out


@pytest.mark.parametrize("kind", ["random", "full", "one"])
def test_stage_kernel_matches_the_restatement_through_restages(kind):
    c = case(kind)
    ptr, nodes, d, n_rows = c["ptr"], c["nodes"], c["d"], c["n_rows"]
    want = np_path_steps(ptr, nodes, c["deg"], c["node"], c["edge"], c["sign"], n_rows)
    assert want["err"] == INT32_MAX
    got = run_steps(c)
    st_dev = {k: _t(got[k], np.float32 if k == "run" else np.int32) for k in ("slot", "row", "run", "next_same")}
    calls = stage_calls(c)
    S = 3
    assert [len(items) for items, _ in calls] == [11, 11, 3, 0, 9]
    seq = run_sequence(c, st_dev, calls, sparse=True)
    cancelled = 0
    for (items, w), (x, last, y) in zip(calls, seq):
        ip, il = [p for p, _ in items], [k for _, k in items]
        wx, wl, wy = np_path_stage(S, ip, il, w, ptr, nodes, want["slot"], want["row"], want["run"], want["next_same"], n_rows, d)
        assert same_floats(x[:S], wx)
        assert (x[S] == JUNK_F).all() and (last[4 * S:] == JUNK_I).all() and (y[4 * S:] == JUNK_F).all()   # the slab behind: untouched
        assert last.dtype == np.int32 and np.array_equal(last[:4 * S], wl)
        assert same_floats(y[:4 * S], wy)
        for i, (p, k) in enumerate(items):                          # the explicit zeros of cancelled edges are written, not skipped
            if 0 <= p < len(ptr) - 1:
                end = int(ptr[p]) + k - 1
                cancelled += sum(1 for t in range(int(ptr[p]), end)
                                 if want["row"][t] >= 0 and want["next_same"][t] >= end and want["run"][t] == 0)
        if w is not None:                                           # the weights arrive in the rows; (2, 1) has a target, (1, 1) none
            assert y[0].max() == w[0] and y[3].max() == w[3] and not y[7].any() and (wy[:len(items)].max(axis=1) > 0).sum() == 7
    assert kind == "one" or cancelled > 0
    # columns 3 .. 10 of the third call came back to zero, and the fourth call left nothing
    cols = lambda x: x[:S, :, :, 0].transpose(0, 2, 1).reshape(4 * S, n_rows)
    assert cols(seq[0][0])[3:11].any() and cols(seq[1][0])[3:11].any()
    assert not cols(seq[2][0])[3:].any() and not seq[3][0][:S].any() and not seq[3][2][:4 * S].any() and not seq[3][1][:4 * S].any()
    # the dense fill throughout, and the whole sequence a second time: the same bytes
    for other in (run_sequence(c, st_dev, calls, sparse=False), run_sequence(c, st_dev, calls, sparse=True)):
        for (x, last, y), (x2, last2, y2) in zip(seq, other):
            assert same_floats(x, x2) and np.array_equal(last, last2) and same_floats(y, y2)


# ------------------------------------------------------------------------------------------------------------------
# 2. refusals
# ------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_before_any_launch():
    from scone_gcn_amd import _lib, ops
    lib = _lib.load()
    i = torch.zeros((64,), device=_dev(), dtype=torch.int32)
    f = torch.full((64,), JUNK_F, device=_dev())
    pi, pf, st = _p(i), _p(f), ops._stream()
    BAD_SHAPE = -2

    def stage(n=1, n_slabs=1, n_prev=-1, ns=4, d=3, x=pf, last=pi, y=pf, ip=pi, prev=pi, row=pi, n_rows=8):
        return lib.scn_path_stage(n, n_slabs, ip, pi, None, n_prev, prev, pi, 1, pi, pi, pi, row, pf, pi, n_rows, ns, d, x, last, y, st)
    assert stage(x=None) == stage(last=None) == stage(y=None) == stage(ip=None) == stage(row=None) == _lib.SCN_ERR_BAD_ARG
    assert stage(n_prev=1, prev=None) == _lib.SCN_ERR_BAD_ARG
    assert stage(x=_p(f[1:])) == _lib.SCN_ERR_BAD_ARG                              # not 16-byte aligned
    assert stage(ns=1) == stage(ns=8) == _lib.SCN_ERR_UNSUPPORTED
    assert stage(n=5, n_slabs=1) == stage(n_prev=5, n_slabs=1) == stage(d=0) == stage(n=-1) == stage(n_slabs=-1) == BAD_SHAPE
    assert stage(n_rows=0) == BAD_SHAPE
    assert stage(n=0, n_slabs=0, n_prev=0) == 0 and stage(n=0, n_slabs=0, n_prev=0, x=None, last=None, y=None) == 0
    assert stage(n=1, n_slabs=0) == BAD_SHAPE
    torch.cuda.synchronize()
    assert (f.cpu().numpy() == JUNK_F).all() and not i.cpu().numpy().any()         # nothing was launched


# ------------------------------------------------------------------------------------------------------------------
# end to end: generate_dataset(150, 45), the first 11 paths prefix + [target]: 59 items at min_prefix = 2
# ------------------------------------------------------------------------------------------------------------------

def _items(s, min_prefix=2):
    from scone_gcn_amd import path_scores
    ptr, nodes = path_scores.ragged(s["paths"])
    item_ptr, item_path, item_len = path_scores.path_items(ptr, min_prefix)
    return ptr, nodes, item_ptr, item_path, item_len


def _oracle(data, s, model_type, hidden=None):
    """(loss_and_grad(w, last, flows (M, E), y (M, D), weight_decay)) of the fp64 oracle on the complex of `s`."""
    from scone_gcn_amd import dataset_io
    import scipy.sparse as sp
    cwd = os.getcwd()
    os.chdir(data["dir"])
    try:
        _, (B1, B2), *_ = dataset_io.load_dataset("trajectory_data_1hop_ps")
    finally:
        os.chdir(cwd)
    B1, B2 = (np.asarray(sp.csr_matrix(m).toarray(), np.float64) for m in (B1, B2))
    nb, _ = so.neighborhoods(np.asarray(s["sc"].cx.edges), B1.shape[0])
    if model_type == "bunch":
        shifts = so.bunch_shifts(B1, B2)
        return lambda w, last, X, y, wd: so.bunch_loss_and_grad(w, shifts, nb, last, X[:, :, None], y[:, :, None], np.ones(len(last), int), wd)
    F = None if s["flips"] is None else np.diag(s["flips"])
    S = so.ebli_shifts(B1, B2, F) if model_type == "ebli" else so.scone_shifts(B1, B2, F)        # ebli: as tests/test_gpu_parity.py
    Bc = so.make_Bconds(B1, nb, F)
    act = "leaky_relu" if model_type == "ebli" else "tanh"
    return lambda w, last, X, y, wd: so.scone_loss_and_grad(w, S[0], S[1], Bc, last, X[:, :, None], y[:, :, None],
                                                            np.ones(len(last), int), wd, act)


def _targets(s, sel, weight, min_prefix=2):
    """The oracle's inputs for the items sel: (last, flows, y) with y the weighted one-hot rows TIMES len(sel) / sum(w): the
    oracle's loss is a mean over its rows (-sum <logp, y> / N), the sequence loss a weighted mean (-sum w logp / sum w)."""
    from scone_gcn_amd import path_train
    ptr, nodes, item_ptr, item_path, item_len = _items(s, min_prefix)
    w = path_train.item_weights(item_ptr, item_path, weight).astype(np.float64)[sel]
    ip, il = item_path[sel], item_len[sel]
    last = nodes[ptr[ip] + il - 1]
    nxt = nodes[ptr[ip] + il]
    nb = s["nbrhoods"]
    y = np.zeros((len(sel), nb.shape[1]), np.float64)
    for i, (v, u) in enumerate(zip(last, nxt)):
        y[i, list(nb[v]).index(u)] = w[i] * len(sel) / w.sum()
    return last, _prefix_flows(s, s["paths"], ip, il), y


def _fresh_net(s, model_type, hidden=None, weights=None, batch=8, wd=0.0, epochs=1, lr=1e-3):
    """A trainer of its own on the operators of `s` (the shared one of _setup stays unchanged), with the same weights unless given."""
    from scone_gcn_amd import scone_trajectory_model as stm
    old = s["net"]
    net = stm.Scone_GCN(epochs, lr, batch, wd, verbose=False)
    D = s["nbrhoods"].shape[1]
    net.setup(old.model, hidden or HIDDEN[model_type], old.shifts, s["inputs"], np.zeros((1, D, 1)), None, np.ones(1), model_type=model_type)
    net._install(weights if weights is not None else [w.cpu().numpy() for w in old.weights])
    stm.reseed(1030)
    return net


def _grad(net):
    torch.cuda.synchronize()
    return net._flat_g.cpu().numpy().copy()


def _check_grad(net, ref_loss, ref_g, loss):
    assert _close(float(loss), ref_loss, TOL)
    for k, g in enumerate(net._grads):
        assert _maxdiff(g.cpu().numpy(), ref_g[k]) <= TOL, "weight %d" % k


@pytest.mark.parametrize("small", [True, False], ids=["one-launch", "layers"])
@pytest.mark.parametrize("weight", ["step", "path"])
@pytest.mark.parametrize("model_type,flip", [("scone", False), ("ebli", False), ("bunch", False), ("scone", True)],
                         ids=["scone", "ebli", "bunch", "scone-flipped"])
def test_sequence_gradient_follows_the_oracle(data, monkeypatch, model_type, flip, weight, small):
    """"one-launch": every micro-batch of a scone plan is taken by SconePlan.small_step; "layers": small_step and the cone step both
    decline (|E| = 370), so forward / scn_masked_ce_begin / backward read the staged buffers.  The routes are asserted from what the
    two calls returned.  A Bunch plan has neither call: both ids run its layer kernels, kept so that every model sees both settings."""
    from scone_gcn_amd import ops
    s = _setup(data, model_type, flip)
    monkeypatch.setattr(ops, "SMALL_STEP", small)
    routes = {"small_step": [], "step": []}
    for name in routes:
        def spy(self, *a, _real=getattr(ops.SconePlan, name), _log=routes[name], **k):
            _log.append(bool(_real(self, *a, **k)))
            return _log[-1]
        monkeypatch.setattr(ops.SconePlan, name, spy)
    key = ("seq-oracle", model_type, flip, weight)
    if key not in data:                                                          # the reference: once per (model, weight)
        fn = _oracle(data, s, model_type)
        w64 = [w.cpu().numpy().astype(np.float64) for w in s["net"].weights]
        data[key] = fn(w64, *_targets(s, np.arange(59), weight), 0.0)
    ref_loss, ref_g = data[key]
    net = _fresh_net(s, model_type)
    net.path_micro_batch = 8                                                     # eight micro-batches, the last slab partial
    ps = net.path_set(s["inputs"], s["paths"])
    item_ptr, item_path, item_len = ps.items(2)
    assert len(item_path) == 59 and np.array_equal(item_path, _items(s)[3]) and np.array_equal(item_len, _items(s)[4])
    loss = net.path_grad_step(s["inputs"], ps, np.arange(59), apply=False, weight=weight)
    assert loss.dim() == 0 and loss.is_cuda
    _check_grad(net, ref_loss, ref_g, loss)
    plan = net._plan(s["inputs"])
    if model_type == "bunch":
        assert type(plan) is ops.BunchPlan and routes == {"small_step": [], "step": []}
    elif model_type == "scone":
        assert type(plan) is ops.SconePlan
        assert routes == ({"small_step": [True] * 8, "step": []} if small else {"small_step": [False] * 8, "step": [False] * 8})
    else:                                                                        # ebli: whichever plan its operators get; off: the layer kernels
        assert small or not any(routes["small_step"] + routes["step"])
    assert [b["x"].shape[0] for b in net._path_pool.bufs] == [2] * 7 + [1]          # 7 x 8 items and 3: what stage() would hold
    assert max(np.abs(g).max() for g in ref_g) > 1e-3                            # (not trivially zero)
    for a, b in zip(net.weights, s["net"].weights):                              # apply=False: the weights stand
        assert torch.equal(a, b)
    # the value the scoring call reports is the loss that was differentiated
    assert _close(net.path_loss(s["inputs"], s["paths"], weight=weight), ref_loss, TOL)


def test_sequence_gradient_hidden_32(data):
    s = _setup(data, "scone")
    hidden = [(3, 32)] * 3
    rs = np.random.RandomState(17)
    w = [0.3 * rs.randn(*sh) for sh in so.weight_shapes(1, hidden, 1)]
    net = _fresh_net(s, "scone", hidden=hidden, weights=w)
    net.path_micro_batch = 8
    w64 = [a.cpu().numpy().astype(np.float64) for a in net.weights]
    ref_loss, ref_g = _oracle(data, s, "scone")(w64, *_targets(s, np.arange(59), "path"), 0.0)
    ps = net.path_set(s["inputs"], s["paths"])
    loss = net.path_grad_step(s["inputs"], ps, np.arange(59), apply=False, weight="path")
    _check_grad(net, ref_loss, ref_g, loss)


# ------------------------------------------------------------------------------------------------------------------
# 4. / 5. the pool's sparse reset; the same bits as grad_step
# ------------------------------------------------------------------------------------------------------------------

def test_sparse_reset_of_the_pool_gives_the_bits_of_a_dense_fill(data, monkeypatch):
    from scone_gcn_amd import ops
    s = _setup(data, "scone")
    A, B = np.arange(0, 40), np.arange(20, 59)

    def steps(seq):
        net = _fresh_net(s, "scone")
        net.path_micro_batch = 8
        ps = net.path_set(s["inputs"], s["paths"])
        out = []
        for sel in seq:
            loss = net.path_grad_step(s["inputs"], ps, sel, apply=False)
            out.append((_grad(net), float(loss)))
        return net, out
    net, (ga, gb) = steps([A, B])
    assert all(b["prev"] is not None for b in net._path_pool.bufs) and len(net._path_pool.bufs) == 5
    assert [int(b["prev"][0].shape[0]) for b in net._path_pool.bufs] == [8, 8, 8, 8, 7]
    _, (alone,) = steps([B])
    assert same_floats(gb[0], alone[0]) and gb[1] == alone[1]
    assert not np.array_equal(ga[0], gb[0])
    monkeypatch.setattr(ops, "PATH_STAGE_SPARSE_CLEAR", False)
    _, (_, dense) = steps([A, B])
    assert same_floats(gb[0], dense[0]) and gb[1] == dense[1]
    monkeypatch.setattr(ops, "PATH_STAGE_SPARSE_CLEAR", True)
    # another path set on the same trainer: the remembered items index the old set's records, so nothing carries over
    rev = s["paths"][::-1]
    fresh = _fresh_net(s, "scone")
    got = []
    for trainer in (net, fresh):
        trainer.path_micro_batch = 8
        ps = trainer.path_set(s["inputs"], rev)
        loss = trainer.path_grad_step(s["inputs"], ps, B, apply=False)
        assert trainer._path_pool.ps is ps
        got.append((_grad(trainer), float(loss)))
    assert same_floats(got[0][0], got[1][0]) and got[0][1] == got[1][1] and not np.array_equal(got[0][0], gb[0])
    net.drop_path_stage()
    assert net._path_pool is None
    # setup() again means another plan: the buffers go with the old one
    assert fresh._path_pool is not None
    fresh.setup(fresh.model, HIDDEN["scone"], fresh.shifts, s["inputs"], np.zeros((1, s["nbrhoods"].shape[1], 1)), None, np.ones(1),
                model_type="scone")
    assert fresh._path_pool is None
    from scone_gcn_amd import scone_trajectory_model as stm
    stm.reseed(1030)                                                             # (setup drew weights from the module stream)


def test_last_items_give_the_bits_of_grad_step(data):
    s = _setup(data, "scone")
    nb, paths = s["nbrhoods"], s["paths"]
    net = _fresh_net(s, "scone")
    assert net.path_micro_batch is None                                         # both sides cut by one rule
    y = np.zeros((N_PATHS, nb.shape[1], 1))
    for i, p in enumerate(paths):
        y[i, list(nb[p[-2]]).index(p[-1]), 0] = 1.0
    loss_a = net.grad_step(s["inputs"], y, np.ones(N_PATHS, int), apply=False)
    ga, la = _grad(net), float(loss_a)
    ps = net.path_set(s["inputs"], paths)
    item_ptr, _, item_len = ps.items(2)
    last_items = item_ptr[1:] - 1
    assert np.array_equal(item_len[last_items], [len(p) - 1 for p in paths])
    net._flat_g.fill_(3.0)
    loss_b = net.path_grad_step(s["inputs"], ps, last_items, apply=False)
    gb, lb = _grad(net), float(loss_b)
    assert same_floats(ga, gb) and la == lb and np.abs(ga).max() > 1e-3


# ------------------------------------------------------------------------------------------------------------------
# 6. train_paths beside the oracle's Adam
# ------------------------------------------------------------------------------------------------------------------

def test_train_paths_follows_oracle_adam_and_repeats_bitwise(data):
    from scone_gcn_amd import path_train, scone_trajectory_model as stm
    s = _setup(data, "scone")
    wd, lr = 5e-5, 1e-3
    fn = _oracle(data, s, "scone")
    mask = np.ones(N_PATHS, int)

    def run(spy):
        net = _fresh_net(s, "scone", batch=16, wd=wd, epochs=2, lr=lr)
        before = net.path_loss(s["inputs"], s["paths"], mask)
        log = []
        if spy:
            orig = net.path_grad_step

            def path_grad_step(inputs, ps, items, **kw):
                w64 = [w.cpu().numpy().astype(np.float64) for w in net.weights]
                loss = orig(inputs, ps, items, **kw)
                log.append((np.array(items), float(loss), w64, net._step))
                return loss
            net.path_grad_step = path_grad_step
        stm.reseed(1030)
        scores = net.train_paths(s["inputs"], s["paths"], mask, mask)
        torch.cuda.synchronize()
        return net, before, scores, log
    net, before, scores, log = run(True)
    assert net._path_pool is None                                                # the run's buffers are freed with it
    assert net.trained and len(log) == 6 and [r[3] for r in log] == [1, 2, 3, 4, 5, 6]      # (_step after the step: i + 1)
    rs = np.random.RandomState(1030)
    batches = path_train.epoch_batches(rs, 59, 16) + path_train.epoch_batches(rs, 59, 16)
    adam = so.Adam(log[0][2], lr)
    for i in range(3):
        items, loss, w64, _ = log[i]
        assert np.array_equal(items, batches[i]) and len(items) == 16
        ridge = wd * so.ridge(adam.x)
        ref_loss, g = fn(adam.x, *_targets(s, items, "step"), wd)
        assert _close(loss + ridge, ref_loss, TOL), "step %d" % i
        adam.update(i, g)
    assert all(np.array_equal(r[0], b) for r, b in zip(log, batches))
    after = net.path_loss(s["inputs"], s["paths"], mask)
    assert after < before
    assert scores[0] == scores[1] == net.score_paths(s["inputs"], s["paths"], mask)
    assert _close(-scores[0]["mean_step_logp"] + wd * float((net._flat_w.double() ** 2).sum()), after, 1e-12)
    net2, before2, scores2, _ = run(False)
    assert before2 == before and scores2 == scores
    assert same_floats(net._flat_w.cpu().numpy(), net2._flat_w.cpu().numpy())
    stm.reseed(1030)


# ------------------------------------------------------------------------------------------------------------------
# 7. the driver
# ------------------------------------------------------------------------------------------------------------------

def test_train_model_train_paths_switch(tmp_path, monkeypatch):
    from scone_gcn_amd import dataset_io, scone_trajectory_model as stm, trajectory_experiments as te
    monkeypatch.chdir(tmp_path)
    dataset_io.generate_dataset(150, 45, folder="drv", holes=True)
    argv = ["prog", "-epochs", "1", "-batch_size", "12", "-data_folder_suffix", "drv", "-describe", "0", "-train_paths", "1"]
    hp = te.hyperparams(argv)
    seen = {}
    setup = te.data_setup

    def data_setup(*a, **kw):
        out = setup(*a, **kw)
        X = out[0][0][-1]
        seen["X"], seen["before"] = X, np.array(X.val if isinstance(X, SparseFlows) else X, copy=True)
        return out
    monkeypatch.setattr(te, "data_setup", data_setup)
    calls = []
    monkeypatch.setattr(stm.Scone_GCN, "train", lambda self, *a, **kw: calls.append("train"))
    real = stm.Scone_GCN.train_paths

    def train_paths(self, *a, **kw):
        calls.append(("train_paths", kw))
        return real(self, *a, **kw)
    monkeypatch.setattr(stm.Scone_GCN, "train_paths", train_paths)
    stm.reseed(1030)
    net, (train_loss, train_acc, test_loss, test_acc) = te.train_model(hp)
    assert calls == [("train_paths", {"min_prefix": 2, "weight": "step"})]
    assert net.trained and net._step > 1
    assert np.isfinite([train_loss, train_acc, test_loss, test_acc]).all() and 0.0 <= test_acc <= 1.0
    res = net.experiment_results
    assert {"train_2target", "test_2target", "log_probs"} <= set(res) and np.isfinite(res["log_probs"]).all()
    X = seen["X"]
    after = X.val if isinstance(X, SparseFlows) else X
    assert np.array_equal(seen["before"].view(np.uint8), np.asarray(after).view(np.uint8))              # the caller's flows: bitwise
    stm.reseed(1030)
