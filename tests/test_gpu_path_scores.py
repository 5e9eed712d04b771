"""Teacher-forced path scoring on the MI355X (csrc/scn_paths.hip; Scone_GCN.path_step_log_probs): each of the three kernels through
the C-ABI against the numpy restatement of tests/test_host_path_scores.py -- integers, run and step_logp bitwise, step_mass within
1e-5 of max(1, |fp64 value|) (HIP's expf / logf are not numpy's) -- with every output buffer pre-filled with junk; then end to end on
a generated data set against the fp64 oracle on host-built prefix flows, for scone, ebli, bunch and scone under -flip_edges 1."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import scone_oracle as so
from scone_gcn_amd.synthetic_data_gen import SparseFlows
from tests.test_gpu_beam import HIDDEN, _close
from tests.test_host_multihop import oracle_model
from tests.test_host_path_scores import INT32_MAX, flow_tables, np_path_score, np_path_slabs, np_path_steps, same_floats, tab_arrays

pytestmark = pytest.mark.gpu

N_PATHS = 11


# ------------------------------------------------------------------------------------------------------------------
# the kernels through the C-ABI
# ------------------------------------------------------------------------------------------------------------------

def _dev():
    return torch.device("cuda")


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(_dev())


def _p(x):
    from scone_gcn_amd import ops
    return None if x is None else ops._dev(x, x.dtype)


def tables(rs, n_nodes, d, n_rows, deg):
    """Random step tables: neighbours and rows repeat, so a pair can sit in two slots (the first wins) and edges recur."""
    deg = np.asarray(deg)
    live = np.arange(d)[None, :] < deg[:, None]
    step_node = np.where(live, rs.randint(0, n_nodes, size=(n_nodes, d)), -1)
    step_edge = np.where(live, rs.randint(0, n_rows, size=(n_nodes, d)), -1)
    step_sign = np.where(live, rs.choice([-1.0, 1.0], size=(n_nodes, d)), 0.0)
    return deg, step_node, step_edge, step_sign.astype(np.float32)


def walks(rs, lengths, deg, step_node):
    out = []
    for n in lengths:
        walk = [int(rs.randint(len(deg)))] if n else []
        while len(walk) < n:
            walk.append(int(step_node[walk[-1], rs.randint(deg[walk[-1]])]))
        out.append(walk)
    return out


def case(kind):
    from scone_gcn_amd import path_scores
    rs = np.random.RandomState({"random": 0, "full": 1, "one": 2}[kind])
    n_nodes, d, n_rows = 12, 5, 17
    deg = {"random": rs.randint(2, d + 1, size=n_nodes), "full": np.full(n_nodes, d), "one": np.ones(n_nodes, np.int64)}[kind]
    deg, sn, se, ss = tables(rs, n_nodes, d, n_rows, deg)
    ptr, nodes = path_scores.ragged(walks(rs, [0, 1, 2, 5, 9, 9, 70], deg, sn))
    return dict(ptr=ptr, nodes=nodes, deg=deg, node=sn, edge=se, sign=ss, n_nodes=n_nodes, d=d, n_rows=n_rows, rs=rs)


def run_steps(c, nodes=None, edge=None):
    from scone_gcn_amd import _lib, ops
    lib = _lib.load()
    nodes = c["nodes"] if nodes is None else nodes
    T = len(nodes)
    ins = [_t(c["ptr"], np.int32), _t(nodes, np.int32), _t(c["deg"], np.int32), _t(c["node"], np.int32),
           _t(c["edge"] if edge is None else edge, np.int32), _t(c["sign"], np.float32)]
    slot, row, nxt = (torch.full((T,), -7, device=_dev(), dtype=torch.int32) for _ in range(3))
    run = torch.full((T,), 7.5, device=_dev())
    err = torch.full((1,), INT32_MAX, device=_dev(), dtype=torch.int32)
    status = lib.scn_path_steps(len(c["ptr"]) - 1, _p(ins[0]), _p(ins[1]), c["n_nodes"], c["d"], _p(ins[2]), _p(ins[3]), _p(ins[4]),
                                _p(ins[5]), c["n_rows"], _p(slot), _p(row), _p(run), _p(nxt), _p(err), ops._stream())
    assert status == 0
    torch.cuda.synchronize()
    return dict(slot=slot.cpu().numpy(), row=row.cpu().numpy(), run=run.cpu().numpy(), next_same=nxt.cpu().numpy(), err=int(err.item()))


def same_steps(got, want):
    assert got["err"] == want["err"]
    for key in ("slot", "row", "next_same"):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), key
    assert same_floats(got["run"], want["run"])


@pytest.mark.parametrize("kind", ["random", "full", "one"])
def test_kernels_match_the_restatement(kind):
    from scone_gcn_amd import _lib, ops, path_scores
    lib = _lib.load()
    c = case(kind)
    ptr, nodes, d, n_rows = c["ptr"], c["nodes"], c["d"], c["n_rows"]
    want = np_path_steps(ptr, nodes, c["deg"], c["node"], c["edge"], c["sign"], n_rows)
    assert want["err"] == INT32_MAX
    got = run_steps(c)
    same_steps(got, want)
    assert np.abs(want["run"]).max() >= 2 and (want["next_same"] != INT32_MAX).sum() > 20          # edges do repeat
    assert kind == "one" or (want["run"][want["row"] >= 0] == 0).any()                             # ... and cancel
    same_steps(run_steps(c), got)                                                                  # a second call: the same bytes
    # slabs and scores: chunks of 11 items (a partial last slab), chunk boundaries inside the paths
    _, item_path, item_len = path_scores.path_items(ptr, 1)
    M = len(item_path)
    assert M == 0 + 0 + 1 + 4 + 8 + 8 + 69
    rs = c["rs"]
    logp = (-0.25 * rs.randint(0, 6, size=(M, d))).astype(np.float32)                              # a 0.25 grid: ranks tie
    logp[3, :] = np.nan
    logp[4, 1], logp[5, 0], logp[6, :] = np.nan, np.inf, -np.inf
    logp[7, 2], logp[8, 0] = -np.inf, np.nan
    dev_in = [_t(ptr, np.int32), _t(nodes, np.int32), _t(c["deg"], np.int32)]
    st = {k: _t(got[k], np.float32 if k == "run" else np.int32) for k in ("slot", "row", "run", "next_same")}
    n_chunks = 0
    for c0 in range(0, M, 11):
        ip, il = item_path[c0:c0 + 11], item_len[c0:c0 + 11]
        n = len(ip)
        S = (n + 3) // 4
        ip_d, il_d = _t(ip, np.int32), _t(il, np.int32)
        x = torch.full((S + 1, n_rows, 4, 1), 7.5, device=_dev())                                  # one slab more than the call owns
        assert lib.scn_path_slabs(n, S, _p(ip_d), _p(il_d), len(ptr) - 1, _p(dev_in[0]), _p(st["row"]), _p(st["run"]),
                                  _p(st["next_same"]), n_rows, 4, _p(x), ops._stream()) == 0
        lp_d = _t(logp[c0:c0 + n], np.float32)
        outs = [torch.full((n,), 7.5, device=_dev()), torch.full((n,), -7, device=_dev(), dtype=torch.int32),
                torch.full((n,), 7.5, device=_dev())]
        assert lib.scn_path_score(n, d, _p(ip_d), _p(il_d), len(ptr) - 1, _p(dev_in[0]), _p(dev_in[1]), _p(st["slot"]), _p(dev_in[2]),
                                  c["n_nodes"], _p(lp_d), _p(outs[0]), _p(outs[1]), _p(outs[2]), ops._stream()) == 0
        torch.cuda.synchronize()
        xs = x.cpu().numpy()
        assert same_floats(xs[:S], np_path_slabs(S, ip, il, ptr, want["row"], want["run"], want["next_same"], n_rows))
        assert (xs[S] == 7.5).all()
        w_lp, w_rank, w_mass = np_path_score(ip, il, ptr, nodes, want["slot"], c["deg"], logp[c0:c0 + n])
        g_lp, g_rank, g_mass = (o.cpu().numpy() for o in outs)
        assert same_floats(g_lp, w_lp) and g_rank.dtype == np.int32 and np.array_equal(g_rank, w_rank)
        fin = np.isfinite(w_mass)
        assert np.array_equal(g_mass[~fin].astype(np.float64), w_mass[~fin], equal_nan=True)       # NaN stays NaN, an infinity itself
        assert np.all(np.abs(g_mass[fin] - w_mass[fin]) <= 1e-5 * np.maximum(1.0, np.abs(w_mass[fin])))
        if c0 == 0:
            assert n == 11 and np.isnan(w_mass[3]) and w_mass[5] == np.inf and w_mass[6] == -np.inf
            assert w_rank.max() > 0 or kind == "one"                                                # (a single slot is always first)
            assert len(set(ip.tolist())) > 1 and ip[-1] == item_path[c0 + 11]                      # the boundary cuts a path
        n_chunks += 1
    assert n_chunks == 9 and M % 11 % 4 != 0


def test_error_word_takes_the_lowest_position_and_nothing_else_changes():
    c = case("random")
    ptr, nodes = c["ptr"], c["nodes"].copy()
    clean = np_path_steps(ptr, nodes, c["deg"], c["node"], c["edge"], c["sign"], c["n_rows"])
    t0 = int(ptr[6])                                                              # the 70-node walk
    # a row out of range on a step the walk takes, an id past the table, and a pair that is no neighbour
    edge = c["edge"].copy()
    t_row = t0 + 40
    edge[nodes[t_row], clean["slot"][t_row]] = c["n_rows"]
    nodes[t0 + 30] = c["n_nodes"] + 3
    v = int(nodes[t0 + 10])
    nodes[t0 + 11] = next(u for u in range(c["n_nodes"]) if u not in c["node"][v][:c["deg"][v]])
    want = np_path_steps(ptr, nodes, c["deg"], c["node"], edge, c["sign"], c["n_rows"])
    is_step = np.ones(len(nodes), bool)
    is_step[ptr[1:][np.diff(ptr) > 0] - 1] = False
    bad = np.flatnonzero(is_step & (want["slot"] < 0))
    assert set([t0 + 10, t0 + 29, t0 + 30, t_row]) <= set(bad.tolist()) and want["err"] == bad.min() <= t0 + 10
    got = run_steps(c, nodes, edge)
    same_steps(got, want)
    same_steps(run_steps(c, nodes, edge), got)
    ok = want["slot"] >= 0                                                        # a step that is fine keeps its slot and its row
    assert np.array_equal(got["slot"][ok], clean["slot"][ok]) and np.array_equal(got["row"][ok], clean["row"][ok])
    assert (got["run"][~ok] == 0).all() and (got["next_same"][~ok] == INT32_MAX).all()
    if bad.min() == t0 + 10:                                                      # without the first: the next one
        nodes[t0 + 11] = c["nodes"][t0 + 11]
        assert run_steps(c, nodes, edge)["err"] == bad[bad > t0 + 11].min()


def test_bad_arguments_are_refused():
    from scone_gcn_amd import _lib, ops
    lib = _lib.load()
    i = torch.zeros((64,), device=_dev(), dtype=torch.int32)
    f = torch.zeros((64,), device=_dev())
    pi, pf, st = _p(i), _p(f), ops._stream()
    BAD_SHAPE = -2

    def steps(n=1, ptr=pi, n_nodes=4, slot=pi):
        return lib.scn_path_steps(n, ptr, pi, n_nodes, 3, pi, pi, pi, pf, 8, slot, pi, pf, pi, pi, st)

    def slabs(n=1, n_slabs=1, ns=4, x=pf, row=pi):
        return lib.scn_path_slabs(n, n_slabs, pi, pi, 1, pi, row, pf, pi, 8, ns, x, st)

    def score(n=1, d=3, logp=pf, rank=pi):
        return lib.scn_path_score(n, d, pi, pi, 1, pi, pi, pi, pi, 4, logp, pf, rank, pf, st)
    assert steps(n=0) == 0 and slabs(n=0) == 0 and score(n=0) == 0
    assert steps(n=0, ptr=None) == 0 and score(n=0, logp=None) == 0                # nothing is looked at
    assert steps(ptr=None) == steps(slot=None) == _lib.SCN_ERR_BAD_ARG
    assert slabs(x=None) == slabs(row=None) == _lib.SCN_ERR_BAD_ARG
    assert slabs(x=_p(f[1:])) == _lib.SCN_ERR_BAD_ARG                              # not 16-byte aligned
    assert score(logp=None) == score(rank=None) == _lib.SCN_ERR_BAD_ARG
    assert steps(n=-1) == steps(n_nodes=0) == slabs(n=-1) == slabs(n=5, n_slabs=1) == score(n=-1) == score(d=0) == BAD_SHAPE
    assert slabs(ns=8) == slabs(ns=1) == _lib.SCN_ERR_UNSUPPORTED
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------
# end to end: generate_dataset(150, 45), the first 11 paths prefix + [target]: 59 items at min_prefix = 2
# ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from scone_gcn_amd import dataset_io
    d = tmp_path_factory.mktemp("pathscores")
    cwd = os.getcwd()
    os.chdir(d)
    try:
        dataset_io.generate_dataset(150, 45, folder="ps", holes=True)
    finally:
        os.chdir(cwd)
    return {"dir": str(d)}


def _setup(data, model_type, flip=False, seed=3):
    """One model and one oracle per (type, flip), shared and unchanged: the weights of tests/test_gpu_beam.py::_setup."""
    key = (model_type, flip)
    if key in data:
        return data[key]
    from scone_gcn_amd import dataset_io, scone_trajectory_model as stm, trajectory_experiments as te
    from scone_gcn_amd.scone_trajectory_model import Scone_GCN
    cwd = os.getcwd()
    os.chdir(data["dir"])
    try:
        hp = te.hyperparams(["prog", "-model", model_type, "-flip_edges", "1" if flip else "0"])
        out = te.data_setup(hops=(1, 2), folder_suffix="ps", hp=hp)
        _, (B1, B2), *_ = dataset_io.load_dataset("trajectory_data_1hop_ps")
    finally:
        os.chdir(cwd)
        stm.reseed(1030)
    inputs_all, y_all, train_mask, test_mask, shifts, G, E_lookup, nbrhoods, n_nbrs, targets_all, prefixes = out
    net = Scone_GCN(1, 1e-3, 8, 0.0, verbose=False)
    net.setup(te.MODEL_FUNCS[model_type], HIDDEN[model_type], shifts, inputs_all[0], y_all[0], None, train_mask, model_type=model_type)
    rs = np.random.RandomState(seed)
    scale = 0.05 if model_type == "ebli" else 0.4
    w = [scale * rs.randn(*s) for s in so.weight_shapes(1, HIDDEN[model_type], 1, model_type)]
    net._install(w)
    flips = None if model_type == "bunch" else inputs_all[0][0].flips
    assert (flips is not None and (flips < 0).any()) == flip
    B1, B2 = (np.asarray(sp.csr_matrix(m).toarray(), np.float64) for m in (B1, B2))
    edges = np.array(sorted(E_lookup, key=E_lookup.get))
    fn = oracle_model(model_type, w, B1, B2, edges, B1.shape[0], flips)
    idx = np.arange(N_PATHS)
    X = inputs_all[0][-1]
    Xs = X.select(idx) if isinstance(X, SparseFlows) else np.asarray(X)[idx]
    sub = [inputs_all[0][0], inputs_all[0][1][idx], Xs]
    paths = [[int(v) for v in prefixes[i]] + [int(targets_all[0][i])] for i in idx]
    net.multi_hop_micro_batch = 8                                              # paths straddle chunks, the last slab is partial
    data[key] = dict(net=net, fn=fn, inputs=sub, paths=paths, sc=G.complex, flips=flips, nbrhoods=np.asarray(nbrhoods))
    return data[key]


def _prefix_flows(s, paths, item_path, item_len):
    from scone_gcn_amd import synthetic_data_gen as g
    from scone_gcn_amd.trajectory_experiments import apply_flips
    prefixes = [paths[p][:k] for p, k in zip(item_path, item_len)]
    return apply_flips(g.paths_to_flows(s["sc"].cx, prefixes), s["flips"]).todense()[:, :, 0].astype(np.float64)


def _traced(net, *args, **kw):
    net._multi_hop_trace = trace = []
    try:
        out = net.path_step_log_probs(*args, **kw)
    finally:
        del net._multi_hop_trace
    return out, trace


def _check(s, paths, min_prefix=2):
    """The checks of one call against the oracle and the restatement; returns the scores."""
    from scone_gcn_amd import path_scores
    net, nb = s["net"], s["nbrhoods"]
    sc, trace = _traced(net, s["inputs"], paths, min_prefix=min_prefix)
    ptr, nodes = path_scores.ragged(paths)
    item_ptr, item_path, item_len = path_scores.path_items(ptr, min_prefix)
    M = len(item_path)
    assert np.array_equal(sc.ptr, item_ptr) and sc.ptr.dtype == np.int64 and np.array_equal(sc.prefix_len, item_len)
    assert sc.logp.shape == sc.mass.shape == sc.rank.shape == (M,) and sc.logp.dtype == sc.mass.dtype == np.float64 and sc.rank.dtype == np.int64
    assert len(trace) == -(-M // 8) and [r["item0"] for r in trace] == list(range(0, M, 8))
    flows = _prefix_flows(s, paths, item_path, item_len)
    last = nodes[ptr[item_path] + item_len - 1]
    assert np.array_equal(np.concatenate([r["flows"] for r in trace]), flows.astype(np.float32))          # the columns, exactly
    assert np.array_equal(np.concatenate([r["last"] for r in trace]), last)
    ref = s["fn"](last, flows)                                                                            # (M, D) fp64
    nxt = nodes[ptr[item_path] + item_len]
    slot = np.array([list(nb[v]).index(u) for v, u in zip(last, nxt)])
    assert _close(sc.logp, ref[np.arange(M), slot])
    # rank and mass: the restatement on the device's own rows; no exclusions, no tie margin
    rows = np.concatenate([r["logp"] for r in trace])
    deg = (nb >= 0).sum(axis=1)
    deg_t, node_t, edge_t, sign_t = tab_arrays(flow_tables(s["sc"].cx, nb, np.arange(s["sc"].cx.n_edges), s["flips"]))
    st = np_path_steps(ptr, nodes, deg_t, node_t, edge_t, sign_t, s["sc"].cx.n_edges)
    assert np.array_equal(st["slot"][ptr[item_path] + item_len - 1], slot)
    w_lp, w_rank, w_mass = np_path_score(item_path, item_len, ptr, nodes, st["slot"], deg, rows)
    assert np.array_equal(sc.logp, w_lp.astype(np.float64)) and np.array_equal(sc.rank, w_rank)
    assert _close(sc.mass, w_mass) and np.all(sc.mass <= 1e-5)                                            # a share of a distribution
    return sc


@pytest.mark.parametrize("model_type,flip", [("scone", False), ("ebli", False), ("bunch", False), ("scone", True)],
                         ids=["scone", "ebli", "bunch", "scone-flipped"])
def test_step_log_probs_follow_the_oracle(data, model_type, flip):
    s = _setup(data, model_type, flip)
    net, paths, nb = s["net"], s["paths"], s["nbrhoods"]
    X = s["inputs"][-1]
    before = np.array(X.val if isinstance(X, SparseFlows) else X, copy=True)
    sc = _check(s, paths)
    assert len(sc.logp) == 59 and 4 <= min(len(p) for p in paths) - 1 and max(len(p) for p in paths) - 1 <= 10
    # every path's last item is the model's own 1-hop prediction of the target
    pred = net._predict(net.weights, s["inputs"]).cpu().numpy().astype(np.float64)
    for i, p in enumerate(paths):
        assert _close(sc.logp[sc.ptr[i + 1] - 1], pred[i, list(nb[p[-2]]).index(p[-1]), 0])
    # the reductions
    ll, n_steps = net.path_log_likelihood(s["inputs"], paths)
    assert np.array_equal(n_steps, np.diff(sc.ptr)) and ll.dtype == np.float64
    assert np.array_equal(ll, np.array([sc.logp[a:b].sum() for a, b in zip(sc.ptr[:-1], sc.ptr[1:])]))
    norm = net.path_step_log_probs(s["inputs"], paths, normalise=True)
    assert np.array_equal(norm.logp, sc.logp - sc.mass) and np.array_equal(norm.mass, sc.mass)
    mask = (np.arange(N_PATHS) % 3 != 0).astype(int)
    got = net.score_paths(s["inputs"], paths, mask)
    sel = np.concatenate([np.arange(sc.ptr[i], sc.ptr[i + 1]) for i in np.flatnonzero(mask)])
    mean = float(sc.logp[sel].sum() / len(sel))
    assert got == {"mean_step_logp": mean, "perplexity": float(np.exp(-mean)), "accuracy": float(np.mean(sc.rank[sel] == 0)),
                   "n_steps": len(sel)}
    assert net.score_paths(s["inputs"], paths)["n_steps"] == 59
    after = X.val if isinstance(X, SparseFlows) else X
    assert np.array_equal(before.view(np.uint8), np.asarray(after).view(np.uint8))                         # the caller's flows: bitwise


def test_backtracking_short_and_min_prefix_paths(data):
    s = _setup(data, "scone")
    p0 = s["paths"][0]
    a, b = p0[0], p0[1]
    paths = s["paths"][:3] + [[a, b, a, b] + p0[2:], [], [a], [a, b], [a, b, a]]
    sc = _check(s, paths)
    assert np.diff(sc.ptr)[3:].tolist() == [len(p0), 0, 0, 0, 1]
    sc1 = _check(s, paths, min_prefix=1)                                                                   # the zero-flow items
    assert np.diff(sc1.ptr)[3:].tolist() == [len(p0) + 1, 0, 0, 1, 2]
    sc3 = _check(s, paths, min_prefix=3)
    assert np.diff(sc3.ptr)[3:].tolist() == [len(p0) - 1, 0, 0, 0, 0]
    ll, n = s["net"].path_log_likelihood(s["inputs"], paths, min_prefix=3)
    assert ll[4:].tolist() == [0.0] * 4 and n[4:].tolist() == [0] * 4


def test_a_non_edge_raises_key_error_before_any_forward(data):
    s = _setup(data, "scone")
    net, nb = s["net"], s["nbrhoods"]
    p0 = s["paths"][0]
    far = next(u for u in range(len(nb)) if u != p0[1] and u not in nb[p0[1]])
    net._multi_hop_trace = trace = []
    try:
        with pytest.raises(KeyError) as exc:
            net.path_step_log_probs(s["inputs"], s["paths"] + [[p0[0], p0[1], far], [p0[0], len(nb) + 5]])
    finally:
        del net._multi_hop_trace
    assert exc.value.args[0] == (p0[1], far) and trace == []
    with pytest.raises(KeyError) as exc:
        net.score_paths(s["inputs"], [[p0[0], len(nb) + 5]])
    assert exc.value.args[0] == (p0[0], len(nb) + 5)


def test_train_model_path_likelihood_switch(tmp_path, monkeypatch):
    from scone_gcn_amd import dataset_io, scone_trajectory_model as stm, trajectory_experiments as te
    monkeypatch.chdir(tmp_path)
    dataset_io.generate_dataset(150, 45, folder="drv", holes=True)
    argv = ["prog", "-epochs", "1", "-batch_size", "12", "-data_folder_suffix", "drv", "-describe", "0", "-path_likelihood", "1"]
    hp = te.hyperparams(argv)
    hp["hidden_layers"] = [(3, 16)] * 3
    stm.reseed(1030)
    net, _ = te.train_model(hp)
    got = net.experiment_results["path_likelihood"]
    inputs_all, _, train_mask, test_mask, _, _, _, _, _, targets_all, prefixes = te.data_setup(hops=(1, 2), folder_suffix="drv", hp=hp)
    paths = [list(p) + [int(t)] for p, t in zip(prefixes, targets_all[0])]
    assert got == {"train": net.score_paths(inputs_all[0], paths, train_mask), "test": net.score_paths(inputs_all[0], paths, test_mask)}
    for r in got.values():
        assert r["n_steps"] > 0 and r["mean_step_logp"] < 0 and r["perplexity"] > 1 and 0.0 <= r["accuracy"] <= 1.0
    stm.reseed(1030)
