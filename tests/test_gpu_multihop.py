"""Multi-hop prediction on the MI355X (STM:110-206, csrc/scn_hops.hip): the probability tree and the greedy rollouts against the
fp64 restatement of tests/test_host_multihop.py on generated data sets, the select kernel through the C-ABI, chunking,
determinism, immutability of the caller's flows, a ~50k-edge complex and the -multi_hop switch of train_model()."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import scone_oracle as so
from scone_gcn_amd.synthetic_data_gen import SparseFlows
from tests.test_host_multihop import oracle_model, ref_binary, ref_target_probs

pytestmark = pytest.mark.gpu

HIDDEN = {"scone": [(3, 16)] * 3, "ebli": [(3, 16)] * 3, "bunch": [(7, 8)] * 3}
N_ROOTS = 12


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from scone_gcn_amd import dataset_io
    d = tmp_path_factory.mktemp("mh")
    cwd = os.getcwd()
    os.chdir(d)
    try:
        dataset_io.generate_dataset(150, 45, folder="mh", holes=True)
    finally:
        os.chdir(cwd)
    return str(d)


def _setup(data, model_type, seed=3):
    from scone_gcn_amd import dataset_io, trajectory_experiments as te
    from scone_gcn_amd.scone_trajectory_model import Scone_GCN
    cwd = os.getcwd()
    os.chdir(data)
    try:
        hp = te.hyperparams(["prog", "-model", model_type])
        out = te.data_setup(hops=(1, 2), folder_suffix="mh", hp=hp)
        _, (B1, B2), *_ = dataset_io.load_dataset("trajectory_data_1hop_mh")
    finally:
        os.chdir(cwd)
    inputs_all, y_all, train_mask, test_mask, shifts, G, E_lookup, nbrhoods, n_nbrs, targets_all, prefixes = out
    net = Scone_GCN(1, 1e-3, 8, 0.0, verbose=False)
    net.setup(te.MODEL_FUNCS[model_type], HIDDEN[model_type], shifts, inputs_all[0], y_all[0], None, train_mask, model_type=model_type)
    rs = np.random.RandomState(seed)
    scale = 0.05 if model_type == "ebli" else 0.4          # choices far from ties; Ebli's L1^2 shift needs smaller weights to keep
    w = [scale * rs.randn(*s) for s in so.weight_shapes(1, HIDDEN[model_type], 1, model_type)]   # log-probabilities above -100
    net._install(w)
    B1, B2 = (np.asarray(sp.csr_matrix(m).toarray(), np.float64) for m in (B1, B2))
    edges = np.array(sorted(E_lookup, key=E_lookup.get))
    fn = oracle_model(model_type, w, B1, B2, edges, B1.shape[0])
    idx = np.arange(N_ROOTS)
    X = inputs_all[0][-1]
    Xs = X.select(idx) if isinstance(X, SparseFlows) else np.asarray(X)[idx]
    dense = Xs.todense() if isinstance(Xs, SparseFlows) else Xs
    sub = [inputs_all[0][0], inputs_all[0][1][idx], Xs]
    return dict(net=net, fn=fn, inputs=sub, flows=np.asarray(dense)[:, :, 0].astype(np.float64), y=y_all[0][idx],
                E_lookup=E_lookup, nbrhoods=nbrhoods, n_nbrs=np.asarray(n_nbrs)[idx], targets=np.asarray(targets_all[1])[idx],
                last=np.asarray(inputs_all[0][1])[idx], masks=[train_mask[idx], test_mask[idx]], full=out)


def _close(got, ref, tol=1e-5):
    """|got - ref| <= tol relative to max(1, |ref|) (fp32 resolves ~1e-7 of a log-probability's magnitude)."""
    return bool(np.all(np.abs(got - ref) <= tol * np.maximum(1.0, np.abs(ref))))


def _argmax_ok(p, choice, tol=2e-5):
    best = p.max(axis=1)
    return bool(np.all(p[np.arange(len(p)), choice] >= best - tol * np.maximum(1.0, np.abs(best))))


def _same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


@pytest.mark.parametrize("model_type", ["scone", "ebli", "bunch"])
@pytest.mark.parametrize("hops", [1, 2, 3])
def test_dist_tree_matches_restatement(data, model_type, hops):
    s = _setup(data, model_type)
    net = s["net"]
    got = net.multi_hop_target_probs(s["inputs"], s["targets"], s["nbrhoods"], s["E_lookup"], s["last"], hops)
    ref = ref_target_probs(s["fn"], s["flows"], s["targets"], s["nbrhoods"], s["E_lookup"], s["last"], hops)
    assert _same_nan(got, ref)
    ok = ~np.isnan(ref)
    assert ok.any() or hops == 1
    assert np.abs(got[ok] - ref[ok]).max(initial=0.0) <= 1e-5
    again = net.multi_hop_target_probs(s["inputs"], s["targets"], s["nbrhoods"], s["E_lookup"], s["last"], hops)
    assert np.array_equal(got.view(np.int64), again.view(np.int64))                      # bitwise, NaN payloads included
    accs = net.multi_hop_accuracy_dist(None, s["inputs"], s["targets"], s["masks"], s["nbrhoods"], s["E_lookup"], s["last"], None, hops)
    want = [np.average(ref[np.asarray(m) == 1]) for m in s["masks"]]
    for a, b in zip(accs, want):
        assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-5
    if hops == 3:
        # the tree holds a backtracking path (v -> a -> v) and a step over an edge the root flow already carries (the last edge of the
        # prefix, set -- not added -- by the step back along it)
        i = 0
        v = int(s["last"][i])
        prev = [u for u in s["nbrhoods"][v] if u >= 0 and s["flows"][i, s["E_lookup"][tuple(sorted((v, int(u))))]] != 0]
        assert prev


@pytest.mark.parametrize("model_type", ["scone", "ebli", "bunch"])
@pytest.mark.parametrize("hops", [1, 2, 3])
def test_binary_and_predict_paths_follow_the_oracle(data, model_type, hops):
    s = _setup(data, model_type)
    net, fn, nb = s["net"], s["fn"], np.asarray(s["nbrhoods"])
    net._multi_hop_trace = trace = []
    acc = net.multi_hop_accuracy_binary(None, s["inputs"], s["y"], np.ones(N_ROOTS), s["nbrhoods"], s["E_lookup"], s["last"],
                                        s["n_nbrs"], hops)
    assert len(trace) == hops
    for flows, last, logp, choice in trace:
        assert np.array_equal(last, s["last"])                                            # the readout's node never advances
        ref = fn(last, flows)
        assert _close(logp, ref)
        p = ref.copy()
        for i in range(N_ROOTS):
            p[i, s["n_nbrs"][i]:] = -100
        assert _argmax_ok(p, choice)
    rtrace = []
    assert acc == ref_binary(fn, s["flows"], s["last"], s["y"], np.ones(N_ROOTS), s["nbrhoods"], s["E_lookup"], s["last"],
                             s["n_nbrs"], hops, rtrace)
    for (gf, _, _, gc), (rf, rc) in zip(trace, rtrace):
        assert np.array_equal(gc, rc) and np.abs(gf - rf).max() == 0.0
    trace.clear()
    paths = net.predict_paths(s["inputs"], hops)
    del net._multi_hop_trace
    assert paths.shape == (N_ROOTS, hops) and paths.dtype == np.int64
    prev = s["last"]
    for h in range(hops):
        flows, last, logp, choice = trace[h]
        assert np.array_equal(last, prev)                                                 # the readout's node advances
        ref = fn(last, flows)
        assert _close(logp, ref)
        p = ref.copy()
        deg = (nb[last] >= 0).sum(1)
        for i in range(N_ROOTS):
            p[i, deg[i]:] = -100
        assert _argmax_ok(p, choice)
        assert np.array_equal(paths[:, h], nb[last, choice])
        for i in range(N_ROOTS):
            assert paths[i, h] in nb[prev[i]]                                            # consecutive nodes are adjacent
        prev = paths[:, h]


def test_hop_select_through_the_c_abi():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from scone_gcn_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device("cuda")
    nan = float("nan")
    logp = torch.tensor([[-1.0, -0.5, -0.5, -3.0],          # tie: first maximum -> 1
                         [-2.0, nan, -1.0, nan],            # NaN wins, first NaN -> 1
                         [-200.0, -300.0, -250.0, -400.0],  # all below -100: the first masked slot (2) wins
                         [-1.0, -2.0, -0.1, -0.2],          # limit 2 hides slot 2 -> 0
                         [-5.0, -4.0, -3.0, -2.0],          # choice 3 has no edge: error word = 4, nothing written
                         [-0.1, -9.0, -9.0, -9.0]], device=dev)
    lim = torch.tensor([4, 4, 2, 2, 4, 1], device=dev, dtype=torch.int32)
    node = torch.tensor([[1, 2, 3, 4], [0, 2, 3, 4], [0, 1, 3, 4], [0, 1, 2, 4], [0, 1, 2, -1]], device=dev, dtype=torch.int32)
    edge = torch.tensor([[0, 1, 2, 3], [0, 4, 5, 6], [1, 4, 7, 8], [2, 5, 7, 9], [3, 6, 8, -1]], device=dev, dtype=torch.int32)
    sign = torch.where(edge >= 0, 1.0, 0.0).to(torch.float32) * torch.tensor([1.0, -1.0, 1.0, -1.0], device=dev)
    deg = torch.tensor([4, 4, 4, 4, 3], device=dev, dtype=torch.int32)
    cur = torch.tensor([0, 1, 2, 3, 4, 2], device=dev, dtype=torch.int32)
    last = cur.clone()
    x = torch.zeros((2, 10, 4, 1), device=dev)
    choice = torch.full((6,), -7, device=dev, dtype=torch.int32)
    nxt = torch.full((6,), -7, device=dev, dtype=torch.int32)
    err = torch.full((1,), ops.INT32_MAX, device=dev, dtype=torch.int32)
    p = lambda t, dt=torch.float32: ops._dev(t, dt)
    assert lib.scn_hop_select(6, 4, p(logp), p(lim, torch.int32), -100.0, p(deg, torch.int32), p(cur, torch.int32), p(last, torch.int32), 5,
                              p(node, torch.int32), p(edge, torch.int32), p(sign), 10, 4, p(x), 1, p(choice, torch.int32),
                              p(nxt, torch.int32), p(err, torch.int32), ops._stream()) == 0
    torch.cuda.synchronize()
    assert choice.tolist() == [1, 1, 2, 0, 3, 0]
    assert int(err.item()) == 4
    assert nxt.tolist() == [2, 2, 3, 0, -7, 0]
    assert cur.tolist() == [2, 2, 3, 0, 4, 0] and last.tolist() == cur.tolist()
    want = torch.zeros((8, 10), device=dev)
    want[0, 1], want[1, 4], want[2, 7], want[3, 2], want[5, 1] = -1.0, -1.0, 1.0, 1.0, 1.0
    assert torch.equal(x.permute(0, 2, 1, 3).reshape(8, 10), want)                      # trajectory i = slab i // 4, lane i % 4
    # no x, no lookup: the final hop of the accuracy writes only the choices
    choice.fill_(-7)
    assert lib.scn_hop_select(6, 4, p(logp), p(lim, torch.int32), -100.0, p(deg, torch.int32), p(cur, torch.int32), None, 5, None, None, None,
                              10, 4, None, 0, p(choice, torch.int32), None, None, ops._stream()) == 0
    torch.cuda.synchronize()
    assert choice.tolist() == [1, 1, 2, 0, 3, 0]
    # a negative count is refused before anything is launched
    assert lib.scn_hop_select(-1, 4, None, None, -100.0, None, None, None, 5, None, None, None, 10, 4, None, 0, None, None, None, None) != 0


def test_missing_pair_raises_key_error_and_flows_stay(data):
    s = _setup(data, "scone")
    net, X = s["net"], s["inputs"][-1]
    before = X.copy()
    acc0 = net.accuracy(None, s["full"][0][0], s["full"][1][0], s["full"][2], s["full"][8])
    with pytest.raises(KeyError):
        net.multi_hop_accuracy_binary(None, s["inputs"], s["y"], np.ones(N_ROOTS), s["nbrhoods"], {}, s["last"], s["n_nbrs"], 2)
    with pytest.raises(KeyError):
        net.multi_hop_accuracy_dist(None, s["inputs"], s["targets"], s["masks"], s["nbrhoods"], {}, s["last"], None, 2)
    net.multi_hop_accuracy_binary(None, s["inputs"], s["y"], np.ones(N_ROOTS), s["nbrhoods"], s["E_lookup"], s["last"], s["n_nbrs"], 3)
    net.multi_hop_accuracy_dist(None, s["inputs"], s["targets"], s["masks"], s["nbrhoods"], s["E_lookup"], s["last"], None, 3)
    net.predict_paths(s["inputs"], 3)
    assert np.array_equal(before.view(np.uint8), X.view(np.uint8))                          # bitwise
    # a dense caller-owned flow tensor stays bitwise as it was too
    dense = torch.as_tensor(s["flows"][:, :, None], dtype=torch.float32, device="cuda")
    snap = dense.clone()
    net.multi_hop_accuracy_binary(None, [s["inputs"][0], s["last"], dense], s["y"], np.ones(N_ROOTS), s["nbrhoods"], s["E_lookup"],
                                  s["last"], s["n_nbrs"], 3)
    assert torch.equal(dense, snap)
    assert net.accuracy(None, s["full"][0][0], s["full"][1][0], s["full"][2], s["full"][8]) == acc0


def _without(E_lookup, *pairs):
    """A copy of E_lookup without the key of every (a, b) of pairs, whichever way round it is stored."""
    lookup = dict(E_lookup)
    for a, b in pairs:
        del lookup[(a, b) if (a, b) in lookup else (b, a)]
    return lookup


def test_rollout_key_error_names_the_lowest_trajectorys_unsorted_pair(data):
    s = _setup(data, "scone")
    net, nbrhoods = s["net"], s["inputs"][0].nbrhoods
    first = net.predict_paths(s["inputs"], 1)[:, 0]
    steps = [(int(v), int(u)) for v, u in zip(s["last"], first)]
    v0, u0 = steps[0]
    # trajectory 0's pair and the first other pair a later trajectory steps across: both fail at the first hop, the lowest is named
    other = next(p for p in steps[1:] if set(p) != {v0, u0})
    with pytest.raises(KeyError) as exc:
        net.predict_paths(s["inputs"], 2, nbrhoods, _without(s["E_lookup"], (v0, u0), other))
    assert exc.value.args == ((v0, u0),)                                       # (current node, chosen neighbour), not sorted


def test_tree_key_error_names_the_sorted_pair_and_spares_the_last_level(data):
    s = _setup(data, "scone")
    net = s["net"]
    v0 = int(s["last"][0])
    u0 = int(next(u for u in s["nbrhoods"][v0] if u >= 0))
    lookup = _without(s["E_lookup"], (v0, u0))
    with pytest.raises(KeyError) as exc:
        net.multi_hop_target_probs(s["inputs"], s["targets"], s["nbrhoods"], lookup, s["last"], 2)
    assert exc.value.args == (tuple(sorted((v0, u0))),)
    # the last level is never expanded: one hop looks no edge up
    got = net.multi_hop_target_probs(s["inputs"], s["targets"], s["nbrhoods"], lookup, s["last"], 1)
    want = net.multi_hop_target_probs(s["inputs"], s["targets"], s["nbrhoods"], s["E_lookup"], s["last"], 1)
    assert np.array_equal(got.view(np.int64), want.view(np.int64))


def test_level_split_over_chunks_gives_the_same_result(data):
    s = _setup(data, "scone")
    net = s["net"]
    one = net.multi_hop_target_probs(s["inputs"], s["targets"], s["nbrhoods"], s["E_lookup"], s["last"], 3)
    net.multi_hop_micro_batch = 8
    many = net.multi_hop_target_probs(s["inputs"], s["targets"], s["nbrhoods"], s["E_lookup"], s["last"], 3)
    paths_many = net.predict_paths(s["inputs"], 3)
    net.multi_hop_micro_batch = None
    assert _same_nan(one, many)
    ok = ~np.isnan(one)
    assert np.abs(one[ok] - many[ok]).max() <= 1e-6
    assert np.array_equal(paths_many, net.predict_paths(s["inputs"], 3))


def test_tree_at_50k_edges():
    """configs[1] size (|E| ~ 50k), 512 roots, dist with 2 hops; 32 roots against the restatement (sparse fp64 forwards)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from scone_gcn_amd import synthetic_data_gen as g, trajectory_experiments as te
    from scone_gcn_amd.complex import SimplicialComplex
    from scone_gcn_amd.scone_trajectory_model import Scone_GCN
    cx = g.random_SC_graph(g.calibrate_n_points(50_000))
    sc = SimplicialComplex(cx)
    paths = g.generate_random_walks(cx, m=512, seed=5)
    flows, choice, last, _, _ = g.path_dataset(cx, paths, seed=6)
    shifts, readout, _ = te.setup_from_complex(sc, "scone")
    E_lookup = {(int(a), int(b)): k for k, (a, b) in enumerate(cx.edges.tolist())}
    rs = np.random.RandomState(11)
    targets = np.array([rs.choice([u for u in sc.nbrhoods[b] if u >= 0]) for b in
                        (rs.choice([u for u in sc.nbrhoods[v] if u >= 0]) for v in last)])
    net = Scone_GCN(1, 1e-3, 8, 0.0, verbose=False)
    y = np.zeros((len(last), sc.max_degree, 1))
    net.setup(te.scone_func, HIDDEN["scone"], shifts, [readout, last, flows], y, None, np.ones(len(last)))
    w = [0.4 * rs.randn(*s) for s in so.weight_shapes(1, HIDDEN["scone"], 1)]
    net._install(w)
    got = net.multi_hop_target_probs([readout, last, flows], targets, sc.nbrhoods, E_lookup, last, 2)
    assert got.shape == (len(last),) and not np.isnan(got).any()
    B1 = sp.csr_matrix(sc.B1, dtype=np.float64)
    L_lo, L_up = (B1.T @ B1).tocsr(), (sp.csr_matrix(sc.B2) @ sp.csr_matrix(sc.B2).T).tocsr()
    B1z = sp.vstack([B1, sp.csr_matrix((1, B1.shape[1]))]).tocsr()
    nb = np.asarray(sc.nbrhoods)

    def fn(lastn, X):
        H = so.conv_forward(w, L_lo, L_up, X[:, :, None])
        lg = np.stack([(B1z[nb[v]] @ H[n]) @ w[-1] for n, v in enumerate(lastn)])[:, :, 0]
        return lg - so.logsumexp(lg, axis=1)
    k = 32
    ref = ref_target_probs(fn, flows.select(np.arange(k)).todense()[:, :, 0].astype(np.float64), targets[:k], nb, E_lookup, last[:k], 2)
    assert np.abs(got[:k] - ref).max() <= 1e-5


def test_train_model_multi_hop_switch(tmp_path, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from scone_gcn_amd import dataset_io, scone_trajectory_model as stm, trajectory_experiments as te
    monkeypatch.chdir(tmp_path)
    dataset_io.generate_dataset(150, 45, folder="drv", holes=True)
    hp = te.hyperparams(["prog", "-epochs", "1", "-batch_size", "12", "-data_folder_suffix", "drv", "-describe", "0",
                         "-multi_hop", "1"])
    hp["hidden_layers"] = [(3, 16)] * 3
    stm.reseed(1030)
    net, _ = te.train_model(hp)
    got = net.experiment_results["multi_hop"]
    inputs_all, y_all, train_mask, test_mask, shifts, G, E_lookup, nbrhoods, n_nbrs, targets_all, prefixes = \
        te.data_setup(hops=(1, 2), folder_suffix="drv", hp=hp)
    # (same weights, same data; the readout / shift objects are fresh ones of the same complex)
    want = net.multi_hop_accuracy_dist(shifts, inputs_all[0], targets_all[1], [train_mask, test_mask], nbrhoods, E_lookup,
                                       inputs_all[0][1], prefixes, 2)
    assert len(got) == 2
    for a, b in zip(got, want):
        assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-6
    stm.reseed(1030)
