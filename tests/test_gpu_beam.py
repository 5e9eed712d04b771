"""Beam-search multi-hop prediction on the MI355X (csrc/scn_hops.hip: scn_beam_step; Scone_GCN.predict_paths_beam): the pruning
kernel through the C-ABI against a numpy restatement (a float32 add and a stable sort on the order key), bitwise; then end to end on
a generated data set against the fp64 oracle, with the two limits as the check: beam = 1 is predict_paths, a beam as wide as the
tree is multi_hop_target_probs."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import scone_oracle as so
from scone_gcn_amd.synthetic_data_gen import SparseFlows
from tests.test_host_beam import order_key, step_flow
from tests.test_host_multihop import oracle_model

pytestmark = pytest.mark.gpu

HIDDEN = {"scone": [(3, 16)] * 3, "ebli": [(3, 16)] * 3, "bunch": [(7, 8)] * 3}
N_ROOTS = 11                                             # the last slab of four trajectories is partial
INT32_MAX = (1 << 31) - 1


# ------------------------------------------------------------------------------------------------------------------
# the kernel through the C-ABI
# ------------------------------------------------------------------------------------------------------------------

def np_beam_step(n_roots, w_in, w_out, h, d, node, score, path_row, path_sign, logp, deg, step_node, step_edge, step_sign, n_rows):
    """scn_beam_step (include/scone_hip.h) in numpy: per root every (k, j) of a live entry, its score one float32 add, a stable sort
    on (NaN first, higher score) over the candidates in (k, j) order."""
    n = n_roots * w_out
    out = dict(root=np.full(n, -1, np.int32), node=np.full(n, -1, np.int32), score=np.full(n, -np.inf, np.float32),
               parent=np.full(n, -1, np.int32), slot=np.full(n, -1, np.int32), path_row=np.full((n, h + 1), -1, np.int32),
               path_sign=np.zeros((n, h + 1), np.float32), err=INT32_MAX)
    for r in range(n_roots):
        cands = []
        for k in range(w_in):
            e = r * w_in + k
            v = int(node[e])
            if v < 0:
                continue
            for j in range(int(deg[v])):
                cands.append((np.float32(score[e]) + np.float32(logp[e, j]), k, j))
                if step_edge[v, j] < 0 or step_edge[v, j] >= n_rows or step_node[v, j] < 0:
                    out["err"] = min(out["err"], e * d + j)
        cands.sort(key=lambda c: order_key(c[0], 0, 0))                       # stable: equal scores stay in (k, j) order
        for o, (s, k, j) in enumerate(cands[:w_out]):
            c, e = r * w_out + o, r * w_in + k
            v = int(node[e])
            out["root"][c], out["node"][c], out["score"][c], out["parent"][c], out["slot"][c] = r, step_node[v, j], s, k, j
            out["path_row"][c, :h], out["path_row"][c, h] = path_row[e], step_edge[v, j]
            out["path_sign"][c, :h], out["path_sign"][c, h] = path_sign[e], step_sign[v, j]
    return out


def run_beam_step(n_roots, w_in, w_out, h, d, node, score, path_row, path_sign, logp, deg, step_node, step_edge, step_sign, n_rows,
                  with_paths=True):
    """One call with every output buffer pre-filled with junk: whatever comes back was written by the library."""
    from scone_gcn_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device("cuda")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    p = lambda x: None if x is None else ops._dev(x, x.dtype)
    n = n_roots * w_out
    ins = [t(node, np.int32), t(score, np.float32), t(path_row, np.int32) if h else None, t(path_sign, np.float32) if h else None,
           t(logp, np.float32), t(deg, np.int32)]
    tabs = [t(step_node, np.int32), t(step_edge, np.int32), t(step_sign, np.float32)]
    outs = [torch.full((n,), -7, device=dev, dtype=torch.int32), torch.full((n,), -7, device=dev, dtype=torch.int32),
            torch.full((n,), 7.0, device=dev), torch.full((n,), -7, device=dev, dtype=torch.int32),
            torch.full((n,), -7, device=dev, dtype=torch.int32)]
    paths = [torch.full((n, h + 1), -7, device=dev, dtype=torch.int32), torch.full((n, h + 1), 7.0, device=dev)] if with_paths \
        else [None, None]
    err = torch.full((1,), INT32_MAX, device=dev, dtype=torch.int32)
    status = lib.scn_beam_step(n_roots, w_in, w_out, h, d, *[p(x) for x in ins[:5]], p(ins[5]), len(deg), *[p(x) for x in tabs], n_rows,
                               *[p(x) for x in outs], *[p(x) for x in paths], p(err), ops._stream())
    assert status == 0
    torch.cuda.synchronize()
    got = dict(zip(("root", "node", "score", "parent", "slot"), (x.cpu().numpy() for x in outs)))
    if with_paths:
        got["path_row"], got["path_sign"] = paths[0].cpu().numpy(), paths[1].cpu().numpy()
    got["err"] = int(err.item())
    return got


def same(got, want):
    for key, g in got.items():
        w = want[key]
        if key == "err":
            assert g == w, (key, g, w)
        else:
            assert g.dtype == w.dtype and np.array_equal(g.view(np.int32), w.view(np.int32)), key       # scores bitwise


def tables(rs, n_nodes, d, n_rows, deg=None):
    deg = rs.randint(1, d + 1, size=n_nodes) if deg is None else np.asarray(deg)
    live = np.arange(d)[None, :] < deg[:, None]
    step_node = np.where(live, rs.randint(0, n_nodes, size=(n_nodes, d)), -1)
    step_edge = np.where(live, rs.randint(0, n_rows, size=(n_nodes, d)), -1)
    step_sign = np.where(live, rs.choice([-1.0, 1.0], size=(n_nodes, d)), 0.0)
    return deg, step_node, step_edge, step_sign


def level(rs, n_roots, w_in, h, d, n_nodes, n_rows, quantum):
    """A random input level; scores and log-probabilities on a grid of `quantum`, so that sums tie exactly."""
    node = rs.randint(0, n_nodes, size=n_roots * w_in)
    score = -quantum * rs.randint(0, 12, size=n_roots * w_in)
    logp = -quantum * rs.randint(1, 12, size=(n_roots * w_in, d))
    path_row = rs.randint(0, n_rows, size=(n_roots * w_in, h))
    path_sign = rs.choice([-1.0, 1.0], size=(n_roots * w_in, h))
    return node, score.astype(np.float32), path_row, path_sign, logp.astype(np.float32)


def case_a():
    rs = np.random.RandomState(0)
    deg, sn, se, ss = tables(rs, 4, 3, 9, deg=[3, 2, 3, 1])
    node, score, prow, psign, logp = level(rs, 1, 1, 0, 3, 4, 9, 0.25)
    node[:] = 0
    return (1, 1, 1, 0, 3, node, score, prow, psign, logp, deg, sn, se, ss, 9)


def case_b():
    """Root 0: a single candidate (one live entry on the degree-1 node), so four of five outputs are dead.  Root 1: a dead entry
    after two live ones.  Root 2: equal scores on all three parents and repeated log-probabilities: ties across parents and slots.
    Root 3: a NaN, a +inf and a -inf among the log-probabilities.  Root 4: random."""
    rs = np.random.RandomState(1)
    n_roots, w_in, w_out, h, d, n_nodes, n_rows = 5, 3, 5, 2, 7, 6, 23
    deg, sn, se, ss = tables(rs, n_nodes, d, n_rows, deg=[1, 7, 4, 3, 5, 2])
    node, score, prow, psign, logp = level(rs, n_roots, w_in, h, d, n_nodes, n_rows, 0.25)
    node[0:3] = [0, -1, -1]
    node[3:6] = [2, 4, -1]
    node[6:9] = [3, 3, 1]
    score[6:9] = -1.5
    logp[6:9] = np.float32([-0.5, -1.0, -0.5, -1.0, -0.5, -2.0, -0.5])
    node[9:12] = [1, 4, 2]
    logp[9, 2], logp[10, 1], logp[10, 3], logp[11, 0] = np.nan, np.inf, -np.inf, np.nan
    return (n_roots, w_in, w_out, h, d, node, score, prow, psign, logp, deg, sn, se, ss, n_rows)


def case_c():
    rs = np.random.RandomState(2)
    n_roots, w_in, w_out, h, d, n_nodes, n_rows = 3, 64, 70, 2, 5, 40, 101
    deg, sn, se, ss = tables(rs, n_nodes, d, n_rows)
    node, score, prow, psign, logp = level(rs, n_roots, w_in, h, d, n_nodes, n_rows, 0.125)
    node[2 * w_in + 50:] = -1                                                 # the last root's tail is dead
    return (n_roots, w_in, w_out, h, d, node, score, prow, psign, logp, deg, sn, se, ss, n_rows)


def case_d():
    from scone_gcn_amd._lib import SCN_BEAM_MAX as M
    rs = np.random.RandomState(3)
    n_roots, h, d, n_nodes, n_rows = 2, 1, 20, 300, 1009
    deg, sn, se, ss = tables(rs, n_nodes, d, n_rows)
    node, score, prow, psign, logp = level(rs, n_roots, M, h, d, n_nodes, n_rows, 0.0625)
    logp += rs.randn(*logp.shape).astype(np.float32) * (rs.rand(*logp.shape) < 0.5)      # half on the grid (ties), half off it
    node[M + 12:] = -1                                                       # root 1: 12 live entries, fewer than M candidates
    return (n_roots, M, M, h, d, node, score, prow, psign, logp, deg, sn, se, ss, n_rows)


@pytest.mark.parametrize("case", [case_a, case_b, case_c, case_d], ids=["a", "b", "c", "d"])
def test_beam_step_matches_numpy_bitwise(case):
    args = case()
    want = np_beam_step(*args)
    got = run_beam_step(*args)
    same(got, want)
    n_roots, w_in, w_out = args[:3]
    live = (want["root"] >= 0).reshape(n_roots, w_out)
    assert np.array_equal(live, np.sort(live, axis=1)[:, ::-1])               # dead entries sit after the live ones
    if case is case_b:
        assert live.sum(axis=1).tolist() == [1, 5, 5, 5, 5]
        assert np.isnan(want["score"][15:17]).all() and want["score"][17] == np.inf     # NaN first, then +inf
        tied = want["score"][10:15]
        assert (tied == -2.0).all() and want["parent"][10:15].tolist() == [0, 0, 1, 1, 2] and want["slot"][10:12].tolist() == [0, 2]
    if case is case_c:
        assert live.all()
    if case is case_d:
        assert live[0].all() and 0 < live[1].sum() < w_out
    # without the path outputs (final level) nothing else differs; a second call gives the same bytes
    short = run_beam_step(*args, with_paths=False)
    same(short, {k: v for k, v in want.items() if not k.startswith("path")})
    again = run_beam_step(*args)
    same(again, got)


def test_beam_step_reports_an_unselected_candidate_without_an_edge():
    """The error word does not depend on the scores: each missing pair sits on the worst candidate of its root, far below the two
    that are kept, and the lowest index wins."""
    rs = np.random.RandomState(4)
    n_roots, w_in, w_out, h, d, n_nodes, n_rows = 2, 2, 2, 1, 4, 5, 17
    deg, sn, se, ss = tables(rs, n_nodes, d, n_rows, deg=[4, 4, 3, 4, 2])
    node, score, prow, psign, logp = level(rs, n_roots, w_in, h, d, n_nodes, n_rows, 0.25)
    node[:] = [0, 1, 2, 3]
    logp[3, 2] = -1000.0
    se[3, 2] = -1
    se[1, 3] = n_rows                                                         # a row out of range counts too: entry 1, slot 3
    logp[1, 3] = -900.0
    se[4, 1] = -1                                                             # a node no entry stands on: not a candidate
    args = (n_roots, w_in, w_out, h, d, node, score, prow, psign, logp, deg, sn, se, ss, n_rows)
    want = np_beam_step(*args)
    assert want["err"] == 1 * d + 3
    got = run_beam_step(*args)
    same(got, want)
    assert not ((got["parent"] == 1) & (got["slot"] == 3))[:w_out].any()
    se[1, 3] = 5
    args = (n_roots, w_in, w_out, h, d, node, score, prow, psign, logp, deg, sn, se, ss, n_rows)
    got = run_beam_step(*args)
    assert got["err"] == 3 * d + 2
    same(got, np_beam_step(*args))


def test_beam_step_refuses_bad_arguments():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from scone_gcn_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device("cuda")
    i = torch.zeros((4 * (_lib.SCN_BEAM_MAX + 1),), device=dev, dtype=torch.int32)
    f = torch.zeros((4 * (_lib.SCN_BEAM_MAX + 1),), device=dev)
    pi, pf = ops._dev(i, torch.int32), ops._dev(f)

    def call(w_in=1, w_out=1, logp=pf, n_roots=1):
        return lib.scn_beam_step(n_roots, w_in, w_out, 0, 3, pi, pf, None, None, logp, pi, 1, pi, pi, pf, 8, pi, pi, pf, pi, pi, None,
                                 None, pi, ops._stream())
    assert call(w_out=_lib.SCN_BEAM_MAX + 1) == _lib.SCN_ERR_UNSUPPORTED
    assert call(w_in=_lib.SCN_BEAM_MAX + 1) == _lib.SCN_ERR_UNSUPPORTED
    assert call(logp=None) == _lib.SCN_ERR_BAD_ARG
    assert call(n_roots=-1) not in (0, _lib.SCN_ERR_BAD_ARG, _lib.SCN_ERR_UNSUPPORTED)        # SCN_ERR_BAD_SHAPE
    assert call(w_out=0) == call(n_roots=-1)
    assert call(n_roots=0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------
# end to end (the data set and weights of tests/test_gpu_multihop.py)
# ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def data(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from scone_gcn_amd import dataset_io
    d = tmp_path_factory.mktemp("beam")
    cwd = os.getcwd()
    os.chdir(d)
    try:
        dataset_io.generate_dataset(150, 45, folder="mh", holes=True)
    finally:
        os.chdir(cwd)
    return {"dir": str(d)}


def _setup(data, model_type, seed=3):
    if model_type in data:                                                    # one model and one oracle per type, shared and unchanged
        return data[model_type]
    from scone_gcn_amd import dataset_io, trajectory_experiments as te
    from scone_gcn_amd.scone_trajectory_model import Scone_GCN
    cwd = os.getcwd()
    os.chdir(data["dir"])
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
    data[model_type] = dict(net=net, fn=fn, inputs=sub, flows=np.asarray(dense)[:, :, 0].astype(np.float64),
                            E_lookup=E_lookup, nbrhoods=np.asarray(nbrhoods), targets=np.asarray(targets_all[1])[idx],
                            last=np.asarray(inputs_all[0][1])[idx])
    return data[model_type]


def _close(got, ref, tol=1e-5):
    """|got - ref| <= tol relative to max(1, |ref|) (fp32 resolves ~1e-7 of a log-probability's magnitude)."""
    return bool(np.all(np.abs(got - ref) <= tol * np.maximum(1.0, np.abs(ref))))


def _traced(net, *args):
    net._multi_hop_trace = trace = []
    try:
        out = net.predict_paths_beam(*args)
    finally:
        del net._multi_hop_trace
    return out, trace


def _check_against_oracle(s, inputs, last, hops, beam):
    """Replays every entry of every level on the fp64 oracle and checks what the issue lists; returns (paths, logp, trace)."""
    net, fn, nb, E_lookup = s["net"], s["fn"], s["nbrhoods"], s["E_lookup"]
    N, D = len(last), nb.shape[1]
    deg = (nb >= 0).sum(axis=1)
    (paths, logp), trace = _traced(net, inputs, hops, beam)
    assert paths.shape == (N, beam, hops) and paths.dtype == np.int64 and logp.shape == (N, beam) and logp.dtype == np.float64
    assert len(trace) == hops
    # per trajectory the entries of the current level: (node, flow, oracle score, node path)
    entries = [[(int(last[i]), s["flows"][i].copy(), 0.0, ())] for i in range(N)]
    W = 1
    for h, rec in enumerate(trace):
        W2 = min(beam, W * D)
        assert rec["node"].shape == (N, W) and rec["score"].shape == (N, W) and rec["logp"].shape == (N, W, D)
        assert rec["parent"].shape == (N, W2) and rec["slot"].shape == (N, W2)
        flat = [(i, k) for i in range(N) for k in range(len(entries[i]))]
        ref = fn(np.asarray([entries[i][k][0] for i, k in flat]), np.stack([entries[i][k][1] for i, k in flat]))
        new = []
        for i in range(N):
            n_live = len(entries[i])
            assert np.array_equal(rec["node"][i], [e[0] for e in entries[i]] + [-1] * (W - n_live))     # dead after the live ones
            rows = ref[[n for n, (r, _) in enumerate(flat) if r == i]]
            assert _close(rec["logp"][i, :n_live], rows)
            osc = np.array([e[2] for e in entries[i]])
            assert _close(rec["score"][i, :n_live], osc, tol=max(h, 1) * 1e-5)
            cand = sorted((osc[k] + rows[k, j] for k in range(n_live) for j in range(deg[entries[i][k][0]])), reverse=True)
            n_sel = min(W2, len(cand))
            assert np.array_equal(rec["parent"][i] >= 0, np.arange(W2) < n_sel)
            bar = cand[n_sel - 1]                                            # the W-th best oracle candidate
            out = []
            for o in range(n_sel):
                k, j = int(rec["parent"][i, o]), int(rec["slot"][i, o])
                v, f, sc, path = entries[i][k]
                assert j < deg[v]
                assert sc + rows[k, j] >= bar - 2e-5 * max(1.0, abs(bar))
                u = int(nb[v][j])
                out.append((u, step_flow(f, v, u, E_lookup), sc + rows[k, j], path + (u,)))
            assert len(set(e[3] for e in out)) == n_sel                      # pairwise distinct
            new.append(out)
        entries, W = new, W2
    for i in range(N):
        n_live = len(entries[i])
        assert np.array_equal(paths[i, :n_live], np.array([e[3] for e in entries[i]]).reshape(n_live, hops))
        assert (paths[i, n_live:] == -1).all() and (logp[i, n_live:] == -np.inf).all()
        ref_lp = np.array([e[2] for e in entries[i]])
        assert _close(logp[i, :n_live], ref_lp, tol=hops * 1e-5)
        assert np.all(np.diff(logp[i, :n_live]) <= 0)                        # best first
        for path in paths[i, :n_live]:
            prev = int(last[i])
            for u in path:
                assert u in nb[prev][:deg[prev]]                             # consecutive nodes are adjacent
                prev = int(u)
    for h in range(1, hops):                                                 # ... and sorted at every level on the way
        with np.errstate(invalid="ignore"):                                  # (-inf) - (-inf) between two dead entries
            assert np.all((np.diff(trace[h]["score"], axis=1) <= 0) | (trace[h]["node"][:, 1:] < 0))
    return paths, logp, trace


@pytest.mark.parametrize("model_type", ["scone", "ebli", "bunch"])
def test_beam_of_one_is_predict_paths(data, model_type):
    s = _setup(data, model_type)
    for hops in (1, 2, 3):
        paths, logp = s["net"].predict_paths_beam(s["inputs"], hops, 1)
        assert paths.shape == (N_ROOTS, 1, hops) and np.array_equal(paths[:, 0, :], s["net"].predict_paths(s["inputs"], hops))
        assert np.isfinite(logp).all()


@pytest.mark.parametrize("model_type", ["scone", "ebli", "bunch"])
@pytest.mark.parametrize("hops", [2, 4])
@pytest.mark.parametrize("beam", [2, 5])
def test_beam_follows_the_oracle(data, model_type, hops, beam):
    s = _setup(data, model_type)
    _check_against_oracle(s, s["inputs"], s["last"], hops, beam)


@pytest.mark.parametrize("model_type", ["scone", "ebli", "bunch"])
def test_full_width_beam_is_the_probability_tree(data, model_type):
    s = _setup(data, model_type)
    net, nb, last = s["net"], s["nbrhoods"], s["last"]
    deg = (nb >= 0).sum(axis=1)
    beam = 256
    count = np.array([sum(deg[u] for u in nb[v][:deg[v]]) for v in last])
    assert count.max() < beam                                                # the beam holds every two-step path
    paths, logp = net.predict_paths_beam(s["inputs"], 2, beam)
    assert np.array_equal((paths[:, :, -1] >= 0).sum(axis=1), count)
    assert np.array_equal(np.isfinite(logp), paths[:, :, -1] >= 0)
    tree = net.multi_hop_target_probs(s["inputs"], s["targets"], s["nbrhoods"], s["E_lookup"], last, 2)
    with np.errstate(invalid="ignore"):
        got = np.array([np.float64(np.exp(logp[i][paths[i, :, -1] == s["targets"][i]]).sum()) /
                        np.float64((paths[i, :, -1] == s["targets"][i]).sum()) for i in range(N_ROOTS)])
    assert np.array_equal(np.isnan(got), np.isnan(tree))
    ok = ~np.isnan(tree)
    assert ok.any() and np.abs(got[ok] - tree[ok]).max() <= 1e-5


def test_a_root_of_low_degree_leaves_a_dead_tail(data):
    s = _setup(data, "scone")
    nb = s["nbrhoods"]
    deg = (nb >= 0).sum(axis=1)
    v = int(np.argmin(np.where(deg > 0, deg, nb.shape[1] + 1)))              # a node of degree 1 if the complex has one
    beam = int(deg[v]) + 2
    last = s["last"].copy()
    last[0] = v
    inputs = [s["inputs"][0], last, s["inputs"][2]]
    paths, logp, trace = _check_against_oracle(s, inputs, last, 3, beam)
    assert (trace[1]["node"][0, deg[v]:] == -1).all() and (trace[1]["node"][0, :deg[v]] >= 0).all()
    assert np.isneginf(trace[1]["score"][0, deg[v]:]).all()
    assert (paths[0, 0] >= 0).all() and np.isfinite(logp[0, 0])


def test_level_split_over_chunks_gives_the_same_result(data):
    s = _setup(data, "scone")
    net = s["net"]
    one = net.predict_paths_beam(s["inputs"], 3, 5)
    net.multi_hop_micro_batch = 8
    try:
        many = net.predict_paths_beam(s["inputs"], 3, 5)
    finally:
        net.multi_hop_micro_batch = None
    assert np.array_equal(one[0], many[0])
    assert np.abs(one[1] - many[1]).max() <= 1e-5
    again = net.predict_paths_beam(s["inputs"], 3, 5)
    assert np.array_equal(one[0], again[0]) and np.array_equal(one[1], again[1])


def test_missing_pair_raises_key_error_and_flows_stay(data):
    s = _setup(data, "scone")
    net, X = s["net"], s["inputs"][-1]
    before = X.copy()
    with pytest.raises(KeyError):
        net.predict_paths_beam(s["inputs"], 2, 3, s["nbrhoods"], {})
    v = int(s["last"][0])
    u = int(s["nbrhoods"][v][0])
    lookup = dict(s["E_lookup"])
    del lookup[(min(v, u), max(v, u))]
    with pytest.raises(KeyError) as exc:
        net.predict_paths_beam(s["inputs"], 2, 3, s["nbrhoods"], lookup)
    assert exc.value.args[0] == (v, u)                                        # the lowest (entry, slot) without an edge
    net.predict_paths_beam(s["inputs"], 2, 3)
    assert np.array_equal(np.asarray(before.view(np.uint8)), np.asarray(X.view(np.uint8)))     # bitwise


def test_top_k_accuracy(data):
    s = _setup(data, "scone")
    net = s["net"]
    mask = (np.arange(N_ROOTS) % 3 != 0).astype(int)
    for beam in (1, 4):
        paths, _ = net.predict_paths_beam(s["inputs"], 2, beam)
        want = float(np.mean([s["targets"][i] in paths[i, :, -1] for i in range(N_ROOTS) if mask[i]]))
        assert net.multi_hop_accuracy_topk(s["inputs"], s["targets"], mask, 2, beam) == want
    greedy = net.predict_paths(s["inputs"], 2)
    assert net.multi_hop_accuracy_topk(s["inputs"], s["targets"], mask, 2, 1) == float(np.mean((greedy[:, -1] == s["targets"])[mask == 1]))


def test_train_model_beam_switch(tmp_path, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from scone_gcn_amd import dataset_io, scone_trajectory_model as stm, trajectory_experiments as te
    monkeypatch.chdir(tmp_path)
    dataset_io.generate_dataset(150, 45, folder="drv", holes=True)
    argv = ["prog", "-epochs", "1", "-batch_size", "12", "-data_folder_suffix", "drv", "-describe", "0", "-multi_hop", "1", "-beam", "3"]
    hp = te.hyperparams(argv)
    hp["hidden_layers"] = [(3, 16)] * 3
    stm.reseed(1030)
    net, _ = te.train_model(hp)
    got = net.experiment_results["multi_hop_topk"]
    inputs_all, y_all, train_mask, test_mask, shifts, G, E_lookup, nbrhoods, n_nbrs, targets_all, prefixes = \
        te.data_setup(hops=(1, 2), folder_suffix="drv", hp=hp)
    want = [net.multi_hop_accuracy_topk(inputs_all[0], targets_all[1], m, 2, 3) for m in (train_mask, test_mask)]
    assert got == want and all(0.0 <= a <= 1.0 for a in got)
    assert len(net.experiment_results["multi_hop"]) == 2
    stm.reseed(1030)
