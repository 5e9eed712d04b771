"""Multi-hop prediction (STM:110-206) without a GPU: the step tables the device kernels read, the -multi_hop switch, and this
file's fp64 restatement of the reference's two multi-hop metrics (used by tests/test_gpu_multihop.py as the reference) checked
against brute-force enumeration of every 2-step path with per-sample oracle forwards on the 4-node graph."""
import os

import numpy as np
import pytest
import torch

from oracle import scone_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ------------------------------------------------------------------------------------------------------------------
# fp64 restatement of STM:110-206 (treelib replaced by plain lists; every path its own leaf)
# model_fn(last_nodes (n,), flows (n, E)) -> log-probabilities (n, D)
# ------------------------------------------------------------------------------------------------------------------

def masked_argmax(preds, limit):
    p = np.array(preds, np.float64)
    for i in range(len(p)):
        p[i, int(limit[i]):] = -100                                          # STM:116-117
    return np.argmax(p, axis=1)


def ref_binary(model_fn, flows, readout_last, y, mask, nbrhoods, E_lookup, last_nodes, n_nbrs, hops, trace=None):
    """multi_hop_accuracy_binary (STM:110-152) on a COPY of the flows; trace gets (flows, choice) per hop."""
    X = np.array(flows, np.float64)
    cur = np.asarray(last_nodes)
    for h in range(hops):
        preds = model_fn(np.asarray(readout_last), X)
        choice = masked_argmax(preds, n_nbrs)
        if trace is not None:
            trace.append((X.copy(), choice))
        if h == hops - 1:
            m = np.asarray(mask) == 1
            return float(np.average(choice[m] == np.argmax(np.asarray(y)[m], axis=1).reshape(-1)))
        for i in range(len(X)):
            v = int(cur[i])
            j = int(np.asarray(nbrhoods)[v][choice[i]])
            if (v, j) in E_lookup:
                X[i, E_lookup[(v, j)]] = 1
            else:
                X[i, E_lookup[(j, v)]] = -1                                  # KeyError when neither key exists


def ref_target_probs(model_fn, flows, target_nodes, nbrhoods, E_lookup, last_nodes, hops):
    """Per-root target probability of multi_hop_accuracy_dist (STM:154-204); NaN for 0 / 0."""
    nb = [np.asarray(n)[np.asarray(n) != -1] for n in nbrhoods]
    leaves = [[(int(last_nodes[i]), np.array(flows[i], np.float64), 1.0)] for i in range(len(flows))]
    for h in range(hops):
        flat = [(i, leaf) for i in range(len(leaves)) for leaf in leaves[i]]
        probs = np.exp(model_fn(np.asarray([l[0] for _, l in flat]), np.stack([l[1] for _, l in flat])))
        new = [[] for _ in leaves]
        for k, (i, (v, f, p)) in enumerate(flat):
            for j, u in enumerate(nb[v]):
                f2 = f.copy()
                f2[E_lookup[tuple(sorted((v, int(u))))]] = 1 if v < u else -1
                new[i].append((int(u), f2, p * probs[k, j]))
        leaves = new
    out = np.zeros(len(leaves))
    with np.errstate(invalid="ignore"):
        for i, ls in enumerate(leaves):
            hit = [p for v, _, p in ls if v == int(target_nodes[i])]
            out[i] = np.float64(sum(hit)) / np.float64(len(hit))
    return out


def oracle_model(model_type, weights, B1, B2, edges, n_nodes, flips=None):
    """model_fn of the fp64 oracle for scone / ebli / bunch on a dense complex."""
    nb, D = so.neighborhoods(edges, n_nodes)
    if model_type == "bunch":
        shifts = so.bunch_shifts(B1, B2)
        return lambda last, X: so.bunch_forward(weights, shifts, nb, last, X[:, :, None])[:, :, 0]
    F = None if flips is None else np.diag(flips)
    S = so.ebli_shifts(B1, B2, F) if model_type == "ebli" else so.scone_shifts(B1, B2, F)
    Bc = so.make_Bconds(B1, nb, F)
    fwd = so.ebli_forward if model_type == "ebli" else so.scone_forward
    return lambda last, X: fwd(weights, S[0], S[1], Bc, last, X[:, :, None])[:, :, 0]


# ------------------------------------------------------------------------------------------------------------------
# the 4-node graph (PM:128-151)
# ------------------------------------------------------------------------------------------------------------------

def _tiny4():
    t = np.load(os.path.join(GOLDEN, "tiny4_complex.npz"))
    edges = np.asarray(t["edges"])
    return t["B1"].astype(np.float64), t["B2"].astype(np.float64), edges, {(int(a), int(b)): k for k, (a, b) in enumerate(edges)}


@pytest.mark.parametrize("model_type", ["scone", "ebli", "bunch"])
def test_restatement_matches_brute_force_two_step_paths(model_type):
    B1, B2, edges, E_lookup = _tiny4()
    nb, D = so.neighborhoods(edges, 4)
    rs = np.random.RandomState(7)
    hidden = [(7, 8)] * 2 if model_type == "bunch" else [(3, 8)] * 2
    weights = [0.5 * rs.randn(*s) for s in so.weight_shapes(1, hidden, 1, model_type)]
    fn = oracle_model(model_type, weights, B1, B2, edges, 4)
    flows = np.zeros((4, 5))
    flows[0, E_lookup[(0, 1)]] = 1                      # 0 -> 1, last node 1
    flows[1, E_lookup[(1, 2)]] = -1                     # 2 -> 1, last node 1
    flows[2, E_lookup[(0, 3)]] = -1                     # 3 -> 0, last node 0
    flows[3, E_lookup[(2, 3)]] = 1                      # 2 -> 3, last node 3
    last = np.array([1, 1, 0, 3])
    targets = np.array([3, 0, 1, 1])
    got = ref_target_probs(fn, flows, targets, nb, E_lookup, last, 2)
    for i in range(4):
        num, cnt = 0.0, 0
        p0 = np.exp(fn(last[i:i + 1], flows[i:i + 1])[0])
        nbr0 = [u for u in nb[last[i]] if u >= 0]
        for a_slot, a in enumerate(nbr0):
            f1 = flows[i].copy()
            v = int(last[i])
            f1[E_lookup[(min(v, a), max(v, a))]] = 1.0 if v < a else -1.0
            p1 = np.exp(fn(np.array([a]), f1[None])[0])
            for b_slot, b in enumerate(u for u in nb[a] if u >= 0):
                if b == targets[i]:
                    num += p0[a_slot] * p1[b_slot]
                    cnt += 1
        want = num / cnt if cnt else np.nan
        assert (np.isnan(want) and np.isnan(got[i])) or abs(got[i] - want) <= 1e-12
    # greedy rollout, 2 hops: the second choice is made on the flow with the first step SET, current / readout node unchanged
    n_nbrs = (nb[last] >= 0).sum(1)
    y = np.zeros((4, D, 1))
    trace = []
    acc = ref_binary(fn, flows, last, y, np.ones(4), nb, E_lookup, last, n_nbrs, 2, trace)
    c0 = masked_argmax(fn(last, flows), n_nbrs)
    X = flows.copy()
    for i in range(4):
        j = nb[last[i]][c0[i]]
        k = E_lookup.get((last[i], j))
        if k is not None:
            X[i, k] = 1
        else:
            X[i, E_lookup[(j, last[i])]] = -1
    c1 = masked_argmax(fn(last, X), n_nbrs)
    assert np.array_equal(trace[1][1], c1) and acc == float(np.mean(c1 == 0))


def test_restatement_keeps_nan_for_unreachable_targets():
    B1, B2, edges, E_lookup = _tiny4()
    nb, _ = so.neighborhoods(edges, 4)
    fn = oracle_model("scone", so.generate_weights(1, [(3, 8)] * 2, 1), B1, B2, edges, 4)
    flows = np.zeros((1, 5))
    # one hop from node 1 reaches 0 and 2 only
    assert np.isnan(ref_target_probs(fn, flows, [3], nb, E_lookup, [1], 1)[0])


# ------------------------------------------------------------------------------------------------------------------
# step tables (multihop.StepTables) against a direct walk of the dicts, on a complex with a non-identity edge layout
# ------------------------------------------------------------------------------------------------------------------

def _walk(nbrhoods, E_lookup, perm, rule):
    V, D = nbrhoods.shape
    node = -np.ones((V, D), np.int64)
    edge = -np.ones((V, D), np.int64)
    sign = np.zeros((V, D))
    for v in range(V):
        row = [int(u) for u in nbrhoods[v] if u != -1] if rule == "dist" else [int(u) for u in nbrhoods[v]]
        for j, u in enumerate(row):
            node[v, j] = u
            if u < 0:
                continue
            if rule == "binary":
                if (v, u) in E_lookup:
                    edge[v, j], sign[v, j] = perm[E_lookup[(v, u)]], 1
                elif (u, v) in E_lookup:
                    edge[v, j], sign[v, j] = perm[E_lookup[(u, v)]], -1
            else:
                k = E_lookup.get(tuple(sorted((v, u))))
                if k is not None:
                    edge[v, j], sign[v, j] = perm[k], (1 if v < u else -1)
    return node, edge, sign


@pytest.mark.parametrize("rule", ["binary", "dist"])
def test_step_tables_match_a_dict_walk(rule):
    from scone_gcn_amd import multihop
    from scone_gcn_amd import synthetic_data_gen as g
    from scone_gcn_amd.complex import SimplicialComplex
    cx = g.random_SC_graph(60)
    sc = SimplicialComplex(cx)
    perm = sc.layout.perm[1]
    assert not sc.layout.is_identity(1)
    E_lookup = {(int(a), int(b)): k for k, (a, b) in enumerate(cx.edges.tolist())}
    # a caller's table with a reversed key (binary rule: sign -1 through E_lookup[(u, v)]), a missing pair and padding in the middle
    a, b = (int(x) for x in cx.edges[3])
    E_lookup[(b, a)] = E_lookup.pop((a, b))
    c, d = (int(x) for x in cx.edges[7])
    del E_lookup[(c, d)]
    nb = np.array(sc.nbrhoods)
    v_mid = int(np.argmax((nb >= 0).sum(1)))
    nb[v_mid, 1:] = np.concatenate([[-1], nb[v_mid, 1:-1]])
    tab = multihop.StepTables(nb, E_lookup, perm, rule, torch.device("cpu"))
    node, edge, sign = _walk(nb, E_lookup, perm, rule)
    assert np.array_equal(tab.h_node, node) and np.array_equal(tab.node.numpy(), node)
    assert np.array_equal(tab.edge.numpy(), edge)
    assert np.array_equal(tab.sign.numpy(), sign.astype(np.float32))
    assert np.array_equal(tab.deg.numpy(), (nb >= 0).sum(1))
    # the missing pair is the sentinel on both sides
    jc = list(node[c]).index(d)
    jd = list(node[d]).index(c)
    assert edge[c, jc] == -1 and edge[d, jd] == -1
    # the reversed key: the binary rule finds it from both ends (+1 from b), the dist rule looks up sorted pairs only
    jb, ja = list(node[b]).index(a), list(node[a]).index(b)
    if rule == "binary":
        assert sign[b, jb] == 1 and sign[a, ja] == -1 and edge[b, jb] == edge[a, ja] == perm[E_lookup[(b, a)]]
    else:
        assert edge[b, jb] == edge[a, ja] == -1


def test_multi_hop_switch():
    from scone_gcn_amd import trajectory_experiments as te
    assert te.hyperparams(["prog"])["multi_hop"] == 0
    assert te.hyperparams(["prog", "-multi_hop", "1"])["multi_hop"] == 1


def test_probed_closure_is_refused():
    """A plain Bcond_func closure only knows the last nodes it has been probed at: multi-hop refuses it with a TypeError
    before anything touches a device."""
    from scone_gcn_amd.scone_trajectory_model import Scone_GCN
    net = Scone_GCN(1, 1e-3, 4, 0.0, verbose=False)
    net.model_type = "scone"
    B1, B2, edges, E_lookup = _tiny4()
    nb, _ = so.neighborhoods(edges, 4)
    inputs = [so.make_Bconds(B1, nb), np.array([1]), np.zeros((1, 5, 1))]
    with pytest.raises(TypeError, match="Bconds"):
        net.multi_hop_accuracy_dist(None, inputs, [3], [np.ones(1)], nb, E_lookup, [1], None, 2)
    with pytest.raises(TypeError, match="Bconds"):
        net.predict_paths(inputs, 2)


def test_hops_below_one_raise():
    from scone_gcn_amd.scone_trajectory_model import Scone_GCN
    net = Scone_GCN(1, 1e-3, 4, 0.0, verbose=False)
    with pytest.raises(ValueError):
        net.multi_hop_accuracy_binary(None, [None, [0], None], None, None, None, None, [0], [1], 0)
    with pytest.raises(ValueError):
        net.multi_hop_accuracy_dist(None, [None, [0], None], [0], [], None, None, [0], None, 0)
