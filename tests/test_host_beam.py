"""Beam-search multi-hop prediction without a GPU: this file's fp64 restatement of Scone_GCN.predict_paths_beam (used by
tests/test_gpu_beam.py for its order rule) checked against brute force on the 4-node graph -- at beam = 1 it walks the greedy path,
at full width it is the probability tree -- plus the argument checks and the -beam switch."""
import os
import re

import numpy as np
import pytest

from oracle import scone_oracle as so
from scone_gcn_amd._lib import SCN_BEAM_MAX
from tests.test_host_multihop import _tiny4, oracle_model, ref_target_probs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------
# fp64 restatement: model_fn(last_nodes (n,), flows (n, E)) -> log-probabilities (n, D)
# ------------------------------------------------------------------------------------------------------------------

def order_key(score, k, j):
    """The beam's total order as a sort key (ascending = best first): a NaN before every number, then the higher score, then the
    lower parent k, then the lower slot j."""
    return (0, 0.0, k, j) if np.isnan(score) else (1, -float(score), k, j)


def step_flow(flow, v, u, E_lookup):
    """The "binary" step v -> u (STM:139-147): SET +1 on E_lookup[(v, u)] if that key exists, else -1 on E_lookup[(u, v)]."""
    f = flow.copy()
    if (v, u) in E_lookup:
        f[E_lookup[(v, u)]] = 1
    else:
        f[E_lookup[(u, v)]] = -1                                             # KeyError when neither key exists
    return f


def ref_beam(model_fn, flows, last_nodes, nbrhoods, E_lookup, hops, beam):
    """Per trajectory the list of (path (hops node ids), score), best first, at most `beam` long.  Entry = (node, flow, score, path);
    a level is one model_fn call over every entry of every trajectory; the candidates of a trajectory are every (entry k, slot j <
    degree of the entry's node)."""
    nb = np.asarray(nbrhoods)
    deg = (nb >= 0).sum(axis=1)
    beams = [[(int(last_nodes[i]), np.array(flows[i], np.float64), 0.0, ())] for i in range(len(flows))]
    for _ in range(hops):
        flat = [(i, k, e) for i in range(len(beams)) for k, e in enumerate(beams[i])]
        logp = model_fn(np.asarray([e[0] for _, _, e in flat]), np.stack([e[1] for _, _, e in flat]))
        cands = [[] for _ in beams]
        for n, (i, k, (v, f, s, path)) in enumerate(flat):
            for j in range(deg[v]):
                cands[i].append((s + logp[n, j], k, j))
        new = []
        for i, cs in enumerate(cands):
            kept = sorted(cs, key=lambda c: order_key(*c))[:beam]
            out = []
            for s, k, j in kept:
                v, f, _, path = beams[i][k]
                u = int(nb[v][j])
                out.append((u, step_flow(f, v, u, E_lookup), s, path + (u,)))
            new.append(out)
        beams = new
    return [[(e[3], e[2]) for e in b] for b in beams]


# ------------------------------------------------------------------------------------------------------------------
# the 4-node graph (PM:128-151)
# ------------------------------------------------------------------------------------------------------------------

def _case(model_type):
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
    return fn, flows, np.array([1, 1, 0, 3]), nb, E_lookup


@pytest.mark.parametrize("model_type", ["scone", "ebli", "bunch"])
def test_beam_of_one_walks_the_greedy_path(model_type):
    fn, flows, last, nb, E_lookup = _case(model_type)
    hops = 3
    got = ref_beam(fn, flows, last, nb, E_lookup, hops, 1)
    for i in range(4):
        assert len(got[i]) == 1 and len(got[i][0][0]) == hops
        v, f, total = int(last[i]), flows[i].copy(), 0.0
        for u in got[i][0][0]:
            # one forward per step, as a host loop would run it.  The graph's symmetry makes two neighbours of node 2 tie to the last
            # bits of fp64, where the batched and the single forward round differently: the step taken must be A maximum to 1e-12
            lp = fn(np.array([v]), f[None])[0]
            live = lp[:(nb[v] >= 0).sum()]
            j = list(nb[v]).index(u)
            assert j < len(live) and live[j] >= live.max() - 1e-12
            f = step_flow(f, v, int(u), E_lookup)
            total += lp[j]
            v = int(u)
        assert abs(got[i][0][1] - total) <= 1e-12


@pytest.mark.parametrize("model_type", ["scone", "ebli", "bunch"])
@pytest.mark.parametrize("hops", [1, 2, 3])
def test_full_width_beam_is_the_probability_tree(model_type, hops):
    """Averaging exp(score) over the paths that end at t gives ref_target_probs (the tree multiplies probabilities where the beam
    adds their logarithms: a few units in the last place of fp64 apart, hence 1e-12 and not 0); NaN where no path ends at t."""
    fn, flows, last, nb, E_lookup = _case(model_type)
    got = ref_beam(fn, flows, last, nb, E_lookup, hops, SCN_BEAM_MAX)
    deg = (nb >= 0).sum(axis=1)
    for i in range(4):
        count, level = 0, [int(last[i])]                                       # brute-force number of paths
        for _ in range(hops):
            level = [int(u) for v in level for u in nb[v][:deg[v]]]
        count = len(level)
        assert count < SCN_BEAM_MAX and len(got[i]) == count
        assert len(set(p for p, _ in got[i])) == count                         # every path once
        scores = [s for _, s in got[i]]
        assert all(a >= b for a, b in zip(scores, scores[1:]))
    for t in range(4):
        targets = np.full(4, t)
        want = ref_target_probs(fn, flows, targets, nb, E_lookup, last, hops)
        for i in range(4):
            hit = [np.exp(s) for p, s in got[i] if p[-1] == t]
            if not hit:
                assert np.isnan(want[i])
            else:
                assert abs(np.mean(hit) - want[i]) <= 1e-12


def test_order_rule_on_ties_and_nan():
    """A model that answers the same row everywhere: equal scores fall to the lower parent, then the lower slot; a NaN comes first."""
    _, flows, last, nb, E_lookup = _case("scone")
    row = np.array([-1.0, -1.0, -2.0])
    got = ref_beam(lambda ln, X: np.tile(row, (len(ln), 1)), flows[:1], last[:1], nb, E_lookup, 2, 3)
    # node 1 has the neighbours nb[1][0], nb[1][1]: level 1 keeps slots 0 and 1 (tie, lower slot first); level 2 ties at -2 again
    a, b = int(nb[1][0]), int(nb[1][1])
    assert [p for p, _ in got[0]] == [(a, int(nb[a][0])), (a, int(nb[a][1])), (b, int(nb[b][0]))]
    assert [s for _, s in got[0]] == [-2.0, -2.0, -2.0]
    row_nan = np.array([-1.0, np.nan, -2.0])
    got = ref_beam(lambda ln, X: np.tile(row_nan, (len(ln), 1)), flows[:1], last[:1], nb, E_lookup, 1, 2)
    assert got[0][0][0] == (b,) and np.isnan(got[0][0][1]) and got[0][1] == ((a,), -1.0)
    assert order_key(np.nan, 5, 5) < order_key(np.inf, 0, 0) < order_key(1.0, 0, 0) < order_key(1.0, 0, 1) < order_key(1.0, 1, 0)


# ------------------------------------------------------------------------------------------------------------------
# arguments and switches
# ------------------------------------------------------------------------------------------------------------------

def test_beam_and_hops_below_one_raise():
    from scone_gcn_amd.scone_trajectory_model import Scone_GCN
    net = Scone_GCN(1, 1e-3, 4, 0.0, verbose=False)
    for hops, beam in ((0, 1), (1, 0), (2, -3), (1, SCN_BEAM_MAX + 1)):
        with pytest.raises(ValueError):
            net.predict_paths_beam([None, [0], None], hops, beam)
        with pytest.raises(ValueError):
            net.multi_hop_accuracy_topk([None, [0], None], [0], [1], hops, beam)


def test_probed_closure_is_refused():
    from scone_gcn_amd.scone_trajectory_model import Scone_GCN
    net = Scone_GCN(1, 1e-3, 4, 0.0, verbose=False)
    net.model_type = "scone"
    B1, B2, edges, E_lookup = _tiny4()
    nb, _ = so.neighborhoods(edges, 4)
    inputs = [so.make_Bconds(B1, nb), np.array([1]), np.zeros((1, 5, 1))]
    with pytest.raises(TypeError, match="Bconds"):
        net.predict_paths_beam(inputs, 2, 2)


def test_beam_switch_parses():
    from scone_gcn_amd import trajectory_experiments as te
    assert te.hyperparams(["prog"])["beam"] == 0
    hp = te.hyperparams(["prog", "-multi_hop", "1", "-beam", "4"])
    assert hp["beam"] == 4 and hp["multi_hop"] == 1


def test_beam_max_matches_the_header():
    src = open(os.path.join(ROOT, "include", "scone_hip.h")).read()
    assert int(re.search(r"#define\s+SCN_BEAM_MAX\s+(\d+)", src).group(1)) == SCN_BEAM_MAX >= 256
