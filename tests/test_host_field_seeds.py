"""The end-to-end data of tests/test_gpu_field.py on the fp64 oracle alone, without a GPU: with these seeds no root comes within 1e-5
of a tie at any level of the greedy rollout or of the beam search, so a root the GPU tests leave out as a near-tie is fp32's doing
(and at most one may be).  tests/test_host_multihop.oracle_model is dense (B1 and both shifts as ndarrays: 8.6 GB and 2 x 23 GB at
this complex), so the model here runs the oracle's own layer loop (so.conv_forward) on scipy operators and a sparse readout operand;
the first test ties it to oracle_model on a complex small enough for both."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import scone_oracle as so
from tests.test_host_multihop import oracle_model

N_ROOTS = 11                                             # the last slab of four trajectories is partial
N_POINTS = 20000                                         # |E| = 53 801
WALK_SEED, DATA_SEED, WEIGHT_SEED, WEIGHT_SCALE = 3, 2, 1030, 20.0
GAP = 1e-5


def sparse_oracle_model(weights, B1, B2, nbr):
    """model_fn(last (n,), flows (n, E)) -> log-probabilities (n, D) of the scone oracle: so.conv_forward on scipy shifts, and
    logits = Bcond(v) @ H @ W_last, log-softmax over all D slots, with Bcond(v) = the rows nbr[v] of B1 (a zero row for -1)."""
    B1 = sp.csr_matrix(B1)
    B2 = sp.csr_matrix(B2)
    S_lo, S_up = (B1.T @ B1).tocsr(), (B2 @ B2.T).tocsr()
    B1_ext = sp.vstack([B1, sp.csr_matrix((1, B1.shape[1]))]).tocsr()

    def fn(last, X):
        H = so.conv_forward(weights, S_lo, S_up, np.asarray(X, np.float64)[:, :, None])
        out = []
        for n, v in enumerate(np.asarray(last)):
            logits = (B1_ext[nbr[int(v)]] @ H[n]) @ weights[-1]
            out.append((logits - so.logsumexp(logits, axis=0))[:, 0])
        return np.stack(out)
    return fn


def test_sparse_model_is_the_oracle_model():
    from scone_gcn_amd import synthetic_data_gen as g
    cx = g.random_SC_graph(300)
    B1, B2 = (m.toarray() for m in g.incidence_matrices(cx))
    nbr, _ = so.neighborhoods(cx.edges, cx.n_nodes)
    rs = np.random.RandomState(4)
    w = [0.3 * rs.randn(*s) for s in so.weight_shapes(1, [(3, 16)] * 3, 1)]
    last = rs.randint(0, cx.n_nodes, size=6)
    X = rs.choice([-1.0, 0.0, 1.0], size=(6, cx.n_edges))
    want = oracle_model("scone", w, B1, B2, cx.edges, cx.n_nodes)(last, X)
    got = sparse_oracle_model(w, B1, B2, nbr)(last, X)
    assert np.array_equal(np.isfinite(want), np.isfinite(got))
    assert np.allclose(got, want, rtol=0, atol=1e-12)


def gap_ok(scores, keep, gap=GAP):
    """Whether the `keep` best of the candidate scores are separated from each other and from the next one by more than gap."""
    s = np.asarray(scores, np.float64)
    s = np.sort(s[np.isfinite(s)])[::-1][:keep + 1]
    return len(s) < 2 or float(np.min(-np.diff(s))) > gap


def host_weights(hidden):
    """What Scone_GCN.setup installs after reseed(WEIGHT_SEED) and the GPU tests then scale: 0.01 randn in fp32, times 20 in fp32."""
    rs = np.random.RandomState(WEIGHT_SEED)
    shapes = so.weight_shapes(1, [(3, hidden)] * 3, 1)
    return [(np.float32(0.01 * rs.randn(*s)) * np.float32(WEIGHT_SCALE)).astype(np.float64) for s in shapes]


@pytest.fixture(scope="module")
def host_world():
    from scone_gcn_amd import synthetic_data_gen as g
    cx = g.random_SC_graph(N_POINTS)
    paths = g.generate_random_walks(cx, m=N_ROOTS, seed=WALK_SEED)
    flows, _, last, _, _ = g.path_dataset(cx, paths, seed=DATA_SEED)
    X = flows.todense() if isinstance(flows, g.SparseFlows) else np.asarray(flows)
    X = np.asarray(X, np.float64).reshape(N_ROOTS, cx.n_edges)
    B1, B2 = g.incidence_matrices(cx)
    nbr, _ = so.neighborhoods(cx.edges, cx.n_nodes)
    E_lookup = {(int(a), int(b)): k for k, (a, b) in enumerate(cx.edges.tolist())}
    return {"cx": cx, "X": X, "last": np.asarray(last), "B1": B1, "B2": B2, "nbr": nbr, "E_lookup": E_lookup}


def _step(E_lookup, x, v, u):
    """The flow after the step v -> u: the step SETS its edge (+1 along the stored orientation, lower id first)."""
    x = x.copy()
    x[E_lookup[(min(v, u), max(v, u))]] = 1.0 if v < u else -1.0
    return x


@pytest.mark.parametrize("hidden", [32, 16])
@pytest.mark.parametrize("beam", [4, 1])
def test_no_root_of_the_gpu_tests_is_a_near_tie(host_world, hidden, beam):
    """Beam search of 3 hops (beam 1: the greedy rollout) in fp64: at every level, for every root, the kept candidates and the best
    one left out lie more than 1e-5 apart -- the test the GPU tests apply to the dense fp32 candidates before they compare paths."""
    wd = host_world
    nbr, E_lookup = wd["nbr"], wd["E_lookup"]
    deg = (nbr >= 0).sum(axis=1)
    model = sparse_oracle_model(host_weights(hidden), wd["B1"], wd["B2"], nbr)
    hops = 3
    entries = [[(int(wd["last"][i]), wd["X"][i], 0.0)] for i in range(N_ROOTS)]
    smallest = np.inf
    for h in range(hops):
        W2 = min(beam, len(entries[0]) * nbr.shape[1])
        new = []
        flat = [e for ent in entries for e in ent]                           # one forward per level over every root's entries
        logp_all = model([e[0] for e in flat], np.stack([e[1] for e in flat]))
        first = np.cumsum([0] + [len(ent) for ent in entries])
        for i in range(N_ROOTS):
            logp = logp_all[first[i]:first[i + 1]]
            cand = [(s + logp[k, j], k, j) for k, (v, _, s) in enumerate(entries[i]) for j in range(deg[v])]
            scores = [c[0] for c in cand]
            assert gap_ok(scores, W2), (h, i)
            top = np.sort(scores)[::-1][:W2 + 1]
            if len(top) > 1:
                smallest = min(smallest, float(np.min(-np.diff(top))))
            kept = sorted(cand, key=lambda c: -c[0])[:W2]
            new.append([(int(nbr[entries[i][k][0], j]), _step(E_lookup, entries[i][k][1], entries[i][k][0], int(nbr[entries[i][k][0], j])), s)
                        for s, k, j in kept])
        entries = new
    print("hidden %d, beam %d: smallest gap between kept candidates %.3e" % (hidden, beam, smallest))
    assert smallest > GAP
