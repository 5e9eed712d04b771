"""The harmonic projection baseline without a GPU: this file's NumPy fp64 restatement of the reference's projection model by two routes
-- the dense null_space of L1 the reference itself takes, and the route the device takes (random probes, conjugate gradients on L1 X =
L1 R, Gram eigendecomposition, doubling of the probes while none drops out) -- both checked against tests/golden/cfg1_projection.npz,
the outputs of the reference's own functions (tests/golden/make_golden_projection.py).  Plus the small complexes whose harmonic
space is known in closed form, the argument checks that need no device and the -projection switch.  tests/test_gpu_projection.py
imports the restatement and the complexes."""
import ctypes
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.linalg import null_space

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL = 1e-9                    # against the fixture: the routes differ by 9e-12, the smallest top-two logit gap is 1.1e-5
MAX_PROBES, DROP, GAP = 32, 1e-12, 1e6


# ------------------------------------------------------------------------------------------------------------------
# complexes
# ------------------------------------------------------------------------------------------------------------------

def incidence(n_nodes, edges, faces):
    """Dense B1 (V, E), B2 (E, F): -1 at an edge's tail, +1 at its head; a face (a, b, c) takes (a, b), (b, c) with +1, (a, c) with -1."""
    edges, faces = np.asarray(edges, np.int64).reshape(-1, 2), np.asarray(faces, np.int64).reshape(-1, 3)
    at = {tuple(e): i for i, e in enumerate(edges.tolist())}
    B1, B2 = np.zeros((n_nodes, len(edges))), np.zeros((len(edges), len(faces)))
    B1[edges[:, 0], np.arange(len(edges))] = -1
    B1[edges[:, 1], np.arange(len(edges))] = 1
    for j, (a, b, c) in enumerate(faces.tolist()):
        B2[at[(a, b)], j] = B2[at[(b, c)], j] = 1
        B2[at[(a, c)], j] = -1
    assert not (B1 @ B2).any()
    return B1, B2


def neighbour_table(n_nodes, edges):
    rows = [set() for _ in range(n_nodes)]
    for a, b in np.asarray(edges).tolist():
        rows[a].add(b)
        rows[b].add(a)
    D = max(1, max(len(r) for r in rows))
    nbr = np.full((n_nodes, D), -1, np.int64)
    for v, r in enumerate(rows):
        nbr[v, :len(r)] = sorted(r)
    return nbr, (nbr >= 0).sum(axis=1)


class Cx:
    """n_nodes, sorted edges (E, 2), sorted faces (F, 3) and what follows from them."""

    def __init__(self, n_nodes, edges, faces):
        self.n_nodes = int(n_nodes)
        self.edges = np.asarray(sorted(tuple(sorted(e)) for e in np.asarray(edges).tolist()), np.int64).reshape(-1, 2)
        self.faces = np.asarray(sorted(tuple(sorted(f)) for f in np.asarray(faces).tolist()), np.int64).reshape(-1, 3)
        self.B1, self.B2 = incidence(self.n_nodes, self.edges, self.faces)
        self.L1 = sp.csr_matrix(self.B1.T @ self.B1 + self.B2 @ self.B2.T)
        self.nbr, self.deg = neighbour_table(self.n_nodes, self.edges)
        self.E, self.D = len(self.edges), self.nbr.shape[1]
        self.at = {tuple(e): i for i, e in enumerate(self.edges.tolist())}

    def flow(self, walk):
        """(E,) flow of a node walk: +1 along an edge's orientation, -1 against it, summed over the steps."""
        f = np.zeros(self.E)
        for a, b in zip(walk[:-1], walk[1:]):
            f[self.at[(min(a, b), max(a, b))]] += 1.0 if a < b else -1.0
        return f


@functools.lru_cache(None)
def cfg1():
    c = np.load(os.path.join(GOLDEN, "cfg1_complex.npz"))
    return Cx(int(c["n_nodes"]), c["edges"], c["faces"])


@functools.lru_cache(None)
def cfg1_data():
    """flows (E, N) forward / reversed, last nodes, target slots, masks of the 1000 fixture walks."""
    p, E = np.load(os.path.join(GOLDEN, "cfg1_paths.npz")), cfg1().E

    def dense(name):
        ptr, X = p[name + "_ptr"], np.zeros((E, len(p["last1"])))
        X[p[name + "_idx"], np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))] = p[name + "_val"]
        return X
    return {"fwd": dense("flow1"), "rev": dense("rev_flow1"), "last": p["last1"].astype(np.int64), "rev_last": p["rev_last1"].astype(np.int64),
            "target": p["targets1"].astype(np.int64), "rev_target": p["rev_targets1"].astype(np.int64), "test": p["test_mask"] == 1,
            "transfer": np.arange(len(p["last1"])) % 3 == 2}


@functools.lru_cache(None)
def fixture():
    z = np.load(os.path.join(GOLDEN, "cfg1_projection.npz"))
    return {k: z[k] for k in z.files}


def tiny4():
    t = np.load(os.path.join(GOLDEN, "tiny4_complex.npz"))
    return Cx(4, t["edges"], t["faces"])


def cycle4():
    return Cx(4, [(0, 1), (1, 2), (2, 3), (0, 3)], [])


def two_cycles():
    return Cx(8, [(0, 1), (1, 2), (2, 3), (0, 3), (4, 5), (5, 6), (6, 7), (4, 7)], [])


def wheel70():
    """Hub 0, rim 1 .. 70, 68 of the 70 triangles (0, i, i + 1) filled: two holes, and 70 neighbours at the hub."""
    rim = [tuple(sorted((i, i % 70 + 1))) for i in range(1, 71)]
    return Cx(71, [(0, i) for i in range(1, 71)] + rim, [(0,) + e for e in rim if e not in ((7, 8), (40, 41))])


def buoy():
    z = np.load(os.path.join(GOLDEN, "buoy.npz"))
    edges = np.unique(np.sort(z["elist"].astype(np.int64).T, axis=1), axis=0)          # 0-based in the fixture
    faces = np.unique(np.sort(z["tlist"].astype(np.int64).T, axis=1), axis=0)
    return Cx(int(edges.max()) + 1, edges, faces)


# ------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------

def basis_null_space(cx):
    """The reference's route (PM:58-71)."""
    return null_space(cx.L1.toarray())


def cg_solve(A, B, tol, max_iter):
    """X of A X = B from 0, all columns at once, a column frozen once |r| <= tol |r0| or when its p.Ap is not positive:
    (X, iterations, largest relative residual, converged)."""
    X, R = np.zeros_like(B), B.copy()
    rr0 = (R * R).sum(axis=0)
    rr, frozen, P = rr0.copy(), ~(rr0 > tol * tol * rr0), R.copy()
    it = 0
    while not frozen.all() and it < max_iter:
        it += 1
        AP = A @ P
        den = (P * AP).sum(axis=0)
        frozen = frozen | ~(den > 0)
        alpha = np.where(frozen, 0.0, rr / np.where(frozen, 1.0, den))
        X, R = X + alpha * P, R - alpha * AP
        rr_new = (R * R).sum(axis=0)
        frozen = frozen | ~(rr_new > tol * tol * rr0)
        P = R + np.where(frozen, 0.0, rr_new / np.where(rr > 0, rr, 1.0)) * P
        rr = rr_new
    rel = np.sqrt(rr[rr0 > 0] / rr0[rr0 > 0])
    return X, it, float(rel.max()) if len(rel) else 0.0, bool(frozen.all())


def kept(w, scale):
    """Eigenvalues (ascending) above DROP * lambda_max, less those below a gap wider than GAP among them; none when lambda_max is
    itself noise against the probes' mean squared norm."""
    if not w[-1] > DROP * scale:
        return np.zeros(len(w), bool)
    keep = w > DROP * w[-1]
    k = np.flatnonzero(keep)
    for a, b in zip(k[:-1], k[1:]):
        if w[b] > GAP * w[a]:
            keep[:b] = False
    return keep


def sift(H, scale):
    w, U = np.linalg.eigh(H.T @ H)
    keep = kept(w, scale)
    return H @ (U[:, keep] / np.sqrt(w[keep])), w


def basis_cg(cx, n_probes=8, seed=0, tol=1e-12, max_iter=50000):
    """The device's route: (V, n_probes used, iterations, residual, eigenvalues of the last H^T H)."""
    while True:
        R = np.random.RandomState(seed).randn(cx.E, n_probes)
        X, it, res, done = cg_solve(cx.L1, cx.L1 @ R, tol, max_iter)
        if not done:
            raise RuntimeError("not converged: %.3e" % res)
        V, w = sift(R - X, float((R ** 2).sum() / n_probes))
        if V.shape[1] < n_probes:
            break
        if 2 * n_probes > MAX_PROBES:
            raise ValueError("every eigenvalue kept")
        n_probes *= 2
    if V.shape[1]:
        V, _ = sift(V, 1.0)
    return V, n_probes, it, res, w


def ref_predict(cx, V, flows, last, D=None):
    """(probs (N, D), logits (N, D)) of PM:80-96 for flows (E, N): the projected flow on the edges at the last node, times the
    neighbours' incidence rows, soft-max over all D slots."""
    D = cx.D if D is None else D
    projs = V @ (V.T @ flows)
    res = np.zeros((len(last), D))
    for i, v in enumerate(last):
        n0, e0 = cx.nbr[v, :cx.deg[v]], np.flatnonzero(cx.B1[v])
        res[i, :len(n0)] = cx.B1[n0][:, e0] @ projs[e0, i]
    ex = np.exp(res - res.max(axis=1, keepdims=True))
    return ex / ex.sum(axis=1, keepdims=True), res


def ref_loss(probs, target):
    """PM:98-105 for probs (N, D) and target slots: log 0 counts as 0, divided by the number of rows."""
    with np.errstate(divide="ignore"):
        lg = np.log(probs[np.arange(len(target)), target])
    lg[lg == -np.inf] = 0
    return float(-lg.sum() / len(target))


def ref_accuracy(probs, target):
    return float(np.average(np.argmax(probs, axis=1) == target))


def two_target_score(probs, target, other):
    """What PM:121-124 adds for each row given the drawn other slot."""
    pt, po = probs[np.arange(len(target)), target], probs[np.arange(len(target)), other]
    return np.where(pt == po, 0.5, np.where(pt > po, 1.0, 0.0))


# ------------------------------------------------------------------------------------------------------------------
# the fixture against both routes
# ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def cfg1_bases():
    return {"null_space": basis_null_space(cfg1()), "cg": basis_cg(cfg1())[0]}


def check_against_fixture(probs_of, proj8):
    """probs_of(which) -> (N, D) for "fwd" / "rev"; proj8 (8, E).  Everything the fixture holds, to TOL; arg-max and accuracy exactly."""
    fx, d = fixture(), cfg1_data()
    rows = fx["prob_rows"]
    assert np.abs(proj8 - fx["proj8"]).max() <= TOL
    for which, last, target in (("fwd", "last", "target"), ("rev", "rev_last", "rev_target")):
        probs = probs_of(which)
        assert probs.shape == (1000, 13) and np.abs(probs[rows] - fx["probs_" + which]).max() <= TOL
        assert np.array_equal(np.argmax(probs, axis=1), fx["argmax_" + which])          # all 1000 rows
        for name, mask in (("test", d["test"]), ("transfer", d["transfer"])):
            if which == "rev" and name == "transfer":
                continue
            want = fx[name if which == "fwd" else "rev_test"]
            assert abs(ref_loss(probs[mask], d[target][mask]) - want[0]) <= TOL
            assert ref_accuracy(probs[mask], d[target][mask]) == want[1]


@pytest.mark.parametrize("route", ("null_space", "cg"))
def test_restatement_agrees_with_the_reference_outputs(route):
    cx, d, V = cfg1(), cfg1_data(), cfg1_bases()[route]
    assert V.shape == (1001, int(fixture()["dim"])) == (1001, 2)
    check_against_fixture(lambda which: ref_predict(cx, V, d[which], d["last" if which == "fwd" else "rev_last"])[0],
                          (V @ (V.T @ d["fwd"][:, :8])).T)


def test_fixture_is_consistent():
    fx, d = fixture(), cfg1_data()
    assert len(fx["prob_rows"]) == 1000 and fx["all_fwd"][1] == 0.519 and fx["test"][1] == 0.55
    probs = fx["probs_fwd"]
    assert np.allclose(probs.sum(axis=1), 1.0, atol=1e-12)
    deg = cfg1().deg[d["last"]]
    assert np.array_equal(np.diff(fx["tt_ptr"]), deg - 1)
    row = np.repeat(np.arange(1000), np.diff(fx["tt_ptr"]))
    other = fx["tt_other"].astype(np.int64)
    assert (other < deg[row]).all() and (other != d["target"][row]).all()
    assert np.array_equal(two_target_score(probs[row], d["target"][row], other), fx["tt_score"])


def test_cg_route_finds_the_gap_and_the_projector():
    cx = cfg1()
    V, used, it, res, w = basis_cg(cx)
    N0 = cfg1_bases()["null_space"]
    assert used == 8 and V.shape[1] == 2 and res <= 1e-12 and 0 < it < 2000
    assert w[-3] <= 1e-13 and w[-2] > 1.0                        # dropped against kept: the rank is no guess
    assert np.abs(V @ V.T - N0 @ N0.T).max() <= 1e-10
    assert np.abs(V.T @ V - np.eye(2)).max() <= 1e-12 and np.abs(cx.L1 @ V).max() <= 1e-9


def test_solve_errors_above_the_fixed_threshold_are_dropped_at_the_gap():
    """The eigenvalues embed() met at |E| = 996 634 (profiles/projection.txt): six squared solve errors of 1e-12 .. 8e-12 under
    4.15 and 7.25, one of them above 1e-12 lambda_max.  The module's rule and the restatement's, on those and on the edge cases."""
    from scone_gcn_amd.projection_model import kept_eigenvalues
    met = np.array([1.1589143443878565e-12, 1.8008044339715867e-12, 2.616470134017326e-12, 5.246034833915078e-12, 6.61278314377704e-12,
                    8.235735340939297e-12, 4.15015974185983, 7.253739577701286])
    assert met[5] > DROP * met[-1]
    cases = [(met, 1e6, [6, 7]), (np.array([-1e-15, 1e-16, 2.7, 7.8]), 1001.0, [2, 3]), (np.array([1e-31, 3e-31]), 5.0, []),
             (np.array([0.03, 2.0, 30.0]), 100.0, [0, 1, 2]), (np.array([1e-11, 2e-11, 3.0, 4e7]), 1e6, [3]), (np.array([0.0]), 1.0, []),
             (np.array([5.0]), 1.0, [0]), (np.array([1e-11, 1e-4, 3.0]), 10.0, [1, 2])]
    for w, scale, want in cases:
        assert np.flatnonzero(kept_eigenvalues(w, scale)).tolist() == np.flatnonzero(kept(w, scale)).tolist() == want, w
    # on the 400-point complex: the harmonic part of the probes plus an error of that size inside range(L1)
    cx = cfg1()
    R = np.random.RandomState(0).randn(cx.E, 8)
    X, _, _, _ = cg_solve(cx.L1, cx.L1 @ R, 1e-12, 5000)
    noise = cx.L1 @ np.random.RandomState(1).randn(cx.E, 8)
    H = R - X + 3e-6 * noise / np.linalg.norm(noise, axis=0)
    w = np.linalg.eigvalsh(H.T @ H)
    assert (w[:6] > DROP * w[-1]).any() and np.flatnonzero(kept(w, 1001.0)).tolist() == [6, 7]
    V, _ = sift(H, 1001.0)
    N0 = cfg1_bases()["null_space"]
    assert V.shape[1] == 2 and np.abs(V @ V.T - N0 @ N0.T).max() <= 1e-5


@pytest.mark.parametrize("n_probes", (1, 2))
def test_too_few_probes_double(n_probes):
    V, used, _, _, _ = basis_cg(cfg1(), n_probes=n_probes)
    N0 = cfg1_bases()["null_space"]
    assert used == 4 and V.shape[1] == 2 and np.abs(V @ V.T - N0 @ N0.T).max() <= 1e-10


def test_known_harmonic_spaces():
    V, used, it, res, _ = basis_cg(tiny4())
    assert V.shape == (5, 0) and it <= 8 and np.isfinite(res)    # no hole: every logit 0, every slot 1 / D
    cx = tiny4()
    probs, _ = ref_predict(cx, V, np.stack([cx.flow([2, 3, 0]), cx.flow([1, 0, 3])], axis=1), [0, 3])
    assert (probs == 1.0 / 3.0).all()
    cx = cycle4()
    V = basis_cg(cx)[0]
    s = cx.flow([0, 1, 2, 3, 0])                                 # the cycle's sign vector: (0, 3) runs against it
    assert s.tolist() == [1.0, -1.0, 1.0, 1.0] and V.shape[1] == 1 and np.abs(V @ V.T - np.outer(s, s) / 4).max() <= 1e-14
    assert basis_cg(two_cycles())[0].shape[1] == 2
    cx = wheel70()
    assert cx.E == 140 and len(cx.faces) == 68 and cx.deg[0] == 70
    assert basis_cg(cx)[0].shape[1] == null_space(cx.L1.toarray()).shape[1] == 2
    cx = buoy()
    assert cx.edges.min() == 0 and (cx.n_nodes, cx.E, len(cx.faces)) == (133, 320, 186)
    # two holes: the dimension of the reference's own null_space on the complex buoy_data.buoy_complex builds from the fixture.  (Read
    # as 1-based -- every id lowered by one -- node -1 wraps round to the last node and closes a third, spurious cycle.)
    assert basis_cg(cx)[0].shape[1] == null_space(cx.L1.toarray()).shape[1] == 2


def test_saturated_probes_raise():
    """A graph of 33 disjoint 4-cycles has 33 harmonic dimensions: 32 probes keep every eigenvalue."""
    edges = [(4 * c + a, 4 * c + b) for c in range(33) for a, b in ((0, 1), (1, 2), (2, 3), (0, 3))]
    with pytest.raises(ValueError):
        basis_cg(Cx(132, edges, []), n_probes=16)


# ------------------------------------------------------------------------------------------------------------------
# what needs no device: the module's surface, the switch, the argument checks of the C-ABI
# ------------------------------------------------------------------------------------------------------------------

def test_module_exposes_the_reference_names():
    from scone_gcn_amd import projection_model as pm
    for name in ("build_flow", "embed", "project_flows", "loss", "accuracy", "accuracy_2target", "eval_dataset", "Projection_Model"):
        assert callable(getattr(pm, name))
    assert pm.SCN_PROJECT_MAX_PROBES == MAX_PROBES and pm.DROP == DROP
    import inspect
    assert list(inspect.signature(pm.project_flows).parameters) == ["V", "B1", "flows", "last_nodes", "nbrhoods", "max_deg"]
    assert list(inspect.signature(pm.eval_dataset).parameters)[:10] == ["G", "paths", "last_nodes", "y", "edge_to_idx", "idx_to_edge",
                                                                         "target_nodes", "B1", "B2", "max_deg"]
    assert "flip" in pm.__doc__


def test_host_functions_follow_the_reference():
    from scone_gcn_amd import projection_model as pm
    fx, d = fixture(), cfg1_data()
    y = np.zeros((13, 1000))
    y[d["target"], np.arange(1000)] = 1
    m = d["test"]
    assert abs(pm.loss(y[:, m], fx["probs_fwd"][m].T) - fx["test"][0]) <= 1e-12
    assert pm.accuracy(y[:, m], fx["probs_fwd"][m].T) == fx["test"][1]
    assert pm.loss(np.array([[1.0], [0.0]]), np.array([[0.0], [1.0]])) == 0.0                # log 0 counts as 0 (PM:104)

    class G:
        edges = [(0, 1), (0, 2), (1, 2)]
    assert pm.build_flow(G, [2, 0, 1], {e: i for i, e in enumerate(G.edges)}).tolist() == [1.0, -1.0, 0.0]


def test_class_checks_its_arguments_before_touching_a_device():
    from scone_gcn_amd.projection_model import Projection_Model
    for bad in (0, 33, 2.5):
        with pytest.raises(ValueError, match="n_probes"):
            Projection_Model(n_probes=bad)
    with pytest.raises(ValueError, match="tol"):
        Projection_Model(tol=0.0)
    pm = Projection_Model()
    assert (pm.n_probes, pm.seed, pm.tol, pm.max_iter) == (8, 0, 1e-12, 50000) and pm.basis is None and pm.dim is None
    with pytest.raises(RuntimeError, match="embed"):
        pm.predict(np.zeros((5, 1)), [0])
    with pytest.raises(TypeError):
        pm.embed(np.zeros((4, 5)))


def test_hyperparams_have_projection():
    from scone_gcn_amd import trajectory_experiments as te
    assert te.hyperparams(["prog"])["projection"] == 0
    assert te.hyperparams(["prog", "-projection", "1"])["projection"] == 1


def test_unsupported_and_empty_calls_return_before_any_launch():
    from scone_gcn_amd import _lib
    lib = _lib.load()
    src = open(os.path.join(ROOT, "include", "scone_hip.h")).read()
    assert "#define SCN_PROJECT_MAX_K 32" in src and _lib.SCN_PROJECT_MAX_K == 32
    U, seed, tol = _lib.SCN_ERR_UNSUPPORTED, ctypes.c_uint64(0), ctypes.c_double(1e-12)
    for k in (0, 33, -1):
        assert lib.scn_csr_apply_f64(5, k, None, None, None, None, None, None, None) == U
        assert lib.scn_cg_update_xr(5, k, 1, 0, None, None, None, None, None, None, None, None, None) == U
        assert lib.scn_cg_update_p(5, k, 1, 0, tol, None, None, None, None, None, None) == U
        assert lib.scn_gram_f64(5, k, 3, None, None, None, None, None) == U and lib.scn_gram_f64(5, 3, k, None, None, None, None, None) == U
        assert lib.scn_project_parts(5, k) == U
    pred = lambda n, k: lib.scn_project_predict(n, k, 5, None, None, None, None, None, 4, None, None, None, None, 3, None, None, None,
                                                None, None, None, None)
    assert pred(3, 33) == U and pred(3, -1) == U and pred(0, 2) == 0 and pred(3, 2) == _lib.SCN_ERR_BAD_ARG and pred(-1, 2) == -2
    assert lib.scn_csr_apply_f64(0, 8, None, None, None, None, None, None, None) == 0
    assert lib.scn_cg_update_xr(0, 8, 1, 0, None, None, None, None, None, None, None, None, None) == 0
    assert lib.scn_cg_update_p(0, 8, 1, 0, tol, None, None, None, None, None, None) == 0
    assert lib.scn_gram_f64(0, 8, 8, None, None, None, None, None) == 0
    assert lib.scn_project_two_target(0, 13, seed, None, None, None, None, None, None, None) == 0
    assert lib.scn_csr_apply_f64(5, 8, None, None, None, None, None, None, None) == _lib.SCN_ERR_BAD_ARG
    assert lib.scn_csr_apply_f64(-1, 8, None, None, None, None, None, None, None) == -2
    # a wave covers 64 / k rows, a workgroup four waves, at most 1024 workgroups
    for n, k, want in ((1001, 1, 4), (1001, 3, 12), (1001, 8, 32), (1001, 32, 126), (5, 8, 1), (0, 8, 1), (10 ** 6, 8, 1024)):
        assert lib.scn_project_parts(n, k) == want, (n, k)
    assert lib.scn_gram_parts(1001) == 16 and lib.scn_gram_parts(10 ** 6) == 1024 and lib.scn_gram_parts(0) == 1
