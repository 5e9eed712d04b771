"""The harmonic projection baseline on the device: the fp64 kernels of csrc/scn_project.hip through the C-ABI against scipy and the
NumPy restatement of tests/test_host_projection.py, then projection_model.Projection_Model and the -projection 1 switch of
train_model() end to end against tests/golden/cfg1_projection.npz, the outputs of the reference's own functions."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.linalg import null_space

from tests.test_host_projection import (GOLDEN, TOL, basis_null_space, buoy, cfg1, cfg1_data, check_against_fixture, cycle4, fixture,
                                        ref_predict, tiny4, two_cycles, two_target_score, wheel70)

pytestmark = pytest.mark.gpu
EPS = 2.2e-16


def lib():
    from scone_gcn_amd import _lib
    return _lib.load()


def up(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype).contiguous()


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def complex_of(cx, coords=None):
    from scone_gcn_amd.complex import SimplicialComplex
    from scone_gcn_amd.synthetic_data_gen import Complex
    return SimplicialComplex(Complex(n_nodes=cx.n_nodes, edges=cx.edges, faces=cx.faces, coords=coords))


def cfg1_complex():
    return complex_of(cfg1(), np.load(os.path.join(GOLDEN, "cfg1_complex.npz"))["coords"])


def model(cx, sc=None, **kw):
    from scone_gcn_amd.projection_model import Projection_Model
    return Projection_Model(**kw).embed(complex_of(cx) if sc is None else sc)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ------------------------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------------------------

def csr_apply(A, X, status=0, k=None):
    """(Y, parts, the sentinel behind Y) of scn_csr_apply_f64 for a scipy CSR A and X (n, k)."""
    n, k = A.shape[0], X.shape[1] if k is None else k
    W = max(lib().scn_project_parts(n, min(k, 32)), 1)
    rowptr, col, val = up(A.indptr, torch.int32), up(A.indices, torch.int32), up(A.data, torch.float64)
    d_x = up(X)
    y = torch.full((n * X.shape[1] + 64,), -7.0, dtype=torch.float64, device="cuda")
    parts = torch.full((W * X.shape[1] + 64,), -7.0, dtype=torch.float64, device="cuda")
    assert lib().scn_csr_apply_f64(n, k, p(rowptr), p(col), p(val), p(d_x), p(y), p(parts), stream()) == status
    torch.cuda.synchronize()
    y, parts = y.cpu().numpy(), parts.cpu().numpy()
    return y[:n * X.shape[1]].reshape(n, -1), parts[:W * X.shape[1]].reshape(W, -1), np.concatenate([y[n * X.shape[1]:], parts[W * X.shape[1]:]])


def check_csr_apply(A, k, seed):
    """Per entry |y - A x| <= 64 eps sum |a| |x| (a row has at most 25 terms), and the partial sums of x . y add up within the same
    bound on their own terms; against products summed in long double, so the reference's rounding is not in the way."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    assert np.diff(A.indptr).max() <= 25
    X = np.random.RandomState(seed).randn(A.shape[0], k)
    Y, parts, tail = csr_apply(A, X)
    Xl, coo = X.astype(np.longdouble), A.tocoo()
    want, mag = np.zeros(X.shape, np.longdouble), np.zeros(X.shape, np.longdouble)
    np.add.at(want, coo.row, coo.data.astype(np.longdouble)[:, None] * Xl[coo.col])
    np.add.at(mag, coo.row, np.abs(coo.data).astype(np.longdouble)[:, None] * np.abs(Xl[coo.col]))
    err = np.abs(Y - want).astype(np.float64)
    print("k", k, "n", A.shape[0], "largest error / bound", float((err / (64 * EPS * mag + 1e-300)).max()))
    assert (err <= 64 * EPS * mag).all() and (tail == -7.0).all()
    dot, dot_mag = (Xl * want).sum(axis=0), (np.abs(Xl) * mag).sum(axis=0)
    got = parts.astype(np.longdouble).sum(axis=0)
    print("      p.Ap error / bound", float((np.abs(got - dot) / (64 * EPS * dot_mag)).max()))
    assert (np.abs(got - dot) <= 64 * EPS * dot_mag).all()
    Y2, parts2, _ = csr_apply(A, X)
    assert same_bits(Y, Y2) and same_bits(parts, parts2)


@pytest.mark.parametrize("k", (1, 3, 8, 32))
def test_csr_apply_on_the_400_point_laplacian(k):
    """E = 1001 is no multiple of a wave's rows at any k; the rows of the edges round the two holes are the short ones."""
    check_csr_apply(cfg1().L1, k, 5 + k)


def ring_laplacian(n):
    return sp.diags([np.full(n, 2.5), -np.ones(n - 1), -np.ones(n - 1)], [0, 1, -1], format="csr")


@pytest.mark.parametrize("n,k", ((8193, 32), (4 * 64 * 1024 + 3, 1)))
def test_csr_apply_past_the_grid_cap(n, k):
    """More rows than 1024 workgroups cover in one pass (8192 at k = 32, 262 144 at k = 1): the grid-stride loop."""
    assert lib().scn_project_parts(n, k) == 1024
    check_csr_apply(ring_laplacian(n), k, 3)


def test_csr_apply_refuses_k_33_and_launches_nothing():
    from scone_gcn_amd import _lib
    A = sp.csr_matrix(cfg1().L1)
    X = np.random.RandomState(0).randn(A.shape[0], 33)
    Y, parts, tail = csr_apply(A, X, status=_lib.SCN_ERR_UNSUPPORTED)
    assert (Y == -7.0).all() and (parts == -7.0).all() and (tail == -7.0).all()


@pytest.mark.parametrize("n,ka,kb", ((1001, 8, 8), (1001, 3, 32), (63, 1, 1), (65536 + 77, 2, 5), (4097, 32, 32)))
def test_gram_against_numpy(n, ka, kb):
    """n below one workgroup's 64 rows, no multiple of them, and past the 1024 workgroups' 65 536 (the grid-stride loop)."""
    rs = np.random.RandomState(n + ka)
    A, B = rs.randn(n, ka), rs.randn(n, kb)
    W = lib().scn_gram_parts(n)
    outs = []
    for _ in range(2):
        d_a, d_b = up(A), up(B)
        parts = torch.full((W * ka * kb + 64,), -7.0, dtype=torch.float64, device="cuda")
        out = torch.full((ka * kb + 64,), -7.0, dtype=torch.float64, device="cuda")
        assert lib().scn_gram_f64(n, ka, kb, p(d_a), p(d_b), p(parts), p(out), stream()) == 0
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
        assert (parts[W * ka * kb:] == -7.0).all() and (outs[-1][ka * kb:] == -7.0).all()
    got = outs[0][:ka * kb].reshape(ka, kb)
    Al, Bl = A.astype(np.longdouble), B.astype(np.longdouble)
    # any summation order of n products: n eps sum |a| |b| bounds it; the device's tree is far shallower
    assert (np.abs(got - Al.T @ Bl) <= n * EPS * (np.abs(Al).T @ np.abs(Bl))).all()
    assert same_bits(outs[0], outs[1])


def test_cg_kernels_past_the_grid_cap():
    """The update kernels' grid-stride loop (8193 rows at k = 32) and a column that starts converged: the solve of A X = A R gives
    X = R for a positive definite A, the zero probe stays zero and is frozen from the start."""
    from scone_gcn_amd.projection_model import Projection_Model
    from scone_gcn_amd import ops
    A = ring_laplacian(8193)
    R = np.random.RandomState(1).randn(8193, 32)
    R[:, 5] = 0.0
    pm = Projection_Model()
    pm.device = ops.default_device()
    X, it, res, done = pm._solve(A, up(R))
    X = X.cpu().numpy()
    assert done and 0 < it < 200 and res <= 1e-12 and np.isfinite(X).all()
    assert np.abs(X - R).max() <= 1e-10 and not X[:, 5].any()
    X2, it2, res2, _ = pm._solve(A, up(R))
    assert same_bits(X, X2.cpu().numpy()) and (it, res) == (it2, res2)


# ------------------------------------------------------------------------------------------------------------------
# small complexes with a known harmonic space
# ------------------------------------------------------------------------------------------------------------------

def test_four_node_graph_has_no_harmonic_space():
    cx = tiny4()
    pm = model(cx)
    assert pm.dim == 0 and pm.basis.shape == (5, 0) and pm.iterations <= 8 and pm.n_probes_used == 8
    assert np.isfinite(pm.residual) and np.isfinite(pm.gram_eigenvalues).all()
    flows = np.stack([cx.flow([2, 3, 0]), cx.flow([1, 0, 3]), cx.flow([0])], axis=1)
    probs, logits, arg = pm.predict_all(flows, [0, 3, 2])
    assert probs.shape == (3, 3) and (probs == 1.0 / 3.0).all() and not logits.any() and (arg == 0).all()
    assert not pm.project(flows).any()


def test_cycles_without_faces():
    cx = cycle4()
    pm = model(cx)
    s = cx.flow([0, 1, 2, 3, 0])
    assert pm.dim == 1 and np.abs(pm.basis @ pm.basis.T - np.outer(s, s) / 4).max() <= 1e-14
    assert model(two_cycles()).dim == 2


def test_wheel_with_a_hub_wider_than_a_wave():
    """Degree 70 at the hub; a flow of 67 entries, an empty one, walks ending on the rim as well."""
    from scone_gcn_amd.synthetic_data_gen import SparseFlows
    cx = wheel70()
    pm = model(cx)
    assert pm.dim == 2 and pm.width == 70
    walks = [list(range(1, 68)) + [0], [0], [3, 0], [9, 8, 7, 0], [0, 5, 6], [41, 40, 0, 8, 7, 0], [1, 70, 69, 0, 41]]
    flows = np.stack([cx.flow(w) for w in walks], axis=1)
    last = [w[-1] for w in walks]
    assert np.count_nonzero(flows[:, 0]) == 67 and not flows[:, 1].any()
    want, want_logits = ref_predict(cx, basis_null_space(cx), flows, last)
    for form in (flows, SparseFlows.fromdense(flows.T[:, :, None])):
        probs, logits, arg = pm.predict_all(form, last)
        assert np.abs(probs - want).max() <= TOL and np.abs(logits - want_logits).max() <= TOL
        assert np.array_equal(arg, np.argmax(want, axis=1)) and (arg[[0, 2, 3]] < 70).all()
        assert (probs[1] == 1.0 / 70.0).all() and arg[1] == 0
        assert (logits[6, 3:] == 0).all() and np.abs(probs[6, 3:] - probs[6, 3]).max() == 0          # padding at a rim node
    assert np.abs(pm.project(flows) - (basis_null_space(cx) @ basis_null_space(cx).T @ flows).T).max() <= TOL


# ------------------------------------------------------------------------------------------------------------------
# the 400-point complex against the reference's outputs
# ------------------------------------------------------------------------------------------------------------------

def check_cfg1_model(pm):
    cx, d, fx = cfg1(), cfg1_data(), fixture()
    V = pm.basis
    assert pm.dim == 2 and V.shape == (1001, 2)
    assert np.abs(V.T @ V - np.eye(2)).max() <= 1e-12 and np.abs(cx.L1 @ V).max() <= 1e-9
    assert pm.residual <= 1e-12 and 0 < pm.iterations < 2000
    got = {"fwd": pm.predict_all(d["fwd"], d["last"]), "rev": pm.predict_all(d["rev"], d["rev_last"])}
    check_against_fixture(lambda which: got[which][0], pm.project(d["fwd"][:, :8]))
    assert np.array_equal(got["fwd"][2], fx["argmax_fwd"]) and np.array_equal(got["rev"][2], fx["argmax_rev"])     # the kernel's own arg-max
    y, y_rev = np.eye(13)[d["target"]], np.eye(13)[d["rev_target"]]
    for flows, last, yy, mask, want in ((d["fwd"], d["last"], y, d["test"], fx["test"]), (d["rev"], d["rev_last"], y_rev, d["test"], fx["rev_test"]),
                                        (d["fwd"], d["last"], y, d["transfer"], fx["transfer"])):
        ce, acc = pm.test(flows, last, yy, mask.astype(int))
        assert abs(ce - want[0]) <= TOL and acc == want[1]


@pytest.mark.parametrize("n_probes", (3, 8, 32))
def test_embed_and_accuracy_on_the_400_point_complex(n_probes):
    pm = model(None, sc=cfg1_complex(), n_probes=n_probes)
    assert pm.n_probes_used == n_probes
    w = pm.gram_eigenvalues
    assert len(w) == n_probes and w[-3] <= 1e-12 * w[-1] and w[-2] > 1e-3
    check_cfg1_model(pm)


@pytest.mark.parametrize("n_probes", (1, 2))
def test_too_few_probes_double(n_probes):
    pm = model(None, sc=cfg1_complex(), n_probes=n_probes)
    assert pm.n_probes_used == 4
    check_cfg1_model(pm)


def test_incidence_matrices_and_the_module_functions():
    """embed(B1, B2), project_flows and eval_dataset with the reference's arguments: dense matrices, (E, N) flows, y (D, N)."""
    from scone_gcn_amd import projection_model as pmod
    cx, d, fx = cfg1(), cfg1_data(), fixture()
    V, B1 = pmod.embed(cx.B1, sp.csr_matrix(cx.B2))
    assert B1 is cx.B1 and V.shape == (1001, 2)
    N0 = basis_null_space(cx)
    assert np.abs(V @ V.T - N0 @ N0.T).max() <= 1e-10
    rows = np.flatnonzero(d["test"])
    nb = [cx.nbr[n, :cx.deg[n]] for n in d["last"][rows]]
    preds = pmod.project_flows(V, cx.B1, d["fwd"][:, rows], d["last"][rows], nb, 13)
    assert preds.shape == (13, 200) and np.abs(preds.T - fx["probs_fwd"][rows]).max() <= TOL
    wider = pmod.project_flows(N0, cx.B1, d["fwd"][:, rows[:5]], d["last"][rows[:5]], nb[:5], 15)
    assert wider.shape == (15, 5) and np.abs(wider.T - ref_predict(cx, N0, d["fwd"][:, rows[:5]], d["last"][rows[:5]], D=15)[0]).max() <= TOL
    y = np.eye(13)[d["target"][rows]].T
    ce, acc = pmod.eval_dataset(None, None, d["last"][rows], y, None, None, None, cx.B1, cx.B2, 13, flows=d["fwd"][:, rows])
    assert abs(ce - fx["test"][0]) <= TOL and acc == fx["test"][1]
    with pytest.raises(ValueError, match="sorted neighbourhood"):
        pmod.project_flows(V, cx.B1, d["fwd"][:, rows[:2]], d["last"][rows[:2]], [nb[0], nb[1][::-1]], 13)


# ------------------------------------------------------------------------------------------------------------------
# other complexes and failure paths
# ------------------------------------------------------------------------------------------------------------------

def test_drifter_complex():
    """The dimension is the reference's own: null_space of the dense L1 of the complex buoy_data.buoy_complex builds (2)."""
    from scone_gcn_amd.buoy_data import buoy_complex
    from scone_gcn_amd.complex import SimplicialComplex
    z = np.load(os.path.join(GOLDEN, "buoy.npz"))
    cx = buoy()
    sc = SimplicialComplex(buoy_complex(z["elist"].astype(np.int64), z["tlist"].astype(np.int64), z["coords"]))
    assert np.array_equal(sc.cx.edges, cx.edges) and np.array_equal(sc.cx.faces, cx.faces)
    pm = model(None, sc=sc)
    N0 = null_space(cx.L1.toarray())
    assert pm.dim == N0.shape[1] == 2 and np.abs(pm.basis @ pm.basis.T - N0 @ N0.T).max() <= 1e-9


def test_same_seed_same_bits():
    sc = cfg1_complex()
    a, b, c = model(None, sc=sc), model(None, sc=sc), model(None, sc=sc, seed=1)
    assert same_bits(a.basis, b.basis) and (a.iterations, a.residual) == (b.iterations, b.residual)
    assert not same_bits(a.basis, c.basis) and np.abs(a.basis @ a.basis.T - c.basis @ c.basis.T).max() <= 1e-10
    d = cfg1_data()
    assert all(same_bits(x, y) for x, y in zip(a.predict_all(d["fwd"], d["last"]), b.predict_all(d["fwd"], d["last"])))


def test_max_iter_reached_raises_and_installs_no_basis():
    from scone_gcn_amd.projection_model import Projection_Model
    pm = Projection_Model(max_iter=3)
    with pytest.raises(RuntimeError, match="largest relative residual"):
        pm.embed(cfg1_complex())
    assert pm.basis is None and pm.dim is None
    with pytest.raises(RuntimeError, match="embed"):
        pm.predict(cfg1_data()["fwd"][:, :2], [0, 1])


def test_two_target_draws():
    cx, d, fx = cfg1(), cfg1_data(), fixture()
    pm = model(None, sc=cfg1_complex())
    y, deg = np.eye(13)[d["target"]], cx.deg[d["last"]]
    acc, slots = pm.test_2_target(d["fwd"], d["last"], y, deg, seed=4)
    assert slots.shape == (1000,) and (slots >= 0).all() and (slots < deg).all() and (slots != d["target"]).all()
    score = np.empty(1000)
    for i in range(1000):
        lo, hi = fx["tt_ptr"][i], fx["tt_ptr"][i + 1]
        score[i] = fx["tt_score"][lo:hi][list(fx["tt_other"][lo:hi]).index(slots[i])]
    assert acc == float(score.sum()) / 1000
    assert np.array_equal(score, two_target_score(fx["probs_fwd"], d["target"], slots))
    acc2, slots2 = pm.test_2_target(d["fwd"], d["last"], y, deg, seed=4)
    assert acc2 == acc and np.array_equal(slots, slots2)
    _, slots3 = pm.test_2_target(d["fwd"], d["last"], y, deg, seed=5)
    assert not np.array_equal(slots, slots3)
    assert len(set(slots[deg == deg.max()].tolist())) > 2       # the draw moves over the neighbourhood
    from tests.test_host_projection import Cx
    path = Cx(3, [(0, 1), (1, 2)], [])
    pm = model(path)
    assert pm.dim == 0
    flows = np.stack([path.flow([0, 1]), path.flow([2, 1, 0])], axis=1)
    assert pm.test_2_target(flows[:, :1], [1], np.eye(2)[[1]], [2])[0] == 0.5
    with pytest.raises(ValueError, match="no second neighbour"):
        pm.test_2_target(flows, [1, 0], np.eye(2)[[1, 0]], [2, 1])


# ------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------

def write_cfg1_dataset(suffix):
    """The fixture's data set in the reference's folder format (1-hop and 2-hop, forward and reversed)."""
    cx = cfg1()
    c, q = np.load(os.path.join(GOLDEN, "cfg1_complex.npz")), np.load(os.path.join(GOLDEN, "cfg1_paths.npz"))

    def flows(name):
        ptr, X = q[name + "_ptr"], np.zeros((1000, cx.E, 1))
        X[np.repeat(np.arange(1000), np.diff(ptr)), q[name + "_idx"], 0] = q[name + "_val"]
        return X
    for h in ("1", "2"):
        fol = "trajectory_data_%shop_%s" % (h, suffix)
        os.makedirs(fol)
        for pre in ("", "rev_"):
            np.save(os.path.join(fol, pre + "flows_in.npy"), flows(pre + "flow" + h))
            np.save(os.path.join(fol, pre + "targets.npy"), np.eye(13)[q[pre + "targets" + h]][:, :, None])
            np.save(os.path.join(fol, pre + "last_nodes.npy"), q[pre + "last" + h].astype(np.int64))
            np.save(os.path.join(fol, pre + "target_nodes.npy"), q[pre + "tnode" + h].astype(np.int64))
        np.save(os.path.join(fol, "B1.npy"), cx.B1)
        np.save(os.path.join(fol, "B2.npy"), cx.B2)
        np.save(os.path.join(fol, "coords.npy"), c["coords"])
        np.save(os.path.join(fol, "train_mask.npy"), q["train_mask"].astype(np.int64))
        np.save(os.path.join(fol, "test_mask.npy"), q["test_mask"].astype(np.int64))


@pytest.mark.parametrize("flip", (0, 1))
def test_train_model_projection_switch(tmp_path, monkeypatch, capsys, flip):
    from scone_gcn_amd import scone_trajectory_model as stm, trajectory_experiments as te
    monkeypatch.chdir(tmp_path)
    write_cfg1_dataset("pm")
    hp = te.hyperparams(["prog", "-epochs", "2", "-batch_size", "100", "-data_folder_suffix", "pm", "-describe", "0", "-projection", "1",
                         "-flip_edges", str(flip)])
    hp["hidden_layers"] = [(3, 16)] * 3
    stm.reseed(1030)
    net, res = te.train_model(hp)
    assert len(res) == 4 and np.isfinite(res[0])               # training still runs afterwards
    got, fx = net.experiment_results["projection"], fixture()
    for key, want in (("standard", fx["test"]), ("reverse", fx["rev_test"]), ("transfer", fx["transfer"])):
        assert abs(got[key][0] - want[0]) <= TOL and got[key][1] == want[1]
    assert got["dim"] == 2 and 0.0 <= got["two_target"] <= 1.0 and len(got["two_target_slots"]) == 200
    out = capsys.readouterr().out
    labels = ["Standard experiment loss / acc:", "Reverse experiment loss / acc:", "2-target acc:", "Transfer experiment loss / acc:"]
    assert [l[:len(m)] for l in out.splitlines() for m in labels if l.startswith(m)] == labels
    assert "markov" not in net.experiment_results
    net._drop_graphs()
