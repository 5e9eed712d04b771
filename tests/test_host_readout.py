"""The fp64 restatement of the readout at the C-ABI's own layout (oracle/scone_oracle.py: slab_readout_*, slab_node_readout_*),
pinned without a GPU: against the oracle's readout_scone and the readout inside bunch_forward on config 1 (with and without
flips), its backward against central finite differences, and its dz support against the edges incident to the live
neighbours of each last node.  The complexes tests/test_gpu_readout.py launches on are built here, from edge lists."""
import numpy as np
import pytest

from oracle import scone_oracle as so

# ------------------------------------------------------------------------------------------------------------------
# complexes (edge lists; no faces) that reach every launch path of csrc/scn_readout.hip
# ------------------------------------------------------------------------------------------------------------------


def _complex(name, n_nodes, edges, last, S, ns, seed):
    """Edges in a shuffled order (edge ids are not sorted by node), a third of them flipped, and last_nodes for S x ns
    trajectories: the given ones, then padding trajectories ending at node 0 (as ops._last_nodes_dev pads)."""
    rs = np.random.RandomState(seed)
    edges = np.asarray(edges, np.int64)
    edges = edges[rs.permutation(len(edges))]
    flips = np.where(rs.rand(len(edges)) < 0.33, -1.0, 1.0)
    nbr, D = so.neighborhoods(edges, n_nodes)
    N = S * ns
    assert len(last) <= N
    ln = np.zeros(N, np.int32)
    ln[:len(last)] = last
    ptr, inc_edge, inc_sign, edge_nodes = so.incidence_csr(edges, n_nodes, flips)
    return {"name": name, "n_nodes": n_nodes, "edges": edges, "flips": flips, "nbr": nbr.astype(np.int32), "D": D,
            "S": S, "ns": ns, "n_real": len(last), "last": ln, "inc_ptr": ptr, "inc_edge": inc_edge, "inc_sign": inc_sign,
            "edge_nodes": edge_nodes}


def complex_mixed():
    """(a) fast and serial item lists in one launch, plus the degenerate cases.  Hub A joined to 40 nodes u_i, 12 satellites
    joined to every u_i, u_{2j} - u_{2j+1} joined (neighbours of A and of the satellites adjacent to each other): A, the
    satellites and the u_i have > 512 items (serial form).  Hub B with 48 leaves (max_deg 48: A and the satellites have 8
    padding slots), two leaf pairs joined: B and its leaves take the fast form.  One isolated node.  u_0 is node V - 1, so
    at A and at the satellites its real slot and the wrapped -1 slots of the node readout collide."""
    A, sat, B, leaf, iso = 0, list(range(1, 13)), 13, list(range(14, 62)), 62
    u = [102 - k for k in range(40)]                                                 # u_0 = 102 = V - 1
    e = [(A, x) for x in u] + [(s, x) for s in sat for x in u] + [(u[2 * j], u[2 * j + 1]) for j in range(10)]
    e += [(B, x) for x in leaf] + [(leaf[0], leaf[1]), (leaf[2], leaf[3])]
    last = [A, leaf[0], sat[0], B, u[0], iso, leaf[5], u[3], sat[7], leaf[2], u[30]]
    return _complex("mixed", 103, e, last, 4, 3, 1)                                   # 11 of 12: the last slab is padded


def complex_wide():
    """(b) a hub of degree 80 (the wide kernels), ten leaf pairs joined; leaf 80 = V - 1 is joined to leaf 79."""
    e = [(0, x) for x in range(1, 81)] + [(2 * j + 1, 2 * j + 2) for j in range(10)] + [(79, 80)]
    return _complex("wide", 81, e, [0, 79, 1, 0, 80, 5, 12, 0, 33, 3, 79, 60, 2, 0, 7, 21, 64, 70, 4, 0], 7, 3, 2)


def complex_star(n_leaves, pairs):
    e = [(0, x) for x in range(1, n_leaves + 1)] + [(2 * j + 1, 2 * j + 2) for j in range(pairs)]
    last = [0, 1, n_leaves, 0, 3, 2, 0, n_leaves - 1]
    return e, n_leaves + 1, last


def complex_deg64():
    e, V, last = complex_star(64, 6)
    return _complex("deg64", V, e, last, 2, 4, 3)


def complex_deg65():
    e, V, last = complex_star(65, 6)
    return _complex("deg65", V, e, last[:3], 3, 1, 4)


def complex_deg1024():
    e, V, last = complex_star(1024, 0)
    return _complex("deg1024", V, e, last[:6], 2, 3, 5)


def complex_items():
    """Item lists of exactly 512 and 513: X joined to 32 nodes w_j, each joined to 15 shared nodes z_k (X and every z_k:
    32 x 16 = 512 items); a second copy with one extra edge w'_0 - q (513: the serial form)."""
    e = []
    for off, extra in ((0, False), (48, True)):
        X, w, z = off, [off + 1 + j for j in range(32)], [off + 33 + k for k in range(15)]
        e += [(X, x) for x in w] + [(x, y) for x in w for y in z]
        if extra:
            e.append((w[0], off + 48))
    last = [0, 48, 33, 81, 0, 48, 1, 49]
    return _complex("items", 97, e, last, 4, 2, 6)


COMPLEXES = {"mixed": complex_mixed, "wide": complex_wide, "deg64": complex_deg64, "deg65": complex_deg65,
             "deg1024": complex_deg1024, "items": complex_items}


def items_of(cx):
    """Readout items (incident edges of the live neighbours) of each trajectory's last node."""
    deg = np.diff(cx["inc_ptr"])
    rows = cx["nbr"][cx["last"]]
    return np.where(rows >= 0, deg[np.maximum(rows, 0)], 0).sum(axis=1)


def slab(T, S, ns):
    """[N][R](...) -> [S][R][ns](...)."""
    T = np.asarray(T)
    return np.swapaxes(T.reshape((S, ns) + T.shape[1:]), 1, 2)


def random_H(rs, S, E, ns, C):
    """Activation outputs in (-1, 1) with exact zeros (the relu / leaky_relu derivative at 0)."""
    H = rs.uniform(-1, 1, (S, E, ns, C))
    H[rs.rand(*H.shape) < 0.1] = 0.0
    return H.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------
# the complexes reach the paths they are named for
# ------------------------------------------------------------------------------------------------------------------


def test_the_complexes_reach_every_launch_path():
    a = complex_mixed()
    it = items_of(a)[:a["n_real"]]
    assert a["D"] == 48 and (it > 512).any() and (it <= 512).any()
    assert it[list(a["last"]).index(62)] == 0                                         # the isolated node: all slots -1
    assert complex_wide()["D"] == 80 and complex_deg64()["D"] == 64 and complex_deg65()["D"] == 65
    assert complex_deg1024()["D"] == 1024
    assert sorted(set(items_of(complex_items()).tolist())) == [512, 513]
    # d_w_last: N x max_deg below 1024 and above it, neither a multiple of the 4 x row-group stride (256 rows at c <= 16)
    w = complex_wide()
    assert a["S"] * a["ns"] * a["D"] < 1024 < w["S"] * w["ns"] * w["D"]
    assert (a["S"] * a["ns"] * a["D"]) % 256 and (w["S"] * w["ns"] * w["D"]) % 256


# ------------------------------------------------------------------------------------------------------------------
# pinned against the oracle's own readouts on config 1
# ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("flipped", [False, True])
def test_slab_readout_matches_readout_scone_on_cfg1(cfg1, flipped):
    rs = np.random.RandomState(11)
    E, V = cfg1["E"], cfg1["n_nodes"]
    flips = np.where(rs.rand(E) < 0.3, -1.0, 1.0) if flipped else None
    ptr, edge, sign, edge_nodes = so.incidence_csr(cfg1["edges"], V, flips)
    B1 = cfg1["B1"] if flips is None else cfg1["B1"] * flips
    assert np.array_equal(so.b1_from_csr(ptr, edge, sign, E), B1)
    assert np.array_equal(edge_nodes, cfg1["edges"])
    nb, D = so.neighborhoods(cfg1["edges"], V)
    S, ns, C = 5, 4, 6
    N = S * ns
    last = cfg1["last_nodes"][:N]
    Hn = rs.randn(N, E, C)
    W = rs.randn(C, 1)
    ref, Bc, logits = so.readout_scone(Hn, W, so.make_Bconds(cfg1["B1"], nb, None if flips is None else np.diag(flips)), last)
    out = so.slab_readout_forward(slab(Hn, S, ns), W[:, 0], nb, last, ptr, edge, sign)
    assert np.abs(out["logits"] - logits[:, :, 0]).max() <= 1e-12
    assert np.abs(out["logp"] - ref[:, :, 0]).max() <= 1e-12
    assert np.abs(out["bh"] - np.einsum("nde,nec->ndc", Bc, Hn)).max() <= 1e-12


def test_slab_node_readout_matches_bunch_forward_on_cfg1(cfg1):
    rs = np.random.RandomState(12)
    shifts = so.bunch_shifts(cfg1["B1"], cfg1["B2"])
    w = [0.3 * rs.randn(*s) for s in so.weight_shapes(1, [(7, 4)] * 2, 1, "bunch")]
    S, ns = 3, 4
    sel = np.arange(S * ns)
    last = cfg1["last_nodes"][sel]
    nb, _ = so.neighborhoods(cfg1["edges"], cfg1["n_nodes"])
    ref = so.bunch_forward(w, shifts, nb, last, cfg1["flows"][sel])
    nodes_out = so.bunch_conv_forward(w, shifts, cfg1["flows"][sel])[0][:, :, 0]     # (N, V)
    out = so.slab_node_readout_forward(slab(nodes_out, S, ns), nb, last)
    assert np.abs(out["logp"] - ref[:, :, 0]).max() <= 1e-12
    assert (nb[last] < 0).any()                                                      # padding slots are exercised


# ------------------------------------------------------------------------------------------------------------------
# backward against central finite differences
# ------------------------------------------------------------------------------------------------------------------


def _fd(f, x, h=1e-6):
    g = np.zeros_like(x)
    for k in np.ndindex(x.shape):
        xp, xm = x.copy(), x.copy()
        xp[k] += h
        xm[k] -= h
        g[k] = (f(xp) - f(xm)) / (2 * h)
    return g


@pytest.mark.parametrize("act", [0, 1])
def test_slab_readout_backward_matches_finite_differences(act):
    """L = sum d_logp * logp.  dz is dL/dZ with H = act(Z) (act 0: H = Z, 1: H = tanh Z); d_w is dL/dw."""
    rs = np.random.RandomState(13)
    n_nodes = 7
    edges = [(0, 1), (0, 2), (0, 3), (1, 2), (2, 4), (3, 5), (4, 5)]                  # 1-2 and 3-... : neighbours joined
    cx = _complex("fd", n_nodes, edges, [0, 2, 6, 5, 1], 3, 2, 7)
    S, ns, C, E = cx["S"], cx["ns"], 3, len(edges)
    tab = (cx["nbr"], cx["last"], cx["inc_ptr"], cx["inc_edge"], cx["inc_sign"])
    Z = rs.randn(S, E, ns, C) * 0.7
    w = rs.randn(C)
    g = rs.randn(S * ns, cx["D"])
    f_act = (lambda z: z) if act == 0 else np.tanh

    def loss_z(z):
        return float(np.sum(g * so.slab_readout_forward(f_act(z), w, *tab)["logp"]))

    def loss_w(ww):
        return float(np.sum(g * so.slab_readout_forward(f_act(Z), ww, *tab)["logp"]))

    H = f_act(Z)
    fw = so.slab_readout_forward(H, w, *tab)
    bw = so.slab_readout_backward(H, w, *tab, fw["bh"], g, fw["logp"], act)
    assert np.abs(bw["dz"] - _fd(loss_z, Z)).max() <= 1e-7
    assert np.abs(bw["d_w"] - _fd(loss_w, w)).max() <= 1e-7
    # d_logits is the gradient w.r.t. the logits: L(logits) = sum g * log_softmax(logits)
    lg = fw["logits"]
    fd_l = _fd(lambda x: float(np.sum(g * (x - so.logsumexp(x, axis=1)))), lg)
    assert np.abs(bw["d_logits"] - fd_l).max() <= 1e-7


@pytest.mark.parametrize("act", [0, 1])
def test_slab_node_readout_backward_matches_finite_differences(act):
    rs = np.random.RandomState(14)
    n_nodes = 6
    edges = [(0, 5), (0, 1), (1, 2), (2, 5), (3, 4)]                                    # node 5 = V - 1 is a real neighbour of 0 and 2
    nbr, D = so.neighborhoods(edges, n_nodes)
    last = np.array([0, 2, 4, 1, 5, 3], np.int32)
    S, ns = 2, 3
    Z = rs.randn(S, n_nodes, ns)
    g = rs.randn(S * ns, D)
    f_act = (lambda z: z) if act == 0 else np.tanh
    lz = lambda z: float(np.sum(g * so.slab_node_readout_forward(f_act(z), nbr, last)["logp"]))
    X = f_act(Z)
    fw = so.slab_node_readout_forward(X, nbr, last)
    bw = so.slab_node_readout_backward(X, nbr, last, g, fw["logp"], act)
    assert np.abs(bw["dz"] - _fd(lz, Z)).max() <= 1e-7
    assert (nbr[last] < 0).any() and (nbr[last] == n_nodes - 1).any()


# ------------------------------------------------------------------------------------------------------------------
# the support the backward writes
# ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", sorted(COMPLEXES))
def test_support_is_the_edges_incident_to_the_live_neighbours(name):
    cx = COMPLEXES[name]()
    S, ns, E = cx["S"], cx["ns"], len(cx["edges"])
    rs = np.random.RandomState(15)
    C = 2
    H = random_H(rs, S, E, ns, C)
    w = rs.randn(C)
    tab = (cx["nbr"], cx["last"], cx["inc_ptr"], cx["inc_edge"], cx["inc_sign"])
    fw = so.slab_readout_forward(H, w, *tab)
    bw = so.slab_readout_backward(H, w, *tab, fw["bh"], rs.randn(S * ns, cx["D"]), fw["logp"], 0)
    for n in range(S * ns):
        s, i = divmod(n, ns)
        live = {int(v) for v in cx["nbr"][cx["last"][n]] if v >= 0}
        want = np.array([int(a) in live or int(b) in live for a, b in cx["edges"]])
        assert np.array_equal(bw["support"][s, :, i], want), (name, n)
        assert np.all(bw["dz"][s, ~want, i] == 0.0)
