"""Host tests of the cases tests/test_gpu_small_step_limits.py runs the one-launch step on (tests/small_step_cases.py builds them):
every case is proved ON THE CPU to be the case it claims to be, and to be able to see an error.

1. The kernel's host-side selection (small_waves / small_lds / small_blocks / the instance choice of csrc/scn_small.hip) is restated in
   Python (small_step_cases.restate_form) and the regime of every row of the case table is asserted from it: waves, tiles per wave,
   instance (unpaired and paired), whether the overflow list and the first layer's shifted input have room in the LDS, whether the
   instance reads the list there.  The GPU test compares the restatement with the library's own answer (scn_small_step_layout).
2. The operators have the rows they claim: exact lengths at the special device rows, an entry in column 0 and column |E| - 1, entries
   of one value array only, per class; nothing else longer than 11; symmetric / not; the graphs meet max_deg and max_items exactly.
3. Sensitivity: with ONE entry zeroed in the reference operator only -- the 12th of a row of twelve, the 13th of a row of thirteen, the
   last of each longer class, the only entry of a row of one, a column-0 entry, an entry of the last row -- the fp64 oracle's
   gradients move by at least ten times the comparison bar in some weight tensor.
4. Conditioning: oracle/torch_dense.py in float32 (autograd) agrees with the fp64 oracle within a quarter of the bar, so float32
   arithmetic itself is four times better than what the kernel is held to (and tanh is out of saturation); every reference gradient
   tensor has an entry of at least 0.1, so the bars, relative to max(1, .), are relative in effect.
5. The oracle's hand-written non-symmetric backward against torch autograd in float64 on a nonsym case.
"""
import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")
torch = pytest.importorskip("torch")

from tests import small_step_cases as sc

TOL = 1e-5                      # tests/test_gpu_small_step.py: loss and every weight-gradient tensor against fp64


def _maxdiff(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(b))))


def test_restated_selection_by_hand():
    """The numbers the case table rests on: 132 epad + 15744 bytes for eight waves, support up to epad = 1120, y in LDS up to
    epad = 1056 with an empty list, 1253 list entries of room at |E| = 1001; instance and pairing boundaries."""
    f = lambda E, n=0, p=False: sc.restate_form(E, n, n, p, True)
    assert f(1120)["supported"] == 1 and f(1120)["lds_bytes"] == 132 * 1120 + 15744 and f(1121)["supported"] == 0
    assert f(1056)["y_lds"] == 1 and f(1057)["y_lds"] == 0 and f(1056, 22)["y_lds"] == 0 and f(1056, 21)["y_lds"] == 1
    assert f(1001, 1253)["ovf_lds"] == 1 and f(1001, 1254)["ovf_lds"] == 0 and f(1001, 581)["y_lds"] == 1 and f(1001, 582)["y_lds"] == 0
    assert [f(E)["waves"] for E in (1, 384, 385)] == [12, 12, 8]
    assert [f(E)["instance"] for E in (16, 192, 193, 384, 385, 768, 769, 1024, 1025, 1120)] == [1, 1, 2, 2, 6, 6, 8, 8, 9, 9]
    assert [f(E, 0, True)["instance"] for E in (385, 512, 513, 768, 769, 1024, 1025, 1120)] == [2, 2, 3, 3, 4, 4, 5, 5]
    assert f(384, 0, True)["paired"] == 0 and f(385, 0, True)["paired"] == 1
    assert all(f(E)["tiles_per_wave"] >= 4 for E in range(385, 1121)), "eight waves never run three tiles per wave: no instance <3, 8>"
    assert f(1025, 300)["ovf_lds"] == 1 and f(1025, 300)["ovf_in_kernel"] == 0 and f(1025, 300, True)["ovf_in_kernel"] == 1
    assert f(193, 300)["ovf_lds"] == 0


def test_case_table_rotates_layers_and_activations():
    for L in (2, 5, 6):
        hits = [c for c in sc.CASES if c[5] == L]
        assert len(hits) >= 2 and any(c[3] == "nonsym" for c in hits), L
    for act in sc.ACTS:
        hits = [c for c in sc.CASES if c[6] == act]
        assert len(hits) >= 2 and any(c[3] == "nonsym" for c in hits), act
    assert all(c[5] == 6 for c in sc.CASES if c[1] == 520)
    assert sorted(sc.REGIMES) == sorted(sc.CASE_NAMES)


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_case_is_in_the_regime_it_claims(name):
    c = sc.get_case(name)
    one, two = c.form(False), c.form(True)
    for k, v in sc.REGIMES[name].items():
        got = two["instance"] if k == "paired_instance" else one.get(k)
        assert got == v, (name, k, got, v)
    assert 9 <= c.n_traj <= 13 and c.n_traj % 4 != 0, "the last slab of four is partly padding"
    if one["supported"]:
        assert two["paired"] == int(c.E > 384)
        if two["paired"]:
            assert two["ovf_in_kernel"] == two["ovf_lds"] and two["lds_bytes"] == one["lds_bytes"]
    if name == "e385_sym":
        assert one["tiles"] == 25 and one["blocks"] == 4 and c.E - 3 * 128 == 1, "the fourth block is one row"
    if name == "e17_sym":
        assert one["tiles"] == 2 and c.E % 16 == 1
    if name == "e1040_sym":
        assert sc.restate_form(c.E, 0, 0, False, True)["y_lds"] == 1, "without the list y would have had room"
    if name == "e1001_nonsym_long":
        assert max(c.n_ovf, c.n_ovf_t) > 1253 and min(c.n_ovf, c.n_ovf_t) > 0
    if c.variant == "nonsym":
        assert 0 < c.n_ovf_t != c.n_ovf > 0


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_graph_and_operator_are_what_they_claim(name):
    c = sc.get_case(name)
    E = c.E
    # the graph: no faces, a node without edges, the readout bounds
    deg = np.bincount(c.cx.edges.ravel(), minlength=c.cx.n_nodes)
    assert c.cx.n_faces == 0 and c.cx.n_edges == E and deg[c.roles["isolated"]] == 0 and (np.asarray(c.sc.nbrhoods)[c.roles["isolated"]] < 0).all()
    if c.graph == "hub":
        assert (c.max_deg, c.max_items) == (64, 512) and deg[0] == 64 and sorted(set(deg[1:65])) == [8] and deg[65:].max() <= 3
    elif c.graph == "hub24":
        assert (c.max_deg, c.max_items) == (24, 216) and deg[0] == 24 and sorted(set(deg[1:25])) == [9] and deg[25:].max() <= 3
        assert deg[c.roles["nbr"]] > 6, "a neighbour with more incident edges than the kernel requests at its start (SM_RO_PRE)"
    else:
        assert c.max_deg == 3 and deg.max() == 3
    assert [c.last_nodes[k] for k in (c.T_HUB, c.T_NBR, c.T_LEAF, c.T_ISOLATED)] == [c.roles[r] for r in ("hub", "nbr", "leaf", "isolated")]
    assert not c.y[c.T_ZERO_Y].any() and not c.flows[c.T_ZERO_FLOW].any()
    assert all(c.y[n].sum() == 1 for n in range(c.n_traj) if n != c.T_ZERO_Y) and np.abs(c.flows).min(axis=1).max() > 0
    # the operator in device order: the special rows' exact lengths, every other row at most 11
    lo, up = (c.dev_lo, c.dev_up) if c.variant != "tonly" else (c.dev_lo.T.tocsr(), c.dev_up.T.tocsr())
    pat = (abs(lo) + abs(up)).tocsr()
    pat.sort_indices()
    n = np.diff(pat.indptr)
    for r in sc.special_rows(E):
        assert r in c.targets
    for r, t in c.targets.items():
        assert n[r] == t, (r, t, n[r])
    rest = np.setdiff1d(np.arange(E), list(c.targets))
    assert n[rest].max() <= sc.ORDINARY_MAX and n[rest].min() >= 0
    classes = [k for k in sc.CLASSES if k <= E - 4]
    assert {c.targets[r] for r in c.targets} >= set(classes) and (E < 200 or set(classes) == set(sc.CLASSES))
    for k in classes:
        rows = [r for r in c.targets if c.targets[r] == k]
        cols = [pat.indices[pat.indptr[r]:pat.indptr[r + 1]] for r in rows]
        if k >= 1:
            assert any(0 in cc for cc in cols), "class %d: no entry in column 0" % k
        if k >= 2 or (k == 1 and len(rows) > 1):
            assert any(E - 1 in cc for cc in cols), "class %d: no entry in the last column" % k
        if k >= 2:
            only_lo = only_up = False
            for r in rows:
                a, b = lo[r].toarray().ravel(), up[r].toarray().ravel()
                only_lo |= bool(((a != 0) & (b == 0)).any())
                only_up |= bool(((a == 0) & (b != 0)).any())
            assert only_lo and only_up, "class %d: no entry of one value array only" % k
    sym = abs(c.dev_lo - c.dev_lo.T).nnz == 0 and abs(c.dev_up - c.dev_up.T).nnz == 0
    assert sym == (c.variant == "sym")
    if c.variant == "tonly":
        assert c.n_ovf == 0 < c.n_ovf_t and sc.row_lengths(c.dev_lo, c.dev_up).max() <= sc.ORDINARY_MAX
    # the caller-order matrices are the device ones under the layout
    perm = c.sc.layout.perm[1]
    coo = c.S_lo.tocoo()
    back = sp.csr_matrix((coo.data, (perm[coo.row], perm[coo.col])), shape=(E, E))
    assert abs(back - c.dev_lo.astype(np.float64)).nnz == 0
    assert c.S_lo.dtype == np.float64 and np.array_equal(c.S_lo.data, c.S_lo.data.astype(np.float32).astype(np.float64))


def _probes(c):
    """[(what, device row, device column)]: the entries whose loss a case has to see."""
    lo, up = (c.dev_lo, c.dev_up) if c.variant != "tonly" else (c.dev_lo.T.tocsr(), c.dev_up.T.tocsr())
    pat = (abs(lo) + abs(up)).tocsr()
    pat.sort_indices()
    row = lambda r: pat.indices[pat.indptr[r]:pat.indptr[r + 1]]
    out = []
    for k, r in sorted(c.reps.items()):
        if k == 0:
            continue
        out.append(("entry %d of a row of %d" % (k, k), r, int(row(r)[k - 1])))
        if k in (12, 13) and 0 in row(r) and not any(w.startswith("column 0") for w, _, _ in out):
            out.append(("column 0 of a row of %d" % k, r, 0))
    last = row(c.E - 1)
    out.append(("first entry of the last row", c.E - 1, int(last[0])))
    out.append(("last entry of the last row", c.E - 1, int(last[-1])))
    if c.variant == "tonly":
        out = [(w, col, r) for w, r, col in out]              # the rows are A^T's: entry (r, c) of A^T is (c, r) of A
    return out


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_every_special_entry_moves_the_reference(name):
    c = sc.get_case(name)
    loss, ref = sc.reference(name)
    order = c.sc.layout.order[1]
    probes = _probes(c)
    assert len(probes) >= 6
    for what, r, col in probes:
        mats = []
        for m in (c.S_lo, c.S_up):
            m = m.tolil(copy=True)
            m[order[r], order[col]] = 0.0
            mats.append(m.tocsr())
        assert abs(mats[0] - c.S_lo).nnz + abs(mats[1] - c.S_up).nnz >= 1, what
        _, g = c.oracle(mats[0], mats[1])
        moved = max(_maxdiff(a, b) for a, b in zip(g, ref))
        print("%s: %s moves the gradients by %.3g (needs %.1e)" % (name, what, moved, 10 * TOL))
        assert moved >= 10 * TOL, (name, what, moved)


def _torch_dense(c, dtype):
    from oracle import torch_dense as td
    act = {"tanh": td.tanh, "relu": td.relu, "leaky_relu": td.leaky_relu, "none": lambda x: x}[c.act]
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    w = [t(a).requires_grad_(True) for a in c.weights]
    B1 = sc._b1_dense(c.cx)
    B1_ext = t(np.concatenate([B1, np.zeros((1, c.E))], axis=0))
    nbr = torch.tensor(np.asarray(c.sc.nbrhoods), dtype=torch.int64)
    preds = td.scone_func(w, t(c.S_lo.toarray()), t(c.S_up.toarray()), B1_ext, nbr, torch.tensor(c.last_nodes), t(c.flows), act=act)
    loss = td.loss_fn(preds, t(c.y), torch.ones(c.n_traj), w, 0.0)
    loss.backward()
    return float(loss.detach()), [a.grad.numpy().astype(np.float64) for a in w]


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_float32_resolves_the_case_four_times_better_than_the_bar(name):
    c = sc.get_case(name)
    ref_loss, ref = sc.reference(name)
    loss, g = _torch_dense(c, torch.float32)
    worst = max(_maxdiff(a, b) for a, b in zip(g, ref))
    small = min(float(np.abs(b).max()) for b in ref)
    print("%s: float32 autograd against fp64: loss %.3g, gradients %.3g (bar / 4 = %.2e); smallest tensor maximum %.3g"
          % (name, abs(loss - ref_loss) / max(1.0, abs(ref_loss)), worst, TOL / 4, small))
    assert abs(loss - ref_loss) <= TOL / 4 * max(1.0, abs(ref_loss))
    assert worst <= TOL / 4
    assert small >= 0.1, "a reference gradient tensor without an entry of 0.1: the bars would be absolute for it"


def test_oracle_nonsymmetric_backward_against_autograd_in_float64():
    c = sc.get_case("e193_nonsym")
    ref_loss, ref = sc.reference("e193_nonsym")
    loss, g = _torch_dense(c, torch.float64)
    assert abs(loss - ref_loss) <= 1e-12 * max(1.0, abs(ref_loss))
    for k, (a, b) in enumerate(zip(g, ref)):
        assert _maxdiff(a, b) <= 1e-11, k
    assert abs(c.S_lo - c.S_lo.T).nnz > 0 and abs(c.S_up - c.S_up.T).nnz > 0


def test_special_trajectories_contribute_log_d_and_no_gradient():
    """In the oracle: the trajectory on the node without edges and the one with an all-zero flow, alone."""
    c = sc.get_case("e520_nonsym")
    for n in (c.T_ISOLATED, c.T_ZERO_FLOW):
        loss, g = c.oracle(sel=[n])
        assert abs(loss - np.log(c.max_deg) / c.n_traj) <= 1e-14 and all(not a.any() for a in g)
