"""Field-of-view multi-hop prediction on the MI355X (csrc/scn_field.hip; Scone_GCN(multi_hop_skip="field")): scn_field_lists through
the C-ABI against the numpy restatement of tests/test_host_field.py, integer-exact into junk-filled buffers; scn_tree_slabs_list
against scn_tree_slabs on the listed items, bitwise, with the junk intact everywhere else; then end to end, "field" against "dense"
on one net: per-level log-probabilities, predictions, pooled buffers, and the models that fall back.  A root whose dense candidates
come within 1e-5 of a tie at some level is left out of the comparison of paths; at most one of the 11 may be
(tests/test_host_field_seeds.py: on the fp64 oracle these seeds leave no root that close to a tie)."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_host_field import np_field_lists, random_tables

pytestmark = pytest.mark.gpu

JUNK = -7
N_ROOTS = 11                                             # the last slab of four trajectories is partial
N_POINTS = 20000                                         # |E| = 53 801.  At 6000 points (|E| = 16 020, some 266 blocks) the input level of
                                                         # three layers lists 0.72 of the items, at 12 000 0.43, here about 0.23


# ------------------------------------------------------------------------------------------------------------------
# scn_field_lists through the C-ABI
# ------------------------------------------------------------------------------------------------------------------

def run_field_lists(n, ns, node, n_nodes, top, adj, nb, n_levels, cap):
    """One call with every output buffer (and the workspace) pre-filled with junk: whatever differs was written by the library."""
    from scone_gcn_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.append(np.asarray(a, np.int32), 0), np.int32)).to(dev)
    p = lambda x: ops._dev(x, torch.int32)
    junk = lambda *shape: torch.full(shape, JUNK, device=dev, dtype=torch.int32)
    block, ptr, slab, counts = junk(n_levels, nb), junk(n_levels, nb + 1), junk(n_levels, max(cap, 1)), junk(n_levels, 2)
    n_slabs = max(1, -(-n // ns))
    nbytes = int(lib.scn_field_lists_workspace(nb, n_slabs, n_levels))
    assert nbytes > 0
    ws = torch.full((nbytes,), 0x5a, device=dev, dtype=torch.uint8)
    ins = [t(node), t(top[0]), t(top[1]), t(adj[0]), t(adj[1])]
    st = lib.scn_field_lists(n, ns, p(ins[0]), n_nodes, p(ins[1]), p(ins[2]), nb, p(ins[3]), p(ins[4]), n_levels, p(block), p(ptr),
                             p(slab), cap, p(counts), ctypes.c_void_p(ws.data_ptr()), nbytes, ops._stream())
    assert st == 0
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (block, ptr, slab, counts)]


def same_lists(got, want, cap):
    block, ptr, slab, counts = got
    for l, lv in enumerate(want):
        nw, items = lv["counts"]
        assert tuple(counts[l]) == (nw, items), (l, counts[l], lv["counts"])
        if "block" not in lv:                                                # empty or over cap: the counts and nothing else
            nw = items = 0
            assert ptr[l, 0] == JUNK
        else:
            assert np.array_equal(block[l, :nw], lv["block"]) and np.array_equal(ptr[l, :nw + 1], lv["ptr"]), l
            assert np.array_equal(slab[l, :items], lv["slab"]), l
            assert np.all(ptr[l, nw + 1:] == JUNK)
        assert np.all(block[l, nw:] == JUNK) and np.all(slab[l, items:] == JUNK), l


def _case(name):
    """(n, ns, node, n_nodes, top, adj, n_blocks, n_levels)"""
    rs = np.random.RandomState(sum(map(ord, name)))
    nb = {"one_block": 1, "blocks_65": 65, "blocks_257": 257, "slabs_130": 65, "slabs_130_blocks_257": 257}.get(name, 23)
    n_levels = {"levels_2": 2, "levels_7": 7}.get(name, 4)
    n_nodes = 9
    top, adj = random_tables(rs, n_nodes, nb, top_max=min(4, nb), adj_max=2)
    n = 4 * 130 if name.startswith("slabs_130") else (5 if name in ("one_block", "blocks_65", "blocks_257", "partial_slab") else 14)
    node = rs.randint(0, n_nodes, size=n)
    node[0] = 0                                                              # (T(0) holds the last block: random_tables)
    if name == "one_node":
        node[:] = 4
    if name == "all_dead":
        node[:] = -1
    if name == "mixed_slab":
        node[[0, 2, 3, 5, 9]] = -1                                           # slab 0 keeps one live leaf, slab 1 three, slab 2 three
        node[12] = n_nodes                                                   # a caller's error: guarded, contributes nothing
    if name.startswith("slabs_130"):
        node[rs.rand(n) < 0.7] = -1                                          # most slabs partly dead, some wholly
    return n, 4, node, n_nodes, top, adj, nb, n_levels


CASES = ["one_block", "blocks_65", "blocks_257", "partial_slab", "slabs_130", "slabs_130_blocks_257", "one_node", "all_dead",
         "mixed_slab", "levels_2", "levels_7"]


@pytest.mark.parametrize("name", CASES)
def test_field_lists_match_numpy(name):
    n, ns, node, n_nodes, top, adj, nb, n_levels = args = _case(name)
    cap = nb * max(1, -(-n // ns))
    want = np_field_lists(*args, cap)
    got = run_field_lists(*args, cap)
    same_lists(got, want, cap)
    if name == "all_dead":
        assert all(lv == {"counts": (0, 0)} for lv in want)
    else:
        assert want[-1]["counts"][0] > 0 and want[0]["counts"][1] >= want[-1]["counts"][1]
    if name in ("blocks_65", "blocks_257"):
        assert all(lv["block"][-1] == nb - 1 for lv in want)                  # the last block, past one wave / one workgroup of the scan
    again = run_field_lists(*args, cap)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("name", ["mixed_slab", "slabs_130_blocks_257"])
def test_a_level_over_cap_writes_its_counts_only(name):
    args = _case(name)
    full = np_field_lists(*args, 10 ** 9)
    cap = full[1]["counts"][1] - 1                                           # one short of level 1: levels 0 and 1 do not fit, the rest do
    want = np_field_lists(*args, cap)
    assert "block" not in want[0] and "block" not in want[1] and all("block" in lv for lv in want[2:])
    assert [lv["counts"] for lv in want] == [lv["counts"] for lv in full]
    same_lists(run_field_lists(*args, cap), want, cap)


def test_field_lists_refuse_bad_arguments():
    from scone_gcn_amd import _lib
    lib = _lib.load()
    assert lib.scn_field_lists(4, 4, None, 1, None, None, 1, None, None, 2, None, None, None, 0, None, None, 0, None) == _lib.SCN_ERR_BAD_ARG
    assert lib.scn_field_lists_workspace(1 << 20, 1 << 10, 4) == 0


# ------------------------------------------------------------------------------------------------------------------
# end to end: one complex, its plans and nets, shared and unchanged
# ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def world():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from scone_gcn_amd import synthetic_data_gen as g
    from scone_gcn_amd.complex import SimplicialComplex
    cx = g.random_SC_graph(N_POINTS)
    sc = SimplicialComplex(cx)
    paths = g.generate_random_walks(cx, m=N_ROOTS, seed=3)
    flows, choice, last, _, _ = g.path_dataset(cx, paths, seed=2)
    E_lookup = {(int(a), int(b)): k for k, (a, b) in enumerate(cx.edges.tolist())}
    return {"cx": cx, "sc": sc, "flows": flows, "last": np.asarray(last), "E_lookup": E_lookup, "nets": {}}


def _net(world, model, hidden, power=False):
    """(net, inputs) of one model type and width; the same net serves "dense" and "field" (the attribute is switched)."""
    key = (model, hidden, power)
    if key in world["nets"]:
        return world["nets"][key]
    from oracle import scone_oracle as so
    from scone_gcn_amd import ops, scone_trajectory_model as stm, trajectory_experiments as te
    sc, flows, last = world["sc"], world["flows"], world["last"]
    shifts, readout, _ = te.setup_from_complex(sc, model)
    inputs = [readout, last, flows]
    if power:
        # the composed Ebli plan is what a complex with a row of L1^2 beyond 128 sources gets; this one has none, so the plan cache
        # is seeded with it (get_scone_plan's key)
        dev = ops.default_device()
        plan = ops.PowerPlan(shifts[0], shifts[1], readout, te.MODEL_ACT[model], dev)
        assert plan.op.plan_info()[0] > 0
        shifts[0]._cache[("scone", id(shifts[1]), id(readout), te.MODEL_ACT[model], str(dev))] = plan
    stm.reseed(1030)
    net = stm.Scone_GCN(1, 1e-3, N_ROOTS, 0.0, verbose=False)
    layers = [(7 if model == "bunch" else 3, hidden)] * 3
    y = so.onehot_targets(np.zeros(N_ROOTS, int), sc.max_degree)
    net.setup(te.MODEL_FUNCS[model], layers, shifts, inputs, y, None, np.ones(N_ROOTS, int), model_type=model)
    for w in net.weights:                                   # larger weights than 0.01 randn: log-probabilities well apart
        w.mul_(20.0 if model == "scone" else 3.0)
    world["nets"][key] = (net, inputs)
    return net, inputs


def _run(net, mode, fn):
    """fn(net) under multi_hop_skip = mode: (result, trace, active fractions)."""
    net.multi_hop_skip = mode
    net._multi_hop_trace, net._multi_hop_fractions = trace, fr = [], []
    try:
        out = fn(net)
    finally:
        del net._multi_hop_trace, net._multi_hop_fractions
        net.multi_hop_skip = "dense"
    return out, trace, fr


def _pools_are_zero(net, inputs):
    plan = net._plan(inputs)
    n = 0
    for pool in plan._zero_pool.values():
        for t in pool:
            assert float(t.abs().max()) == 0.0
            n += 1
    return n


def _close(field, dense, tol=1e-6):
    """|field - dense| <= tol * max(1, |dense|), the bound listed-vs-dense execution is held to; printed before it is asserted."""
    f, d = np.asarray(field, np.float64), np.asarray(dense, np.float64)
    ok = np.isfinite(d)
    assert np.array_equal(ok, np.isfinite(f))
    err = float((np.abs(f[ok] - d[ok]) / np.maximum(1.0, np.abs(d[ok]))).max()) if ok.any() else 0.0
    print("max |field - dense| / max(1, |dense|) = %.3e, bitwise equal: %s" % (err, np.array_equal(f[ok], d[ok])))
    assert err <= tol


def _active(fr, bound=0.5):
    worst = max(max([f["input"]] + list(f["fwd"])) for f in fr)
    print("field forwards: %d, largest active fraction %.3f" % (len(fr), worst))
    assert fr and worst < bound                             # not vacuous: every level leaves more than half of the items out
    return worst


def _gap_ok(scores, keep):
    """Whether the `keep` best of the candidate scores are separated from each other and from the next one by more than 1e-5."""
    s = np.sort(np.asarray(scores, np.float64)[np.isfinite(scores)])[::-1][:keep + 1]
    return len(s) < 2 or float(np.min(-np.diff(s))) > 1e-5


@pytest.mark.parametrize("hidden", [32, 16])
def test_greedy_paths_match_dense(world, hidden):
    net, inputs = _net(world, "scone", hidden)
    hops = 3
    (pd, td, _), (pf, tf, fr) = (_run(net, m, lambda n: n.predict_paths(inputs, hops)) for m in ("dense", "field"))
    _active(fr)
    assert len(td) == len(tf) == hops
    deg = (np.asarray(world["sc"].nbrhoods) >= 0).sum(axis=1)
    clear = np.ones(N_ROOTS, bool)
    for h in range(hops):
        flows_d, last_d, logp_d, _ = td[h]
        flows_f, last_f, logp_f, _ = tf[h]
        for i in range(N_ROOTS):
            clear[i] &= _gap_ok(logp_d[i, :deg[last_d[i]]], 1)
        same = clear & (last_d == last_f)
        _close(logp_f[same], logp_d[same])                   # (a root past a near-tie walks another path: its later levels differ)
    assert clear.sum() >= N_ROOTS - 1
    assert np.array_equal(pd[clear], pf[clear])
    assert _pools_are_zero(net, inputs) > 0


@pytest.mark.parametrize("hidden", [32, 16])
@pytest.mark.parametrize("beam", [4, 1])
def test_beam_matches_dense(world, hidden, beam):
    net, inputs = _net(world, "scone", hidden)
    hops = 3
    call = lambda n: n.predict_paths_beam(inputs, hops, beam)
    ((pd, sd), td, _), ((pf, sf), tf, fr) = (_run(net, m, call) for m in ("dense", "field"))
    _active(fr)
    clear = np.ones(N_ROOTS, bool)
    deg = (np.asarray(world["sc"].nbrhoods) >= 0).sum(axis=1)
    for h in range(hops):
        d, f = td[h], tf[h]
        W2 = d["parent"].shape[1]
        for i in range(N_ROOTS):
            cand = [d["score"][i, k] + d["logp"][i, k, j] for k in range(d["node"].shape[1]) if d["node"][i, k] >= 0
                    for j in range(deg[d["node"][i, k]])]
            clear[i] &= _gap_ok(np.float32(cand), W2)
        same = clear & np.all(d["node"] == f["node"], axis=1)
        live = d["node"][same] >= 0
        _close(f["logp"][same][live], d["logp"][same][live])
        assert np.array_equal(d["parent"][clear], f["parent"][clear]) and np.array_equal(d["slot"][clear], f["slot"][clear])
    assert clear.sum() >= N_ROOTS - 1
    assert np.array_equal(pd[clear], pf[clear])
    _close(sf[clear], sd[clear], tol=hops * 1e-6)
    assert _pools_are_zero(net, inputs) > 0


@pytest.mark.parametrize("hidden", [32, 16])
def test_target_probabilities_match_dense(world, hidden):
    net, inputs = _net(world, "scone", hidden)
    sc, last, hops = world["sc"], world["last"], 2
    nb = np.asarray(sc.nbrhoods)
    rs = np.random.RandomState(9)
    first = np.array([rs.choice(nb[v][nb[v] >= 0]) for v in last])
    targets = np.array([rs.choice(nb[u][nb[u] >= 0]) for u in first])
    call = lambda n: n.multi_hop_target_probs(inputs, targets, sc.nbrhoods, world["E_lookup"], last, hops)
    (tp_d, _, _), (tp_f, _, fr) = (_run(net, m, call) for m in ("dense", "field"))
    _active(fr)
    assert np.all(np.isfinite(tp_d)) and np.all(tp_d > 0)
    err = float((np.abs(tp_f - tp_d) / np.abs(tp_d)).max())
    print("target probabilities: max relative difference %.3e" % err)
    assert err <= hops * 1e-6                              # the log-probability bound through a product of `hops` factors
    assert _pools_are_zero(net, inputs) > 0


@pytest.mark.parametrize("model", ["ebli", "bunch", "scone_hidden_8"])
def test_models_the_lists_do_not_serve_run_dense(world, model, monkeypatch):
    """The composed Ebli plan (PowerPlan), Bunch and a scone model of hidden width 8 (a blocked plan, but no *_list kernel of that
    width): "field" returns bitwise the "dense" result and no list entry point is called."""
    from scone_gcn_amd import ops
    if model == "scone_hidden_8":
        net, inputs = _net(world, "scone", 8)
        plan = net._plan(inputs)
        assert type(plan) is ops.SconePlan and plan.field_tables_dev() is not None
    else:
        net, inputs = _net(world, model, 32 if model == "ebli" else 8, power=model == "ebli")
        plan = net._plan(inputs)
        assert type(plan) is (ops.PowerPlan if model == "ebli" else ops.BunchPlan)
    assert ops.field_served(plan, net.weights) is None
    lib = ops._lib.load()
    calls = []
    for name in ("scn_field_lists", "scn_tree_slabs_list", "scn_clear_list"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _n=name, _f=fn: (calls.append(_n), _f(*a))[1], raising=False)
    sc, last = world["sc"], world["last"]
    nb = np.asarray(sc.nbrhoods)
    rs = np.random.RandomState(9)
    targets = np.array([rs.choice(nb[u][nb[u] >= 0]) for u in [rs.choice(nb[v][nb[v] >= 0]) for v in last]])
    for call in (lambda n: n.predict_paths(inputs, 2), lambda n: n.predict_paths_beam(inputs, 2, 3),
                 lambda n: n.multi_hop_target_probs(inputs, targets, sc.nbrhoods, world["E_lookup"], last, 2)):
        (d, td, _), (f, tf, fr) = (_run(net, m, call) for m in ("dense", "field"))
        assert not fr and not calls
        flat = lambda o: o if isinstance(o, tuple) else (o,)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(flat(d), flat(f)))
        for a, b in zip(td, tf):
            la, lb = (a["logp"], b["logp"]) if isinstance(a, dict) else (a[2], b[2])
            assert np.array_equal(la.view(np.int32), lb.view(np.int32))


def test_tables_follow_the_readout_and_a_probed_closure_gets_none(world):
    """sync_readout() re-uploading the readout drops the cached tables (the next call builds equal ones); a plan whose readout is a
    plain Bcond_func closure (ProbedBconds) serves no tables, so field_served and field_activity answer None and the caller runs dense."""
    from scone_gcn_amd import ops, trajectory_experiments as te
    net, inputs = _net(world, "scone", 32)
    plan = net._plan(inputs)
    tabs = plan.field_tables_dev()
    assert tabs is not None and plan._field is tabs and plan.field_tables_dev() is tabs
    plan._readout_version -= 1                               # (what a readout that has grown since the upload looks like)
    plan.sync_readout()
    assert plan._field is None
    again = plan.field_tables_dev()
    assert again is not tabs and again.n_blocks == tabs.n_blocks
    assert all(torch.equal(a, b) for a, b in zip(again[1:], tabs[1:]))
    sc, last = world["sc"], world["last"]
    closure = lambda v: inputs[0](v)                         # the rows of the Bconds object, behind a plain function
    shifts, _, _ = te.setup_from_complex(sc, "scone")
    shifts, readout = te.resolve_operands("scone", shifts, closure)
    probed = ops.get_scone_plan(shifts[0], shifts[1], readout, te.MODEL_ACT["scone"], plan.device)
    readout.prepare(last)
    probed.sync_readout()
    assert type(probed) is ops.SconePlan and probed._probed and probed.conv.plan_info()[0] > 0
    assert probed.field_tables_dev() is None and probed._field is None
    assert ops.field_served(probed, net.weights) is None
    node = torch.zeros((N_ROOTS,), device=plan.device, dtype=torch.int32)
    assert ops.field_activity(probed, node, N_ROOTS, 3) is None


# ------------------------------------------------------------------------------------------------------------------
# scn_tree_slabs_list against scn_tree_slabs, on the plan of the complex above
# ------------------------------------------------------------------------------------------------------------------

def test_tree_slabs_list_writes_the_listed_items_only(world):
    from scone_gcn_amd import _lib, ops
    lib = _lib.load()
    net, inputs = _net(world, "scone", 32)
    plan = net._plan(inputs)
    dev, E, NS = plan.device, plan.n_edges, ops.NS
    rs = np.random.RandomState(21)
    root_x, _ = ops.flows_to_slabs(world["flows"], plan.layout, dev)
    n, h = 10, 3                                            # three slabs, the last one partial
    S = ops.pad_count(n) // NS
    row0 = plan.conv.plan_blocks()
    nb = len(row0) - 1
    blk_of = np.searchsorted(row0, np.arange(E), side="right") - 1
    node = world["last"][rs.randint(0, N_ROOTS, size=n)].astype(np.int32)
    node[4] = -1                                            # a dead entry: lists nothing, its column is zero
    root = rs.randint(0, N_ROOTS, size=n).astype(np.int32)
    root[4] = -1
    act = ops.field_activity(plan, torch.from_numpy(node).to(dev), n, 3)
    wl = act["input"]
    assert 0 < wl.items < 0.5 * S * nb
    blocks = wl.block[:wl.n_work].cpu().numpy()
    ptr = wl.ptr[:wl.n_work + 1].cpu().numpy()
    slabs = wl.slab[:wl.items].cpu().numpy()
    listed = np.zeros((S, nb), bool)
    for u, b in enumerate(blocks):
        listed[slabs[ptr[u]:ptr[u + 1]], b] = True
    # path entries: rows inside and outside the leaf's listed blocks, a repeated row (the last write wins), -1 and a row past the end
    path_row = np.zeros((n, h), np.int32)
    for l in range(n):
        inside = np.flatnonzero(listed[l // NS][blk_of])
        outside = np.flatnonzero(~listed[l // NS][blk_of])
        path_row[l] = [rs.choice(inside), rs.choice(outside), rs.choice(inside)]
    path_row[1, 2] = path_row[1, 0]
    path_row[2, 0], path_row[3, 2] = -1, E
    path_row[4] = -1                                        # (as scn_beam_step writes a dead entry)
    path_sign = rs.choice([-1.0, 1.0], size=(n, h)).astype(np.float32)
    path_sign[1, 2] = -path_sign[1, 0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_root, d_row, d_sign = t(root), t(path_row), t(path_sign)
    i32 = lambda x: ops._dev(x, torch.int32)
    junk = np.float32(-1234.5)
    x_dense = torch.full((S, E, NS, 1), float(junk), device=dev)
    x_list = torch.full((S, E, NS, 1), float(junk), device=dev)
    _lib.check(lib.scn_tree_slabs(n, S, h, i32(d_root), i32(d_row), ops._dev(d_sign), N_ROOTS, ops._dev(root_x), E, NS, ops._dev(x_dense),
                                  ops._stream()), "scn_tree_slabs")
    _lib.check(lib.scn_tree_slabs_list(plan.conv.handle, n, S, h, i32(d_root), i32(d_row), ops._dev(d_sign), N_ROOTS, ops._dev(root_x), E,
                                       NS, ops._dev(x_list), wl.ref(), ops._stream()), "scn_tree_slabs_list")
    torch.cuda.synchronize()
    a, b = x_dense.cpu().numpy()[..., 0], x_list.cpu().numpy()[..., 0]      # [S, E, NS]
    in_list = listed[:, blk_of]                                              # [S, E]
    assert np.array_equal(a[in_list].view(np.int32), b[in_list].view(np.int32))
    assert np.all(b[~in_list] == junk) and not np.any(a == junk)
    # the entry outside the list was set by the dense call and left alone by the listed one; the repeated row holds the last value
    assert a[0, path_row[0, 1], 0] == path_sign[0, 1] and b[0, path_row[0, 1], 0] == junk
    assert b[0, path_row[1, 0], 1] == path_sign[1, 2]
    assert np.all(b[1, in_list[1], 0] == 0.0)                                # the dead leaf's column (leaf 4 = slab 1, column 0)
    # an empty list writes nothing at all
    dead = ops.field_activity(plan, torch.full((n,), -1, device=dev, dtype=torch.int32), n, 3)
    assert dead["input"].n_work == 0 and all(w.items == 0 for w in dead["fwd"])
    x_none = torch.full((S, E, NS, 1), float(junk), device=dev)
    _lib.check(lib.scn_tree_slabs_list(plan.conv.handle, n, S, h, i32(d_root), i32(d_row), ops._dev(d_sign), N_ROOTS, ops._dev(root_x), E,
                                       NS, ops._dev(x_none), dead["input"].ref(), ops._stream()), "scn_tree_slabs_list")
    assert bool((x_none == float(junk)).all())


@pytest.mark.parametrize("hidden", [32, 16])
def test_listed_forward_reads_nothing_outside_the_lists(world, hidden):
    """The closure property on the device: x is NaN everywhere, scn_tree_slabs_list fills the items of list_0, and the listed
    forward gives finite log-probabilities within the listed-vs-dense bound of the dense forward on the full input; the pooled
    buffers go back all-zero (a NaN that reached an unlisted item would stay there)."""
    from scone_gcn_amd import _lib, ops
    lib = _lib.load()
    net, inputs = _net(world, "scone", hidden)
    plan = net._plan(inputs)
    dev, E, NS = plan.device, plan.n_edges, ops.NS
    rs = np.random.RandomState(33)
    root_x, _ = ops.flows_to_slabs(world["flows"], plan.layout, dev)
    n, h = 10, 2                                            # three slabs, the last one partial
    S = ops.pad_count(n) // NS
    node = world["last"][rs.randint(0, N_ROOTS, size=n)].astype(np.int32)
    root = rs.randint(0, N_ROOTS, size=n).astype(np.int32)
    node[4] = root[4] = -1                                  # a dead entry
    path_row = rs.randint(0, E, size=(n, h)).astype(np.int32)
    path_row[4] = -1
    path_sign = rs.choice([-1.0, 1.0], size=(n, h)).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_node, d_root, d_row, d_sign = t(node), t(root), t(path_row), t(path_sign)
    i32 = lambda x: ops._dev(x, torch.int32)
    act = ops.field_activity(plan, d_node, n, 3)
    worst = max([act["active_fraction"]["input"]] + act["active_fraction"]["fwd"])
    assert 0 < worst < 0.5
    x_dense = torch.full((S, E, NS, 1), float("nan"), device=dev)
    x_list = torch.full((S, E, NS, 1), float("nan"), device=dev)
    _lib.check(lib.scn_tree_slabs(n, S, h, i32(d_root), i32(d_row), ops._dev(d_sign), N_ROOTS, ops._dev(root_x), E, NS, ops._dev(x_dense),
                                  ops._stream()), "scn_tree_slabs")
    _lib.check(lib.scn_tree_slabs_list(plan.conv.handle, n, S, h, i32(d_root), i32(d_row), ops._dev(d_sign), N_ROOTS, ops._dev(root_x), E,
                                       NS, ops._dev(x_list), act["input"].ref(), ops._stream()), "scn_tree_slabs_list")
    assert not bool(torch.isnan(x_dense).any()) and bool(torch.isnan(x_list).any())
    last = torch.zeros((S * NS,), device=dev, dtype=torch.int32)
    last[:n] = d_node.clamp(min=0)
    logp_d = ops.forward_logp(plan, x_dense, last, net.weights)[:n].cpu().numpy()
    logp_f = ops.forward_logp(plan, x_list, last, net.weights, act)[:n].cpu().numpy()
    live = node >= 0
    deg = (np.asarray(world["sc"].nbrhoods) >= 0).sum(axis=1)
    for i in np.flatnonzero(live):
        assert np.all(np.isfinite(logp_f[i, :deg[node[i]]])), i
    assert not np.isnan(logp_f[live]).any()
    _close(logp_f[live], logp_d[live])
    assert _pools_are_zero(net, inputs) > 0
