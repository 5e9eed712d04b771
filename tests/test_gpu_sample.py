"""Monte-Carlo multi-hop prediction on the MI355X (csrc/scn_hops.hip: scn_sample_draw / scn_sample_expand; Scone_GCN.sample_paths,
multi_hop_reach_probs, multi_hop_target_probs_sampled): the two kernels through the C-ABI against a numpy restatement -- everything
integer equal, scores and path values bitwise, a pick free only where the draw is undecided -- then end to end on a generated data
set: every level replayed on the fp64 oracle, temperature 0 against predict_paths, and the sampled shares against the exact reach
probabilities within five standard deviations."""

import numpy as np
import pytest
import torch

from tests.test_gpu_beam import N_ROOTS, _close, _setup, data, level, tables  # noqa: F401  (data: the module's fixture)
from tests.test_host_beam import step_flow
from tests.test_host_sample import SEED, slot_pick, slot_weights, uniform, within_five_sigma

pytestmark = pytest.mark.gpu

INT32_MAX = (1 << 31) - 1


def delta_of(d):
    """How far from a boundary of the running sum a draw counts as undecided, relative to the total: expf and the fp32 running sum
    against fp64 over at most d terms."""
    return 16 * d * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------
# the kernels through the C-ABI
# ------------------------------------------------------------------------------------------------------------------

def np_sample_draw(c):
    """scn_sample_draw in numpy: (pick, allowed, n_child, err); allowed[r][s] = the picks the device may return for the sample."""
    R, S, d = c["n_roots"], c["n_samples"], c["d"]
    pick = np.full((R, S), -1, np.int32)
    allowed = [[{-1} for _ in range(S)] for _ in range(R)]
    err = INT32_MAX
    for r in range(R):
        l0, l1 = c["leaf_ptr"][r], c["leaf_ptr"][r + 1]
        us = uniform(c["seed"], r, np.arange(S), c["h"])
        tabs = {}
        for k in range(l1 - l0):
            v = int(c["node"][l0 + k])
            if v < 0 or v >= len(c["deg"]):
                continue
            for j in range(int(c["deg"][v])):
                if c["step_edge"][v, j] < 0 or c["step_edge"][v, j] >= c["n_rows"] or c["step_node"][v, j] < 0:
                    err = min(err, (l0 + k) * d + j)
            if c["deg"][v] > 0:
                tabs[k] = slot_weights(c["logp"][l0 + k], int(c["deg"][v]), c["inv_T"], z32=True)
        for s in range(S):
            k = int(c["entry_of"][r, s])
            if k in tabs:
                j, alt = slot_pick(*tabs[k], float(us[s]), delta_of(d))
                pick[r, s] = k * d + j
                allowed[r][s] = {k * d + q for q in alt}
    return pick, allowed, np_n_child(pick), err


def np_n_child(pick):
    return np.array([len(set(row[row >= 0].tolist())) for row in pick], np.int32)


def np_sample_expand(c, pick, with_paths=True):
    """scn_sample_expand in numpy on the given picks."""
    R, S, d, h = c["n_roots"], c["n_samples"], c["d"], c["h"]
    child_ptr = np.concatenate([[0], np.cumsum(np_n_child(pick))]).astype(np.int32)
    C = int(child_ptr[-1])
    out = dict(root=np.zeros(C, np.int32), node=np.zeros(C, np.int32), score=np.zeros(C, np.float32), parent=np.zeros(C, np.int32),
               slot=np.zeros(C, np.int32), count=np.zeros(C, np.int32), entry_of_next=np.full((R, S), -1, np.int32))
    if with_paths:
        out["path_row"], out["path_sign"] = np.zeros((C, h + 1), np.int32), np.zeros((C, h + 1), np.float32)
    for r in range(R):
        l0 = c["leaf_ptr"][r]
        distinct = sorted(set(pick[r][pick[r] >= 0].tolist()))
        for rank, p in enumerate(distinct):
            k, j = divmod(p, d)
            e, ch = l0 + k, child_ptr[r] + rank
            v = int(c["node"][e])
            out["root"][ch], out["node"][ch], out["parent"][ch], out["slot"][ch] = r, c["step_node"][v, j], k, j
            out["score"][ch] = np.float32(c["score"][e]) + np.float32(c["logp"][e, j])
            out["count"][ch] = int((pick[r] == p).sum())
            if with_paths:
                out["path_row"][ch, :h], out["path_row"][ch, h] = c["path_row"][e], c["step_edge"][v, j]
                out["path_sign"][ch, :h], out["path_sign"][ch, h] = c["path_sign"][e], c["step_sign"][v, j]
            out["entry_of_next"][r][pick[r] == p] = rank
    return child_ptr, out


def _dev_tools():
    from scone_gcn_amd import _lib, ops
    dev = torch.device("cuda")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    p = lambda x: None if x is None else ops._dev(x, x.dtype)
    return _lib.load(), ops, dev, t, p


def run_draw(c):
    """One scn_sample_draw with every output pre-filled with junk."""
    lib, ops, dev, t, p = _dev_tools()
    R, S = c["n_roots"], c["n_samples"]
    pick = torch.full((R, S), -7, device=dev, dtype=torch.int32)
    n_child = torch.full((R,), -7, device=dev, dtype=torch.int32)
    err = torch.full((1,), INT32_MAX, device=dev, dtype=torch.int32)
    ins = [t(c["leaf_ptr"], np.int32), t(c["node"], np.int32), t(c["logp"], np.float32), t(c["entry_of"], np.int32), t(c["deg"], np.int32)]
    tabs = [t(c["step_node"], np.int32), t(c["step_edge"], np.int32)]
    status = lib.scn_sample_draw(R, S, c["max_entries"], len(c["node"]), c["h"], c["d"], c["seed"], c["inv_T"], *[p(x) for x in ins],
                                 len(c["deg"]), *[p(x) for x in tabs], c["n_rows"], p(pick), p(n_child), p(err), ops._stream())
    assert status == 0
    torch.cuda.synchronize()
    return pick.cpu().numpy(), n_child.cpu().numpy(), int(err.item())


def run_expand(c, pick, child_ptr, with_paths=True):
    """One scn_sample_expand with every output pre-filled with junk."""
    lib, ops, dev, t, p = _dev_tools()
    R, S, h = c["n_roots"], c["n_samples"], c["h"]
    C = int(child_ptr[-1])
    i32 = lambda *s: torch.full(s, -7, device=dev, dtype=torch.int32)
    outs = [i32(C), i32(C), torch.full((C,), 7.0, device=dev), i32(C), i32(C), i32(C)]
    paths = [i32(C, h + 1), torch.full((C, h + 1), 7.0, device=dev)] if with_paths else [None, None]
    nxt = i32(R, S)
    ins = [t(c["leaf_ptr"], np.int32), t(c["node"], np.int32), t(c["score"], np.float32), t(c["path_row"], np.int32) if h else None,
           t(c["path_sign"], np.float32) if h else None, t(c["logp"], np.float32), t(pick, np.int32), t(child_ptr, np.int32)]
    tabs = [t(c["step_node"], np.int32), t(c["step_edge"], np.int32), t(c["step_sign"], np.float32)]
    status = lib.scn_sample_expand(R, S, c["max_entries"], len(c["node"]), h, c["d"], *[p(x) for x in ins], C, len(c["deg"]),
                                   *[p(x) for x in tabs], *[p(x) for x in outs], *[p(x) for x in paths], p(nxt), ops._stream())
    assert status == 0
    torch.cuda.synchronize()
    got = dict(zip(("root", "node", "score", "parent", "slot", "count"), (x.cpu().numpy() for x in outs)))
    got["entry_of_next"] = nxt.cpu().numpy()
    if with_paths:
        got["path_row"], got["path_sign"] = paths[0].cpu().numpy(), paths[1].cpu().numpy()
    return got


def same(got, want):
    assert set(got) == set(want)
    for key, g in got.items():
        w = want[key]
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g.view(np.int32), w.view(np.int32)), key   # floats bitwise


def make_case(rs, leaf_ptr, n_samples, h, d, n_nodes, n_rows, deg=None, seed=SEED, inv_T=1.0):
    leaf_ptr = np.asarray(leaf_ptr, np.int32)
    L = int(leaf_ptr[-1])
    dg, sn, se, ss = tables(rs, n_nodes, d, n_rows, deg=deg)
    node, score, prow, psign, logp = level(rs, 1, L, h, d, n_nodes, n_rows, 0.25)
    logp = (logp + rs.randn(L, d)).astype(np.float32)                        # off the grid: boundaries of the running sum in general position
    return dict(n_roots=len(leaf_ptr) - 1, n_samples=n_samples, max_entries=int(np.diff(leaf_ptr).max()), h=h, d=d, seed=seed,
                inv_T=inv_T, leaf_ptr=leaf_ptr, node=node, score=score, path_row=prow, path_sign=psign, logp=logp, deg=dg,
                step_node=sn, step_edge=se, step_sign=ss, n_rows=n_rows, entry_of=np.zeros((len(leaf_ptr) - 1, n_samples), np.int32))


def case_a(inv_T=1.0):
    c = make_case(np.random.RandomState(0), [0, 1], 1, 0, 3, 4, 9, deg=[3, 2, 3, 1], inv_T=inv_T)
    c["node"][:] = 0
    return c


def case_b(inv_T=1.0):
    """Root 0: one entry on the degree-1 node, all samples merge into one child.  Root 1: 3 entries, 5 samples.  Root 2: a dropped
    sample (entry_of = -1) and an entry on the degree-0 node.  Root 3: an entry with a NaN, one with +inf and one with all -inf
    among the live log-probabilities.  Root 4: random."""
    rs = np.random.RandomState(1)
    c = make_case(rs, [0, 1, 4, 6, 9, 11], 5, 2, 7, 6, 23, deg=[1, 7, 4, 3, 5, 0], inv_T=inv_T)
    c["node"][:] = [0, 2, 4, 1, 5, 3, 1, 4, 2, 1, 4]
    c["entry_of"][:] = [[0, 0, 0, 0, 0], [0, 1, 2, 1, 0], [0, -1, 1, 1, 0], [0, 1, 2, 0, 1], [1, 0, 0, 1, 1]]
    c["logp"][6, 2], c["logp"][7, 1], c["logp"][7, 3] = np.nan, np.inf, np.inf
    c["logp"][8, :4] = -np.inf
    c["logp"][5, 1] = -np.inf                                                # a slot of weight 0 inside an ordinary entry
    return c


def case_c(inv_T=1.0):
    """70 samples over 64 entries: more samples than lanes of a wave, entries no sample sits in; the last root's tail unused."""
    rs = np.random.RandomState(2)
    c = make_case(rs, [0, 64, 128, 192], 70, 2, 5, 40, 101, inv_T=inv_T)
    c["entry_of"][:2] = rs.randint(0, 64, size=(2, 70))
    c["entry_of"][2] = rs.randint(0, 50, size=70)
    return c


def case_d(inv_T=1.0):
    from scone_gcn_amd._lib import SCN_SAMPLE_MAX as M
    rs = np.random.RandomState(3)
    c = make_case(rs, [0, 1, 201], M, 1, 20, 300, 1009, inv_T=inv_T)
    c["entry_of"][1] = rs.randint(0, 200, size=M)
    return c


CASES = [(case_a, 1.0), (case_b, 1.0), (case_b, 0.5), (case_b, float("inf")), (case_c, 1.0), (case_d, 1.0)]


@pytest.mark.parametrize("case,inv_T", CASES, ids=["a", "b-1", "b-0.5", "b-inf", "c", "d"])
def test_draw_and_expand_match_numpy(case, inv_T):
    c = case(inv_T)
    pick, allowed, n_child, err = np_sample_draw(c)
    n_draws = int((pick >= 0).sum())
    undecided = sum(len(a) > 1 for row in allowed for a in row)
    assert undecided <= 0.005 * n_draws, "badly chosen case: %d of %d draws undecided" % (undecided, n_draws)
    got_pick, got_n_child, got_err = run_draw(c)
    assert got_pick.dtype == np.int32 and got_pick.shape == pick.shape
    moved = 0
    for r in range(c["n_roots"]):
        for s in range(c["n_samples"]):
            assert int(got_pick[r, s]) in allowed[r][s], (r, s, got_pick[r, s], pick[r, s])
            moved += int(got_pick[r, s] != pick[r, s])
    print("draws %d, undecided %d, moved %d" % (n_draws, undecided, moved))
    if moved == 0:
        assert np.array_equal(got_pick, pick)
    assert np.array_equal(got_n_child, np_n_child(got_pick)) and got_err == err == INT32_MAX
    # everything downstream of the picks on the device's picks
    child_ptr, want = np_sample_expand(c, got_pick)
    got = run_expand(c, got_pick, child_ptr)
    same(got, want)
    assert got["count"].sum() == (got_pick >= 0).sum()
    for r in range(c["n_roots"]):
        ch = slice(child_ptr[r], child_ptr[r + 1])
        assert np.all(np.diff(got["parent"][ch] * c["d"] + got["slot"][ch]) > 0)          # ascending (k, j), pairwise distinct
    if case is case_b:
        assert got_n_child[0] == 1 and got["count"][0] == 5                  # all samples of root 0 in one child
        assert got_pick[2].tolist()[0] == got_pick[2].tolist()[1] == got_pick[2].tolist()[4] == -1 and (got_pick[2, 2:4] >= 0).all()
        assert got_pick[3, 0] == got_pick[3, 3] == 0 * 7 + 2 and got_pick[3, 1] == got_pick[3, 4] == 1 * 7 + 1 and got_pick[3, 2] == 2 * 7
        if np.isinf(inv_T):
            lim = c["deg"][c["node"]]
            for r in range(5):
                for s in range(5):
                    k = c["entry_of"][r, s]
                    if got_pick[r, s] >= 0:
                        e = c["leaf_ptr"][r] + k
                        row = c["logp"][e, :lim[e]]
                        assert got_pick[r, s] % 7 == (np.flatnonzero(np.isnan(row))[0] if np.isnan(row).any() else np.argmax(row))
    if case is case_c:
        assert (got_n_child <= 70).all() and (np.bincount(c["entry_of"][0], minlength=64) == 0).any()
    if case is case_d:
        assert got_n_child[0] <= 20 and got_n_child[1] > 200
    # the final-level form differs in nothing else; a second call gives the same bytes
    short = run_expand(c, got_pick, child_ptr, with_paths=False)
    same(short, {k: v for k, v in want.items() if not k.startswith("path")})
    again = run_draw(c)
    assert np.array_equal(again[0], got_pick) and np.array_equal(again[1], got_n_child)
    same(run_expand(c, got_pick, child_ptr), got)


def test_draw_reports_an_undrawn_slot_without_an_edge():
    """The error word does not depend on the draws: each missing pair sits on a slot of weight exp(-1000) = 0, which no sample can
    take, and the lowest (entry, slot) wins."""
    rs = np.random.RandomState(4)
    c = make_case(rs, [0, 2, 4], 6, 1, 4, 5, 17, deg=[4, 4, 3, 4, 2])
    c["node"][:] = [0, 1, 2, 3]
    c["entry_of"][:] = rs.randint(0, 2, size=(2, 6))
    c["logp"][3, 2] = -1000.0
    c["step_edge"][3, 2] = -1
    c["step_edge"][1, 3] = c["n_rows"]                                       # a row out of range counts too: entry 1, slot 3
    c["logp"][1, 3] = -900.0
    c["step_edge"][4, 1] = -1                                                # a node no entry stands on
    pick, allowed, n_child, err = np_sample_draw(c)
    assert err == 1 * 4 + 3
    for seed in (SEED, SEED + 1):
        c["seed"] = seed
        got_pick, _, got_err = run_draw(c)
        assert got_err == err
        assert not (got_pick[0] == 1 * 4 + 3).any() and not (got_pick[1] == 1 * 4 + 2).any()
    c["step_edge"][1, 3] = 5
    assert run_draw(c)[2] == 3 * 4 + 2 == np_sample_draw(c)[3]


def test_sample_steps_refuse_bad_arguments():
    from scone_gcn_amd import _lib
    lib, ops, dev, t, p = _dev_tools()
    M = _lib.SCN_SAMPLE_MAX
    i = torch.zeros((4 * (M + 1),), device=dev, dtype=torch.int32)
    f = torch.zeros((4 * (M + 1),), device=dev)
    pi, pf = ops._dev(i, torch.int32), ops._dev(f)

    def draw(n_samples=1, logp=pf, n_roots=1, max_entries=1, d=3):
        return lib.scn_sample_draw(n_roots, n_samples, max_entries, 1, 0, d, 0, 1.0, pi, pi, logp, pi, pi, 1, pi, pi, 8, pi, pi, pi,
                                   ops._stream())

    def expand(n_samples=1, logp=pf, n_roots=1, max_entries=1, d=3):
        return lib.scn_sample_expand(n_roots, n_samples, max_entries, 1, 0, d, pi, pi, pf, None, None, logp, pi, pi, 1, 1, pi, pi, pf,
                                     pi, pi, pf, pi, pi, pi, None, None, pi, ops._stream())
    for call in (draw, expand):
        assert call(n_samples=M + 1) == _lib.SCN_ERR_UNSUPPORTED
        assert call(max_entries=_lib.SCN_SAMPLE_PAIRS_MAX // 32 + 1, d=32) == _lib.SCN_ERR_UNSUPPORTED
        assert call(max_entries=_lib.SCN_SAMPLE_PAIRS_MAX // 32, d=32, n_roots=0) == 0
        assert call(logp=None) == _lib.SCN_ERR_BAD_ARG
        assert call(n_roots=-1) not in (0, _lib.SCN_ERR_BAD_ARG, _lib.SCN_ERR_UNSUPPORTED)        # SCN_ERR_BAD_SHAPE
        assert call(n_samples=0) == call(n_roots=-1)
        assert call(n_roots=0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------
# end to end (the data set, roots and weights of tests/test_gpu_beam.py)
# ------------------------------------------------------------------------------------------------------------------

def _traced(net, fn, skip="dense", micro_batch=None):
    net._multi_hop_trace, net._multi_hop_fractions = trace, fr = [], []
    net.multi_hop_skip, net.multi_hop_micro_batch = skip, micro_batch
    try:
        out = fn(net)
    finally:
        del net._multi_hop_trace, net._multi_hop_fractions
        net.multi_hop_skip, net.multi_hop_micro_batch = "dense", None
    return out, trace, fr


def _check_against_oracle(s, hops, S, seed=SEED, temperature=1.0, **how):
    """Replays every level of the trace on the fp64 oracle; returns (paths, logp, trace, active fractions)."""
    net, fn, nb, E_lookup, last = s["net"], s["fn"], s["nbrhoods"], s["E_lookup"], s["last"]
    N, D = len(last), nb.shape[1]
    deg = (nb >= 0).sum(axis=1)
    inv_T = np.inf if temperature == 0 else float(np.float32(1.0) / np.float32(temperature))
    (paths, logp), trace, fr = _traced(net, lambda n: n.sample_paths(s["inputs"], hops, S, seed=seed, temperature=temperature), **how)
    assert paths.shape == (N, S, hops) and paths.dtype == np.int64 and logp.shape == (N, S) and logp.dtype == np.float64
    assert len(trace) == hops
    entries = [[(int(last[i]), s["flows"][i].copy(), 0.0, ())] for i in range(N)]
    entry_of = np.zeros((N, S), np.int64)
    undecided = draws = 0
    for h, rec in enumerate(trace):
        ptr = rec["leaf_ptr"]
        assert np.array_equal(np.diff(ptr), [len(e) for e in entries]) and ptr[0] == 0
        flat = [(i, k) for i in range(N) for k in range(len(entries[i]))]
        assert np.array_equal(rec["node"], [entries[i][k][0] for i, k in flat])           # the oracle's entries, in order
        ref = fn(np.asarray([entries[i][k][0] for i, k in flat]), np.stack([entries[i][k][1] for i, k in flat]))
        assert rec["logp"].shape == ref.shape and _close(rec["logp"], ref)
        assert _close(rec["score"], np.array([entries[i][k][2] for i, k in flat]), tol=max(h, 1) * 1e-5)
        assert np.array_equal(rec["entry_of"], entry_of)
        new, new_of = [], np.full((N, S), -1, np.int64)
        for i in range(N):
            n_e = len(entries[i])
            live = entry_of[i] >= 0
            assert np.array_equal(rec["count"][ptr[i]:ptr[i + 1]], np.bincount(entry_of[i][live], minlength=n_e))
            assert rec["count"][ptr[i]:ptr[i + 1]].sum() == live.sum() and (rec["count"][ptr[i]:ptr[i + 1]] > 0).all()
            us = uniform(seed, i, np.arange(S), h)
            tabs = [slot_weights(rec["logp"][ptr[i] + k], deg[entries[i][k][0]], inv_T, z32=True) for k in range(n_e)]
            for sm in range(S):                                              # the slot rule on the TRACED log-probabilities
                k, pk = int(entry_of[i, sm]), int(rec["pick"][i, sm])
                if k < 0:
                    assert pk == -1
                    continue
                _, alt = slot_pick(*tabs[k], float(us[sm]), delta_of(D))
                assert pk // D == k and pk % D in alt
                draws += 1
                undecided += len(alt) > 1
            distinct = sorted(set(rec["pick"][i][rec["pick"][i] >= 0].tolist()))
            ch = slice(rec["child_ptr"][i], rec["child_ptr"][i + 1])
            assert (rec["parent"][ch] * D + rec["slot"][ch]).tolist() == distinct          # ascending (k, j), pairwise distinct
            out = []
            for rank, pk in enumerate(distinct):
                k, j = divmod(pk, D)
                v, f, sc, path = entries[i][k]
                assert j < deg[v]
                u = int(nb[v][j])
                out.append((u, step_flow(f, v, u, E_lookup), sc + ref[ptr[i] + k, j], path + (u,)))
                new_of[i][rec["pick"][i] == pk] = rank
            assert len(set(e[3] for e in out)) == len(out)
            new.append(out)
        entries, entry_of = new, new_of
    assert (entry_of >= 0).all()                                             # no node of this complex is without neighbours
    for i in range(N):
        for sm in range(S):
            path, sc = entries[i][entry_of[i, sm]][3], entries[i][entry_of[i, sm]][2]
            assert tuple(paths[i, sm]) == path and abs(logp[i, sm] - sc) <= hops * 1e-5 * max(1.0, abs(sc))
            prev = int(last[i])
            for u in path:
                assert u in nb[prev][:deg[prev]]                             # consecutive nodes are adjacent
                prev = int(u)
    print("draws %d, undecided %d" % (draws, undecided))
    return paths, logp, trace, fr


@pytest.mark.parametrize("model_type", ["scone", "ebli", "bunch"])
@pytest.mark.parametrize("hops", [2, 4])
@pytest.mark.parametrize("S", [3, 64])
def test_samples_follow_the_oracle(data, model_type, hops, S):
    _check_against_oracle(_setup(data, model_type), hops, S)


@pytest.mark.parametrize("hops", [2, 4])
@pytest.mark.parametrize("S", [3, 64])
def test_samples_follow_the_oracle_on_field_of_view_lists(data, hops, S):
    *_, fr = _check_against_oracle(_setup(data, "scone"), hops, S, skip="field")
    assert fr                                                                # the forwards did run on lists


def test_micro_batches_move_no_decided_draw(data):
    s = _setup(data, "scone")
    *_, trace, _ = _check_against_oracle(s, 4, 64, micro_batch=8)
    assert max(len(rec["node"]) for rec in trace) > 8                        # the levels were split


@pytest.mark.parametrize("model_type", ["scone", "ebli", "bunch"])
def test_temperature_zero_is_predict_paths(data, model_type):
    s = _setup(data, model_type)
    hops, S = 3, 7
    (paths, logp), trace, _ = _traced(s["net"], lambda n: n.sample_paths(s["inputs"], hops, S, seed=5, temperature=0.0))
    greedy = s["net"].predict_paths(s["inputs"], hops)
    assert np.array_equal(paths, np.broadcast_to(greedy[:, None, :], paths.shape)) and np.isfinite(logp).all()
    for rec in trace:
        assert np.array_equal(rec["leaf_ptr"], np.arange(N_ROOTS + 1)) and (rec["count"] == S).all()


def test_shares_are_within_five_sigma_of_the_reach_probabilities(data):
    """The exact reach probabilities come from the full-width beams (predict_paths_beam: every path with its summed
    log-probability).  The model's log-softmax runs over all max_deg slots, so on a node of lower degree the live log-probabilities
    do not sum to one, and the slot rule draws from their renormalisation over the live slots: each step of a path is renormalised
    the same way -- the first step by the total of the 1-hop beam, the second by the total over the paths that share the first
    node -- before the paths ending at a node are summed."""
    from scone_gcn_amd._lib import SCN_SAMPLE_MAX as S
    s = _setup(data, "scone")
    net, inputs = s["net"], s["inputs"]
    one_p, one_lp = net.predict_paths_beam(inputs, 1, 256)
    two_p, two_lp = net.predict_paths_beam(inputs, 2, 256)
    nodes, freq = net.multi_hop_reach_probs(inputs, 2, S, seed=SEED)
    paths, _ = net.sample_paths(inputs, 2, S, seed=SEED)
    targets = s["targets"]
    tp = net.multi_hop_target_probs_sampled(inputs, targets, 2, S, seed=SEED)
    assert nodes.dtype == np.int64 and freq.dtype == np.float64 and nodes.shape == freq.shape
    seen = 0
    for i in range(N_ROOTS):
        live1, live2 = one_p[i, :, 0] >= 0, two_p[i, :, 0] >= 0
        assert live2.sum() < 256                                             # the beam held every path
        z0 = np.exp(one_lp[i][live1]).sum()
        step1 = dict(zip(one_p[i, live1, 0].tolist(), np.exp(one_lp[i][live1])))
        p = {}
        for a in step1:
            sel = live2 & (two_p[i, :, 0] == a)
            z1 = np.exp(two_lp[i][sel]).sum() / step1[a]
            for b, lp in zip(two_p[i, sel, 1].tolist(), two_lp[i][sel]):
                p[b] = p.get(b, 0.0) + np.exp(lp) / (z0 * z1)
        assert abs(sum(p.values()) - 1.0) <= 1e-5
        got = {int(v): f for v, f in zip(nodes[i], freq[i]) if v >= 0}
        assert set(got) <= set(p)
        for b in p:
            assert within_five_sigma(got.get(b, 0.0), p[b], S), (i, b, got.get(b, 0.0), p[b])
            seen += 1
        # the layout: highest share first, ties by the lower node id, tail -1 / 0; the shares of a root sum to 1
        k = len(got)
        assert (nodes[i, k:] == -1).all() and (freq[i, k:] == 0).all() and abs(freq[i].sum() - 1.0) <= 1e-12
        order = sorted(got, key=lambda v: (-got[v], v))
        assert nodes[i, :k].tolist() == order
        ends = paths[i, :, -1]
        assert all(got[v] == (ends == v).sum() / np.float64(S) for v in got)
        assert tp[i] == np.mean(ends == targets[i])                          # exactly
    assert seen > N_ROOTS and tp.shape == (N_ROOTS,) and tp.dtype == np.float64


def test_same_seed_same_bytes_other_seed_other_paths(data):
    s = _setup(data, "scone")
    net = s["net"]
    a = net.sample_paths(s["inputs"], 3, 16, seed=11)
    b = net.sample_paths(s["inputs"], 3, 16, seed=11)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    c = net.sample_paths(s["inputs"], 3, 16, seed=(1 << 40) + 11)
    assert not np.array_equal(a[0], c[0])
    r1, r2 = net.multi_hop_reach_probs(s["inputs"], 3, 16, seed=11), net.multi_hop_reach_probs(s["inputs"], 3, 16, seed=11)
    assert r1[0].tobytes() == r2[0].tobytes() and r1[1].tobytes() == r2[1].tobytes()


def test_missing_pair_raises_key_error_and_flows_stay(data):
    s = _setup(data, "scone")
    net, X = s["net"], s["inputs"][-1]
    before = X.copy()
    with pytest.raises(KeyError):
        net.sample_paths(s["inputs"], 2, 3, nbrhoods=s["nbrhoods"], E_lookup={})
    v = int(s["last"][0])
    u = int(s["nbrhoods"][v][0])
    lookup = dict(s["E_lookup"])
    del lookup[(min(v, u), max(v, u))]
    for seed in (0, 1):
        with pytest.raises(KeyError) as exc:
            net.sample_paths(s["inputs"], 2, 3, seed=seed, nbrhoods=s["nbrhoods"], E_lookup=lookup)
        assert exc.value.args[0] == (v, u)                                    # the lowest (entry, slot) without an edge, whatever the draws
    net.sample_paths(s["inputs"], 2, 3)
    assert np.array_equal(np.asarray(before.view(np.uint8)), np.asarray(X.view(np.uint8)))     # bitwise


def test_train_model_samples_switch(tmp_path, monkeypatch):
    from scone_gcn_amd import dataset_io, scone_trajectory_model as stm, trajectory_experiments as te
    monkeypatch.chdir(tmp_path)
    dataset_io.generate_dataset(150, 45, folder="drv", holes=True)
    argv = ["prog", "-epochs", "1", "-batch_size", "12", "-data_folder_suffix", "drv", "-describe", "0", "-multi_hop", "1",
            "-multi_hop_samples", "64"]
    hp = te.hyperparams(argv)
    hp["hidden_layers"] = [(3, 16)] * 3
    stm.reseed(1030)
    net, _ = te.train_model(hp)
    got = net.experiment_results["multi_hop_sampled"]
    inputs_all, y_all, train_mask, test_mask, shifts, G, E_lookup, nbrhoods, n_nbrs, targets_all, prefixes = \
        te.data_setup(hops=(1, 2), folder_suffix="drv", hp=hp)
    tp = net.multi_hop_target_probs_sampled(inputs_all[0], targets_all[1], 2, 64, seed=0)
    want = [float(np.average(tp[np.asarray(m) == 1])) for m in (train_mask, test_mask)]
    assert got == want and len(got) == 2 and all(0.0 <= a <= 1.0 for a in got)
    assert len(net.experiment_results["multi_hop"]) == 2
    net._drop_graphs()                                                        # the captured training steps go now, not whenever the collector runs
    stm.reseed(1030)
