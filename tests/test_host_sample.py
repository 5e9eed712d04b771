"""Monte-Carlo multi-hop prediction without a GPU: the generator (Philox4x32-10, known answers, the library's host entry point
bitwise), this file's restatements of the slot rule and of Scone_GCN.sample_paths -- S independent chains, and the merged form the
device runs (one entry per distinct path, with a count) -- checked against each other, against the greedy path and against the exact
reach probabilities on the 4-node graph, plus the argument checks and the -multi_hop_samples switch.  tests/test_gpu_sample.py
imports the restatements."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import scone_oracle as so
from scone_gcn_amd._lib import SCN_BEAM_MAX, SCN_SAMPLE_MAX
from tests.test_host_beam import _case, ref_beam, step_flow
from tests.test_host_multihop import _tiny4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261018                                                              # the seed of the five-sigma checks, here and on the GPU
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------------
# the generator
# ------------------------------------------------------------------------------------------------------------------

def philox4x32_10(ctr, key):
    """The block function on numpy uint64 arrays of shape (..., 4) / (..., 2) holding 32-bit words; returns (..., 4)."""
    c = [np.asarray(ctr, np.uint64)[..., i] for i in range(4)]
    k = [np.asarray(key, np.uint64)[..., i] for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & np.uint64(M32), (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & np.uint64(M32)]
        k = [(k[0] + np.uint64(0x9E3779B9)) & np.uint64(M32), (k[1] + np.uint64(0xBB67AE85)) & np.uint64(M32)]
    return np.stack(c, axis=-1)


def uniform(seed, r, s, h):
    """The uniform of (seed, root, sample, hop) as float64 (24 bits: exact in float32 too); r, s, h broadcast."""
    r, s, h = np.broadcast_arrays(np.asarray(r, np.int64), np.asarray(s, np.int64), np.asarray(h, np.int64))
    ctr = np.stack([r & M32, s & M32, h & M32, np.zeros_like(r)], axis=-1).astype(np.uint64)
    key = np.broadcast_to(np.array([int(seed) & M32, (int(seed) >> 32) & M32], np.uint64), r.shape + (2,))
    return (philox4x32_10(ctr, key)[..., 0] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((M32,) * 4, (M32,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def test_philox_known_answers():
    for ctr, key, want in KNOWN:
        assert " ".join("%08x" % int(x) for x in philox4x32_10(ctr, key)) == want


def test_library_uniform_matches_the_restatement_bitwise():
    from scone_gcn_amd import _lib
    lib = _lib.load()
    rs = np.random.RandomState(0)
    seeds = [0, 1, SEED, (1 << 32) + 5, (0xDEADBEEF << 32) | 0x12345678, (1 << 64) - 1]
    n = 0
    for seed in seeds:
        r = np.concatenate([[0, 0, 1, 4095], rs.randint(0, 1 << 20, 60)])
        s = np.concatenate([[0, 1, 0, SCN_SAMPLE_MAX - 1], rs.randint(0, SCN_SAMPLE_MAX, 60)])
        h = np.concatenate([[0, 0, 0, 7], rs.randint(0, 16, 60)])
        want = uniform(seed, r, s, h)
        assert ((0 <= want) & (want < 1)).all()
        for i in range(len(r)):
            u = ctypes.c_float(-1.0)
            assert lib.scn_sample_uniform(seed, int(r[i]), int(s[i]), int(h[i]), ctypes.byref(u)) == 0
            assert np.float32(u.value).view(np.uint32) == np.float32(want[i]).view(np.uint32)
            n += 1
    assert n >= 300
    assert lib.scn_sample_uniform(0, 0, 0, 0, None) == _lib.SCN_ERR_BAD_ARG
    # the seed's high word is part of the key
    assert uniform(5, 0, 0, 0) != uniform((1 << 32) + 5, 0, 0, 0)


def test_sample_max_matches_the_header():
    from scone_gcn_amd import _lib
    src = open(os.path.join(ROOT, "include", "scone_hip.h")).read()
    assert int(re.search(r"#define\s+SCN_SAMPLE_MAX\s+(\d+)", src).group(1)) == SCN_SAMPLE_MAX == 4096
    pairs = int(re.search(r"#define\s+SCN_SAMPLE_PAIRS_MAX\s+(\d+)", src).group(1))
    assert pairs == _lib.SCN_SAMPLE_PAIRS_MAX >= 4096 * 32


# ------------------------------------------------------------------------------------------------------------------
# the slot rule and the two restatements: model_fn(last_nodes (n,), flows (n, E)) -> log-probabilities (n, D)
# ------------------------------------------------------------------------------------------------------------------

def first_argmax(row):
    """np.argmax with a NaN counting as the maximum (the first NaN wins): the rule of scn_hop_select."""
    nan = np.flatnonzero(np.isnan(row))
    return int(nan[0]) if len(nan) else int(np.argmax(row))


def slot_weights(row, lim, inv_T, z32=False):
    """(argmax a, weights w, running sums c) of an entry with lim >= 1 live slots; w = c = None where the rule is the argmax (inv_T
    = +inf, or a maximum that is NaN or +-inf).  fp64 throughout, or with z32 the fp32 subtract and multiply of the device followed
    by fp64 exp and running sum."""
    row = np.asarray(row)[:lim]
    a = first_argmax(row)
    m = row[a]
    if np.isinf(inv_T) or not np.isfinite(m):
        return a, None, None
    if z32:
        z = ((row.astype(np.float32) - np.float32(m)) * np.float32(inv_T)).astype(np.float64)
    else:
        z = (row.astype(np.float64) - np.float64(m)) * np.float64(inv_T)
    w = np.exp(z)
    return a, w, np.cumsum(w)


def slot_pick(a, w, c, u, delta=0.0):
    """(slot, allowed) of the uniform u on slot_weights' output.  allowed = the slots the device may return: the slot itself and,
    with delta > 0, every slot of positive weight whose interval of the running sum comes within delta * total of u * total (an
    undecided draw: allowed has more than one member)."""
    if w is None:
        return a, {a}
    thr = u * c[-1]
    j = int(np.searchsorted(c, thr, side="right"))                           # the first j with c[j] > thr
    if j >= len(c):
        j = int(np.flatnonzero(w > 0)[-1])
    allowed = {j}
    if delta:
        lo, hi = thr - delta * c[-1], thr + delta * c[-1]
        for q in np.flatnonzero(w > 0):
            if c[q] > lo and (c[q - 1] if q else 0.0) <= hi:
                allowed.add(int(q))
    return j, allowed


def slot_rule(row, lim, inv_T, u, z32=False, delta=0.0):
    """The slot rule of one sample in one entry: the first slot whose running sum of exp((logp_j - m) * inv_T) exceeds u * total."""
    return slot_pick(*slot_weights(row, lim, inv_T, z32), u, delta)


def _inv_T(temperature):
    return np.inf if temperature == 0 else float(np.float32(1.0) / np.float32(temperature))


def ref_sample(model_fn, flows, last_nodes, nbrhoods, E_lookup, hops, n_samples, seed, temperature):
    """S independent chains per root, no merging: (paths [N][S] tuples of node ids or None for a dropped sample, logp (N, S))."""
    nb = np.asarray(nbrhoods)
    deg = (nb >= 0).sum(axis=1)
    inv_T = _inv_T(temperature)
    N = len(flows)
    chains = {(i, s): (int(last_nodes[i]), np.array(flows[i], np.float64), 0.0, ()) for i in range(N) for s in range(n_samples)}
    for h in range(hops):
        keys = sorted(chains)
        logp = model_fn(np.asarray([chains[k][0] for k in keys]), np.stack([chains[k][1] for k in keys]))
        for n, (i, s) in enumerate(keys):
            v, f, sc, path = chains.pop((i, s))
            if deg[v] == 0:
                continue
            j, _ = slot_rule(logp[n], deg[v], inv_T, float(uniform(seed, i, s, h)))
            u = int(nb[v][j])
            chains[(i, s)] = (u, step_flow(f, v, u, E_lookup), sc + logp[n, j], path + (u,))
    paths = [[chains[(i, s)][3] if (i, s) in chains else None for s in range(n_samples)] for i in range(N)]
    lp = np.array([[chains[(i, s)][2] if (i, s) in chains else -np.inf for s in range(n_samples)] for i in range(N)])
    return paths, lp


def ref_sample_merged(model_fn, flows, last_nodes, nbrhoods, E_lookup, hops, n_samples, seed, temperature, sizes=None):
    """The same samples the way the device computes them: per root one entry per distinct path with a count, every sample drawn
    inside its entry, equal (entry, slot) picks merged into one child, children in ascending (k, j).  sizes: a list that gets
    the entries per root of every level."""
    nb = np.asarray(nbrhoods)
    deg = (nb >= 0).sum(axis=1)
    inv_T = _inv_T(temperature)
    N = len(flows)
    entries = [[(int(last_nodes[i]), np.array(flows[i], np.float64), 0.0, (), n_samples)] for i in range(N)]
    entry_of = np.zeros((N, n_samples), np.int64)
    for h in range(hops):
        if sizes is not None:
            sizes.append([len(e) for e in entries])
        flat = [(i, k) for i in range(N) for k in range(len(entries[i]))]
        logp = model_fn(np.asarray([entries[i][k][0] for i, k in flat]), np.stack([entries[i][k][1] for i, k in flat]))
        at = {ik: n for n, ik in enumerate(flat)}
        new, new_of = [], np.full((N, n_samples), -1, np.int64)
        for i in range(N):
            picks = {}
            us = uniform(seed, i, np.arange(n_samples), h)
            tables = [slot_weights(logp[at[(i, k)]], deg[e[0]], inv_T) if deg[e[0]] else None for k, e in enumerate(entries[i])]
            for s in range(n_samples):
                k = int(entry_of[i, s])
                if k < 0 or tables[k] is None:
                    continue
                j, _ = slot_pick(*tables[k], float(us[s]))
                picks.setdefault((k, j), []).append(s)
            assert sum(len(v) for v in picks.values()) <= sum(e[4] for e in entries[i])
            out = []
            for rank, (k, j) in enumerate(sorted(picks)):
                v, f, sc, path, _ = entries[i][k]
                u = int(nb[v][j])
                out.append((u, step_flow(f, v, u, E_lookup), sc + logp[at[(i, k)], j], path + (u,), len(picks[(k, j)])))
                new_of[i, picks[(k, j)]] = rank
            new.append(out)
        entries, entry_of = new, new_of
    paths = [[entries[i][entry_of[i, s]][3] if entry_of[i, s] >= 0 else None for s in range(n_samples)] for i in range(N)]
    lp = np.array([[entries[i][entry_of[i, s]][2] if entry_of[i, s] >= 0 else -np.inf for s in range(n_samples)] for i in range(N)])
    return paths, lp


def over_live_slots(model_fn, nbrhoods):
    """model_fn with every row renormalised over the live slots of its node (dead slots -inf).  The model's log-softmax runs over
    all D slots, so on a node of lower degree its live log-probabilities do not sum to one; the slot rule draws from their
    renormalisation (it divides by the total over the live slots), and the exact probabilities have to be taken from the same."""
    deg = (np.asarray(nbrhoods) >= 0).sum(axis=1)

    def fn(last, X):
        lp = np.array(model_fn(last, X), np.float64)
        for n, v in enumerate(np.asarray(last)):
            lp[n, deg[v]:] = -np.inf
            lp[n] -= np.log(np.exp(lp[n, :deg[v]]).sum())
        return lp
    return fn


def reach_probs(model_fn, flows, last_nodes, nbrhoods, E_lookup, hops, n_nodes):
    """Exact probability of standing on node t after `hops` steps, (N, n_nodes): the sum of exp(score) over the paths of the
    full-width beam that end at t, on the log-probabilities over_live_slots."""
    full = ref_beam(over_live_slots(model_fn, nbrhoods), flows, last_nodes, nbrhoods, E_lookup, hops, SCN_BEAM_MAX)
    p = np.zeros((len(flows), n_nodes))
    for i, paths in enumerate(full):
        assert len(paths) < SCN_BEAM_MAX                                     # the beam held every path
        for path, score in paths:
            p[i, path[-1]] += np.exp(score)
    return p


def within_five_sigma(f, p, n_samples):
    """|f - p| <= 5 sqrt(p (1 - p) / S) + 1 / S: five standard deviations of a binomial share, plus one sample."""
    p = np.clip(p, 0.0, 1.0)
    return np.abs(f - p) <= 5.0 * np.sqrt(p * (1.0 - p) / n_samples) + 1.0 / n_samples


def test_slot_rule_edges():
    row = np.log(np.array([0.5, 0.25, 0.25, 1e-30]))
    assert slot_rule(row, 3, 1.0, 0.0)[0] == 0 and slot_rule(row, 3, 1.0, 0.49)[0] == 0
    assert slot_rule(row, 3, 1.0, 0.5)[0] == 1 and slot_rule(row, 3, 1.0, 0.76)[0] == 2
    assert slot_rule(row, 3, 1.0, 1 - 2.0 ** -24)[0] == 2                   # slot 3 is not live
    assert slot_rule(row, 3, np.inf, 0.9)[0] == 0                            # temperature 0: the argmax
    assert slot_rule(row, 3, 0.5, 0.40)[0] == 0 and slot_rule(row, 3, 0.5, 0.42)[0] == 1    # sqrt weights: .414 / .293 / .293
    assert slot_rule([-1.0, np.nan, 0.0], 3, 1.0, 0.99)[0] == 1              # NaN: the argmax rule, a NaN is the maximum
    assert slot_rule([-1.0, np.inf, np.inf], 3, 1.0, 0.99)[0] == 1           # first +inf
    assert slot_rule([-np.inf, -np.inf], 2, 1.0, 0.99)[0] == 0               # all -inf
    assert slot_rule([-np.inf, 0.0, -np.inf], 3, 1.0, 0.0)[0] == 1           # a slot of weight 0 is never drawn, not even at u = 0
    j, allowed = slot_rule(row, 3, 1.0, 0.5 + 1e-9, z32=True, delta=1e-6)
    assert j == 1 and allowed == {0, 1}
    assert slot_rule(row, 3, 1.0, 0.6, z32=True, delta=1e-6) == (1, {1})


@pytest.mark.parametrize("model_type", ["scone", "ebli", "bunch"])
def test_temperature_zero_is_the_greedy_path(model_type):
    """Every sample of a root walks one path, the merged form keeps one entry per root, and that path is ref_beam(beam = 1)'s.
    The graph's symmetry makes two neighbours of node 2 tie to the last bits of fp64 (tests/test_host_beam.py), where the beam's
    order (on score + log-probability) and the argmax of the row may part: every step must be A maximum to 1e-12 of a single
    forward, and a path none of whose steps came closer than 1e-9 to a tie must be the beam's, with its score."""
    fn, flows, last, nb, E_lookup = _case(model_type)
    hops = 3
    greedy = ref_beam(fn, flows, last, nb, E_lookup, hops, 1)
    sizes = []
    paths, lp = ref_sample(fn, flows, last, nb, E_lookup, hops, 5, SEED, 0.0)
    assert ref_sample_merged(fn, flows, last, nb, E_lookup, hops, 5, SEED, 0.0, sizes)[0] == paths
    assert sizes == [[1] * 4] * hops
    for i in range(4):
        assert all(path == paths[i][0] for path in paths[i])
        v, f, total, tied = int(last[i]), flows[i].copy(), 0.0, False
        for u in paths[i][0]:
            row = fn(np.array([v]), f[None])[0]
            live = row[:(nb[v] >= 0).sum()]
            j = list(nb[v]).index(u)
            assert j < len(live) and live[j] >= live.max() - 1e-12
            tied = tied or (len(live) > 1 and np.sort(live)[-2] >= live.max() - 1e-9)
            f = step_flow(f, v, int(u), E_lookup)
            total += row[j]
            v = int(u)
        assert abs(lp[i, 0] - total) <= 1e-12
        if not tied:
            assert paths[i][0] == greedy[i][0][0] and abs(lp[i, 0] - greedy[i][0][1]) <= 1e-12


@pytest.mark.parametrize("model_type", ["scone", "ebli", "bunch"])
def test_merged_restatement_gives_every_sample_the_same_path(model_type):
    fn, flows, last, nb, E_lookup = _case(model_type)
    for temperature in (1.0, 0.5):
        sizes = []
        one = ref_sample(fn, flows, last, nb, E_lookup, 3, 96, SEED, temperature)
        merged = ref_sample_merged(fn, flows, last, nb, E_lookup, 3, 96, SEED, temperature, sizes)
        assert one[0] == merged[0]
        assert np.abs(one[1] - merged[1]).max() <= 1e-12
        assert sizes[0] == [1] * 4 and max(sizes[2]) <= 9 and sum(sizes[2]) > 4            # distinct paths, far fewer than samples


@pytest.mark.parametrize("model_type", ["scone", "ebli", "bunch"])
@pytest.mark.parametrize("hops", [2, 3])
def test_sampled_shares_are_within_five_sigma_of_the_reach_probabilities(model_type, hops):
    fn, flows, last, nb, E_lookup = _case(model_type)
    S = SCN_SAMPLE_MAX
    p = reach_probs(fn, flows, last, nb, E_lookup, hops, 4)
    assert np.abs(p.sum(axis=1) - 1.0).max() <= 1e-12
    paths, _ = ref_sample_merged(fn, flows, last, nb, E_lookup, hops, S, SEED, 1.0)
    f = np.array([[sum(path[-1] == t for path in paths[i]) / S for t in range(4)] for i in range(4)])
    assert within_five_sigma(f, p, S).all(), (f, p)
    print(model_type, hops, 'p', p.round(4).tolist(), 'f', f.round(4).tolist())
    assert (f[p == 0] == 0).all()


# ------------------------------------------------------------------------------------------------------------------
# arguments and switches
# ------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_raise():
    from scone_gcn_amd.scone_trajectory_model import Scone_GCN
    net = Scone_GCN(1, 1e-3, 4, 0.0, verbose=False)
    inputs = [None, [0], None]
    for hops, n, temp in ((0, 4, 1.0), (1, 0, 1.0), (2, -3, 1.0), (1, SCN_SAMPLE_MAX + 1, 1.0), (1, 4, -0.5), (1, 4, float("nan"))):
        with pytest.raises(ValueError):
            net.sample_paths(inputs, hops, n, temperature=temp)
        with pytest.raises(ValueError):
            net.multi_hop_reach_probs(inputs, hops, n, temperature=temp)
    for hops, n in ((0, 4), (1, 0), (1, SCN_SAMPLE_MAX + 1)):
        with pytest.raises(ValueError):
            net.multi_hop_target_probs_sampled(inputs, [0], hops, n)


def test_probed_closure_is_refused():
    from scone_gcn_amd.scone_trajectory_model import Scone_GCN
    net = Scone_GCN(1, 1e-3, 4, 0.0, verbose=False)
    net.model_type = "scone"
    B1, B2, edges, E_lookup = _tiny4()
    nb, _ = so.neighborhoods(edges, 4)
    inputs = [so.make_Bconds(B1, nb), np.array([1]), np.zeros((1, 5, 1))]
    for call in (lambda: net.sample_paths(inputs, 2, 4), lambda: net.multi_hop_reach_probs(inputs, 2, 4),
                 lambda: net.multi_hop_target_probs_sampled(inputs, [0], 2, 4)):
        with pytest.raises(TypeError, match="Bconds"):
            call()


def test_samples_switch_parses():
    from scone_gcn_amd import trajectory_experiments as te
    assert te.hyperparams(["prog"])["multi_hop_samples"] == 0
    hp = te.hyperparams(["prog", "-multi_hop", "1", "-multi_hop_samples", "64"])
    assert hp["multi_hop_samples"] == 64 and hp["multi_hop"] == 1


def test_docstring_states_the_difference_from_the_tree():
    from scone_gcn_amd.scone_trajectory_model import Scone_GCN
    doc = Scone_GCN.multi_hop_target_probs_sampled.__doc__
    assert "NUMBER of paths" in doc and "scn_tree_target" in doc
