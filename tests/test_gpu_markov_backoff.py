"""The variable-order Markov baseline on the device: the scn_markov_hash_* kernels through the C-ABI and Markov_Backoff against the
dictionary restatement of tests/test_host_markov_backoff.py -- every integer equal, every float64 bitwise.  Without back-off they are
the direct-addressed kernels bit for bit; with it cfg1 at K = 2, 4, 8; then the table at its limits (load above 0.9, wrapping probe
chains, a capacity below the number of keys), 4096 writers per key, the shapes the direct-table tests single out, and train_model()
with -markov_backoff 1."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_gpu_markov import Dev, same_bits, star70
from tests.test_host_baseline_paths import path_items
from tests.test_host_markov import INT32_MAX, TINY_WALKS, cfg1_markov, ragged, table_from_edges, tiny4
from tests.test_host_markov_backoff import (KEY_SHIFT, cfg1_backoff, key_bound, n_states, perplexity, ref_backoff_path_scores,
                                            ref_backoff_probs, ref_backoff_rollout, ref_backoff_train, ref_backoff_two_target)

pytestmark = pytest.mark.gpu

GUARD = 8                      # guard words before and after every buffer of a table
GUARD32, GUARD64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


def guarded(n, dtype, fill):
    """(the n elements, the whole buffer): GUARD elements of the guard pattern on either side."""
    buf = torch.full((n + 2 * GUARD,), GUARD64 if dtype == torch.int64 else GUARD32, dtype=dtype, device="cuda")
    buf[GUARD:GUARD + n] = fill
    return buf[GUARD:GUARD + n], buf


class Table:
    """A table built by the three launches; every buffer sits between guard words."""

    def __init__(self, dev, ptr, nodes, K, capacity):
        self.dev, self.K, self.capacity = dev, K, capacity
        lib, p = dev.lib, dev.p
        d_ptr, d_nodes = dev.up(ptr), dev.up(nodes)
        self.keys, self.keys_buf = guarded(capacity, torch.int64, -1)
        self.row_of, self.row_buf = guarded(capacity, torch.int32, -9)
        self.words, self.words_buf = guarded(3 + K, torch.int32, 0)          # n_states | err | overflow | n_states per order
        self.words[1:3] = INT32_MAX
        walk = (len(ptr) - 1, p(d_ptr), p(d_nodes), K) + tuple(dev.graph())
        self.status = [lib.scn_markov_hash_insert(*walk, p(self.keys), capacity, p(self.words[1:2]), p(self.words[2:3]), dev.stream()),
                       lib.scn_markov_hash_number(p(self.keys), capacity, K, p(self.row_of), p(self.words[0:1]), p(self.words[3:]),
                                                  dev.stream())]
        host = self.words.cpu().numpy()
        self.n, self.err, self.overflow, self.per_order = int(host[0]), int(host[1]), int(host[2]), host[3:].tolist()
        self.counts, self.counts_buf = guarded(max(self.n, 1) * dev.D, torch.int32, 0)
        self.status.append(lib.scn_markov_hash_count(*walk, p(self.keys), p(self.row_of), capacity, self.n, p(self.counts),
                                                     p(self.words[1:2]), dev.stream()))
        torch.cuda.synchronize()
        self.err = int(self.words[1].item())

    def args(self):
        p = self.dev.p
        return p(self.keys), p(self.row_of), self.capacity, p(self.counts)

    def intact(self):
        """Nothing was written outside the buffers."""
        for buf in (self.keys_buf, self.row_buf, self.words_buf, self.counts_buf):
            g = GUARD64 if buf.dtype == torch.int64 else GUARD32
            if not (bool((buf[:GUARD] == g).all()) and bool((buf[-GUARD:] == g).all())):
                return False
        return True

    def slots(self):
        """(slot numbers, keys as Python ints, rows) of the slots that hold a key."""
        keys = self.keys.cpu().numpy().view(np.uint64)
        at = np.flatnonzero(keys != np.uint64(2 ** 64 - 1))
        return at, [int(k) for k in keys[at]], self.row_of.cpu().numpy()[at]

    def as_dict(self):
        """{(order, state): counts row}; every key in one slot, the rows a numbering of 0 .. n - 1, -1 in the empty slots."""
        at, keys, rows = self.slots()
        assert len(set(keys)) == len(keys) == self.n and sorted(rows.tolist()) == list(range(self.n))
        assert int((self.row_of.cpu().numpy() == -1).sum()) == self.capacity - self.n
        counts = self.counts.cpu().numpy().reshape(-1, self.dev.D)
        return {((k >> KEY_SHIFT) + 1, k & ((1 << KEY_SHIFT) - 1)): counts[r] for k, r in zip(keys, rows)}


def same_table(got, want):
    return sorted(got) == sorted(want) and all(np.array_equal(got[k], want[k]) for k in want)


class HDev(Dev):
    """The readers of the hashed table: host arrays and the err word(s)."""

    def build(self, walks, K, capacity=None):
        ptr, nodes = ragged(walks)
        if capacity is None:
            capacity = 1 << max(1, int(2 * sum(key_bound(ptr, K)) - 1).bit_length())
        return Table(self, ptr, nodes, K, capacity)

    def h_rollout(self, t, ptr, nodes, backoff, min_count, hops, seed):
        n = len(ptr) - 1
        d_ptr, d_nodes, err = self.up(ptr), self.up(nodes), self.word()
        pred, tied, used = (torch.full((n, hops), -7, dtype=torch.int32, device="cuda") for _ in range(3))
        assert self.lib.scn_markov_hash_rollout(n, self.p(d_ptr), self.p(d_nodes), t.K, int(backoff), min_count, hops, ctypes.c_uint64(seed),
                                                *self.graph(), *t.args(), self.p(pred), self.p(tied), self.p(used), self.p(err),
                                                self.stream()) == 0
        torch.cuda.synchronize()
        return pred.cpu().numpy(), tied.cpu().numpy(), used.cpu().numpy(), int(err.item())

    def h_two_target(self, t, ptr, nodes, backoff, min_count, seed, target):
        n = len(ptr) - 1
        d_ptr, d_nodes, err, err_t = self.up(ptr), self.up(nodes), self.word(), self.word()
        d_t = self.up(np.asarray(target, np.int32))
        score = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        other, used = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
        assert self.lib.scn_markov_hash_two_target(n, self.p(d_ptr), self.p(d_nodes), t.K, int(backoff), min_count, ctypes.c_uint64(seed),
                                                   self.p(d_t), *self.graph(), *t.args(), self.p(score), self.p(other), self.p(used),
                                                   self.p(err), self.p(err_t), self.stream()) == 0
        torch.cuda.synchronize()
        return score.cpu().numpy(), other.cpu().numpy(), used.cpu().numpy(), int(err.item()), int(err_t.item())

    def h_probs(self, t, ptr, nodes, backoff, min_count):
        n = len(ptr) - 1
        d_ptr, d_nodes, err = self.up(ptr), self.up(nodes), self.word()
        probs = torch.full((n, self.D), -7.0, dtype=torch.float64, device="cuda")
        used = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        assert self.lib.scn_markov_hash_probs(n, self.p(d_ptr), self.p(d_nodes), t.K, int(backoff), min_count, *self.graph(), *t.args(),
                                              self.p(probs), self.p(used), self.p(err), self.stream()) == 0
        torch.cuda.synchronize()
        return probs.cpu().numpy(), used.cpu().numpy(), int(err.item())

    def h_path_scores(self, t, ptr, nodes, backoff, min_count, alpha):
        T = len(nodes)
        d_ptr, d_nodes, err = self.up(ptr), self.up(nodes), self.word()
        prob = torch.full((T,), -7.0, dtype=torch.float64, device="cuda")
        rank, total, used = (torch.full((T,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
        assert self.lib.scn_markov_hash_path_scores(len(ptr) - 1, self.p(d_ptr), self.p(d_nodes), t.K, int(backoff), min_count,
                                                    ctypes.c_double(alpha), *self.graph(), *t.args(), self.p(prob), self.p(rank),
                                                    self.p(total), self.p(used), self.p(err), self.stream()) == 0
        torch.cuda.synchronize()
        return prob.cpu().numpy(), rank.cpu().numpy(), total.cpu().numpy(), used.cpu().numpy(), int(err.item())


def same_all(got, want):
    return all((same_bits(a, b) if isinstance(b, np.ndarray) else a == b) for a, b in zip(got, want))


def check_readers(dev, t, table, prefixes, targets, paths, backoff, min_count, hops=(1, 3), seed=5, alpha=1.0):
    """Rollout, 2-target, probs and path scores of a built table against the restatement on the dictionary `table`."""
    nbr, deg, K = dev.nbr_h, dev.deg_h, t.K
    pptr, pnodes = ragged(prefixes)
    for h in hops:
        want = ref_backoff_rollout(pptr, pnodes, K, backoff, min_count, h, seed, nbr, deg, table)
        assert same_all(dev.h_rollout(t, pptr, pnodes, backoff, min_count, h, seed), want[:4])
    if targets is not None:
        want = ref_backoff_two_target(pptr, pnodes, K, backoff, min_count, seed, targets, nbr, deg, table)
        assert same_all(dev.h_two_target(t, pptr, pnodes, backoff, min_count, seed, targets), want)
    assert same_all(dev.h_probs(t, pptr, pnodes, backoff, min_count), ref_backoff_probs(pptr, pnodes, K, backoff, min_count, nbr, deg, table))
    ptr, nodes = ragged(paths)
    for a in (0.0, alpha):
        want = ref_backoff_path_scores(ptr, nodes, K, backoff, min_count, a, nbr, deg, table)
        assert same_all(dev.h_path_scores(t, ptr, nodes, backoff, min_count, a), want)


def built(dev, walks, K, capacity=None):
    """The table of the walks on the device, equal to the restatement's, and that dictionary."""
    want, werr = ref_backoff_train(*ragged(walks), K, dev.nbr_h, dev.deg_h)
    t = dev.build(walks, K, capacity)
    assert t.status == [0, 0, 0] and t.err == werr and t.overflow == INT32_MAX and t.intact()
    assert t.per_order == n_states(want, K) and t.n == len(want) and same_table(t.as_dict(), want)
    return t, want


# ------------------------------------------------------------------------------------------------------------------
# without back-off: the direct-addressed kernels, bit for bit
# ------------------------------------------------------------------------------------------------------------------

TINY_PREFIXES = [[0, 1], [1], [], [3, 0], [0, 1, 2], [2, 3, 0, 1], [1, 2, 0, 3, 2], [3, 2, 1, 0]]


@pytest.mark.parametrize("name,order", [("tiny4", k) for k in (1, 2, 3, 4)] + [("cfg1", k) for k in (1, 2, 3)])
def test_without_backoff_it_is_the_direct_table_bit_for_bit(name, order):
    from scone_gcn_amd.markov_model import HASH_KEY_SHIFT, Markov_Backoff, Markov_Model
    if name == "tiny4":
        (nbr, deg), walks, prefixes, paths = tiny4(), TINY_WALKS, TINY_PREFIXES, TINY_WALKS + TINY_PREFIXES
    else:
        d = cfg1_backoff()
        nbr, deg, walks, paths = d["nbr"], d["deg"], d["train_walks"], d["test_walks"]
        prefixes = d["prefixes"][::3] + [p[:k] for p in d["prefixes"][:30] for k in (0, 1, 2, 3)]
    direct, hashed = Markov_Model(order, seed=9), Markov_Backoff(order, seed=9, backoff=False)
    direct.train(nbr, walks)
    hashed.train(nbr, walks)
    # the counts, gathered through row_of: every visited state of the direct table has its row, and no other key has the order
    keys = hashed.keys.cpu().numpy().view(np.uint64)
    at = np.flatnonzero((keys != np.uint64(2 ** 64 - 1)) & ((keys >> np.uint64(HASH_KEY_SHIFT)) == np.uint64(order - 1)))
    states = (keys[at] & np.uint64((1 << HASH_KEY_SHIFT) - 1)).astype(np.int64)
    table = direct.counts.cpu().numpy()
    assert sorted(states.tolist()) == np.flatnonzero(table.sum(axis=1)).tolist() and hashed.n_states[order - 1] == len(states)
    assert same_bits(hashed.counts.cpu().numpy()[hashed.row_of.cpu().numpy()[at]], table[states])
    # the readers
    assert same_bits(hashed.next_node_probs(prefixes), direct.next_node_probs(prefixes))
    assert set(hashed.used_orders.tolist()) <= {0, order}
    for hops in (1, 3):
        got, want = hashed.predict_paths(prefixes, hops), direct.predict_paths(prefixes, hops)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    full = [p for p in prefixes if len(p) >= order and deg[p[-1]] > 1]
    targets = [int(nbr[p[-1], (3 * i) % deg[p[-1]]]) for i, p in enumerate(full)]
    got, want = hashed.two_target_scores(full, targets), direct.two_target_scores(full, targets)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert hashed.test(prefixes[:2], [1, 1], 2) == direct.test(prefixes[:2], [1, 1], 2)        # the short prefix's own last node
    for alpha in (0.0, 1.0):
        for min_prefix in (1, 2):
            got, want = hashed.path_step_log_probs(paths, min_prefix, alpha), direct.path_step_log_probs(paths, min_prefix, alpha)
            assert all(same_bits(np.asarray(a), np.asarray(b)) for a, b in zip(got, want))
            assert np.array_equal(hashed.path_totals, direct.path_totals)
            assert np.array_equal(hashed.used_orders > 0, direct.path_totals > 0)
        assert hashed.score_paths(paths, alpha=alpha)["n_unseen"] == direct.score_paths(paths, alpha=alpha)["n_unseen"]
    if order > 1:
        with pytest.raises(KeyError):
            hashed.predict(prefixes[0][:order - 1])


# ------------------------------------------------------------------------------------------------------------------
# back-off on cfg1
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", (2, 4, 8))
def test_backoff_on_cfg1_against_the_restatement(K):
    from scone_gcn_amd.markov_model import Markov_Backoff
    d = cfg1_backoff()
    nbr, deg = d["nbr"], d["deg"]
    dev = HDev(nbr, deg)
    t, want = built(dev, d["train_walks"], K)
    assert t.per_order == [307, 646, 945, 1270, 1612, 1878, 1995, 1947][:K]
    rows = np.flatnonzero(d["test"])
    prefixes = d["test_prefixes"] + [p[:k] for p in d["prefixes"][:12] for k in range(0, K + 1)]
    for min_count in (1, 2):
        targets = [int(d["t1"][i]) for i in rows] + [int(nbr[p[-1], 0]) if p else 0 for p in prefixes[200:]]
        check_readers(dev, t, want, prefixes, targets, d["test_walks"], True, min_count)
        # the class: the same table and the same numbers through the public calls
        mb = Markov_Backoff(K, seed=5, min_count=min_count)
        mb.train(nbr, d["train_walks"])
        assert mb.n_states == t.per_order and mb.capacity == 1 << int(2 * sum(key_bound(ragged(d["train_walks"])[0], K)) - 1).bit_length()
        assert mb.table_bytes == 12 * mb.capacity + 4 * 13 * sum(mb.n_states)
        pptr, pnodes = ragged(d["test_prefixes"])
        probs, used, _ = ref_backoff_probs(pptr, pnodes, K, True, min_count, nbr, deg, want)
        assert same_bits(mb.next_node_probs(d["test_prefixes"]), probs) and np.array_equal(mb.used_orders, used)
        pred, tied, used, _, ties = ref_backoff_rollout(pptr, pnodes, K, True, min_count, 2, 5, nbr, deg, want)
        got = mb.predict_paths(d["test_prefixes"], 2)
        assert np.array_equal(got[0], pred) and np.array_equal(got[1], tied) and np.array_equal(mb.used_orders, used)
        for (i, h), nodes in ties.items():                           # every rollout lies in the restatement's tied set
            assert got[0][i, h] in nodes
        assert mb.test(d["test_prefixes"], d["t2"][rows], 2) == np.average(d["t2"][rows] == pred[:, 1])
        assert mb.n_rand_choices == int((tied > 1).sum())
        ptr, nodes = ragged(d["test_walks"])
        prob, rank, total, used, _ = ref_backoff_path_scores(ptr, nodes, K, True, min_count, 1.0, nbr, deg, want)
        sc = mb.path_step_log_probs(d["test_walks"], 2, 1.0)
        ppl, at = perplexity(prob, ptr)
        assert same_bits(sc.logp, np.log(prob[at])) and np.array_equal(sc.rank, rank[at]) and np.array_equal(mb.used_orders, used[at])
        assert np.array_equal(mb.path_totals, total[at]) and not np.isinf(sc.mass).any()
        res = mb.score_paths(d["paths"], d["test"].astype(np.int64), alpha=1.0)
        assert res["order_hist"] == np.bincount(used[at], minlength=K + 1).tolist() and res["n_unseen"] == res["order_hist"][0]
        assert res["n_steps"] == 1899 == sum(res["order_hist"]) and abs(res["perplexity"] - ppl) <= 1e-12 * ppl
        # single prefixes: a node from any non-empty prefix, the counts of the chosen row
        for i in (0, 1, 2):
            p = d["test_prefixes"][i]
            for pre in (p, p[-1:], p[-2:]):
                k_probs, k_used, _ = ref_backoff_probs(*ragged([pre]), K, True, min_count, nbr, deg, want)
                node, _ = mb.predict(pre)
                assert node in nbr[pre[-1], :deg[pre[-1]]]
                w = mb.weights_of(pre)
                assert list(w.values()) == k_probs[0, :deg[pre[-1]]].tolist()
                c = mb.counts_of(pre)
                assert list(c) == list(w) and (sum(c.values()) >= min_count) == bool(k_used[0])
                assert [v / max(sum(c.values()), 1) for v in c.values()] == list(w.values())
        with pytest.raises(KeyError):
            mb.predict([])


# ------------------------------------------------------------------------------------------------------------------
# probing at its limits
# ------------------------------------------------------------------------------------------------------------------

def ring_walks():
    """A ring of 300 nodes, a walk of 120 nodes along it, a part of it again and a turn: at K = 2, 119 + 119 = 238 distinct keys,
    0.93 of 256 slots."""
    nbr, deg = table_from_edges(300, [(i, (i + 1) % 300) for i in range(300)])
    return nbr, deg, [list(range(120)), list(range(40, 60)), [5, 4, 5, 6]]


def test_a_table_at_load_above_nine_tenths_wraps_and_answers_as_the_roomy_one():
    from scone_gcn_amd.markov_model import hash_mix
    nbr, deg, walks = ring_walks()
    dev = HDev(nbr, deg)
    roomy, want = built(dev, walks, 2, 1024)
    assert len(want) == 238 >= 0.9 * 256
    tight, _ = built(dev, walks, 2, 256)                             # the next power of two above the number of distinct keys
    at, keys, _ = tight.slots()
    home = np.asarray([hash_mix(k) & 255 for k in keys])
    assert (home > at).any()                                         # a chain that ran past slot 255 and went on from slot 0
    assert ((at - home) & 255).max() >= 8                            # and chains of some length
    prefixes = [list(range(a, b)) for a, b in ((0, 5), (100, 120), (50, 51), (118, 120), (119, 121), (200, 204))] + [[5, 4, 5], [7, 6]]
    targets = [int(nbr[p[-1], 0]) for p in prefixes]
    for t in (roomy, tight):
        check_readers(dev, t, want, prefixes, targets, walks + prefixes, True, 1)
        check_readers(dev, t, want, prefixes, targets, walks + prefixes, False, 1)


def test_a_capacity_below_the_number_of_keys_sets_the_overflow_word_and_writes_nothing_outside():
    from scone_gcn_amd.markov_model import Markov_Backoff
    nbr, deg, walks = ring_walks()
    dev = HDev(nbr, deg)
    want, _ = ref_backoff_train(*ragged(walks), 2, nbr, deg)
    t = dev.build(walks, 2, 128)                                     # 238 keys for 128 slots: every probe loop ends at 128 slots
    assert t.status == [0, 0, 0] and t.overflow == 0 and t.err == INT32_MAX and t.intact()
    assert t.n == 128 and sum(t.per_order) == 128
    got = t.as_dict()
    assert all(k in want and np.array_equal(got[k], want[k]) for k in got)      # what found a slot is counted in full
    ptr, nodes = ragged([[0, 1, 2], [100, 101]])
    probs, used, err = dev.h_probs(t, ptr, nodes, True, 1)           # a full table still answers from a bounded loop
    assert err == INT32_MAX and set(used.tolist()) <= {0, 1, 2} and t.intact()
    mb = Markov_Backoff(2)
    with pytest.raises(RuntimeError, match="full"):
        mb.train(nbr, walks, capacity=128)
    assert mb.counts is None and mb.keys is None
    with pytest.raises(RuntimeError, match="train"):
        mb.predict_paths([[0, 1]], 1)
    mb.train(nbr, walks, capacity=256)
    assert sum(mb.n_states) == len(want) and mb.capacity == 256


def test_memory_error_before_any_launch(monkeypatch):
    from scone_gcn_amd.markov_model import Markov_Backoff
    mb = Markov_Backoff(2)
    monkeypatch.setattr(mb, "_free_bytes", lambda: 100)
    monkeypatch.setattr(mb, "_build", lambda *a: pytest.fail("a launch"))
    with pytest.raises(MemoryError, match=r"need \d+ bytes; 100 are free"):
        mb.train(tiny4()[0], TINY_WALKS)


def test_one_key_many_writers():
    """4096 copies of one 12-node walk at K = 8: every key in exactly one slot, every count exactly 4096."""
    d = cfg1_markov()
    dev = HDev(d["nbr"], d["deg"])
    walk = max(d["paths"], key=len)[:12]
    single, want = built(dev, [walk], 8)
    many = dev.build([walk] * 4096, 8, 1024)
    assert many.status == [0, 0, 0] and many.overflow == many.err == INT32_MAX and many.intact()
    assert many.n == single.n == len(want) and many.per_order == n_states(want, 8)
    got = many.as_dict()                                             # asserts: no key twice
    assert sorted(got) == sorted(want) and all(np.array_equal(got[k], 4096 * want[k]) for k in want)
    assert sum(int(v.sum()) for v in got.values()) == 4096 * sum(key_bound(ragged([walk])[0], 8))


# ------------------------------------------------------------------------------------------------------------------
# the shapes the direct-table tests single out
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", (1, 2, 3))
def test_neighbourhood_wider_than_a_wave(K):
    nbr, deg, walks, prefixes = star70()
    dev = HDev(nbr, deg)
    t, want = built(dev, walks, K)
    targets = [int(nbr[p[-1], (3 * i) % deg[p[-1]]]) for i, p in enumerate(prefixes)]
    for backoff, min_count in ((True, 1), (True, 2), (False, 1)):
        check_readers(dev, t, want, prefixes, targets, walks + prefixes[::7], backoff, min_count, seed=3)
    ptr, nodes = ragged(prefixes)
    pred, tied, used, _ = dev.h_rollout(t, ptr, nodes, True, 1, 1, 3)
    hub = np.asarray([p[-1] == 0 for p in prefixes])
    assert (tied[hub, 0][used[hub, 0] == 1] == 4).all() and (pred[hub, 0] > 64).any()       # a choice past the 64th lane


@pytest.mark.parametrize("K", (1, 4, 8))
def test_walk_longer_than_one_wave_pass(K):
    """One walk of 200 nodes round a ring (and one that goes round twice and turns): windows on either side of the 64-window passes."""
    nbr, deg = table_from_edges(200, [(i, (i + 1) % 200) for i in range(200)])
    dev = HDev(nbr, deg)
    round_twice = [i % 200 for i in range(130, 130 + 415)]
    walks = [list(range(200)), round_twice + round_twice[-2::-1][:131]]
    t, want = built(dev, walks, K)
    assert sum(int(v.sum()) for v in want.values()) == sum(key_bound(ragged(walks)[0], K))
    prefixes = [w[:k] for w in walks for k in (1, 2, 3, 8, 9, 64, 65, 199)]
    check_readers(dev, t, want, prefixes, None, walks + [walks[1][::-1]], True, 1, hops=(2,), seed=1)
    check_readers(dev, t, want, prefixes, None, walks, False, 1, hops=(2,), seed=1)


@pytest.mark.parametrize("K", (1, 3, 8))
def test_walks_of_k_and_k_plus_one_nodes_and_prefixes_of_every_length(K):
    d = cfg1_markov()
    dev = HDev(d["nbr"], d["deg"])
    long = [p for p in d["paths"] if len(p) >= 10][:6]
    walks = [long[0][:K], long[1][:K + 1], long[2][:K + 2], long[3][:1], [], long[4]]
    t, want = built(dev, walks, K)
    assert n_states(want, K)[-1] == 1 + 2 + (len(long[4]) - K)      # the walk of K nodes has no window of order K with a node after it
    prefixes = [long[4][:k] for k in range(0, K + 2)] + [long[1][:k] for k in range(1, K + 2)] + [long[5][:k] for k in range(1, K + 1)]
    targets = [int(d["nbr"][p[-1], 0]) if p else 0 for p in prefixes]
    for backoff, min_count in ((True, 1), (True, 2), (False, 1)):
        check_readers(dev, t, want, prefixes, targets, walks + prefixes, backoff, min_count)


def test_degree_one_last_node_in_test_2_target():
    from scone_gcn_amd.markov_model import Markov_Backoff
    nbr, deg = table_from_edges(3, [(0, 1), (1, 2)])
    dev = HDev(nbr, deg)
    t, want = built(dev, [[0, 1, 2, 1, 0]], 2)
    pptr, pnodes = ragged([[1, 0], [0, 1], [0, 1], [1]])
    got = dev.h_two_target(t, pptr, pnodes, True, 1, 0, [1, 2, 1, 0])
    assert same_all(got, ref_backoff_two_target(pptr, pnodes, 2, True, 1, 0, [1, 2, 1, 0], nbr, deg, want))
    assert got[0][0] == 0 and got[1][0] == -1 and got[4] == 2        # one neighbour: nothing to compare; 1 is no neighbour of 1
    mb = Markov_Backoff(2)
    mb.train(nbr, [[0, 1, 2, 1, 0]])
    assert mb.test_2_target([[0, 1], [1]], [2, 0]) == 0.75           # (0, 1) > 2 once and > 0 never; 1 > 0 and 1 > 2 twice each
    assert mb.used_orders.tolist() == [2, 1]
    with pytest.raises(ValueError, match="no second neighbour"):
        mb.test_2_target([[0, 1], [1, 0]], [2, 1])
    with pytest.raises(ValueError, match="shorter"):
        mb.test_2_target([[0, 1], []], [2, 1])


@pytest.mark.parametrize("K", (1, 2, 4))
def test_offending_walks_lower_err_and_insert_nothing_there(K):
    from scone_gcn_amd.markov_model import Markov_Backoff
    nbr, deg = tiny4()
    dev = HDev(nbr, deg)
    good = [[0, 1, 2], [2, 3, 0, 1, 2, 0]]
    for bad, pos in (([0, 1, 3, 2, 0, 1], 1), ([2, 0, 4, 0, 1], 1), ([2, 0, 1, 2, -1], 3), ([0, 2, 3, 0, 2 ** 31 - 1, 0], 3)):
        walks = good + [bad] + good
        t, want = built(dev, walks, K)                               # err equal to the restatement's, and the same keys
        assert t.err == 9 + pos
        ptr, nodes = ragged(walks)
        for backoff in (True, False):                                # the prefix calls: the word is the position in the window read
            for h in (1, 2):
                assert same_all(dev.h_rollout(t, ptr, nodes, backoff, 1, h, 2),
                                ref_backoff_rollout(ptr, nodes, K, backoff, 1, h, 2, nbr, deg, want)[:4])
            assert same_all(dev.h_probs(t, ptr, nodes, backoff, 1), ref_backoff_probs(ptr, nodes, K, backoff, 1, nbr, deg, want))
            assert same_all(dev.h_two_target(t, ptr, nodes, backoff, 1, 2, [0] * 5),
                            ref_backoff_two_target(ptr, nodes, K, backoff, 1, 2, [0] * 5, nbr, deg, want))
            got = dev.h_path_scores(t, ptr, nodes, backoff, 1, 1.0)
            assert same_all(got, ref_backoff_path_scores(ptr, nodes, K, backoff, 1, 1.0, nbr, deg, want)) and got[4] == 9 + pos
    mb = Markov_Backoff(K)
    with pytest.raises(ValueError, match=r"path 2, position 1: \(1, 3\) is not an edge"):
        mb.train(nbr, good + [[0, 1, 3, 2, 0, 1]])
    assert mb.counts is None
    mb.train(nbr, good)
    with pytest.raises(ValueError, match="path 1, position"):
        mb.predict_paths([[0, 1, 2], [9]], 2)
    with pytest.raises(ValueError, match="not a neighbour"):
        mb.test_2_target([[0, 1, 2], [0, 1, 2]], [0, 2])


def test_two_trainings_give_the_same_bytes():
    from scone_gcn_amd.markov_model import Markov_Backoff
    d = cfg1_backoff()
    outs = []
    for _ in range(2):
        mb = Markov_Backoff(8, seed=4)
        mb.train(d["nbr"], d["train_walks"])
        pred, tied = mb.predict_paths(d["test_prefixes"], 3)
        used = mb.used_orders
        sc = mb.path_step_log_probs(d["test_walks"], 1, 0.5)
        score, other = mb.two_target_scores(d["test_prefixes"], d["t1"][d["test"]])
        outs.append([pred, tied, used, mb.next_node_probs(d["test_prefixes"]), score, other, mb.used_orders, mb.path_totals,
                     np.asarray(mb.n_states)] + [np.asarray(a) for a in sc])
    assert all(same_bits(a, b) for a, b in zip(*outs))


# ------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------

def test_train_model_with_the_backoff_flag(tmp_path, monkeypatch, capsys):
    from scone_gcn_amd import dataset_io, scone_trajectory_model as stm, trajectory_experiments as te
    monkeypatch.chdir(tmp_path)
    dataset_io.generate_dataset(400, 1000, folder="bo", holes=True)     # the 400-point data set of cfg1's recipe
    argv = ["prog", "-epochs", "1", "-batch_size", "100", "-data_folder_suffix", "bo", "-describe", "0", "-markov", "1",
            "-markov_backoff", "1", "-markov_order", "3", "-path_likelihood", "1"]
    hp = te.hyperparams(argv)
    stm.reseed(1030)
    net, res = te.train_model(hp)
    assert len(res) == 4 and np.isfinite(res[0])
    results = net.experiment_results
    labels = ["train accs", "test accs", "Reversed test accs", "Mixed train accs", "Mixed test accs", "Middle region train accs",
              "Middle region test accs", "Upper region train accs", "Lower region accs"]
    assert list(results["markov"]) == labels and all(0.0 <= a <= 1.0 for k in labels for a in results["markov"][k])
    got = results["path_likelihood_markov"]
    assert set(got) == {"train", "test"}
    # the restatement on the data set's own rows: the walks prefix + [target 1], the table of the train mask's
    _, _, train_mask, test_mask, _, G, _, _, _, targets_all, prefixes = te.data_setup(hops=(1, 2), folder_suffix="bo", hp=hp)
    from scone_gcn_amd.markov_model import neighbour_table
    nbr, deg = neighbour_table(G)
    paths = [[int(v) for v in p] + [int(t)] for p, t in zip(prefixes, targets_all[0])]
    table, _ = ref_backoff_train(*ragged([paths[i] for i in np.flatnonzero(train_mask == 1)]), 3, nbr, deg)
    for name, mask in (("train", train_mask), ("test", test_mask)):
        ptr, nodes = ragged([paths[i] for i in np.flatnonzero(mask == 1)])
        prob, _, _, used, _ = ref_backoff_path_scores(ptr, nodes, 3, True, 1, 1.0, nbr, deg, table)
        ppl, at = perplexity(prob, ptr)
        r = got[name]
        assert r["order_hist"] == np.bincount(used[at], minlength=4).tolist() and sum(r["order_hist"]) == r["n_steps"] == len(at)
        assert r["n_unseen"] == r["order_hist"][0] and abs(r["perplexity"] - ppl) <= 1e-12 * ppl
        assert r["n_steps"] == results["path_likelihood"][name]["n_steps"]
    assert len(path_items(ptr, 2)) == got["test"]["n_steps"]
    assert "Path likelihood, markov baseline (test)" in capsys.readouterr().out
    net._drop_graphs()
