"""The Markov baseline on the device: every scn_markov_* kernel through the C-ABI against the NumPy restatement of
tests/test_host_markov.py -- every integer equal, probs bitwise -- on the 4-node graph, on cfg1 at orders 1-3, on a star of 70 leaves
(neighbourhoods wider than a wave), on walks longer than one wave pass, under contended atomics, with offending walks and with
unsupported orders; then Markov_Model and the -markov 1 switch of train_model() end to end."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_host_markov import (INT32_MAX, TINY_WALKS, cfg1_counts, cfg1_markov, ragged, ref_count, ref_probs, ref_rollout,
                                    ref_test, ref_two_target, table_from_edges, table_rows, tiny4)

pytestmark = pytest.mark.gpu


class Dev:
    """The graph on the device and the four calls, each returning host arrays and the err word(s)."""

    def __init__(self, nbr, deg):
        from scone_gcn_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.nbr_h, self.deg_h = nbr, deg
        self.V, self.D = nbr.shape
        self.nbr, self.deg = self.up(nbr), self.up(deg)

    @staticmethod
    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    @staticmethod
    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    @staticmethod
    def word():
        return torch.full((1,), INT32_MAX, dtype=torch.int32, device="cuda")

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def graph(self):
        return self.V, self.D, self.p(self.nbr), self.p(self.deg)

    def count(self, ptr, nodes, order, counts=None, status=0):
        rows = table_rows(self.V, self.D, order)
        if counts is None:
            counts = torch.zeros((rows, self.D), dtype=torch.int32, device="cuda")
        d_ptr, d_nodes, err = self.up(ptr), self.up(nodes), self.word()
        st = self.lib.scn_markov_count(len(ptr) - 1, self.p(d_ptr), self.p(d_nodes), order, *self.graph(), self.p(counts), self.p(err),
                                       self.stream())
        assert st == status
        torch.cuda.synchronize()
        return counts, int(err.item())

    def rollout(self, ptr, nodes, order, hops, seed, counts):
        n = len(ptr) - 1
        d_ptr, d_nodes, err = self.up(ptr), self.up(nodes), self.word()
        pred = torch.full((n, hops), -7, dtype=torch.int32, device="cuda")
        tied = torch.full((n, hops), -7, dtype=torch.int32, device="cuda")
        assert self.lib.scn_markov_rollout(n, self.p(d_ptr), self.p(d_nodes), order, hops, ctypes.c_uint64(seed), *self.graph(),
                                           self.p(counts), self.p(pred), self.p(tied), self.p(err), self.stream()) == 0
        torch.cuda.synchronize()
        return pred.cpu().numpy(), tied.cpu().numpy(), int(err.item())

    def two_target(self, ptr, nodes, order, seed, target, counts):
        n = len(ptr) - 1
        d_ptr, d_nodes, err, err_t = self.up(ptr), self.up(nodes), self.word(), self.word()
        d_t = self.up(np.asarray(target, np.int32))
        score = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        other = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        assert self.lib.scn_markov_two_target(n, self.p(d_ptr), self.p(d_nodes), order, ctypes.c_uint64(seed), self.p(d_t), *self.graph(),
                                              self.p(counts), self.p(score), self.p(other), self.p(err), self.p(err_t),
                                              self.stream()) == 0
        torch.cuda.synchronize()
        return score.cpu().numpy(), other.cpu().numpy(), int(err.item()), int(err_t.item())

    def probs(self, ptr, nodes, order, counts):
        n = len(ptr) - 1
        d_ptr, d_nodes, err = self.up(ptr), self.up(nodes), self.word()
        probs = torch.full((n, self.D), -7.0, dtype=torch.float64, device="cuda")
        assert self.lib.scn_markov_probs(n, self.p(d_ptr), self.p(d_nodes), order, *self.graph(), self.p(counts), self.p(probs),
                                         self.p(err), self.stream()) == 0
        torch.cuda.synchronize()
        return probs.cpu().numpy(), int(err.item())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_all(dev, walks, prefixes, targets, order, hops, seed):
    """Table, rollout, 2-target and probs of one case against the restatement; returns the device's table."""
    nbr, deg = dev.nbr_h, dev.deg_h
    ptr, nodes = ragged(walks)
    want, werr = ref_count(ptr, nodes, order, nbr, deg)
    counts, err = dev.count(ptr, nodes, order)
    assert err == werr and same_bits(counts.cpu().numpy(), want)
    pptr, pnodes = ragged(prefixes)
    for h in hops:
        got, want_r = dev.rollout(pptr, pnodes, order, h, seed, counts), ref_rollout(pptr, pnodes, order, h, seed, nbr, deg, want)
        assert same_bits(got[0], want_r[0]) and same_bits(got[1], want_r[1]) and got[2] == want_r[2]
    if targets is not None:
        got, want_t = dev.two_target(pptr, pnodes, order, seed, targets, counts), ref_two_target(pptr, pnodes, order, seed, targets,
                                                                                                  nbr, deg, want)
        assert same_bits(got[0], want_t[0]) and same_bits(got[1], want_t[1]) and got[2:] == want_t[2:]
    got, want_p = dev.probs(pptr, pnodes, order, counts), ref_probs(pptr, pnodes, order, nbr, deg, want)
    assert same_bits(got[0], want_p[0]) and got[1] == want_p[1]
    return counts


@pytest.mark.parametrize("order", (1, 2, 3, 4))
def test_tiny4_hand_written_walks(order):
    """Walks with len <= order among them; prefixes shorter than the order, empty, and on unseen states."""
    dev = Dev(*tiny4())
    prefixes = [[0, 1], [1], [], [3, 0], [0, 1, 2], [2, 3, 0, 1], [1, 2, 0, 3, 2], [3, 2, 1, 0]]
    targets = [2, 0, 0, 1, 3, 0, 1, 2]                           # neighbours of the last node (row 2 has none: it is short at any order)
    counts = check_all(dev, TINY_WALKS, prefixes, targets, order, (1, 2, 3), 11)
    if order == 1:
        assert counts.cpu().numpy().tolist() == [[1, 1, 1], [1, 2, 0], [2, 1, 1], [1, 1, 0]]


@pytest.mark.parametrize("order", (1, 2, 3))
def test_cfg1_against_the_restatement(order):
    d = cfg1_markov()
    dev = Dev(d["nbr"], d["deg"])
    train = [d["paths"][i] for i in np.flatnonzero(d["train"])]
    counts = check_all(dev, train, d["prefixes"], d["t1"], order, (1, 2), 0)
    assert same_bits(counts.cpu().numpy(), cfg1_counts(order))   # the table the fixture of the reference's weights was checked on
    assert counts.shape == ((400, 5200, 67600)[order - 1], 13)


def star70():
    """A hub (node 0) with 70 leaves and a ring through the leaves: D = 70 > 64 lanes at the hub (leaf l in slot l - 1), 3 at a leaf.
    At order 1 the hub's row has four tied maxima in slots 10, 63, 64 and 69; at order 2 the states (1, 0), (2, 0), (3, 0) tie those
    four, (4, 0) has its one maximum in slot 67 and every other (leaf, 0) was never seen: all 70 slots tie."""
    edges = [(0, i) for i in range(1, 71)] + [(i, i % 70 + 1) for i in range(1, 71)]
    nbr, deg = table_from_edges(71, edges)
    assert nbr.shape == (71, 70) and deg[0] == 70 and (deg[1:] == 3).all() and nbr[0].tolist() == list(range(1, 71))
    walks = [[l, 0, x] for x in (11, 64, 65, 70) for l in (1, 2, 3)] + [[4, 0, 68], [4, 0, 68], [4, 0, 5]]
    walks += [[5, 6, 7, 8, 9, 10], [10, 9, 8, 7, 6], [0], [70, 1]]
    prefixes = [[l, 0] for l in range(1, 71)] + [[0, l] for l in range(1, 71)] + [[0], [5]] + [[l, l % 70 + 1, 0] for l in range(1, 71)]
    return nbr, deg, walks, prefixes


@pytest.mark.parametrize("order", (1, 2))
def test_neighbourhood_wider_than_a_wave(order):
    nbr, deg, walks, prefixes = star70()
    dev = Dev(nbr, deg)
    targets = [int(nbr[p[-1], (3 * i) % deg[p[-1]]]) for i, p in enumerate(prefixes)]
    counts = check_all(dev, walks, prefixes, targets, order, (1, 3), 3)
    assert counts.shape == ((71, 71 * 70)[order - 1], 70)
    ptr, nodes = ragged(prefixes)
    pred, tied, _ = dev.rollout(ptr, nodes, order, 1, 3, counts)
    hub = np.asarray([p[-1] == 0 and len(p) >= order for p in prefixes])
    if order == 1:
        assert (tied[hub, 0] == 4).all() and set(pred[hub, 0].tolist()) == {11, 64, 65, 70}
    else:
        assert set(tied[hub, 0].tolist()) == {1, 4, 70} and (pred[hub, 0][tied[hub, 0] == 1] == 68).all()
        assert (pred[hub, 0][tied[hub, 0] == 70] > 64).any()    # a choice among all 70 lands past the 64th lane


@pytest.mark.parametrize("order", (1, 2, 3, 4))
def test_walk_longer_than_one_wave_pass(order):
    """One walk of 200 nodes round a ring (and one that goes round twice and turns): more windows than the 64 of one pass."""
    nbr, deg = table_from_edges(200, [(i, (i + 1) % 200) for i in range(200)])
    dev = Dev(nbr, deg)
    round_twice = [i % 200 for i in range(130, 130 + 415)]
    walks = [list(range(200)), round_twice + round_twice[-2::-1][:131]]
    counts = check_all(dev, walks, [w[:k] for w in walks for k in (1, 2, 3, 64, 65, 199)], None, order, (2,), 1)
    assert int(counts.sum()) == sum(len(w) - order for w in walks)


def test_contended_atomics_count_exactly():
    d = cfg1_markov()
    dev = Dev(d["nbr"], d["deg"])
    walk = max(d["paths"], key=len)
    for order in (1, 2):
        single, err = dev.count(*ragged([walk]), order)
        many, err2 = dev.count(*ragged([walk] * 4096), order)
        assert err == err2 == INT32_MAX and int(single.sum()) == len(walk) - order
        assert torch.equal(many, single * 4096)
        again, _ = dev.count(*ragged([walk] * 4096), order, counts=many.clone())      # it accumulates
        assert torch.equal(again, single * 8192)


@pytest.mark.parametrize("order", (1, 2, 3))
def test_offending_walks_lower_err_and_count_nothing_there(order):
    nbr, deg = tiny4()
    dev = Dev(nbr, deg)
    good = [[0, 1, 2], [2, 3, 0, 1, 2, 0]]
    for bad, pos in (([0, 1, 3, 2, 0, 1], 1), ([2, 0, 4, 0, 1], 1), ([2, 0, 1, 2, -1], 3), ([0, 2, 3, 0, 2 ** 31 - 1, 0], 3)):
        walks = good + [bad] + good
        ptr, nodes = ragged(walks)
        want, werr = ref_count(ptr, nodes, order, nbr, deg)
        counts, err = dev.count(ptr, nodes, order)
        assert err == werr == 9 + pos and same_bits(counts.cpu().numpy(), want)
        # the prefix calls: the word is the position in the window that is read, rows beside it are served
        for h in (1, 2):
            got, want_r = dev.rollout(ptr, nodes, order, h, 2, counts), ref_rollout(ptr, nodes, order, h, 2, nbr, deg, want)
            assert same_bits(got[0], want_r[0]) and same_bits(got[1], want_r[1]) and got[2] == want_r[2]
        got, want_p = dev.probs(ptr, nodes, order, counts), ref_probs(ptr, nodes, order, nbr, deg, want)
        assert same_bits(got[0], want_p[0]) and got[1] == want_p[1]
        targets = [0, 0, 0, 0, 0]
        got, want_t = dev.two_target(ptr, nodes, order, 2, targets, counts), ref_two_target(ptr, nodes, order, 2, targets, nbr, deg, want)
        assert same_bits(got[0], want_t[0]) and same_bits(got[1], want_t[1]) and got[2:] == want_t[2:]
    from scone_gcn_amd.markov_model import Markov_Model
    mm = Markov_Model(order)
    with pytest.raises(ValueError, match=r"path 2, position 1: \(1, 3\) is not an edge"):
        mm.train(nbr, good + [[0, 1, 3, 2, 0, 1]])
    assert mm.counts is None
    with pytest.raises(ValueError, match=r"path 1, position 1: \(0, 4\) is not an edge"):
        mm.train(nbr, (np.array([0, 3, 8]), np.array([0, 1, 2, 2, 0, 4, 0, 1])))
    mm.train(nbr, good)
    with pytest.raises(ValueError, match="path 1, position"):
        mm.predict_paths([[0, 1, 2], [1, 2, 9][-max(order, 2):] if order > 1 else [9]], 2)
    with pytest.raises(ValueError, match="not a neighbour"):
        mm.test_2_target([[0, 1, 2], [0, 1, 2]], [0, 2])


def test_unsupported_orders_launch_nothing_and_empty_calls_succeed():
    from scone_gcn_amd import _lib
    dev = Dev(*tiny4())
    ptr, nodes = ragged(TINY_WALKS)
    counts = torch.full((4 * 27, 3), 5, dtype=torch.int32, device="cuda")
    _, err = dev.count(ptr, nodes, 5, counts=counts, status=_lib.SCN_ERR_UNSUPPORTED)
    assert err == INT32_MAX and bool((counts == 5).all())
    wide_nbr, wide_deg = table_from_edges(1300, [(0, i) for i in range(1, 1300)])
    wide = Dev(wide_nbr, wide_deg)
    assert table_rows(1300, 1299, 3) is None                     # 1300 * 1299^3 entries
    one = torch.full((1, 1299), 5, dtype=torch.int32, device="cuda")
    d_ptr, d_nodes, word = wide.up(ptr), wide.up(nodes), wide.word()
    assert wide.lib.scn_markov_count(len(ptr) - 1, wide.p(d_ptr), wide.p(d_nodes), 3, *wide.graph(), wide.p(one), wide.p(word),
                                     wide.stream()) == _lib.SCN_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert int(word.item()) == INT32_MAX and bool((one == 5).all())
    # n = 0
    e_ptr, e_nodes = np.zeros(1, np.int32), np.zeros(0, np.int32)
    c, err = dev.count(e_ptr, e_nodes, 2)
    assert err == INT32_MAX and not bool(c.any())
    assert dev.rollout(e_ptr, e_nodes, 2, 2, 0, c)[0].shape == (0, 2)
    assert dev.two_target(e_ptr, e_nodes, 2, 0, [], c)[0].shape == (0,)
    assert dev.probs(e_ptr, e_nodes, 2, c)[0].shape == (0, 3)
    from scone_gcn_amd.markov_model import Markov_Model
    with pytest.raises(ValueError, match="2\\^31"):
        Markov_Model(3).train(wide_nbr, [[0, 1]])


# ------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", (1, 2, 3))
def test_markov_model_accuracies_equal_the_restatement(order):
    from scone_gcn_amd.markov_model import Markov_Model
    d = cfg1_markov()
    nbr, deg, counts = d["nbr"], d["deg"], cfg1_counts(order)
    rows = np.flatnonzero(d["test"])
    pre, t1, t2 = [d["prefixes"][i] for i in rows], d["t1"][rows], d["t2"][rows]
    ptr, nodes = ragged(pre)
    import networkx as nx
    G = nx.Graph()
    G.add_nodes_from(range(400))
    G.add_edges_from(np.load(cfg1_complex_path())["edges"].tolist())
    for seed, graph in ((0, nbr), (20261019, G)):
        mm = Markov_Model(order, seed=seed)
        mm.train(graph, [d["paths"][i] for i in np.flatnonzero(d["train"])])
        assert same_bits(mm.counts.cpu().numpy(), counts)
        for hops, target in ((1, t1), (2, t2)):
            pred, tied, _ = ref_rollout(ptr, nodes, order, hops, seed, nbr, deg, counts)
            assert mm.test(pre, target, hops) == ref_test(pred, ptr, nodes, order, target)
            assert mm.n_rand_choices == int((tied > 1).sum())
        score, other, _, _ = ref_two_target(ptr, nodes, order, seed, t1, nbr, deg, counts)
        assert mm.test_2_target(pre, t1) == float(score.astype(np.float64).sum()) / len(score)
        paths, n_tied = mm.predict_paths(pre, 2)
        assert np.array_equal(paths, pred) and np.array_equal(n_tied, tied)
        # the reference's single-prefix calls: row 0 of a batch of one
        node, was_random = mm.predict(pre[0][-order:])
        one = ref_rollout(*ragged([pre[0]]), order, 1, seed, nbr, deg, counts)
        assert node == one[0][0, 0] and was_random == (one[1][0, 0] > 1)
        want_p, _ = ref_probs(ptr, nodes, order, nbr, deg, counts)
        assert same_bits(mm.next_node_probs(pre), want_p)
        w = mm.weights_of(pre[3])
        v = pre[3][-1]
        assert list(w) == nbr[v, :deg[v]].tolist() and list(w.values()) == want_p[3, :deg[v]].tolist()
    short = Markov_Model(order)
    short.train(nbr, [d["paths"][0]])
    assert short.test([pre[0][:order - 1] + [] if order > 1 else pre[0][:1]], [pre[0][order - 2] if order > 1 else -5], 2) == \
        (1.0 if order > 1 else 0.0)                              # MM:92: a short prefix is compared by its own last node
    with pytest.raises(KeyError):
        short.predict(pre[0][:order - 1])


def cfg1_complex_path():
    import os
    from tests.test_host_markov import GOLDEN
    return os.path.join(GOLDEN, "cfg1_complex.npz")


def test_degree_one_last_node_raises_in_test_2_target():
    from scone_gcn_amd.markov_model import Markov_Model
    nbr, _ = table_from_edges(3, [(0, 1), (1, 2)])
    mm = Markov_Model(1)
    mm.train(nbr, [[0, 1, 2, 1, 0]])
    assert mm.test_2_target([[0, 1]], [2]) == 0.5
    with pytest.raises(ValueError, match="no second neighbour"):
        mm.test_2_target([[0, 1], [1, 0]], [2, 1])


def test_train_model_markov_switch(tmp_path, monkeypatch, capsys):
    from scone_gcn_amd import dataset_io, scone_trajectory_model as stm, trajectory_experiments as te
    monkeypatch.chdir(tmp_path)
    dataset_io.generate_dataset(150, 90, folder="drv", holes=True)      # 18 test rows: every third of them is never empty in practice
    argv = ["prog", "-epochs", "1", "-batch_size", "12", "-data_folder_suffix", "drv", "-describe", "0", "-markov", "1",
            "-markov_order", "2"]
    hp = te.hyperparams(argv)
    hp["hidden_layers"] = [(3, 16)] * 3
    stm.reseed(1030)
    net, res = te.train_model(hp)                                # the reference raises after the block (TE:433); training follows here
    assert len(res) == 4 and np.isfinite(res[0])
    got = net.experiment_results["markov"]
    labels = ["train accs", "test accs", "Reversed test accs", "Mixed train accs", "Mixed test accs", "Middle region train accs",
              "Middle region test accs", "Upper region train accs", "Lower region accs"]
    assert list(got) == labels
    assert [len(got[k]) for k in labels] == [3, 3] + [2] * 7 and all(0.0 <= a <= 1.0 for k in labels for a in got[k])
    out = capsys.readouterr().out
    assert [l for l in out.splitlines() if l in labels] == labels
    # the forward experiment is the class on the data set's own rows
    inputs_all, y_all, train_mask, test_mask, shifts, G, E_lookup, nbrhoods, n_nbrs, targets_all, prefixes = \
        te.data_setup(hops=(1, 2), folder_suffix="drv", hp=hp)
    from scone_gcn_amd.markov_model import Markov_Model
    mm = Markov_Model(2)
    paths = [list(p) + [int(a), int(b)] for p, a, b in zip(prefixes, targets_all[0], targets_all[1])]
    tr, te_rows = np.flatnonzero(train_mask == 1), np.flatnonzero(test_mask == 1)
    mm.train(G, [paths[i] for i in tr])
    pre = [list(prefixes[i]) for i in te_rows]
    t1, t2 = (np.asarray(t)[te_rows] for t in targets_all[:2])
    assert got["test accs"] == [mm.test(pre, t1, 1), mm.test(pre, t2, 2), mm.test_2_target(pre, t1)]
    net._drop_graphs()                                          # the captured training steps go now, not whenever the collector runs
