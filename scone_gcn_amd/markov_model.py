"""The k-th order Markov next-node baseline (the reference's trajectory_analysis/markov_model.py = MM) on the device.

Same call surface as the reference's Markov_Model -- train(G, paths), predict(prefix), test(prefixes, target_nodes, hops),
test_2_target(prefixes, target_nodes) -- on a direct-addressed integer count table instead of nested dictionaries: a walk of
`order` nodes is the state ((v0 D + slot(v0, v1)) D + ...) of the padded neighbour table (include/scone_hip.h, scn_markov_*),
training is one launch over all walks and a whole multi-hop test is one launch over all prefixes (csrc/scn_markov.hip).
The reference's weights are counts[s][j] / counts[s].sum(): next_node_probs / weights_of return exactly those float64 values.

Where the reference calls np.random.choice -- among tied maxima (MM:71-72) and for the other neighbour of the 2-target test
(MM:104) -- the draw here is the Philox uniform of (seed, row of the prefix in the call, ...), so a result depends on the seed
and the row's position and on nothing else (not the global NumPy stream, not the rest of the batch).  Equal counts are equal
probabilities (one divisor per row), so the tied sets are the reference's.  All math runs in libscone_hip.so; nothing falls
back to the CPU.
"""
import ctypes

import numpy as np
import torch

from . import _lib, ops
from ._lib import SCN_MARKOV_HASH_MAX_ORDER, SCN_MARKOV_MAX_ORDER, check
from .ops import INT32_MAX


def neighbour_table(G):
    """(nbr (V, D) int32, deg (V,) int32) of G: every node's neighbours ascending and left-aligned, -1 behind them.  G is the
    project's UndirGraph, a (V, D) table padded with -1 (sc.nbrhoods), or a networkx-style graph on the nodes 0 .. V-1."""
    if hasattr(G, "complex") and hasattr(G.complex, "nbrhoods"):
        G = G.complex.nbrhoods
    if torch.is_tensor(G):
        G = G.cpu().numpy()
    if isinstance(G, np.ndarray):
        nb = np.asarray(G, np.int64)
        if nb.ndim != 2 or nb.shape[1] < 1:
            raise ValueError("the neighbour table must be (V, D), padded with -1")
        V = nb.shape[0]
        if np.any(nb >= V):
            raise ValueError("the neighbour table names a node outside its %d rows" % V)
        key = np.where(nb >= 0, nb, V)                          # real neighbours ascending, the padding behind them
        nb = np.sort(key, axis=1)
        nb = np.where(nb < V, nb, -1)
    else:
        nodes = sorted(int(v) for v in G.nodes)
        V = len(nodes)
        if V == 0 or nodes[0] != 0 or nodes[-1] != V - 1:
            raise ValueError("the graph's nodes must be the integers 0 .. V-1")
        rows = [sorted(int(u) for u in G[v]) for v in range(V)]
        D = max(1, max(len(r) for r in rows))
        nb = np.full((V, D), -1, np.int64)
        for v, r in enumerate(rows):
            nb[v, :len(r)] = r
    deg = (nb >= 0).sum(axis=1)
    return np.ascontiguousarray(nb, np.int32), np.ascontiguousarray(deg, np.int32)


def ragged(paths):
    """(ptr (n + 1,) int32, nodes int32) of a list of node lists, or of a (ptr, nodes) pair of arrays as it is."""
    if isinstance(paths, tuple) and len(paths) == 2 and all(isinstance(a, np.ndarray) or torch.is_tensor(a) for a in paths):
        ptr, nodes = (np.asarray(a.cpu() if torch.is_tensor(a) else a).astype(np.int64).ravel() for a in paths)
        if len(ptr) < 1 or ptr[0] != 0 or np.any(np.diff(ptr) < 0) or ptr[-1] != len(nodes):
            raise ValueError("ptr must rise from 0 to len(nodes)")
    else:
        lens = [len(p) for p in paths]
        ptr = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.int64)
        nodes = np.fromiter((int(v) for p in paths for v in p), np.int64, int(ptr[-1]))
    if len(nodes) >= INT32_MAX:
        raise ValueError("the paths hold %d nodes; fewer than 2^31 - 1 are served" % len(nodes))
    if len(nodes) and (nodes.min() < -INT32_MAX or nodes.max() > INT32_MAX):
        raise ValueError("a node id does not fit 32 bits")
    return np.ascontiguousarray(ptr, np.int32), np.ascontiguousarray(nodes, np.int32)


def select_paths(paths, mask):
    """The paths with mask == 1 as a (ptr, nodes) pair, in their order (all of them without a mask)."""
    ptr, nodes = ragged(paths)
    if mask is None:
        return ptr, nodes
    rows = np.flatnonzero(np.asarray(mask) == 1)
    lens = np.diff(ptr).astype(np.int64)[rows]
    new_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.repeat(ptr[rows].astype(np.int64) - new_ptr[:-1], lens) + np.arange(int(new_ptr[-1]), dtype=np.int64)
    return np.ascontiguousarray(new_ptr, np.int32), np.ascontiguousarray(nodes[idx])


def table_rows(n_nodes, d, order):
    """Rows of the count table (scn_markov_table_rows); ValueError for an order or a size the library does not serve."""
    if int(order) != order or not 1 <= int(order) <= SCN_MARKOV_MAX_ORDER:
        raise ValueError("order must be an integer in 1 .. %d, got %r" % (SCN_MARKOV_MAX_ORDER, order))
    rows = _lib.load().scn_markov_table_rows(int(n_nodes), int(d), int(order))
    if rows == _lib.SCN_ERR_UNSUPPORTED:
        raise ValueError("the order-%d table of %d nodes x %d slots passes 2^31 - 1 entries" % (order, n_nodes, d))
    if rows < 0:
        raise ValueError("no count table for %d nodes x %d slots" % (n_nodes, d))
    return rows


class Markov_Model:
    def __init__(self, order, seed=0, device=None):
        """
        :param order: number of prior states to consider when making a prediction (1 .. SCN_MARKOV_MAX_ORDER)
        :param seed: key of every random choice (ties, the 2-target test's other neighbour)
        """
        if int(order) != order or not 1 <= int(order) <= SCN_MARKOV_MAX_ORDER:
            raise ValueError("order must be an integer in 1 .. %d, got %r" % (SCN_MARKOV_MAX_ORDER, order))
        self.order, self.seed, self.device = int(order), int(seed), device
        self.counts = None                                      # (rows, D) int32 on the device after train()
        self.n_rand_choices = 0                                 # tied predictions of the last test() (MM:81, 87)
        self.h_nbr = self.h_deg = None

    # ---- plumbing ----
    def _upload(self, a):
        return torch.from_numpy(a).to(self.device)

    def _graph_args(self):
        return self.n_nodes, self.width, ops._dev(self.nbr, torch.int32), ops._dev(self.deg, torch.int32)

    def _err_word(self):
        return torch.full((1,), INT32_MAX, dtype=torch.int32, device=self.device)

    def _raise_bad_pair(self, err, ptr, nodes):
        t = int(err.item())
        if t == INT32_MAX:
            return
        p = int(np.searchsorted(ptr, t, side="right")) - 1
        q = t - int(ptr[p])
        if t + 1 < int(ptr[p + 1]):
            raise ValueError("path %d, position %d: (%d, %d) is not an edge" % (p, q, nodes[t], nodes[t + 1]))
        raise ValueError("path %d, position %d: node %d is outside the graph" % (p, q, nodes[t]))

    def _prefix_args(self, prefixes):
        if self.counts is None:
            raise RuntimeError("train() first")
        ptr, nodes = ragged(prefixes)
        return ptr, nodes, self._upload(ptr), self._upload(nodes)

    def _two_target_args(self, prefixes, target_nodes, shortest):
        """The prefixes and targets of a 2-target call, checked on the host: ValueError for a prefix of fewer than `shortest` nodes
        and for a last node with a single neighbour."""
        ptr, nodes, d_ptr, d_nodes = self._prefix_args(prefixes)
        n = len(ptr) - 1
        target = np.ascontiguousarray([int(t) for t in target_nodes], np.int32)
        if len(target) != n:
            raise ValueError("prefixes and target_nodes disagree on the number of paths")
        lens = np.diff(ptr)
        if np.any(lens < shortest):
            raise ValueError("path %d is shorter than the order %d" % (int(np.flatnonzero(lens < shortest)[0]), shortest))
        last = nodes[ptr[1:] - 1] if n else nodes[:0]
        inside = (last >= 0) & (last < self.n_nodes)
        single = np.flatnonzero(inside & (self.h_deg[np.where(inside, last, 0)] < 2))
        if len(single):
            raise ValueError("path %d ends at node %d, which has no second neighbour to compare the target with"
                             % (int(single[0]), int(last[single[0]])))
        return ptr, nodes, d_ptr, d_nodes, n, target, last

    # ---- the reference's surface ----
    def train(self, G, paths):
        """
        :param G: UndirGraph, networkx graph on 0 .. V-1, or (V, D) neighbour table
        :param paths: paths over G: a list of node lists or a (ptr, nodes) pair
        Builds the count table from scratch (MM:43-51); one upload, one launch.  ValueError for a pair of consecutive nodes that
        is not an edge (the reference: KeyError).
        """
        nbr, deg = neighbour_table(G)
        rows = table_rows(nbr.shape[0], nbr.shape[1], self.order)
        ptr, nodes = ragged(paths)
        if self.device is None:
            self.device = ops.default_device()
        lib = _lib.load()
        self.h_nbr, self.h_deg = nbr, deg
        self.n_nodes, self.width = int(nbr.shape[0]), int(nbr.shape[1])
        self.nbr, self.deg = self._upload(nbr), self._upload(deg)
        d_ptr, d_nodes = self._upload(ptr), self._upload(nodes)
        counts = torch.zeros((rows, self.width), dtype=torch.int32, device=self.device)
        err = self._err_word()
        with torch.cuda.device(self.device):
            check(lib.scn_markov_count(len(ptr) - 1, ops._dev(d_ptr, torch.int32), ops._dev(d_nodes, torch.int32), self.order,
                                       *self._graph_args(), ops._dev(counts, torch.int32), ops._dev(err, torch.int32),
                                       ops._stream()), "scn_markov_count")
        self.counts = None
        self._raise_bad_pair(err, ptr, nodes)
        self.counts = counts

    def predict_paths(self, prefixes, hops):
        """(pred (n, hops) node ids, n_tied (n, hops)) of the greedy rollout of every prefix (MM:58-93): -1 / 0 from the hop on
        at which nothing is predicted (a prefix shorter than `order`, a node without neighbours).  Row i draws from (seed, i)."""
        ptr, nodes, d_ptr, d_nodes = self._prefix_args(prefixes)
        n, hops = len(ptr) - 1, int(hops)
        if hops < 1:
            raise ValueError("hops must be at least 1")
        pred = torch.empty((n, hops), dtype=torch.int32, device=self.device)
        tied = torch.empty((n, hops), dtype=torch.int32, device=self.device)
        err = self._err_word()
        with torch.cuda.device(self.device):
            check(_lib.load().scn_markov_rollout(n, ops._dev(d_ptr, torch.int32), ops._dev(d_nodes, torch.int32), self.order, hops,
                                                 ctypes.c_uint64(self.seed & (2 ** 64 - 1)), *self._graph_args(),
                                                 ops._dev(self.counts, torch.int32), ops._dev(pred, torch.int32),
                                                 ops._dev(tied, torch.int32), ops._dev(err, torch.int32), ops._stream()),
                  "scn_markov_rollout")
        self._raise_bad_pair(err, ptr, nodes)
        return pred.cpu().numpy(), tied.cpu().numpy()

    def predict(self, prefix):
        """
        Predicts which node will be visited next, given that prefix was just visited: (node, was_random), from the last `order`
        nodes of prefix (MM:58-74).  KeyError for a prefix shorter than `order`, as the reference's dictionary raises.
        """
        if len(prefix) < self.order:
            raise KeyError(tuple(prefix))
        pred, tied = self.predict_paths([list(prefix)], 1)
        return (int(pred[0, 0]) if pred[0, 0] >= 0 else None), bool(tied[0, 0] > 1)

    def test(self, prefixes, target_nodes, hops):
        """
        Returns the model's accuracy over the given prefixes and targets: the node of the last hop against the target (MM:76-93).
        A prefix shorter than `order` is never extended, so its own last node is compared (MM:85, 92).
        """
        ptr, _ = ragged(prefixes)
        pred, tied = self.predict_paths(prefixes, hops)
        self.n_rand_choices = int((tied > 1).sum())
        last = pred[:, -1].astype(np.int64)
        lens = np.diff(ptr)
        short = np.flatnonzero(lens < self.order)
        if len(short):
            if np.any(lens[short] == 0):
                raise IndexError("an empty prefix has no last node")
            _, nodes = ragged(prefixes)
            last[short] = nodes[ptr[short + 1] - 1]
        target = np.asarray([int(t) for t in target_nodes], np.int64)
        if len(target) != len(last):
            raise ValueError("prefixes and target_nodes disagree on the number of paths")
        return np.average(target == last)

    def test_2_target(self, prefixes, target_nodes):
        """
        Returns 2-target accuracy of model (MM:95-112): the target against one other neighbour of the last node, drawn from
        (seed, row).  ValueError for a last node with a single neighbour (np.random.choice([]) raises in the reference too),
        for a target that is not a neighbour and for a prefix shorter than `order`.
        """
        score, _ = self.two_target_scores(prefixes, target_nodes)
        return float(score.sum()) / len(score)

    # ---- beyond the reference ----
    def two_target_scores(self, prefixes, target_nodes):
        """(score (n,) of 1 / 0.5 / 0, other (n,) node ids) behind test_2_target."""
        ptr, nodes, d_ptr, d_nodes, n, target, last = self._two_target_args(prefixes, target_nodes, self.order)
        score = torch.empty((n,), dtype=torch.float32, device=self.device)
        other = torch.empty((n,), dtype=torch.int32, device=self.device)
        d_target = self._upload(target)
        err, err_t = self._err_word(), self._err_word()
        with torch.cuda.device(self.device):
            check(_lib.load().scn_markov_two_target(n, ops._dev(d_ptr, torch.int32), ops._dev(d_nodes, torch.int32), self.order,
                                                    ctypes.c_uint64(self.seed & (2 ** 64 - 1)), ops._dev(d_target, torch.int32),
                                                    *self._graph_args(), ops._dev(self.counts, torch.int32),
                                                    ops._dev(score, torch.float32), ops._dev(other, torch.int32),
                                                    ops._dev(err, torch.int32), ops._dev(err_t, torch.int32), ops._stream()),
                  "scn_markov_two_target")
        self._raise_bad_pair(err, ptr, nodes)
        i = int(err_t.item())
        if i != INT32_MAX:
            raise ValueError("path %d: target %d is not a neighbour of its last node %d" % (i, target[i], last[i]))
        return score.cpu().numpy().astype(np.float64), other.cpu().numpy()

    def next_node_probs(self, prefixes):
        """(n, D) float64: the reference's weights of every prefix's state by slot of its last node (0 in the padding, for a
        state nobody visited and for a prefix shorter than `order`)."""
        ptr, nodes, d_ptr, d_nodes = self._prefix_args(prefixes)
        n = len(ptr) - 1
        probs = torch.empty((n, self.width), dtype=torch.float64, device=self.device)
        err = self._err_word()
        with torch.cuda.device(self.device):
            check(_lib.load().scn_markov_probs(n, ops._dev(d_ptr, torch.int32), ops._dev(d_nodes, torch.int32), self.order,
                                               *self._graph_args(), ops._dev(self.counts, torch.int32),
                                               ops._dev(probs, torch.float64), ops._dev(err, torch.int32), ops._stream()),
                  "scn_markov_probs")
        self._raise_bad_pair(err, ptr, nodes)
        return probs.cpu().numpy()

    # ---- whole paths: the teacher-forced score of every node (scn_markov_path_scores) ----
    def _path_records(self, ptr, nodes, alpha):
        """(prob float64, rank int32, total int32) [T] of scn_markov_path_scores on the host: the paths go up in one buffer, one
        launch, and the three arrays and the error word come back in one."""
        P, T = len(ptr) - 1, len(nodes)
        if T == 0:
            return np.zeros(0), np.zeros(0, np.int32), np.zeros(0, np.int32)
        up = self._upload(np.concatenate([ptr, nodes]))
        d_ptr, d_nodes = up[:P + 1], up[P + 1:]
        out = torch.empty((4 * T + 1,), dtype=torch.int32, device=self.device)      # prob [T] fp64 | rank [T] | total [T] | err
        out[4 * T:] = INT32_MAX
        prob, rank, total, err = out[:2 * T].view(torch.float64), out[2 * T:3 * T], out[3 * T:4 * T], out[4 * T:]
        with torch.cuda.device(self.device):
            check(_lib.load().scn_markov_path_scores(P, ops._dev(d_ptr, torch.int32), ops._dev(d_nodes, torch.int32), self.order,
                                                     ctypes.c_double(alpha), *self._graph_args(), ops._dev(self.counts, torch.int32),
                                                     ops._dev(prob, torch.float64), ops._dev(rank, torch.int32),
                                                     ops._dev(total, torch.int32), ops._dev(err, torch.int32), ops._stream()),
                  "scn_markov_path_scores")
        host = out.cpu()
        self._raise_bad_pair(host[4 * T:], ptr, nodes)
        host = host.numpy()
        return host[:2 * T].view(np.float64), host[2 * T:3 * T], host[3 * T:4 * T]

    def path_step_log_probs(self, paths, min_prefix=2, alpha=0.0):
        """The teacher-forced scores of every step of every path under the count table, as Scone_GCN.path_step_log_probs gives the
        model's: a path_scores.PathScores over the items (path p, prefix of k = max(min_prefix, 1) .. len - 1 nodes), each predicting
        p[k] from the state of the `order` nodes before it.  The probability is (c_j + alpha) / (total + alpha deg): alpha = 0 is
        the reference's weight (next_node_probs' bits; logp = -inf for a step the table never saw, and for every prefix shorter
        than `order`), alpha > 0 additive smoothing over the real neighbours (an unseen or short state is uniform).  rank counts
        the neighbours with a higher count, or an equal one in a lower slot; mass is 0, or -inf where the state has no
        distribution at all (alpha = 0 and total = 0).  Leaves the items' row totals in self.path_totals.  ValueError for a
        step that is no edge."""
        from . import path_scores
        alpha = float(alpha)
        if not alpha >= 0.0:
            raise ValueError("alpha must be at least 0, got %r" % alpha)
        if self.counts is None:
            raise RuntimeError("train() first")
        ptr, nodes = ragged(paths)
        prob, rank, total = self._path_records(ptr, nodes, alpha)
        item_ptr, item_path, item_len = path_scores.path_items(ptr, min_prefix)
        at = path_scores.item_positions(ptr, item_path, item_len)
        prob, rank, total = prob[at], rank[at].astype(np.int64), total[at].astype(np.int64)
        with np.errstate(divide="ignore"):
            logp = np.log(prob)
        empty = (total == 0) & ((alpha == 0.0) | (self.h_deg[nodes[at - 1]] == 0))
        self.path_totals = total
        return path_scores.PathScores(item_ptr, logp, rank, np.where(empty, -np.inf, 0.0), item_len)

    def path_log_likelihood(self, paths, min_prefix=2, alpha=0.0):
        """(ll [P] float64 = the sum of every path's step log-probabilities, n_steps [P] int64)."""
        from . import path_scores
        sc = self.path_step_log_probs(paths, min_prefix, alpha)
        return path_scores.segment_sums(sc.logp, sc.ptr), np.diff(sc.ptr)

    def score_paths(self, paths, mask=None, min_prefix=2, alpha=0.0):
        """The dict of Scone_GCN.score_paths over the paths with mask == 1 (all without a mask) -- mean_step_logp, perplexity,
        accuracy (rank 0), n_steps -- plus n_unseen: the items whose state was never counted (total == 0)."""
        from . import path_scores
        sc = self.path_step_log_probs(select_paths(paths, mask), min_prefix, alpha)
        return dict(path_scores.summary(sc), n_unseen=int((self.path_totals == 0).sum()))

    def weights_of(self, prefix):
        """The reference's weights[tuple(prefix)]: {neighbour: probability} of the state of the last `order` nodes of prefix."""
        if len(prefix) < self.order:
            raise KeyError(tuple(prefix))
        p = self.next_node_probs([list(prefix)])[0]
        v = int(prefix[-1])
        return {int(self.h_nbr[v, j]): float(p[j]) for j in range(int(self.h_deg[v]))}


# ----------------------------------------------------------------------------------------------
# variable order: every order 1 .. K in one hashed table, read with back-off (csrc/scn_markov_hash.hip)
# ----------------------------------------------------------------------------------------------

HASH_EMPTY = (1 << 64) - 1
HASH_KEY_SHIFT = 59


def hash_mix(x):
    """The table's hash of a key (the finaliser of splitmix64) for a Python int or a uint64 array; a slot is hash_mix(key) &
    (capacity - 1), then linearly on."""
    if isinstance(x, np.ndarray):
        x = x.astype(np.uint64)
        with np.errstate(over="ignore"):
            x = (x ^ (x >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
            x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
            return x ^ (x >> np.uint64(31))
    x = int(x) & HASH_EMPTY
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & HASH_EMPTY
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & HASH_EMPTY
    return x ^ (x >> 31)


def key_bound(ptr, max_order):
    """The most keys the walks can insert: sum over walks and orders k of max(0, len - k)."""
    lens = np.diff(np.asarray(ptr)).astype(np.int64)
    return int(sum(int(np.maximum(lens - k, 0).sum()) for k in range(1, int(max_order) + 1)))


def hash_capacity(bound, load):
    """The next power of two >= bound / load (at least 1)."""
    need = max(1, int(np.ceil(bound / load)))
    return 1 << (need - 1).bit_length()


class Markov_Backoff(Markov_Model):
    """Markov_Model on the count rows of every order 1 .. max_order at once, kept in one hashed table (only the states the training
    walks visit have a row), and read with back-off: a prediction takes the longest context of at most max_order nodes that the
    table holds with a row total >= min_count (the PPM rule of variable-order Markov models), so a prefix of any length >= 1
    predicts and an unseen long state falls back to a shorter one.  The context alone picks the order, so every row is a proper
    distribution.  backoff=False reads the order-max_order rows only and gives Markov_Model(max_order)'s outputs bit for bit (with
    min_count = 1).  After a reading call used_orders holds the order every row / hop / item took (0: none qualified)."""

    def __init__(self, max_order, seed=0, backoff=True, min_count=1, device=None, load=0.5):
        if int(max_order) != max_order or not 1 <= int(max_order) <= SCN_MARKOV_HASH_MAX_ORDER:
            raise ValueError("max_order must be an integer in 1 .. %d, got %r" % (SCN_MARKOV_HASH_MAX_ORDER, max_order))
        if int(min_count) != min_count or int(min_count) < 1:
            raise ValueError("min_count must be an integer >= 1, got %r" % (min_count,))
        if not 0.0 < float(load) <= 1.0:
            raise ValueError("load must lie in (0, 1], got %r" % (load,))
        self.order = self.max_order = int(max_order)
        self.seed, self.device = int(seed), device
        self.backoff, self.min_count, self.load = bool(backoff), int(min_count), float(load)
        self.shortest = 1 if self.backoff else self.max_order     # the shortest prefix that predicts
        self.counts = self.keys = self.row_of = None              # on the device after train()
        self.capacity, self.n_states, self.table_bytes = 0, [], 0
        self.used_orders = None
        self.n_rand_choices = 0
        self.h_nbr = self.h_deg = None

    # ---- plumbing ----
    def _table_args(self):
        return ops._dev(self.keys, torch.int64), ops._dev(self.row_of, torch.int32), self.capacity, ops._dev(self.counts, torch.int32)

    def _rule(self):
        return self.max_order, int(self.backoff), self.min_count

    def _build(self, ptr, nodes, capacity):
        """The three launches on buffers of `capacity` slots; returns the host copy of the words [n_states, err, overflow,
        n_states per order ...] read between the second and the third."""
        lib, K = _lib.load(), self.max_order
        d_ptr, d_nodes = self._upload(ptr), self._upload(nodes)
        words = self._upload(np.array([0, INT32_MAX, INT32_MAX] + [0] * K, np.int32))
        keys = torch.full((capacity,), -1, dtype=torch.int64, device=self.device)      # all-ones: the empty key
        row_of = torch.empty((capacity,), dtype=torch.int32, device=self.device)
        walk_args = (len(ptr) - 1, ops._dev(d_ptr, torch.int32), ops._dev(d_nodes, torch.int32), K) + tuple(self._graph_args())
        with torch.cuda.device(self.device):
            check(lib.scn_markov_hash_insert(*walk_args, ops._dev(keys, torch.int64), capacity, ops._dev(words[1:2], torch.int32),
                                             ops._dev(words[2:3], torch.int32), ops._stream()), "scn_markov_hash_insert")
            check(lib.scn_markov_hash_number(ops._dev(keys, torch.int64), capacity, K, ops._dev(row_of, torch.int32),
                                             ops._dev(words[0:1], torch.int32), ops._dev(words[3:], torch.int32), ops._stream()),
                  "scn_markov_hash_number")
            host = words.cpu().numpy()                               # the one synchronisation point: it sizes the count rows
            counts = torch.zeros((max(int(host[0]), 1), self.width), dtype=torch.int32, device=self.device)
            if host[1] == INT32_MAX and host[2] == INT32_MAX:
                check(lib.scn_markov_hash_count(*walk_args, ops._dev(keys, torch.int64), ops._dev(row_of, torch.int32), capacity,
                                                int(host[0]), ops._dev(counts, torch.int32), ops._dev(words[1:2], torch.int32),
                                                ops._stream()), "scn_markov_hash_count")
        return host, keys, row_of, counts

    # ---- the reference's surface ----
    def train(self, G, paths, capacity=None):
        """Builds the table of all orders from scratch: three launches (claim a slot per distinct key, number the slots, count) and
        one look at the device between the second and the third, which sizes the count rows.  The capacity is the next power of two
        >= (the most keys the walks can insert) / load unless one is given.  ValueError for a pair that is no edge; MemoryError,
        before any launch, for buffers that do not fit the free device memory; RuntimeError for a key that found no slot (a given
        capacity below the number of distinct keys)."""
        nbr, deg = neighbour_table(G)
        ptr, nodes = ragged(paths)
        bound = key_bound(ptr, self.max_order)
        capacity = hash_capacity(bound, self.load) if capacity is None else int(capacity)
        st = _lib.load().scn_markov_hash_check(int(nbr.shape[0]), int(nbr.shape[1]), self.max_order, capacity)
        if st == _lib.SCN_ERR_UNSUPPORTED:
            raise ValueError("the states of order %d on %d nodes x %d slots pass 2^59" % (self.max_order, nbr.shape[0], nbr.shape[1]))
        if st != 0 or capacity >= 1 << 31:
            raise ValueError("no table of %d slots for %d nodes x %d slots (the capacity is a power of two below 2^31)"
                             % (capacity, nbr.shape[0], nbr.shape[1]))
        if self.device is None:
            self.device = ops.default_device()
        need = 12 * capacity + 4 * int(nbr.shape[1]) * max(1, min(bound, capacity)) + 4 * (nbr.size + len(deg) + len(ptr) + len(nodes))
        free = self._free_bytes()
        if need > free:
            raise MemoryError("the table of %d slots and its count rows need %d bytes; %d are free on the device" % (capacity, need, free))
        self.h_nbr, self.h_deg = nbr, deg
        self.n_nodes, self.width = int(nbr.shape[0]), int(nbr.shape[1])
        self.nbr, self.deg = self._upload(nbr), self._upload(deg)
        self.counts = self.keys = self.row_of = None
        host, keys, row_of, counts = self._build(ptr, nodes, capacity)
        self._raise_bad_pair(host[1:2], ptr, nodes)
        if host[2] != INT32_MAX:
            raise RuntimeError("the hash table of %d slots is full: a key of walk %d found no slot" % (capacity, int(host[2])))
        self.keys, self.row_of, self.counts, self.capacity = keys, row_of, counts, capacity
        self.n_states = [int(x) for x in host[3:]]
        self.table_bytes = 12 * capacity + 4 * int(counts.numel())

    def _free_bytes(self):
        return int(torch.cuda.mem_get_info(self.device)[0])

    def predict_paths(self, prefixes, hops):
        """Markov_Model.predict_paths with the order chosen anew at every hop, from the prefix and the predictions so far;
        used_orders is (n, hops).  With back-off only an empty prefix predicts nothing."""
        ptr, nodes, d_ptr, d_nodes = self._prefix_args(prefixes)
        n, hops = len(ptr) - 1, int(hops)
        if hops < 1:
            raise ValueError("hops must be at least 1")
        pred, tied, used = (torch.empty((n, hops), dtype=torch.int32, device=self.device) for _ in range(3))
        err = self._err_word()
        with torch.cuda.device(self.device):
            check(_lib.load().scn_markov_hash_rollout(n, ops._dev(d_ptr, torch.int32), ops._dev(d_nodes, torch.int32), *self._rule(), hops,
                                                      ctypes.c_uint64(self.seed & (2 ** 64 - 1)), *self._graph_args(),
                                                      *self._table_args(), ops._dev(pred, torch.int32), ops._dev(tied, torch.int32),
                                                      ops._dev(used, torch.int32), ops._dev(err, torch.int32), ops._stream()),
                  "scn_markov_hash_rollout")
        self._raise_bad_pair(err, ptr, nodes)
        self.used_orders = used.cpu().numpy()
        return pred.cpu().numpy(), tied.cpu().numpy()

    def predict(self, prefix):
        """(node, was_random) from the longest context of prefix the table holds; KeyError for an empty prefix (without back-off:
        for one shorter than max_order, as Markov_Model)."""
        if len(prefix) < self.shortest:
            raise KeyError(tuple(prefix))
        pred, tied = self.predict_paths([list(prefix)], 1)
        return (int(pred[0, 0]) if pred[0, 0] >= 0 else None), bool(tied[0, 0] > 1)

    def test(self, prefixes, target_nodes, hops):
        """Accuracy of the last hop's node.  With back-off every non-empty prefix is extended, so none is compared by its own last
        node; without, Markov_Model.test."""
        if not self.backoff:
            return super().test(prefixes, target_nodes, hops)
        ptr, _ = ragged(prefixes)
        if np.any(np.diff(ptr) == 0):
            raise IndexError("an empty prefix has no last node")
        pred, tied = self.predict_paths(prefixes, hops)
        self.n_rand_choices = int((tied > 1).sum())
        target = np.asarray([int(t) for t in target_nodes], np.int64)
        if len(target) != len(pred):
            raise ValueError("prefixes and target_nodes disagree on the number of paths")
        return np.average(target == pred[:, -1].astype(np.int64))

    def two_target_scores(self, prefixes, target_nodes):
        """Markov_Model.two_target_scores on the chosen rows; used_orders is (n,)."""
        ptr, nodes, d_ptr, d_nodes, n, target, last = self._two_target_args(prefixes, target_nodes, self.shortest)
        score = torch.empty((n,), dtype=torch.float32, device=self.device)
        other, used = (torch.empty((n,), dtype=torch.int32, device=self.device) for _ in range(2))
        d_target = self._upload(target)
        err, err_t = self._err_word(), self._err_word()
        with torch.cuda.device(self.device):
            check(_lib.load().scn_markov_hash_two_target(n, ops._dev(d_ptr, torch.int32), ops._dev(d_nodes, torch.int32), *self._rule(),
                                                         ctypes.c_uint64(self.seed & (2 ** 64 - 1)), ops._dev(d_target, torch.int32),
                                                         *self._graph_args(), *self._table_args(), ops._dev(score, torch.float32),
                                                         ops._dev(other, torch.int32), ops._dev(used, torch.int32),
                                                         ops._dev(err, torch.int32), ops._dev(err_t, torch.int32), ops._stream()),
                  "scn_markov_hash_two_target")
        self._raise_bad_pair(err, ptr, nodes)
        i = int(err_t.item())
        if i != INT32_MAX:
            raise ValueError("path %d: target %d is not a neighbour of its last node %d" % (i, target[i], last[i]))
        self.used_orders = used.cpu().numpy()
        return score.cpu().numpy().astype(np.float64), other.cpu().numpy()

    def next_node_probs(self, prefixes):
        """(n, D) float64: counts / total of every prefix's chosen row by slot of its last node (0 in the padding and where no
        order qualifies); used_orders is (n,)."""
        ptr, nodes, d_ptr, d_nodes = self._prefix_args(prefixes)
        n = len(ptr) - 1
        probs = torch.empty((n, self.width), dtype=torch.float64, device=self.device)
        used = torch.empty((n,), dtype=torch.int32, device=self.device)
        err = self._err_word()
        with torch.cuda.device(self.device):
            check(_lib.load().scn_markov_hash_probs(n, ops._dev(d_ptr, torch.int32), ops._dev(d_nodes, torch.int32), *self._rule(),
                                                    *self._graph_args(), *self._table_args(), ops._dev(probs, torch.float64),
                                                    ops._dev(used, torch.int32), ops._dev(err, torch.int32), ops._stream()),
                  "scn_markov_hash_probs")
        self._raise_bad_pair(err, ptr, nodes)
        self.used_orders = used.cpu().numpy()
        return probs.cpu().numpy()

    def weights_of(self, prefix):
        """{neighbour: probability} of the row chosen for prefix."""
        if len(prefix) < self.shortest:
            raise KeyError(tuple(prefix))
        p = self.next_node_probs([list(prefix)])[0]
        v = int(prefix[-1])
        return {int(self.h_nbr[v, j]): float(p[j]) for j in range(int(self.h_deg[v]))}

    def counts_of(self, prefix):
        """{neighbour: count} of the row chosen for prefix (all 0 where no order qualifies), read from the table slot by slot."""
        if len(prefix) < self.shortest:
            raise KeyError(tuple(prefix))
        self.next_node_probs([list(prefix)])
        k, v = int(self.used_orders[0]), int(prefix[-1])
        nbrs = [int(u) for u in self.h_nbr[v, :self.h_deg[v]]]
        if k == 0:
            return {u: 0 for u in nbrs}
        ctx = [int(x) for x in prefix[-k:]]
        s = ctx[0]
        for a, b in zip(ctx[:-1], ctx[1:]):
            s = s * self.width + int(np.flatnonzero(self.h_nbr[a, :self.h_deg[a]] == b)[0])
        key = ((k - 1) << HASH_KEY_SHIFT) | s
        h = hash_mix(key) & (self.capacity - 1)
        for _ in range(self.capacity):
            at = int(self.keys[h].item()) & HASH_EMPTY
            if at == key:
                row = self.counts[int(self.row_of[h].item())].cpu().numpy()
                return {u: int(c) for u, c in zip(nbrs, row)}
            if at == HASH_EMPTY:
                break
            h = (h + 1) & (self.capacity - 1)
        raise KeyError(tuple(ctx))                                  # the readers chose this key: the table holds it

    # ---- whole paths ----
    def _path_records(self, ptr, nodes, alpha):
        """Markov_Model._path_records through scn_markov_hash_path_scores; the used order of every position stays in
        self._used_at."""
        P, T = len(ptr) - 1, len(nodes)
        if T == 0:
            self._used_at = np.zeros(0, np.int32)
            return np.zeros(0), np.zeros(0, np.int32), np.zeros(0, np.int32)
        up = self._upload(np.concatenate([ptr, nodes]))
        d_ptr, d_nodes = up[:P + 1], up[P + 1:]
        out = torch.empty((5 * T + 1,), dtype=torch.int32, device=self.device)      # prob [T] fp64 | rank | total | used [T] | err
        out[5 * T:] = INT32_MAX
        prob, rank, total, used, err = out[:2 * T].view(torch.float64), out[2 * T:3 * T], out[3 * T:4 * T], out[4 * T:5 * T], out[5 * T:]
        with torch.cuda.device(self.device):
            check(_lib.load().scn_markov_hash_path_scores(P, ops._dev(d_ptr, torch.int32), ops._dev(d_nodes, torch.int32), *self._rule(),
                                                          ctypes.c_double(alpha), *self._graph_args(), *self._table_args(),
                                                          ops._dev(prob, torch.float64), ops._dev(rank, torch.int32),
                                                          ops._dev(total, torch.int32), ops._dev(used, torch.int32),
                                                          ops._dev(err, torch.int32), ops._stream()), "scn_markov_hash_path_scores")
        host = out.cpu()
        self._raise_bad_pair(host[5 * T:], ptr, nodes)
        host = host.numpy()
        self._used_at = host[4 * T:5 * T]
        return host[:2 * T].view(np.float64), host[2 * T:3 * T], host[3 * T:4 * T]

    def path_step_log_probs(self, paths, min_prefix=2, alpha=0.0):
        """Markov_Model.path_step_log_probs with every item predicted from its chosen row; used_orders holds the items' orders."""
        from . import path_scores
        sc = super().path_step_log_probs(paths, min_prefix, alpha)
        ptr, _ = ragged(paths)
        _, item_path, item_len = path_scores.path_items(ptr, min_prefix)
        self.used_orders = self._used_at[path_scores.item_positions(ptr, item_path, item_len)]
        return sc

    def score_paths(self, paths, mask=None, min_prefix=2, alpha=0.0):
        """Markov_Model.score_paths plus order_hist: the items per used order 0 .. max_order.  n_unseen = order_hist[0]."""
        from . import path_scores
        sc = self.path_step_log_probs(select_paths(paths, mask), min_prefix, alpha)
        hist = np.bincount(self.used_orders, minlength=self.max_order + 1)
        return dict(path_scores.summary(sc), n_unseen=int(hist[0]), order_hist=[int(x) for x in hist])
