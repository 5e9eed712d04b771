"""Training on whole node paths behind Scone_GCN.path_set / path_loss / path_grad_step / train_paths: the teacher-forced sequence
loss whose value path_step_log_probs (path_scores.py) reports.  An item is (path p, prefix of k nodes) and its target is the node
p[k]; a path of n nodes holds n - 2 of them at min_prefix = 2, where train() sees one.  The paths go to the device once per training
run (PathSet: the scn_path_steps records of every step, and per min_prefix the item list); an optimiser step names its items by
index, cuts this rank's share into micro-batches by the rule of Scone_GCN.stage(), and scn_path_stage (csrc/scn_paths.hip) turns
each into the (x, last_nodes, y) a step reads -- the prefixes' flows as slabs, their last nodes, and one-hot target rows that carry
the item's weight, since every loss kernel computes d_logp = y * scale.  The micro-batches then go through
Scone_GCN._accumulate_staged like any others.  The buffers live in a pool that is kept from step to step together with the items
each buffer last held, so a restage resets only the words those items wrote (ops.PATH_STAGE_SPARSE_CLEAR) instead of zero-filling
|E| rows per slab.  Nothing of size sum(len^2) is built anywhere, and the caller's flows are neither read nor written."""
from collections import namedtuple

import numpy as np
import torch

from . import _lib, ops, path_scores
from . import distributed as dp
from ._lib import check
from .ops import NS

WEIGHTS = ("step", "path")

ItemSet = namedtuple("ItemSet", "item_ptr item_path item_len path_d len_d weight weight_d")
ItemSet.__doc__ = """The items of a path set at one min_prefix: path_scores.path_items on the host (int64), item_path / item_len on the
device (int32), and the "path" weights fp32(1 / items of the item's path) on both sides."""


def item_weights(item_ptr, item_path, weight):
    """w [M] float32 of the items of path_scores.path_items: "step" 1 for every item; "path" 1 / (items of the item's path), rounded to
    fp32, so that every path with an item counts the same."""
    if weight not in WEIGHTS:
        raise ValueError("weight must be 'step' or 'path'")
    if weight == "step":
        return np.ones(len(item_path), np.float32)
    count = np.diff(np.asarray(item_ptr, np.int64))
    return (1.0 / count[np.asarray(item_path, np.int64)]).astype(np.float32)


def epoch_batches(rs, n_items, batch_size):
    """The optimiser steps of one epoch of train_paths: ONE rs.permutation(n_items), cut into max(1, n_items // batch_size) batches
    of batch_size items in the order drawn.  The n_items % batch_size items at the permutation's end sit the epoch out (train() takes
    n // batch_size steps per epoch too) -- except below one full batch, where the single batch holds all n_items.  Returns a list
    of int64 arrays; [] without an item."""
    n_items, batch_size = int(n_items), int(batch_size)
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    if n_items <= 0:
        return []
    perm = np.asarray(rs.permutation(n_items), np.int64)
    n_batches = max(1, n_items // batch_size)
    return [perm[b * batch_size:(b + 1) * batch_size] for b in range(n_batches)]


class PathSet:
    """Node paths resident on the device for training (Scone_GCN.path_set): path_scores.device_steps once, and per min_prefix the
    item list on both sides.  Bound to the plan it was looked up in."""

    def __init__(self, net, inputs, paths):
        self.steps = path_scores.device_steps(net, inputs, paths)
        self.plan = self.steps.plan
        self.n_paths = self.steps.n_paths
        self._items = {}

    def _item_set(self, min_prefix):
        k0 = max(int(min_prefix), 1)
        it = self._items.get(k0)
        if it is None:
            item_ptr, item_path, item_len = path_scores.path_items(self.steps.path_ptr, k0)
            w = item_weights(item_ptr, item_path, "path")
            dev = self.plan.device
            i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
            it = self._items[k0] = ItemSet(item_ptr, item_path, item_len, i32(item_path), i32(item_len), w, torch.from_numpy(w).to(dev))
        return it

    def items(self, min_prefix=2):
        """(item_ptr [P + 1], item_path [M], item_len [M]) int64, as path_scores.path_items gives them: what `items` of
        path_grad_step index."""
        it = self._item_set(min_prefix)
        return it.item_ptr, it.item_path, it.item_len


class StagePool:
    """The micro-batch buffers of path_grad_step, kept from step to step: per micro-batch position x [cap, E, NS, 1], last [cap * NS],
    y [cap * NS, D] and the items the buffer last held (device slices), which is what lets the next scn_path_stage reset only their
    words.  A buffer is replaced (and dense-filled once) only when a micro-batch needs more slabs than it has.  The remembered items
    index ONE path set's records, so the pool belongs to that path set (and through it to its plan)."""

    def __init__(self, ps):
        self.ps = ps
        self.bufs = []

    def stage(self, j, ip, il, wt):
        """Micro-batch j = the items (ip, il[, wt]) (device slices): staged -> (x, last, y, None) as _accumulate_staged takes it."""
        plan, st = self.ps.plan, self.ps.steps
        dev, E, D = plan.device, plan.n_edges, plan.max_deg
        n = int(ip.shape[0])
        S = ops.pad_count(n) // NS
        while len(self.bufs) <= j:
            self.bufs.append(None)
        buf = self.bufs[j]
        if buf is None or buf["cap"] < S:
            buf = self.bufs[j] = {"cap": S, "x": torch.empty((S, E, NS, 1), device=dev, dtype=torch.float32),
                                  "last": torch.empty((S * NS,), device=dev, dtype=torch.int32),
                                  "y": torch.empty((S * NS, D), device=dev, dtype=torch.float32), "prev": None}
        prev = buf["prev"] if ops.PATH_STAGE_SPARSE_CLEAR else None
        buf["prev"] = None                                           # (until the call below has been queued the buffer holds anything)
        p = lambda t: None if t is None else ops._dev(t, t.dtype)
        # the whole buffer, not its first S slabs: a longer previous occupant's columns are reset, and every last node and target row
        # behind the items is written (zero)
        check(_lib.load().scn_path_stage(n, buf["cap"], p(ip), p(il), p(wt), -1 if prev is None else int(prev[0].shape[0]),
                                         p(prev[0]) if prev else None, p(prev[1]) if prev else None, st.n_paths, p(st.ptr_d),
                                         p(st.nodes_d), p(st.slot), p(st.row), p(st.run), p(st.next_same), E, NS, D, p(buf["x"]),
                                         p(buf["last"]), p(buf["y"]), ops._stream()), "scn_path_stage")
        buf["prev"] = (ip, il)
        return buf["x"][:S], buf["last"][:S * NS], buf["y"][:S * NS], None


def _pool(net, ps):
    pool = net._path_pool
    if pool is None or pool.ps is not ps:                            # another path set (or, with it, another plan): nothing carries over
        pool = net._path_pool = StagePool(ps)
    return pool


def _accumulate(net, plan, ps, it, local, weight, total):
    """This rank's items `local` (indices into the item list): staged micro-batch by micro-batch, then one _accumulate_staged."""
    dev = plan.device
    n = len(local)
    mb = net.path_micro_batch or net._stage_micro_batch(plan, n)
    mb = max(NS, ops.pad_count(int(mb)))
    idx_d = torch.from_numpy(np.ascontiguousarray(local, np.int64)).to(dev)
    ip, il = it.path_d[idx_d], it.len_d[idx_d]                        # one upload (the indices) and three gathers per step
    wt = it.weight_d[idx_d] if weight == "path" else None
    pool = _pool(net, ps)
    staged = [pool.stage(j, ip[c0:c0 + mb], il[c0:c0 + mb], None if wt is None else wt[c0:c0 + mb])
              for j, c0 in enumerate(range(0, n, mb))]
    return net._accumulate_staged(plan, staged, total, fresh=True)


def grad_step(net, inputs, ps, items, apply=True, min_prefix=2, weight="step"):
    """Scone_GCN.path_grad_step."""
    if weight not in WEIGHTS:
        raise ValueError("weight must be 'step' or 'path'")
    if net.skip_mode != "dense":
        raise ValueError("path_grad_step runs the dense step only (skip_mode %r)" % net.skip_mode)
    plan = net._plan(inputs)
    if plan is None or plan is not ps.plan:
        raise ValueError("the path set was built for other operators than these inputs")
    it = ps._item_set(min_prefix)
    items = np.asarray(items, np.int64).reshape(-1)
    M = len(it.item_path)
    if len(items) and (int(items.min()) < 0 or int(items.max()) >= M):
        raise IndexError("item index outside the path set's %d items" % M)
    # the GLOBAL batch's weight, summed in fp64 from the fp32 weights the kernels multiply by
    total = float(len(items)) if weight == "step" else float(np.sum(it.weight[items], dtype=np.float64))
    acc = {}

    def grad_fn(local, _count):
        acc["loss"] = _accumulate(net, plan, ps, it, local, weight, total)
    dp.data_parallel_grad(items, grad_fn, net._flat_g, net.process_group, force=net.collective_always)
    if apply:
        net._adam()
    return acc.get("loss", torch.zeros((), device=net._flat_w.device, dtype=torch.float64))


def path_loss(net, inputs, paths, mask=None, min_prefix=2, weight="step"):
    """Scone_GCN.path_loss."""
    if mask is not None:
        paths = [paths[i] for i in np.flatnonzero(np.asarray(mask) == 1)]
    sc = path_scores.step_log_probs(net, inputs, paths, min_prefix)
    if len(sc.logp) == 0:
        return float("nan")
    item_path = np.repeat(np.arange(len(sc.ptr) - 1), np.diff(sc.ptr))
    w = item_weights(sc.ptr, item_path, weight).astype(np.float64)
    return float(-np.sum(w * sc.logp) / np.sum(w)) + net._ridge(net.weights)


def train_paths(net, inputs, paths, train_mask, test_mask, min_prefix=2, weight="step"):
    """Scone_GCN.train_paths: train() with every (path, prefix) item of the train paths as an example.  The Adam state is reset; the
    paths go to the device once (path_set over ALL paths, so that the masks index them); per epoch the train items are permuted once
    from the module RNG and cut by epoch_batches; step i sets the bias correction's index to the loop index, as train() does; after
    every epoch score_paths runs on both masks and one line is printed.  Returns (train_scores, test_scores) of the last epoch."""
    from . import scone_trajectory_model as stm
    if weight not in WEIGHTS:
        raise ValueError("weight must be 'step' or 'path'")
    train_mask, test_mask = np.asarray(train_mask), np.asarray(test_mask)
    ps = net.path_set(inputs, paths)
    _, item_path, _ = ps.items(min_prefix)
    train_items = np.flatnonzero(train_mask[item_path] == 1) if len(item_path) else np.zeros(0, np.int64)
    net._m.zero_(); net._v.zero_(); net._step = 0                     # adam state re-initialised (STM:312)
    train_scores = test_scores = None
    i = 0
    try:
        for epoch in range(net.epochs):
            for batch in epoch_batches(stm._RNG, len(train_items), net.batch_size):
                net._step = i                                        # update_fun(i, ...): bias correction with the LOOP index (STM:310)
                net.path_grad_step(inputs, ps, train_items[batch], min_prefix=min_prefix, weight=weight)
                i += 1
            train_scores = net.score_paths(inputs, paths, train_mask, min_prefix)
            test_scores = net.score_paths(inputs, paths, test_mask, min_prefix)
            if net.verbose and dp.world(net.process_group)[0] == 0:
                print('Epoch {} -- train step log-prob: {:.6f} -- train step acc {:.3f} -- test step log-prob {:.6f} -- test step acc {:.3f}'
                      .format(epoch, train_scores["mean_step_logp"], train_scores["accuracy"], test_scores["mean_step_logp"],
                              test_scores["accuracy"]))
    finally:
        net.drop_path_stage()                                        # the run's path set ends here: what follows training gets the memory back
    if net.verbose and dp.world(net.process_group)[0] == 0:
        print("Epochs: {}, learning rate: {}, batch size: {} items, weight: {}, model: {}".format(
            net.epochs, net.step_size, net.batch_size, weight, getattr(net.model, '__name__', str(net.model))))
    net.trained = True
    return train_scores, test_scores
