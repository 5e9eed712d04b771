"""Teacher-forced scoring of whole node paths behind Scone_GCN.path_step_log_probs / path_log_likelihood / score_paths: the model's
log-probability of the node actually visited, step by step, with every prefix as input.  An item is (path p, prefix of k nodes) and
predicts node p[k]; the items of a call are path-major with k ascending.  The paths go to the device once and scn_path_steps
(csrc/scn_paths.hip) turns every step into (slot, device row, value of its edge's flow after the step, next step on that edge);
then, per chunk of items, scn_path_slabs writes the prefixes' flows as slabs, ONE batched forward (ops.forward_logp with the
prefixes' last nodes) reads them and scn_path_score takes the log-probability, the rank and the neighbour mass at the slot the path
took.  Nothing of size sum(len^2) is ever built on the host, the caller's flows are neither read nor written, the evaluation cache is
not touched, and the results come back in one copy at the end."""
from collections import namedtuple

import numpy as np
import torch

from . import _lib, multihop, ops
from ._lib import check
from .complex import Bconds
from .ops import INT32_MAX, NS

PathScores = namedtuple("PathScores", "ptr logp rank mass prefix_len")
PathScores.__doc__ = """Per-step scores of P paths.  ptr [P + 1] int64: path p owns the items ptr[p] .. ptr[p + 1]; per item, path-major
with the prefix length ascending: logp (float64) the log-probability of the node visited (minus mass when normalised), rank (int64)
how many real neighbours the model ranks before it (0: the model's own choice), mass (float64) log of the probability the model leaves
on real neighbours, prefix_len (int64) the k nodes the item's input holds."""


def ragged(paths):
    """(ptr [P + 1], nodes) int64 of a list of node paths."""
    lens = np.fromiter((len(p) for p in paths), np.int64, len(paths))
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nodes = np.concatenate([np.asarray(p, np.int64).reshape(-1) for p in paths]) if len(paths) and ptr[-1] else np.zeros(0, np.int64)
    return ptr, nodes


def path_items(path_ptr, min_prefix):
    """The items of a call: (item_ptr [P + 1], item_path [M], item_len [M]) int64.  Path p of n nodes owns the prefixes of
    k = max(min_prefix, 1) .. n - 1 nodes, in that order; a shorter path has none."""
    k0 = max(int(min_prefix), 1)
    lens = np.diff(np.asarray(path_ptr, np.int64))
    count = np.maximum(lens - k0, 0)
    item_ptr = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    item_path = np.repeat(np.arange(len(lens), dtype=np.int64), count)
    item_len = k0 + np.arange(int(item_ptr[-1]), dtype=np.int64) - item_ptr[:-1][item_path]
    return item_ptr, item_path, item_len


PathSteps = namedtuple("PathSteps", "plan tab n_paths path_ptr nodes ptr_d nodes_d slot row run next_same")
PathSteps.__doc__ = """Paths resident on the device with their scn_path_steps records: the plan and step tables they were looked up in,
path_ptr [P + 1] / nodes [T] int64 on the host, ptr_d / nodes_d int32 on the device, and slot / row / run / next_same [T] parallel to
nodes_d (None, like ptr_d and nodes_d, when the paths hold no node at all)."""


def device_steps(net, inputs, paths):
    """The paths of a scoring call or a path set (path_train.py) on the device, every step looked up by scn_path_steps: PathSteps.
    Refuses a probed closure (TypeError) and a step between two nodes that are no neighbours (KeyError((a, b)), after the one look
    at the error word and before any forward)."""
    if net.model_type != 'bunch' and not isinstance(inputs[0], Bconds):
        raise TypeError("multi-hop prediction needs the Bconds object of SimplicialComplex.bconds() (what data_setup returns) as "
                        "the readout operand: a plain Bcond_func closure only knows the last nodes it has been probed at")
    plan = net._plan(inputs)
    if plan is None:
        raise TypeError("path scoring runs the native model functions (scone_func / ebli_func / bunch_func) only")
    nbrhoods = inputs[0] if net.model_type == 'bunch' else inputs[0].nbrhoods
    tab = multihop.step_tables(plan, nbrhoods, net._edge_lookup(inputs), "flow")
    lib, dev, D, E = _lib.load(), plan.device, plan.max_deg, plan.n_edges
    path_ptr, nodes = ragged(paths)
    P, T = len(path_ptr) - 1, int(path_ptr[-1])
    if T >= INT32_MAX:
        raise ValueError("paths of %d nodes in all are too many" % T)
    if T == 0:
        return PathSteps(plan, tab, P, path_ptr, nodes, None, None, None, None, None, None)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
    p = lambda t: ops._dev(t, t.dtype)
    ptr_d, nodes_d = i32(path_ptr), i32(np.clip(nodes, -1, INT32_MAX))
    slot, row, next_same = (torch.empty((T,), device=dev, dtype=torch.int32) for _ in range(3))
    run = torch.empty((T,), device=dev, dtype=torch.float32)
    err = torch.full((1,), INT32_MAX, device=dev, dtype=torch.int32)
    check(lib.scn_path_steps(P, p(ptr_d), p(nodes_d), tab.n_nodes, D, tab.p_deg, tab.p_node, tab.p_edge, tab.p_sign, E, p(slot), p(row),
                             p(run), p(next_same), p(err), ops._stream()), "scn_path_steps")
    t = int(err.item())                                              # the one look before the forwards: a bad pair costs none
    if t != INT32_MAX:
        raise KeyError((int(nodes[t]), int(nodes[t + 1])))
    return PathSteps(plan, tab, P, path_ptr, nodes, ptr_d, nodes_d, slot, row, run, next_same)


def step_log_probs(net, inputs, paths, min_prefix=2, normalise=False):
    """Scone_GCN.path_step_log_probs."""
    st = device_steps(net, inputs, paths)
    plan, tab, P, path_ptr, nodes, ptr_d, nodes_d, slot, row, run, next_same = st
    lib, dev, D, E, weights = _lib.load(), plan.device, plan.max_deg, plan.n_edges, net.weights
    item_ptr, item_path, item_len = path_items(path_ptr, min_prefix)
    M = int(item_ptr[-1])
    if M == 0:                                                       # (paths without a node have no item either)
        return PathScores(item_ptr, np.zeros(0), np.zeros(0, np.int64), np.zeros(0), np.zeros(0, np.int64))
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
    p = lambda t: ops._dev(t, t.dtype)
    ip_d, il_d = i32(item_path), i32(item_len)
    item_last = i32(nodes[path_ptr[item_path] + item_len - 1])
    out_logp, out_mass = (torch.empty((M,), device=dev, dtype=torch.float32) for _ in range(2))
    out_rank = torch.empty((M,), device=dev, dtype=torch.int32)
    mb = net.multi_hop_micro_batch or ops.forward_micro_batch(plan, weights, M)
    mb = min(max(NS, ops.pad_count(int(mb))), ops.pad_count(M))
    x = torch.empty((mb // NS, E, NS, 1), device=dev, dtype=torch.float32)
    last = torch.zeros((mb,), device=dev, dtype=torch.int32)
    trace = net._multi_hop_trace
    for c0 in range(0, M, mb):
        n = min(mb, M - c0)
        S = ops.pad_count(n) // NS
        ip, il = p(ip_d[c0:c0 + n]), p(il_d[c0:c0 + n])
        check(lib.scn_path_slabs(n, S, ip, il, P, p(ptr_d), p(row), p(run), p(next_same), E, NS, p(x), ops._stream()), "scn_path_slabs")
        last[:n].copy_(item_last[c0:c0 + n])
        if n < S * NS:
            last[n:S * NS].zero_()                                   # padding columns: an all-zero flow read at node 0
        logp = ops.forward_logp(plan, x[:S], last[:S * NS], weights).contiguous()
        if trace is not None:
            trace.append({"item0": c0, "flows": ops.slabs_to_batch(x[:S], plan.layout, 1, n)[:, :, 0].cpu().numpy(),
                          "last": last[:n].cpu().numpy(), "logp": logp[:n].cpu().numpy()})
        check(lib.scn_path_score(n, D, ip, il, P, p(ptr_d), p(nodes_d), p(slot), tab.p_deg, tab.n_nodes, p(logp), p(out_logp[c0:c0 + n]),
                                 p(out_rank[c0:c0 + n]), p(out_mass[c0:c0 + n]), ops._stream()), "scn_path_score")
    logp, mass = out_logp.cpu().numpy().astype(np.float64), out_mass.cpu().numpy().astype(np.float64)
    return PathScores(item_ptr, logp - mass if normalise else logp, out_rank.cpu().numpy().astype(np.int64), mass, item_len)


def log_likelihood(net, inputs, paths, min_prefix=2, normalise=False):
    """Scone_GCN.path_log_likelihood: (ll [P] float64 = the fp64 sum of every path's step log-probabilities, n_steps [P] int64)."""
    sc = step_log_probs(net, inputs, paths, min_prefix, normalise)
    return segment_sums(sc.logp, sc.ptr), np.diff(sc.ptr)


def segment_sums(values, ptr):
    """sum of values[ptr[p] : ptr[p + 1]] per p, fp64; an empty segment sums to 0 (np.add.reduceat would repeat a neighbour there)."""
    ptr = np.asarray(ptr, np.int64)
    out = np.zeros(len(ptr) - 1, np.float64)
    full = np.diff(ptr) > 0
    if full.any():
        out[full] = np.add.reduceat(np.asarray(values, np.float64), ptr[:-1][full])
    return out


def score_paths(net, inputs, paths, mask=None, min_prefix=2, normalise=False):
    """Scone_GCN.score_paths."""
    if mask is not None:
        paths = [paths[i] for i in np.flatnonzero(np.asarray(mask) == 1)]
    return summary(step_log_probs(net, inputs, paths, min_prefix, normalise))


def summary(sc):
    """The dict of score_paths (the model's and the baselines') from a PathScores."""
    n = len(sc.logp)
    mean = float(np.sum(sc.logp) / n) if n else float("nan")
    return {"mean_step_logp": mean, "perplexity": float(np.exp(-mean)), "accuracy": float(np.mean(sc.rank == 0)) if n else float("nan"),
            "n_steps": n}


def item_positions(path_ptr, item_path, item_len):
    """The flat node position path_ptr[p] + k of every item (p, k): where the per-position records of the baselines' kernels
    (scn_markov_path_scores, scn_project_path_scores) hold the item's prediction."""
    return np.asarray(path_ptr, np.int64)[:-1][item_path] + item_len
