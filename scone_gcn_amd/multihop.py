"""Multi-hop prediction (STM:110-206) behind the multi-hop methods of Scone_GCN: the greedy rollout, the probability tree, the beam
search and the sampled paths.  Each hop / tree level is ONE batched forward over all its trajectories / leaves (chunked by
ops.forward_micro_batch, or by the net's multi_hop_micro_batch when set); the steps between -- choose the next node, set the edge
it crosses, build the children, reduce the leaf probabilities -- are csrc/scn_hops.hip.  The caller's flows are never written (the
reference writes into them, STM:149-150) and the evaluation cache is not touched.  A decoder is a function of (net, inputs, ...):
its setup is one Call, the entries of a level are one Level, and what every decoder does per level -- forward it, allocate its
children, name the pair behind an error word -- is Call.level_logp, Call.children and Call.missing_edge."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib, ops
from ._lib import check
from .complex import Bconds
from .ops import INT32_MAX, NS
from .synthetic_data_gen import SparseFlows

_STEP_TABLES = {}


class StepTables:
    """Where a step from node v through slot j leads, as scn_hop_select / scn_tree_expand read it (include/scone_hip.h):
    node / edge / sign [V, D] (edge = DEVICE row, -1 where the pair has no edge) and deg [V], on the device and on the host, and
    the tables' device pointers as the launches take them (p_deg, p_node, p_edge, p_sign).
    rule "binary" (STM:139-147): slot j of nbrhoods[v] as it is; +1 on E_lookup[(v, u)] if that key exists, else -1 on
    E_lookup[(u, v)].  rule "dist" (STM:160, 176-187): the real neighbours of v left-aligned (the -1 padding dropped), -1 / +1 on
    E_lookup[sorted(v, u)] by whether v > u.  rule "flow" (path_scores.py; path_to_flow, SDG:327-344): slot j as the readout numbers
    it -- this project's left-aligned table, interior padding is refused --, +1 / -1 on E_lookup[sorted(v, u)] by whether v < u, times
    flips[that edge] (the Bconds flips, caller's edge order) where there are any: the value a step adds to the flow the model reads."""

    def __init__(self, nbrhoods, E_lookup, edge_perm, rule, device, flips=None):
        nb = np.asarray(nbrhoods, np.int64)
        if nb.ndim != 2:
            raise ValueError("nbrhoods must be a (V, D) table padded with -1")
        V, D = nb.shape
        if rule == "dist":
            real = nb >= 0
            order = np.argsort(~real, axis=1, kind="stable")
            nb = np.where(np.take_along_axis(real, order, 1), np.take_along_axis(nb, order, 1), -1)
        elif rule == "flow":
            if np.any((nb >= 0) != (np.arange(D)[None, :] < (nb >= 0).sum(axis=1)[:, None])):
                raise ValueError("rule 'flow' needs a left-aligned nbrhoods table (the -1 padding behind a node's neighbours)")
        elif rule != "binary":
            raise ValueError("rule must be 'binary', 'dist' or 'flow'")
        n = len(E_lookup)
        keys = np.fromiter((c for k in E_lookup.keys() for c in k), np.int64, 2 * n).reshape(n, 2)
        vals = np.fromiter(E_lookup.values(), np.int64, n)
        M = int(max(V, keys.max() + 1 if n else 0, 1))
        code = keys[:, 0] * M + keys[:, 1]
        srt = np.argsort(code, kind="stable")
        code, vals = code[srt], vals[srt]

        def lookup(a, b):                                       # E_lookup[(a, b)] elementwise, -1 where the key is missing
            if n == 0:
                return np.full(np.shape(a), -1, np.int64)
            ok = (a >= 0) & (b >= 0) & (a < M) & (b < M)
            c = np.where(ok, a * M + b, -1)
            pos = np.minimum(np.searchsorted(code, c), n - 1)
            return np.where(ok & (code[pos] == c), vals[pos], -1)
        v = np.broadcast_to(np.arange(V, dtype=np.int64)[:, None], nb.shape)
        if rule == "binary":
            fwd, bwd = lookup(v, nb), lookup(nb, v)
            edge = np.where(fwd >= 0, fwd, bwd)
            sign = np.where(fwd >= 0, 1.0, -1.0)
        else:
            edge = lookup(np.minimum(v, nb), np.maximum(v, nb))
            sign = np.where(v < nb, 1.0, -1.0)
        edge = np.where(nb >= 0, edge, -1)
        E = len(edge_perm)
        if np.any(edge >= E):
            raise ValueError("E_lookup holds an edge index outside the complex's %d edges" % E)
        if rule == "flow" and flips is not None:
            sign = sign * np.asarray(flips, np.float64).reshape(-1)[np.maximum(edge, 0)]
        row = np.where(edge >= 0, np.asarray(edge_perm)[np.maximum(edge, 0)], -1)
        self.rule, self.n_nodes, self.width = rule, V, D
        self.h_node, self.h_edge = nb, row
        self.h_deg = (nb >= 0).sum(axis=1)
        to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(device)
        self.node, self.edge = to(nb, np.int32), to(row, np.int32)
        self.sign = to(np.where(edge >= 0, sign, 0.0), np.float32)
        self.deg = to(self.h_deg, np.int32)
        self.p_deg, self.p_node, self.p_edge, self.p_sign = (ctypes.c_void_p(t.data_ptr()) for t in
                                                             (self.deg, self.node, self.edge, self.sign))


def step_tables(plan, nbrhoods, E_lookup, rule):
    """StepTables of (plan, nbrhoods, E_lookup, rule), cached on the objects' identity (treated as immutable while cached)."""
    key = (id(plan), id(nbrhoods), id(E_lookup), rule)
    hit = _STEP_TABLES.get(key)
    if hit is not None and hit[0] is nbrhoods and hit[1] is E_lookup and hit[2] is plan:
        return hit[3]
    flips = getattr(getattr(plan, "bconds", None), "flips", None) if rule == "flow" else None      # (the plan's readout operand owns them)
    tab = StepTables(nbrhoods, E_lookup, plan.layout.perm[1], rule, plan.device, flips)
    if tab.width != plan.max_deg:
        raise ValueError("nbrhoods has %d slots, the model's readout %d" % (tab.width, plan.max_deg))
    if len(_STEP_TABLES) >= 8:
        _STEP_TABLES.pop(next(iter(_STEP_TABLES)))
    _STEP_TABLES[key] = (nbrhoods, E_lookup, plan, tab)
    return tab


def _p(t):                                                       # the device pointer of a launch argument (None stays NULL)
    return None if t is None else ops._dev(t, t.dtype)


Level = namedtuple("Level", "root node score path_row path_sign parent slot count leaf_ptr entry_of", defaults=(None,) * 5)
Level.__doc__ = """The entries of one level of a decoder, one per path kept (device tensors).  root: the trajectory the entry belongs
to; node: where its path stands (-1: a dead entry); score: its summed log-probability (the tree: its probability); path_row /
path_sign [n, h]: the edges its h steps set (None on a final level, whose entries are never forwarded).  parent / slot: the entry
of the level before that it continues, counted inside its root, and the slot it took (beam, samples).  The sampled decoder adds
count (samples on the entry), leaf_ptr [N + 1] (root r owns entries leaf_ptr[r] .. leaf_ptr[r + 1]) and entry_of [N, S] (the
entry of every sample inside its root, -1: dropped)."""


def root_level(n, last_nodes, device, score=0.0):
    """Level 0: one entry per trajectory at its last node, no steps yet."""
    return Level(torch.arange(n, device=device, dtype=torch.int32),
                 torch.from_numpy(np.ascontiguousarray(np.asarray(last_nodes).reshape(-1), np.int32)).to(device),
                 torch.full((n,), score, device=device, dtype=torch.float32),
                 torch.empty((n, 0), device=device, dtype=torch.int32), torch.empty((n, 0), device=device, dtype=torch.float32))


class Call:
    """What one multi-hop call of `net` on `inputs` works with: the plan (native model functions on a Bconds readout only), the
    step tables of `rule`, N trajectories of D slots, the resident root slabs (a copy: the caller's flows stay as they are),
    whether the forwards run on field-of-view lists (multi_hop_skip = "field" and the lists serve the model), and the net's trace
    and fractions lists.  refuse: (test, message) pairs on the decoder's own arguments, called in order after the hops check and
    raised as ValueError; sized: (label, arrays ...) that need one entry per trajectory; defaults: a missing nbrhoods / E_lookup is the complex's own."""

    def __init__(self, net, inputs, hops, rule, nbrhoods, E_lookup, sized, refuse=(), defaults=False):
        self.hops = int(hops)
        if self.hops < 1:
            raise ValueError("hops must be at least 1")
        for bad, message in refuse:
            if bad():
                raise ValueError(message)
        if net.model_type != 'bunch' and not isinstance(inputs[0], Bconds):
            raise TypeError("multi-hop prediction needs the Bconds object of SimplicialComplex.bconds() (what data_setup returns) as "
                            "the readout operand: a plain Bcond_func closure only knows the last nodes it has been probed at")
        self.net, self.plan = net, net._plan(inputs)
        if self.plan is None:
            raise TypeError("multi-hop prediction runs the native model functions (scone_func / ebli_func / bunch_func) only")
        if defaults and nbrhoods is None:
            nbrhoods = inputs[0] if net.model_type == 'bunch' else inputs[0].nbrhoods
        if defaults and E_lookup is None:
            E_lookup = net._edge_lookup(inputs)
        self.tab = step_tables(self.plan, nbrhoods, E_lookup, rule)
        self.lib, self.dev = _lib.load(), self.plan.device
        X = inputs[-1]
        self.N, self.D = len(X) if isinstance(X, SparseFlows) else X.shape[0], self.plan.max_deg
        label, *arrays = sized
        if any(a is not None and len(np.asarray(a).reshape(-1)) != self.N for a in arrays):
            raise ValueError("%s need one entry per trajectory of inputs (%d)" % (label, self.N))
        self.root_x, _ = ops.flows_to_slabs(X, self.plan.layout, self.dev)
        self.field = net.multi_hop_skip == "field" and ops.field_served(self.plan, net.weights) is not None
        self.trace, self.fractions = net._multi_hop_trace, net._multi_hop_fractions

    def micro_batch(self, n):                                   # entries per forward of a level of n entries (a multiple of NS)
        mb = self.net.multi_hop_micro_batch or ops.forward_micro_batch(self.plan, self.net.weights, n)
        return max(NS, ops.pad_count(int(mb)))

    def level_logp(self, lv, dead=False):
        """Log-probabilities [L, D] of the L entries of lv: per chunk of micro_batch(L) entries, scn_tree_slabs builds the input slabs
        from the resident root slabs and the entries' path entries, and the forward reads them with the entries' nodes as last nodes.
        dead: the level may hold dead entries (node -1: the child of a pair without an edge, a beam's unused tail); they ride along
        with last node 0 and their output is never read (the tree has none: its nodes go in as they are).  On field-of-view lists (ops.field_activity of the chunk's nodes, a dead entry lists nothing),
        scn_tree_slabs_list fills only the listed items of the scratch input and the forward computes only its listed items."""
        plan, lib, weights, root_x = self.plan, self.lib, self.net.weights, self.root_x
        L, h, E = int(lv.root.shape[0]), int(lv.path_row.shape[1]), root_x.shape[1]
        mb = min(self.micro_batch(L), ops.pad_count(L))
        n_layers = (len(weights) - 1) // 3
        x = torch.empty((mb // NS, E, NS, 1), device=self.dev, dtype=torch.float32)
        last = torch.zeros((mb,), device=self.dev, dtype=torch.int32)
        out = torch.empty((L, self.D), device=self.dev, dtype=torch.float32)
        for c0 in range(0, L, mb):
            n = min(mb, L - c0)
            S = ops.pad_count(n) // NS
            activity = ops.field_activity(plan, lv.node[c0:c0 + n], n, n_layers) if self.field else None
            root, rows, signs = _p(lv.root[c0:c0 + n]), _p(lv.path_row[c0:c0 + n] if h else None), _p(lv.path_sign[c0:c0 + n] if h else None)
            if activity:
                if self.fractions is not None:
                    self.fractions.append(activity["active_fraction"])
                check(lib.scn_tree_slabs_list(plan.conv.handle, n, S, h, root, rows, signs, self.N, _p(root_x), E, NS, _p(x),
                                              activity["input"].ref(), ops._stream()), "scn_tree_slabs_list")
            else:
                check(lib.scn_tree_slabs(n, S, h, root, rows, signs, self.N, _p(root_x), E, NS, _p(x), ops._stream()), "scn_tree_slabs")
            if n < S * NS:
                last[n:S * NS].zero_()
            node = lv.node[c0:c0 + n]
            torch.clamp(node, min=0, out=last[:n]) if dead else last[:n].copy_(node)
            out[c0:c0 + n] = ops.forward_logp(plan, x[:S], last[:S * NS], weights, activity)[:n]
        return out

    def children(self, n, h, final=False, links=False, count=False):
        """The unwritten n children of a level of h steps; a final level carries no paths."""
        i32 = lambda *s: torch.empty(s, device=self.dev, dtype=torch.int32)
        f32 = lambda *s: torch.empty(s, device=self.dev, dtype=torch.float32)
        return Level(root=i32(n), node=i32(n), score=f32(n), path_row=None if final else i32(n, h + 1),
                     path_sign=None if final else f32(n, h + 1), parent=i32(n) if links else None, slot=i32(n) if links else None,
                     count=i32(n) if count else None)

    def missing_edge(self, word, nodes, choice=None, sort=False):
        """The KeyError((node, neighbour)) of error word `word`, like the reference's E_lookup: entry word // D of `nodes` through
        slot word % D -- or, with the rollout's choices, trajectory `word` through its choice.  sort: the tree's sorted key."""
        entry, slot = divmod(word, self.D) if choice is None else (word, int(choice[word]))
        v = int(nodes[entry])
        pair = (v, int(self.tab.h_node[v, slot]) if 0 <= v < self.tab.n_nodes else -1)
        return KeyError(tuple(sorted(pair)) if sort else pair)

    def raise_first_missing_edge(self, err, levels):
        """err [hops]: the error words of all levels, read once at the end; the first failing level wins."""
        errs = err.cpu().numpy()
        for h in np.flatnonzero(errs != INT32_MAX)[:1]:
            raise self.missing_edge(int(errs[h]), levels[h].node)


# ------------------------------------------------------------------ greedy rollout
def rollout(net, inputs, hops, nbrhoods, E_lookup, cur_nodes=None, n_limit=None, advance=True, fill=float("-inf"), defaults=True):
    """Greedy rollout on the device: returns (choices [N] of the final hop, nodes [hops, N] or None).  advance: the current node and
    the readout's last node move to the chosen neighbour (predict_paths); else both stay (cur_nodes) and slots at or past n_limit
    are filled with `fill` (multi_hop_accuracy_binary).  The net's trace list gets, per hop, (flows (N, E) in the caller's edge
    order, readout last nodes, logp (N, D)) as the forward saw them and the choices."""
    ctx = Call(net, inputs, hops, "binary", nbrhoods, E_lookup, ("last nodes and n_nbrs", inputs[1], cur_nodes, n_limit),
               defaults=defaults)
    plan, tab, N, dev, x, trace = ctx.plan, ctx.tab, ctx.N, ctx.dev, ctx.root_x, ctx.trace
    last = ops._last_nodes_dev(inputs[1], x.shape[0] * NS, dev)
    cur = last[:N].clone() if cur_nodes is None else torch.from_numpy(np.ascontiguousarray(cur_nodes, np.int32)).to(dev)
    lim = None if n_limit is None else torch.from_numpy(np.ascontiguousarray(n_limit, np.int32)).to(dev)
    choice, err = (torch.empty((n,), device=dev, dtype=torch.int32) for n in (N, 1))
    nodes = torch.empty((ctx.hops, N), device=dev, dtype=torch.int32) if advance else None
    mb, n_layers = ctx.micro_batch(N), (len(net.weights) - 1) // 3
    for h in range(ctx.hops):
        outs = []
        for c0 in range(0, x.shape[0] * NS, mb):                        # mb trajectories per launch; on field-of-view lists every launch
            last_c = last[c0:c0 + mb]                                   # computes what the readouts of its real trajectories can see
            activity = ops.field_activity(plan, last_c, min(int(last_c.shape[0]), N - c0), n_layers) if ctx.field else None
            if activity and ctx.fractions is not None:                  # (the lists follow `last` at every hop; x stays dense)
                ctx.fractions.append(activity["active_fraction"])
            outs.append(ops.forward_logp(plan, x[c0 // NS:(c0 + mb) // NS], last_c, net.weights, activity))
        logp = outs[0] if len(outs) == 1 else torch.cat(outs)
        rec = None if trace is None else (ops.slabs_to_batch(x, plan.layout, 1, N)[:, :, 0].cpu().numpy(), last[:N].cpu().numpy(),
                                          logp[:N].cpu().numpy())
        final = h == ctx.hops - 1
        lookup = advance or not final                                   # the accuracy's final hop looks nothing up (STM:121-122)
        err.fill_(INT32_MAX)
        cur_h = cur.cpu().numpy() if lookup else None
        check(ctx.lib.scn_hop_select(N, ctx.D, _p(logp), _p(lim), fill, tab.p_deg, _p(cur), _p(last), tab.n_nodes, tab.p_node,
                                     tab.p_edge if lookup else None, tab.p_sign, plan.n_edges, NS, None if final else _p(x),
                                     1 if (advance and not final) else 0, _p(choice), _p(nodes[h]) if advance else None, _p(err),
                                     ops._stream()), "scn_hop_select")
        if rec is not None:
            trace.append(rec + (choice.cpu().numpy(),))
        if lookup:
            i = int(err.item())
            if i != INT32_MAX:
                raise ctx.missing_edge(i, cur_h, choice=choice)
    return choice.cpu().numpy(), (nodes.cpu().numpy().astype(np.int64) if advance else None)


# ------------------------------------------------------------------ probability tree
def target_probs(net, inputs, target_nodes, nbrhoods, E_lookup, last_nodes, hops):
    """Scone_GCN.multi_hop_target_probs: every path a leaf of its own; the last level is forwarded, never expanded, then reduced."""
    ctx = Call(net, inputs, hops, "dist", nbrhoods, E_lookup, ("last_nodes and target_nodes", last_nodes, target_nodes))
    plan, tab, lib, N, D, dev = ctx.plan, ctx.tab, ctx.lib, ctx.N, ctx.D, ctx.dev
    lv = root_level(N, last_nodes, dev, score=1.0)
    err = torch.empty((1,), device=dev, dtype=torch.int32)
    for h in range(ctx.hops):
        L = int(lv.root.shape[0])
        logp = ctx.level_logp(lv)
        if h == ctx.hops - 1:
            break
        cnt = tab.deg[lv.node.long()]
        offset = (torch.cumsum(cnt, 0) - cnt).to(torch.int32)
        C = int(cnt.sum().item())                                     # the one copy back per level: the next level's size
        if C >= INT32_MAX // max(D, 1):
            raise ValueError("tree level of %d leaves is too large" % C)
        kids = ctx.children(C, h)
        err.fill_(INT32_MAX)
        check(lib.scn_tree_expand(L, h, D, _p(lv.root), _p(lv.node), _p(lv.score), _p(lv.path_row) if h else None,
                                  _p(lv.path_sign) if h else None, _p(logp), _p(offset), tab.p_deg, tab.n_nodes, tab.p_node, tab.p_edge,
                                  tab.p_sign, plan.n_edges, C, _p(kids.root), _p(kids.node), _p(kids.score), _p(kids.path_row),
                                  _p(kids.path_sign), _p(err), ops._stream()), "scn_tree_expand")
        t = int(err.item())
        if t != INT32_MAX:
            raise ctx.missing_edge(t, lv.node, sort=True)
        lv = kids
    leaf_ptr = torch.searchsorted(lv.root, torch.arange(N + 1, device=dev, dtype=torch.int32)).to(torch.int32)
    target = torch.from_numpy(np.ascontiguousarray(np.asarray(target_nodes).reshape(-1), np.int32)).to(dev)
    out = torch.empty((N,), device=dev, dtype=torch.float32)
    check(lib.scn_tree_target(N, _p(leaf_ptr), _p(lv.node), _p(lv.score), _p(logp), D, tab.p_deg, tab.n_nodes, tab.p_node, _p(target),
                              _p(out), ops._stream()), "scn_tree_target")
    return out.cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------ beam search
def beam_paths(net, inputs, hops, beam, nbrhoods=None, E_lookup=None):
    """Scone_GCN.predict_paths_beam: level h holds W_h entries per trajectory, scn_beam_step keeps the best W_{h+1} children."""
    hops, beam = int(hops), int(beam)
    ctx = Call(net, inputs, hops, "binary", nbrhoods, E_lookup, ("last nodes", inputs[1]), defaults=True,
               refuse=[(lambda: beam < 1 or beam > _lib.SCN_BEAM_MAX, "beam must be between 1 and %d (SCN_BEAM_MAX)" % _lib.SCN_BEAM_MAX)])
    plan, tab, N, D, dev, trace = ctx.plan, ctx.tab, ctx.N, ctx.D, ctx.dev, ctx.trace
    if N * beam * D >= INT32_MAX:
        raise ValueError("beam level of %d x %d entries is too large" % (N, beam))
    lv, W = root_level(N, inputs[1], dev), 1
    err = torch.full((hops,), INT32_MAX, device=dev, dtype=torch.int32)
    levels, widths = [lv], [W]
    for h in range(hops):
        logp = ctx.level_logp(lv, dead=True)
        W2 = min(beam, W * D)
        kids = ctx.children(N * W2, h, final=h == hops - 1, links=True)
        check(ctx.lib.scn_beam_step(N, W, W2, h, D, _p(lv.node), _p(lv.score), _p(lv.path_row) if h else None,
                                    _p(lv.path_sign) if h else None, _p(logp), tab.p_deg, tab.n_nodes, tab.p_node, tab.p_edge, tab.p_sign,
                                    plan.n_edges, _p(kids.root), _p(kids.node), _p(kids.score), _p(kids.parent), _p(kids.slot),
                                    _p(kids.path_row), _p(kids.path_sign), _p(err[h:]), ops._stream()), "scn_beam_step")
        if trace is not None:
            trace.append({"node": lv.node.view(N, W).cpu().numpy(), "score": lv.score.view(N, W).cpu().numpy(),
                          "logp": logp.view(N, W, D).cpu().numpy(), "parent": kids.parent.view(N, W2).cpu().numpy(),
                          "slot": kids.slot.view(N, W2).cpu().numpy()})
        levels.append(kids)
        widths.append(W2)
        lv, W = kids, W2
    ctx.raise_first_missing_edge(err, levels)
    # node paths from the per-level parents, on the device: walk every final entry back to its root
    dead = lv.node.view(N, W) < 0
    k = torch.arange(W, device=dev).expand(N, W)
    steps = []
    for level, w in zip(levels[:0:-1], widths[:0:-1]):
        steps.append(torch.gather(level.node.view(N, w), 1, k))
        k = torch.gather(level.parent.view(N, w), 1, k).clamp(min=0).long()
    paths = torch.stack(steps[::-1], dim=2).long().masked_fill(dead[:, :, None], -1)
    out_paths, out_logp = np.full((N, beam, hops), -1, np.int64), np.full((N, beam), -np.inf, np.float64)
    out_paths[:, :W] = paths.cpu().numpy()
    out_logp[:, :W] = lv.score.view(N, W).cpu().numpy()
    return out_paths, out_logp


# ------------------------------------------------------------------ sampled paths
def sample_levels(net, inputs, hops, n_samples, seed, temperature, nbrhoods, E_lookup):
    """The sampled decoder's levels on the device.  A level keeps one entry per distinct path with the number of samples on it
    (the probability tree's layout: entries sorted by trajectory, leaf_ptr); one batched forward over the entries
    (Call.level_logp), then scn_sample_draw picks every sample's slot inside the entry it sits in and scn_sample_expand
    merges equal picks into one child (include/scone_hip.h) -- sample by sample what n_samples independent chains give, at the
    cost of the distinct paths.  One size copy back per level; the error words of all levels are read once, at the end.
    Returns the Level records of levels 0 .. hops (level 0 = the roots), each with its leaf_ptr, count and entry_of."""
    hops, S = int(hops), int(n_samples)
    ctx = Call(net, inputs, hops, "binary", nbrhoods, E_lookup, ("last nodes", inputs[1]), defaults=True,
               refuse=[(lambda: S < 1 or S > _lib.SCN_SAMPLE_MAX, "n_samples must be between 1 and %d (SCN_SAMPLE_MAX)" % _lib.SCN_SAMPLE_MAX),
                       (lambda: not float(temperature) >= 0.0, "temperature must not be negative")])
    temperature = float(temperature)
    inv_T = float("inf") if temperature == 0.0 else float(np.float32(1.0) / np.float32(temperature))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    plan, tab, lib, N, D, dev, trace = ctx.plan, ctx.tab, ctx.lib, ctx.N, ctx.D, ctx.dev, ctx.trace
    if S * D > _lib.SCN_SAMPLE_PAIRS_MAX or N * S * D >= INT32_MAX:
        raise ValueError("sampled level of %d x %d entries of %d slots is too large" % (N, S, D))
    lv = root_level(N, inputs[1], dev)._replace(count=torch.full((N,), S, device=dev, dtype=torch.int32),
                                                 leaf_ptr=torch.arange(N + 1, device=dev, dtype=torch.int32),
                                                 entry_of=torch.zeros((N, S), device=dev, dtype=torch.int32))
    err = torch.full((hops,), INT32_MAX, device=dev, dtype=torch.int32)
    levels = [lv]
    for h in range(hops):
        L = int(lv.node.shape[0])
        if L == 0:                                                       # every sample has been dropped: the level stays empty
            levels.append(lv._replace(entry_of=torch.full_like(lv.entry_of, -1)))
            continue
        logp = ctx.level_logp(lv, dead=True)                             # (the samples of an entry on node -1 are dropped)
        pick, n_child = (torch.empty(shape, device=dev, dtype=torch.int32) for shape in ((N, S), (N,)))
        check(lib.scn_sample_draw(N, S, S, L, h, D, seed, inv_T, _p(lv.leaf_ptr), _p(lv.node), _p(logp), _p(lv.entry_of), tab.p_deg,
                                  tab.n_nodes, tab.p_node, tab.p_edge, plan.n_edges, _p(pick), _p(n_child), _p(err[h:]), ops._stream()),
              "scn_sample_draw")
        child_ptr = torch.zeros((N + 1,), device=dev, dtype=torch.int32)
        child_ptr[1:] = torch.cumsum(n_child, 0)
        C = int(child_ptr[-1].item())                                    # the one copy back per level: the next level's size
        kids = ctx.children(C, h, final=h == hops - 1, links=True, count=True)._replace(
            leaf_ptr=child_ptr, entry_of=torch.empty((N, S), device=dev, dtype=torch.int32))
        check(lib.scn_sample_expand(N, S, S, L, h, D, _p(lv.leaf_ptr), _p(lv.node), _p(lv.score), _p(lv.path_row) if h else None,
                                    _p(lv.path_sign) if h else None, _p(logp), _p(pick), _p(child_ptr), C, tab.n_nodes, tab.p_node,
                                    tab.p_edge, tab.p_sign, _p(kids.root), _p(kids.node), _p(kids.score), _p(kids.parent), _p(kids.slot),
                                    _p(kids.count), _p(kids.path_row), _p(kids.path_sign), _p(kids.entry_of), ops._stream()),
              "scn_sample_expand")
        if trace is not None:
            trace.append({"leaf_ptr": lv.leaf_ptr.cpu().numpy(), "node": lv.node.cpu().numpy(), "score": lv.score.cpu().numpy(),
                          "count": lv.count.cpu().numpy(), "logp": logp.cpu().numpy(), "entry_of": lv.entry_of.cpu().numpy(),
                          "pick": pick.cpu().numpy(), "child_ptr": child_ptr.cpu().numpy(), "parent": kids.parent.cpu().numpy(),
                          "slot": kids.slot.cpu().numpy(), "child_count": kids.count.cpu().numpy()})
        levels.append(kids)
        lv = kids
    ctx.raise_first_missing_edge(err, levels)
    return levels


def _entry_at(lv, values, missing):
    """values[the entry every sample of lv sits on] [N, S] (`missing` where the level is empty; dropped samples read entry 0)."""
    at, n = lv.leaf_ptr[:-1, None].long() + lv.entry_of.clamp(min=0).long(), int(values.shape[0])
    return values[at.clamp(max=n - 1)] if n else torch.full_like(at, missing, dtype=values.dtype)


def sample_paths(net, inputs, hops, n_samples, seed, temperature, nbrhoods, E_lookup):
    """Scone_GCN.sample_paths: the levels, then every sample's path and score gathered on the device, one copy at the end."""
    levels = sample_levels(net, inputs, hops, n_samples, seed, temperature, nbrhoods, E_lookup)
    dead = levels[-1].entry_of < 0
    paths = torch.stack([_entry_at(lv, lv.node.long(), -1) for lv in levels[1:]], dim=2).masked_fill(dead[:, :, None], -1)
    lp = _entry_at(levels[-1], levels[-1].score.double(), 0.0).masked_fill(dead, float("-inf"))
    return paths.cpu().numpy(), lp.cpu().numpy()


def sample_end_counts(net, inputs, hops, n_samples, seed, temperature):
    """Per distinct (trajectory, end node) of the final level the number of samples there: (trajectory [M], node [M],
    samples [M]) int64 device tensors, sorted by trajectory, then node."""
    end = sample_levels(net, inputs, hops, n_samples, seed, temperature, None, None)[-1]
    leaf_ptr, node, count = end.leaf_ptr, end.node, end.count
    N = int(leaf_ptr.shape[0]) - 1
    V = int(node.max().item()) + 2 if node.shape[0] else 1
    root = torch.repeat_interleave(torch.arange(N, device=node.device), (leaf_ptr[1:] - leaf_ptr[:-1]).long())
    live = node >= 0
    key, inv = torch.unique(root[live] * V + node[live].long(), return_inverse=True)
    total = torch.zeros(key.shape, device=node.device, dtype=torch.int64).index_add_(0, inv, count[live].long())
    return torch.div(key, V, rounding_mode="floor"), key % V, total


def reach_probs(net, inputs, hops, n_samples, seed, temperature):
    """Scone_GCN.multi_hop_reach_probs, from the final level's entries and counts."""
    r, v, c = sample_end_counts(net, inputs, hops, n_samples, seed, temperature)
    N = int(np.asarray(inputs[1]).reshape(-1).shape[0])
    order = torch.sort(-c, stable=True)[1]                                # (r, v) ascending already; stable sorts keep the ties
    order = order[torch.sort(r[order], stable=True)[1]]
    r, v, c = r[order].cpu().numpy(), v[order].cpu().numpy(), c[order].cpu().numpy()
    start = np.searchsorted(r, np.arange(N))
    K = int(np.bincount(r, minlength=N).max()) if len(r) else 0
    nodes, freq = np.full((N, K), -1, np.int64), np.zeros((N, K), np.float64)
    col = np.arange(len(r)) - start[r]
    nodes[r, col], freq[r, col] = v, c / np.float64(int(n_samples))
    return nodes, freq


def target_probs_sampled(net, inputs, target_nodes, hops, n_samples, seed):
    """Scone_GCN.multi_hop_target_probs_sampled: the share of every trajectory's samples that end at its target."""
    r, v, c = (t.cpu().numpy() for t in sample_end_counts(net, inputs, hops, n_samples, seed, 1.0))
    target = np.asarray(target_nodes).reshape(-1)
    N = int(np.asarray(inputs[1]).reshape(-1).shape[0])
    if len(target) != N:
        raise ValueError("target_nodes needs one entry per trajectory of inputs (%d)" % N)
    hit = np.zeros(N, np.int64)
    m = v == target[r]
    hit[r[m]] = c[m]
    return hit / np.float64(int(n_samples))
