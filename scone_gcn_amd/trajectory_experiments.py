"""Host-side mirror of the reference's model functions and experiment driver
(trajectory_analysis/trajectory_experiments.py = TE).

Same names, argument order and error behaviour as the reference's call surface for the hot path:
    scone_func(weights, S_lower, S_upper, Bcond_func, last_node, flow)                    TE:137-152
    ebli_func (weights, S_lower, S_upper, Bcond_func, last_node, flow)                    TE:155-170
    bunch_func(weights, S_00, S_10, S_01, S_11, S_21, S_12, S_22, nbrhoods, last_node, flow)   TE:173-203
    hyperparams(), data_setup(), train_model()                                            TE:78-117, 206-311, 313-510
The functions are batched natively (the reference wraps them in vmap, STM:256): last_node (N,), flow (N, E, 1)
or SparseFlows -> log-probabilities (N, D, 1).  Per-sample arguments (scalar last_node, flow (E, 1)) work too
and return (D, 1).  All math runs in libscone_hip.so on the current CUDA (ROCm) device; nothing falls back to CPU.
"""
import os
import sys

import numpy as np
import torch

from . import ops
from .complex import Bconds, Shift, SimplicialComplex, adopt_bconds, adopt_shift, identity_layout
from .synthetic_data_gen import SparseFlows

MODEL_ACT = {"scone": "tanh", "ebli": "leaky_relu", "bunch": "relu"}


def hyperparams(args=None):
    """Parse `-name value` flags with the reference's names and defaults (TE:78-117)."""
    args = sys.argv if args is None else args
    hp = {'model': 'scone', 'epochs': 1000, 'learning_rate': 0.001, 'weight_decay': 0.00005, 'batch_size': 100,
          'hidden_layers': [(3, 16), (3, 16), (3, 16)], 'describe': 1, 'reverse': 0, 'load_data': 1,
          'load_model': 0, 'markov': 0, 'model_name': 'model', 'regional': 0, 'flip_edges': 0,
          'data_folder_suffix': 'working', 'multi_graph': '', 'holes': 1,
          'skip_mode': 'dense',          # not in the reference: dense | zeros | field (exact zero-skipping, Scone_GCN)
          'multi_hop': 0,                # 1: the 2-hop probability-tree accuracies (the reference's commented-out call, TE:508-510)
          'multi_hop_skip': 'dense',     # not in the reference: dense | field (field-of-view work lists for the multi-hop forwards)
          'beam': 0,                     # B > 0 with -multi_hop 1: also the 2-hop top-B accuracies of a beam search of width B
          'multi_hop_samples': 0,        # S > 0 with -multi_hop 1: also the mean 2-hop target probability estimated from S sampled paths
          'markov_order': 1,             # not in the reference (order = 1 is hard-coded, TE:329): the order K of the -markov 1 baseline
          'projection': 0,               # 1: the harmonic projection baseline's experiments first (the reference's projection_model.py)
          'path_likelihood': 0,          # not in the reference: 1 = after training, the teacher-forced scores of prefix + [target] (score_paths)
          'train_paths': 0,              # not in the reference: 1 = train on every (path, prefix) item of prefix + [target] (train_paths)
          'path_min_prefix': 2,          # ... the shortest prefix that is an item
          'path_weight': 'step',         # ... step | path: every item counts the same, or every path does
          'n_points': 400, 'n_walks': 1000,   # not in the reference (hard-coded, TE:224): the size of the -load_data 0 data set
          'walks': 'host',               # host | device: device = generate_random_walks_batched (fresh waypoints per walk on the GPU)
          'walk_metric': 'hops'}         # hops | euclid: the shortest-path metric of the generated walks
    for i in range(len(args) - 1):
        if args[i] and args[i][0] == '-':
            name = args[i][1:]
            if name == 'hidden_layers':
                nums = list(map(int, args[i + 1].split("_")))
                hp['hidden_layers'] = [(nums[j], nums[j + 1]) for j in range(0, len(nums), 2)]
            elif name in ['model_name', 'data_folder_suffix', 'multi_graph', 'model', 'skip_mode', 'multi_hop_skip', 'walks',
                          'walk_metric', 'path_weight']:
                hp[name] = str(args[i + 1])
            else:
                try:
                    hp[name] = float(args[i + 1])
                except ValueError:
                    pass
    return hp


HYPERPARAMS = hyperparams([])


# ----------------------------------------------------------------------------------------------
# model functions
# ----------------------------------------------------------------------------------------------

def _prep_batch(last_node, flow):
    single = False
    if isinstance(flow, SparseFlows):
        ln = np.atleast_1d(np.asarray(last_node.cpu() if torch.is_tensor(last_node) else last_node))
        return ln, flow, single
    f = flow if torch.is_tensor(flow) else np.asarray(flow)
    if f.ndim == 2:                                   # per-sample call: flow (E, 1), scalar last_node
        single = True
        f = f[None]
    ln = np.atleast_1d(np.asarray(last_node.cpu() if torch.is_tensor(last_node) else last_node))
    return ln, f, single


def _run_batched(plan, weights, last_nodes, flow):
    device = plan.device
    w = ops.as_device_weights(weights, device)
    x, N = ops.flows_to_slabs(flow, plan.layout, device)
    if len(last_nodes) != N:
        raise ValueError("last_node and flow disagree on the number of trajectories")
    last_dev = ops._last_nodes_dev(last_nodes, x.shape[0] * ops.NS, device)
    sl = ops.forward_micro_batch(plan, w, N) // ops.NS
    outs = []
    for s0 in range(0, x.shape[0], sl):
        outs.append(ops.PlanFn.apply(plan, x[s0:s0 + sl], last_dev[s0 * ops.NS:(s0 + sl) * ops.NS], *w))
    logp = torch.cat(outs) if len(outs) > 1 else outs[0]
    return logp[:N].unsqueeze(-1)


def resolve_operands(model_type, shifts, readout):
    """Native operands for what a caller passed: Shift / Bconds objects go through untouched; dense ndarrays, torch tensors
    or scipy matrices (the reference's L1_lower, L1_upper, S_ab -- TE:240-257) and a plain Bcond_func closure (TE:298-303)
    are wrapped once and cached on the object (small complexes; identity row order)."""
    shifts = list(shifts)
    if all(isinstance(m, Shift) for m in shifts):
        layout = shifts[0].layout
    elif model_type == 'bunch':
        sizes = (shifts[0].shape[0], shifts[3].shape[0], shifts[6].shape[0])          # S_00 (V,V), S_11 (E,E), S_22 (F,F)
        layout = next((m.layout for m in shifts if isinstance(m, Shift)), None) or identity_layout(sizes)
        lv = [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (2, 1), (2, 2)]
        shifts = [adopt_shift(m, layout, r, c) for m, (r, c) in zip(shifts, lv)]
    else:
        E = shifts[0].shape[0]
        layout = next((m.layout for m in shifts if isinstance(m, Shift)), None) or identity_layout((1, E, 1))
        shifts = [adopt_shift(m, layout, 1, 1) for m in shifts]
    if model_type == 'bunch':
        return shifts, np.asarray(readout.cpu() if torch.is_tensor(readout) else readout)
    return shifts, adopt_bconds(readout, shifts[0].shape[0], layout)


def _scone_like(weights, S_lower, S_upper, Bcond_func, last_node, flow, act):
    n_layers = (len(weights) - 1) / 3
    assert n_layers % 1 == 0, 'wrong number of weights'                    # TE:141-142 / 159-160
    (S_lower, S_upper), bconds = resolve_operands('scone', [S_lower, S_upper], Bcond_func)
    plan = ops.get_scone_plan(S_lower, S_upper, bconds, act, ops.default_device())
    ln, f, single = _prep_batch(last_node, flow)
    ln = ops.remap_last_nodes(plan, ln)
    out = _run_batched(plan, weights, ln, f)
    return out[0] if single else out


def scone_func(weights, S_lower, S_upper, Bcond_func, last_node, flow):
    """Forward pass of the SCoNe model with variable number of layers (TE:137-152); tanh activation."""
    return _scone_like(weights, S_lower, S_upper, Bcond_func, last_node, flow, "tanh")


def ebli_func(weights, S_lower, S_upper, Bcond_func, last_node, flow):
    """Forward pass of the Ebli (SNN) model (TE:155-170); leaky_relu(0.01) activation."""
    return _scone_like(weights, S_lower, S_upper, Bcond_func, last_node, flow, "leaky_relu")


def bunch_func(weights, S_00, S_10, S_01, S_11, S_21, S_12, S_22, nbrhoods, last_node, flow):
    """Forward pass of the Bunch (SCCONV) model (TE:173-203); relu on all three levels."""
    n_layers = (len(weights)) / 7
    assert n_layers % 1 == 0, 'wrong number of weights'                    # TE:177-178
    shifts, nbrhoods = resolve_operands('bunch', [S_00, S_10, S_01, S_11, S_21, S_12, S_22], nbrhoods)
    plan = ops.get_bunch_plan(shifts, nbrhoods, ops.default_device())
    ln, f, single = _prep_batch(last_node, flow)
    out = _run_batched(plan, weights, ln, f)
    return out[0] if single else out


MODEL_FUNCS = {"scone": scone_func, "ebli": ebli_func, "bunch": bunch_func}


# ----------------------------------------------------------------------------------------------
# data setup (TE:206-311) on an in-memory or on-disk dataset
# ----------------------------------------------------------------------------------------------

def setup_from_complex(sc, model='scone', flip_edges=False, flips=None):
    """shifts + readout operand for a SimplicialComplex (TE:214-219, 240-260, 270-309).  flips: an explicit +-1 vector
    (data_setup draws it from the trainer's global stream like the reference); flip_edges=True draws it under seed 1."""
    if flips is None:
        flips = sc.flip_vector(1) if flip_edges else None
    if model == 'scone':
        shifts = sc.scone_shifts(flips)
    elif model == 'ebli':
        shifts = sc.ebli_shifts(flips)
    elif model == 'bunch':
        shifts = sc.bunch_shifts()
    else:
        raise Exception('invalid model type')                              # TE:260
    readout = sc.nbrhoods if model == 'bunch' else sc.bconds(flips)        # TE:305-309
    return shifts, readout, flips


def apply_flips(flows, flips):
    """X -> X F (TE:292-296)."""
    if flips is None:
        return flows
    if isinstance(flows, SparseFlows):
        return SparseFlows(flows.ptr, flows.idx, (flows.val * flips[flows.idx]).astype(np.float32), flows.n_edges)
    return np.asarray(flows) * np.asarray(flips).reshape(1, -1, 1)


def data_setup(hops=(1,), load=True, folder_suffix='schaub', hp=None):
    """Imports and sets up flow, target, and shift matrices for model training (TE:206-311).  Returns the reference's
    eleven values (TE:311): inputs_all, y_all, train_mask, test_mask, shifts, G_undir, E_lookup, nbrhoods, n_nbrs,
    target_nodes_all, prefixes -- shifts as sparse Shift objects and Bconds_func as a Bconds object (both also answer the
    dense questions the reference asks of them: .shape, @, .toarray(), Bconds_func(n))."""
    from .complex import UndirGraph
    from .dataset_io import load_dataset, generate_dataset, load_prefixes
    from .synthetic_data_gen import flow_to_path
    hp = HYPERPARAMS if hp is None else hp
    if hp['flip_edges']:                                                   # TE:214-219: the GLOBAL stream is reseeded with 1 and
        from . import scone_trajectory_model as stm                        # the flips are drawn from it, so the weights drawn
        stm.reseed(1)                                                      # afterwards (STM:237) continue that stream
    if not load:
        generate_dataset(int(hp.get('n_points', 400)), int(hp.get('n_walks', 1000)), folder=folder_suffix, holes=bool(hp['holes']),
                         walks=hp.get('walks', 'host'), metric=hp.get('walk_metric', 'hops'))
        raise Exception('Data generation done')                            # TE:225
    inputs_all, y_all, target_nodes_all = [], [], []
    sc = None
    for h in hops:
        folder = 'trajectory_data_' + str(h) + 'hop_' + folder_suffix
        X, (B1, B2), y, train_mask, test_mask, coords, last_nodes, target_nodes = load_dataset(folder)
        if sc is None:
            sc = SimplicialComplex.from_incidence(B1, B2, coords=coords)
        target_nodes_all.append(target_nodes)
        inputs_all.append([None, np.array(last_nodes), X])
        y_all.append(y)
    flips = None
    if hp['flip_edges']:
        from . import scone_trajectory_model as stm
        flips = stm._RNG.choice([1, -1], size=sc.cx.n_edges, replace=True, p=[0.8, 0.2]).astype(np.float64)
    shifts, readout, flips = setup_from_complex(sc, hp['model'], flips=flips)
    for i in range(len(inputs_all)):
        inputs_all[i][-1] = apply_flips(inputs_all[i][-1], flips)
        inputs_all[i][0] = readout
    last_nodes = inputs_all[0][1]
    n_nbrs = sc.n_nbrs(last_nodes)
    edges = [tuple(e) for e in sc.cx.edges.tolist()]
    E_lookup = {e: i for i, e in enumerate(edges)}                          # TE:263-268
    prefixes = load_prefixes('trajectory_data_1hop_' + folder_suffix)      # TE:281-284
    if prefixes is None:
        X0 = inputs_all[0][-1]
        dense = X0.todense() if isinstance(X0, SparseFlows) else np.asarray(X0)
        if flips is not None:
            dense = dense * flips.reshape(1, -1, 1)                         # undo X F: paths live on the unflipped orientation
        prefixes = [flow_to_path(dense[i], edges, last_nodes[i]) for i in range(len(last_nodes))]
    return inputs_all, y_all, train_mask, test_mask, shifts, UndirGraph(sc), E_lookup, sc.nbrhoods, n_nbrs, \
        target_nodes_all, prefixes


def markov_baseline(order, seed=0, backoff=False, min_count=1):
    """The count-table baseline of the -markov flags: markov_model.Markov_Model(order), or with -markov_backoff 1 the variable-order
    markov_model.Markov_Backoff(order as the maximum, min_count), which predicts from the longest context it has seen."""
    from . import markov_model
    if backoff:
        return markov_model.Markov_Backoff(order, seed=seed, backoff=True, min_count=min_count)
    return markov_model.Markov_Model(order, seed=seed)


def markov_rule(hp):
    """The keyword arguments -markov_backoff 1 [-markov_min_count C] add to markov_baseline and markov_experiments; none with the flag
    off, whatever the count says."""
    if hp.get('markov_backoff', 0) != 1:
        return {}
    return {"backoff": True, "min_count": int(hp.get('markov_min_count', 1))}


def markov_experiments(G_undir, prefixes, target_nodes_all, train_mask, test_mask, order=1, seed=0, backoff=False, min_count=1):
    """The Markov baseline's five experiments (TE:327-432) with the reference's masks and print labels, on the device
    (markov_baseline: markov_model.Markov_Model of the given order, or Markov_Backoff up to it).  The mixed experiment's forward /
    backward mask is shuffled by the trainer's
    global stream (scone_trajectory_model._RNG), where the reference uses NumPy's.  Returns {label: [accuracies in print order]}."""
    from . import scone_trajectory_model as stm
    markov = markov_baseline(order, seed, backoff, min_count)
    prefixes = [[int(v) for v in p] for p in prefixes]
    t1, t2 = (np.asarray(t).astype(np.int64) for t in target_nodes_all[:2])
    train_mask, test_mask = np.asarray(train_mask), np.asarray(test_mask)
    n = len(prefixes)
    paths = [p + [int(a), int(b)] for p, a, b in zip(prefixes, t1, t2)]            # TE:331
    pick = lambda seq, mask: [seq[i] for i in np.flatnonzero(np.asarray(mask))]
    results = {}

    def report(label, rows):
        print(label)
        results[label] = [float(r) for r in rows]
        for r in rows:
            print(r)

    def accs(pre, a, b, mask, two_target=False):
        pre, a, b = pick(pre, mask), np.asarray(pick(a, mask)), np.asarray(pick(b, mask))
        return [markov.test(pre, a, 1), markov.test(pre, b, 2)] + ([markov.test_2_target(pre, a)] if two_target else [])

    # forward paths (TE:341-350)
    markov.train(G_undir, pick(paths, train_mask == 1))
    report("train accs", accs(prefixes, t1, t2, train_mask == 1, True))
    report("test accs", accs(prefixes, t1, t2, test_mask == 1, True))
    # reversed test paths (TE:354-364)
    rev_paths = [p[::-1] for p in paths]
    rev_prefixes = [p[:-2] for p in rev_paths]
    rev_t1, rev_t2 = np.asarray([p[-2] for p in rev_paths]), np.asarray([p[-1] for p in rev_paths])
    report("Reversed test accs", accs(rev_prefixes, rev_t1, rev_t2, test_mask == 1))
    # half forward, half backward (TE:366-392)
    fwd_mask = np.array([True] * int(n / 2) + [False] * int(n / 2))
    stm._RNG.shuffle(fwd_mask)
    fwd, bkwd = np.flatnonzero(fwd_mask), np.flatnonzero(~fwd_mask)
    mixed_paths = [paths[i] for i in fwd] + [rev_paths[i] for i in bkwd]
    mixed_prefixes = [prefixes[i] for i in fwd] + [rev_prefixes[i] for i in bkwd]
    mixed_t1, mixed_t2 = np.concatenate((t1[fwd], rev_t1[bkwd])), np.concatenate((t2[fwd], rev_t2[bkwd]))
    m = len(mixed_paths)                                                           # n - 1 for an odd n, where the reference's masks misfit
    markov.train(G_undir, pick(mixed_paths, train_mask[:m] == 1))
    report("Mixed train accs", accs(mixed_prefixes, mixed_t1, mixed_t2, train_mask[:m] == 1))
    report("Mixed test accs", accs(mixed_prefixes, mixed_t1, mixed_t2, test_mask[:m] == 1))
    # train on middle, test on middle (TE:394-412)
    third = np.arange(n) % 3
    mid_train, mid_test = (third == 0) & (train_mask == 1), (third == 0) & (test_mask == 1)
    markov.train(G_undir, pick(paths, mid_train))
    report("Middle region train accs", accs(prefixes, t1, t2, mid_train))
    report("Middle region test accs", accs(prefixes, t1, t2, mid_test))
    # train on upper, test on lower (TE:415-432)
    markov.train(G_undir, pick(paths, third == 1))
    report("Upper region train accs", accs(prefixes, t1, t2, third == 1))
    report("Lower region accs", accs(prefixes, t1, t2, third == 2))
    return results


def projection_experiments(sc, folder, seed=0, pm=None):
    """The harmonic projection baseline's experiments (the reference's projection_model.py, PM:215-227) with its print labels, on
    the device (projection_model.Projection_Model): standard test set, reversed test set when the folder has the rev_* files,
    2-target, transfer (rows i % 3 == 2).  The data set is read again, as PM reads it itself: the baseline works on the unflipped
    flows whatever -flip_edges says (the result does not depend on the flips).  The basis is computed once, or taken from pm, a
    Projection_Model already embedded in sc.  Returns
    {"standard": (loss, acc), "reverse": (loss, acc), "two_target": acc, "two_target_slots": drawn slots, "transfer": (loss, acc),
    "dim", "iterations", "residual"}."""
    from .dataset_io import load_dataset, load_reverse
    from .projection_model import Projection_Model
    X, _, y, _, test_mask, _, last_nodes, _ = load_dataset(folder)
    last_nodes, test_mask = np.asarray(last_nodes), np.asarray(test_mask)
    pm = Projection_Model(seed=seed).embed(sc) if pm is None else pm
    results = {"dim": pm.dim, "iterations": pm.iterations, "residual": pm.residual}
    results["standard"] = pm.test(X, last_nodes, y, test_mask)
    print('Standard experiment loss / acc:', results["standard"])
    if all(os.path.exists(os.path.join(folder, f)) for f in ('rev_targets.npy', 'rev_last_nodes.npy')) and \
            any(os.path.exists(os.path.join(folder, 'rev_flows_in' + ext)) for ext in ('.npy', '.npz')):
        rev_flows, rev_targets, rev_last_nodes = load_reverse(folder)
        results["reverse"] = pm.test(rev_flows, rev_last_nodes, rev_targets, test_mask)
        print('Reverse experiment loss / acc:', results["reverse"])
    rows = np.flatnonzero(test_mask == 1)
    results["two_target"], results["two_target_slots"] = pm.test_2_target(pm._select(X, rows), last_nodes[rows], np.asarray(y)[rows],
                                                                          sc.n_nbrs(last_nodes[rows]), seed=seed)
    print('2-target acc:', results["two_target"])
    regional_mask = np.array([1 if i % 3 == 2 else 0 for i in range(len(last_nodes))])
    results["transfer"] = pm.test(X, last_nodes, y, regional_mask)
    print('Transfer experiment loss / acc:', results["transfer"])
    return results


def train_model(hp=None):
    """Trains a model to predict the next node in each input path (TE:313-510).  With -markov 1 the k-th order Markov baseline
    (-markov_order K, default 1) runs its five experiments first (TE:327-432) and its accuracies go to
    experiment_results["markov"]; with -markov_backoff 1 (default 0) the baseline is the variable-order Markov_Backoff instead: K (up to
    8) is then the maximum order, every prediction takes the longest context seen at least -markov_min_count C (default 1) times, and
    the path likelihood's results gain order_hist, the items per order used.  The reference then stops (`raise Exception`, TE:433);
    this driver does not: it goes on to
    train the model.  With -projection 1 the harmonic projection baseline runs next (projection_experiments) and its results go to
    experiment_results["projection"]; training follows as well.  With -path_likelihood 1 the trained model scores every path
    prefixes[i] + [target_nodes_all[0][i]] step by step (Scone_GCN.score_paths) over the train and the test mask:
    experiment_results["path_likelihood"] = {"train": ..., "test": ...}; with -markov 1 and / or -projection 1 beside it, the same
    items are scored by a Markov_Model(-markov_order) trained on the train mask's paths (additive smoothing -markov_alpha, default 1)
    and by the projection (Markov_Model.score_paths, Projection_Model.score_paths): experiment_results["path_likelihood_markov"] /
    ["path_likelihood_projection"], same layout.  With -train_paths 1 (-path_min_prefix, -path_weight) the
    model is trained on every (path, prefix) item of those same paths (Scone_GCN.train_paths) in place of train(); the losses and
    accuracies returned are then test()'s on the two masks, and everything after training runs as before."""
    from .scone_trajectory_model import Scone_GCN
    hp = hyperparams() if hp is None else hp
    inputs_all, y_all, train_mask, test_mask, shifts, G_undir, E_lookup, nbrhoods, n_nbrs, target_nodes_all, prefixes = \
        data_setup(hops=(1, 2), load=hp['load_data'], folder_suffix=hp['data_folder_suffix'], hp=hp)
    (inputs_1hop, inputs_2hop), (y_1hop, y_2hop) = inputs_all, y_all
    in_axes = tuple(([None] * len(shifts)) + [None, None, 0, 0])          # TE:325
    markov_results = None
    rule = markov_rule(hp)
    if hp.get('markov', 0) == 1:                                           # TE:327-432
        markov_results = markov_experiments(G_undir, prefixes, target_nodes_all, train_mask, test_mask,
                                            order=int(hp.get('markov_order', 1)), **rule)
    projection_results = projection = None
    if hp.get('projection', 0) == 1:                                       # the reference's projection_model.py, PM:215-227
        from .projection_model import Projection_Model
        projection = Projection_Model(seed=0).embed(G_undir.complex)       # one basis: the experiments' and the path likelihood's
        projection_results = projection_experiments(G_undir.complex, 'trajectory_data_1hop_' + hp['data_folder_suffix'], pm=projection)
    scone = Scone_GCN(hp['epochs'], hp['learning_rate'], hp['batch_size'], hp['weight_decay'],
                      skip_mode=hp.get('skip_mode', 'dense'), multi_hop_skip=hp.get('multi_hop_skip', 'dense'))
    if hp['model'] not in MODEL_FUNCS:
        raise Exception('invalid model')                                   # TE:445
    model_func = MODEL_FUNCS[hp['model']]
    scone.setup(model_func, hp['hidden_layers'], shifts, inputs_1hop, y_1hop, in_axes, train_mask,
                model_type=hp['model'])
    if hp['regional']:                                                     # TE:449-453
        train_mask = np.array([1 if i % 3 == 1 else 0 for i in range(len(y_1hop))])
        test_mask = np.array([1 if i % 3 == 2 else 0 for i in range(len(y_1hop))])
    if hp['describe'] == 1:                                                # TE:456-461
        print('Graph nodes: {}, edges: {}, avg degree: {}'.format(len(G_undir.nodes), len(G_undir.edges),
                                                                  np.average([G_undir.degree[node] for node in
                                                                              G_undir.nodes])))
        print('Training paths: {}, Test paths: {}'.format(train_mask.sum(), test_mask.sum()))
        print('Model: {}'.format(hp['model']))
    os.makedirs('models', exist_ok=True)
    path = os.path.join('models', hp['model_name'] + '.npz')
    train_paths = hp.get('train_paths', 0) == 1                            # not in the reference: every prefix of a path is an example

    def fit():
        if not train_paths:
            return scone.train(inputs_1hop, y_1hop, train_mask, test_mask, n_nbrs)
        whole = [[int(v) for v in pre] + [int(t)] for pre, t in zip(prefixes, target_nodes_all[0])]
        scone.train_paths(inputs_1hop, whole, train_mask, test_mask, min_prefix=int(hp.get('path_min_prefix', 2)),
                          weight=hp.get('path_weight', 'step'))
        return scone.test(inputs_1hop, y_1hop, train_mask, n_nbrs) + scone.test(inputs_1hop, y_1hop, test_mask, n_nbrs)
    if hp['load_model']:                                                   # TE:464-476
        scone.load_weights(path)
        if hp['epochs'] != 0:
            fit()
            scone.save_weights(path)
        (train_loss, train_acc), (test_loss, test_acc) = scone.test(inputs_1hop, y_1hop, train_mask, n_nbrs), \
            scone.test(inputs_1hop, y_1hop, test_mask, n_nbrs)
    else:
        train_loss, train_acc, test_loss, test_acc = fit()
        scone.save_weights(path)                                           # TE:482-486
    print('standard test set:')                                            # TE:489-494
    train_2target, test_2target = scone.two_target_accuracy(shifts, inputs_1hop, y_1hop, train_mask, n_nbrs), \
        scone.two_target_accuracy(shifts, inputs_1hop, y_1hop, test_mask, n_nbrs)
    scone.test(inputs_1hop, y_1hop, test_mask, n_nbrs)
    print('2-target accs:', train_2target, test_2target)
    results = {"train_2target": train_2target, "test_2target": test_2target,
               "log_probs": scone._predict(scone.weights, inputs_1hop).cpu().numpy()}      # final predictions, kept for inspection
    if hp['reverse']:                                                      # TE:497-504
        from .dataset_io import load_reverse
        rev_flows_in, rev_targets_1hop, rev_last_nodes = load_reverse('trajectory_data_1hop_' + hp['data_folder_suffix'])
        rev_n_nbrs = np.asarray([len(G_undir[n]) for n in rev_last_nodes])                # TE:501
        print('Reverse experiment:')
        # (as in the reference, the reversed flows are fed as stored -- NOT multiplied by F under -flip_edges, TE:499-504)
        rev_inputs = [inputs_1hop[0], rev_last_nodes, rev_flows_in]
        results["reverse"] = scone.test(rev_inputs, rev_targets_1hop, test_mask, rev_n_nbrs)
        results["reverse_log_probs"] = scone._predict(scone.weights, rev_inputs).cpu().numpy()
    if hp.get('multi_hop', 0):                                             # TE:508-510
        results["multi_hop"] = scone.multi_hop_accuracy_dist(shifts, inputs_1hop, target_nodes_all[1], [train_mask, test_mask],
                                                             nbrhoods, E_lookup, inputs_1hop[1], prefixes, 2)
        print('Multi hop accs:', results["multi_hop"])
        if int(hp.get('beam', 0)) > 0:                                     # not in the reference: is the target among the beam's end nodes
            results["multi_hop_topk"] = [scone.multi_hop_accuracy_topk(inputs_1hop, target_nodes_all[1], m, 2, int(hp['beam']))
                                         for m in (train_mask, test_mask)]
            print('Multi hop top-%d accs:' % int(hp['beam']), results["multi_hop_topk"])
        if int(hp.get('multi_hop_samples', 0)) > 0:                        # not in the reference: the share of sampled paths ending at the target (seed 0)
            tp = scone.multi_hop_target_probs_sampled(inputs_1hop, target_nodes_all[1], 2, int(hp['multi_hop_samples']))
            results["multi_hop_sampled"] = [float(np.average(tp[np.asarray(m) == 1])) for m in (train_mask, test_mask)]
            print('Multi hop sampled target probs (%d samples):' % int(hp['multi_hop_samples']), results["multi_hop_sampled"])
    if hp.get('path_likelihood', 0) == 1:                                  # not in the reference: how likely are the observed paths, step by step
        paths = [[int(v) for v in pre] + [int(t)] for pre, t in zip(prefixes, target_nodes_all[0])]
        results["path_likelihood"] = {name: scone.score_paths(inputs_1hop, paths, m) for name, m in (("train", train_mask), ("test", test_mask))}
        for name, r in results["path_likelihood"].items():
            print('Path likelihood ({}): mean step log-prob {:.6f} -- perplexity {:.4f} -- step acc {:.3f} -- steps {}'.format(
                name, r["mean_step_logp"], r["perplexity"], r["accuracy"], r["n_steps"]))
        masks = (("train", train_mask), ("test", test_mask))
        baselines = {}
        if hp.get('markov', 0) == 1:                                       # the count table of the train paths, smoothed (-markov_alpha)
            markov = markov_baseline(int(hp.get('markov_order', 1)), **rule)
            markov.train(G_undir, [paths[i] for i in np.flatnonzero(np.asarray(train_mask) == 1)])
            alpha = float(hp.get('markov_alpha', 1.0))
            baselines["markov"] = {name: markov.score_paths(paths, m, alpha=alpha) for name, m in masks}
        if projection is not None:
            baselines["projection"] = {name: projection.score_paths(paths, m) for name, m in masks}
        for which, res in baselines.items():
            results["path_likelihood_" + which] = res
            for name, r in res.items():
                print('Path likelihood, {} baseline ({}): mean step log-prob {:.6f} -- perplexity {:.4f} -- step acc {:.3f} -- steps {}'
                      .format(which, name, r["mean_step_logp"], r["perplexity"], r["accuracy"], r["n_steps"]))
                if "order_hist" in r:                                      # -markov_backoff 1: the items per order used, 0 .. K
                    print('    items per order used (0: none seen): {}'.format(r["order_hist"]))
    if markov_results is not None:
        results["markov"] = markov_results
    if projection_results is not None:
        results["projection"] = projection_results
    scone.experiment_results = results
    return scone, (train_loss, train_acc, test_loss, test_acc)


if __name__ == '__main__':
    train_model()
