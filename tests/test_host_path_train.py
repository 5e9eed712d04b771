"""Training on whole paths (Scone_GCN.path_grad_step / train_paths; scone_gcn_amd/path_train.py) without a GPU: this file's numpy
restatement of the contract of scn_path_stage (include/scone_hip.h; tests/test_gpu_path_train.py imports it as the reference of
the kernel), built on np_path_slabs and checked against brute force -- every column must be paths_to_flows of its prefix, every
last node the prefix's last, every target row the weighted one-hot of the neighbour slot the path takes next -- then the "path"
weights, the batches of an epoch, the export and the new switches of the driver.  The tests of the restatement alone
(test_restatement_*) exercise only this file's numpy and so do not depend on the feature: they validate the reference the GPU test
holds the kernel to.  Every other test here needs path_train.py, the export or the new keys."""
import ctypes
import os

import numpy as np
import pytest

from tests.test_host_path_scores import (INT32_MAX, check_columns, flow_tables, np_path_slabs, np_path_steps, random_walks, same_floats,
                                         tab_arrays, tiny_complex)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def np_path_stage(n_slabs, item_path, item_len, item_weight, ptr, nodes, slot, row, run, next_same, n_rows, d):
    """scn_path_stage on a buffer in any state: (x [n_slabs][n_rows][4][1] float32, last [4 n_slabs] int32, y [4 n_slabs][d]
    float32).  An item whose path lies outside [0, n_paths) or whose k lies outside [1, length] is guarded: an all-zero column,
    last node 0 and a zero row, like the padding behind the items."""
    ptr = np.asarray(ptr, np.int64)
    n_paths, n = len(ptr) - 1, len(item_path)
    assert n <= 4 * n_slabs
    valid = [bool(0 <= p < n_paths and 1 <= k <= ptr[p + 1] - ptr[p]) for p, k in zip(item_path, item_len)]
    # (a guarded item as the empty prefix of path 0: np_path_slabs writes nothing for a prefix of one node)
    ip = [int(p) if ok else 0 for p, ok in zip(item_path, valid)]
    il = [int(k) if ok else 1 for k, ok in zip(item_len, valid)]
    x = np_path_slabs(n_slabs, ip, il, ptr, row, run, next_same, n_rows)
    last = np.zeros(4 * n_slabs, np.int32)
    y = np.zeros((4 * n_slabs, d), np.float32)
    for i in range(n):
        if not valid[i]:
            continue
        t = int(ptr[ip[i]]) + il[i] - 1
        last[i] = nodes[t]
        if 0 <= slot[t] < d:
            y[i, slot[t]] = np.float32(1.0 if item_weight is None else item_weight[i])
    return x, last, y


def _stage_case(paths, min_prefix, flips=None, seed=0):
    """Every item of `paths` plus the prefixes that END their path, shuffled, through the restatement and against brute force."""
    from scone_gcn_amd import path_scores
    from scone_gcn_amd import synthetic_data_gen as g
    from scone_gcn_amd.trajectory_experiments import apply_flips
    cx, nb = tiny_complex()
    E, d = cx.n_edges, nb.shape[1]
    perm = np.random.RandomState(seed).permutation(E)
    deg, node, edge, sign = tab_arrays(flow_tables(cx, nb, perm, flips))
    ptr, nodes = path_scores.ragged(paths)
    st = np_path_steps(ptr, nodes, deg, node, edge, sign, E)
    assert st["err"] == INT32_MAX
    item_ptr, item_path, item_len = path_scores.path_items(ptr, min_prefix)
    lens = np.diff(ptr)
    whole = np.flatnonzero(lens >= 1)                                            # k == len: the prefix is the path, no target
    item_path = np.concatenate([item_path, whole, [len(paths) + 2, -1, 0]])      # ... and three guarded items (the last: k = 0)
    item_len = np.concatenate([item_len, lens[whole], [1, 1, 0]])
    rs = np.random.RandomState(seed + 1)
    order = rs.permutation(len(item_path))
    item_path, item_len = item_path[order], item_len[order]
    w = (0.25 + rs.randint(0, 8, size=len(item_path)) / 8.0).astype(np.float32)
    M = len(item_path)
    S = (M + 3) // 4 + 1                                                         # a slab of padding behind the items
    for weights in (None, w):
        x, last, y = np_path_stage(S, item_path, item_len, weights, ptr, nodes, st["slot"], st["row"], st["run"], st["next_same"], E, d)
        assert x.dtype == y.dtype == np.float32 and last.dtype == np.int32
        cols = x[:, :, :, 0].transpose(0, 2, 1).reshape(S * 4, E)
        n_no_target = 0
        for i, (p, k) in enumerate(zip(item_path, item_len)):
            want_y = np.zeros(d, np.float32)
            if not (0 <= p < len(paths)) or not (1 <= k <= len(paths[p])):
                assert not cols[i].any() and last[i] == 0 and not y[i].any()
                continue
            prefix = list(paths[p])[:k]
            want = apply_flips(g.paths_to_flows(cx, [prefix]), flips).todense()[0, :, 0]
            assert np.array_equal(cols[i][perm], want), (i, prefix)
            assert last[i] == prefix[-1]
            if k < len(paths[p]):
                want_y[list(nb[prefix[-1]]).index(paths[p][k])] = 1.0 if weights is None else weights[i]
            else:
                n_no_target += 1
            assert same_floats(y[i], want_y), (i, prefix)
        assert n_no_target == len(whole) > 0
        assert not cols[M:].any() and not last[M:].any() and not y[M:].any()
    return M


@pytest.mark.parametrize("flip", [False, True])
def test_restatement_matches_brute_force_on_the_four_node_graph(flip):
    cx, nb = tiny_complex()
    rs = np.random.RandomState(11)
    flips = np.array([1.0, -1.0, 1.0, -1.0, -1.0]) if flip else None
    paths = random_walks(nb, rs, 25, 12) + [[], [2], [0, 1, 0, 1, 2]]            # an empty path, a single node, a backtrack
    for min_prefix in (1, 2):
        assert _stage_case(paths, min_prefix, flips, seed=min_prefix) > 100


def test_restatement_x_is_np_path_slabs_for_valid_items():
    from scone_gcn_amd import path_scores
    cx, nb = tiny_complex()
    paths = random_walks(nb, np.random.RandomState(3), 10, 9)
    st, (_, item_path, item_len), x = check_columns(cx, nb, np.arange(5), paths, 1)
    ptr, nodes = path_scores.ragged(paths)
    S = (len(item_path) + 3) // 4
    got, _, _ = np_path_stage(S, item_path, item_len, None, ptr, nodes, st["slot"], st["row"], st["run"], st["next_same"], 5, nb.shape[1])
    assert same_floats(got, x)


def test_path_weights_make_every_path_count_the_same():
    from scone_gcn_amd import path_scores, path_train
    paths = [[0, 1, 2, 3, 0], [], [1], [0, 1], [0, 1, 2], [3, 0, 1, 2, 3, 0, 1, 2, 3]]
    ptr, _ = path_scores.ragged(paths)
    item_ptr, item_path, item_len = path_scores.path_items(ptr, 2)
    assert np.diff(item_ptr).tolist() == [3, 0, 0, 0, 1, 7]
    w = path_train.item_weights(item_ptr, item_path, "path")
    assert w.dtype == np.float32 and len(w) == 11
    assert same_floats(w, np.array([np.float32(1.0 / 3)] * 3 + [np.float32(1.0)] + [np.float32(1.0 / 7)] * 7, np.float32))
    per_path = np.bincount(item_path, weights=w.astype(np.float64), minlength=len(paths))
    assert np.allclose(per_path[[0, 4, 5]], 1.0, atol=1e-6) and not per_path[[1, 2, 3]].any()
    one = path_train.item_weights(item_ptr, item_path, "step")
    assert one.dtype == np.float32 and (one == 1).all() and len(one) == 11
    with pytest.raises(ValueError, match="step"):
        path_train.item_weights(item_ptr, item_path, "mean")
    assert len(path_train.item_weights(np.array([0, 0]), np.zeros(0, np.int64), "path")) == 0


def test_epoch_batches_permute_once_and_drop_the_short_tail():
    from scone_gcn_amd.path_train import epoch_batches
    # 59 items in batches of 16: three steps, the permutation's last 11 items sit the epoch out
    got = epoch_batches(np.random.RandomState(4), 59, 16)
    perm = np.random.RandomState(4).permutation(59)
    assert [len(b) for b in got] == [16, 16, 16] and all(b.dtype == np.int64 for b in got)
    assert np.array_equal(np.concatenate(got), perm[:48])
    assert len(set(np.concatenate(got).tolist())) == 48
    # a multiple: a full permutation
    got = epoch_batches(np.random.RandomState(4), 64, 16)
    assert [len(b) for b in got] == [16] * 4 and sorted(np.concatenate(got).tolist()) == list(range(64))
    # below one batch: the single batch keeps all items
    got = epoch_batches(np.random.RandomState(4), 7, 16)
    assert len(got) == 1 and sorted(got[0].tolist()) == list(range(7))
    assert np.array_equal(got[0], np.random.RandomState(4).permutation(7))
    # the same seed: the same batches; one draw per call, so a second epoch from the same stream differs
    rs = np.random.RandomState(9)
    a, b = epoch_batches(rs, 40, 8), epoch_batches(rs, 40, 8)
    c = epoch_batches(np.random.RandomState(9), 40, 8)
    assert all(np.array_equal(u, v) for u, v in zip(a, c)) and not all(np.array_equal(u, v) for u, v in zip(a, b))
    ref = np.random.RandomState(9)
    ref.permutation(40), ref.permutation(40)
    assert rs.randint(1 << 30) == ref.randint(1 << 30)                           # exactly one permutation drawn per epoch
    assert epoch_batches(rs, 0, 8) == []
    with pytest.raises(ValueError):
        epoch_batches(rs, 5, 0)


def test_library_exports_the_stage_call():
    from scone_gcn_amd import _lib
    assert "scn_path_stage" in _lib.SIGNATURES and len(_lib.SIGNATURES["scn_path_stage"][1]) == 22
    lib_path = os.path.join(ROOT, "scone_gcn_amd", "libscone_hip.so")
    assert os.path.exists(lib_path), "the library has not been built"
    lib = ctypes.CDLL(lib_path)
    assert hasattr(lib, "scn_path_stage")
    # refused before any launch (no GPU is touched): a negative count, ns, too many items, d, and the empty buffer
    lib.scn_path_stage.restype = ctypes.c_int
    lib.scn_path_stage.argtypes = _lib.SIGNATURES["scn_path_stage"][1]

    def call(n=1, n_slabs=1, n_prev=-1, n_paths=1, n_rows=8, ns=4, d=3):
        return lib.scn_path_stage(n, n_slabs, None, None, None, n_prev, None, None, n_paths, None, None, None, None, None, None, n_rows,
                                  ns, d, None, None, None, None)
    assert call(n=-1) == call(n_slabs=-1) == call(n_paths=-1) == call(n_rows=0) == call(d=0) == -2
    assert call(n=5) == call(n_prev=5) == -2
    assert call(ns=1) == call(ns=8) == _lib.SCN_ERR_UNSUPPORTED
    assert call(n=0, n_slabs=0, n_prev=0) == 0
    assert call() == _lib.SCN_ERR_BAD_ARG                                         # a null x


def test_switch_defaults_and_module_bool():
    from scone_gcn_amd import ops
    from scone_gcn_amd.scone_trajectory_model import Scone_GCN
    assert ops.PATH_STAGE_SPARSE_CLEAR is True
    net = Scone_GCN(1, 1e-3, 4, 0.0, verbose=False)
    assert net.path_micro_batch is None and net._path_pool is None
    net.drop_path_stage()
    for name in ("path_set", "path_loss", "path_grad_step", "train_paths"):
        assert callable(getattr(net, name))


def test_hyperparams_gain_three_keys_and_nothing_else_changes():
    from scone_gcn_amd import trajectory_experiments as te
    new = {"train_paths": 0, "path_min_prefix": 2, "path_weight": "step"}
    for argv in (["prog"], ["prog", "-epochs", "3", "-model", "ebli", "-hidden_layers", "3_8_3_8", "-path_likelihood", "1"]):
        hp = te.hyperparams(argv)
        for k, v in new.items():
            assert hp[k] == v and type(hp[k]) is type(v)
    hp = te.hyperparams(["prog"])
    today = {'model': 'scone', 'epochs': 1000, 'learning_rate': 0.001, 'weight_decay': 0.00005, 'batch_size': 100,
             'hidden_layers': [(3, 16), (3, 16), (3, 16)], 'describe': 1, 'reverse': 0, 'load_data': 1, 'load_model': 0, 'markov': 0,
             'model_name': 'model', 'regional': 0, 'flip_edges': 0, 'data_folder_suffix': 'working', 'multi_graph': '', 'holes': 1,
             'skip_mode': 'dense', 'multi_hop': 0, 'multi_hop_skip': 'dense', 'beam': 0, 'multi_hop_samples': 0, 'markov_order': 1,
             'projection': 0, 'path_likelihood': 0, 'n_points': 400, 'n_walks': 1000, 'walks': 'host', 'walk_metric': 'hops'}
    assert hp == {**today, **new}
    on = te.hyperparams(["prog", "-train_paths", "1", "-path_min_prefix", "3", "-path_weight", "path"])
    assert on["train_paths"] == 1 and on["path_min_prefix"] == 3 and on["path_weight"] == "path"
    assert {k: v for k, v in on.items() if k not in new} == today


def test_probed_closure_is_refused_by_the_path_set():
    from oracle import scone_oracle as so
    from scone_gcn_amd.scone_trajectory_model import Scone_GCN
    from tests.test_host_multihop import _tiny4
    net = Scone_GCN(1, 1e-3, 4, 0.0, verbose=False)
    net.model_type = "scone"
    B1, B2, edges, E_lookup = _tiny4()
    nb, _ = so.neighborhoods(edges, 4)
    inputs = [so.make_Bconds(B1, nb), np.array([1]), np.zeros((1, 5, 1))]
    with pytest.raises(TypeError, match="Bconds"):
        net.path_set(inputs, [[0, 1, 2]])
    with pytest.raises(TypeError, match="Bconds"):
        net.path_loss(inputs, [[0, 1, 2]])
    with pytest.raises(TypeError, match="Bconds"):
        net.train_paths(inputs, [[0, 1, 2]], np.ones(1), np.ones(1))
