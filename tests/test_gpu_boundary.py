"""GPU tests of the boundary and the host harness (through the C-ABI): reference-style operands (dense ndarray shifts, a plain
Bcond_func closure -- TE:240-257, 298-303), the experiment driver train_model() with its -reverse / -regional / -flip_edges
branches (TE:313-510) against an oracle trainer on the same RNG stream, the two-rank data-parallel gradient step through the HIP
path, the split-operand MFMA kernels against fp64 on wide-dynamic-range data, and flow inputs with
repeated entries."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import scone_oracle as so

pytestmark = pytest.mark.gpu
TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _maxdiff(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(b))))


def _rand_weights(shapes, scale, seed):
    rs = np.random.RandomState(seed)
    return [scale * rs.randn(*s) for s in shapes]


# ------------------------------------------------------------------------------------------------------------------
# reference-style operands
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["scone", "ebli", "bunch"])
def test_dense_shifts_and_a_plain_bcond_closure_run_unchanged(cfg1, model):
    """A caller that built its operands like the reference's data_setup (dense L1_lower / L1_upper / S_ab ndarrays, the
    Bconds_func closure over B1_jax and nbrhoods) calls the model functions and the trainer with them: same log-probabilities
    and gradients as the oracle."""
    _need_gpu()
    from scone_gcn_amd import trajectory_experiments as te
    from scone_gcn_amd import scone_trajectory_model as stm
    B1, B2 = cfg1["B1"], cfg1["B2"]
    nb, D = so.neighborhoods(cfg1["edges"], cfg1["n_nodes"])
    sel = np.arange(9)
    X, y, last = cfg1["flows"][sel], cfg1["targets"][sel], cfg1["last_nodes"][sel]
    mask = np.ones(len(sel), int)
    if model == "bunch":
        shifts = so.bunch_shifts(B1, B2)                                   # seven dense ndarrays (TE:255-257)
        readout = nb                                                       # nbrhoods (TE:309)
        w = _rand_weights(so.weight_shapes(1, [(7, 8)] * 3, 1, "bunch"), 0.4, 3)
        ref = so.bunch_forward(w, shifts, nb, last, X)
        ref_loss, ref_g = so.bunch_loss_and_grad(w, shifts, nb, last, X, y, mask, 0.0)
        fn = te.bunch_func
    else:
        shifts = so.scone_shifts(B1, B2) if model == "scone" else so.ebli_shifts(B1, B2)   # dense (E, E) ndarrays (TE:240-253)
        B1_jax = np.append(B1, np.zeros((1, B1.shape[1])), axis=0)         # TE:288

        def readout(n):                                                    # TE:298-303, verbatim semantics
            return B1_jax[nb[n]]
        w = _rand_weights(so.weight_shapes(1, [(3, 16)] * 3, 1), 0.3 if model == "scone" else 0.1, 4)
        act = "tanh" if model == "scone" else "leaky_relu"
        ref = so.scone_forward(w, shifts[0], shifts[1], readout, last, X, act=act)
        ref_loss, ref_g = so.scone_loss_and_grad(w, shifts[0], shifts[1], readout, last, X, y, mask, 0.0, act=act)
        fn = te.MODEL_FUNCS[model]
    wt = [torch.tensor(a, dtype=torch.float32, device="cuda", requires_grad=True) for a in w]
    out = fn(wt, *shifts, readout, last, X)
    assert _maxdiff(out.detach().cpu().numpy(), ref) <= TOL
    loss = -(out * torch.as_tensor(y, dtype=torch.float32, device="cuda")).sum() / len(sel)
    loss.backward()
    assert abs(float(loss.detach()) - ref_loss) <= TOL * max(1.0, abs(ref_loss))     # (relative, like _maxdiff: fp32 resolves a loss of 35 to 4e-6)
    for a, b in zip(wt, ref_g):
        assert _maxdiff(a.grad.cpu().numpy(), b) <= TOL
    # second call: other last nodes (the closure is probed for the new ones), per-sample call, and the trainer surface
    sel2 = np.arange(20, 27)
    ref2 = (so.bunch_forward(w, shifts, nb, cfg1["last_nodes"][sel2], cfg1["flows"][sel2]) if model == "bunch" else
            so.scone_forward(w, shifts[0], shifts[1], readout, cfg1["last_nodes"][sel2], cfg1["flows"][sel2], act=act))
    out2 = fn(w, *shifts, readout, cfg1["last_nodes"][sel2], cfg1["flows"][sel2])
    assert _maxdiff(out2.cpu().numpy(), ref2) <= TOL
    one = fn(w, *shifts, readout, int(cfg1["last_nodes"][21]), cfg1["flows"][21])
    assert one.shape == (D, 1) and _maxdiff(one.cpu().numpy(), ref2[1]) <= TOL
    stm.reseed(1030)
    net = stm.Scone_GCN(1, 1e-3, len(sel), 0.0, verbose=False)
    k = 7 if model == "bunch" else 3
    hl = [(k, 8)] * 3 if model == "bunch" else [(3, 16)] * 3
    net.setup(fn, hl, shifts, [readout, last, X], y, None, mask, model_type=model)
    for a, b in zip(net.weights, w):
        a.copy_(torch.as_tensor(b, dtype=torch.float32))
    net.grad_step([readout, last, X], y, mask, apply=False)
    for a, b in zip(net._grads, ref_g):
        assert _maxdiff(a.cpu().numpy(), b) <= TOL
    assert abs(net.loss(net.weights, [readout, last, X], y, mask) - ref_loss) <= TOL * max(1.0, abs(ref_loss))


def test_repeated_flow_entries_accumulate(cfg1):
    """A SparseFlows with the same (trajectory, edge) twice means f[k] += v twice (SDG:327-344): device scatter == host todense."""
    _need_gpu()
    from scone_gcn_amd import ops
    from scone_gcn_amd.complex import SimplicialComplex
    from scone_gcn_amd.synthetic_data_gen import Complex, SparseFlows
    cx = Complex(n_nodes=cfg1["n_nodes"], edges=cfg1["edges"].astype(np.int64), faces=cfg1["faces"].astype(np.int64),
                 coords=cfg1["coords"])
    sc = SimplicialComplex(cx)
    fl = SparseFlows(np.array([0, 4, 6], np.int64), np.array([3, 9, 3, 3, 7, 7], np.int64),
                     np.array([1, -1, 1, 1, 2, -2], np.float32), cfg1["E"])
    x, n = ops.flows_to_slabs(fl, sc.layout, ops.default_device())
    back = ops.slabs_to_batch(x, sc.layout, 1, n).cpu().numpy()
    assert np.array_equal(back, fl.todense())
    assert back[0, 3, 0] == 3.0 and back[1, 7, 0] == 0.0


# ------------------------------------------------------------------------------------------------------------------
# experiment driver
# ------------------------------------------------------------------------------------------------------------------

def _oracle_driver(hp, folder_suffix, gpu_preds=None, gpu_rev_preds=None):
    """The reference driver's sequence (TE:313-510, STM:215-368) on the oracle: same global RNG stream for flips, weights,
    batch masks and random targets.  The DISCRETE metrics (argmax accuracies, the 2-target comparison and its redraws) are
    evaluated on the log-probabilities handed in (the HIP path's, already checked against the oracle's to 1e-5): after two
    epochs from 0.01-scale weights the logits of a node's neighbours differ by ~1e-6, so an argmax is decided by fp32 noise --
    what is under test there is the metric logic and the RNG stream, not a tie."""
    from scone_gcn_amd import dataset_io
    model = hp["model"]
    f1 = "trajectory_data_1hop_" + folder_suffix
    X, (B1s, B2s), y, train_mask, test_mask, coords, last, tnodes = dataset_io.load_dataset(f1)
    B1, B2 = B1s.toarray(), B2s.toarray()
    X = np.asarray(X, np.float64)
    N = len(last)
    rs = np.random.RandomState(1030)
    F = None
    if hp["flip_edges"]:
        rs = np.random.RandomState(1)
        F = np.diag(rs.choice([1, -1], size=B1.shape[1], replace=True, p=[0.8, 0.2]).astype(np.float64))
        X = X * np.diag(F)[None, :, None]
    edges = np.array([(np.nonzero(B1[:, e] < 0)[0][0], np.nonzero(B1[:, e] > 0)[0][0]) for e in range(B1.shape[1])])
    nb, D = so.neighborhoods(edges, B1.shape[0])
    n_nbrs = (nb[last] >= 0).sum(1)
    if model == "bunch":
        shifts = so.bunch_shifts(B1, B2)
        k, wshape = 7, so.weight_shapes(1, hp["hidden_layers"], 1, "bunch")
        fwd = lambda w, ln, XX: so.bunch_forward(w, shifts, nb, ln, XX)
        lg = lambda w, m: so.bunch_loss_and_grad(w, shifts, nb, last, X, y, m, hp["weight_decay"])
    else:
        shifts = so.scone_shifts(B1, B2, F) if model == "scone" else so.ebli_shifts(B1, B2, F)
        act = "tanh" if model == "scone" else "leaky_relu"
        Bc = so.make_Bconds(B1, nb, F)
        k, wshape = 3, so.weight_shapes(1, hp["hidden_layers"], 1)
        fwd = lambda w, ln, XX: so.scone_forward(w, shifts[0], shifts[1], Bc, ln, XX, act=act)
        lg = lambda w, m: so.scone_loss_and_grad(w, shifts[0], shifts[1], Bc, last, X, y, m, hp["weight_decay"], act=act)
    w = [(0.01 * rs.randn(*s)).astype(np.float32).astype(np.float64) for s in wshape]
    if hp["regional"]:
        train_mask = np.array([1 if i % 3 == 1 else 0 for i in range(N)])
        test_mask = np.array([1 if i % 3 == 2 else 0 for i in range(N)])
    adam = so.Adam(w, hp["learning_rate"])
    bs = int(hp["batch_size"])
    n_batches = int(train_mask.sum()) // bs
    for i in range(int(hp["epochs"]) * n_batches):
        bm = so.draw_batch_mask(rs, N, bs, train_mask)
        if bm.sum() == 0:
            continue
        adam.update(i, lg(adam.x, bm)[1])
    out = fwd(adam.x, last, X)
    dis = out if gpu_preds is None else np.asarray(gpu_preds, np.float64)
    res = (so.loss_from_preds(out, y, train_mask, adam.x, hp["weight_decay"]), so.accuracy_from_preds(dis, y, train_mask, n_nbrs),
           so.loss_from_preds(out, y, test_mask, adam.x, hp["weight_decay"]), so.accuracy_from_preds(dis, y, test_mask, n_nbrs))
    t2_train, rt = so.two_target_accuracy_from_preds(dis, y, train_mask, n_nbrs, rs)
    t2_test, rt = so.two_target_accuracy_from_preds(dis, y, test_mask, n_nbrs, rs, random_targets=rt)
    extra = {"train_2target": t2_train, "test_2target": t2_test, "log_probs": out}
    if hp["reverse"]:
        rX, ry, rl = dataset_io.load_reverse(f1)
        rout = fwd(adam.x, rl, np.asarray(rX, np.float64))                  # stored reverse flows, not flipped (TE:499-504)
        rn = (nb[rl] >= 0).sum(1)
        rdis = rout if gpu_rev_preds is None else np.asarray(gpu_rev_preds, np.float64)
        extra["reverse"] = (so.loss_from_preds(rout, ry, test_mask, adam.x, hp["weight_decay"]),
                            so.accuracy_from_preds(rdis, ry, test_mask, rn))
        extra["reverse_log_probs"] = rout
    return adam.x, res, extra


@pytest.mark.parametrize("flags", [["-model", "scone"], ["-model", "ebli"], ["-model", "bunch", "-hidden_layers", "7_8_7_8_7_8"],
                                   ["-model", "scone", "-reverse", "1"], ["-model", "scone", "-regional", "1"],
                                   ["-model", "scone", "-flip_edges", "1", "-reverse", "1"]])
def test_train_model_driver_matches_the_oracle_driver(tmp_path, monkeypatch, flags):
    """train_model() (TE:313-510) end to end on a generated 150-point dataset: final weights, the returned losses / accuracies,
    both 2-target accuracies (STM:73-108, same random-target stream) and the reverse experiment, for every model and for the
    -reverse / -regional / -flip_edges branches (TE:449-453, 497-504, 214-219)."""
    _need_gpu()
    from scone_gcn_amd import dataset_io, scone_trajectory_model as stm, trajectory_experiments as te
    monkeypatch.chdir(tmp_path)
    dataset_io.generate_dataset(150, 45, folder="drv", holes=True)
    hp = te.hyperparams(["prog", "-epochs", "2", "-batch_size", "12", "-data_folder_suffix", "drv", "-describe", "1"] + flags)
    if "-hidden_layers" not in flags:
        hp["hidden_layers"] = [(3, 16)] * 3
    stm.reseed(1030)
    net, res = te.train_model(hp)
    got = net.experiment_results
    ref_w, ref_res, ref_extra = _oracle_driver(hp, "drv", got["log_probs"], got.get("reverse_log_probs"))
    for a, b in zip(net.weights, ref_w):
        assert _maxdiff(a.cpu().numpy(), b) <= 5e-6
    assert _maxdiff(got["log_probs"], ref_extra["log_probs"]) <= TOL
    if hp["reverse"]:
        assert _maxdiff(got["reverse_log_probs"], ref_extra["reverse_log_probs"]) <= TOL
    assert abs(res[0] - ref_res[0]) <= TOL and abs(res[2] - ref_res[2]) <= TOL
    assert res[1] == ref_res[1] and res[3] == ref_res[3]
    assert got["train_2target"] == ref_extra["train_2target"] and got["test_2target"] == ref_extra["test_2target"]
    if hp["reverse"]:
        assert abs(got["reverse"][0] - ref_extra["reverse"][0]) <= TOL and got["reverse"][1] == ref_extra["reverse"][1]
    assert os.path.exists(os.path.join("models", "model.npz"))
    # -load_model 1 with epochs 0: the stored weights reproduce the test numbers (TE:464-476)
    hp2 = dict(hp, load_model=1.0, epochs=0)
    net2, res2 = te.train_model(hp2)
    assert abs(res2[2] - res[2]) <= 1e-6 and res2[3] == res[3]
    stm.reseed(1030)


# ------------------------------------------------------------------------------------------------------------------
# data parallel: two ranks on one GPU, gloo rendezvous, HIP compute
# ------------------------------------------------------------------------------------------------------------------

_DP_SCRIPT = r'''
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
rank, world, port, out = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
from scone_gcn_amd import synthetic_data_gen as g, trajectory_experiments as te, scone_trajectory_model as stm
from scone_gcn_amd.complex import SimplicialComplex
torch.cuda.set_device(0)
if world > 1:
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", port
    dist.init_process_group("gloo", rank=rank, world_size=world)
cx = g.random_SC_graph(1500)
sc = SimplicialComplex(cx)
paths = g.generate_random_walks(cx, m=37, seed=5, waypoint_pool=8, metric="euclid")
flows, choice, last, _, _ = g.path_dataset(cx, paths, seed=6)
y = np.zeros((37, sc.max_degree, 1)); y[np.arange(37), choice, 0] = 1.0
shifts, readout, _ = te.setup_from_complex(sc, "scone")
inputs = [readout, last, flows]
stm.reseed(1030)
net = stm.Scone_GCN(1, 1e-2, 30, 5e-5, verbose=False)
net.setup(te.scone_func, [(3, 32)] * 3, shifts, inputs, y, None, np.ones(37, int), model_type="scone")
with torch.no_grad():
    for w in net.weights:
        w.mul_(12.0)
mask = np.ones(37, int); mask[[1, 8, 30]] = 0            # 34 trajectories: 17 + 17, uneven slabs
part = float(net.grad_step(inputs, y, mask, apply=False))
grad = net._flat_g.cpu().numpy().copy()
for _ in range(2):
    net.grad_step(inputs, y, mask)                        # two optimiser steps: replicas must stay identical
np.savez(out, grad=grad, part=part, w=net._flat_w.cpu().numpy())
if world > 1:
    dist.destroy_process_group()
'''


def test_two_rank_gradient_step_through_the_hip_path(tmp_path):
    """Scone_GCN.grad_step under torch.distributed with TWO ranks (gloo rendezvous, both on GPU 0 -- the RCCL leg needs two
    GPUs): the all-reduced flat gradient equals the single-process one (fp32 summation order differs between one and two
    shards: <= 1e-6 of the largest entry), the ranks hold bit-identical gradients and weights after two optimiser steps, and
    the local loss shares add up (STM:313-322 sharded per SURVEY section 8e)."""
    _need_gpu()
    script = tmp_path / "dp_rank.py"
    script.write_text(_DP_SCRIPT)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    one = subprocess.run([sys.executable, str(script), ROOT, "0", "1", port, str(tmp_path / "single.npz")], env=env,
                         capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, one.stderr[-2000:]
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(r), "2", port, str(tmp_path / ("rank%d.npz" % r))], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    outs = [p.communicate(timeout=600) for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[1][-2000:]
    ref = np.load(tmp_path / "single.npz")
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert np.array_equal(r0["grad"], r1["grad"]) and np.array_equal(r0["w"], r1["w"])
    gmax = np.abs(ref["grad"]).max()
    assert gmax > 1e-4
    assert np.abs(r0["grad"] - ref["grad"]).max() <= 1e-6 * gmax
    assert abs(float(r0["part"]) + float(r1["part"]) - float(ref["part"])) <= 1e-6 * max(1.0, abs(float(ref["part"])))
    assert np.abs(r0["w"] - ref["w"]).max() <= 2e-6


# ------------------------------------------------------------------------------------------------------------------
# split-operand MFMA kernels on a wide dynamic range
# ------------------------------------------------------------------------------------------------------------------

def test_split_operand_mfma_kernels_hold_fp32_accuracy_on_wide_dynamic_range():
    """The C=32 / C=16 kernels evaluate fp32 products on the f16 MFMA: both operands split hi + lo under power-of-two row scales,
    three products, fp32 accumulation (rounds 1-4: six bf16 products of an exact three-way split; the test and its tolerances are
    unchanged).  On slabs whose every row spans 1e-4 .. 1e3 (both signs: the scales and both parts of the split all matter) forward,
    input gradient and weight gradients must agree with an fp64 evaluation to fp32 accuracy, relative to each output's own sum of
    |terms| -- a truncated split (plain f16 / bf16, or an un-scaled f16 split) fails this by orders of magnitude."""
    _need_gpu()
    import scipy.sparse as sp
    from scone_gcn_amd import ops, synthetic_data_gen as g, trajectory_experiments as te
    from scone_gcn_amd.complex import SimplicialComplex
    cx = g.random_SC_graph(3000)
    sc = SimplicialComplex(cx)
    shifts, readout, _ = te.setup_from_complex(sc, "scone")
    plan = ops.get_scone_plan(shifts[0], shifts[1], readout, "tanh", ops.default_device())
    E = cx.n_edges
    lo, up = shifts[0].device_csr().astype(np.float64), shifts[1].device_csr().astype(np.float64)
    rs = np.random.RandomState(11)
    for C in (32, 16):
        S = 3
        mag = 10.0 ** rs.uniform(-4, 3, size=(S, E, 4, C))
        x32 = (mag * rs.choice([-1.0, 1.0], size=mag.shape)).astype(np.float32)
        aux32 = np.tanh(rs.randn(S, E, 4, C)).astype(np.float32)
        W32 = [(10.0 ** rs.uniform(-3, 0, size=(C, C)) * rs.choice([-1.0, 1.0], size=(C, C))).astype(np.float32) for _ in range(3)]
        xt, at = torch.from_numpy(x32).cuda(), torch.from_numpy(aux32).cuda()
        Wt = [torch.from_numpy(w).cuda() for w in W32]
        fwd = plan.conv.forward([xt], Wt, C, "none").cpu().numpy()
        dWs = [torch.zeros_like(w) for w in Wt]
        dx = plan.conv.backward([xt], Wt, at, "tanh", True, dWs).cpu().numpy()
        x, aux, W = x32.astype(np.float64), aux32.astype(np.float64), [w.astype(np.float64) for w in W32]
        flat = x.transpose(1, 0, 2, 3).reshape(E, -1)
        sh = lambda m, f: (m @ f).reshape(E, S, 4, C).transpose(1, 0, 2, 3)
        gk = [x, sh(lo, flat), sh(up, flat)]
        ga = [np.abs(x), sh(abs(lo), np.abs(flat)), sh(abs(up), np.abs(flat))]
        ref = sum(a @ w for a, w in zip(gk, W))
        scale = sum(a @ np.abs(w) for a, w in zip(ga, W))            # sum of |terms| of every output
        assert (np.abs(fwd - ref) / scale).max() <= 8e-6, C
        # backward: dx = (sum_k G_k W_k^T) * tanh'(aux) with G = gathered dz (symmetric shifts), dW_k = aux^T G_k
        refdx = sum(a @ w.T for a, w in zip(gk, W)) * (1.0 - aux ** 2)
        sdx = sum(a @ np.abs(w).T for a, w in zip(ga, W))
        assert (np.abs(dx - refdx) / sdx).max() <= 8e-6, C
        for k in range(3):
            refw = np.einsum("srnc,srnd->cd", aux, gk[k])
            sw = np.einsum("srnc,srnd->cd", np.abs(aux), ga[k])
            assert (np.abs(dWs[k].cpu().numpy() - refw) / sw).max() <= 1e-4, (C, k)   # fp32 accumulation over S*E*4 = 1e5 terms


def test_trajectories_of_different_magnitude_sharing_a_slab():
    """The scales of the split are per POINT in the forward and per 32-point TILE (8 rows x the 4 trajectories of a slab) in the
    backward.  Trajectories are independent samples, so their magnitudes may differ inside a tile:
    (1) three orders of magnitude between the trajectories of a slab (a wide spread for gradients of one batch): forward, input
        gradient and weight gradients hold the same bars as on uniform data, every output relative to ITS OWN sum of |terms|;
    (2) nine orders: the forward still does (its scale is the point's own); the input gradient of the smallest trajectory is held
        relative to the largest trajectory of its tile (1e-11 of that trajectory's sum of |terms|: f16 subnormals under the tile's
        scale; measured ~1e-12), and the weight gradients, which add all trajectories up, hold their bar unchanged."""
    _need_gpu()
    from scone_gcn_amd import ops, synthetic_data_gen as g, trajectory_experiments as te
    from scone_gcn_amd.complex import SimplicialComplex
    cx = g.random_SC_graph(2500)
    sc = SimplicialComplex(cx)
    shifts, readout, _ = te.setup_from_complex(sc, "scone")
    plan = ops.get_scone_plan(shifts[0], shifts[1], readout, "tanh", ops.default_device())
    E, C, S = cx.n_edges, 32, 2
    lo, up = shifts[0].device_csr().astype(np.float64), shifts[1].device_csr().astype(np.float64)
    rs = np.random.RandomState(23)
    W32 = [(0.1 * rs.randn(C, C)).astype(np.float32) for _ in range(3)]
    Wt = [torch.from_numpy(w).cuda() for w in W32]
    W = [w.astype(np.float64) for w in W32]
    aux32 = np.tanh(rs.randn(S, E, 4, C)).astype(np.float32)
    at = torch.from_numpy(aux32).cuda()
    aux = aux32.astype(np.float64)
    for spread, dx_bar_own in ((1e-1, 8e-6), (1e-3, None)):
        mags = np.array([1.0, spread, spread ** 2, spread ** 3])            # 1, 1e-1, 1e-2, 1e-3  /  1, 1e-3, 1e-6, 1e-9
        x32 = (rs.randn(S, E, 4, C) * mags[None, None, :, None]).astype(np.float32)
        xt = torch.from_numpy(x32).cuda()
        fwd = plan.conv.forward([xt], Wt, C, "none").cpu().numpy()
        dWs = [torch.zeros_like(w) for w in Wt]
        dx = plan.conv.backward([xt], Wt, at, "tanh", True, dWs).cpu().numpy()
        x = x32.astype(np.float64)
        flat = x.transpose(1, 0, 2, 3).reshape(E, -1)
        sh = lambda m, f: (m @ f).reshape(E, S, 4, C).transpose(1, 0, 2, 3)
        gk = [x, sh(lo, flat), sh(up, flat)]
        ga = [np.abs(x), sh(abs(lo), np.abs(flat)), sh(abs(up), np.abs(flat))]
        ref = sum(a @ w for a, w in zip(gk, W))
        scale = sum(a @ np.abs(w) for a, w in zip(ga, W))
        assert (np.abs(fwd - ref) / scale).max() <= 8e-6, spread            # per point: every trajectory to its own magnitude
        refdx = sum(a @ w.T for a, w in zip(gk, W)) * (1.0 - aux ** 2)
        sdx = sum(a @ np.abs(w).T for a, w in zip(ga, W))
        err = np.abs(dx - refdx)
        if dx_bar_own is not None:
            assert (err / sdx).max() <= dx_bar_own, spread
        tile_max = sdx[:, :, :1, :].max(axis=3, keepdims=True)                 # the slab's largest trajectory (index 0) at the same row
        assert (err / (8e-6 * sdx + 1e-11 * tile_max)).max() <= 1.0, spread    # own terms to fp32 accuracy + 1e-11 of the tile's largest
        for k in range(3):
            refw = np.einsum("srnc,srnd->cd", aux, gk[k])
            sw = np.einsum("srnc,srnd->cd", np.abs(aux), ga[k])
            assert (np.abs(dWs[k].cpu().numpy() - refw) / sw).max() <= 1e-4, (spread, k)


def test_weight_gradient_accumulators_across_slabs_of_very_different_magnitude():
    """The backward keeps its weight-gradient accumulators in the units of the LARGEST tile a wave has seen so far and rescales them when
    a larger one arrives.  Slabs are visited in order, so slab magnitudes that rise, fall, vanish (exact-zero
    slabs: the early-out leaves the running exponent alone) and rise again drive every branch of that bookkeeping; dW (which adds all
    slabs up) must hold its usual bar, and dx every output's own."""
    _need_gpu()
    from scone_gcn_amd import ops, synthetic_data_gen as g, trajectory_experiments as te
    from scone_gcn_amd.complex import SimplicialComplex
    cx = g.random_SC_graph(1500)
    sc = SimplicialComplex(cx)
    shifts, readout, _ = te.setup_from_complex(sc, "scone")
    plan = ops.get_scone_plan(shifts[0], shifts[1], readout, "tanh", ops.default_device())
    E = cx.n_edges
    lo, up = shifts[0].device_csr().astype(np.float64), shifts[1].device_csr().astype(np.float64)
    rs = np.random.RandomState(31)
    for C, act in ((32, "tanh"), (16, "relu")):
        slab_scale = np.array([1e-6, 1e-3, 0.0, 1.0, 1e4, 0.0, 0.0, 1e-2, 1e-9, 3.0, 1e2])      # rises, vanishes, falls, rises again
        S = len(slab_scale)
        x32 = (rs.randn(S, E, 4, C) * slab_scale[:, None, None, None]).astype(np.float32)
        aux32 = (np.tanh(rs.randn(S, E, 4, C)) if act == "tanh" else np.maximum(rs.randn(S, E, 4, C), 0.0) * 50.0).astype(np.float32)
        W32 = [(0.2 * rs.randn(C, C)).astype(np.float32) for _ in range(3)]
        xt, at = torch.from_numpy(x32).cuda(), torch.from_numpy(aux32).cuda()
        Wt = [torch.from_numpy(w).cuda() for w in W32]
        dWs = [torch.zeros_like(w) for w in Wt]
        dx = plan.conv.backward([xt], Wt, at, act, True, dWs).cpu().numpy()
        x, aux, W = x32.astype(np.float64), aux32.astype(np.float64), [w.astype(np.float64) for w in W32]
        flat = x.transpose(1, 0, 2, 3).reshape(E, -1)
        sh = lambda m, f: (m @ f).reshape(E, S, 4, C).transpose(1, 0, 2, 3)
        gk = [x, sh(lo, flat), sh(up, flat)]
        ga = [np.abs(x), sh(abs(lo), np.abs(flat)), sh(abs(up), np.abs(flat))]
        dact = (1.0 - aux ** 2) if act == "tanh" else (aux > 0).astype(np.float64)
        refdx = sum(a @ w.T for a, w in zip(gk, W)) * dact
        sdx = sum(a @ np.abs(w).T for a, w in zip(ga, W)) + 1e-300
        assert (np.abs(dx - refdx) / sdx).max() <= 8e-6, (C, act)
        assert np.all(dx[slab_scale == 0.0] == 0.0)
        for k in range(3):
            refw = np.einsum("srnc,srnd->cd", aux, gk[k])
            sw = np.einsum("srnc,srnd->cd", np.abs(aux), ga[k])
            assert (np.abs(dWs[k].cpu().numpy() - refw) / sw).max() <= 1e-4, (C, act, k)


def test_bench_lines_of_one_and_two_ranks_agree_on_loss_and_weights():
    """bench.py is self-validating across rank counts (the host draws the batch once, shards by index; STM:256's
    batch axis, STM:313-322's mask semantics): `--gpus 1` and `--gpus 2 --backend gloo` (both ranks on this one GPU, the
    gradient all-reduce through gloo) on the same complex take the same optimiser steps -- equal loss and weights to the
    summation order of the reduction -- and the two replicas hold bitwise identical weights."""
    import json
    import subprocess
    import sys
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    lines = {}
    for n in (1, 2):
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", str(n), "--backend", "gloo", "--full", "--extras", "0",
               "--edges", "50000", "--hidden", "16", "--global-batch", "64", "--steps", "3", "--warmup", "1"]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out_lines = r.stdout.splitlines()
        # the driver keeps an 8 KB tail of stdout: the LAST line is the compact record, the full one sits on a DETAIL line before it
        assert out_lines[-1].startswith("{") and len(out_lines[-1]) < 8000, len(out_lines[-1])
        last = json.loads(out_lines[-1])
        for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype", "scaling", "config", "roofline",
                    "cpu_baseline", "loss", "replicas_identical"):
            assert key in last, key
        lines[n] = json.loads([l for l in out_lines if l.startswith("DETAIL {")][-1][len("DETAIL "):])
        assert last["value"] == lines[n]["value"] and last["loss"] == lines[n]["loss"]
        assert json.load(open(os.path.join(root, "bench_full.json"))) == lines[n]
    a, b = lines[1], lines[2]
    assert a["n_gpus"] == 1 and b["n_gpus"] == 2 and b["config"]["per_gpu_batch"] == 32
    assert a["replicas_identical"] is True and b["replicas_identical"] is True
    assert "world_size() = 2" in b["config"]["collective"]
    assert abs(a["loss"] - b["loss"]) <= 1e-6 * max(1.0, abs(a["loss"]))
    va, vb = a["validation"], b["validation"]
    assert abs(va["weights_sum"] - vb["weights_sum"]) <= 1e-6 * max(1.0, abs(va["weights_sum"]))
    assert abs(va["weights_l2"] - vb["weights_l2"]) <= 1e-6 * va["weights_l2"]


def test_plain_bench_run_times_its_steps_and_dumps_what_the_last_one_computed(tmp_path):
    """A plain `bench.py` run (no --full) prints the headline line alone, takes exactly --warmup + --steps optimiser steps, and
    --dump-outputs writes what the last of them computed: the same arguments give bitwise the same files, and moving one step
    from the timed to the untimed side changes nothing, while one step fewer does."""
    import json
    _need_gpu()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    runs = {"a": (3, 1), "a_again": (3, 1), "moved": (2, 2), "fewer": (2, 1)}
    for name, (steps, warmup) in runs.items():
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--edges", "50000", "--hidden", "16",
               "--global-batch", "64", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / name)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        last = json.loads(r.stdout.splitlines()[-1])
        assert last["metric"].startswith("trajectories/sec") and last["unit"] == "trajectories/s" and last["dtype"] == "f32"
        assert last["higher_is_better"] is True and last["steps"] == steps and last["warmup"] == warmup
        assert last["ms_per_step"] > 0 and abs(last["value"] - 64 * 1e3 / last["ms_per_step"]) <= 1e-9 * last["value"]
        assert last["roofline"] is None and last["cpu_baseline"] is None and "configs" not in last
    names = ("loss", "weights", "weight_grad", "adam_m", "adam_v")
    out = {run: {n: np.load(tmp_path / run / (n + ".npy")) for n in names} for run in runs}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in names)
    a = out["a"]
    assert a["loss"].dtype == np.float64 and a["loss"].shape == (1,) and 0 < a["loss"][0] < 10
    assert all(a[n].dtype == np.float32 and a[n].size == a["weights"].size and np.isfinite(a[n]).all() for n in names[1:])
    for n in names:
        assert np.array_equal(out["a_again"][n], a[n]) and np.array_equal(out["moved"][n], a[n]), n
    assert not np.array_equal(out["fewer"]["weights"], a["weights"])


def test_evaluation_cache_follows_every_way_the_weights_can_change(cfg1):
    """Scone_GCN.loss / accuracy on a small data set read ONE forward of the whole set per weight version (the epoch-end passes of
    train(), STM:328-337).  The cached log-probabilities must follow an optimiser step (a raw-pointer write), an in-place torch
    operation on a weight view, load_weights, other masks and other input objects -- against the uncached evaluation each time."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from scone_gcn_amd import scone_trajectory_model as stm
    from scone_gcn_amd import trajectory_experiments as te
    from scone_gcn_amd.complex import SimplicialComplex
    from scone_gcn_amd.synthetic_data_gen import Complex
    cx = Complex(n_nodes=cfg1["n_nodes"], edges=cfg1["edges"].astype(np.int64), faces=cfg1["faces"].astype(np.int64), coords=cfg1["coords"])
    sc = SimplicialComplex(cx)
    shifts, readout, _ = te.setup_from_complex(sc, "scone")
    N = 300
    inputs = [readout, cfg1["last_nodes"][:N], cfg1["flows"][:N]]
    y, n_nbrs = cfg1["targets"][:N], sc.n_nbrs(cfg1["last_nodes"][:N])
    train = cfg1["train_mask"][:N]
    test = 1 - train
    stm.reseed(1030)
    net = stm.Scone_GCN(1, 1e-2, 50, 5e-5, verbose=False)
    net.setup(te.scone_func, [(3, 16)] * 3, shifts, inputs, y, None, train, model_type="scone")

    def both():
        out = []
        for cached in (True, False):
            net.use_eval_cache = cached
            out.append((net.loss(net.weights, inputs, y, train), net.accuracy(shifts, inputs, y, train, n_nbrs),
                        net.loss(net.weights, inputs, y, test), net.accuracy(shifts, inputs, y, test, n_nbrs)))
        net.use_eval_cache = True
        assert out[0] == out[1], out
        return out[0]
    seen = [both()]
    bm = np.zeros(N, int)
    bm[:50] = 1
    net.grad_step(inputs, y, np.logical_and(bm, train))                    # Adam: a raw-pointer write
    seen.append(both())
    with torch.no_grad():
        net.weights[3].mul_(1.5)                                            # an in-place operation on a view of the flat buffer
    seen.append(both())
    assert len({s[0] for s in seen}) == 3                                   # the loss moved each time: nothing stale was served
    assert net._eval is not None and net._eval["n"] == N
    other = [readout, cfg1["last_nodes"][N:2 * N], cfg1["flows"][N:2 * N]]  # other input objects: a new staging, a new forward
    net.use_eval_cache = True
    a = net.loss(net.weights, other, cfg1["targets"][N:2 * N], np.ones(N, int))
    net.use_eval_cache = False
    b = net.loss(net.weights, other, cfg1["targets"][N:2 * N], np.ones(N, int))
    assert a == b


def test_evaluation_cache_with_the_bunch_model_and_a_probed_readout_closure(cfg1):
    """The same cache under the other plan types: a Bunch model (BunchPlan, node readout) and a scone model whose readout operand is a
    plain Bcond_func closure probed on demand (ProbedBconds: the tables grow with the last nodes seen) -- cached == uncached."""
    _need_gpu()
    from scone_gcn_amd import scone_trajectory_model as stm
    from scone_gcn_amd import trajectory_experiments as te
    from scone_gcn_amd.complex import SimplicialComplex
    from scone_gcn_amd.synthetic_data_gen import Complex
    cx = Complex(n_nodes=cfg1["n_nodes"], edges=cfg1["edges"].astype(np.int64), faces=cfg1["faces"].astype(np.int64), coords=cfg1["coords"])
    sc = SimplicialComplex(cx)
    N = 120
    y, last, flows = cfg1["targets"][:N], cfg1["last_nodes"][:N], cfg1["flows"][:N]
    n_nbrs = sc.n_nbrs(last)
    mask = (np.arange(N) % 3 != 0).astype(int)
    nb, D = so.neighborhoods(cfg1["edges"], cfg1["n_nodes"])
    closure = so.make_Bconds(cfg1["B1"], nb, None)
    cases = []
    shifts_b, readout_b, _ = te.setup_from_complex(sc, "bunch")
    cases.append(("bunch", te.bunch_func, [(7, 16)] * 2, shifts_b, readout_b))
    shifts_s, _, _ = te.setup_from_complex(sc, "scone")
    cases.append(("scone", te.scone_func, [(3, 16)] * 2, shifts_s, closure))
    for model, fn, layers, shifts, readout in cases:
        inputs = [readout, last, flows]
        stm.reseed(1030)
        net = stm.Scone_GCN(1, 1e-2, 40, 0.0, verbose=False)
        net.setup(fn, layers, shifts, inputs, y, None, mask, model_type=model)
        got = []
        for cached in (True, False, True):
            net.use_eval_cache = cached
            got.append((net.loss(net.weights, inputs, y, mask), net.accuracy(shifts, inputs, y, mask, n_nbrs),
                        net.loss(net.weights, inputs, y, 1 - mask)))
        assert got[0] == got[1] == got[2], (model, got)
