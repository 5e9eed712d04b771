"""scn_step_epilogue (csrc/scn_step_epilogue.inc): every job of the one-launch epilogue against its stand-alone entry point, BIT FOR BIT.

  loss          scn_masked_ce_begin, overwrite 0 and 1
  readout_dw    scn_readout_backward's weight gradient, accumulated into non-zero values
  reduces       scn_dw_reduce on hand-made partial sums of 8, 256 and 264 workgroups (the loop's four-at-a-time part, its tail, both),
                one of them holding an Inf, into non-zero targets; and the first layer's scn_dw_first_reduce, both forms
  clears        scn_readout_clear_dz and scn_clear_mask on sentinel-filled tensors: exactly the stand-alone clears' items
One reference per module; then the epilogue with every job present, each job absent alone (what is absent stays untouched), one reduce
with the first layer's (a two-layer tail), four reduces (five layers), no masked clear -- and more jobs than the descriptor holds, which
is refused before any launch.  The two _partial backwards are run against their reducing twins through the epilogue as well.

Shapes: the cfg1 golden complex of tests/test_gpu_readout_cone.py (|E| = 1001, 17 plan blocks or so), 5 slabs of 4."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_keep_last import SENTINEL, _need_gpu, _pack, _sentinel
from tests.test_gpu_readout_cone import _env, _first_case, _bwd_case, _mask
from tests.test_host_readout import random_H

pytestmark = pytest.mark.gpu
S, NS, C = 5, 4, 32
SCN_ERR_BAD_SHAPE = -2
_REF = {}


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _ref():
    """Inputs of every job and the stand-alone entries' results on them (computed once, never modified)."""
    if _REF:
        return _REF
    from scone_gcn_amd import _lib, ops
    lib, env = _lib.load(), _env()
    plan = env["plan"]()
    rs = np.random.RandomState(2024)
    E, V, D, N = env["E"], plan.n_nodes, plan.max_deg, S * NS
    R = dict(lib=lib, plan=plan, E=E, D=D, N=N)
    # loss
    R["logp"] = _cuda((-rs.uniform(0, 20, (N, D))).astype(np.float32))
    R["y"] = _cuda(((rs.rand(N, D) < 0.2) * rs.uniform(0.5, 1.5, (N, D))).astype(np.float32))
    R["scale"] = -1.0 / 123.0
    R["loss0"] = 2.5
    for ow in (0, 1):
        loss = torch.full((1,), R["loss0"], device="cuda", dtype=torch.float64)
        assert lib.scn_masked_ce_begin(N * D, _p(R["logp"]), _p(R["y"]), R["scale"], _p(torch.empty((N, D), device="cuda")), _p(loss), ow, None, 0,
                                       ops._stream()) == 0
        R["loss_ref%d" % ow] = loss.clone()
    # the readout's weight gradient: d_logits and bh of a real backward
    last = np.zeros(N, np.int32)
    last[:18] = rs.randint(0, V, 18)
    R["last"] = _cuda(last)
    H, w = _cuda(random_H(rs, S, E, NS, C)), _cuda((rs.randn(C) / np.sqrt(C)).astype(np.float32))
    tabs = (_p(plan.nbr), V, D, _p(R["last"]), _p(plan.inc_ptr), _p(plan.inc_edge))
    bh, logits, logp = torch.empty((N, D, C), device="cuda"), torch.empty((N, D), device="cuda"), torch.empty((N, D), device="cuda")
    assert lib.scn_readout_forward(S, NS, E, C, _p(H), _p(w), *tabs, _p(plan.inc_sign), _p(bh), _p(logits), _p(logp), ops._stream()) == 0
    R["d_w0"] = _cuda(rs.randn(C).astype(np.float32))
    d_w, dl, dz = R["d_w0"].clone(), torch.empty((N, D), device="cuda"), torch.zeros_like(H)
    assert lib.scn_readout_backward(S, NS, E, C, _p(H), _p(w), *tabs, _p(plan.inc_sign), _p(plan.edge_nodes), _p(bh), _p(R["y"]), _p(logp), 1, _p(dl),
                                    _p(dz), 1, _p(d_w), ops._stream()) == 0
    R.update(bh=bh, dl=dl, d_w_ref=d_w)
    # reduces
    R["reduce"] = []
    for k, n_wg in enumerate((8, 256, 264, 8)):
        part = rs.randn(n_wg, C, 3 * C).astype(np.float32)
        if k == 1:
            part[n_wg // 2, 3, 70] = np.inf
        part, dW0 = _cuda(part), [_cuda(rs.randn(C, C).astype(np.float32)) for _ in range(3)]
        ref = [t.clone() for t in dW0]
        assert lib.scn_dw_reduce(_p(part), n_wg, C, C, ops._ptrs(ref), ops._stream()) == 0
        R["reduce"].append(dict(part=part, n_wg=n_wg, dW0=dW0, ref=ref))
    R["first"] = {}
    for form, width in ((1, 32), (2, 16)):
        part, dW0 = _cuda(rs.randn(264, 96).astype(np.float32)), [_cuda(rs.randn(1, width).astype(np.float32)) for _ in range(3)]
        ref = [t.clone() for t in dW0]
        assert lib.scn_dw_first_reduce(_p(part), 264, form, ops._ptrs(ref), ops._stream()) == 0
        R["first"][form] = dict(part=part, dW0=dW0, ref=ref)
    # clears
    rc = _sentinel((S, E, NS, C))
    assert lib.scn_readout_clear_dz(S, NS, E, C, _p(plan.nbr), V, D, _p(R["last"]), _p(plan.inc_ptr), _p(plan.inc_edge), _p(plan.edge_nodes), _p(rc),
                                    ops._stream()) == 0
    R["rc_ref"] = rc
    R["clear"] = []
    for pattern in ("random", "runs", "all", "empty"):
        mask = _pack(_mask(pattern, env["nb"], S, rs))
        t = _sentinel((S, E, NS, C))
        plan.conv.clear_mask(t, mask)
        R["clear"].append(dict(mask=mask, ref=t))
    torch.cuda.synchronize()
    assert bool((_bits(R["rc_ref"]) == 0).any()) and bool((_bits(R["clear"][0]["ref"]) == 0).any())
    assert not torch.isfinite(R["reduce"][1]["ref"][2]).all()          # (column 70 of 96: slot 2)
    _REF.update(R)
    return _REF


def _run(jobs, overwrite=0, first_form=1):
    """One epilogue launch with the named jobs; returns (status, outputs) -- every output buffer exists, the absent jobs' untouched."""
    from scone_gcn_amd import _lib, ops
    R = _ref()
    plan, E, D, N = R["plan"], R["E"], R["D"], R["N"]
    d = _lib.StepEpilogueDesc()
    out = dict(loss=torch.full((1,), R["loss0"], device="cuda", dtype=torch.float64), d_w=R["d_w0"].clone(),
               reduce=[[t.clone() for t in q["dW0"]] for q in R["reduce"]], first=[t.clone() for t in R["first"][first_form]["dW0"]],
               rc=_sentinel((S, E, NS, C)), clear=[_sentinel((S, E, NS, C)) for _ in R["clear"]])
    if "loss" in jobs:
        d.loss_n, d.logp, d.y, d.scale, d.loss, d.overwrite = N * D, R["logp"].data_ptr(), R["y"].data_ptr(), R["scale"], out["loss"].data_ptr(), overwrite
    if "readout_dw" in jobs:
        d.rd_nd, d.rd_c, d.rd_dl, d.rd_bh, d.rd_d_w = N * D, C, R["dl"].data_ptr(), R["bh"].data_ptr(), out["d_w"].data_ptr()
    for k in [j for j in jobs if isinstance(j, tuple) and j[0] == "reduce"]:
        q, src = d.reduce[d.n_reduce], R["reduce"][k[1] % len(R["reduce"])]
        q.partial, q.n_wg, q.c_aux, q.c_dz = src["part"].data_ptr(), src["n_wg"], C, C
        for s in range(3):
            q.dW[s] = out["reduce"][k[1] % len(R["reduce"])][s].data_ptr()
        d.n_reduce += 1
        if d.n_reduce == _lib.SCN_EPI_MAX_REDUCES and len([j for j in jobs if isinstance(j, tuple) and j[0] == "reduce"]) > d.n_reduce:
            d.n_reduce = _lib.SCN_EPI_MAX_REDUCES + 1                         # more than the descriptor holds
            break
    if "first" in jobs:
        src = R["first"][first_form]
        d.first_form, d.first_partial, d.first_n_wg = first_form, src["part"].data_ptr(), 264
        for s in range(3):
            d.first_dW[s] = out["first"][s].data_ptr()
    if "rc" in jobs:
        d.rc_n_slabs, d.rc_ns, d.rc_n_edges, d.rc_c, d.rc_max_deg = S, NS, E, C, D
        d.rc_nbr, d.rc_last_nodes, d.rc_inc_ptr, d.rc_inc_edge = plan.nbr.data_ptr(), R["last"].data_ptr(), plan.inc_ptr.data_ptr(), plan.inc_edge.data_ptr()
        d.rc_edge_nodes, d.rc_dz = plan.edge_nodes.data_ptr(), out["rc"].data_ptr()
    for k in [j for j in jobs if isinstance(j, tuple) and j[0] == "clear"]:
        if d.n_clear == _lib.SCN_EPI_MAX_CLEARS:
            d.n_clear += 1
            break
        q = d.clear[d.n_clear]
        q.tensor, q.mask, q.n_slabs, q.ns, q.channels = out["clear"][k[1]].data_ptr(), R["clear"][k[1]]["mask"].data_ptr(), S, NS, C
        d.n_clear += 1
    st = R["lib"].scn_step_epilogue(plan.conv.handle, ctypes.byref(d), ops._stream())
    torch.cuda.synchronize()
    return st, out


def _assert_jobs(jobs, out, overwrite=0, first_form=1):
    R = _ref()
    same = lambda a, b, what: np.array_equal(_bits(a), _bits(b)) or pytest.fail("%s differs (jobs %s)" % (what, jobs))
    same(out["loss"], R["loss_ref%d" % overwrite] if "loss" in jobs else torch.full((1,), R["loss0"], dtype=torch.float64), "loss")
    same(out["d_w"], R["d_w_ref"] if "readout_dw" in jobs else R["d_w0"], "the readout's weight gradient")
    for k, q in enumerate(R["reduce"]):
        for s in range(3):
            same(out["reduce"][k][s], (q["ref"] if ("reduce", k) in jobs else q["dW0"])[s], "reduce %d (%d workgroups), slot %d" % (k, q["n_wg"], s))
    f = R["first"][first_form]
    for s in range(3):
        same(out["first"][s], (f["ref"] if "first" in jobs else f["dW0"])[s], "the first layer's dW, form %d, slot %d" % (first_form, s))
    same(out["rc"], R["rc_ref"] if "rc" in jobs else _sentinel(out["rc"].shape), "the readout gradient's clear")
    for k, q in enumerate(R["clear"]):
        same(out["clear"][k], q["ref"] if ("clear", k) in jobs else _sentinel(out["clear"][k].shape), "masked clear %d" % k)


FULL = ["loss", "readout_dw", ("reduce", 0), ("reduce", 1), ("reduce", 2), "first", "rc", ("clear", 0), ("clear", 1)]
COMBOS = {"all": FULL, "two_layers": ["loss", "readout_dw", ("reduce", 2), "first", "rc"],
          "five_layers": ["loss", "readout_dw"] + [("reduce", k) for k in range(4)] + ["first", ("clear", 0), ("clear", 1)],
          "every_cap_full": ["loss"] + [("reduce", k) for k in range(4)] + [("clear", k) for k in range(4)],
          "no_masked_clear": [j for j in FULL if not (isinstance(j, tuple) and j[0] == "clear")], "nothing": []}
COMBOS.update({"without_%s" % (j if isinstance(j, str) else "%s%d" % j): [x for x in FULL if x != j] for j in FULL})


@pytest.mark.parametrize("name", sorted(COMBOS))
def test_every_job_has_its_stand_alone_launchs_bits(name):
    _need_gpu()
    jobs = COMBOS[name]
    st, out = _run(jobs)
    assert st == 0
    _assert_jobs(jobs, out)


def test_loss_overwrite_and_the_slab_pair_form_of_the_first_reduce():
    _need_gpu()
    st, out = _run(["loss", "first"], overwrite=1, first_form=2)
    assert st == 0
    _assert_jobs(["loss", "first"], out, overwrite=1, first_form=2)


def test_more_jobs_than_the_descriptor_holds_are_refused_before_any_launch():
    _need_gpu()
    for jobs in (FULL + [("reduce", 3), ("reduce", 4)], FULL + [("clear", 2), ("clear", 3), ("clear", 0)]):
        st, out = _run(jobs)
        assert st == SCN_ERR_BAD_SHAPE
        _assert_jobs([], out)


@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_partial_backwards_plus_epilogue_equal_the_reducing_backwards(act):
    """scn_conv_backward_visit_partial and scn_conv_backward_fused_first_from_y_visit_partial leave their reduces to the epilogue: dx and
    every weight gradient (accumulated into non-zero values) are the reducing entries' bits."""
    _need_gpu()
    from scone_gcn_amd import _lib, ops
    env = _env()
    rs = np.random.RandomState(7 + (act == "relu"))
    c = _bwd_case(env, act, S, "random", rs)
    plan = c["plan"]
    dW_ref, dx_ref = [t.clone() for t in c["dW0"]], _sentinel(c["dx"].shape)
    assert plan.conv_T.backward([c["dz"]], c["W"], c["aux"], act, True, dW_ref, dx=dx_ref, visit=c["mask"]) is not False
    f = _first_case(env, act, S, "random", rs)
    fW_ref, fF_ref = [t.clone() for t in f["dW0"]], [t.clone() for t in f["dWf0"]]
    assert f["plan"].conv_T.backward_fused_first(f["dz"], f["W"], None, act, f["y"], fW_ref, fF_ref, Ws_first=f["Wf"], visit=f["mask"])
    jobs = []
    dW, dx = [t.clone() for t in c["dW0"]], _sentinel(c["dx"].shape)
    assert plan.conv_T.backward([c["dz"]], c["W"], c["aux"], act, True, dW, dx=dx, visit=c["mask"], defer=jobs) is not False
    fW, fF = [t.clone() for t in f["dW0"]], [t.clone() for t in f["dWf0"]]
    assert f["plan"].conv_T.backward_fused_first(f["dz"], f["W"], None, act, f["y"], fW, fF, Ws_first=f["Wf"], visit=f["mask"], defer=jobs)
    torch.cuda.synchronize()
    assert [type(j) for j in jobs] == [ops.ReduceJob, ops.ReduceJob, ops.FirstReduceJob]
    for a, b in zip(dW + fW + fF, c["dW0"] + f["dW0"] + f["dWf0"]):
        assert np.array_equal(_bits(a), _bits(b)), "a deferred backward touched a weight gradient"
    d = _lib.StepEpilogueDesc()
    for job in jobs:
        if isinstance(job, ops.ReduceJob):
            q = d.reduce[d.n_reduce]
            assert job.partial == job.ws[0].value
            q.partial, q.n_wg, q.c_aux, q.c_dz = job.partial, job.n_wg, job.c_aux, job.c_dz
            for k in range(3):
                q.dW[k] = job.dWs[k].data_ptr()
            d.n_reduce += 1
        else:
            ch = f["dz"].shape[3]
            assert job.partial == job.ws[0].value + 4 * job.n_wg * 3 * ch * ch, "the first layer's partials lie behind the layer's own"
            d.first_form, d.first_partial, d.first_n_wg = 1, job.partial, job.n_wg
            for k in range(3):
                d.first_dW[k] = job.dWs[k].data_ptr()
    assert _lib.load().scn_step_epilogue(None, ctypes.byref(d), ops._stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dx), _bits(dx_ref)), "dx"
    for k, (a, b) in enumerate(zip(dW + fW + fF, dW_ref + fW_ref + fF_ref)):
        assert np.array_equal(_bits(a), _bits(b)), "weight gradient %d" % k
