"""The cone step with its tail in two launches (ops.STEP_TAIL, SconePlan.step: scn_readout_step + scn_step_epilogue) against the separate
calls (forward, scn_masked_ce_begin, backward), BIT FOR BIT on the loss and every weight gradient, at the plan and at the trainer.

  * 2, 3, 4 and 5 layers of 32 at 4 slabs and at 33 (two mask words); two layers have no cone: the step declines and the caller's
    separate calls run;
  * two consecutive steps on one plan that end at different last nodes: the pooled gradient buffers are all-zero after each and as
    many as the separate calls leave (a deferred clear must not raise the pool's peak);
  * step(), the separate calls and step() again on ONE plan of four layers: the one pool both feed is all-zero and as large after each,
    and each micro-batch equals the same one on a fresh plan;
  * Scone_GCN._accumulate_staged over two micro-batches with fresh = True and the flat gradient buffer pre-filled with garbage;
  * hidden 16, READOUT_CONE off and a PowerPlan: declined, today's results;
  * the launches of a 3 x 32 step: the two new entries once each, the four readout / loss entries they replace not at all, one
    launch under the masked clear's timer key;
  * one step captured with torch.cuda.graph and replayed equals the eager step; every launch of the capture went to the one
    capturing stream (a single chain, no parallel branches).

The complex and batch of tests/test_gpu_readout_cone.py (cfg1 golden, |E| = 1001, twelve trajectories and a padding slab), the plan's
three size bounds set to 0 as there."""
import ctypes
import gc

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import scone_oracle as so
from tests.test_gpu_keep_last import _need_gpu, _same_bits
from tests.test_gpu_readout_cone import _data, _env, _pools_all_zero, _thresholds

pytestmark = pytest.mark.gpu


def _weights(layers, hidden=32, seed=41):
    rs = np.random.RandomState(seed)
    return [torch.tensor(0.3 * rs.randn(*s), dtype=torch.float32, device="cuda") for s in so.weight_shapes(1, [(3, hidden)] * layers, 1)]


def _batch(slabs=4):
    """(x, last nodes, targets, trajectories) of the golden batch, tiled to `slabs` slabs."""
    d = _data()
    if slabs == 4:
        return d["x"], d["last_dev"], d["y_dev"], d["N"]
    reps = -(-slabs // 4)
    x = torch.cat([d["x"]] * reps)[:slabs].contiguous()
    return x, torch.cat([d["last_dev"]] * reps)[:4 * slabs].contiguous(), torch.cat([d["y_dev"]] * reps)[:4 * slabs].contiguous(), 3 * d["N"]


def _micro(plan, w, on, monkeypatch, batch, grads=None, last_dev=None):
    """One micro-batch the way the trainer runs it: (the step ran, loss [1] fp64, grads)."""
    from scone_gcn_amd import _lib, ops
    monkeypatch.setattr(ops, "STEP_TAIL", on)
    x, last, yt, n = batch
    last = last if last_dev is None else last_dev
    part = torch.full((1,), 7.0, device="cuda", dtype=torch.float64)
    grads = [torch.zeros_like(a) for a in w] if grads is None else grads
    ran = plan.step(x, last, yt, -1.0 / n, w, grads, part, overwrite=True)
    if not ran:
        logp, saved = plan.forward(x, last, w)
        d_logp = torch.empty_like(logp)
        _lib.check(_lib.load().scn_masked_ce_begin(logp.numel(), ops._dev(logp), ops._dev(yt), -1.0 / n, ops._dev(d_logp),
                                                   ctypes.c_void_p(part.data_ptr()), 1, None, 0, ops._stream()), "scn_masked_ce_begin")
        plan.backward(saved, logp, d_logp, last, w, grads)
    torch.cuda.synchronize()
    return ran, part, grads


def _assert_same(a, b, what):
    _same_bits(a[1].view(torch.int32), b[1].view(torch.int32), "loss, " + what)
    for k, (p, q) in enumerate(zip(a[2], b[2])):
        _same_bits(p, q, "gradient of weight %d, %s" % (k, what))
    assert max(float(g.abs().max()) for g in a[2]) > 0 and float(a[1]) != 7.0


@pytest.mark.parametrize("slabs", [4, 33])
@pytest.mark.parametrize("layers", [2, 3, 4, 5])
def test_step_tail_on_against_off(layers, slabs, monkeypatch):
    _need_gpu()
    _thresholds(monkeypatch)
    plan, w, batch = _env()["plan"](fresh=True), _weights(layers), _batch(slabs)
    on = _micro(plan, w, True, monkeypatch, batch)
    assert on[0] == (layers >= 3), "the step runs wherever the stack has a cone"
    assert layers < 3 or _pools_all_zero(plan)
    n_on = sum(len(v) for v in plan._dz_zero.values())
    ref = _env()["plan"](fresh=True)
    off = _micro(ref, w, False, monkeypatch, batch)
    assert not off[0]
    _assert_same(on, off, "%d layers, %d slabs" % (layers, slabs))
    assert n_on == sum(len(v) for v in ref._dz_zero.values()), "the pool's size is the separate calls'"


def test_two_steps_with_different_last_nodes_on_one_plan(monkeypatch):
    _need_gpu()
    _thresholds(monkeypatch)
    env, batch = _env(), _batch()
    w = _weights(4, seed=23)
    rs = np.random.RandomState(23)
    other = torch.as_tensor(rs.randint(0, env["plan"]().n_nodes, size=batch[1].numel()).astype(np.int32), device="cuda")
    plans = {on: env["plan"](fresh=True) for on in (True, False)}
    for k, last in enumerate((batch[1], other, batch[1])):
        res = {}
        for on in (True, False):
            res[on] = _micro(plans[on], w, on, monkeypatch, batch, last_dev=last)
            assert res[on][0] == on and _pools_all_zero(plans[on])
        _assert_same(res[True], res[False], "step %d" % k)
        assert sum(len(v) for v in plans[True]._dz_zero.values()) == sum(len(v) for v in plans[False]._dz_zero.values())


def test_step_and_separate_calls_interleaved_on_one_plan_share_the_pool(monkeypatch):
    """step(), the separate calls, step() again on ONE plan: both hand their gradient buffers to one pool through one loop
    (SconePlan._cone_backward).  Four layers: the smallest stack with an inline release and a deferred clear."""
    _need_gpu()
    _thresholds(monkeypatch)
    env, batch = _env(), _batch()
    w = _weights(4, seed=23)
    rs = np.random.RandomState(23)
    other = torch.as_tensor(rs.randint(0, env["plan"]().n_nodes, size=batch[1].numel()).astype(np.int32), device="cuda")
    plan, n_first = env["plan"](fresh=True), None
    for k, (on, last) in enumerate(((True, batch[1]), (False, other), (True, batch[1]))):
        res = _micro(plan, w, on, monkeypatch, batch, last_dev=last)
        assert res[0] == on and _pools_all_zero(plan)
        n = sum(len(v) for v in plan._dz_zero.values())
        n_first = n if n_first is None else n_first
        assert n == n_first > 0, "micro-batch %d left %d pooled buffers, the first %d" % (k, n, n_first)
        _assert_same(res, _micro(env["plan"](fresh=True), w, on, monkeypatch, batch, last_dev=last), "micro-batch %d against a fresh plan" % k)


def test_the_trainers_loop_over_two_micro_batches_into_a_garbage_gradient_buffer(monkeypatch):
    _need_gpu()
    from scone_gcn_amd import ops, scone_trajectory_model as stm
    _thresholds(monkeypatch)
    monkeypatch.setattr(ops, "SMALL_STEP", False)
    env, d = _env(), _data()
    te, N = env["te"], d["N"]
    shifts, readout, _ = te.setup_from_complex(env["sc"], "scone")
    inputs = [readout, d["last"], d["flows"]]
    y = np.asarray(d["y"])
    stm.reseed(1030)
    net = stm.Scone_GCN(1, 1e-3, N, 0.0, verbose=False)
    net.setup(te.scone_func, [(3, 32)] * 3, shifts, inputs, y, None, np.ones(N, int), model_type="scone")
    plan = net._plan(inputs)
    assert type(plan) is ops.SconePlan
    staged = net.stage(inputs, y, np.arange(0, 8)) + net.stage(inputs, y, np.arange(8, N))
    assert len(staged) == 2
    calls = []
    real = ops.SconePlan.step
    monkeypatch.setattr(ops.SconePlan, "step", lambda self, *a, **k: calls.append(real(self, *a, **k)) or calls[-1])
    res = {}
    for on in (True, False):
        monkeypatch.setattr(ops, "STEP_TAIL", on)
        del calls[:]
        net._flat_g.copy_(torch.as_tensor(np.random.RandomState(5).randn(net._flat_g.numel()).astype(np.float32) * 1e3))
        loss = net._accumulate_staged(plan, staged, N, fresh=True)
        torch.cuda.synchronize()
        assert calls == [on, on]
        res[on] = (loss.detach().clone().reshape(1), net._flat_g.detach().clone())
    _same_bits(res[True][0].view(torch.int32), res[False][0].view(torch.int32), "loss")
    _same_bits(res[True][1], res[False][1], "the flat gradient")
    assert bool(torch.isfinite(res[True][1]).all()) and float(res[True][1].abs().max()) > 0


@pytest.mark.parametrize("case", ["hidden16", "cone_off", "power_plan"])
def test_declined_cases_give_todays_results(case, monkeypatch):
    _need_gpu()
    from scone_gcn_amd import ops
    _thresholds(monkeypatch)
    env, batch = _env(), _batch()
    if case == "cone_off":
        monkeypatch.setattr(ops, "READOUT_CONE", False)
    w = _weights(3, hidden=16 if case == "hidden16" else 32)

    def plan():
        if case != "power_plan":
            return env["plan"](fresh=True)
        shifts, readout, _ = env["te"].setup_from_complex(env["sc"], "scone")
        return ops.PowerPlan(shifts[0], shifts[1], readout, "tanh", ops.default_device())
    on = _micro(plan(), w, True, monkeypatch, batch)
    off = _micro(plan(), w, False, monkeypatch, batch)
    assert not on[0] and not off[0]
    _assert_same(on, off, case)


def test_launches_of_a_three_layer_step(monkeypatch):
    _need_gpu()
    from scone_gcn_amd import _lib, ops
    _thresholds(monkeypatch)
    plan, w, batch = _env()["plan"](fresh=True), _weights(3), _batch()
    _micro(plan, w, True, monkeypatch, batch)                                  # (tables, pooled buffers)
    lib = _lib.load()
    names = ["scn_readout_step", "scn_step_epilogue", "scn_readout_forward", "scn_masked_ce_begin", "scn_masked_ce", "scn_readout_backward",
             "scn_readout_clear_dz", "scn_clear_mask", "scn_conv_backward_visit", "scn_conv_backward_fused_first_from_y_visit",
             "scn_conv_backward_visit_partial", "scn_conv_backward_fused_first_from_y_visit_partial"]
    count = dict.fromkeys(names, 0)

    class Counting:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name not in count:
                return fn

            def call(*a):
                count[name] += 1
                return fn(*a)
            return call
    monkeypatch.setattr(_lib, "load", lambda: Counting())
    with ops.KernelTimer() as kt:
        ran, _, _ = _micro(plan, w, True, monkeypatch, batch)
    assert ran
    table = kt.table()
    assert {k: v for k, v in count.items() if v} == {"scn_readout_step": 1, "scn_step_epilogue": 1, "scn_conv_backward_visit_partial": 1,
                                                     "scn_conv_backward_fused_first_from_y_visit_partial": 1}
    assert table["clear_mask"]["launches"] == 1 and table["clear_mask"]["alg_bytes"] is None
    # the timed launches: y, two kept forwards, the masks' three, two backwards, the epilogue
    assert sum(r["launches"] for r in table.values()) == 9, {k: r["launches"] for k, r in table.items()}


def test_a_captured_step_replays_the_eager_step(monkeypatch):
    _need_gpu()
    from scone_gcn_amd import _lib, ops
    _thresholds(monkeypatch)
    monkeypatch.setattr(ops, "STEP_TAIL", True)
    plan, w, (x, last, yt, n) = _env()["plan"](fresh=True), _weights(3), _batch()
    eager = _micro(plan, w, True, monkeypatch, (x, last, yt, n))               # (also builds the tables and the pooled buffers)
    assert eager[0]
    part = torch.zeros((1,), device="cuda", dtype=torch.float64)
    grads = [torch.zeros_like(a) for a in w]
    lib, streams = _lib.load(), set()

    class Recording:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith("scn_") or fn.argtypes is None or not fn.argtypes or fn.restype is not ctypes.c_int:
                return fn

            def call(*a):
                if isinstance(a[-1], ctypes.c_void_p):
                    streams.add(a[-1].value)
                return fn(*a)
            return call
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    # as Scone_GCN._graph_accumulate does: torch.cuda.graph no longer collects garbage before a capture, and a dead cycle of an earlier
    # test that still holds device memory would be freed whenever the collector next runs -- a free inside the capture invalidates it
    torch.cuda.synchronize()
    gc.collect()
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.stream(side):
            monkeypatch.setattr(_lib, "load", lambda: Recording())
            with torch.cuda.graph(g, stream=side):
                capture_stream = torch.cuda.current_stream().cuda_stream
                assert plan.step(x, last, yt, -1.0 / n, w, grads, part, overwrite=True)
            monkeypatch.setattr(_lib, "load", lambda: lib)
    finally:
        if gc_was_on:
            gc.enable()
    torch.cuda.current_stream().wait_stream(side)
    assert streams == {capture_stream}, "every launch of the capture goes to the one capturing stream: a single chain"
    for _ in range(2):
        for t in grads:
            t.zero_()
        part.fill_(3.0)
        g.replay()
        torch.cuda.synchronize()
        _assert_same((True, part, grads), eager, "replay")
    assert _pools_all_zero(plan)
