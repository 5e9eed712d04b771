"""The trainer's micro-batch loop with the cone masks of the whole step from one launch (ops.STEP_MASKS, SconePlan.step_cones,
scn_cone_masks) against each micro-batch building its own (scn_keep_mask_units + two scn_mask_hop_units and their memset), BIT FOR BIT
on the loss and the flat gradient, the pooled gradient buffers all-zero afterwards.

  * Scone_GCN._accumulate_staged over three micro-batches of four trajectories, switch on against off;
  * the launches with the switch on: one under the timer key "cone_masks" per call, none under "keep_mask" / "dz_mask_hop", and no
    call of an entry that memsets a mask (scn_keep_mask, scn_keep_mask_units);
  * a single micro-batch through the captured graph (Scone_GCN._graph_accumulate: eager, capture, replays) gives the eager bits, the
    new launch inside the capture;
  * step_cones declining (the limit patched down to three words; the library's refusal): every micro-batch builds its own masks as
    today, the same bits.

The complex and batch of tests/test_gpu_readout_cone.py (cfg1 golden, |E| = 1001), the plan's three size bounds set to 0 and the
one-launch small step off, as tests/test_gpu_step_tail.py does."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_keep_last import _need_gpu, _same_bits
from tests.test_gpu_readout_cone import _data, _env, _pools_all_zero, _thresholds

pytestmark = pytest.mark.gpu

MASK_ENTRIES = ["scn_cone_masks", "scn_keep_mask", "scn_keep_mask_units", "scn_mask_hop", "scn_mask_hop_units"]


def _net(monkeypatch):
    """(net, plan, the three staged micro-batches, N) on the golden complex; the switches every test here runs under."""
    from scone_gcn_amd import ops, scone_trajectory_model as stm
    _thresholds(monkeypatch)
    monkeypatch.setattr(ops, "SMALL_STEP", False)
    monkeypatch.setattr(ops, "STEP_TAIL", True)
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
    staged = net.stage(inputs, y, np.arange(0, 4)) + net.stage(inputs, y, np.arange(4, 8)) + net.stage(inputs, y, np.arange(8, N))
    assert len(staged) == 3
    return net, plan, staged, N


def _counting(mp):
    """Counts the calls of the mask entries while the patch context `mp` lasts: the dict."""
    from scone_gcn_amd import _lib
    lib = _lib.load()
    count = dict.fromkeys(MASK_ENTRIES, 0)

    class Counting:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name not in count:
                return fn

            def call(*a):
                count[name] += 1
                return fn(*a)
            return call
    mp.setattr(_lib, "load", lambda: Counting())
    return count


def _run(net, plan, staged, N, on, patch=None):
    """One _accumulate_staged into a garbage gradient buffer with STEP_MASKS = on: (loss [1], flat gradient, timer table, calls of the
    mask entries, (what SconePlan.step returned, whether it was handed a cone) per micro-batch).  patch(mp): further patches."""
    from scone_gcn_amd import ops
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "STEP_MASKS", on)
        if patch is not None:
            patch(mp)
        calls = []
        real = ops.SconePlan.step
        mp.setattr(ops.SconePlan, "step", lambda self, *a, **k: calls.append((real(self, *a, **k), k.get("cone") is not None)) or calls[-1][0])
        count = _counting(mp)
        net._flat_g.copy_(torch.as_tensor(np.random.RandomState(5).randn(net._flat_g.numel()).astype(np.float32) * 1e3))
        with ops.KernelTimer() as kt:
            loss = net._accumulate_staged(plan, staged, N, fresh=True)
        torch.cuda.synchronize()
        table = kt.table()
    assert _pools_all_zero(plan)
    return loss.detach().clone().reshape(1), net._flat_g.detach().clone(), table, count, calls


def _assert_same(a, b, what):
    _same_bits(a[0].view(torch.int32), b[0].view(torch.int32), "loss, " + what)
    _same_bits(a[1], b[1], "the flat gradient, " + what)
    assert bool(torch.isfinite(a[1]).all()) and float(a[1].abs().max()) > 0


def test_three_micro_batches_on_against_off(monkeypatch):
    _need_gpu()
    net, plan, staged, N = _net(monkeypatch)
    _run(net, plan, staged, N, False)                                          # (tables, pooled buffers)
    on, off, again = _run(net, plan, staged, N, True), _run(net, plan, staged, N, False), _run(net, plan, staged, N, True)
    _assert_same(on, off, "STEP_MASKS on against off")
    _assert_same(again, off, "STEP_MASKS on, a second call")
    # the launches: one for the masks of all three micro-batches, none of today's three per micro-batch, no entry that memsets a mask
    assert on[4] == [(True, True)] * 3 and off[4] == [(True, False)] * 3, "every micro-batch took the cone step"
    assert on[2]["cone_masks"]["launches"] == 1 and on[2]["cone_masks"]["alg_bytes"] > 0
    assert "keep_mask" not in on[2] and "dz_mask_hop" not in on[2]
    assert on[3] == {"scn_cone_masks": 1, "scn_keep_mask": 0, "scn_keep_mask_units": 0, "scn_mask_hop": 0, "scn_mask_hop_units": 0}
    assert "cone_masks" not in off[2] and off[2]["keep_mask"]["launches"] == 3 and off[2]["dz_mask_hop"]["launches"] == 6
    assert off[3] == {"scn_cone_masks": 0, "scn_keep_mask": 0, "scn_keep_mask_units": 3, "scn_mask_hop": 0, "scn_mask_hop_units": 6}
    launches = lambda t: sum(r["launches"] for r in t.values())
    assert launches(off[2]) - launches(on[2]) == 3 * 3 - 1, "three timed launches fewer per micro-batch, one more per call"


@pytest.mark.parametrize("who", ["the wrapper's limit", "the library"])
def test_a_declined_step_cones_falls_back_to_todays_launches(who, monkeypatch):
    _need_gpu()
    from scone_gcn_amd import ops
    net, plan, staged, N = _net(monkeypatch)
    served = _run(net, plan, staged, N, True)
    if who == "the library":                   # (ConvOp.cone_masks returns None for SCN_ERR_UNSUPPORTED)
        declined = _run(net, plan, staged, N, True, lambda mp: mp.setattr(ops.ConvOp, "cone_masks", lambda self, *a, **k: None))
    else:
        declined = _run(net, plan, staged, N, True, lambda mp: mp.setattr(ops, "cone_masks_limit", lambda: 3))
    _assert_same(declined, served, "step_cones declined against served")
    assert served[4] == [(True, True)] * 3 and served[3]["scn_cone_masks"] == 1
    assert declined[4] == [(True, False)] * 3, "the step runs, on masks of its own"
    assert declined[3] == {"scn_cone_masks": 0, "scn_keep_mask": 0, "scn_keep_mask_units": 3, "scn_mask_hop": 0, "scn_mask_hop_units": 6}


def test_a_captured_single_micro_batch_replays_the_eager_step(monkeypatch):
    _need_gpu()
    from scone_gcn_amd import ops
    net, plan, staged, N = _net(monkeypatch)
    monkeypatch.setattr(ops, "STEP_MASKS", True)
    one = staged[2:3]
    eager_loss = net._accumulate_staged(plan, one, N, fresh=True).detach().clone().reshape(1)
    torch.cuda.synchronize()
    eager = (eager_loss, net._flat_g.detach().clone())
    with pytest.MonkeyPatch.context() as mp:
        count = _counting(mp)
        first = net._graph_accumulate(plan, one, N)                    # eager once more, then the capture
        torch.cuda.synchronize()
        assert count["scn_cone_masks"] == 2 and count["scn_keep_mask_units"] == 0 and count["scn_mask_hop_units"] == 0, count
        _assert_same((first.detach().clone().reshape(1), net._flat_g.detach().clone()), eager, "the call that captures")
        for k in range(2):
            net._flat_g.fill_(float("nan"))
            loss = net._graph_accumulate(plan, one, N)                 # a replay
            torch.cuda.synchronize()
            assert count["scn_cone_masks"] == 2, "a replay launches through the graph"
            _assert_same((loss.detach().clone().reshape(1), net._flat_g.detach().clone()), eager, "replay %d" % k)
    assert _pools_all_zero(plan)
    net._drop_graphs(0)
