"""What a plan's forward hands its backward belongs to that call alone.

Plans are cached and shared (ops.get_scone_plan / get_bunch_plan): one plan serves training, evaluation and the multi-hop forwards,
and stacks of different shapes take different paths through it (the Bunch fold, the recompute-first, wide and plain scone stacks).
Here several forwards of different shapes run on ONE plan before any backward, and the backwards consume the saved records in reverse
order: log-probabilities and every weight gradient must equal, bit for bit, the same stack run alone on the same plan.  Bit for bit
because the same launches see the same inputs either way and the step is reproducible from run to run (per-workgroup partials summed
in a fixed order, no float atomics: tools/determinism.py).  The golden config-1 complex, 8 trajectories.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import scone_oracle as so

pytestmark = pytest.mark.gpu

SEL = np.arange(8)


@pytest.fixture(scope="module")
def sc1(cfg1):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from scone_gcn_amd.complex import SimplicialComplex
    from scone_gcn_amd.synthetic_data_gen import Complex
    cx = Complex(n_nodes=cfg1["n_nodes"], edges=cfg1["edges"].astype(np.int64), faces=cfg1["faces"].astype(np.int64),
                 coords=cfg1["coords"])
    return SimplicialComplex(cx)


def _stack(layers, model, scale, seed, n_rows, D):
    """(weights, d_logp) of one stack: seeded, on the device."""
    rs = np.random.RandomState(seed)
    w = [torch.tensor(scale * rs.randn(*s), dtype=torch.float32, device="cuda") for s in so.weight_shapes(1, layers, 1, model)]
    return w, torch.tensor(rs.randn(n_rows, D).astype(np.float32), device="cuda")


def _alone(plan, x, last, stack):
    w, d_logp = stack
    logp, saved = plan.forward(x, last, w)
    grads = [torch.zeros_like(a) for a in w]
    plan.backward(saved, logp, d_logp, last, w, grads)
    return logp.clone(), grads


def _interleaved(plan, x, last, stacks):
    """Every forward first, in order; then the backwards in reverse order.  Returns ([(logp, grads)], [saved])."""
    fwd = [plan.forward(x, last, w) for w, _ in stacks]
    out = [None] * len(stacks)
    for k in reversed(range(len(stacks))):
        w, d_logp = stacks[k]
        logp, saved = fwd[k]
        grads = [torch.zeros_like(a) for a in w]
        plan.backward(saved, logp, d_logp, last, w, grads)
        out[k] = (logp.clone(), grads)
    return out, [s for _, s in fwd]


def _bunch(cfg1, sc1):
    from scone_gcn_amd import ops, trajectory_experiments as te
    dev = ops.default_device()
    shifts, nbrhoods, _ = te.setup_from_complex(sc1, "bunch")
    plan = ops.get_bunch_plan(shifts, nbrhoods, dev)                       # the cached plan every caller of this complex shares
    x, _ = ops.flows_to_slabs(cfg1["flows"][SEL], sc1.layout, dev)
    last = ops._last_nodes_dev(cfg1["last_nodes"][SEL], x.shape[0] * ops.NS, dev)
    n = x.shape[0] * ops.NS
    # A: three layers, hidden 32 -- the first two as the rank-one fold; B: two layers, hidden 8 -- promoted to 16, per shift, no fold
    stacks = [_stack([(7, 32)] * 2, "bunch", 0.4, 5, n, plan.max_deg), _stack([(7, 8)], "bunch", 0.4, 6, n, plan.max_deg)]
    return plan, x, last, stacks


def _scone(cfg1, sc1):
    from scone_gcn_amd import ops, trajectory_experiments as te
    dev = ops.default_device()
    shifts, readout, _ = te.setup_from_complex(sc1, "scone")
    plan = ops.get_scone_plan(shifts[0], shifts[1], readout, "tanh", dev)
    assert type(plan) is ops.SconePlan
    x, _ = ops.flows_to_slabs(cfg1["flows"][SEL], sc1.layout, dev)
    last = ops._last_nodes_dev(cfg1["last_nodes"][SEL], x.shape[0] * ops.NS, dev)
    n = x.shape[0] * ops.NS
    # recompute-first (hidden 32, three layers: H1 is never stored), wide (hidden 64: 32-channel blocks), plain hidden 16
    stacks = [_stack([(3, 32)] * 3, "scone", 0.25, 7, n, plan.max_deg), _stack([(3, 64)] * 2, "scone", 0.25, 8, n, plan.max_deg),
              _stack([(3, 16)] * 2, "scone", 0.25, 9, n, plan.max_deg)]
    return plan, x, last, stacks


def _assert_same(got, ref, what):
    # (not vacuous; per weight would ask too much: Bunch slots from an all-zero level or into an unread one rightly see no gradient)
    assert float(ref[0].abs().max()) > 0 and max(float(g.abs().max()) for g in ref[1]) > 0, what
    assert torch.equal(got[0], ref[0]), "%s: logp" % what
    for k, (a, b) in enumerate(zip(got[1], ref[1])):
        assert torch.equal(a, b), "%s: gradient of weight %d" % (what, k)


@pytest.mark.parametrize("family", ["bunch", "scone"])
def test_interleaved_forwards_equal_each_stack_run_alone(cfg1, sc1, family):
    plan, x, last, stacks = (_bunch if family == "bunch" else _scone)(cfg1, sc1)
    alone = [_alone(plan, x, last, st) for st in stacks]
    mixed, _ = _interleaved(plan, x, last, stacks)
    for k in range(len(stacks)):
        _assert_same(mixed[k], alone[k], "%s stack %d" % (family, k))
    again = [_alone(plan, x, last, st) for st in stacks]                   # ... and the plan is as it was
    for k in range(len(stacks)):
        _assert_same(again[k], alone[k], "%s stack %d, alone once more" % (family, k))


def test_saved_records_expose_their_fields_by_name(cfg1, sc1):
    """The records say by name which path their forward took -- the backward reads that, never a position or a length -- and the
    promoted weights have the same name on both."""
    from scone_gcn_amd import ops
    plan, x, last, stacks = _bunch(cfg1, sc1)
    _, (a, b) = _interleaved(plan, x, last, stacks)
    assert isinstance(a, ops.BunchState) and isinstance(b, ops.BunchState)
    assert a.fold is not None and a.promoted is None and a.states[1] == [None] * 3       # the fold: layer 1 never materialised
    assert b.fold is None and b.first_g and [tuple(w.shape) for w in b.promoted[:7]] == [(1, 16)] * 7
    assert len(a.zeros) == len(a.states) == 4 and len(b.zeros) == len(b.states) == 3
    plan, x, last, stacks = _scone(cfg1, sc1)
    _, (r, w, p) = _interleaved(plan, x, last, stacks)
    assert all(isinstance(s, ops.SconeState) for s in (r, w, p))
    assert (r.wide, w.wide, p.wide) == (False, True, False)
    assert r.hs[1] is None and r.y0 is not None and r.promoted is None                     # recompute-first: H1 is not stored
    assert [len(blocks) for blocks in w.hs[1:]] == [2, 2] and len(w.bh) == 2               # two 32-channel blocks per layer
    assert p.hs[1] is not None and tuple(p.hs[-1].shape[2:]) == (ops.NS, 16) and p.promoted is None
    assert r.activity is None and w.activity is None and p.activity is None
