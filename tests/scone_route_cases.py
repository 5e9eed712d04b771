"""The cases of the scone route table (tests/golden/scone_routes.json) and what is observed of each.

A case is one training step (forward, then backward) of a plain scone stack on the cfg1 golden complex with the batch of
tests/test_gpu_readout_cone.py::_data -- twelve trajectories plus a slab of padding, four slabs -- tanh throughout.  What is observed is
WHICH launches ran and what the forward's record says, never a value: the timer keys in order of first launch, per key the launches
and those that state a byte model, and the fields of the record that tests and tools read.  tools/record_scone_routes.py writes the
table, tests/test_gpu_scone_routes.py compares a tree with it, tests/test_host_scone_route.py holds ops.stack_route against it.

Only the public surface is used (a SconePlan as tests/test_gpu_readout_cone.py builds it, plan.forward / plan.backward, the ops
switches, the three SconePlan bounds, KernelTimer), so observe() runs unchanged on any revision that has the switches."""
import contextlib

SWITCHES = ("FUSE_FIRST", "RECOMPUTE_FIRST", "KEEP_LAST", "TOP_DZ_MASK", "READOUT_CONE", "CONE_UNIT_LIST")
BOUNDS = ("KEEP_LAST_MIN_BYTES", "SMALL_DZ_BYTES", "READOUT_CONE_MIN_BYTES")


def _case(name, hidden, layers, off=(), default_bounds=(), separate_conv_T=False, activity=None, slabs=None):
    """off: the switches that are False (every other one True); default_bounds: the bounds left at the class's value (every other one
    0); separate_conv_T: a second operator of the transposes stands for non-symmetric shifts; activity: a work-list mode;
    slabs: the batch repeated to this many slabs."""
    assert set(off) <= set(SWITCHES) and set(default_bounds) <= set(BOUNDS)
    return dict(name=name, hidden=hidden, layers=layers, off=tuple(off), default_bounds=tuple(default_bounds),
                separate_conv_T=separate_conv_T, activity=activity, slabs=slabs)


CASES = (
    # all switches on: five layers reach past UNIT_COUNTERS (the lowest mask has no list), two layers of 32 take the from-y-keep form
    [_case("%dx%d" % (layers, hidden), hidden, layers) for hidden in (16, 32) for layers in (1, 2, 3, 4, 5)]
    + [_case("3x24 promoted", 24, 3), _case("2x64 wide", 64, 2)]
    + [_case("3x32 %s off" % s, 32, 3, off=[s]) for s in SWITCHES]
    + [_case("3x32 READOUT_CONE and KEEP_LAST off", 32, 3, off=["READOUT_CONE", "KEEP_LAST"]),
       _case("3x32 default bounds", 32, 3, default_bounds=BOUNDS)]
    + [_case("3x32 default %s" % b, 32, 3, default_bounds=[b]) for b in BOUNDS]
    + [_case("3x32 separate conv_T", 32, 3, separate_conv_T=True)]
    + [_case("3x%d activity %s" % (hidden, mode), hidden, 3, activity=mode) for hidden in (32, 16) for mode in ("zeros", "field")]
    + [_case("3x32 65 slabs", 32, 3, slabs=65)]
)
assert len({c["name"] for c in CASES}) == len(CASES)


@contextlib.contextmanager
def configured(case, ops):
    """The switches and bounds of a case set on `ops` / `ops.SconePlan`, and put back."""
    before = [(ops, s, getattr(ops, s)) for s in SWITCHES] + [(ops.SconePlan, b, getattr(ops.SconePlan, b)) for b in BOUNDS]
    try:
        for s in SWITCHES:
            setattr(ops, s, s not in case["off"])
        for b in BOUNDS:
            if b not in case["default_bounds"]:
                setattr(ops.SconePlan, b, 0)
        yield
    finally:
        for obj, name, value in before:
            setattr(obj, name, value)


def observe(case):
    """One step of the case on a plan of its own (needs a GPU); the observations as plain JSON values."""
    import numpy as np
    import torch
    from oracle import scone_oracle as so
    from scone_gcn_amd import ops
    from tests.test_gpu_readout_cone import _data, _env
    env, d = _env(), _data()
    plan = env["plan"](fresh=True)
    if case["separate_conv_T"]:                 # (as tests/test_gpu_readout_cone.py::test_refused_cases_give_todays_results builds it)
        lo, up = (s.device_csr() for s in plan._shift_pair)
        E = lo.shape[0]
        plan.conv_T = ops.ConvOp(E, [{"mats": [lo.T.tocsr(), up.T.tocsr()], "identity": True, "n_cols": E}],
                                 plan.layout.block_starts[plan._shift_pair[0].row_level])
    x, last_dev, y_dev = d["x"], d["last_dev"], d["y_dev"]
    if case["slabs"]:
        S, rep = case["slabs"], -(-case["slabs"] // x.shape[0])
        x = torch.cat([x] * rep)[:S].contiguous()
        last_dev = last_dev.repeat(rep)[:S * ops.NS].contiguous()
        y_dev = torch.cat([y_dev] * rep)[:S * ops.NS].contiguous()
    rs = np.random.RandomState(17)
    w = [torch.tensor(0.3 * rs.randn(*s), dtype=torch.float32, device="cuda")
         for s in so.weight_shapes(1, [(3, case["hidden"])] * case["layers"], 1)]
    activity = None
    if case["activity"]:
        activity = plan.activity(d["flows"], d["last"], case["layers"], case["hidden"], case["activity"])
        assert activity is not None
    with configured(case, ops), ops.KernelTimer() as kt:
        logp, saved = plan.forward(x, last_dev, w, activity) if activity is not None else plan.forward(x, last_dev, w)
        grads = [torch.zeros_like(a) for a in w]
        plan.backward(saved, logp, -y_dev / d["N"], last_dev, w, grads)
    torch.cuda.synchronize()
    cone = saved.cone
    return {"x_shape": list(x.shape),
            "keys": list(kt.records),
            "launches": {k: [len(v), sum(1 for _, _, nbytes in v if nbytes is not None)] for k, v in kt.records.items()},
            "cone": cone is not None,
            "units": [u is not None for u in cone.units] if cone is not None and cone.units is not None else None,
            "h1_rebuilt": saved.hs[1] is None,
            "y0": saved.y0 is not None,
            "wide": bool(saved.wide)}
