"""Host tests of ops.stack_route, the one function that decides how a plain scone stack runs: it takes plain
facts and touches no tensor, so it runs here.

  * Against tests/golden/scone_routes.json: for every case of tests/scone_route_cases.py the route it returns agrees with what a
    step of that case was seen to do on the GPU -- the cone, the unit lists, a stored or rebuilt H1, and the launches "keep_mask",
    "dz_mask", "... + dW_first" and "clear_mask".
  * Facts no GPU case reaches, each alone on three layers of 32 that otherwise take the cone: no mask of any kind.
  * Non-symmetric shifts keep the kept last layer and lose the top mask and the cone.
  * The fall-backs: a declined cone gives way to the stack in full with its kept last layer, a declined from-y pair to a stored H1."""
import json
import os

import pytest

torch = pytest.importorskip("torch")

from tests.scone_route_cases import CASES, configured

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scone_routes.json")) as f:
    GOLDEN = json.load(f)
X_SHAPE = (4, 1001, 4, 1)              # the batch of the table on the cfg1 complex


def _facts(hidden, layers, x_shape=X_SHAPE, **other):
    """stack_route's arguments for a stack on a plain scone plan with everything in place, the bounds as they stand now."""
    from scone_gcn_amd import ops
    h = ops.promoted_width([hidden] * layers, wide=True) or hidden
    shapes = [(1, h)] * 3 + [(h, h)] * (3 * (layers - 1)) + [(h, 1)]
    facts = dict(activity=False, last_dev=(x_shape[0] * x_shape[2], torch.int32), fused_conv=True, symmetric=True, blocked=True,
                 tables=True, tables_built=True, capturing=False, keep_last_min=ops.SconePlan.KEEP_LAST_MIN_BYTES,
                 small_dz=ops.SconePlan.SMALL_DZ_BYTES, cone_min=ops.SconePlan.READOUT_CONE_MIN_BYTES)
    facts.update(other)
    return (tuple(x_shape), shapes), facts


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_route_agrees_with_what_the_step_was_seen_to_do(case):
    from scone_gcn_amd import ops
    seen = GOLDEN[case["name"]]
    keys, L = seen["keys"], case["layers"]
    if seen["wide"]:                            # 32-channel blocks: SconePlan._wide_stack, which takes no route
        assert ops.promoted_width([case["hidden"]] * L, wide=True) > 32
        return
    with configured(case, ops):
        args, facts = _facts(case["hidden"], L, seen["x_shape"], activity=case["activity"] is not None,
                             symmetric=not case["separate_conv_T"], tables_built=False)
        route = ops.stack_route(*args, **facts)
    print(case["name"], route)
    assert route.cone == seen["cone"]
    assert route.units == (seen["units"] is not None)
    if route.units:                             # a mask beyond the counters has no list
        assert seen["units"] == [k < ops.UNIT_COUNTERS for k in range(L)]
    assert (route.first == "from_y") == seen["h1_rebuilt"]
    assert (route.first != "plain") == seen["y0"]
    assert route.keep_last == ("keep_mask" in keys)
    assert (route.top_dz_mask and not route.cone) == ("dz_mask" in keys)
    assert (route.fused_first and L >= 2) == any(k.endswith("+ dW_first") for k in keys)
    assert route.cone == ("clear_mask" in keys)
    assert not route.cone or (route.keep_last and route.top_dz_mask and route.first == "from_y")


def _zero_bounds(monkeypatch):
    from scone_gcn_amd import ops
    for name in ("KEEP_LAST_MIN_BYTES", "SMALL_DZ_BYTES", "READOUT_CONE_MIN_BYTES"):
        monkeypatch.setattr(ops.SconePlan, name, 0)


UNREACHED = {"no last_dev": dict(last_dev=None),
             "last_dev int64": dict(last_dev=(16, torch.int64)),
             "last_dev of another count": dict(last_dev=(15, torch.int32)),
             "ns != 4": dict(x_shape=(4, 1001, 2, 1), last_dev=(8, torch.int32)),
             "not blocked": dict(blocked=False),
             "no tables (a probed closure)": dict(tables=False),
             "tables first built under a capture": dict(tables_built=False, capturing=True),
             "activity given": dict(activity=True),
             "fused_conv false": dict(fused_conv=False)}


@pytest.mark.parametrize("fact", sorted(UNREACHED))
def test_a_fact_no_gpu_case_reaches_takes_every_mask_away(fact, monkeypatch):
    from scone_gcn_amd import ops
    _zero_bounds(monkeypatch)
    args, facts = _facts(32, 3)
    assert ops.stack_route(*args, **facts) == ops.StackRoute("from_y", True, True, True, True, True)
    args, facts = _facts(32, 3, **UNREACHED[fact])
    route = ops.stack_route(*args, **facts)
    print(fact, route)
    assert not (route.keep_last or route.top_dz_mask or route.cone or route.units)


def test_tables_built_earlier_serve_under_a_capture(monkeypatch):
    from scone_gcn_amd import ops
    _zero_bounds(monkeypatch)
    args, facts = _facts(32, 3, tables_built=True, capturing=True)
    assert ops.stack_route(*args, **facts).cone


def test_non_symmetric_shifts_keep_the_kept_last_layer_only(monkeypatch):
    from scone_gcn_amd import ops
    _zero_bounds(monkeypatch)
    args, facts = _facts(32, 3, symmetric=False)
    assert ops.stack_route(*args, **facts) == ops.StackRoute("from_y", keep_last=True, cone=False, units=False, top_dz_mask=False,
                                                             fused_first=True)


def test_fallbacks(monkeypatch):
    from scone_gcn_amd import ops
    _zero_bounds(monkeypatch)
    args, facts = _facts(32, 3)
    cone = ops.stack_route(*args, **facts)
    full = cone.fallback()
    assert full == cone._replace(cone=False, units=False) and full.keep_last and full.top_dz_mask and full.first == "from_y"
    assert full.fallback() == full._replace(first="stored")
    with pytest.raises(AssertionError):
        full.fallback().fallback()
