"""GPU test of WHICH launches a plain scone stack makes (ops.stack_route): every case of
tests/scone_route_cases.py against tests/golden/scone_routes.json, the table tools/record_scone_routes.py wrote on the revision
before the route was decided in one place.

Every route of a stack computes the same bits, so a condition lost or added in ops.stack_route fails no other test: it moves a
configuration onto a slower path.  Compared per case: the timer keys in order of first launch, per key the launches and the launches that
state a byte model, and what the forward's record says (cone, unit lists, a rebuilt H1, y0, wide).  One step of a few milliseconds
each, on the four slabs of tests/test_gpu_readout_cone.py (one case on 65: the cone's slab limit)."""
import json
import os

import pytest

torch = pytest.importorskip("torch")

from tests.scone_route_cases import CASES, observe
from tests.test_gpu_keep_last import _need_gpu

pytestmark = pytest.mark.gpu
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scone_routes.json")) as f:
    GOLDEN = json.load(f)


def test_the_table_has_the_cases():
    assert sorted(GOLDEN) == sorted(c["name"] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_a_step_makes_the_recorded_launches(case):
    _need_gpu()
    seen, want = observe(case), GOLDEN[case["name"]]
    for field in sorted(want):
        print("%-10s %s" % (field, seen[field]))
        assert seen[field] == want[field], "%s: %s is %r, recorded %r" % (case["name"], field, seen[field], want[field])
    assert sorted(seen) == sorted(want)
