"""GPU tests of the one-launch step (scn_small_step, csrc/scn_small.hip) on hand-built operators AT THE LIMITS OF ITS LAYOUT.

Every other test of that kernel runs triangulated complexes with the Hodge shifts: symmetric, about 11 entries per row, a few dozen
readout items.  The cases here (tests/small_step_cases.py builds them, tests/test_host_small_step_limits.py proves on the CPU what each
of them is, that float32 resolves it four times better than the bars and that the fp64 reference moves by ten bars when ONE special
entry is dropped) meet what those never do: non-symmetric shifts (the second load of the operator rows, the overflow list reloaded
from the transpose, the first layer's shifted input read back from memory), row tails past the twelfth entry read from the list in
LDS and from memory, in twelve- and eight-wave kernels, rows of exactly 0 / 1 / 11 / 12 / 13 / 24 / 25 / 60 / 100 entries at the tile and
block edges, real entries in column 0, an overflow list that takes the room of the first layer's shifted input, every boundary
between two kernel instances (|E| = 192 / 193, 384 / 385, 768 / 769, 1024 / 1025, 1056 / 1057, 1120 / 1121), max_deg = 64 and
max_items = 512 exactly, 2 / 5 / 6 layers and all four activation codes.

Each case reads the form of its launch from scn_small_step_layout -- the host function the launch itself selects its instance with --
and compares it with the restated selection and the case table; then plan.small_step, in the paired form and with
scn_small_step_pairing(1) where pairing applies, against (a) oracle.scone_loss_and_grad in fp64 and (b) the layer-by-layer kernels on
the same plan.  Bars (tests/test_gpu_small_step.py): loss 1e-5 max(1, |ref|), every weight-gradient tensor 1e-5 of max(1, max |ref|)
against fp64; 2e-6 max(1, gmax) between the two GPU paths.  Every reference gradient tensor has an entry >= 0.1 (host test).

Regime reached per case (the library's answer, equal to the restatement) and the worst weight-gradient error measured on an MI355X,
against fp64 (bar 1e-5) and against the layer kernels (bar 2e-6), over the forms run; the loss errors were <= 2.2e-7 throughout:
  e17_sym            L2 tanh       12 waves, instance 1, list    2 /    2 in memory, y in LDS                 7.4e-08  8.9e-08
  e192_sym           L5 relu       12 waves, instance 1, list  163 /  163 in memory, y in LDS                 1.5e-07  2.4e-07
  e192_nonsym        L2 none       12 waves, instance 1, list  163 /  138 in memory, y in LDS                 6.5e-08  1.2e-07
  e193_sym           L3 leaky_relu 12 waves, instance 2, list  163 /  163 in memory, y in LDS                 1.3e-07  1.5e-07
  e193_nonsym        L6 tanh       12 waves, instance 2, list  163 /  131 in memory, y in LDS                 5.1e-07  8.6e-07
  e384_hub24         L6 none       12 waves, instance 2, list  163 /  163 in memory, y in LDS                 7.8e-07  2.0e-07
  e385_sym           L4 tanh        8 waves, instance 6 / paired 2, list  163 /  163 in LDS, y in LDS         1.9e-07  2.5e-07
  e385_nonsym        L5 leaky_relu  8 waves, instance 6 / paired 2, list  163 /  127 in LDS, y in LDS         3.4e-07  3.0e-07
  e520_sym           L6 relu        8 waves, instance 6 / paired 3, list  324 /  324 in LDS, y in LDS         1.5e-06  2.9e-07
  e520_nonsym        L6 tanh        8 waves, instance 6 / paired 3, list  324 /  274 in LDS, y in LDS         6.1e-07  6.2e-07
  e520_tonly         L6 leaky_relu  8 waves, instance 6 / paired 3, list    0 /  324 in LDS, y in LDS         2.7e-07  1.9e-07
  e768_sym           L3 relu        8 waves, instance 6 / paired 3, list  224 /  224 in LDS, y in LDS         1.7e-07  4.7e-07
  e769_sym           L5 none        8 waves, instance 8 / paired 4, list  324 /  324 in LDS, y in LDS         6.9e-07  3.2e-07
  e1001_nonsym_fits  L3 tanh        8 waves, instance 8 / paired 4, list  486 /  403 in LDS, y in LDS         1.5e-07  2.1e-07
  e1001_nonsym_long  L5 relu        8 waves, instance 8 / paired 4, list 1494 / 1188 in memory, y in LDS      2.7e-07  4.3e-07
  e1024_sym          L2 leaky_relu  8 waves, instance 8 / paired 4, list  324 /  324 in LDS, y in LDS         2.0e-07  4.0e-07
  e1024_nonsym       L2 relu        8 waves, instance 8 / paired 4, list  324 /  240 in LDS, y in LDS         1.7e-07  3.7e-07
  e1025_sym          L3 tanh        8 waves, instance 9 / paired 5, list  325 /  325 (*), y recomputed        1.7e-07  3.5e-07
  e1025_nonsym       L5 none        8 waves, instance 9 / paired 5, list  325 /  260 (*), y from memory       1.4e-06  1.4e-06
  e1040_sym          L4 relu        8 waves, instance 9 / paired 5, list  338 /  338 (*), y recomputed        2.6e-07  3.0e-07
  e1040_nonsym       L6 none        8 waves, instance 9 / paired 5, list  338 /  279 (*), y from memory       3.3e-07  1.7e-07
  e1056_sym          L3 leaky_relu  8 waves, instance 9 / paired 5, list  866 /  866 in memory, y in LDS      1.8e-07  3.0e-07
  e1056_nonsym       L4 tanh        8 waves, instance 9 / paired 5, list 1130 /  943 in memory, y in LDS      4.2e-07  2.1e-07
  e1057_sym          L5 tanh        8 waves, instance 9 / paired 5, list  338 /  338 (*), y recomputed        9.8e-07  4.5e-07
  e1057_nonsym       L3 relu        8 waves, instance 9 / paired 5, list  338 /  272 (*), y from memory       2.2e-07  4.1e-07
  e1120_nonsym       L4 leaky_relu  8 waves, instance 9 / paired 5, list  338 /  237 in memory, y from memory 2.7e-07  3.0e-07
  e1121_sym          refused: beyond the LDS; the layer kernels against fp64                                  2.4e-07
  (*) the list has room in the LDS: the paired form reads it there, the nine-tile instance of one workgroup reads the tails from memory
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import small_step_cases as sc

pytestmark = pytest.mark.gpu

TOL, TOL_PATHS = 1e-5, 2e-6
_ENV = {}


@pytest.fixture(autouse=True)
def _every_size():
    from scone_gcn_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    old = ops.SMALL_STEP_MAX_EDGES
    ops.SMALL_STEP_MAX_EDGES = 1 << 30
    yield
    ops.SMALL_STEP_MAX_EDGES = old


def _maxdiff(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(b))))


class Env:
    """A case on the device: the plan, the staged trajectories (sel: a subset, alone) and weight / gradient buffers."""

    def __init__(self, c, sel=None):
        from scone_gcn_amd import ops
        from scone_gcn_amd.complex import Shift
        self.c = c
        dev = self.dev = ops.default_device()
        key = ("plan", c.name)
        if key not in _ENV:
            shifts = [Shift(c.S_lo, c.sc.layout, 1, 1), Shift(c.S_up, c.sc.layout, 1, 1)]
            readout = c.sc.bconds()
            _ENV[key] = (ops.get_scone_plan(shifts[0], shifts[1], readout, c.act, dev), shifts, readout)
        self.plan = _ENV[key][0]
        assert type(self.plan) is ops.SconePlan and self.plan.act == c.act
        assert (self.plan.max_deg, self.plan.max_items) == (c.max_deg, c.max_items)
        assert (self.plan.conv_T is self.plan.conv) == c.same_t
        sel = np.arange(c.n_traj) if sel is None else np.asarray(sel)
        self.n = len(sel)
        self.x, n = ops.flows_to_slabs(c.flows[sel], c.sc.layout, dev)
        self.n_pad = self.x.shape[0] * ops.NS
        self.last = ops._last_nodes_dev(ops.remap_last_nodes(self.plan, c.last_nodes[sel]), self.n_pad, dev)
        self.yt = torch.zeros((self.n_pad, c.max_deg), device=dev, dtype=torch.float32)
        self.yt[:self.n] = torch.as_tensor(c.y[sel, :, 0], dtype=torch.float32).to(dev)
        sizes = [w.size for w in c.weights]
        self.flat_w = torch.tensor(np.concatenate([w.ravel() for w in c.weights]), dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros_like(self.flat_w)
        off = np.concatenate([[0], np.cumsum(sizes)])
        self.weights = [self.flat_w[off[k]:off[k + 1]].view(*w.shape) for k, w in enumerate(c.weights)]
        self.grads = [self.flat_g[off[k]:off[k + 1]].view(*w.shape) for k, w in enumerate(c.weights)]
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)

    def layout(self):
        """scn_small_step_layout of the launch small_step() makes, as a dict"""
        from scone_gcn_amd import _lib
        out = np.full(len(sc.LAYOUT_FIELDS), -1, np.int32)
        st = _lib.load().scn_small_step_layout(self.plan.conv.handle, self.plan.conv_T.handle, self.n_pad, out.ctypes.data, len(out))
        assert st == 0
        return dict(zip(sc.LAYOUT_FIELDS, (int(v) for v in out)))

    def result(self):
        torch.cuda.synchronize()
        return float(self.loss[0]), [g.detach().cpu().numpy().astype(np.float64) for g in self.grads]

    def small(self, scale=None, overwrite=True):
        scale = -1.0 / self.n if scale is None else scale
        served = self.plan.small_step(self.x, self.last, self.yt, scale, self.weights, self.grads, self.loss, overwrite=overwrite)
        return served and self.result()

    def layers(self):
        """the layer-by-layer kernels on the same plan and buffers (what the trainer runs with ops.SMALL_STEP = False)"""
        from scone_gcn_amd import _lib, ops
        logp, saved = self.plan.forward(self.x, self.last, self.weights)
        d_logp = torch.empty_like(logp)
        _lib.check(_lib.load().scn_masked_ce_begin(logp.numel(), ops._dev(logp), ops._dev(self.yt), -1.0 / self.n, ops._dev(d_logp),
                                                   ctypes.c_void_p(self.loss.data_ptr()), 1, ops._dev(self.flat_g), self.flat_g.numel(),
                                                   ops._stream()), "scn_masked_ce_begin")
        self.plan.backward(saved, logp, d_logp, self.last, self.weights, self.grads)
        return self.result()


def _unpaired(fn):
    from scone_gcn_amd import _lib
    lib = _lib.load()
    try:
        assert lib.scn_small_step_pairing(1) == 0
        return fn()
    finally:
        lib.scn_small_step_pairing(0)


def _against(name, what, got, ref, bar, scale_all=False):
    (la, ga), (lb, gb) = got, ref
    gmax = max(float(np.abs(g).max()) for g in gb)
    e_loss = abs(la - lb) / max(1.0, abs(lb))
    if scale_all:
        e_g = max(float(np.abs(a - b).max()) for a, b in zip(ga, gb)) / max(1.0, gmax)
    else:
        e_g = max(_maxdiff(a, b) for a, b in zip(ga, gb))
    print("%s %s: loss %.3g, gradients %.3g (bar %.0e)" % (name, what, e_loss, e_g, bar))
    assert np.isfinite(la) and all(np.isfinite(a).all() for a in ga), (name, what)
    assert e_loss <= bar, (name, what, "loss", e_loss)
    assert e_g <= bar, (name, what, "gradients", e_g)


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_small_step_at_its_layout_limits(name):
    from scone_gcn_amd import ops
    c = sc.get_case(name)
    e = Env(c)
    ref = sc.reference(name)
    assert min(float(np.abs(g).max()) for g in ref[1]) >= 0.1
    lay = e.layout()
    want = sc.REGIMES[name]
    if not want.get("supported", 1):
        assert lay["supported"] == 0 and c.form()["supported"] == 0
        assert e.small() is False, "a complex beyond the LDS is refused"
        _against(name, "layer kernels against fp64", e.layers(), ref, TOL)
        return
    # the form of the launch: the library's own answer against the restated selection and the case table
    assert lay["paired"] == int(c.E > 384 and 2 * e.n_pad <= ops.device_cus(e.dev))
    restated = c.form(paired=lay["paired"])
    for k in sc.LAYOUT_FIELDS:
        assert lay[k] == restated[k], (name, k, lay[k], restated[k])
    if lay["paired"]:
        assert lay["instance"] == want["paired_instance"]
        one = _unpaired(e.layout)
        assert one["paired"] == 0 and one == {k: c.form()[k] for k in sc.LAYOUT_FIELDS}
    else:
        one = lay
    for k, v in want.items():
        if k in sc.LAYOUT_FIELDS:
            assert one[k] == v, (name, k, one[k], v)
    print(name, "layout", lay, "| unpaired instance", one["instance"], "ovf_in_kernel", one["ovf_in_kernel"])
    lb = e.layers()
    _against(name, "layer kernels against fp64", lb, ref, TOL)
    forms = [("paired" if lay["paired"] else "one workgroup", e.small)]
    if lay["paired"]:
        forms.append(("pairing off", lambda: _unpaired(e.small)))
    for what, run in forms:
        e.flat_g.fill_(7.0)
        e.loss.fill_(7.0)                                           # overwrite: what the buffers held does not matter
        got = run()
        assert got is not False, (name, what, "not served")
        _against(name, what + " against fp64", got, ref, TOL)
        _against(name, what + " against the layer kernels", got, lb, TOL_PATHS, scale_all=True)


def test_accumulating_call_adds_to_what_the_buffers_hold():
    """overwrite = 0 called directly: gradients prefilled with 0.25, the loss with 1.5, a scale other than -1 / N -- prefill plus the
    overwrite form's result, exactly (one float32 add per entry, one float64 add)."""
    c = sc.get_case("e520_nonsym")
    e = Env(c)
    for run in (lambda f: f(), _unpaired):
        l1, g1 = run(lambda: e.small(scale=0.37))
        e.flat_g.fill_(0.25)
        e.loss.fill_(1.5)
        l0, g0 = run(lambda: e.small(scale=0.37, overwrite=False))
        assert l0 == 1.5 + l1 and abs(l1) > 0.1
        for a, b in zip(g0, g1):
            assert np.array_equal(a.astype(np.float32), np.float32(0.25) + b.astype(np.float32)) and np.abs(b).max() > 0.01


@pytest.mark.parametrize("name", ["e520_nonsym", "e1057_nonsym"])
def test_two_launches_give_the_same_bits(name):
    e = Env(sc.get_case(name))
    for run in (lambda f: f(), _unpaired):
        a, b = run(e.small), run(e.small)
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("name", ["e520_nonsym", "e193_nonsym"])
def test_node_without_neighbours_and_zero_flow_alone(name):
    """The trajectory that ends on the node without edges and the one with an all-zero flow, each alone: log D (float32 logf: two
    ulp) and a gradient of exact zeros."""
    c = sc.get_case(name)
    for t in (c.T_ISOLATED, c.T_ZERO_FLOW):
        e = Env(c, sel=[t])
        for run in (lambda f: f(), _unpaired):
            e.flat_g.fill_(7.0)
            loss, g = run(e.small)
            assert abs(loss - np.log(c.max_deg)) <= 2.4e-7 * np.log(c.max_deg), (name, t, loss)
            assert all(not a.any() for a in g), (name, t)
