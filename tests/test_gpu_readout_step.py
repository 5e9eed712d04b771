"""scn_readout_step (csrc/scn_readout.hip): the readout's forward, the cross-entropy's scaling and the readout's backward in ONE launch,
against scn_readout_forward + scn_masked_ce_begin + scn_readout_backward on the same inputs, BIT FOR BIT: bh, logits, logp, d_logp,
d_logits and every row of dz (both dz buffers start all-zero: rows outside the written set must still be +0).

Shapes: the readout tables of the cfg1 golden complex (tests/test_gpu_readout_cone.py's plan) with 4, 8 and 20 trajectories -- one slab
of four, two, and five with the suite's padding trajectories (last node 0, y = 0) -- at 32 and 16 channels, tanh and relu; the hand-built
complexes of tests/test_host_readout.py whose item lists pass RO_ITEMS = 512 (`mixed`: fast and serial trajectories in one launch;
`items`: 512 and 513), so the in-kernel serial form runs; a neighbourhood of 64 slots (served) and of 65 (declined, nothing written).
zero_buf comes in as NaN and goes out as zeros, and only zero_n of it; NULL is accepted."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_readout import SENTINEL, _filled, _p, _stream, _t, _tables
from tests.test_gpu_readout_cone import _env
from tests.test_host_readout import items_of, random_H

pytestmark = pytest.mark.gpu
SCN_ERR_UNSUPPORTED = -4
TANH, RELU = 1, 2


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from scone_gcn_amd import _lib
    return _lib.load()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _both(lib, tab, S, ns, E, V, D, H, w, y, scale, act, zero=None, zero_n=0):
    """(outputs of the one launch, outputs of the three) as dicts of tensors; tab: device nbr, last, inc_ptr, inc_edge, inc_sign, edge_nodes."""
    N, c = S * ns, H.shape[-1]
    new = lambda *shape: _filled(shape, "sentinel", None)
    head = (S, ns, E, c, _p(H), _p(w), _p(tab["nbr"]), V, D, _p(tab["last"]), _p(tab["inc_ptr"]), _p(tab["inc_edge"]), _p(tab["inc_sign"]))
    a = dict(bh=new(N, D, c), logits=new(N, D), logp=new(N, D), d_logp=new(N, D), d_logits=new(N, D), dz=torch.zeros_like(H))
    st = lib.scn_readout_step(*head, _p(tab["edge_nodes"]), _p(y), float(scale), act, _p(a["bh"]), _p(a["logits"]), _p(a["logp"]),
                              _p(a["d_logp"]), _p(a["d_logits"]), _p(a["dz"]), 1, _p(zero) if zero is not None else None, zero_n, _stream())
    torch.cuda.synchronize()
    if st != 0:
        return st, a, None
    b = dict(bh=new(N, D, c), logits=new(N, D), logp=new(N, D), d_logp=new(N, D), d_logits=new(N, D), dz=torch.zeros_like(H))
    assert lib.scn_readout_forward(*head, _p(b["bh"]), _p(b["logits"]), _p(b["logp"]), _stream()) == 0
    loss = torch.zeros(1, device="cuda", dtype=torch.float64)
    assert lib.scn_masked_ce_begin(N * D, _p(b["logp"]), _p(y), float(scale), _p(b["d_logp"]), _p(loss), 1, None, 0, _stream()) == 0
    d_w = torch.zeros(c, device="cuda")
    assert lib.scn_readout_backward(*head, _p(tab["edge_nodes"]), _p(b["bh"]), _p(b["d_logp"]), _p(b["logp"]), act, _p(b["d_logits"]),
                                    _p(b["dz"]), 1, _p(d_w), _stream()) == 0
    torch.cuda.synchronize()
    return st, a, b


def _assert_same(a, b, what):
    for k in ("bh", "logits", "logp", "d_logp", "d_logits", "dz"):
        x, y = _bits(a[k]), _bits(b[k])
        assert np.array_equal(x, y), "%s: %s differs in %d of %d words" % (what, k, int((x != y).sum()), x.size)
    assert float(a["dz"].abs().max()) > 0, what + ": the backward wrote nothing"


def _targets(rs, N, n_real, D):
    y = np.zeros((N, D), np.float32)
    y[np.arange(n_real), rs.randint(0, D, n_real)] = rs.uniform(0.5, 1.5, n_real).astype(np.float32)
    return y


@pytest.mark.parametrize("act", [TANH, RELU])
@pytest.mark.parametrize("n_traj", [4, 8, 20])
@pytest.mark.parametrize("c", [32, 16])
def test_one_launch_equals_the_three_on_the_golden_complex(lib, c, n_traj, act):
    env = _env()
    plan = env["plan"]()
    rs = np.random.RandomState(1000 * c + 10 * n_traj + act)
    ns, E, V, D = 4, env["E"], plan.n_nodes, plan.max_deg
    S = {4: 1, 8: 2, 20: 5}[n_traj]
    n_real = n_traj if n_traj != 20 else 18                            # five slabs, the last one with two padding trajectories
    last = np.zeros(S * ns, np.int32)
    last[:n_real] = rs.randint(0, V, n_real)
    last[0] = int(np.argmax((plan._h_nbr >= 0).sum(axis=1)))            # a node of maximal degree
    tab = dict(nbr=plan.nbr, last=_t(last), inc_ptr=plan.inc_ptr, inc_edge=plan.inc_edge, inc_sign=plan.inc_sign, edge_nodes=plan.edge_nodes)
    H, w = _t(random_H(rs, S, E, ns, c)), _t((rs.randn(c) / np.sqrt(c)).astype(np.float32))
    y = _t(_targets(rs, S * ns, n_real, D))
    zero = _filled((6500 + 16,), "sentinel", rs)
    st, a, b = _both(lib, tab, S, ns, E, V, D, H, w, y, -1.0 / 123.0, act, zero=zero, zero_n=6500)
    assert st == 0
    _assert_same(a, b, "c=%d, %d trajectories, act %d" % (c, n_traj, act))
    z = zero.cpu().numpy()
    assert not z[:6500].view(np.uint32).any() and np.all(z[6500:].view(np.uint32) == SENTINEL), "zero_buf: not exactly zero_n floats of +0"
    # rows outside the written set are still +0: the stand-alone clear returns the buffer to all-zero bits
    assert lib.scn_readout_clear_dz(S, ns, E, c, _p(tab["nbr"]), V, D, _p(tab["last"]), _p(tab["inc_ptr"]), _p(tab["inc_edge"]),
                                    _p(tab["edge_nodes"]), _p(a["dz"]), _stream()) == 0
    torch.cuda.synchronize()
    assert not _bits(a["dz"]).any()


@pytest.mark.parametrize("act", [TANH, RELU])
@pytest.mark.parametrize("name", ["mixed", "items"])
def test_item_lists_past_the_table_take_the_serial_form(lib, name, act):
    cx, dv = _tables(name)
    it = items_of(cx)[:cx["n_real"]]
    assert (it > 512).any() and (it <= 512).any(), "fast and serial trajectories in one launch"
    rs = np.random.RandomState(77 + act)
    S, ns, E, D, c = cx["S"], cx["ns"], len(cx["edges"]), cx["D"], 32
    H, w = _t(random_H(rs, S, E, ns, c)), _t((rs.randn(c) / np.sqrt(c)).astype(np.float32))
    y = _t(_targets(rs, S * ns, cx["n_real"], D))
    st, a, b = _both(lib, dv, S, ns, E, cx["n_nodes"], D, H, w, y, -0.01, act)               # (zero_buf = NULL)
    assert st == 0
    _assert_same(a, b, "%s, act %d" % (name, act))


def test_64_slots_are_served_and_65_declined_with_nothing_written(lib):
    rs = np.random.RandomState(3)
    for name, served in (("deg64", True), ("deg65", False)):
        cx, dv = _tables(name)
        S, ns, E, D, c = cx["S"], cx["ns"], len(cx["edges"]), cx["D"], 32
        assert D == (64 if served else 65)
        H, w = _t(random_H(rs, S, E, ns, c)), _t((rs.randn(c) / np.sqrt(c)).astype(np.float32))
        y = _t(_targets(rs, S * ns, cx["n_real"], D))
        zero = _filled((40,), "sentinel", rs)
        st, a, b = _both(lib, dv, S, ns, E, cx["n_nodes"], D, H, w, y, -0.5, TANH, zero=zero, zero_n=40)
        if served:
            assert st == 0
            _assert_same(a, b, name)
            continue
        assert st == SCN_ERR_UNSUPPORTED
        for k in ("bh", "logits", "logp", "d_logp", "d_logits"):
            assert np.all(_bits(a[k]) == SENTINEL), name + ": " + k + " was written"
        assert not _bits(a["dz"]).any() and np.all(_bits(zero) == SENTINEL)
    # the other forms the entry leaves to the separate launches: a buffer that is not kept all-zero, rows wider than a wave
    cx, dv = _tables("deg64")
    S, ns, E, D = cx["S"], cx["ns"], len(cx["edges"]), cx["D"]
    buf = torch.zeros(S * E * ns * 96, device="cuda")
    P = _p(buf)
    head = lambda c: (S, ns, E, c, P, P, _p(dv["nbr"]), cx["n_nodes"], D, _p(dv["last"]), _p(dv["inc_ptr"]), _p(dv["inc_edge"]), _p(dv["inc_sign"]),
                      _p(dv["edge_nodes"]), P, -1.0, TANH, P, P, P, P, P, P)
    for c, mode in ((32, 0), (32, 2), (96, 1)):
        assert lib.scn_readout_step(*head(c), mode, None, 0, _stream()) == SCN_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert not _bits(buf).any()
