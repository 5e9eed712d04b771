"""GPU tests of the visit sequence of the last layer's kept forward (fwd_c32_w16_kernel<KEEP>, plain and from-y form).

The kernel runs a block's slab loop over the SET bits of its keep window only: an item whose bit is clear is not staged, gathered or
contracted, and a block without a kept slab is left before its metadata is read.  tests/test_gpu_keep_last.py pins the contract (kept
rows = the full forward's bits, every other row untouched) on zero / ones / alternating / last-of-last / random masks; this file walks
the staging pipeline through its short cases -- one, two and three visits per block (the late waves' prologue DMA of visit 1 and both
`vdma` guards), visits whose slabs are far apart, kept blocks between runs of skipped blocks (the deferred store of a kept tile
across skipped units and after the loop), bits only above slab 64 -- at 5, 64 and 130 slabs: whatever slab split the launch grid
picks, 64 and 130 give slab ranges that start inside a mask word.  Every comparison is BIT FOR BIT on a sentinel-filled output.
The complex, the plan and the helpers are those of tests/test_gpu_keep_last.py.

What "not staged" means: input item (b', s) is staged by the kept items (b, s) with b' in A(b), the plan's block adjacency; the
poison test writes NaN over every other input item and expects the same bits.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_keep_last import _env, _expected, _need_gpu, _pack, _same_bits, _sentinel, _weights
from tests.test_gpu_top_dz_mask import _adj, _rows

pytestmark = pytest.mark.gpu

SLABS = [5, 64, 130]
MASKS = ["one_first", "one_last", "one_middle", "one_two_three", "three_then_one", "islands", "above_64"]


def _bits(name, nb, S):
    """bool [nb][S]: the kept (block, slab) items of a mask."""
    k = np.zeros((nb, S), bool)
    rs = np.random.RandomState(S + 7 * MASKS.index(name))
    if name == "one_first":                       # exactly one kept item in the whole launch: the first slab of block 0,
        k[0, 0] = True
    elif name == "one_last":                      # the last slab of the last (short) block: stored after the loop,
        k[nb - 1, S - 1] = True
    elif name == "one_middle":                    # a middle one
        k[nb // 2, S // 2] = True
    elif name == "one_two_three":                 # 1, 2, 3 set bits per block (b mod 3), clear runs of 1 and 2 slabs between them, at
        for b in range(nb):                       # positions that move with b: whatever the slab split, workgroups see 1, 2 and 3 visits
            p = (7 * b) % S
            for j, off in enumerate((0, 2, 5)):
                if j <= b % 3:
                    k[b, min(S - 1, p + off)] = True
    elif name == "three_then_one":                # a run of three set bits, a long clear run, one set bit
        for b in range(nb):
            p = (5 * b) % max(1, S - 13)
            k[b, p:p + 3] = True
            k[b, min(S - 1, p + 12)] = True
    elif name == "islands":                       # kept blocks between runs of empty blocks, the first and the last block empty
        for b in (3, 4, 9, nb // 2, nb - 3, nb - 2):
            k[b] = rs.rand(S) < 0.4
            k[b, rs.randint(S)] = True
    elif name == "above_64":                      # bits only in slabs >= 64 (130 slabs)
        assert S > 64
        k[:, 64:] = rs.rand(nb, S - 64) < 0.3
    return k


def _input(env, S, C, seed):
    """[S, E, 4, C] made on the device: trajectory-like support (a third of the 64-row groups of a slab carry values, the rest exact
    zeros), slab 1 dense."""
    E = env["cx"].n_edges
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.randn(S, E, 4, C, device="cuda", generator=g)
    live = (torch.rand(S, (E + 63) // 64, device="cuda", generator=g) < 0.33).repeat_interleave(64, dim=1)[:, :E]
    live[1] = True
    return x * live[:, :, None, None]


_CASE = {}


def _case(form, act, S):
    """Inputs, weights and the full forward's output of (form, act, S): computed once, one case held at a time (130 slabs are 0.35 GB
    per tensor)."""
    key = (form, act, S)
    if key not in _CASE:
        env = _env()
        _CASE.clear()
        rs = np.random.RandomState(S + 1000 * (form == "from_y") + (act == "relu"))
        W = _weights(32, rs)
        if form == "from_y":
            Wf = _weights(32, rs, c_in=1)
            src = env["plan"].conv.shifted_input(_input(env, S, 1, S + 1))
            assert src is not None
        else:
            Wf = None
            src = _input(env, S, 32, S)
        c = dict(src=src, W=W, Wf=Wf, form=form, act=act)
        c["full"] = _run(c, None, None)
        _CASE[key] = c
    return _CASE[key]


def _run(c, keep, out, src=None, W=None):
    env = _env()
    src, W = c["src"] if src is None else src, c["W"] if W is None else W
    if c["form"] == "from_y":
        got = env["plan"].conv.forward_from_y(src, c["Wf"], W, c["act"], keep=keep, out=out)
    else:
        got = env["plan"].conv.forward([src], W, 32, c["act"], out=out, keep=keep)
    assert got is not None, "forward not served"
    torch.cuda.synchronize()
    return got


def _kept(c, k, **kw):
    return _run(c, _pack(k), _sentinel(c["full"].shape), **kw)


@pytest.mark.parametrize("S,mask", [(S, m) for S in SLABS for m in MASKS if m != "above_64" or S > 64])   # (innermost: a case's tensors are shared)
@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("form", ["plain", "from_y"])
def test_kept_forward_visits_the_set_items_only(form, act, S, mask):
    _need_gpu()
    env = _env()
    k = _bits(mask, len(env["row0"]) - 1, S)
    assert k.any() and not k.all()
    c = _case(form, act, S)
    _same_bits(_kept(c, k).view(torch.int32), _expected(c["full"], k, env["row0"]), "%s, %s, %d slabs, mask %s" % (form, act, S, mask))


@pytest.mark.parametrize("form", ["plain", "from_y"])
def test_one_inf_weight(form):
    """A NaN / Inf weight turns the zero-tile early-out off (w_bad): the kept rows equal the full forward's bits under the same
    weights, NaNs included."""
    _need_gpu()
    env = _env()
    c = _case(form, "tanh", 64)
    W = [w.clone() for w in c["W"]]
    W[1][3, 7] = float("inf")
    full = _run(c, None, None, W=W)
    assert bool(torch.isnan(full).any())
    for mask in ("one_two_three", "islands"):
        k = _bits(mask, len(env["row0"]) - 1, 64)
        _same_bits(_kept(c, k, W=W).view(torch.int32), _expected(full, k, env["row0"]), "%s, one Inf weight, mask %s" % (form, mask))


@pytest.mark.parametrize("mask", ["one_middle", "one_two_three", "islands"])
@pytest.mark.parametrize("form", ["plain", "from_y"])
def test_input_no_kept_item_stages_is_never_read(form, mask):
    """NaN over every input item that no kept item stages: the result does not move by a bit (a staged NaN would count as non-zero
    in the early-out and reach every output of its tile)."""
    _need_gpu()
    env = _env()
    S = 64
    c = _case(form, "tanh", S)
    k = _bits(mask, len(env["row0"]) - 1, S)
    adj_ptr, adj_blk = _adj(env)
    staged = np.zeros_like(k)
    for b in range(k.shape[0]):
        staged[adj_blk[adj_ptr[b]:adj_ptr[b + 1]]] |= k[b]
    assert not (k & ~staged).any() and not staged.all(), "a block stages itself; something is left to poison"
    nan = torch.full((), float("nan"), device="cuda")
    src = torch.where(_rows(~staged, env["row0"])[:, :, None, None], nan, c["src"])
    assert bool(torch.isnan(src).any())
    _same_bits(_kept(c, k, src=src).view(torch.int32), _expected(c["full"], k, env["row0"]), "%s, poisoned input, mask %s" % (form, mask))
