"""Host tests of the plan layer's pool of all-zero buffers (ops.ZeroPool) and of the rule by which a cone step leaves wipes to its epilogue
(ops.deferred_clears, SconePlan._cone_backward): plain Python over CPU tensors, no library call.

  * take of an unseen shape gives zeros of that shape; give then take returns the same object; two shapes do not mix; the pool reads
    as a mapping from shape to list, which is how the GPU tests count and inspect its buffers.
  * deferred_clears for 3 .. 6 layers: layers 2 and 1 wait, the top of a deeper stack is released inline, and no waiting layer lies
    above one that takes a pooled buffer (layer j >= 2 takes one for its dx).
  * The shared loop itself, on a plan whose launches are stand-ins: with a defer list it leaves exactly the wipes of deferred_clears,
    never takes from the pool while one of them waits, and allocates as many buffers as the loop that wipes inline."""
import pytest

torch = pytest.importorskip("torch")


def test_pool_takes_gives_and_reads_as_a_mapping():
    from scone_gcn_amd import ops
    pool = ops.ZeroPool("cpu")
    a = pool.take((2, 3, 4, 5))
    assert tuple(a.shape) == (2, 3, 4, 5) and a.dtype == torch.float32 and not a.any()
    like = torch.ones((2, 3, 4, 8))
    b = pool.take(like)
    assert b is not like and tuple(b.shape) == (2, 3, 4, 8) and not b.any()
    assert tuple(pool.take((3, 3), zeroed=False).shape) == (3, 3)
    pool.give(a)
    pool.give(b)
    assert isinstance(pool, dict) and {k: len(v) for k, v in pool.items()} == {(2, 3, 4, 5): 1, (2, 3, 4, 8): 1}
    assert {id(t) for v in pool.values() for t in v} == {id(a), id(b)}
    assert pool.take(torch.empty((2, 3, 4, 8))) is b, "a pooled buffer of the shape comes back, whatever is asked by"
    assert pool.take((2, 3, 4, 5)) is a and pool.take(a.shape) is not a, "... once"
    assert sum(len(v) for v in pool.values()) == 0


@pytest.mark.parametrize("L", [3, 4, 5, 6])
def test_deferred_clears(L):
    from scone_gcn_amd import ops
    waits = ops.deferred_clears(L)
    assert waits == {2, 1}
    assert (L - 1 in waits) == (L == 3), "the top layer's buffer is released inline on every stack deeper than three"
    takes = {j for j in range(1, L) if j >= 2}          # the loop's layers that take a pooled buffer for their dx
    for i in waits:
        assert not any(j < i for j in takes), "layer %d waits above a layer that takes from the pool" % i
    for i in set(range(1, L)) - waits:
        assert any(j < i for j in takes), "layer %d could wait as well" % i


class _Launches:
    """Stand-in for the plan's operators: the calls _cone_backward makes, recorded."""

    def __init__(self, plan, log):
        self.plan, self.log = plan, log

    def backward(self, dzs, Ws, aux, act, need_dx, dWs, dx=None, visit=None, defer=None):
        dx.fill_(1.0)
        self.log.append(("backward", visit, id(dzs[0])))
        if defer is not None:
            defer.append("reduce")
        return dx

    def backward_fused_first(self, dz, Ws, aux, act, y, dWs, dWs_first, Ws_first=None, visit=None, defer=None):
        self.log.append(("first", visit, id(dz)))
        if defer is not None:
            defer.extend(["reduce", "first"])
        return True

    def clear_mask(self, t, mask):
        t.zero_()
        self.log.append(("clear_mask", mask, id(t)))


def _walk(L, defer):
    from scone_gcn_amd import ops
    plan = object.__new__(ops.SconePlan)
    plan.act, plan.SMALL_DZ_BYTES, plan._dz_zero = "tanh", 1 << 30, ops.ZeroPool("cpu")     # (no readout wipe: the buffer just goes back)
    log = []
    plan.conv = plan.conv_T = _Launches(plan, log)
    taken = []
    take = plan._dz_zero.take

    def logged_take(like, zeroed=True):
        taken.append(take(like, zeroed))
        log.append(("take", None, id(taken[-1])))
        return taken[-1]
    plan._dz_zero.take = logged_take
    hs = [None, None] + [torch.zeros((1, 2, 1, 4)) for _ in range(L - 1)]
    cone = ["M%d" % k for k in range(L)]
    dz = plan._dz_zero.take(hs[-1])
    waiting = plan._cone_backward(hs, "y0", cone, dz, None, [None] * (3 * L + 1), [None] * (3 * L + 1), defer=defer)
    return plan, log, taken, waiting


@pytest.mark.parametrize("L", [3, 4, 5, 6])
def test_the_shared_loop_defers_by_the_rule_and_keeps_the_pools_peak(L):
    from scone_gcn_amd import ops
    inline, log0, taken0, none = _walk(L, None)
    assert none == [] and sum(len(v) for v in inline._dz_zero.values()) == len({id(t) for t in taken0})
    jobs = []
    plan, log, taken, waiting = _walk(L, jobs)
    assert jobs == ["reduce"] * (L - 1) + ["first"]
    # layer i's buffer was written on the mask the layer above visited; the readout gradient has none
    assert [m for _, m in waiting] == [None if i == L - 1 else "M%d" % (L - 1 - i) for i in sorted(ops.deferred_clears(L), reverse=True)]
    calls = lambda entries, *kinds: [c[:2] for c in entries if c[0] in kinds]
    assert calls(log, "backward", "first") == calls(log0, "backward", "first"), "the same backwards on the same masks"
    assert len(calls(log0, "clear_mask")) == L - 2, "inline, every layer below the top wipes its dz by the mask"
    assert calls(log, "clear_mask") + [("clear_mask", m) for _, m in waiting if m is not None] == calls(log0, "clear_mask"), "each once"
    for t, _ in waiting:                                # from the backward that consumed it on, a waiting buffer is not handed out again
        used = [k for k, c in enumerate(log) if c[0] in ("backward", "first") and c[2] == id(t)][-1]
        assert ("take", None, id(t)) not in log[used:], "a buffer that waits for its wipe was taken again"
    assert len({id(t) for t in taken}) == len({id(t) for t in taken0}), "the pool's peak is that of the loop that wipes inline"
    for t, _ in waiting:
        plan._dz_zero.give(t)
    assert sum(len(v) for v in plan._dz_zero.values()) == sum(len(v) for v in inline._dz_zero.values())
