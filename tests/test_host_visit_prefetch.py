"""Host restatement of the unit pipeline of the visiting backwards (csrc/scn_blk_bwd.inc): the staging parity that runs over a
workgroup's whole visit sequence, and which unit's source rows a side slot stages from.  No diagnostic entry point exposes the
kernel's buffers, so the restatement is checked against its own invariants over seeded random windows:

  * no staging buffer is written while the visit in flight gathers from it;
  * every visit gathers from the buffer its own slab went to, staged from its own unit's rows;
  * a slab is staged from the row buffer that holds ITS unit's rows (the buffers swap at every hand-over);
  * nothing staged is left unread when the workgroup is done, and nothing is staged ahead across a table refill.

The walk is the kernel's: per table scan the non-empty windows in unit order; a unit's visits are the set bits of its window in
ascending order; the unit's LAST visit stages the first slab of the table's next entry."""
import numpy as np
import pytest


def _bits(w):
    return [j for j in range(64) if (w >> j) & 1]


def simulate(scans, prefetch=True):
    """scans: list of tables, each a list of (block, window != 0).  Returns the visits in order as (block, slab, buffer) and the
    number of units that found their first slab staged; asserts the invariants on the way."""
    buf = [None, None]                 # what a staging buffer holds: (block, slab)
    rows = [None, None]                # whose source rows a row buffer holds
    vpar, sr_cur, staged = 0, 0, False
    visits, n_staged = [], 0
    for table in scans:
        assert not staged, "a slab staged ahead across a table refill"
        for e, (b, w) in enumerate(table):
            slabs = _bits(w)
            assert slabs
            has_next = prefetch and e + 1 < len(table)
            sr_next = 1 - sr_cur
            # the unit's top: everything in flight has landed (wait + barrier), every wave has left the previous unit
            gathering = None
            if staged:
                assert rows[sr_cur] == b and buf[vpar] == (b, slabs[0]), "the previous unit staged something else"
                n_staged += 1
            else:
                rows[sr_cur] = b
            if has_next:
                rows[sr_next] = table[e + 1][0]
            if not staged:
                buf[vpar] = (b, slabs[0])

            def stage(to, src_rows, owner, slab):
                assert to != gathering, "a buffer is staged while it is being gathered"
                assert rows[src_rows] == owner, "staged from another unit's rows"
                buf[to] = (owner, slab)

            for it, s in enumerate(slabs):
                cur = (vpar + it) & 1
                assert buf[cur] == (b, s), "visit %d of block %d reads a buffer that holds %r" % (it, b, buf[cur])
                gathering = cur
                visits.append((b, s, cur))
                if it + 1 < len(slabs):
                    stage((vpar + it + 1) & 1, sr_cur, b, slabs[it + 1])
                elif has_next:
                    nb, nw = table[e + 1]
                    stage((vpar + it + 1) & 1, sr_next, nb, _bits(nw)[0])
                buf[cur] = None                                          # read once
            if prefetch:
                vpar = (vpar + len(slabs)) & 1
                sr_cur = sr_next if has_next else sr_cur
            staged = has_next
    assert not staged and buf == [None, None], "something staged was never read"
    return visits, n_staged


def _random_scans(rs, n_scans, max_units, density):
    scans = []
    for _ in range(n_scans):
        table = []
        for _ in range(rs.randint(0, max_units + 1)):
            w = 0
            while w == 0:
                w = int(sum(1 << j for j in range(64) if rs.rand() < density))
            table.append((int(rs.randint(0, 100000)), w))
        scans.append(table)
    return scans


@pytest.mark.parametrize("density", [0.02, 0.2, 0.9])
def test_pipeline_invariants_on_seeded_random_windows(density):
    rs = np.random.RandomState(int(density * 100))
    for _ in range(200):
        scans = _random_scans(rs, rs.randint(1, 4), 12, density)
        got, n_staged = simulate(scans)
        plain, none = simulate(scans, prefetch=False)
        assert none == 0
        # the same visits in the same order as the loop without the pipeline: ascending unit and slab order
        assert [(b, s) for b, s, _ in got] == [(b, s) for b, s, _ in plain] == [(b, s) for t in scans for b, w in t for s in _bits(w)]
        # every unit with a predecessor in its table found its slab staged
        assert n_staged == sum(max(len(t) - 1, 0) for t in scans)
        # the buffers alternate over the workgroup's WHOLE sequence; without the pipeline every unit starts in buffer 0
        assert [c for _, _, c in got] == [i & 1 for i in range(len(got))]
        assert [c for _, _, c in plain] == [i & 1 for t in scans for b, w in t for i in range(len(_bits(w)))]


@pytest.mark.parametrize("lens", [(1, 1), (1, 2), (2, 1), (2, 2), (1, 3), (3, 1), (2, 3), (3, 2), (3, 3)])
def test_both_parities_cross_a_unit_boundary(lens):
    """units of 1, 2 and 3 visits in every order of two, started from either buffer"""
    for lead in (1, 2):
        table = [(0, (1 << lead) - 1), (1, (1 << lens[0]) - 1), (2, (1 << lens[1]) - 1)]
        got, n_staged = simulate([table])
        assert n_staged == 2 and [c for _, _, c in got] == [i & 1 for i in range(lead + sum(lens))]


def test_one_unit_none_and_a_refill_between_two():
    assert simulate([[]]) == ([], 0)
    assert simulate([[(5, 1 << 63)]]) == ([(5, 63, 0)], 0)
    got, n_staged = simulate([[(1, 0b1)], [(2, 0b11)]])
    assert n_staged == 0 and got == [(1, 0, 0), (2, 0, 1), (2, 1, 0)]
