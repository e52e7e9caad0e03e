"""Exact segmented-accumulate kernels: every row of tests/_segment_cases.py (every launcher branch of
coclr_segment_softmax_accum / coclr_segment_accum in coclr_amd/csrc/retrieval.hip, see tests/test_segment_cases_cpu.py)
through coclr_amd.ops against the float64 references of tests/_segment_cases.py.

  * sum rows (segment_accum) and softmax rows (segment_softmax_accum): the whole (V, C) table bit for bit, the output rows
    no segment names included -- they keep the prior.  A maximum reduction that misses a wave or a pass of the column loop
    turns a softmax row into inf / NaN: the row's maximum sits in one wave of one pass, 200 above everything else.
  * random rows, both kernels: 1e-6 of the largest reference element (tests/test_segment_cases_cpu.py shows that a plain
    fp32 restatement needs half of that).
  * one call of S segments == S calls of one segment == itself again, bit for bit, however the launcher cuts the call.
  * segment_accum in the 16-byte and in the scalar form: the same bits (one thread sums a column in row order in both).

x lies between memory holding 2^20, out between guards that are compared after the launch; rows of x that belong to no
segment hold NaN.  Every launch is followed by _exact.sync(): a fault ends the session."""
import pytest
import torch

import _segment_cases as S
from _exact import NAN, Placed2D, close, exact, source2d, sync

pytestmark = pytest.mark.gpu


def ops():
    from coclr_amd import ops as o
    return o


def ids(table):
    return [c.name for c in table]


def fn_of(softmax):
    return ops().segment_softmax_accum if softmax else ops().segment_accum


def place(c):
    """(x on the device, out as a Placed2D holding the prior)."""
    x, prior = S.inputs(c)
    xd = source2d(x, shift=c.x_shift)
    unread = S.unread_rows(c)
    if unread:
        xd[torch.tensor(unread, device="cuda")] = NAN
    out = Placed2D(c.V, c.C, shift=c.out_shift)
    out.put(prior)
    assert xd.is_contiguous() and out.view.is_contiguous()
    assert xd.data_ptr() % 16 == 4 * (c.x_shift % 4) and out.view.data_ptr() % 16 == 4 * (c.out_shift % 4)
    return xd, out


def run(c, softmax, calls=None):
    """The table after the row's call -- or after `calls`, lists of segment indices, one ops call each."""
    xd, out = place(c)
    for part in calls if calls is not None else [range(len(c.segs))]:
        fn_of(softmax)(xd, [c.segs[s] for s in part], [c.weights[s] for s in part], out.view)
        sync("%s %s" % ("segment_softmax_accum" if softmax else "segment_accum", c.name))
    got = out.view.clone()
    assert out.untouched_around(), "%s: memory around out was written" % c.name
    return got


SUM, SOFTMAX = S.of(cls="sum"), S.of(cls="softmax")
RANDOM = S.of(cls="rand3") + S.of(cls="rand30")


@pytest.mark.parametrize("c", SUM, ids=ids(SUM))
def test_segment_accum_exact(c):
    exact(run(c, False), S.reference(c, False), "segment_accum " + c.name)


@pytest.mark.parametrize("c", SOFTMAX, ids=ids(SOFTMAX))
def test_segment_softmax_accum_exact(c):
    exact(run(c, True), S.reference(c, True), "segment_softmax_accum " + c.name)


@pytest.mark.parametrize("c", RANDOM, ids=ids(RANDOM))
def test_random_rows_within_the_bar(c):
    for softmax in (True, False):
        got = run(c, softmax)
        close(got, S.reference(c, softmax), 1e-6, "%s %s" % ("softmax sum" if softmax else "plain sum", c.name))
        _, prior = S.inputs(c)
        for o in S.unnamed_outputs(c):
            exact(got[o], prior[o], "%s: output row %d, which no segment names" % (c.name, o))


PARTITION = S.of("partition")


@pytest.mark.parametrize("c", PARTITION, ids=ids(PARTITION))
def test_the_launch_partition_does_not_show(c):
    for softmax in (True, False):               # (bit for bit whatever the data: the exact classes' rows as well)
        whole = run(c, softmax)
        assert torch.equal(whole, run(c, softmax)), "%s: two runs differ" % c.name
        single = run(c, softmax, [[s] for s in range(len(c.segs))])
        assert torch.equal(whole, single), "%s: one call of %d segments differs from %d calls of one" % (
            c.name, len(c.segs), len(c.segs))


@pytest.mark.parametrize("C_", S.BASE_WIDTHS)
@pytest.mark.parametrize("cls", ["sum", "rand3", "rand30"])
def test_segment_accum_is_the_same_in_both_forms(C_, cls):
    aligned, shifted = S.twins(C_, cls)
    assert S.branches(aligned)["vec"] and len(shifted) == 3
    want = run(aligned, False)
    for c in shifted:
        assert not S.branches(c)["vec"]
        assert torch.equal(S.inputs(c)[0], S.inputs(aligned)[0]) and torch.equal(S.inputs(c)[1], S.inputs(aligned)[1])
        assert torch.equal(run(c, False), want), "%s differs from %s" % (c.name, aligned.name)
