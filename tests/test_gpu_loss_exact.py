"""The loss + accuracy epilogue (coclr_amd/csrc/loss.hip) called directly, so that the row statistics, the drop flags and
the five scalars are all visible, on every row of tests/_head_cases.py: LOSS.

Logits live on a grid of 1/4 (ties are frequent, ranks exact); some rows are scaled to +-960, some are constant
(tests/_head_ref.py: loss_inputs, which also places the positives: column 0, the last column, a column >= 256, only the
last column, exactly one positive, several, mask[b][0] == 0).

  * exact: the four hit flags and the drop flag of every row against the rank rule of loss.hip's header (a hit iff fewer
    than k logits are strictly greater than the best positive / than column 0), the four accuracy scalars (means of 0 / 1
    over B, one rounding), the row maximum, and mode 2's positive count.
  * 1e-6 of max|ref| for loss, lse and the loss scalar, 1e-5 for dlogits (with dloss = 0.75), against float64 and its
    autograd -- the bounds of tests/test_gpu_next.py, through _cases.check_close -- separately for the ordinary rows and
    for the scaled ones, so that a large row's magnitude does not hide a small row's error.
  * the scaled rows' dlogits: softmax_j = exp(v_j - lse) carries the rounding of lse ~ 960 (half an ulp = 3e-5) as a
    RELATIVE error unless the backward also gets what that rounding dropped (rowstats' lse_lo / aux_lo, kept for
    rows with |max| >= 64 or a best positive 64 below the max; every other row keeps the plain forms).  The test
    prints the error of the fp32 ATen reference next to the kernel's and holds the kernel to 1e-5 or twice ATen's
    error, whichever is larger.  Before lse_lo / aux_lo existed the N1 = 77 rows measured 1.45e-5 (ATen: 3e-8).

A row without any positive has no finite mode-1 loss: +inf, as the reference's -log(0).
"""
import pytest
import torch
import torch.nn.functional as F

import _head_cases as H
import _head_ref as R
from _cases import check_close, rel_err
from _exact import Placed2D, exact, source2d, sync

pytestmark = pytest.mark.gpu

DLOSS = 0.75


def run_loss(lg, pos, target, mode, drop_self):
    """(rowstats (B, 8), flags (B,), scalars (5,), dlogits (B, N1)) of one forward + backward, guards checked."""
    from coclr_amd import ops
    B, N1 = lg.shape
    logits = source2d(lg)
    mask = source2d(pos.to(torch.uint8)) if mode != 0 else None
    tgt = source2d(target.reshape(1, -1))[0] if mode == 0 else None
    rowstats, flags, scalars = Placed2D(B, 8), Placed2D(1, B, fill=9, around=200, dtype=torch.uint8), Placed2D(1, 5)
    ops.nce_loss_fwd(logits, mask, tgt, rowstats.view, flags.view[0], scalars.view[0], mode, drop_self, 1, 5)
    sync("nce_loss_fwd")
    dlogits = Placed2D(B, N1)
    ops.nce_loss_bwd(logits, mask, tgt, rowstats.view, flags.view[0], source2d(torch.tensor([[DLOSS]]))[0],
                     dlogits.view, mode)
    sync("nce_loss_bwd")
    out = (rowstats.view.clone().cpu(), flags.view[0].clone().cpu(), scalars.view[0].clone().cpu(),
           dlogits.view.clone().cpu())
    for p in (rowstats, flags, scalars, dlogits):
        assert p.untouched_around(), "a guard region was written"
    return out


def hit_bits(flags):
    """(B, 4): hit@1, hit@5, self hit@1, self hit@5 from bits 1..4 of the flag bytes."""
    return torch.stack([(flags >> i) & 1 for i in (1, 2, 3, 4)], 1)


def aten_fp32_gradient(lg, eff, mode):
    """The reference's own fp32 arithmetic (ATen on the CPU) for d(DLOSS * mean loss) / d logits."""
    x = lg.float().requires_grad_(True)
    if mode == 0:
        loss = F.cross_entropy(x, eff.float().argmax(1), reduction="none")
    elif mode == 2:
        loss = -(F.log_softmax(x, 1) * eff).sum(1) / eff.sum(1)
    else:
        loss = -torch.logsumexp(F.log_softmax(x, 1).masked_fill(~eff, R.NEG_INF), 1)
    (loss.mean() * DLOSS).backward()
    return x.grad.double()


@pytest.mark.parametrize("c", H.LOSS, ids=[c.name for c in H.LOSS])
def test_loss_rows(c):
    """Measured on an MI355X, maxima over the table, relative to max|ref| of the row group: ordinary rows loss 9.8e-8,
    lse 1.2e-7, dlogits 1.1e-7; scaled rows loss 7.0e-8, lse 3.0e-8, dlogits 4.3e-8 (the fp32 ATen reference: 4.3e-8 on
    the same rows, 1.6e-5 on the multi-positive rows whose softmax form underflows)."""
    lg, pos, target = R.loss_inputs(c.mode, c.drop_self, c.B, c.N1, R.gen(c.mode, c.B, c.N1))
    ref = R.loss_reference(lg, pos, c.mode, c.drop_self)
    grad = R.loss_gradient(lg, pos, c.mode, c.drop_self, DLOSS)
    rowstats, flags, scalars, dlogits = run_loss(lg, pos, target, c.mode, c.drop_self)

    # exact: ranks, flags, accuracies, row maxima
    exact(hit_bits(flags), ref["hits"], "hit flags")
    assert torch.equal(flags & 1, ref["drop"].to(torch.uint8)), "drop flags"
    assert int(flags.max()) < 32
    exact(scalars[1:], ref["hits"].mean(0), "accuracy scalars")
    exact(rowstats[:, 7], lg.max(1).values, "row maxima")
    if c.mode == 2:
        exact(rowstats[:, 2], ref["aux"], "positive counts")
    # the scaled rows are "wide" rows of loss.hip (|max| >= 64), the others are not (range 6): only the wide rows carry
    # the low parts.  There lse + lse_lo is the log-sum-exp to the accuracy of the small logarithm alone: logf within
    # 2 ulp (2.4e-7) of lz = lse - max, the fp32 sum and the residual's own rounding 6e-8 each
    large = lg.abs().max(1).values > 100
    if c.mode == 0 and bool(large.any()):
        exact(rowstats[large, 2], lg[torch.arange(c.B), target][large], "mode 0, scaled rows: the positive's logit")
    assert bool((rowstats[~large, 3:5] == 0).all()), "low parts on an ordinary row"
    lz = ref["lse"] - lg.max(1).values
    err = (rowstats[:, 1].double() + rowstats[:, 3].double() - ref["lse"]).abs()
    assert bool((err[large] <= 5e-7 * torch.clamp(lz[large], min=1.0)).all()), "lse + lse_lo: %.3e" % float(err.max())

    # tolerances, per row group
    for what, rows in (("ordinary", ~large), ("scaled", large)):
        if not bool(rows.any()):
            continue
        print("%s %s rows: loss %.2e lse %.2e dlogits %.2e" % (
            c.name, what, rel_err(rowstats[rows, 0], ref["loss"][rows]), rel_err(rowstats[rows, 1], ref["lse"][rows]),
            rel_err(dlogits[rows], grad[rows])))
        check_close(rowstats[rows, 0], ref["loss"][rows], 1e-6, what + " rows: loss")
        check_close(rowstats[rows, 1], ref["lse"][rows], 1e-6, what + " rows: lse")
        if c.mode != 2:
            check_close(rowstats[rows, 2], ref["aux"][rows], 1e-6, what + " rows: log-sum-exp of the positives")
        if what == "ordinary":
            check_close(dlogits[rows], grad[rows], 1e-5, "ordinary rows: dlogits")
        else:
            e_aten = rel_err(aten_fp32_gradient(lg, ref["eff"], c.mode)[rows], grad[rows])
            e_got = rel_err(dlogits[rows], grad[rows])
            print("%s scaled rows: dlogits err %.3e, fp32 ATen %.3e" % (c.name, e_got, e_aten))
            assert e_got <= max(1e-5, 2 * e_aten), "scaled rows: dlogits err %.3e, fp32 ATen %.3e" % (e_got, e_aten)
    check_close(scalars[:1], ref["scalars"][:1], 1e-6, "loss scalar")


@pytest.mark.parametrize("drop_self", (False, True))
def test_row_without_a_positive(drop_self):
    B, N1 = 3, 77
    lg, pos, _ = R.loss_inputs(1, drop_self, B, N1, R.gen(B, N1, 11))
    pos[2] = False
    rowstats, flags, scalars, dlogits = run_loss(lg, pos, None, 1, drop_self)
    ref = R.loss_reference(lg, pos, 1, drop_self)
    assert float(rowstats[2, 0]) == float("inf") and float(scalars[0]) == float("inf")
    assert hit_bits(flags)[2, :2].tolist() == [0, 0] and int(flags[2]) & 1 == 0
    keep = torch.tensor([0, 1])
    check_close(rowstats[keep, 0], ref["loss"][keep], 1e-6, "the other rows' loss")
    exact(hit_bits(flags)[keep], ref["hits"][keep], "the other rows' hit flags")
    # no positive: the gradient is DLOSS / B * softmax
    check_close(dlogits[2], torch.softmax(lg[2], 0) * DLOSS / B, 1e-5, "dlogits of the row without a positive")
