"""Exact max-pooling: every row of tests/_pool_cases.py (every kernel instantiation and dispatch edge of
coclr_amd/csrc/pool.hip's launchers, see tests/test_pool_plan_cpu.py) against float64.

  * forward: values and arg-max indices equal F.max_pool3d(..., return_indices=True) on the float64 copy of the
    input.  The input is relu(randn): half of the elements are equal zeros, so first-max-wins is exercised
    everywhere; `special` rows carry -inf / NaN instead.  In-affine rows use scales +-2^k and small-integer shifts,
    so fmaf(x, scale, shift) is the float64 value rounded once.
  * backward: dy holds integers in [-3, 3], so every sum of at most 27 addends is exact in any order and dx equals
    float64 autograd; plain write and accumulate.
  * pooled BatchNorm backward: integer convolution outputs and pool gradients, power-of-two scale and invstd,
    small-integer shift and mean: dgamma / dbeta are exact, dy equals the float64 reference with fp32 roundings at
    the determined points (tests/_exact.py), and equals pool backward + BatchNorm backward run separately.  Also on
    randn data at 5e-4 * max|ref| (tests/test_gpu_kernels.py), twice, bit-identically.

Memory a kernel must not read holds 2^20; memory it must not write holds a sentinel that is compared afterwards;
memory it must write first holds NaN.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import _pool_cases as P
from _exact import NAN, Placed, bn_backward_reference, close, exact, per_channel, source, sync, vector

pytestmark = pytest.mark.gpu

IDS = [c.name for c in P.CASES]
POOLED = [c.name for c in P.CASES if c.pooled]


def _coef(c):
    scale, shift = P.affine(c)
    return torch.tensor(scale, dtype=torch.float64), torch.tensor(shift, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def problem(name):
    """(x fp32, pool input in float64, reference y float64, reference indices, dy int, reference dx float64)."""
    c = P.BY_NAME[name]
    gen = torch.Generator().manual_seed(len(name) * 131 + c.C)
    x = torch.relu(torch.randn(c.N, c.C, *c.idim, generator=gen))
    if c.special:
        x = torch.randn(c.N, c.C, *c.idim, generator=gen)
        x.view(-1)[::7] = -float("inf")
        x.view(-1)[5::131] = float("nan")
        x[0, 0].fill_(-float("inf"))
    a = x.double()
    if c.aff:
        sc, sf = _coef(c)
        a = (a * per_channel(sc) + per_channel(sf)).float().double()       # fmaf: one rounding
        if c.aff == "relu":
            a = torch.relu(a)
    a.requires_grad_(True)
    y, idx = F.max_pool3d(a, c.k, c.s, c.p, return_indices=True)
    dy = torch.randint(-3, 4, y.shape, generator=gen).double()
    y.backward(dy)
    return x, a.detach(), y.detach(), idx, dy, a.grad


def describe(c, with_idx=True):
    pl = P.plan(c, with_idx)
    return "%s fwd %s %s G=%d | bwd %s %s G=%d" % (c.name, pl["fwd"]["family"], pl["fwd"]["template"], pl["fwd"]["G"],
                                                   pl["bwd"]["family"], pl["bwd"]["template"], pl["bwd"]["G"])


def in_affine(c):
    if not c.aff:
        return {}
    sc, sf = _coef(c)
    return dict(in_scale=vector(sc), in_shift=vector(sf), in_relu=c.aff == "relu")


@pytest.mark.parametrize("with_idx", [True, False], ids=["idx", "noidx"])
@pytest.mark.parametrize("name", IDS)
def test_forward(name, with_idx):
    from coclr_amd import ops
    c = P.BY_NAME[name]
    x, _, ref, ridx, _, _ = problem(name)
    what = describe(c, with_idx)
    xd = source(x, c.x_extra, c.x_pad)
    yp = Placed(tuple(ref.shape), c.y_extra, 0)
    ip = Placed(tuple(ref.shape), 0, 0, fill=-7, around=-9, dtype=torch.int32) if with_idx else None
    st = P.strides(c)
    if c.N > 1:
        assert (xd.stride(0), yp.view.stride(0)) == (st["x"], st["y"]), what
    ops.maxpool_fwd(P.geom(c), xd, yp.view, ip.view if with_idx else None, **in_affine(c))
    sync(what)
    exact(yp.view, ref, what + ": y")
    assert yp.untouched_around(), "%s: wrote outside y" % what
    if with_idx:
        exact(ip.view, ridx.int(), what + ": indices")
        assert ip.untouched_around(), "%s: wrote outside the indices" % what


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("name", IDS)
def test_backward(name, accumulate):
    from coclr_amd import ops
    c = P.BY_NAME[name]
    x, _, _, ridx, dy, rdx = problem(name)
    what = describe(c)
    dyd = source(dy, c.d_extra, c.d_pad)
    idx = source(ridx.int())
    dxp = Placed(tuple(x.shape), c.d_extra, c.d_pad)
    prior = None
    if accumulate:
        prior = torch.randint(-8, 9, x.shape, generator=torch.Generator().manual_seed(5)).double()
        dxp.put(prior)
    st = P.strides(c)
    if c.N > 1:
        assert (dyd.stride(0), dxp.view.stride(0)) == (st["dy"], st["dx"]), what
    ops.maxpool_bwd(P.geom(c), dyd, idx, dxp.view, accumulate=accumulate)
    sync(what)
    exact(dxp.view, rdx + prior if accumulate else rdx, what + ": dx")
    assert dxp.untouched_around(), "%s: wrote outside dx" % what


# ---- pooled BatchNorm backward ------------------------------------------------------------------------------------------

def _unit(c, kind):
    """The BatchNorm unit in front of the pool: (y, scale, shift, mean, invstd, pool_dy), float64."""
    gen = torch.Generator().manual_seed(c.C * 7 + 1)
    sc, sf = _coef(c)
    ch = torch.arange(c.C)
    if kind == "int":
        y = torch.randint(-4, 5, (c.N, c.C) + c.idim, generator=gen).double()
        mean = torch.tensor([0.0, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0])[ch % 7].double()
        invstd = 2.0 ** (-(ch % 3).double())
        pdy = torch.randint(-3, 4, (c.N, c.C) + P.odim(c), generator=gen).double()
    else:
        y = torch.randn((c.N, c.C) + c.idim, generator=gen).double()
        mean = torch.randn(c.C, generator=gen).double() * 0.3
        invstd = (torch.rand(c.C, generator=gen).double() + 0.5)
        sc = (torch.rand(c.C, generator=gen).double() + 0.5) * torch.where(ch % 3 == 1, -1.0, 1.0).double()
        sf = torch.randn(c.C, generator=gen).double() * 0.2
        pdy = torch.randn((c.N, c.C) + P.odim(c), generator=gen).double()
    return y, sc, sf, mean, invstd, pdy


@functools.lru_cache(maxsize=None)
def pooled_problem(name, kind):
    c = P.BY_NAME[name]
    y, sc, sf, mean, invstd, pdy = _unit(c, kind)
    y, pdy = y.float().double(), pdy.float().double()
    sc, sf, mean, invstd = (t.float().double() for t in (sc, sf, mean, invstd))
    a = (y * per_channel(sc) + per_channel(sf)).float().double()
    a.requires_grad_(True)
    r = torch.relu(a) if c.aff == "relu" else a
    _, idx = F.max_pool3d(r, c.k, c.s, c.p, return_indices=True)
    F.max_pool3d(r, c.k, c.s, c.p).backward(pdy)
    return y, sc, sf, mean, invstd, pdy, idx, a.grad, a.detach()


def _run_pooled(c, prob, training):
    from coclr_amd import ops
    y, sc, sf, mean, invstd, pdy, idx, _, _ = prob
    g = P.geom(c)
    yd = source(y, c.x_extra, c.x_pad)
    coefs = [vector(t) for t in (sc, sf, mean, invstd)]
    pdyd = source(pdy, c.d_extra, c.d_pad)
    idxd = source(idx.int())
    dyp = Placed(tuple(y.shape), c.d_extra, c.d_pad)
    dgb = Placed((2, c.C), 0, 0)
    sums = torch.full((ops.bn_backward_workspace(c.N, c.C),), NAN, dtype=torch.float64, device="cuda")
    ops.bn_act_backward_pooled(g, pdyd, idxd, yd, coefs[0], coefs[1], coefs[2], coefs[3], sums, dyp.view,
                               dgb.view[0], dgb.view[1], c.aff == "relu", training)
    sync("pooled BatchNorm backward of " + c.name)
    return dyp, dgb, (yd, coefs, pdyd, idxd)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", POOLED)
def test_pooled_bn_backward_exact(name, training):
    from coclr_amd import ops
    c = P.BY_NAME[name]
    prob = pooled_problem(name, "int")
    y, sc, sf, mean, invstd, pdy, idx, dz, a = prob
    q = P.plan(c)["pooled"]
    what = "%s pooled %s G=%d %s" % (name, q["template"], q["G"], "train" if training else "eval")
    if c.aff == "relu":
        assert bool((a == 0).any()), "%s: no element with y * scale + shift == 0" % what
    rdy, rdg, rdb, _, _, _ = bn_backward_reference(dz, y, sc, mean, invstd, training)
    # the forward the backward belongs to gives these indices
    yd = source(y, c.x_extra, c.x_pad)
    fi = Placed(tuple(pdy.shape), 0, 0, fill=-7, around=-9, dtype=torch.int32)
    fy = Placed(tuple(pdy.shape), 0, 0)
    ops.maxpool_fwd(P.geom(c), yd, fy.view, fi.view, in_scale=vector(sc), in_shift=vector(sf),
                    in_relu=c.aff == "relu")
    sync(what)
    exact(fi.view, idx.int(), what + ": forward indices")
    dyp, dgb, (yd, coefs, pdyd, idxd) = _run_pooled(c, prob, training)
    exact(dgb.view[0], rdg, what + ": dgamma")
    exact(dgb.view[1], rdb, what + ": dbeta")
    exact(dyp.view, rdy, what + ": dy")
    # ... and equals pool backward followed by the BatchNorm backward
    dzd = torch.full(tuple(y.shape), NAN, device="cuda")
    ops.maxpool_bwd(P.geom(c), pdyd, idxd, dzd)
    dy2 = torch.full(tuple(y.shape), NAN, device="cuda")
    dgb2 = torch.full((2, c.C), NAN, device="cuda")
    sums = torch.full((ops.bn_backward_workspace(c.N, c.C),), NAN, dtype=torch.float64, device="cuda")
    ops.bn_act_backward(dzd, yd, None, coefs[0], coefs[1], coefs[2], coefs[3], sums, dy2, None, dgb2[0], dgb2[1],
                        c.aff == "relu", training)
    sync(what)
    assert torch.equal(dyp.view, dy2) and torch.equal(dgb.view, dgb2), "%s: differs from the two separate calls" % what
    assert dyp.untouched_around() and dgb.untouched_around(), "%s: wrote outside dy or dgamma / dbeta" % what


@pytest.mark.parametrize("name", POOLED)
def test_pooled_bn_backward_random(name):
    c = P.BY_NAME[name]
    prob = pooled_problem(name, "randn")
    y, sc, sf, mean, invstd, pdy, idx, dz, _ = prob
    rdy, rdg, rdb, _, _, _ = bn_backward_reference(dz, y, sc, mean, invstd, True, exact_roundings=False)
    dyp, dgb, _ = _run_pooled(c, prob, True)
    close(dyp.view, rdy, 5e-4, name + ": dy")
    close(dgb.view[0], rdg, 5e-4, name + ": dgamma")
    close(dgb.view[1], rdb, 5e-4, name + ": dbeta")
    again, dgb2, _ = _run_pooled(c, prob, True)
    assert torch.equal(dyp.view, again.view) and torch.equal(dgb.view, dgb2.view), "%s: not bit-identical" % name
