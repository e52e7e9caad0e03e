"""Exact max-pooling at the edges of the slot and clamp arithmetic in coclr_amd/csrc/pool.hip, next to the dispatch
table of tests/test_gpu_pool_exact.py:

  * the colour-class backward takes a thread slot apart into (volume, a, b, cc) ONCE and every class adds a constant
    offset to it: volumes of 4x4x4 (the gather form), 8x8x8, 16x16x16 and 16x16x8 / 8x16x16 with unequal sides (a
    transposed offset cannot go unnoticed), extents that are no multiple of the class counts, 1, 2, 4 and 8 volumes per
    workgroup, a partial last group, a group that holds the end of one sample and the start of the next with dy and
    dx channel slices, 16-byte and 4-byte stores (one operand one float off alignment), accumulate on and off;
  * quotients by the reciprocal (pool_quot): plane numbers below and above 2^20 in the tiled forward and in the
    backward's store pass (the colour-class loads cannot see a plane number above 2^20 below this file's size
    limit: a template needs G * ceil(To/PT) * ceil(Ho/PH) * ceil(Wo/PW) <= 512 and G stays >= 1024 there);
  * the tiled forward reads every window element from a clamped address and replaces what lies outside by -inf:
    planes that hold only negative values (a padding of 0 would win there), windows that hang over every face,
    data with many ties (values in {0, 1, 2}: first-max-wins decides nearly every index).

The workgroups of these kernels process one group of volumes each (no ring, no loop over groups), so "groups per
workgroup" has no further case; the volumes per group are the G above.

Values and indices are compared with F.max_pool3d(..., return_indices=True) on the float64 copy, dx with float64
autograd of integer-valued dy (every sum of at most 27 addends is exact in any order), all with torch.equal; every
output lies between guard runs that must come back untouched.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import _pool_cases as P
from _exact import Placed, per_channel, source, sync, vector

pytestmark = pytest.mark.gpu

K333, S1, P1 = (3, 3, 3), (1, 1, 1), (1, 1, 1)
K133, S122, P011 = (1, 3, 3), (1, 2, 2), (0, 1, 1)
S222, K222, P0 = (2, 2, 2), (2, 2, 2), (0, 0, 0)

# row, then what the plan must say for it (forward family, forward G, backward family, backward G): a row that no
# longer reaches its edge fails instead of passing for nothing
ROWS = [
    (P.case("v4", 2, 37, (4, 4, 4), K333, S1, P1, x_extra=1, y_extra=1, d_extra=2), "sep333", 16, "gather333", 1),
    (P.case("v8", 2, 5, (8, 8, 8), K333, S1, P1, x_extra=2, y_extra=1, d_extra=1), "sep333", 4, "classes", 1),
    (P.case("v8_g2", 3, 683, (8, 8, 8), K333, S1, P1, d_extra=1), "sep333", 4, "classes", 2),
    (P.case("v8_g4_odd_dx", 2, 2047, (8, 8, 8), K333, S1, P1, d_pad=1), "sep333", 4, "classes", 4),
    (P.case("v16", 2, 3, (16, 16, 16), K333, S1, P1, x_pad=1, d_extra=1), "sep333", 1, "classes", 1),
    (P.case("v16x16x8", 2, 3, (16, 16, 8), K333, S1, P1), "sep333", 2, "classes", 1),
    (P.case("v8x16x16", 1, 5, (8, 16, 16), K333, S1, P1, d_pad=3), "sep333", 1, "classes", 1),
    (P.case("v5x7x6", 2, 3, (5, 7, 6), K333, S1, P1, d_extra=1), "tiled", 1, "classes", 1),      # To, Ho % 3 != 0
    (P.case("v2x4x4_g2", 2, 4093, (2, 4, 4), K333, S1, P1, x_extra=1, y_extra=1, d_extra=1), "sep333", 16,
     "gather333", 2),
    (P.case("t133_g4", 2, 195, (21, 16, 16), K133, S122, P011, x_extra=1, y_extra=1, d_extra=1, aff="relu"),
     "tiled", 4, "classes", 8),                    # 8190 folded planes: partial last group, groups across samples
    (P.case("t133_odd_x", 2, 3, (2, 12, 10), K133, S122, P011, x_pad=1, d_pad=1, aff="plain"), "tiled", 1,
     "classes", 1),
    (P.case("t133_11x13", 2, 3, (3, 11, 13), K133, S122, P011, aff="relu"), "tiled", 1, "classes", 1),   # Si = 143
    (P.case("t133_planes_2p20", 2, 600011, (1, 1, 1), K133, S122, P011, d_extra=1), "tiled", 512, "classes", 1024),
    (P.case("t333s2", 2, 3, (7, 9, 11), K333, S222, P1, d_extra=1), "tiled", 1, "classes", 1),
    (P.case("t333s2_g2", 2, 2049, (4, 8, 8), K333, S222, P1, x_extra=1, y_extra=1, d_extra=1), "tiled", 2,
     "classes", 4),
    (P.case("t222_odd", 2, 3, (5, 6, 7), K222, S222, P0, x_pad=1), "tiled", 1, "classes", 1),
]
CASES = {r[0].name: r for r in ROWS}
IDS = list(CASES)
DATA = ["ties", "negative"]


def _coef(c):
    scale, shift = P.affine(c)
    return torch.tensor(scale, dtype=torch.float64), torch.tensor(shift, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def problem(name, data):
    """(x fp32, reference y float64, reference indices, dy, reference dx float64), computed once per row and kind."""
    c = CASES[name][0]
    assert P.elems(c) <= P.MAX_ELEMS, name
    gen = torch.Generator().manual_seed(len(name) * 977 + c.C + (data == "ties"))
    x = torch.randint(0, 3, (c.N, c.C) + c.idim, generator=gen).float()
    if data == "negative":
        x = -1.0 - x                 # {-1, -2, -3} everywhere: any padding but -inf would be the maximum
        x[:, ::3] += 4.0             # ... and every third channel mixes signs: {3, 2, 1}
    a = x.double()
    if c.aff:
        sc, sf = _coef(c)
        a = (a * per_channel(sc) + per_channel(sf)).float().double()
        if c.aff == "relu":
            a = torch.relu(a)
    a.requires_grad_(True)
    y, idx = F.max_pool3d(a, c.k, c.s, c.p, return_indices=True)
    dy = torch.randint(-3, 4, y.shape, generator=gen).double()
    y.backward(dy)
    return x, y.detach(), idx, dy, a.grad


def describe(c, with_idx=True):
    pl = P.plan(c, with_idx)
    return "%s fwd %s %s G=%d vec=%d | bwd %s %s G=%d vec=%d" % (
        c.name, pl["fwd"]["family"], pl["fwd"]["template"], pl["fwd"]["G"], pl["fwd"]["vec"], pl["bwd"]["family"],
        pl["bwd"]["template"], pl["bwd"]["G"], pl["bwd"]["vec"])


def in_affine(c):
    if not c.aff:
        return {}
    sc, sf = _coef(c)
    return dict(in_scale=vector(sc), in_shift=vector(sf), in_relu=c.aff == "relu")


@pytest.mark.parametrize("name", IDS)
def test_rows_reach_their_edges(name):
    c, ffam, fg, bfam, bg = CASES[name]
    pl = P.plan(c, True)
    print(describe(c))
    assert (pl["fwd"]["family"], pl["fwd"]["G"]) == (ffam, fg), pl["fwd"]
    assert (pl["bwd"]["family"], pl["bwd"]["G"]) == (bfam, bg), pl["bwd"]


def test_rows_cover_the_path_flags():
    plans = [P.plan(r[0], True) for r in ROWS]
    for part in ("fwd", "bwd"):
        assert {bool(p[part]["vec"]) for p in plans} == {True, False}, part      # 16-byte and 4-byte paths
    assert any(r[0].N * r[0].C > 1 << 20 for r in ROWS)                           # plane numbers above 2^20
    # a partial last group, backward and forward
    assert any(p["bwd"]["G"] > 1 and (r[0].N * r[0].C * max(p["bwd"]["tfold"], 1)) % p["bwd"]["G"]
               for p, r in zip(plans, ROWS))
    assert any(p["fwd"]["G"] > 1 and (r[0].N * r[0].C * max(p["fwd"]["tfold"], 1)) % p["fwd"]["G"]
               for p, r in zip(plans, ROWS))


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("with_idx", [True, False], ids=["idx", "noidx"])
@pytest.mark.parametrize("name", IDS)
def test_forward(name, with_idx, data):
    from coclr_amd import ops
    c = CASES[name][0]
    x, ref, ridx, _, _ = problem(name, data)
    what = describe(c, with_idx) + " " + data
    xd = source(x, c.x_extra, c.x_pad)
    yp = Placed(tuple(ref.shape), c.y_extra, 0)
    ip = Placed(tuple(ref.shape), 0, 0, fill=-7, around=-9, dtype=torch.int32) if with_idx else None
    ops.maxpool_fwd(P.geom(c), xd, yp.view, ip.view if with_idx else None, **in_affine(c))
    sync(what)
    assert torch.equal(yp.view.double().cpu(), ref), what + ": y"
    assert yp.untouched_around(), "%s: wrote outside y" % what
    if with_idx:
        assert torch.equal(ip.view.long().cpu(), ridx), what + ": indices"
        assert ip.untouched_around(), "%s: wrote outside the indices" % what


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("name", IDS)
def test_backward(name, accumulate, data):
    from coclr_amd import ops
    c = CASES[name][0]
    x, _, ridx, dy, rdx = problem(name, data)
    what = describe(c) + " " + data
    dyd = source(dy, c.d_extra, c.d_pad)
    idx = source(ridx.int())
    dxp = Placed(tuple(x.shape), c.d_extra, c.d_pad)
    want = rdx
    if accumulate:
        prior = torch.randint(-8, 9, x.shape, generator=torch.Generator().manual_seed(5)).double()
        dxp.put(prior)
        want = rdx + prior
    st = P.strides(c)
    if c.N > 1:
        assert (dyd.stride(0), dxp.view.stride(0)) == (st["dy"], st["dx"]), what
    ops.maxpool_bwd(P.geom(c), dyd, idx, dxp.view, accumulate=accumulate)
    sync(what)
    assert torch.equal(dxp.view.double().cpu(), want), what + ": dx"
    assert dxp.untouched_around(), "%s: wrote outside dx" % what
