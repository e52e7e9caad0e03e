"""Exact weight gradients: every row of tests/_wgrad_cases.py (every kernel instantiation and dispatch edge the
launcher of coclr_amd/csrc/conv_wgrad.hip has, see tests/test_wgrad_plan_cpu.py) against F.conv3d in float64.

Exactness.  x and dy are integers in [-2, 2], so every product and every partial sum below is an integer (or a
dyadic fraction) far below 2^24 units of its granularity and fp32 represents it exactly WHATEVER the summation
order, the split count or the fold order.  With P <= 32768 output positions per row (asserted in the CPU tier):

  * direct forms: |x * dy| <= 4, so every partial sum is an integer of magnitude <= 4 P = 2^17;
  * F(2,3) along T (id 6): the operands are dy0, dy0 + dy1, dy0 - dy1, dy1 (|.| <= 4) and d0 - d2, d1 + d2,
    d2 - d1, d3 - d1 (|.| <= 4): integer terms <= 16 per frame pair, <= 16 * P / 2 = 2^18 in all; the epilogue
    forms dU0 + (dU1 + dU2) / 2, (dU1 - dU2) / 2, (dU1 + dU2) / 2 + dU3: multiples of 1/2 below 2^20;
  * F(2x2,3x3) (id 7): dM = A dY A^T sums at most four dy (|dM| <= 8), V = B^T d B at most four d (|V| <= 8):
    integer terms <= 64 per 2x2 block, <= 64 * P / 4 = 2^19 in all; G^T dU G has entries 1 and 1/2: multiples of
    1/4 below 2^22, i.e. below 2^24 quarter-units;
  * the stem's BatchNorm form: dy = A g + B y + D with A in {1, 2}, B = +-1/2, D in {-1, 0, 1}, integer g and y:
    multiples of 1/2 of magnitude <= 7, products with x <= 14, sums below 2^20 half-units.

No kernel form contains an operation that rounds on such data, so EVERY form -- direct and Winograd-domain -- is
compared with torch.equal against the float64 reference cast to fp32; nothing here uses a tolerance on integer
data.  A prior dw in the accumulate variant holds integers in [-8, 8].  Memory a kernel must not include holds
2^20 (finite: a masked lane that is loaded and multiplied by zero is no false alarm, a stray inclusion breaks
equality); memory it must not write holds a sentinel that is compared afterwards; memory it must write before
it reads (dw of a plain write, the split workspace) holds NaN.

Each row also runs once on randn data against the same float64 reference at the project's 2e-4 * max|ref| (small
integers would stay exact under a reduced-precision matrix instruction; these do not), twice, bit-identically.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import _wgrad_cases as W

pytestmark = pytest.mark.gpu

RTOL = 2e-4            # tests/test_gpu_kernels.py
OUTSIDE = float(2 ** 20)
GUARD = -12345.0
IDS = [c.name for c in W.CASES]


@functools.lru_cache(maxsize=None)
def problem(name, kind):
    """(x, dy, reference dw) on the CPU: x / dy fp32 tensors holding the drawn values, the reference in float64
    from F.conv3d + autograd.  A kt-slice row is checked against its temporal tap of the FULL stencil."""
    c = W.BY_NAME[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 7 + len(kind))
    k, p, t = (c.k, c.p, None) if c.slice_of is None else c.slice_of

    def draw(shape):
        if kind == "int":
            return torch.randint(-2, 3, shape, generator=gen).float()
        return torch.randn(shape, generator=gen)

    x = draw((c.N, c.Cin) + tuple(c.dims))
    w = torch.zeros((c.Cout, c.Cin) + tuple(k), dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x.double(), w, None, c.s, p)
    assert tuple(y.shape[2:]) == W.geom(c).odim
    dy = draw(tuple(y.shape))
    y.backward(dy.double())
    ref = w.grad if t is None else w.grad[:, :, t:t + 1]
    return x, dy, ref.contiguous()


def sync():
    """A launch that faulted ends the session: nothing more is started on a device in that state."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a weight-gradient launch: %s" % e, returncode=3)


def guarded(n, fill, guard=64):
    """n floats holding `fill` between two guard runs; returns (whole buffer, the n floats)."""
    big = torch.full((n + 2 * guard,), GUARD, device="cuda")
    mid = big[guard:guard + n]
    mid.fill_(fill)
    return big, mid


def guards_intact(big, n, guard=64):
    return bool((big[:guard] == GUARD).all()) and bool((big[guard + n:] == GUARD).all())


def wgrad(c, x, dy, dw=None, accumulate=False, co_stride=None, ci_stride=None, tap_base=0):
    """One conv_wgrad call into a NaN-filled (or given) dw with an exactly sized, NaN-filled, guarded workspace."""
    from coclr_amd import ops
    g = W.geom(c)
    taps = g.taps
    n = g.wgrad_workspace()
    big, ws = guarded(n, float("nan"))
    if dw is None:
        dw = torch.full((c.Cout, c.Cin) + tuple(c.k), float("nan"), device="cuda")
    ops.conv_wgrad(g, x, dy, dw, ws, c.Cin * taps if co_stride is None else co_stride,
                   taps if ci_stride is None else ci_stride, tap_base, accumulate)
    sync()
    assert guards_intact(big, n), "%s: the split workspace was written outside wgrad_workspace()" % c.name
    return dw


def exact(got, ref, what):
    got, ref = got.detach().cpu(), ref.float()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not torch.equal(got, ref):
        bad = (got != ref) | got.isnan()
        idx = bad.nonzero()[0].tolist()
        raise AssertionError("%s: %d of %d elements differ from float64; first at %s: got %r, want %r" % (
            what, int(bad.sum()), bad.numel(), idx, got[tuple(idx)].item(), ref[tuple(idx)].item()))


def describe(c, aligned=True, x_nstride=None, y_nstride=None):
    pl = W.geom(c).wgrad_plan(aligned, x_nstride, y_nstride)
    return "%s -> %s" % (c.name, W.instantiation(pl)), pl


@pytest.mark.parametrize("name", IDS)
def test_plain_write(name):
    c = W.BY_NAME[name]
    x, dy, ref = problem(name, "int")
    what, _ = describe(c)
    exact(wgrad(c, x.cuda(), dy.cuda()), ref, what)


@pytest.mark.parametrize("name", IDS)
def test_accumulate(name):
    c = W.BY_NAME[name]
    x, dy, ref = problem(name, "int")
    prior = torch.randint(-8, 9, ref.shape, generator=torch.Generator().manual_seed(5)).float()
    what, _ = describe(c)
    exact(wgrad(c, x.cuda(), dy.cuda(), dw=prior.clone().cuda(), accumulate=True), ref + prior.double(), what)


def channel_slice(t, offset, extra, misalign=0):
    """t as channels [offset, offset + C) of a buffer `extra` channels wider with one extra sample of tail,
    everything else holding OUTSIDE; the buffer starts `misalign` floats into its allocation."""
    N, Cc = t.shape[:2]
    shape = (N + 1, Cc + extra) + tuple(t.shape[2:])
    numel = 1
    for v in shape:
        numel *= v
    flat = torch.full((numel + misalign,), OUTSIDE, device="cuda")
    wide = flat[misalign:].view(shape)
    view = wide[:N, offset:offset + Cc]
    view.copy_(t)
    return view


@pytest.mark.parametrize("name", IDS)
def test_operands_as_channel_slices(name):
    """x and dy at an odd channel offset inside wider buffers (what the separable branches of an inception block
    read: slices of the fused-heads buffer)."""
    c = W.BY_NAME[name]
    x, dy, ref = problem(name, "int")
    xv, dyv = channel_slice(x.cuda(), 3, 5), channel_slice(dy.cuda(), 1, 7)
    aligned = xv.data_ptr() % 16 == 0 and dyv.data_ptr() % 16 == 0
    what, pl = describe(c, aligned, xv.stride(0), dyv.stride(0))
    print(what)
    exact(wgrad(c, xv, dyv), ref, what)


POINTWISE_DMA = [c.name for c in W.CASES if W.geom(c).wgrad_plan(True)["family"] == "pwdma"]


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("name", POINTWISE_DMA)
def test_pointwise_slices_take_the_dma_kernel_only_when_aligned(name, aligned):
    """Channel offset 4 of a buffer 8 channels wider keeps both base pointers 16-byte aligned and the sample
    strides multiples of four: the 16-byte-DMA kernel.  A plane that is eligible holds a multiple of 64
    positions, so no channel offset inside an aligned buffer can misalign it; a buffer that starts an odd number
    of floats into its allocation does (a view into a flat bucket), and the launcher must then take id 4 / 5."""
    c = W.BY_NAME[name]
    x, dy, ref = problem(name, "int")
    mis = 0 if aligned else 1
    xv, dyv = channel_slice(x.cuda(), 4, 8, mis), channel_slice(dy.cuda(), 4, 8, mis)
    is_aligned = xv.data_ptr() % 16 == 0 and dyv.data_ptr() % 16 == 0
    assert is_aligned == aligned
    what, pl = describe(c, is_aligned, xv.stride(0), dyv.stride(0))
    print(what)
    assert pl["family"] == ("pwdma" if aligned else "wave") and pl["id"] in (4, 5)
    exact(wgrad(c, xv, dyv), ref, what)


@pytest.mark.parametrize("name", IDS)
def test_strided_destination(name):
    """dw addressed with co_stride > Cin * taps, ci_stride > taps and tap_base > 0 inside a sentinel-filled
    buffer: every element that is not addressed keeps the sentinel.  A kt-slice row uses the layout it has in
    production -- its temporal tap inside the full [Cout][Cin][kt][kh][kw] parameter."""
    c = W.BY_NAME[name]
    x, dy, ref = problem(name, "int")
    taps = c.k[0] * c.k[1] * c.k[2]
    if c.slice_of is None:
        ci_stride, tap_base = taps + 3, 2
        co_stride = c.Cin * ci_stride + 5
    else:
        full = c.slice_of[0][0] * taps
        ci_stride, tap_base, co_stride = full, c.slice_of[2] * taps, c.Cin * full
        assert tap_base > 0
    n = c.Cout * co_stride
    big, buf = guarded(n, GUARD)
    want = torch.full((n,), GUARD)
    co = torch.arange(c.Cout).view(-1, 1, 1) * co_stride
    ci = torch.arange(c.Cin).view(1, -1, 1) * ci_stride
    tp = torch.arange(taps).view(1, 1, -1) + tap_base
    want[(co + ci + tp).reshape(-1)] = ref.float().reshape(-1)
    what, _ = describe(c)
    wgrad(c, x.cuda(), dy.cuda(), dw=buf, co_stride=co_stride, ci_stride=ci_stride, tap_base=tap_base)
    assert guards_intact(big, n), what
    exact(buf, want, what)


@pytest.mark.parametrize("name", IDS)
def test_both_workgroup_orders(name, monkeypatch):
    """COCLR_WGRAD_ORDER is read per call (tools/wgrad_order_ab.py): split-fastest and tile-fastest XCD-aware
    workgroup ids give the same bits, equal to the reference."""
    c = W.BY_NAME[name]
    x, dy, ref = problem(name, "int")
    xd, dyd = x.cuda(), dy.cuda()
    what, _ = describe(c)
    out = {}
    for order in ("split", "tile"):
        monkeypatch.setenv("COCLR_WGRAD_ORDER", order)
        out[order] = wgrad(c, xd, dyd)
        exact(out[order], ref, "%s, order %s" % (what, order))
    assert torch.equal(out["split"], out["tile"])


@pytest.mark.parametrize("name", IDS)
def test_randn_against_float64_and_run_to_run(name):
    c = W.BY_NAME[name]
    x, dy, ref = problem(name, "randn")
    xd, dyd = x.cuda(), dy.cuda()
    what, _ = describe(c)
    a = wgrad(c, xd, dyd)
    b = wgrad(c, xd, dyd)
    scale = ref.abs().max().item()
    err = (a.cpu().double() - ref).abs().max().item()
    print("%s: max err %.3e of scale %.3e (rel %.2e)" % (what, err, scale, err / scale))
    assert err <= RTOL * scale, "%s: max err %.3e vs scale %.3e (rel %.2e)" % (what, err, scale, err / scale)
    assert torch.equal(a, b), "%s: two runs differ" % what


# ---- several destinations ------------------------------------------------------------------------------------

MULTI_ROWS = ["w4_pw_big", "w4_pw_big_tiles", "w5_pw_small", "pw4_dma", "pw5_dma", "w1_133_pch2"]


def segmentations(Cout):
    """Row ends of 4, 3 and 2 destinations, none on a 32 / 64 / 128-row tile boundary: the issue's
    [17, 64, 65, Cout] (a one-row segment behind a tile boundary), a one-row FIRST segment, and a boundary
    inside the ragged last tile."""
    last_tile = (Cout - 1) // 64 * 64
    assert Cout % 64 != 0 and Cout > 66 and last_tile + 1 < Cout - 1
    return [[17, 64, 65, Cout], [1, 50, Cout], [Cout - 2, Cout]]


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("nseg", [4, 3, 2])
@pytest.mark.parametrize("name", MULTI_ROWS)
def test_multi_destination(name, nseg, kind):
    """coclr_conv3d_wgrad_multi (the fused 1x1x1 heads of an inception block, delivered into DDP's buckets):
    each destination is its own allocation -- unrelated addresses -- with a guard on either side that is wider
    than the whole gradient, so a row delivered with the wrong local index lands in a guard, not outside."""
    from coclr_amd import ops
    c = W.BY_NAME[name]
    x, dy, ref = problem(name, kind)
    xd, dyd = x.cuda(), dy.cuda()
    g = W.geom(c)
    taps = g.taps
    CJ = c.Cin * taps
    ends = {len(e): e for e in segmentations(c.Cout)}[nseg]
    starts = [0] + ends[:-1]
    guard = c.Cout * CJ
    what, _ = describe(c)
    single = wgrad(c, xd, dyd)
    if kind == "int":
        exact(single, ref, what)
    prior_gen = torch.Generator().manual_seed(9)
    for accumulate in (False, True):
        bufs, dsts, priors = [], [], []
        for a, b in zip(starts, ends):
            n = (b - a) * CJ
            big, mid = guarded(n, float("nan"), guard)
            if accumulate:
                pr = torch.randint(-8, 9, (n,), generator=prior_gen).float()
                mid.copy_(pr)
                priors.append(pr.view((b - a, c.Cin) + tuple(c.k)))
            bufs.append((big, n))
            dsts.append(mid.view((b - a, c.Cin) + tuple(c.k)))
        nws = g.wgrad_workspace()
        wbig, ws = guarded(nws, float("nan"))
        ops.conv_wgrad(g, xd, dyd, dsts, ws, CJ, taps, 0, accumulate)
        sync()
        assert guards_intact(wbig, nws), what
        for i, (big, n) in enumerate(bufs):
            assert guards_intact(big, n, guard), "%s: guard of destination %d of %s" % (what, i, ends)
        got = torch.cat(dsts)
        if accumulate:
            # single + prior is one fp32 addition per element, the fold's own
            assert torch.equal(got, single + torch.cat(priors).cuda()), "%s %s accumulate" % (what, ends)
            if kind == "int":
                exact(got, ref + torch.cat(priors).double(), "%s %s accumulate" % (what, ends))
        else:
            assert torch.equal(got, single), "%s: %s differs from the single-destination call" % (what, ends)
            if kind == "int":
                for i, (a, b) in enumerate(zip(starts, ends)):
                    exact(dsts[i], ref[a:b], "%s rows [%d, %d)" % (what, a, b))


# ---- stem with BatchNorm's backward applied while loading ----------------------------------------------------

@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("name", ["stem", "stem_phantom", "stem_cout72"])
def test_stem_batchnorm_form_exact(name, relu):
    """coclr_conv3d_wgrad_bn with hand-made dyadic coefficients: dy = A g + B y + D,
    g = relu ? (y * scale + shift > 0 ? dz : 0) : dz, is exact in fp32, so the kernel must equal -- bit for bit
    -- the plain kernel fed the dy formed on the host, and the float64 weight gradient of that dy."""
    from coclr_amd import ops
    c = W.BY_NAME[name]
    g = W.geom(c)
    assert g.wgrad_plan()["bn"] and g.wgrad_bn_ok()
    x, dz, _ = problem(name, "int")
    gen = torch.Generator().manual_seed(17)
    y = torch.randint(-4, 5, dz.shape, generator=gen).float()
    Cout = c.Cout
    pick = lambda vals: torch.tensor(vals)[torch.randint(0, len(vals), (Cout,), generator=gen)]
    A, B, D = pick([1.0, 2.0]), pick([0.5, -0.5]), pick([-1.0, 0.0, 1.0])
    scale, shift = pick([1.0, -1.0, 0.5]), pick([0.25, -1.25, 2.75])
    bc = lambda v: v.view(1, -1, 1, 1, 1)
    pre = y * bc(scale) + bc(shift)
    assert bool((pre != 0).all()) and bool((pre > 0).any()) and bool((pre < 0).any())
    gz = torch.where(pre > 0, dz, torch.zeros_like(dz)) if relu else dz
    dy = bc(A) * gz + bc(B) * y + bc(D)
    w = torch.zeros((Cout, c.Cin) + tuple(c.k), dtype=torch.float64, requires_grad=True)
    F.conv3d(x.double(), w, None, c.s, c.p).backward(dy.double())
    ref = w.grad

    xd = x.cuda()
    plain = wgrad(c, xd, dy.cuda())
    exact(plain, ref, "%s: plain kernel on the host-formed dy" % name)
    coef = torch.stack([A, B, D, scale, shift]).cuda()
    taps = g.taps
    nws = g.wgrad_workspace()
    wbig, ws = guarded(nws, float("nan"))
    # d(activation) as a channel slice of a wider buffer, like the engine's
    dzv = channel_slice(dz.cuda(), 2, 5)
    dw = torch.full((Cout, c.Cin) + tuple(c.k), float("nan"), device="cuda")
    ops.conv_wgrad_bn(g, xd, dzv, y.cuda(), coef, relu, dw, ws, c.Cin * taps, taps)
    sync()
    assert guards_intact(wbig, nws)
    exact(dw, ref, "%s: BatchNorm form" % name)
    assert torch.equal(dw, plain)
