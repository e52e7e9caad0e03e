"""Exact forward convolutions and data gradients: every row of tests/_fwd_cases.py (every kernel instantiation,
pair route and dispatch edge of coclr_amd/csrc/conv_igemm.hip's launcher, see tests/test_fwd_plan_cpu.py) against
F.conv3d in float64 (data-gradient rows: autograd's x.grad), compared with torch.equal after casting to fp32.

Exactness.  x (or dy) holds integers in [-xa, xa] (xa = 2; 1 on the rows with 32768 positions) and the weights
G * integers in [-wa, wa], G the granule of the row's form, so that every transformed operand, product, accumulator
and output is an integer (a multiple of G in the outputs) below 2^24 and fp32 holds it exactly WHATEVER the order
of summation, the chunking or the tile walk.  With C = Cin <= 72 reduction channels:

  * direct forms, G = 1: |acc| <= C * taps * xa * wa <= 72 * 49 * 4 < 2^14;
  * F(2,3) along T, G = 2: U = w0, (w0 +- w1 + w2) / 2, w2 are integers |U| <= 3 wa; D = d0 - d2, d1 + d2, d2 - d1,
    d1 - d3: |D| <= 2 xa; |m| <= C * 6 * xa * wa; the outputs add three m: < 2^13;
  * F(2x2,3x3), G = 4: U = G g G^T has entries g / 4 * {4, 2, 1}: integers |U| <= 9 wa; V = B^T d B: |V| <= 4 xa;
    |m| <= C * 36 * xa * wa, the outputs add nine: < 2^17;
  * F(2,4) and the polyphase stem form, G = 6: U rows 1/2, -1/2 sum, (.)/6 with integer numerators that are
    multiples of 6: integers |U| <= 15 wa; each (.) * fl(1/6) of a multiple of 6 below 2^20 rounds to the exact
    quotient under any contraction (one rounding of a value within 2^-24 relative of an integer); input transforms
    have integer coefficients of absolute sum <= 20: |m| <= C * 15 wa * 20 xa, outputs add <= 5 m with gains <= 8:
    < 2^22;
  * F(4,3), G = 24: U = g0/4, -(g0 +- g1 + g2)/6, g0/24 +- g1/12 + g2/6, g2: integers |U| <= 24 wa; D has integer
    coefficients of absolute sum <= 10: |m| <= C * 24 wa * 10 xa, outputs gains <= 19: < 2^23 for C <= 24 (the F(4,3)
    rows).  The DEVICE pack of U3 / U4 is (w0 * k24 + w1 * k12) + w2 * k6 with three rounded constants: exact when
    evaluated unfused or fully fused, but one fused product out of three gives 1.00000012 for 24 * (-1, -1, 1) -- a
    compiler choice -- so the F(4,3) rows take their operand from the HOST (float64 transform, exact integers, the
    documented layout) and the device pack is held to its own bound in test_pack_f43_bound.

Statistics: tests/test_fwd_plan_cpu.py asserts per row that sum |y| / G and sum y^2 / G^2 per channel stay below
2^24, so every partial is exact and the float64 sum of the [2][Cout][ntiles] partials must EQUAL the reference's.

Memory a kernel must not include holds 2^20 (finite: a masked lane that loads it and multiplies by zero is no
false alarm, a stray inclusion breaks equality); memory it must not write holds a sentinel that is compared
afterwards; memory it must write before it reads holds NaN.  Nothing here uses a tolerance on integer data.  Each
row also runs on randn data at the project's 2e-4 * max|ref| (small integers would survive a reduced-precision
matrix path; these do not), twice, bit-identically.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import _fwd_cases as W

pytestmark = pytest.mark.gpu

RTOL = 2e-4            # tests/test_gpu_kernels.py
OUTSIDE = float(2 ** 20)
GUARD = -12345.0
NAN = float("nan")
IDS = [c.name for c in W.CASES]


def sync():
    """A launch that faulted ends the session: nothing more is started on a device in that state."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a convolution launch: %s" % e, returncode=3)


def guarded(shape, fill, guard=256):
    """A tensor of `shape` holding `fill` between two guard runs; returns (whole buffer, the tensor)."""
    n = 1
    for v in shape:
        n *= v
    big = torch.full((n + 2 * guard,), GUARD, device="cuda")
    mid = big[guard:guard + n]
    mid.fill_(fill)
    return big, mid.view(shape)


def guards_intact(big, guard=256):
    return bool((big[:guard] == GUARD).all()) and bool((big[-guard:] == GUARD).all())


def exact(got, ref, what):
    got, ref = got.detach().cpu(), ref.float()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    same = (got == ref) | (got.isnan() & ref.isnan())
    if not bool(same.all()):
        idx = (~same).nonzero()[0].tolist()
        raise AssertionError("%s: %d of %d elements differ from float64; first at %s: got %r, want %r" % (
            what, int((~same).sum()), same.numel(), idx, got[tuple(idx)].item(), ref[tuple(idx)].item()))


@functools.lru_cache(maxsize=None)
def problem(name, kind="int"):
    return W.problem(W.base_name(W.BY_NAME[name]), kind)


def describe(c, **kw):
    pl = W.plan(c, **kw)
    return "%s -> %s" % (c.name, W.instantiation(pl)), pl


def place(t, misalign=False, offset=0, extra=0, tail=0, fill=OUTSIDE):
    """t (CPU) on the device as channels [offset, offset + C) of a buffer `extra` channels wider with `tail` extra
    samples, everything else -- and a run in front -- holding `fill`; the buffer starts 4 floats (16 bytes) into
    its allocation, or 5 when the row is there for a 4-byte kernel."""
    N, Cc = t.shape[:2]
    shape = (N + tail, Cc + extra) + tuple(t.shape[2:])
    numel = 1
    for v in shape:
        numel *= v
    lead = 5 if misalign else 4
    flat = torch.full((numel + lead,), fill, device="cuda")
    view = flat[lead:].view(shape)[:N, offset:offset + Cc]
    view.copy_(t.float())
    assert offset or (view.data_ptr() % 16 == 0) == (not misalign)
    return view


def pack(c, w, kind="int"):
    """The row's packed operand on the device: the device pack, except for F(4,3) on integer data (module
    docstring), whose exact operand comes from the host."""
    from coclr_amd import ops
    taps, base, step, tr, wino, full = W.pack_args(c)
    cout, cin = w.shape[:2]
    if wino and taps == 6 and kind == "int":
        host = W.host_pack(w, taps, base, step, tr, True)
        assert bool((host == host.round()).all())
        return host.float().cuda()
    buf = torch.full((ops.conv_packed_size(cin, cout, taps, tr),), NAN, device="cuda")
    ops.conv_pack_weights(w.float().cuda().contiguous(), buf, cout, cin, taps, cin * full, full, base,
                          int(tr) | (2 if wino else 0), step)
    return buf


def destination(c, fill, channels_extra=0, offset=0):
    """(whole buffer, tensor handed to the launch, dense view of the launch's outputs).  A lattice row writes its
    residue class of the full dx; everything off the lattice keeps `fill`."""
    g = W.launch_geom(c)
    full = g.odim if g.lattice is None else tuple(g.lattice[2])
    big, wide = guarded((g.N, g.Cout + channels_extra) + tuple(full), fill)
    y = wide[:, offset:offset + g.Cout]
    if g.lattice is None:
        return big, y, y
    (st, _, _), (ot, _, _) = g.lattice[0], g.lattice[1]
    return big, y, y[:, :, ot::st]


def launch(c, x, packed, y, monkeypatch, **kw):
    from coclr_amd import ops
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    ops.conv_fwd(W.launch_geom(c), x, packed, y, **kw)
    sync()


def stats_buffer(c):
    g = W.launch_geom(c)
    return guarded((2, g.Cout, g.ntiles()), NAN)


def check_stats(st, ref, what):
    got = st.double().sum(-1).cpu()
    assert torch.equal(got[0], ref.sum((0, 2, 3, 4))), "%s: sum y %s vs %s" % (what, got[0], ref.sum((0, 2, 3, 4)))
    assert torch.equal(got[1], (ref * ref).sum((0, 2, 3, 4))), "%s: sum y^2" % what


def off_lattice_keeps(c, y, out, fill):
    if y is out:
        return True
    mask = torch.ones_like(y, dtype=torch.bool)
    g = W.launch_geom(c)
    mask[:, :, g.lattice[1][0]::g.lattice[0][0]] = False
    rest = y[mask]
    return bool(rest.isnan().all()) if fill != fill else bool((rest == fill).all())


# ---- per-row tests --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", IDS)
def test_plain_write(name, monkeypatch):
    c = W.BY_NAME[name]
    x, w, ref = problem(name)
    what, pl = describe(c)
    xd = place(x, c.misalign)
    ybig, y, out = destination(c, NAN)
    sbig, st = stats_buffer(c)
    launch(c, xd, pack(c, w), y, monkeypatch, stats=st.view(-1))
    exact(out, ref, what)
    assert off_lattice_keeps(c, y, out, NAN), what
    assert guards_intact(ybig) and guards_intact(sbig), "%s: wrote outside y or stats" % what
    check_stats(st, ref, what)


@pytest.mark.parametrize("name", IDS)
def test_accumulate(name, monkeypatch):
    """Onto a prior of G * integers in [-8, 8]; the statistics are those of the accumulated tensor."""
    c = W.BY_NAME[name]
    x, w, ref = problem(name)
    what, _ = describe(c)
    prior = torch.randint(-8, 9, ref.shape, generator=torch.Generator().manual_seed(5)).double() * W.granule(c)
    ybig, y, out = destination(c, GUARD)
    out.copy_(prior.float())
    sbig, st = stats_buffer(c)
    launch(c, place(x, c.misalign), pack(c, w), y, monkeypatch, stats=st.view(-1), accumulate=True)
    exact(out, ref + prior, what)
    assert off_lattice_keeps(c, y, out, GUARD) and guards_intact(ybig) and guards_intact(sbig), what
    check_stats(st, ref + prior, what)


@pytest.mark.parametrize("name", IDS)
def test_operands_amid_poison(name, monkeypatch):
    """x is channels [3, 3 + Cin) of a buffer 5 channels wider with one tail sample, y channels [2, 2 + Cout) of one
    7 wider: both sample strides are non-dense; everything x must not read holds 2^20, everything y must not
    write a sentinel."""
    c = W.BY_NAME[name]
    x, w, ref = problem(name)
    g = W.launch_geom(c)
    xd = place(x, c.misalign, offset=3, extra=5, tail=1)
    ybig, y, out = destination(c, GUARD, channels_extra=7, offset=2)
    what, pl = describe(c, x_aligned=xd.data_ptr() % 16 == 0, y_aligned=y.data_ptr() % 8 == 0,
                        x_nstride=xd.stride(0), y_nstride=y.stride(0))
    assert W.instantiation(pl) == W.instantiation(W.plan(c)), "%s: the slices changed the kernel" % what
    y.fill_(NAN)
    sbig, st = stats_buffer(c)
    launch(c, xd, pack(c, w), y, monkeypatch, stats=st.view(-1))
    exact(out, ref, what)
    assert off_lattice_keeps(c, y, out, NAN), what
    wide = ybig[256:-256].view(g.N, g.Cout + 7, -1)
    assert bool((wide[:, :2] == GUARD).all()) and bool((wide[:, 2 + g.Cout:] == GUARD).all()), what
    assert guards_intact(ybig) and guards_intact(sbig), what
    check_stats(st, ref, what)


GATHER = [c.name for c in W.CASES if W.plan(c)["variant"] not in (41, 50, 51, 52, 60)]      # the direct kernels


@pytest.mark.parametrize("name", GATHER)
def test_gather(name, monkeypatch):
    """n_index into Nx = N + 2 samples, a permutation with one index repeated; the unselected samples hold 2^20."""
    c = W.BY_NAME[name]
    x, w, ref = problem(name)
    N = x.shape[0]
    idx = list(range(N, 0, -1))
    if N > 1:
        idx[-1] = idx[0]
    xs = torch.full((N + 2,) + tuple(x.shape[1:]), OUTSIDE, dtype=torch.float64)
    xs[1:N + 1] = x
    what, pl = describe(c, n_index=True, Nx=N + 2)
    assert W.instantiation(pl) == W.instantiation(W.plan(c))
    ybig, y, out = destination(c, NAN)
    launch(c, place(xs, c.misalign), pack(c, w), y, monkeypatch,
           n_index=torch.tensor(idx, dtype=torch.int64, device="cuda"))
    exact(out, ref[[i - 1 for i in idx]], what)
    assert guards_intact(ybig), what


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("name", IDS)
def test_epilogue(name, relu, monkeypatch):
    """y = act((conv + bias) * ep_scale + ep_shift), ep_scale from {1, 2, -1, 0.5}, integer bias and shift; the
    statistics are those of the convolution itself."""
    c = W.BY_NAME[name]
    x, w, ref = problem(name)
    what, _ = describe(c)
    gen = torch.Generator().manual_seed(23)
    Cout = ref.shape[1]
    bias = torch.randint(-3, 4, (Cout,), generator=gen).double()
    sc = torch.tensor([1.0, 2.0, -1.0, 0.5], dtype=torch.float64)[torch.randint(0, 4, (Cout,), generator=gen)]
    sh = torch.randint(-3, 4, (Cout,), generator=gen).double()
    b = lambda v: v.view(1, -1, 1, 1, 1)
    want = (ref + b(bias)) * b(sc) + b(sh)
    if relu:
        want = want.clamp_min(0)
    ybig, y, out = destination(c, NAN)
    sbig, st = stats_buffer(c)
    launch(c, place(x, c.misalign), pack(c, w), y, monkeypatch, stats=st.view(-1), bias=bias.float().cuda(),
           ep_scale=sc.float().cuda(), ep_shift=sh.float().cuda(), relu=relu)
    exact(out, want, what)
    assert guards_intact(ybig) and guards_intact(sbig), what
    check_stats(st, ref, what)


POLY7 = [c.name for c in W.CASES if W.plan(c)["variant"] == 41]


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("name", POLY7)
def test_in_affine(name, relu, monkeypatch):
    """Variant 41 applies x' = act(x * in_scale + in_shift) while it reads; padding stays zero even where
    act(in_shift) != 0."""
    from coclr_amd import ops
    c = W.BY_NAME[name]
    x, w, _ = problem(name)
    gen = torch.Generator().manual_seed(29)
    sc = torch.tensor([1.0, 2.0], dtype=torch.float64)[torch.randint(0, 2, (c.Cin,), generator=gen)]
    sh = torch.randint(-2, 4, (c.Cin,), generator=gen).double()
    assert bool((sh > 0).any())
    b = lambda v: v.view(1, -1, 1, 1, 1)
    xa = x * b(sc) + b(sh)
    if relu:
        xa = xa.clamp_min(0)
    ref = F.conv3d(xa, w, None, c.s, c.p)
    what, pl = describe(c, in_affine=True)
    assert pl["INAFF"]
    g = W.launch_geom(c)
    ybig, y, out = destination(c, NAN)
    sbig, st = stats_buffer(c)
    ops.conv_fwd_multi([dict(geom=g, x=place(x, c.misalign), w=pack(c, w), y=y, stats=st.view(-1),
                             in_affine=(sc.float().cuda(), sh.float().cuda(), relu))])
    sync()
    exact(out, ref, what)
    assert guards_intact(ybig) and guards_intact(sbig), what
    check_stats(st, ref, what)


# every row whose kernel forms the sums (ConvGeom.bwd_sums_ok), the 32768-position rows of the 128-wide tiles and
# the lattice rows of the direct temporal kernels included; tests/test_fwd_plan_cpu.py asserts per row that
# sum |g| / G and sum |g * xhat| * 2 / G stay below 2^24
BWD_SUMS = [c.name for c in W.CASES if W.plan(c)["bwd_sums_ok"]]


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("name", BWD_SUMS)
def test_backward_sums(name, relu, monkeypatch):
    """coclr_conv_call.bwd_y with dyadic coefficients: dz is the plain result bit for bit, the statistics slots
    hold exactly sum g and sum g * xhat, g = relu ? (y * scale + shift > 0 ? dz : 0) : dz, xhat = (y - mean) *
    invstd.  On a lattice row y is laid out like the destination (the full dx) and only the row's residue class
    enters the sums."""
    from coclr_amd import ops
    c = W.BY_NAME[name]
    x, w, ref = problem(name)
    what, pl = describe(c, bwd_sums=True)
    by, scale, shift, mean, invstd, gz, xhat = W.bwd_operands(W.base_name(c), relu)
    for k in c.env:
        monkeypatch.setenv(k, c.env[k])
    ybig, y, out = destination(c, NAN)
    sbig, st = stats_buffer(c)
    f = lambda v: v.float().cuda()
    byd = torch.full(tuple(y.shape), OUTSIDE, device="cuda")       # off the lattice: must not enter the sums
    g = W.launch_geom(c)
    (byd if g.lattice is None else byd[:, :, g.lattice[1][0]::g.lattice[0][0]]).copy_(by.float())
    ops.conv_fwd_multi([dict(geom=g, x=place(x, c.misalign), w=pack(c, w), y=y, stats=st.view(-1),
                             bwd_bn=(byd, f(scale), f(shift), f(mean), f(invstd), relu))])
    sync()
    exact(out, ref, what)
    assert off_lattice_keeps(c, y, out, NAN), what
    assert guards_intact(ybig) and guards_intact(sbig), what
    got = st.double().sum(-1).cpu()
    assert torch.equal(got[0], gz.sum((0, 2, 3, 4))), "%s: sum g" % what
    assert torch.equal(got[1], (gz * xhat).sum((0, 2, 3, 4))), "%s: sum g * xhat" % what


def test_engine_gathers_through_the_direct_kernel():
    """No Winograd kernel has a gather path (the launcher refuses n_index with algo >= 1), so the engine must hand
    a gathered (3,1,1) layer that would otherwise take F(2,3) / F(4,3) to the direct kernel: the unit's output on
    x[n_index] equals the unit on the gathered tensor, bit for bit (same kernel, same data), and ATen's within the
    project's tolerance."""
    from coclr_amd import engine, ops
    from coclr_amd.backbone.s3dg import BasicConv3d
    torch.manual_seed(3)
    unit = BasicConv3d(16, 24, (3, 1, 1), 1, (1, 0, 0)).cuda().eval()
    unit.conv.weight.data.normal_(0, 0.1)
    for T in (4, 16):                                  # F(2,3) and F(4,3) by the policy of conv_geom()
        assert ops.conv_geom(3, 16, 24, (T, 4, 4), (3, 1, 1), (1, 1, 1), (1, 0, 0)).algo == (2 if T == 16 else 1)
        x = torch.randn(5, 16, T, 4, 4, device="cuda")
        idx = torch.tensor([4, 0, 4], device="cuda")
        with torch.no_grad():
            got = engine.run_module(unit, x, n_index=idx)
            sync()
            want = F.relu(unit.bn(F.conv3d(x[idx], unit.conv.weight, None, 1, (1, 0, 0))))
        got = got.view() if hasattr(got, "view") and not torch.is_tensor(got) else got
        err = (got - want).abs().max().item()
        assert err <= RTOL * want.abs().max().item(), (T, err)


@pytest.mark.parametrize("name", IDS)
def test_randn_against_float64_and_run_to_run(name, monkeypatch):
    c = W.BY_NAME[name]
    x, w, ref = problem(name, "randn")
    what, _ = describe(c)
    xd, wp = place(x, c.misalign), pack(c, w, "randn")
    outs = []
    for _ in range(2):
        ybig, y, out = destination(c, NAN)
        launch(c, xd, wp, y, monkeypatch)
        outs.append(out.clone())
    scale = ref.abs().max().item()
    err = (outs[0].cpu().double() - ref).abs().max().item()
    print("%s: max err %.3e of scale %.3e (rel %.2e)" % (what, err, scale, err / scale))
    assert err <= RTOL * scale, "%s: max err %.3e vs scale %.3e (rel %.2e)" % (what, err, scale, err / scale)
    assert torch.equal(outs[0], outs[1]), "%s: two runs differ" % what


# ---- phases of the strided temporal stem conv's data gradient --------------------------------------------------

@pytest.mark.parametrize("wino", [True, False], ids=["winograd_phases", "direct_phases"])
@pytest.mark.parametrize("T", [8, 9, 32, 34, 37])
def test_phases_cover_dx(T, wino, monkeypatch):
    """Every phase of dgrad_phases() writes through its lattice into ONE NaN-filled dx: no NaN is left, the result
    equals float64, a second accumulate pass doubles it."""
    from coclr_amd import ops
    monkeypatch.setattr(ops, "WINOGRAD_PHASES", wino)
    N, Cin, Cout, dims, k, s, p = 2, 24, 20, (T, 2, 4), (7, 1, 1), (2, 1, 1), (3, 0, 0)
    gen = torch.Generator().manual_seed(T)
    x = torch.zeros((N, Cin) + dims, dtype=torch.float64, requires_grad=True)
    w = torch.randint(-2, 3, (Cout, Cin) + k, generator=gen).double() * 24
    yr = F.conv3d(x, w, None, s, p)
    dy = torch.randint(-2, 3, yr.shape, generator=gen).double()
    yr.backward(dy)
    g = ops.ConvGeom(N, Cin, Cout, dims, k, s, p)
    phases = g.dgrad_phases()
    assert phases is not None and sorted(nk for _, _, nk, _ in phases) == [3, 4]
    for pg, _, nk, _ in phases:
        assert pg.algo == (2 if (wino and pg.odim[0] >= 16 and pg.odim[0] == pg.idim[0]) else 0), (nk, pg)
    big, dx = guarded((N, Cin) + dims, NAN)
    dyd, wd = dy.float().cuda(), w.float().cuda().contiguous()
    ops_ = []
    for pg, k0, nk, step in phases:
        if pg.algo == 2 and nk == 3:
            wp = W.host_pack(w, 6, k0, step, True, True).float().cuda()
        else:
            taps = {3: 6, 4: 5}[nk] if pg.algo == 2 else nk
            wp = torch.full((ops.conv_packed_size(Cin, Cout, taps, True),), NAN, device="cuda")
            ops.conv_pack_weights(wd, wp, Cout, Cin, taps, Cin * 7, 7, k0, 1 | (2 if pg.algo else 0), step)
        ops_.append((pg, wp))
    for pg, wp in ops_:
        ops.conv_fwd(pg, dyd, wp, dx)
        sync()
    assert not bool(dx.isnan().any()), "T=%d: a phase left part of dx unwritten" % T
    exact(dx, x.grad, "phases T=%d" % T)
    for pg, wp in ops_:
        ops.conv_fwd(pg, dyd, wp, dx, accumulate=True)
        sync()
    exact(dx, 2 * x.grad, "phases T=%d, accumulate" % T)
    assert guards_intact(big)


# ---- pair routes of coclr_conv3d_fwd_multi ------------------------------------------------------------------------

@pytest.mark.parametrize("names,route", W.PAIRS, ids=["+".join(n) for n, r in W.PAIRS])
def test_pairs(names, route, monkeypatch):
    """Outputs and statistics of one multi call are torch.equal to the single launches' and to float64."""
    from coclr_amd import ops
    calls, singles = [], []
    for n in names:
        c = W.BY_NAME[n]
        x, w, ref = problem(n)
        xd, wp = place(x, c.misalign), pack(c, w)
        ybig, y, out = destination(c, NAN)
        sbig, st = stats_buffer(c)
        calls.append(dict(geom=W.launch_geom(c), x=xd, w=wp, y=y, stats=st.view(-1)))
        y1big, y1, out1 = destination(c, NAN)
        s1big, st1 = stats_buffer(c)
        launch(c, xd, wp, y1, monkeypatch, stats=st1.view(-1))
        singles.append((n, ref, ybig, sbig, out, st, out1, st1))
    ops.conv_fwd_multi(calls)
    sync()
    for n, ref, ybig, sbig, out, st, out1, st1 in singles:
        what = "%s in %s (%s)" % (n, "+".join(names), route)
        exact(out, ref, what)
        assert torch.equal(out, out1) and torch.equal(st, st1), what
        assert guards_intact(ybig) and guards_intact(sbig), what
        check_stats(st, ref, what)


# ---- the device pack ------------------------------------------------------------------------------------------------

PACKS = [
    # (name, cout, cin, stencil taps of the parameter, taps, tap_base, tap_step, transpose, wino, granule)
    ("direct_fwd", 20, 12, 9, 9, 0, 1, False, False, 1),
    ("direct_dgrad", 20, 12, 9, 9, 0, 1, True, False, 1),
    ("direct_kt_slice", 20, 3, 245, 49, 147, 1, False, False, 1),
    ("direct_phase_subset_dgrad", 20, 12, 7, 4, 0, 2, True, False, 1),
    ("direct_phase_subset_odd_dgrad", 20, 12, 7, 3, 1, 2, True, False, 1),
    ("f23_fwd", 20, 36, 3, 4, 0, 1, False, True, 2),
    ("f23_dgrad", 20, 36, 3, 4, 0, 1, True, True, 2),
    ("f24_fwd", 20, 36, 4, 5, 0, 1, False, True, 6),
    ("f24_phase_dgrad", 20, 36, 7, 5, 0, 2, True, True, 6),
    ("poly7_fwd", 20, 36, 7, 9, 0, 1, False, True, 6),
    ("f2x2_fwd", 20, 36, 9, 16, 0, 1, False, True, 4),
    ("f2x2_dgrad", 136, 20, 9, 16, 0, 1, True, True, 4),
]


def _pack_case(cout, cin, full, G, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, (cout, cin, full), generator=gen).double() * G


@pytest.mark.parametrize("case", PACKS, ids=[p[0] for p in PACKS])
def test_pack_exact(case):
    """The device-packed operand of every dyadic form, and of F(2,4) / the stem form on multiples of 6, IS the
    float64 transform in the documented layout -- the bank rotation of the 16-matrix form and the zeros of every
    padding row and column of a stand-alone operand included (the buffer starts as NaN)."""
    from coclr_amd import ops
    name, cout, cin, full, taps, base, step, tr, wino, G = case
    w = _pack_case(cout, cin, full, G, len(name))
    n = ops.conv_packed_size(cin, cout, taps, tr)
    big, buf = guarded((n,), NAN)
    ops.conv_pack_weights(w.float().cuda(), buf, cout, cin, taps, cin * full, full, base,
                          int(tr) | (2 if wino else 0), step)
    sync()
    want = W.host_pack(w, taps, base, step, tr, wino)
    assert want.numel() == n
    exact(buf, want, name)
    assert guards_intact(big)


@pytest.mark.parametrize("tr", [False, True], ids=["fwd", "dgrad"])
def test_pack_placed_sub_block(tr):
    """A sub-block at (row0, col0) inside a wider pre-zeroed operand: only its rows x cols are written."""
    from coclr_amd import ops
    cout, cin, full = 20, 12, 3
    w = _pack_case(cout, cin, full, 1, 77)
    rows_total, cols_total = (40, 140) if not tr else (140, 40)
    row0, col0 = (8, 100) if not tr else (100, 8)
    RP, CP = -(-rows_total // 32) * 32, -(-cols_total // 128) * 128
    big, buf = guarded((full * RP * CP,), GUARD)
    ops.conv_pack_weights(w.float().cuda(), buf, cout, cin, full, cin * full, full, 0, int(tr), 1,
                          row0, rows_total, col0, cols_total)
    sync()
    want = W.host_pack(w, full, 0, 1, tr, False, row0, rows_total, col0, cols_total,
                       into=torch.full((full * RP * CP,), GUARD, dtype=torch.float64))
    exact(buf, want, "placed %s" % ("dgrad" if tr else "fwd"))
    assert guards_intact(big)


@pytest.mark.parametrize("case", [("f43_fwd", 20, 36, 3, 6, 0, 1, False), ("f43_dgrad", 20, 36, 3, 6, 0, 1, True),
                                  ("f43_phase_dgrad", 20, 36, 7, 6, 1, 2, True)], ids=lambda c: c[0])
@pytest.mark.parametrize("kind", ["x24", "randn"])
def test_pack_f43_bound(case, kind):
    """F(4,3): U3 / U4 = (g0 * k24 +- g1 * k12) + g2 * k6 are three constants rounded to fp32 (relative error
    u = 2^-24 each), three products and two sums (u each, or none where the compiler fuses).  Every g_i reaches
    the result through at most four roundings (its constant, its product, two sums), so with
    a = |g0| / 24 + |g1| / 12 + |g2| / 6 the result is within a * ((1 + u)^4 - 1) < 4.0001 u a ~ 2^-22 * a of the
    float64 transform of the fp32 weights.  U1 / U2 = -((g0 +- g1) + g2) * k6: two sums, the constant, the
    product: 4.0001 u * (|g0| + |g1| + |g2|) / 6.  U0 = g0 / 4 and U5 = g2 are exact."""
    from coclr_amd import ops
    name, cout, cin, full, taps, base, step, tr = case
    gen = torch.Generator().manual_seed(41)
    w = _pack_case(cout, cin, full, 24, 43) if kind == "x24" else \
        torch.randn((cout, cin, full), generator=gen).float().double()
    n = ops.conv_packed_size(cin, cout, taps, tr)
    big, buf = guarded((n,), NAN)
    ops.conv_pack_weights(w.float().cuda(), buf, cout, cin, taps, cin * full, full, base, int(tr) | 2, step)
    sync()
    assert guards_intact(big)
    want = W.host_pack(w, taps, base, step, tr, True)
    g = w.abs()[:, :, base:base + 2 * step + 1:step]
    if tr:
        g = g.flip(-1)
    a = torch.stack([g[..., 0] / 4, g.sum(-1) / 6, g.sum(-1) / 6, g[..., 0] / 24 + g[..., 1] / 12 + g[..., 2] / 6,
                     g[..., 0] / 24 + g[..., 1] / 12 + g[..., 2] / 6, g[..., 2]])
    a = a if tr else a.permute(0, 2, 1)          # [matrix][r][c]
    got = buf.double().cpu().view(6, want.numel() // 6)
    RP, CP = -(-a.shape[1] // 32) * 32, -(-a.shape[2] // 128) * 128
    bound = torch.zeros(6, RP, CP, dtype=torch.float64)
    u = 2.0 ** -24
    gains = torch.tensor([0.0, 4.0001, 4.0001, 4.0001, 4.0001, 0.0], dtype=torch.float64) * u
    bound[:, :a.shape[1], :a.shape[2]] = a * gains.view(6, 1, 1)
    err = (got - want.view(6, -1)).abs().view(6, RP, CP)
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print("%s %s: worst error / bound = %.3f" % (name, kind, worst))
    assert bool((err <= bound).all()), "%s: worst error / bound = %.3f" % (name, worst)
