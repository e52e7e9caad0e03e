"""The launches behind tests/golden/fwd_f23_randn.pt: every F(2,3) row of tests/_fwd_cases.py (variant 50) on seeded
randn data, through every epilogue of its kernel, and the F(2,3) pair route.

Shared by the recorder (tools/make_fwd_f23_golden.py, run once with the library of the commit the fixture pins) and
tests/test_gpu_fwd_f23_golden.py, which replays the same launches and compares the raw fp32 bits.  Nothing here is
rounded, summed or compared with a tolerance: on non-integer data the order of the kernel's additions and which of
its multiply-adds the compiler fuses are both visible in the last bit, which is what the fixture holds still.

replay() returns {key: fp32 CPU tensor}; keys are "<row>/<mode>/y" and "<row>/<mode>/stats" with mode one of
  plain      y = conv(x), statistics
  accum      y += conv(x) onto a randn prior, statistics of the sum
  ep_relu    y = relu((conv + bias) * ep_scale + ep_shift), statistics of conv     (ep_linear: without the ReLU)
  bwd0/bwd1  backward sums of a BatchNorm unit (conv_fwd_multi bwd_bn) with relu 0 / 1
and "pair/<row>/y", "pair/<row>/stats" for the two problems of the pair route in one conv_fwd_multi call.
"""
import torch

import _fwd_cases as W

ROWS = [c.name for c in W.CASES if c.name.startswith("w50_")]
PAIR = next(names for names, route in W.PAIRS if names == ("w50_odd_frames", "w50_cin8x"))
FIXTURE = "fwd_f23_randn.pt"


def _place(t, misalign):
    """t on the device, 16 bytes into its allocation (20 when the row is there for the 4-byte kernel)."""
    lead = 5 if misalign else 4
    flat = torch.zeros(t.numel() + lead, device="cuda")
    view = flat[lead:].view(t.shape)
    view.copy_(t.float())
    return view


def _pack(c, w):
    from coclr_amd import ops
    taps, base, step, tr, wino, full = W.pack_args(c)
    cout, cin = w.shape[:2]
    buf = torch.zeros(ops.conv_packed_size(cin, cout, taps, tr), device="cuda")
    ops.conv_pack_weights(w.float().cuda().contiguous(), buf, cout, cin, taps, cin * full, full, base,
                          int(tr) | (2 if wino else 0), step)
    return buf


def _operands(name):
    """(case, geometry, x on the device, packed weights, output shape, per-row seeded generator)."""
    c = W.BY_NAME[name]
    x, w, ref = W.problem(W.base_name(c), "randn")
    g = W.launch_geom(c)
    assert W.plan(c)["variant"] == 50 and g.lattice is None, name
    gen = torch.Generator().manual_seed(1009 + sum(map(ord, W.base_name(c))))
    return c, g, _place(x, c.misalign), _pack(c, w), tuple(ref.shape), gen


def _fresh(g, shape):
    return torch.zeros(shape, device="cuda"), torch.zeros((2, g.Cout, g.ntiles()), device="cuda")


def replay():
    from coclr_amd import ops
    out = {}

    def keep(key, y, st):
        torch.cuda.synchronize()
        out[key + "/y"] = y.cpu().clone()
        out[key + "/stats"] = st.cpu().clone()

    for name in ROWS:
        c, g, xd, wp, shape, gen = _operands(name)
        Cout = shape[1]
        rn = lambda *s: torch.randn(*s, generator=gen)     # noqa: E731

        y, st = _fresh(g, shape)
        ops.conv_fwd(g, xd, wp, y, stats=st.view(-1))
        keep(name + "/plain", y, st)

        y, st = _fresh(g, shape)
        y.copy_(rn(shape))
        ops.conv_fwd(g, xd, wp, y, stats=st.view(-1), accumulate=True)
        keep(name + "/accum", y, st)

        bias, sc, sh = rn(Cout).cuda(), rn(Cout).cuda(), rn(Cout).cuda()
        for relu in (True, False):
            y, st = _fresh(g, shape)
            ops.conv_fwd(g, xd, wp, y, stats=st.view(-1), bias=bias, ep_scale=sc, ep_shift=sh, relu=relu)
            keep(name + ("/ep_relu" if relu else "/ep_linear"), y, st)

        by = rn(shape).cuda()
        scale, shift, mean = rn(Cout).cuda(), rn(Cout).cuda(), rn(Cout).cuda()
        invstd = (rn(Cout).abs() + 0.5).cuda()
        for relu in (0, 1):
            y, st = _fresh(g, shape)
            ops.conv_fwd_multi([dict(geom=g, x=xd, w=wp, y=y, stats=st.view(-1),
                                     bwd_bn=(by, scale, shift, mean, invstd, relu))])
            keep("%s/bwd%d" % (name, relu), y, st)

    calls, kept = [], []
    for name in PAIR:
        c, g, xd, wp, shape, gen = _operands(name)
        assert W.plan(c, slot=True)["slot_filled"], name
        y, st = _fresh(g, shape)
        calls.append(dict(geom=g, x=xd, w=wp, y=y, stats=st.view(-1)))
        kept.append((name, y, st))
    ops.conv_fwd_multi(calls)
    for name, y, st in kept:
        keep("pair/" + name, y, st)
    return out
