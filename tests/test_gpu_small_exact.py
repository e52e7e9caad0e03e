"""Exact optimiser, global average pool and self-gating kernels: every row of tests/_small_cases.py (every launcher
branch of coclr_amd/csrc/optim.hip's Adam and momentum kernels, pool.hip's global average pool and nce.hip's sigmoid /
plane_scale / plane_dot, see tests/test_small_cases_cpu.py) through the C ABI (coclr_amd.ops) with pointer tables built
by hand, against the float64 references of tests/_small_cases.py.

  * momentum update, Adam's exact rows, average pool, plane_scale, plane_dot, sigmoid backward: bit for bit.
  * Adam on random data: ten steps against the float64 recurrence; the kernel's error may be at most twice that of
    torch's own torch.optim.Adam run on the same device from the same inputs.
  * sigmoid: NaN, +-inf and the underflow range by value; everything else in ulps against float64, at most 2 more than
    torch.sigmoid's own on the same device.

Memory a kernel must not read holds 2^20; memory it must not write holds a sentinel that is compared after every launch;
memory it must write first holds NaN.  Every launch is followed by _exact.sync(): a fault ends the session."""
import pytest
import torch

import _small_cases as S
from _exact import NAN, Placed, Placed2D, exact, source, source2d, sync

pytestmark = pytest.mark.gpu


def ops():
    from coclr_amd import ops as o
    return o


def ids(table):
    return [c.name for c in table]


def intact(*placed):
    for p in placed:
        assert p.untouched_around(), "a guard region was written"


def flat(count, shift, fill=NAN):
    """A written 1-D operand `shift` floats past a 16-byte boundary, between guards."""
    p = Placed2D(1, count, shift=shift, fill=fill)
    assert p.view.data_ptr() % 16 == 4 * (shift % 4)
    return p


def readonly(t, shift=0):
    """A read-only 1-D operand `shift` floats past a 16-byte boundary; around it 2^20."""
    v = source2d(t.reshape(1, -1), shift=shift)[0]
    assert v.data_ptr() % 16 == 4 * (shift % 4)
    return v


def unchanged(view, t, what):
    exact(view, t.reshape(view.shape), what + " (a read-only operand)")


# ---- coclr_momentum_update ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", S.MOMENTUM, ids=ids(S.MOMENTUM))
def test_momentum_update(c):
    data = S.momentum_inputs(c)
    rows, dsts, srcs = [], [], []
    for t, (d, s) in zip(c.tensors, data):
        dst = flat(t.count, t.dst_shift)
        dst.put(d.reshape(1, -1))
        src = readonly(s, t.src_shift)
        for off, cnt in S.chunks(t.count):
            rows.append((dst.view.data_ptr() + 4 * off, src.data_ptr() + 4 * off, cnt))
        dsts.append(dst)
        srcs.append(src)
    table = torch.tensor(rows, dtype=torch.int64).cuda()
    ops().momentum_update(table, len(rows), float(c.m), float(1. - c.m))
    sync("momentum_update " + c.name)
    for i, (dst, src, (d, s)) in enumerate(zip(dsts, srcs, data)):
        exact(dst.view[0], S.momentum_cpu32(d, s, c.m), "momentum %s tensor %d" % (c.name, i))
        unchanged(src, s, "src")
        intact(dst)


# ---- coclr_adam_step ---------------------------------------------------------------------------------------------------

def adam_table(params):
    """params: [(count, slot, (p, g, m, v, k or None) device views)] -> the int64[rows][8] launch table."""
    rows = []
    for count, slot, (p, g, m, v, k) in params:
        for off, cnt in S.chunks(count):
            rows.append((p.data_ptr() + 4 * off, g.data_ptr() + 4 * off, m.data_ptr() + 4 * off, v.data_ptr() + 4 * off,
                         0 if k is None else k.data_ptr() + 4 * off, cnt, slot, 0))
    return torch.tensor(rows, dtype=torch.int64).cuda()


def hyper_table(nslots, named):
    """double[nslots][8]; rows no parameter names hold NaN."""
    h = torch.full((nslots, 8), NAN, dtype=torch.float64)
    for slot, vals in named.items():
        h[slot] = 0
        h[slot, :5] = torch.tensor(vals, dtype=torch.float64)
    return h.cuda()


@pytest.mark.parametrize("c", S.ADAM, ids=ids(S.ADAM))
def test_adam_exact_rows(c):
    """One step from zero state on data for which every intermediate is an fp32 value: p - lr * sign(g'), g' / 2 and
    g'^2 / 4 bit for bit, the folded key update, the step counters of the named slots and of nobody else."""
    held, params, named = [], [], {}
    for i, p_ in enumerate(c.params):
        p, g, k = S.adam_exact_inputs(c, i)
        P, M, V = flat(p_.count, p_.shifts[0]), flat(p_.count, p_.shifts[2], fill=0.0), flat(p_.count, p_.shifts[3], fill=0.0)
        P.put(p.reshape(1, -1))
        G = readonly(g, p_.shifts[1])
        K = None
        if p_.key:
            K = flat(p_.count, p_.shifts[4])
            K.put(k.reshape(1, -1))
        params.append((p_.count, p_.slot, (P.view[0], G, M.view[0], V.view[0], None if K is None else K.view[0])))
        named[p_.slot] = (S.lr_of(p_.slot),) + S.EXACT_BETAS + (S.EXACT_EPS, p_.wd)
        held.append((P, G, M, V, K, (p, g, k)))
    outside = S.outside_slots(c)
    steps0 = torch.zeros(c.nslots, dtype=torch.float64)
    for s in outside:
        steps0[s] = S.outside_step(s)
    steps = flat(c.nslots, 0)
    steps.put(steps0.reshape(1, -1))
    groups = readonly(torch.tensor(sorted(named), dtype=torch.int32))
    table = adam_table(params)
    ops().adam_step(table, table.shape[0], hyper_table(c.nslots, named), steps.view, groups, len(named),
                    S.FOLD_M, 1.0 - S.FOLD_M)
    sync("adam_step " + c.name)
    want = steps0.clone()
    want[sorted(named)] += 1.0
    exact(steps.view[0], want, "step counters of " + c.name)
    intact(steps)
    for i, (P, G, M, V, K, (p, g, k)) in enumerate(held):
        pn, m, v, kn = S.adam_exact_expected(c, i, p, g, k)
        what = "%s parameter %d " % (c.name, i)
        exact(P.view[0], pn, what + "p")
        exact(M.view[0], m, what + "exp_avg")
        exact(V.view[0], v, what + "exp_avg_sq")
        unchanged(G, g, what + "grad")
        if K is not None:
            exact(K.view[0], S.momentum_cpu32(k, pn, S.FOLD_M), what + "key")
            intact(K)
        intact(P, M, V)


KINDS = (("p", 0, 0), ("exp_avg", 2, 1), ("exp_avg_sq", 3, 2))       # name, place in (P, G, M, V), place in (p, m, v)


@pytest.mark.parametrize("c", S.BOUNDED, ids=ids(S.BOUNDED))
def test_adam_bounded_rows(c):
    """Ten steps of random data (an lr change at step 5, one parameter starting at step counter 7 with state, one whose
    gradient is a view one float into a flat buffer) against the float64 recurrence.  torch's own Adam (the foreach
    path) runs on the same device from the same inputs; for each of p, exp_avg and exp_avg_sq the kernel's largest
    error relative to the tensor's maximum (the larger of the two parameters') must be at most twice torch's.

    Measured on an MI355X (kernel / torch, relative to the tensor maximum; docs/history.md, "Later test notes"):
        default    p 1.657e-07 / 1.657e-07   exp_avg 9.490e-08 / 9.366e-08   exp_avg_sq 1.880e-07 / 1.925e-07
        no-decay   p 1.700e-07 / 1.700e-07   exp_avg 1.106e-07 / 8.507e-08   exp_avg_sq 1.493e-07 / 1.528e-07
        large      p 1.624e-07 / 1.624e-07   exp_avg 1.015e-07 / 9.242e-08   exp_avg_sq 1.519e-07 / 2.171e-07
    Elements that differ bitwise between kernel and torch after the first step are printed, not asserted (of 32 776:
    p 82 / 74 / 1764, exp_avg 8 / 3 / 2767, exp_avg_sq 11 289 / 11 140 / 13 530): torch's ROCm kernels contract
    multiply-adds that this kernel rounds twice, so the two are not the same "operation for operation"."""
    from coclr_amd import optim as O
    inputs, ref = S.bounded_inputs(c), S.bounded_reference(c)
    # kernel side
    held, params = [], []
    steps = flat(len(S.BOUNDED_PARAMS), 0)
    steps.put(torch.tensor([[float(bp.start_step) for bp in S.BOUNDED_PARAMS]]))
    for i, (bp, (p0, m0, v0, grads)) in enumerate(zip(S.BOUNDED_PARAMS, inputs)):
        P, M, V = (flat(bp.count, bp.shifts[j]) for j in (0, 2, 3))
        for dst, t in ((P, p0), (M, m0), (V, v0)):
            dst.put(t.reshape(1, -1))
        G = readonly(grads[0], bp.shifts[1])
        params.append((bp.count, i, (P.view[0], G, M.view[0], V.view[0], None)))
        held.append((P, G, M, V))
    table = adam_table(params)
    groups = readonly(torch.arange(len(params), dtype=torch.int32))
    # torch side: per-tensor groups, gradients at the same offsets inside flat buffers
    tp = [p0.cuda().requires_grad_(True) for p0, _, _, _ in inputs]
    tflat = [torch.zeros(bp.count + 4, device="cuda") for bp in S.BOUNDED_PARAMS]
    topt = O._TorchAdam([{"params": p} for p in tp], lr=c.lr, betas=c.betas, eps=c.eps, weight_decay=c.wd)
    for p, bp, (_, m0, v0, _) in zip(tp, S.BOUNDED_PARAMS, inputs):
        if bp.start_step:
            topt.state[p] = {"step": torch.tensor(float(bp.start_step)), "exp_avg": m0.cuda(), "exp_avg_sq": v0.cuda()}
    for step in range(S.BOUNDED_STEPS):
        lr = S.bounded_lr(c, step)
        hyper = hyper_table(len(params), {i: (lr,) + c.betas + (c.eps, c.wd) for i in range(len(params))})
        for grp in topt.param_groups:
            grp["lr"] = lr
        for (P, G, M, V), p, fl, bp, (_, _, _, grads) in zip(held, tp, tflat, S.BOUNDED_PARAMS, inputs):
            G.copy_(grads[step])
            p.grad = fl[bp.shifts[1]:bp.shifts[1] + bp.count]
            p.grad.copy_(grads[step])
        ops().adam_step(table, table.shape[0], hyper, steps.view, groups, len(params), 0.0, 0.0)
        sync("adam_step %s step %d" % (c.name, step))
        topt.step()
        if step == 0:
            for kind, j, _ in KINDS:
                diff = total = 0
                for h, p in zip(held, tp):
                    other = p.detach() if kind == "p" else topt.state[p][kind]
                    diff += int((h[j].view[0] != other).sum())
                    total += other.numel()
                print("adam %s: %s differs bitwise from torch in %d of %d elements after the first step (wd %g)" % (
                    c.name, kind, diff, total, c.wd))
    exact(steps.view[0], torch.tensor([float(bp.start_step + S.BOUNDED_STEPS) for bp in S.BOUNDED_PARAMS]), "step counters")
    for p, bp in zip(tp, S.BOUNDED_PARAMS):
        assert float(topt.state[p]["step"]) == bp.start_step + S.BOUNDED_STEPS
    failures = []
    for kind, j, r in KINDS:
        ek = max(S.relative_error(h[j].view[0], traj[-1][r]) for h, traj in zip(held, ref))
        et = max(S.relative_error(p.detach() if kind == "p" else topt.state[p][kind], traj[-1][r])
                 for p, traj in zip(tp, ref))
        print("adam %s: %s error vs float64 after %d steps: kernel %.3e, torch %.3e" % (c.name, kind, S.BOUNDED_STEPS, ek, et))
        assert et > 0
        if ek > 2 * et:
            failures.append("%s: kernel %.3e > 2 x torch %.3e" % (kind, ek, et))
    for (P, G, M, V), (_, _, _, grads) in zip(held, inputs):
        unchanged(G, grads[-1].double(), "grad")
        intact(P, M, V)
    intact(steps)
    assert not failures, failures


# ---- coclr_global_avgpool_fwd / _bwd -----------------------------------------------------------------------------------

@pytest.mark.parametrize("c", S.POOL_FWD, ids=ids(S.POOL_FWD))
def test_global_avgpool_fwd(c):
    x = S.pool_fwd_inputs(c)
    xd = source(x)
    y = Placed((1, c.planes, 1, 1, 1))
    ops().global_avgpool_fwd(xd, y.view)
    sync("global_avgpool_fwd " + c.name)
    if c.random:
        # an fp32 sum of S terms in any order is within S * 2^-24 * sum|x| of the true one (the last of the S roundings
        # is the division's): for the mean, 2^-24 * sum|x|
        err = (y.view.cpu().double() - x.mean((2, 3, 4), keepdim=True)).abs()
        bound = 2.0 ** -24 * x.abs().sum((2, 3, 4), keepdim=True)
        print("avgpool %s: largest error / bound %.2e" % (c.name, float((err / bound).max())))
        assert bool((err <= bound).all())
    else:
        exact(y.view, S.pool_fwd_reference(x), "global_avgpool_fwd " + c.name)
    unchanged(xd, x, "x")
    intact(y)


@pytest.mark.parametrize("c", S.POOL_BWD, ids=ids(S.POOL_BWD))
def test_global_avgpool_bwd(c):
    dy = S.pool_bwd_inputs(c)
    dyd = source(dy)
    dx = Placed((1, c.planes, 1, 1, c.S))
    ops().global_avgpool_bwd(dyd, dx.view)
    sync("global_avgpool_bwd " + c.name)
    exact(dx.view, S.pool_bwd_reference(dy, c.S), "global_avgpool_bwd " + c.name)
    intact(dx)


# ---- coclr_plane_scale / coclr_plane_dot -------------------------------------------------------------------------------

def sliced(flag):
    return S.SLICE if flag else {}


@pytest.mark.parametrize("c", S.PLANES, ids=ids(S.PLANES))
def test_plane_scale(c):
    a, gain, bias, out0 = S.plane_scale_inputs(c)
    for v in S.SCALE_VARIANTS:
        ad = source(a, **sliced(v.a_slice))
        out = Placed(tuple(a.shape), **sliced(v.out_slice))
        if v.accumulate:
            out.put(out0)
        ops().plane_scale(ad, source(gain), source(bias) if v.bias else None, out.view, accumulate=v.accumulate)
        what = "plane_scale %s %s" % (c.name, v)
        sync(what)
        exact(out.view, S.plane_scale_reference(a, gain, bias, out0, v), what)
        unchanged(ad, a, "a")
        intact(out)


@pytest.mark.parametrize("c", S.PLANES, ids=ids(S.PLANES))
def test_plane_dot(c):
    a, b = S.plane_dot_inputs(c)
    for v in S.DOT_VARIANTS:
        out = Placed((c.N, c.C))
        ops().plane_dot(source(a, **sliced(v.a_slice)), source(b, **sliced(v.b_slice)), out.view)
        what = "plane_dot %s %s" % (c.name, v)
        sync(what)
        exact(out.view, S.plane_dot_reference(a, b), what)
        intact(out)


# ---- coclr_sigmoid_fwd / _bwd ------------------------------------------------------------------------------------------

def run_sigmoid(n):
    s = S.sigmoid_args(n)
    sd = readonly(s)
    w = flat(n, 0)
    ops().sigmoid_fwd(sd, w.view)
    sync("sigmoid_fwd n=%d" % n)
    got = w.view[0].clone()
    unchanged(sd, s, "s")
    intact(w)
    return s, sd, got


@pytest.mark.parametrize("n", S.SIGMOID_N)
def test_sigmoid_fwd(n):
    """NaN gives NaN, +inf exactly 1, -inf and every argument whose true value is below the smallest normal a value in
    [0, 2^-126]; everything else within (torch.sigmoid's own largest ulp error on the same inputs) + 2 of float64: the
    kernel is one expf, one add and one divide, each within 1 ulp.

    Measured on an MI355X (largest ulp error, kernel / torch.sigmoid): n = 1: 0 / 0; 255: 1.374 / 1.374; 256: 1.675 /
    1.675; 257: 1.744 / 1.744; 70 000: 2.301 / 2.301; 524 545: 2.375 / 2.375."""
    s, sd, got = run_sigmoid(n)
    theirs = torch.sigmoid(sd).cpu().double()
    got = got.cpu().double()
    nan, one, tiny, rest = S.sigmoid_classes(s)
    assert bool((got[nan] != got[nan]).all()), "NaN"
    assert bool((got[one] == 1.0).all()), "+inf"
    assert bool(((got[tiny] >= 0) & (got[tiny] <= S.TINY)).all()), ("underflow range", got[tiny])
    ref = S.sigmoid_reference(s[rest])
    mine, torchs = float(S.ulp_error(got[rest], ref).max()), float(S.ulp_error(theirs[rest], ref).max())
    print("sigmoid n=%d: largest ulp error vs float64: kernel %.3f, torch.sigmoid %.3f" % (n, mine, torchs))
    assert mine <= torchs + 2


@pytest.mark.parametrize("n", S.SIGMOID_N)
def test_sigmoid_bwd(n):
    _, _, w = run_sigmoid(n)
    w = w.cpu().double()
    dw = S.sigmoid_bwd_inputs(n)
    wd, dwd = readonly(w), readonly(dw)
    ds = flat(n, 0)
    ops().sigmoid_bwd(dwd, wd, ds.view)
    sync("sigmoid_bwd n=%d" % n)
    exact(ds.view[0], S.sigmoid_bwd_reference(dw, w), "sigmoid_bwd n=%d" % n)
    unchanged(wd, w, "w")
    intact(ds)
