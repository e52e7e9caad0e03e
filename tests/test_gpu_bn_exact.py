"""Exact BatchNorm: every row of tests/_bn_cases.py (every route, vector width and dispatch edge of
coclr_amd/csrc/bn.hip's launchers, see tests/test_bn_plan_cpu.py) against float64, with every fp32 operation whose
fusion is the compiler's choice made exact, so the result is determined and compared with torch.equal.

  * finalize / forward: the statistics are an input, independent of y.  Per channel the partials are integers with
    sum = m * count and sumsq = count * (m^2 + 4^k); eps = 3 * 4^k is passed as the argument, momentum is 0.5,
    gamma = +-2^j, beta and the running statistics are integers.  Then var = 4^k, invstd = 2^-(k+1), scale, shift,
    the running mean and z for integer y are exact; the unbiased variance follows the kernel's double expression
    var * count / (count - 1), rounded once to fp32, and the running variance is one more rounding.
  * backward, every route: integer dz in [-3, 3] and y in [-4, 4]; scale = +-2^j, integer shift, mean in
    {0, +-1, +-2, +-4}, invstd = 2^-i given as coefficients.  Elements with y * scale + shift == 0 are present (their
    gradient must be 0).  dgamma / dbeta are exact dyadics; dy is the float64 reference with fp32 roundings at the
    determined points (tests/_exact.py: bn_backward_reference); coef[5][C] of the _coeffs entry point equals the
    same values.
  * every row also runs on randn data at the tolerances of tests/test_gpu_kernels.py (2e-4 forward, 5e-4 backward,
    times max|ref|), twice, bit-identically: small integers alone would pass a reduced-precision path.
  * the non-temporal switch COCLR_BN_NT_MB is read once per process and defaults to 0 (every vector pass
    non-temporal): one test starts a fresh child process with -1 that runs the vector rows and saves its outputs;
    the parent asserts they are bit-identical to its own.  Apart from the apply pass behind partial sums, which is
    always temporal (the from-partials rows), that is the only cover the temporal instantiations have.  A child that
    faults, aborts or hangs ends the session like any other launch here.

Memory a kernel must not read holds 2^20; memory it must not write holds a sentinel that is compared afterwards;
memory it must write first holds NaN.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

import _bn_cases as B
from _exact import NAN, Placed, bn_backward_reference, close, exact, f32, per_channel, source, sync, vector

pytestmark = pytest.mark.gpu

IDS = [c.name for c in B.CASES]
MOMENTUM = 0.5


def shape(c):
    return (c.N, c.C) + c.dims


def place(c, op, t):
    return source(t, int(op in c.extra), int(op in c.pad))


def dest(c, op, fill=NAN):
    return Placed(shape(c), int(op in c.extra), int(op in c.pad), fill=fill)


def signs(C_):
    return torch.where(torch.arange(C_) % 3 == 1, -1.0, 1.0).double()


@functools.lru_cache(maxsize=None)
def unit(name, kind, seed=0):
    """The backward's inputs of a row, float64 holding fp32 values."""
    c = B.BY_NAME[name]
    gen = torch.Generator().manual_seed(1000 * seed + len(name) * 17 + c.C)
    ch = torch.arange(c.C)
    if kind == "int":
        y = torch.randint(-4, 5, shape(c), generator=gen).double()
        dz = torch.randint(-3, 4, shape(c), generator=gen).double()
        res = torch.randint(-2, 3, shape(c), generator=gen).double()
        scale = signs(c.C) * 2.0 ** ((ch % 4) - 2).double()
        shift = ((ch * 5 + seed) % 7 - 3).double()
        mean = torch.tensor([0.0, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0])[(ch + seed) % 7].double()
        invstd = 2.0 ** (-(ch % 3).double())
    else:
        y = (torch.randn(shape(c), generator=gen) * 1.5 + 0.3).double()
        dz = torch.randn(shape(c), generator=gen).double()
        res = torch.randn(shape(c), generator=gen).double()
        scale = signs(c.C) * (torch.rand(c.C, generator=gen) + 0.5).double()
        shift = (torch.randn(c.C, generator=gen) * 0.2).double()
        mean = (torch.randn(c.C, generator=gen) * 0.3).double()
        invstd = (torch.rand(c.C, generator=gen) + 0.5).double()
    return dict(y=y, dz=dz, res=res, scale=scale, shift=shift, mean=mean, invstd=invstd)


def masked(u, relu, z=None):
    """The gradient the BatchNorm sees: dz where the activation let it through (strictly positive), float64."""
    if not relu:
        return u["dz"]
    act = z if z is not None else f32(u["y"] * per_channel(u["scale"]) + per_channel(u["shift"]))
    return u["dz"] * (act > 0)


def zs(u):
    """The z of a residual unit: relu(y * scale + shift + res), fp32 values."""
    return torch.relu(f32(f32(u["y"] * per_channel(u["scale"]) + per_channel(u["shift"])) + u["res"]))


# ---- forward ----------------------------------------------------------------------------------------------------------

def stats_exact(C_, ntiles, count, k, seed=0):
    """[2][C][ntiles] partials (integers; multiples of 1/4 where count * 4^k is no integer) with sum = m * count and
    sumsq = count * (m^2 + 4^k), every one an fp32 value; returns (stats, m)."""
    gen = torch.Generator().manual_seed(31 * ntiles + C_ + seed)
    m = ((torch.arange(C_) + seed) % 5 - 2).double()
    tot = torch.stack([m * count, count * (m * m + 4.0 ** k)])
    part = torch.randint(-50, 51, (2, C_, ntiles), generator=gen).double()
    part[:, :, 0] += tot - part.sum(-1)
    assert bool((part.float().double() == part).all()) and bool((part.sum(-1) == tot).all())
    return part, m


def bn_params(C_, seed=0):
    ch = torch.arange(C_)
    gamma = signs(C_) * 2.0 ** ((ch + seed) % 3).double()
    beta = ((ch * 3 + seed) % 5 - 2).double()
    rm = ((ch + seed) % 4 - 1).double()
    rv = ((ch * 2 + seed) % 6 + 1).double()
    return gamma, beta, rm, rv


def finalize_reference(m, k, count, gamma, beta, rm, rv):
    var = 4.0 ** k
    invstd = torch.full_like(m, 2.0 ** -(k + 1))
    scale = gamma * invstd
    shift = beta - m * scale
    unbiased = float(torch.tensor(var * count / (count - 1.0)).float())       # the kernel's double expression
    new_rm = (1 - MOMENTUM) * rm + MOMENTUM * m
    new_rv = f32((1 - MOMENTUM) * rv + MOMENTUM * unbiased)
    return m, invstd, scale, shift, new_rm, new_rv


class FwdBuffers:
    def __init__(self, C_, stats, gamma, beta, rm, rv):
        self.stats = source(stats.reshape(1, -1)).view(-1)
        self.gamma, self.beta = vector(gamma), vector(beta)
        self.run = Placed((2, C_), 0, 0)
        self.run.view[0].copy_(rm.float())
        self.run.view[1].copy_(rv.float())
        self.nbt = torch.full((3,), 7, dtype=torch.int64, device="cuda")
        self.small = Placed((4, C_), 0, 0)

    def bn(self, eps):
        return (self.gamma, self.beta, self.run.view[0], self.run.view[1], self.nbt[1:2], MOMENTUM, eps)

    def check(self, ref, what, launches=1):
        mean, invstd, scale, shift, new_rm, new_rv = ref
        for i, (r, n) in enumerate(zip((mean, invstd, scale, shift), ("mean", "invstd", "scale", "shift"))):
            exact(self.small.view[i], r, "%s: %s" % (what, n))
        exact(self.run.view[0], new_rm, what + ": running mean")
        exact(self.run.view[1], new_rv, what + ": running var")
        assert self.nbt.tolist() == [7, 7 + launches, 7], what
        assert self.small.untouched_around() and self.run.untouched_around(), "%s: wrote outside" % what


@pytest.mark.parametrize("ntiles", B.FINALIZE_NTILES)
def test_finalize(ntiles):
    from coclr_amd import ops
    C_, count = 5, 96.0
    for k in (0, -1, 1):
        stats, m = stats_exact(C_, ntiles, count, k)
        gamma, beta, rm, rv = bn_params(C_)
        fb = FwdBuffers(C_, stats, gamma, beta, rm, rv)
        s = fb.small.view
        ops.bn_finalize(fb.stats, C_, ntiles, count, *fb.bn(3.0 * 4.0 ** k), s[0], s[1], s[2], s[3])
        sync("bn_finalize")
        fb.check(finalize_reference(m, k, count, gamma, beta, rm, rv), "finalize ntiles=%d k=%d" % (ntiles, k))


def test_eval_affine():
    from coclr_amd import ops
    C_, k = 300, -1
    gamma, beta, rm, _ = bn_params(C_)
    rv = torch.full((C_,), 4.0 ** k).double()
    small = Placed((4, C_), 0, 0)
    s = small.view
    ops.bn_eval_affine(vector(gamma), vector(beta), vector(rm), vector(rv), 3.0 * 4.0 ** k, C_, s[0], s[1], s[2], s[3])
    sync("bn_eval_affine")
    invstd = torch.full((C_,), 2.0 ** -(k + 1)).double()
    for i, r in enumerate((rm, invstd, gamma * invstd, beta - rm * gamma * invstd)):
        exact(s[i], r, "eval affine %d" % i)
    assert small.untouched_around()


def _forward(c, kind, relu, seed=0, k=0, ntiles=3):
    """One coclr_bn_finalize_apply of the row: (reference tuple, reference z, buffers, z destination)."""
    from coclr_amd import ops
    u = unit(c.name, kind, seed)
    count = float(c.N * B.S(c))
    gamma, beta, rm, rv = bn_params(c.C, seed)
    if kind == "int":
        stats, m = stats_exact(c.C, ntiles, count, k, seed)
        ref = finalize_reference(m, k, count, gamma, beta, rm, rv)
        eps = 3.0 * 4.0 ** k
    else:
        gen = torch.Generator().manual_seed(5 + seed)
        gamma = gamma * (torch.rand(c.C, generator=gen) + 0.5).double()
        tot = torch.stack([u["y"].sum((0, 2, 3, 4)), (u["y"] ** 2).sum((0, 2, 3, 4))])
        stats = (tot.unsqueeze(-1) / ntiles * (1 + 0.1 * torch.randn(2, c.C, ntiles, generator=gen))).float().double()
        s, q = stats.sum(-1)
        eps = 1e-5
        mean = s / count
        var = (q / count - mean * mean).clamp_min(0)
        invstd = 1.0 / torch.sqrt(var + float(torch.tensor(eps).float()))
        scale = gamma.float().double() * invstd
        ref = (mean, invstd, scale, beta - mean * scale, (1 - MOMENTUM) * rm + MOMENTUM * mean,
               (1 - MOMENTUM) * rv + MOMENTUM * var * count / (count - 1))
    fb = FwdBuffers(c.C, stats, gamma, beta, rm, rv)
    yd = place(c, "y", u["y"])
    zp = dest(c, "z")
    rz = u["y"] * per_channel(ref[2]) + per_channel(ref[3])
    if relu:
        rz = torch.relu(rz)
    call = dict(stats=fb.stats, C=c.C, ntiles=ntiles, count=count, bn=fb.bn(eps), small=tuple(fb.small.view), y=yd,
                z=zp.view, relu=relu)
    return ref, rz, fb, zp, call, ops


def _call_forward(ops, call):
    ops.bn_finalize_apply(call["stats"], call["C"], call["ntiles"], call["count"], *call["bn"], *call["small"],
                          call["y"], call["z"], call["relu"])
    sync("bn_finalize_apply")


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "plain"])
@pytest.mark.parametrize("name", IDS)
def test_forward_exact(name, relu):
    c = B.BY_NAME[name]
    pl = B.plan(c)["fwd"]
    what = "%s forward one_wg=%d vec=%d" % (name, pl["one_wg"], pl["vec"])
    ref, rz, fb, zp, call, ops = _forward(c, "int", relu, k=(0, -1, 1)[len(name) % 3])
    _call_forward(ops, call)
    exact(zp.view, rz, what + ": z")
    assert zp.untouched_around(), "%s: wrote outside z" % what
    fb.check(ref, what)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "plain"])
@pytest.mark.parametrize("name", [c.name for c in B.CASES if c.dres or c.z])
def test_apply_with_residual_exact(name, relu):
    """z = act(y * scale + shift + residual) of the residual units: always the streaming kernel."""
    from coclr_amd import ops
    c = B.BY_NAME[name]
    u = unit(name, "int")
    zp = dest(c, "z")
    ops.bn_act_apply(place(c, "y", u["y"]), vector(u["scale"]), vector(u["shift"]), place(c, "dres", u["res"]),
                     zp.view, relu)
    sync("bn_act_apply")
    rz = u["y"] * per_channel(u["scale"]) + per_channel(u["shift"]) + u["res"]
    exact(zp.view, torch.relu(rz) if relu else rz, name + ": z with residual")
    assert zp.untouched_around(), name


# ---- backward ---------------------------------------------------------------------------------------------------------

def _backward(c, kind, relu, training, accumulate=False, seed=0, coeffs=False):
    """One coclr_bn_act_backward (or _coeffs) of the row: dict of the outputs' Placed buffers and references."""
    from coclr_amd import ops
    u = unit(c.name, kind, seed)
    z = zs(u) if c.z else None
    g = masked(u, relu, z)
    rdy, rdg, rdb, A, Bc, D = bn_backward_reference(g, u["y"], u["scale"], u["mean"], u["invstd"], training,
                                                    exact_roundings=kind == "int")
    dzd, yd = place(c, "dz", u["dz"]), place(c, "y", u["y"])
    co = [vector(u[k]) for k in ("scale", "shift", "mean", "invstd")]
    sums = torch.full((ops.bn_backward_workspace(c.N, c.C),), NAN, dtype=torch.float64, device="cuda")
    dgb = Placed((2, c.C), 0, 0)
    out = dict(rdy=rdy, rdg=rdg, rdb=rdb, dgb=dgb, g=g, u=u)
    if coeffs:
        coef = Placed((5, c.C), 0, 0)
        ops.bn_act_backward_coeffs(dzd, yd, co[0], co[1], co[2], co[3], sums, coef.view.view(-1), dgb.view[0],
                                   dgb.view[1], relu, training)
        out.update(coef=coef, rcoef=torch.stack([A, Bc, D, u["scale"], u["shift"]]))
    else:
        dyp = dest(c, "dy")
        drp = None
        if c.dres:
            drp = dest(c, "dres")
            if accumulate:
                out["prior"] = torch.randint(-8, 9, shape(c), generator=torch.Generator().manual_seed(9)).double()
                drp.put(out["prior"])
        ops.bn_act_backward(dzd, yd, place(c, "z", z) if c.z else None, co[0], co[1], co[2], co[3], sums, dyp.view,
                            drp.view if drp else None, dgb.view[0], dgb.view[1], relu, training,
                            dres_accumulate=accumulate)
        out.update(dy=dyp, dres=drp)
    sync("bn_act_backward of " + c.name)
    return out


def _has_zero_crossings(u):
    return bool((u["y"] * per_channel(u["scale"]) + per_channel(u["shift"]) == 0).any())


@pytest.mark.parametrize("mode", ["relu-train", "plain-train", "relu-eval"])
@pytest.mark.parametrize("name", IDS)
def test_backward_exact(name, mode):
    c = B.BY_NAME[name]
    relu, training = mode.startswith("relu"), mode.endswith("train")
    pl = B.plan(c)["bwd"]
    what = "%s backward one_wg=%d vec=%d groups=%d grid=%s %s" % (name, pl["one_wg"], pl["vec"], pl["groups"],
                                                                   pl["grid"], mode)
    assert _has_zero_crossings(unit(name, "int")), what
    for accumulate in ((False, True) if c.dres else (False,)):
        o = _backward(c, "int", relu, training, accumulate)
        exact(o["dgb"].view[0], o["rdg"], what + ": dgamma")
        exact(o["dgb"].view[1], o["rdb"], what + ": dbeta")
        exact(o["dy"].view, o["rdy"], what + ": dy")
        assert o["dy"].untouched_around() and o["dgb"].untouched_around(), "%s: wrote outside" % what
        if c.dres:
            exact(o["dres"].view, o["g"] + o["prior"] if accumulate else o["g"], what + ": dres")
            assert o["dres"].untouched_around(), what


@pytest.mark.parametrize("mode", ["relu-train", "plain-train", "relu-eval"])
@pytest.mark.parametrize("name", [c.name for c in B.CASES if not c.z and not c.dres])
def test_backward_coeffs_exact(name, mode):
    c = B.BY_NAME[name]
    relu, training = mode.startswith("relu"), mode.endswith("train")
    o = _backward(c, "int", relu, training, coeffs=True)
    exact(o["coef"].view, o["rcoef"], "%s %s: coef[5][C]" % (name, mode))
    exact(o["dgb"].view[0], o["rdg"], name + ": dgamma")
    exact(o["dgb"].view[1], o["rdb"], name + ": dbeta")
    assert o["coef"].untouched_around() and o["dgb"].untouched_around(), name


# ---- several units per call ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", list(B.MULTI))
def test_multi_forward_exact(which):
    from coclr_amd import ops
    names = B.MULTI[which]
    units = [_forward(B.BY_NAME[n], "int", i % 2 == 0, seed=i + 1, k=(0, -1, 1)[i % 3], ntiles=(3, 1, 300)[i % 3])
             for i, n in enumerate(names)]
    ops.bn_finalize_apply_multi([u[4] for u in units])
    sync("bn_finalize_apply_multi")
    for i, (n, (ref, rz, fb, zp, _, _)) in enumerate(zip(names, units)):
        what = "%s unit %d (%s)" % (which, i, n)
        exact(zp.view, rz, what + ": z")
        assert zp.untouched_around(), what
        fb.check(ref, what)


def _partials(o, tiles, C_):
    """[2][C][ntiles] fp32 arrays whose float64 sum is the unit's exact (sum g, sum g * xhat)."""
    gen = torch.Generator().manual_seed(sum(tiles))
    tot = torch.stack([o["rdb"], o["rdg"]])
    parts = [torch.randint(-8, 9, (2, C_, n), generator=gen).double() / 4 for n in tiles]
    parts[0][:, :, 0] += tot - sum(p.sum(-1) for p in parts)
    assert all(bool((p.float().double() == p).all()) for p in parts)
    return [(source(p.reshape(1, -1)).view(-1), n) for p, n in zip(parts, tiles)]


def _multi_backward(spec, kind="int"):
    from coclr_amd import ops
    calls, outs = [], []
    for i, (n, tiles) in enumerate(spec):
        c = B.BY_NAME[n]
        relu, training = i % 2 == 0, i % 3 != 2
        u = unit(n, kind, i + 1)
        g = masked(u, relu)
        rdy, rdg, rdb, _, _, _ = bn_backward_reference(g, u["y"], u["scale"], u["mean"], u["invstd"], training,
                                                       exact_roundings=kind == "int")
        o = dict(rdy=rdy, rdg=rdg, rdb=rdb, u=u, dy=dest(c, "dy"), dgb=Placed((2, c.C), 0, 0))
        call = dict(dz=place(c, "dz", u["dz"]), y=place(c, "y", u["y"]), scale=vector(u["scale"]),
                    shift=vector(u["shift"]), mean=vector(u["mean"]), invstd=vector(u["invstd"]),
                    sums=torch.full((ops.bn_backward_workspace(c.N, c.C),), NAN, dtype=torch.float64, device="cuda"),
                    dy=o["dy"].view, dgamma=o["dgb"].view[0], dbeta=o["dgb"].view[1], relu=relu, training=training)
        if tiles:
            call["partials"] = _partials(o, tiles, c.C)
        calls.append(call)
        outs.append(o)
    ops.bn_act_backward_multi(calls)
    sync("bn_act_backward_multi")
    return outs


MULTI_BWD = dict([(k, tuple((n, None) for n in v)) for k, v in B.MULTI.items()] + list(B.MULTI_PARTIALS.items()) +
                 [(k, (v,)) for k, v in B.PARTIALS.items()])


@pytest.mark.parametrize("which", list(MULTI_BWD))
def test_multi_backward_exact(which):
    spec = MULTI_BWD[which]
    for i, ((n, tiles), o) in enumerate(zip(spec, _multi_backward(spec))):
        what = "%s unit %d (%s%s)" % (which, i, n, ", partials %s" % (tiles,) if tiles else "")
        exact(o["dgb"].view[0], o["rdg"], what + ": dgamma")
        exact(o["dgb"].view[1], o["rdb"], what + ": dbeta")
        exact(o["dy"].view, o["rdy"], what + ": dy")
        assert o["dy"].untouched_around() and o["dgb"].untouched_around(), "%s: wrote outside" % what


# ---- random data ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", IDS)
def test_random_data(name):
    c = B.BY_NAME[name]
    first = None
    for _ in range(2):
        ref, rz, fb, zp, call, ops = _forward(c, "randn", True)
        _call_forward(ops, call)
        o = _backward(c, "randn", True, True)
        got = [zp.view.clone(), fb.small.view.clone(), o["dy"].view.clone(), o["dgb"].view.clone()]
        if c.dres:
            got.append(o["dres"].view.clone())
        if first is None:
            first = got
            close(zp.view, rz, 2e-4, name + ": z")
            for i in range(4):
                close(fb.small.view[i], ref[i], 2e-4, name + ": " + ("mean", "invstd", "scale", "shift")[i])
            close(o["dy"].view, o["rdy"], 5e-4, name + ": dy")
            close(o["dgb"].view[0], o["rdg"], 5e-4, name + ": dgamma")
            close(o["dgb"].view[1], o["rdb"], 5e-4, name + ": dbeta")
        else:
            assert all(torch.equal(a, b) for a, b in zip(first, got)), "%s: not bit-identical" % name


# ---- the temporal instantiations: a child process with COCLR_BN_NT_MB=-1 ---------------------------------------------------

def _vector_rows():
    return [c for c in B.CASES if not B.plan(c)["bwd"]["one_wg"] and B.plan(c)["bwd"]["vec"]]


def _streaming_outputs():
    """Everything the vector streaming passes write for the vector rows (BatchNorm rows on both kinds of data, the
    pooled BatchNorm backward rows of the pooling table), as CPU tensors."""
    import _pool_cases as P
    import test_gpu_pool_exact as TP
    from coclr_amd import ops
    out = {}
    for c in _vector_rows():
        for kind in ("int", "randn"):
            o = _backward(c, kind, True, True)
            out["%s/%s/dy" % (c.name, kind)] = o["dy"].view.cpu()
            out["%s/%s/dgb" % (c.name, kind)] = o["dgb"].view.cpu()
            if c.dres:
                out["%s/%s/dres" % (c.name, kind)] = o["dres"].view.cpu()
            u = unit(c.name, kind)
            zp = dest(c, "z")
            ops.bn_act_apply(place(c, "y", u["y"]), vector(u["scale"]), vector(u["shift"]),
                             place(c, "dres", u["res"]) if c.dres else None, zp.view, True)
            sync("bn_act_apply")
            out["%s/%s/z" % (c.name, kind)] = zp.view.cpu()
            if not c.z and not c.dres:
                o = _backward(c, kind, True, True, coeffs=True)
                out["%s/%s/coef" % (c.name, kind)] = o["coef"].view.cpu()
    for name in TP.POOLED:
        pc = P.BY_NAME[name]
        if P.plan(pc)["pooled"]["vec"]:
            dyp, dgb, _ = TP._run_pooled(pc, TP.pooled_problem(name, "randn"), True)
            out["pooled/%s/dy" % name] = dyp.view.cpu()
            out["pooled/%s/dgb" % name] = dgb.view.cpu()
            x = TP.problem(name)[0]
            yp = Placed(tuple(TP.problem(name)[2].shape), pc.y_extra, 0)
            ops.maxpool_fwd(P.geom(pc), source(x, pc.x_extra, pc.x_pad), yp.view, None, **TP.in_affine(pc))
            sync("maxpool_fwd")
            out["pooled/%s/y" % name] = yp.view.cpu()
    return out


def test_temporal_instantiations_in_a_child_process(tmp_path):
    import _pool_cases as P
    rows = _vector_rows()
    assert rows and all(B.plan(c)["bwd"]["nt"] for c in rows), "this process does not run the non-temporal passes"
    assert any(P.plan(c)["nt"] for c in P.CASES)
    path = str(tmp_path / "temporal.pt")
    env = dict(os.environ, COCLR_BN_NT_MB="-1")
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, timeout=240).returncode
    except subprocess.TimeoutExpired:
        pytest.exit("the COCLR_BN_NT_MB=-1 child process hung on the GPU", returncode=3)
    if rc < 0 or rc in (3, 124, 134, 137, 139):
        # a signal, an abort or a device error reported through sync(): nothing more is started on that device
        pytest.exit("the COCLR_BN_NT_MB=-1 child process ended with %d" % rc, returncode=3)
    assert rc == 0, "the child process failed with %d" % rc
    theirs = torch.load(path)
    assert theirs.pop("nt") == [False, False]
    mine = _streaming_outputs()
    assert sorted(mine) == sorted(theirs) and len(mine) > 20
    for k in sorted(mine):
        a, b = mine[k], theirs[k]
        assert torch.equal(a, b) or torch.equal(torch.nan_to_num(a, nan=123.0), torch.nan_to_num(b, nan=123.0)), k


if __name__ == "__main__":
    # the child of test_temporal_instantiations_in_a_child_process
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import _pool_cases
    try:
        res = _streaming_outputs()
    except pytest.exit.Exception as e:           # sync() met a device error: tell the parent
        print(e, file=sys.stderr)
        sys.exit(3)
    res["nt"] = [B.plan(B.BY_NAME["large_stream"])["bwd"]["nt"], _pool_cases.plan(_pool_cases.BY_NAME["t133_128"])["nt"]]
    torch.save(res, sys.argv[1])
