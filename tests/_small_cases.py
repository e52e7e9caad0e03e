"""Case tables, input generators and float64 references of the exact optimiser / global-pool / self-gating tests
(tests/test_gpu_small_exact.py), as plain data and host code: nothing here touches a device.
tests/test_small_cases_cpu.py re-derives the launcher branch of every row from the host predicates of
coclr_amd/csrc/optim.hip, pool.hip and nce.hip restated below, asserts that every branch is reached, and checks every
reference against an independent float64 formulation.

Exactness.  Every reference is float64 with an fp32 rounding (`_exact.f32`) exactly where the kernel determines one:
  * momentum update: two products and one add, each rounded (the kernel's __fmul_rn / __fadd_rn);
  * Adam, exact rows: one step from zero state with beta1 = 1/2, beta2 = 3/4, eps = 0, gradients +-2^a, lr a power of
    two, p a small multiple of lr: m = g/2, v = g^2/4, sqrt(v) / sqrt(1 - beta2) = |g| and lr / (1 - beta1) / 2 = lr are
    all exact, so p' = p - lr * sign(g) bit for bit.  With wd = 2^-3 and p in {8g, -4g, -16g}, g + wd * p is 2g, g/2, -g;
  * Adam, bounded rows: the float64 recurrence with the kernel's scalars (doubles, rounded once to fp32 where ATen
    rounds a Scalar to the op-math type) and NO intermediate rounding: the yardstick both implementations are measured by;
  * average pool: integers (any summation order is exact) and the single-rounding quotient fp32(sum) / fp32(S); the
    backward is fp32(dy * fp32(1 / S)), two roundings;
  * plane_scale / plane_dot: operands on a grid of 2^-6 in [-4, 4] / integers in [-3, 3];
  * sigmoid: float64; the backward is fp32(fp32(dw * w) * fp32(1 - w)) from the w it is given."""
import math
from collections import namedtuple

import torch

from _exact import f32
from _head_ref import cdiv, gen, ints, is_fp32  # noqa: F401  (re-exported for the two test files)

CHUNK = 32768                   # coclr_amd/optim.py::_CHUNK, model/pretrain.py::_CHUNK: elements per table row
THREADS = 256
GRID_CAP = 2048                 # grid1d (nce.hip) and coclr_global_avgpool_bwd (pool.hip)
TINY = 2.0 ** -126              # the smallest normal fp32


def f32s(x):
    """A Python float rounded once to fp32 (as ATen rounds a Scalar, as ctypes rounds a c_float argument)."""
    return float(torch.tensor(float(x), dtype=torch.float64).float())


def chunks(count):
    """(offset, count) of the table rows the host builds for one tensor (optim.py::_build_plan)."""
    return [(off, min(CHUNK, count - off)) for off in range(0, count, CHUNK)]


def lanes_branch(cnt, vector):
    """The two loops of momentum_update_kernel / adam_multi_kernel over one table row: n4 float4 iterations over 256
    threads where every pointer is on a 16-byte boundary, then the scalar loop over what is left."""
    n4 = cnt >> 2 if vector else 0
    tail = cnt - 4 * n4
    return {"vector": vector, "n4": n4, "tail": tail, "vector_passes": cdiv(n4, THREADS), "tail_passes": cdiv(tail, THREADS)}


# ---- coclr_momentum_update ---------------------------------------------------------------------------------------------
# tensors: (count, dst shift, src shift); a shift is in floats past a 16-byte boundary
MomT = namedtuple("MomT", "count dst_shift src_shift")
Mom = namedtuple("Mom", "name m tensors")
MOM_COUNTS = (1, 3, 4, 5, 255, 1027, CHUNK - 1, CHUNK)
SHIFTS2 = ((0, 0), (1, 0), (0, 1), (1, 1))


def _mom_rows():
    rows = []
    for i, n in enumerate(MOM_COUNTS):
        for j, (ds, ss) in enumerate(SHIFTS2):
            rows.append(Mom("n%d-d%d-s%d" % (n, ds, ss), (0.999, 0.5)[(i + j) % 2], (MomT(n, ds, ss),)))
    rows.append(Mom("mixed", 0.999, (MomT(5, 0, 0), MomT(1027, 1, 0), MomT(4, 0, 1), MomT(255, 1, 1), MomT(CHUNK, 0, 0),
                                     MomT(3, 0, 0))))
    rows.append(Mom("three-chunks", 0.5, (MomT(2 * CHUNK + 4, 0, 0),)))
    rows.append(Mom("three-chunks-unaligned", 0.999, (MomT(2 * CHUNK + 5, 1, 1),)))
    return rows


MOMENTUM = _mom_rows()


def momentum_branches(c):
    """One branch record per table row (chunk) of a momentum launch."""
    return [lanes_branch(cnt, (t.dst_shift | t.src_shift) % 4 == 0) for t in c.tensors for _, cnt in chunks(t.count)]


def momentum_inputs(c):
    g = gen(len(c.tensors), c.tensors[0].count, int(c.m * 1000))
    return [(f32(torch.randn(t.count, generator=g, dtype=torch.float64)),
             f32(torch.randn(t.count, generator=g, dtype=torch.float64))) for t in c.tensors]


def momentum_reference(d, s, m):
    """d * m + s * (1 - m) as the kernel rounds it: m and 1 - m (formed in double) rounded once to fp32, two products
    and one add, each rounded.  (The product of two fp32 values is exact in float64.)"""
    return f32(f32(d * f32s(m)) + f32(s * f32s(1.0 - m)))


def momentum_cpu32(d, s, m):
    """The reference's tensor expression p_k * m + p_q * (1 - m) (model/pretrain.py:76-80) in CPU fp32."""
    return d.float() * m + s.float() * (1. - m)


# ---- coclr_adam_step, exact rows ---------------------------------------------------------------------------------------
# params: count, slot (the hyper row and step counter the table names), shifts of (p, g, m, v, k) in floats past a 16-byte
# boundary, key (a key-encoder tensor takes the folded momentum update), wd.  Slots no parameter names are OUTSIDE the
# launch: their hyper rows hold NaN, their counters must not move.
AdamP = namedtuple("AdamP", "count slot shifts key wd")
AdamL = namedtuple("AdamL", "name nslots params")
ADAM_COUNTS = (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 3, 2 * CHUNK + 4)
ALIGNED = (0, 0, 0, 0, 0)
POINTERS = "pgmvk"
EXACT_BETAS, EXACT_EPS, EXACT_WD = (0.5, 0.75), 0.0, 2.0 ** -3
FOLD_M = 0.999


def lr_of(slot):
    return 2.0 ** -(5 + slot)


def alone(name):
    return tuple(int(c == name) for c in POINTERS)


def _adam_rows():
    rows = []
    for i, n in enumerate(ADAM_COUNTS):
        rows.append(AdamL("n%d-aligned" % n, 5, (AdamP(n, 1 + i % 3, ALIGNED, bool(i % 2), 0.0),)))
    for i, name in enumerate(POINTERS):
        for n in (4, CHUNK + 3):
            rows.append(AdamL("n%d-%s-unaligned" % (n, name), 5,
                              (AdamP(n, 1 + i % 3, alone(name), name == "k" or bool(i % 2), 0.0),)))
    rows.append(AdamL("three-lr", 7, (AdamP(5, 0, ALIGNED, False, 0.0), AdamP(CHUNK + 1, 2, ALIGNED, True, 0.0),
                                      AdamP(3, 3, ALIGNED, False, 0.0), AdamP(2 * CHUNK + 4, 5, alone("g"), True, 0.0))))
    rows.append(AdamL("weight-decay", 5, (AdamP(CHUNK + 3, 1, ALIGNED, True, EXACT_WD), AdamP(5, 2, ALIGNED, False, 0.0),
                                          AdamP(5, 3, alone("m"), False, EXACT_WD))))
    return rows


ADAM = _adam_rows()


def adam_vector(p):
    """adam_multi_kernel's `vec`: p, g, m, v and k (0 where there is none) all on a 16-byte boundary."""
    s = p.shifts if p.key else p.shifts[:4]
    return all(v % 4 == 0 for v in s)


def adam_branches(c):
    return [dict(lanes_branch(cnt, adam_vector(p)), key=p.key, wd=p.wd != 0, slot=p.slot, chunk=i)
            for p in c.params for i, (_, cnt) in enumerate(chunks(p.count))]


def outside_slots(c):
    return [s for s in range(c.nslots) if s not in {p.slot for p in c.params}]


def outside_step(slot):
    return float(3 + slot)


def adam_exact_inputs(c, i):
    """(p, g, k) of parameter i of an exact launch, float64 holding fp32 values."""
    p_ = c.params[i]
    g = gen(p_.count, p_.slot, i, sum(p_.shifts), int(p_.wd != 0))
    sign = ints((p_.count,), 0, 1, g) * 2 - 1
    grad = sign * 2.0 ** ints((p_.count,), -4, 2, g)
    if p_.wd != 0:
        p = torch.tensor([8.0, -4.0, -16.0], dtype=torch.float64)[torch.randint(0, 3, (p_.count,), generator=g)] * grad
    else:
        p = ints((p_.count,), -64, 64, g) * lr_of(p_.slot)
    k = f32(torch.randn(p_.count, generator=g, dtype=torch.float64))
    return p, grad, k


def adam_exact_expected(c, i, p, grad, k):
    """(p', exp_avg, exp_avg_sq, k') in closed form."""
    p_ = c.params[i]
    g2 = grad + p_.wd * p
    pn = p - lr_of(p_.slot) * torch.sign(g2)
    return pn, g2 / 2, g2 * g2 / 4, momentum_reference(k, pn, FOLD_M)


# ---- coclr_adam_step, bounded rows -------------------------------------------------------------------------------------
Bounded = namedtuple("Bounded", "name lr betas eps wd")
BOUNDED = [Bounded("default", 1e-3, (0.9, 0.999), 1e-8, 1e-5), Bounded("no-decay", 1e-3, (0.9, 0.999), 1e-8, 0.0),
           Bounded("large", 3e-2, (0.8, 0.95), 1e-3, 1e-2)]
BoundedP = namedtuple("BoundedP", "count shifts start_step")
BOUNDED_PARAMS = (BoundedP(5, ALIGNED, 7), BoundedP(CHUNK + 3, alone("g"), 0))      # one aligned, one as a bucket view
BOUNDED_STEPS, BOUNDED_LR_STEP, BOUNDED_LR_FACTOR = 10, 5, 0.1


def bounded_lr(c, step):
    return c.lr * BOUNDED_LR_FACTOR if step >= BOUNDED_LR_STEP else c.lr


def bounded_inputs(c):
    """Per parameter: (p0, exp_avg0, exp_avg_sq0, [gradient of every step]) as fp32 tensors."""
    out = []
    for i, bp in enumerate(BOUNDED_PARAMS):
        g = gen(bp.count, i, int(c.lr * 1e6), int(c.wd * 1e6))
        p0 = torch.randn(bp.count, generator=g)
        if bp.start_step:
            m0, v0 = torch.randn(bp.count, generator=g) * 0.05, torch.rand(bp.count, generator=g) * 0.01 + 1e-4
        else:
            m0, v0 = torch.zeros(bp.count), torch.zeros(bp.count)
        grads = [torch.randn(bp.count, generator=g) * 0.1 for _ in range(BOUNDED_STEPS)]
        out.append((p0, m0, v0, grads))
    return out


def adam_scalars(t, lr, betas, eps, wd):
    """The scalars of step t + 1 as the kernel header forms them: bias corrections in double; step size, sqrt(bc2),
    1 - beta1, 1 - beta2, beta2, eps and wd rounded once to fp32."""
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** (t + 1.0), 1.0 - b2 ** (t + 1.0)
    return {"step_size": f32s(lr / bc1), "bc2_sqrt": f32s(math.sqrt(bc2)), "w1": f32s(1.0 - b1), "w2": f32s(1.0 - b2),
            "b2": f32s(b2), "eps": f32s(eps), "wd": f32s(wd)}


def adam_reference(p, g, m, v, t, lr, betas, eps, wd):
    """One Adam step in float64 from step counter t (no intermediate rounding): (p', m', v')."""
    s = adam_scalars(t, lr, betas, eps, wd)
    if wd != 0:
        g = g + s["wd"] * p
    m = m + (g - m) * s["w1"]
    v = v * s["b2"] + s["w2"] * g * g
    denom = v.sqrt() / s["bc2_sqrt"] + s["eps"]
    return p - s["step_size"] * (m / denom), m, v


def bounded_reference(c):
    """Per parameter the float64 (p, exp_avg, exp_avg_sq) after every step: [param][step] -> (p, m, v)."""
    out = []
    for bp, (p0, m0, v0, grads) in zip(BOUNDED_PARAMS, bounded_inputs(c)):
        p, m, v = p0.double(), m0.double(), v0.double()
        traj = []
        for step in range(BOUNDED_STEPS):
            p, m, v = adam_reference(p, grads[step].double(), m, v, bp.start_step + step, bounded_lr(c, step), c.betas,
                                     c.eps, c.wd)
            traj.append((p, m, v))
        out.append(traj)
    return out


def relative_error(got, ref):
    """max |got - ref| relative to the tensor's maximum magnitude."""
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max().clamp(min=1e-300))


# ---- coclr_global_avgpool_fwd / _bwd -----------------------------------------------------------------------------------
PoolF = namedtuple("PoolF", "name planes S random")
POOL_FWD = ([PoolF("p%d-S%d" % (p, S), p, S, False) for p in (1, 3, 4, 5, 9) for S in (1, 2, 63, 64, 65, 98, 128, 1000)] +
            [PoolF("p5-S1000-random", 5, 1000, True)])
PoolB = namedtuple("PoolB", "name planes S")
POOL_BWD = ([PoolB("p%d-S%d" % (p, S), p, S) for p in (1, 3, 5) for S in (1, 3, 64, 98)] +
            [PoolB("p1030-S513-stride-loop", 1030, 513)])


def wave_per_plane_branch(planes, S):
    """global_avgpool_fwd / plane_scale / plane_dot: four planes per 256-thread workgroup, one wave per plane, lane l
    reads elements l, l + 64, ..."""
    blocks = cdiv(planes, 4)
    return {"blocks": blocks, "last_waves": planes - 4 * (blocks - 1), "per_lane": cdiv(S, 64), "idle_lanes": S < 64,
            "ragged": S % 64 != 0}


def pool_bwd_branch(planes, S):
    """coclr_global_avgpool_bwd: one thread per element, at most 2048 workgroups, then a grid-stride loop."""
    total = planes * S
    blocks = min(cdiv(total, THREADS), GRID_CAP)
    strided = total > blocks * THREADS
    return {"blocks": blocks, "strided": strided, "crosses": strided and (blocks * THREADS) % S != 0,
            "partial_last": total % THREADS != 0}


def pool_fwd_inputs(c):
    g = gen(c.planes, c.S, int(c.random))
    shape = (1, c.planes, 1, 1, c.S)
    return f32(torch.randn(shape, generator=g, dtype=torch.float64)) if c.random else ints(shape, -8, 8, g)


def pool_fwd_reference(x):
    """fp32(sum) / fp32(S), one rounding (the sum of the integer rows is exact)."""
    S = x.shape[2] * x.shape[3] * x.shape[4]
    return f32(x.sum((2, 3, 4), keepdim=True) / S)


def pool_bwd_inputs(c):
    return f32(torch.randn((1, c.planes, 1, 1, 1), generator=gen(c.planes, c.S), dtype=torch.float64))


def pool_bwd_reference(dy, S):
    """dy * (1.f / S): the reciprocal rounded, the product rounded."""
    return f32(dy * f32s(1.0 / S)).expand(dy.shape[0], dy.shape[1], 1, 1, S)


# ---- coclr_plane_scale / coclr_plane_dot -------------------------------------------------------------------------------
Plane = namedtuple("Plane", "name N C S")
PLANES = [Plane("N%d-C%d-S%d" % (N, C, S), N, C, S) for N, C in ((1, 1), (1, 3), (2, 2), (1, 5), (3, 3))
          for S in (1, 63, 64, 65, 70)]
# a / out dense or a channel slice of a wider, sample-padded buffer; bias; accumulate
ScaleV = namedtuple("ScaleV", "a_slice out_slice bias accumulate")
SCALE_VARIANTS = [ScaleV(a, o, b, acc) for a in (False, True) for o in (False, True) for b in (False, True)
                  for acc in (False, True)]
DotV = namedtuple("DotV", "a_slice b_slice")
DOT_VARIANTS = [DotV(a, b) for a in (False, True) for b in (False, True)]
SLICE = {"extra": 3, "pad": 5}            # _exact.Placed: channels [1, 1 + C) of C + 3, samples 5 floats further apart


def grid64(shape, g):
    """Multiples of 2^-6 in [-4, 4]."""
    return ints(shape, -256, 256, g) / 64


def plane_scale_inputs(c):
    g = gen(c.N, c.C, c.S)
    shape = (c.N, c.C, 1, 1, c.S)
    return grid64(shape, g), grid64((c.N, c.C), g), grid64((c.N, c.C), g), grid64(shape, g)     # a, gain, bias, out0


def plane_scale_reference(a, gain, bias, out0, v):
    r = a * gain[:, :, None, None, None]
    if v.bias:
        r = r + bias[:, :, None, None, None]
    r = f32(r)                              # fmaf: one rounding of the exact a * g + b
    return f32(out0 + r) if v.accumulate else r


def plane_dot_inputs(c):
    g = gen(c.S, c.C, c.N)
    shape = (c.N, c.C, 1, 1, c.S)
    return ints(shape, -3, 3, g), ints(shape, -3, 3, g)


def plane_dot_reference(a, b):
    return (a * b).sum((2, 3, 4))


# ---- coclr_sigmoid_fwd / _bwd ------------------------------------------------------------------------------------------
# 1, 255, 256, 257 and 70 000 elements; grid1d gives 70 000 elements 274 workgroups (it caps at 2048), so the last row is
# the one that reaches the grid-stride loop
SIGMOID_N = (1, 255, 256, 257, 70000, GRID_CAP * THREADS + 257)
INF = float("inf")
SIGMOID_FIXED = (0.0, 1.0, -1.0, 16.5, -16.5, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0, INF, -INF, float("nan"))


def grid1d(n, cap=GRID_CAP):
    """nce.hip: grid1d."""
    return max(1, min(cdiv(n, THREADS), cap))


def elementwise_branch(n):
    blocks = grid1d(n)
    return {"blocks": blocks, "strided": n > blocks * THREADS, "partial_last": n % THREADS != 0}


def sigmoid_args(n):
    """Uniform in [-20, 20] with the fixed points at the front and, where they fit twice, at the very end."""
    s = f32(torch.rand(n, generator=gen(n), dtype=torch.float64) * 40 - 20)
    fixed = torch.tensor(SIGMOID_FIXED, dtype=torch.float64)
    k = min(n, len(fixed))
    s[:k] = fixed[:k]
    if n >= 2 * len(fixed):
        s[-len(fixed):] = fixed
    return s


def sigmoid_reference(s):
    return torch.sigmoid(s)


def sigmoid_classes(s):
    """(nan, one, tiny, rest): NaN arguments; +inf; -inf and every argument whose true value is below the smallest
    normal fp32; everything else (held in ulps)."""
    nan = s != s
    one = s == INF
    tiny = ~nan & (sigmoid_reference(s) < TINY)
    return nan, one, tiny, ~(nan | one | tiny)


def ulp_error(got, ref):
    """|got - ref| in units of the fp32 spacing at ref (float64 tensors; ref normal in fp32)."""
    _, e = torch.frexp(ref.abs())
    return (got - ref).abs() / torch.ldexp(torch.ones_like(ref), e - 24)


def sigmoid_bwd_inputs(n):
    return f32(torch.randn(n, generator=gen(n, 1), dtype=torch.float64))


def sigmoid_bwd_reference(dw, w):
    """dw * w * (1.f - w), left to right: no product feeds an add, so contraction cannot change it."""
    return f32(f32(dw * w) * f32(1.0 - w))
