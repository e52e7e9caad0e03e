"""Shared pieces of the exact pooling / BatchNorm GPU tests (tests/test_gpu_pool_exact.py,
tests/test_gpu_bn_exact.py), of the contrastive head (tests/test_gpu_head_exact.py, tests/test_gpu_loss_exact.py) and of
the optimiser, global average pool and self-gating kernels (tests/test_gpu_small_exact.py, with its references in
tests/_small_cases.py): operand placement with guards, exact comparison, and the BatchNorm backward reference
in float64 with fp32 roundings at the points the kernels determine."""
import pytest
import torch

OUTSIDE = float(2 ** 20)       # memory a kernel must not read (finite, and far above every datum)
GUARD = -12345.0               # memory a kernel must not write
NAN = float("nan")
PAD = 256


def sync(what="a launch"):
    """A launch that faulted ends the session: nothing more is started on a device in that state."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after %s: %s" % (what, e), returncode=3)


class Placed:
    """A dense-in-(C, T, H, W) operand of shape (N, C, *dims) on the device as channels [off, off + C) of a buffer
    `extra` channels wider whose samples are `pad` floats further apart, between two guard runs.  Everything that
    is not the operand holds `around`."""

    def __init__(self, shape, extra=0, pad=0, fill=NAN, around=GUARD, dtype=torch.float32):
        N, Cc = shape[:2]
        S = 1
        for v in shape[2:]:
            S *= v
        self.nstride = (Cc + extra) * S + pad
        self.buf = torch.full((2 * PAD + N * self.nstride,), around, device="cuda", dtype=dtype)
        off = min(1, extra)
        strides = [self.nstride, S]
        acc = S
        for v in shape[2:]:
            acc //= v
            strides.append(acc)
        self.view = self.buf.as_strided(tuple(shape), tuple(strides), PAD + off * S)
        self.view.fill_(fill)
        self.around = around

    def put(self, t):
        self.view.copy_(t.to(self.view.dtype))
        return self.view

    def untouched_around(self):
        """Nothing but the operand was written (call after the operand was compared: it is overwritten)."""
        self.view.fill_(self.around)
        return bool((self.buf == self.around).all())


def source(t, extra=0, pad=0):
    """A read-only operand: its surroundings hold OUTSIDE."""
    dtype = torch.int32 if t.dtype in (torch.int32, torch.int64) else torch.float32
    return Placed(tuple(t.shape), extra, pad, fill=0, around=OUTSIDE, dtype=dtype).put(t)


class Placed2D(Placed):
    """A (rows, cols) row-major operand whose rows are `pad` floats further apart than their length, starting `shift`
    floats past a 16-byte boundary, between two guard runs; the row padding holds `around` as well.  `view` is the
    operand, `ld` its leading dimension."""

    def __init__(self, rows, cols, pad=0, shift=0, fill=NAN, around=GUARD, dtype=torch.float32):
        self.ld = cols + pad
        self.buf = torch.full((2 * PAD + shift + rows * self.ld,), around, device="cuda", dtype=dtype)
        self.view = self.buf.as_strided((rows, cols), (self.ld, 1), PAD + shift)
        self.view.fill_(fill)
        self.around = around


def source2d(t, pad=0, shift=0, transposed=False):
    """A read-only (R, C) matrix with padded rows, its surroundings and padding holding OUTSIDE.  `transposed`: the
    matrix is stored column-major ((C, R) rows in memory, each padded) and returned as the (R, C) view of that."""
    dtype = t.dtype if t.dtype in (torch.int32, torch.int64, torch.uint8) else torch.float32
    src = t.t() if transposed else t
    v = Placed2D(src.shape[0], src.shape[1], pad, shift, fill=0, around=OUTSIDE if dtype != torch.uint8 else 77,
                 dtype=dtype).put(src)
    return v.t() if transposed else v


def vector(t):
    """A per-channel read-only vector."""
    return source(t.reshape(1, -1)).view(-1)


def exact(got, ref, what):
    got, ref = got.detach().cpu(), ref.to(got.dtype).cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    same = (got == ref) | ((got != got) & (ref != ref))
    if not bool(same.all()):
        idx = (~same).nonzero()[0].tolist()
        raise AssertionError("%s: %d of %d elements differ from float64; first at %s: got %r, want %r" % (
            what, int((~same).sum()), same.numel(), idx, got[tuple(idx)].item(), ref[tuple(idx)].item()))


def close(got, ref, rtol, what):
    got, ref = got.detach().cpu().double(), ref.double()
    err = float((got - ref).abs().max())
    bound = rtol * float(ref.abs().max())
    print("%s: max abs err %.3e, bound %.3e" % (what, err, bound))
    assert err <= bound, "%s: max abs err %.3e > %.3e" % (what, err, bound)


def f32(t):
    """Round a float64 tensor to fp32 (one rounding) and return it as float64."""
    return t.float().double()


def per_channel(v, ndim=5):
    return v.view(1, -1, *([1] * (ndim - 2)))


def bn_backward_reference(g, y, scale, mean, invstd, training, exact_roundings=True):
    """BatchNorm backward of one unit from the masked gradient g (float64, [N][C][...]) and the convolution output
    y: (dy, dgamma, dbeta, coef A, B, D), all float64.  With exact_roundings the fp32 roundings sit where the
    kernels' are determined: mg, mgx = fp32(sum / count); B and the product inside D exact (scale, invstd and
    mean * invstd are powers of two in the exact rows); D one rounding; dy two single-rounding fmaf."""
    red = (0,) + tuple(range(2, g.dim()))
    count = g.numel() // g.shape[1]
    xhat = (y - per_channel(mean, g.dim())) * per_channel(invstd, g.dim())
    sg, sgx = g.sum(red), (g * xhat).sum(red)
    r = f32 if exact_roundings else (lambda t: t)
    A = scale.clone()
    if training:
        mg, mgx = r(sg / count), r(sgx / count)
        B = r(-scale * invstd * mgx)
        D = r(scale * r(mean * invstd * mgx - mg))
    else:
        B, D = torch.zeros_like(A), torch.zeros_like(A)
    inner = r(per_channel(B, g.dim()) * y + per_channel(D, g.dim()))
    dy = r(per_channel(A, g.dim()) * g + inner)
    return dy, sgx, sg, A, B, D
