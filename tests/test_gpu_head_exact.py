"""Exact contrastive head: every row of tests/_head_cases.py (every launcher branch of coclr_amd/csrc/nce.hip and of the
retrieval half of retrieval.hip, see tests/test_head_cases_cpu.py) against float64, on inputs whose float64 result is an
fp32 value and does not depend on summation order, so the comparison is torch.equal.

  * GEMM family: integer operands in [-3, 3], integer bias, alpha a power of two, K <= 16384: every partial sum is an
    integer below 2^24.  Row normalise (mode 2): product rows with 64 * 4^j entries of +-2^j through a one-hot B, so the
    norm is a power of two; the all-zero row gives y = 0 and inv = fp32(1 / fp32(1e-12)).  l_pos + normalise backward
    (mode 3): 1 / T in {8, 16}, y and k in {0, +-1/8}, integer dlogits, inv_norm a power of two.  Average-pool backward
    (mode 4): one rounding, fp32(v * fp32(1 / S)).
  * l2norm / logits: unit vectors of 4^j entries +-2^-j (tests/_head_ref.py): similarities are multiples of 1/64 and
    tie; the logit is fp32(similarity * (1.f / T)), one rounding.  The fused kernel and the lpos + GEMM fallback (a q
    view one float off a 16-byte boundary; D != 128) must agree bit for bit.
  * positives / retrieval: the reference is the documented rule -- repeated selection in (value descending, column
    ascending) order = a stable descending sort -- on the EXACT similarities, never on the kernel's own output.
  * every GEMM / norm / logits row also runs on randn data at the bound tests/test_gpu_kernels.py uses for these kernels
    (RTOL = 2e-4 of max|ref|; 5e-4 for the normalise backward), twice, bit-identically: integers alone would pass a
    reduced-precision path.

Memory a kernel must not read holds 2^20; memory it must not write holds a sentinel that is compared afterwards; memory
it must write first holds NaN (7 for masks, -7 for integer outputs).
"""
import pytest
import torch
import torch.nn.functional as F

import _head_cases as H
import _head_ref as R
from _exact import NAN, Placed2D, close, exact, source2d, sync, vector

pytestmark = pytest.mark.gpu

RTOL = 2e-4                     # tests/test_gpu_kernels.py: RTOL, the bound of the head's GEMM / norm / logits tests
RTOL_BWD = 5e-4                 # ... and of its normalise backward
EINVAL = r"hipError 1$"         # COCLR_EINVAL through coclr_amd._lib.check


def ops():
    from coclr_amd import ops as o
    return o


def rejected():
    from coclr_amd import _lib
    return pytest.raises(_lib.HipLibraryError, match=EINVAL)


def row(t):
    """A read-only 1-D operand of any dtype."""
    return source2d(t.reshape(1, -1))[0]


def f32t(t):
    return t.float().double()


def compare(kind, got, ref, what, rtol=RTOL):
    if kind == "int":
        exact(got, ref, what)
    else:
        close(got, ref, rtol, what)


def intact(*placed):
    for p in placed:
        assert p.untouched_around(), "a guard region was written"


# ---- coclr_gemm --------------------------------------------------------------------------------------------------------

def gemm_data(c, kind):
    g = R.gen(c.M, c.N, c.K, c.splits, kind == "int")
    if kind == "int":
        return (R.ints((c.M, c.K), -3, 3, g), R.ints((c.K, c.N), -3, 3, g), R.ints((c.N,), -4, 4, g),
                R.ints((c.M, c.N), -5, 5, g))
    return tuple(torch.randn(s, generator=g).double() for s in ((c.M, c.K), (c.K, c.N), (c.N,), (c.M, c.N)))


def gemm_run(c, A, Bm, bias, c0):
    o = ops()
    Ad, Bd = source2d(A, c.pad, transposed=c.ta), source2d(Bm, c.pad, transposed=c.tb)
    sam, sak = R.operand_strides(c.M, c.K, c.pad, c.ta)
    sbk, sbn = R.operand_strides(c.K, c.N, c.pad, c.tb)
    out = Placed2D(c.M, c.N, c.pad)
    if c.accumulate:
        out.put(c0)
    nws = o.gemm_workspace(c.M, c.N, c.K, c.splits)
    ws = Placed2D(1, max(1, nws))
    o.gemm(Ad, sam, sak, Bd, sbk, sbn, out.view, out.ld, vector(bias) if c.bias else None, c.M, c.N, c.K,
           alpha=c.alpha, relu=c.relu, accumulate=c.accumulate, splits=c.splits, workspace=ws.view if nws else None)
    sync("gemm " + c.name)
    got = out.view.clone()
    intact(out, ws)
    return got


def gemm_ref(c, A, Bm, bias, c0):
    v = c.alpha * (A @ Bm) + (bias if c.bias else 0)
    if c.relu:
        v = torch.relu(v)
    return v + c0 if c.accumulate else v


@pytest.mark.parametrize("c", H.GEMM, ids=[c.name for c in H.GEMM])
def test_gemm(c):
    data = gemm_data(c, "int")
    ref = gemm_ref(c, *data)
    if c.accumulate and c.bias:
        v = c.alpha * (data[0] @ data[1]) + data[2]
        assert bool((v == 0).any()) and bool((v < 0).any())
    exact(gemm_run(c, *data), ref, "gemm " + c.name)
    data = gemm_data(c, "randn")
    one, two = gemm_run(c, *data), gemm_run(c, *data)
    assert torch.equal(one, two), "two runs differ"
    close(one, gemm_ref(c, *data), RTOL, "gemm randn " + c.name)


# ---- coclr_gemm_fused --------------------------------------------------------------------------------------------------

def fused_data(c, kind):
    g = R.gen(c.mode, c.M, c.N, c.K, kind == "int")
    M, N, K = c.M, c.N, c.K
    rnd = lambda *s: torch.randn(*s, generator=g).double()
    d = {}
    if c.mode in (0, 1, 4):
        d["A"], d["B"] = (R.ints((M, K), -3, 3, g), R.ints((K, N), -3, 3, g)) if kind == "int" else (rnd(M, K), rnd(K, N))
        d["bias"] = R.ints((N,), -4, 4, g) if kind == "int" else rnd(N)
        if c.mode == 1:
            d["h"] = R.ints((M, N), -2, 2, g) if kind == "int" else rnd(M, N)
    elif c.mode == 2:
        if kind == "int":
            A = R.unit_rows(M, K, 64, g) * 8 * 2.0 ** (torch.arange(M) % 3).double()[:, None]
            A[1::7] = 0
            Bm = torch.zeros(K, N, dtype=torch.float64)
            Bm[torch.arange(K), torch.randperm(N, generator=g)[:K]] = 1
            d["A"], d["B"] = A, Bm
        else:
            d["A"], d["B"] = rnd(M, K), rnd(K, N)
    else:                                   # mode 3: A = dlogits[:, 1:], B = queue^T, reduction over the queue
        if kind == "int":
            d["dl"] = R.ints((M, 1 + K), -3, 3, g)
            d["queue"] = R.ints((N, K), -3, 3, g)
            d["k"], d["y"] = R.ints((M, N), -1, 1, g) / 8, R.ints((M, N), -1, 1, g) / 8
            d["inv"] = 2.0 ** -(torch.arange(M) % 3).double()
        else:
            d["dl"] = rnd(M, 1 + K)
            d["queue"] = f32t(F.normalize(rnd(N, K), dim=0))
            d["k"], d["y"] = f32t(F.normalize(rnd(M, N), dim=1)), f32t(F.normalize(rnd(M, N), dim=1))
            d["inv"] = f32t(1 / (rnd(M).abs() + 0.5))
    return d


def fused_ref(c, d):
    if c.mode == 3:
        f = 1.0 / c.T
        v = f * (d["dl"][:, 1:] @ d["queue"].t()) + (d["dl"][:, :1] * f) * d["k"]
        dot = (v * d["y"]).sum(1, keepdim=True)
        return dict(c=(v - d["y"] * dot) * d["inv"][:, None])
    s = d["A"] @ d["B"]
    if c.mode == 2:
        eps = float(torch.tensor(1e-12, dtype=torch.float32))
        inv = f32t(1 / torch.clamp(s.norm(dim=1), min=eps))
        return dict(c=s * inv[:, None], inv=inv)
    v = 0.5 * s + d["bias"]
    if c.mode == 0:
        return dict(c=v, rowsum=d["A"].sum(1))
    if c.mode == 1:
        return dict(c=torch.where(d["h"] > 0, v, torch.zeros_like(v)))
    inv = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(c.S), dtype=torch.float32))
    return dict(c=f32t(v * inv)[:, :, None].expand(c.M, c.N, c.S).reshape(c.M, c.N * c.S))


def fused_run(c, d):
    o = ops()
    M, N, K = c.M, c.N, c.K
    ws = Placed2D(1, o.gemm_fused_workspace(M, N, K, c.splits))
    got, guards = {}, [ws]
    if c.mode == 3:
        dl, queue = source2d(d["dl"], c.pad), source2d(d["queue"], c.pad)
        out = Placed2D(M, N, c.pad)
        f = 1.0 / c.T
        o.gemm_fused(dl[:, 1:], dl.stride(0), 1, queue, 1, queue.stride(0), out.view, out.ld, None, M, N, K, alpha=f,
                     splits=c.splits, workspace=ws.view, mode=3, ep_a=dl, lda=dl.stride(0), ep_b=source2d(d["k"]),
                     ep_y=source2d(d["y"]), inv_norm=row(d["inv"]), f=f)
        outs = dict(c=out)
    else:
        Ad, Bd = source2d(d["A"], c.pad, transposed=c.ta), source2d(d["B"], c.pad, transposed=c.tb)
        sam, sak = R.operand_strides(M, K, c.pad, c.ta)
        sbk, sbn = R.operand_strides(K, N, c.pad, c.tb)
        args = lambda out: (Ad, sam, sak, Bd, sbk, sbn, out.view, out.ld)
        if c.mode == 2:
            out, inv = Placed2D(M, N, c.pad), Placed2D(1, M)
            o.gemm_fused(*args(out), None, M, N, K, splits=c.splits, workspace=ws.view, mode=2, out2=inv.view, f=1e-12)
            outs = dict(c=out, inv=inv)
        elif c.mode == 0:
            out, rs = Placed2D(M, N, c.pad), Placed2D(1, M)
            o.gemm_fused(*args(out), vector(d["bias"]), M, N, K, alpha=0.5, splits=1, workspace=None, mode=0,
                         rowsum=rs.view)
            outs = dict(c=out, rowsum=rs)
        elif c.mode == 1:
            out, h = Placed2D(M, N, c.pad), source2d(d["h"], c.pad)
            o.gemm_fused(*args(out), vector(d["bias"]), M, N, K, alpha=0.5, splits=c.splits, workspace=ws.view, mode=1,
                         ep_a=h, lda=h.stride(0))
            outs = dict(c=out)
        else:
            out = Placed2D(M, N * c.S)
            o.gemm_fused(Ad, sam, sak, Bd, sbk, sbn, out.view, N, vector(d["bias"]), M, N, K, alpha=0.5,
                         splits=c.splits, workspace=ws.view, mode=4, S=c.S)
            outs = dict(c=out)
    sync("gemm_fused " + c.name)
    for k, p in outs.items():
        got[k] = p.view.clone().reshape(-1) if k != "c" else p.view.clone()
        guards.append(p)
    intact(*guards)
    return got


@pytest.mark.parametrize("c", H.FUSED, ids=[c.name for c in H.FUSED])
def test_gemm_fused(c):
    for kind in ("int", "randn"):
        d = fused_data(c, kind)
        ref, got = fused_ref(c, d), fused_run(c, d)
        if kind == "int":
            assert all(R.is_fp32(v) for v in ref.values()), "the exact row is not exact"
            if c.mode == 2:
                assert bool((ref["c"].abs().sum(1) == 0).any()) and float(ref["inv"].max()) > 1e11
        else:
            again = fused_run(c, d)
            assert all(torch.equal(got[k], again[k]) for k in got), "two runs differ"
        for k in ref:
            if kind == "randn" and k == "inv":
                close(got[k] * 0 + 1, (got[k].cpu().double() / ref[k]), RTOL, "%s %s %s (ratio)" % (c.name, kind, k))
                continue
            compare(kind, got[k], ref[k], "%s %s %s" % (c.name, kind, k))


@pytest.mark.parametrize("mode", (2, 3))
def test_gemm_fused_rejects_rows_wider_than_a_wave_holds(mode):
    o = ops()
    M, N, K = 4, H.FUSED_REJECTED_N, 8
    z = lambda *s: torch.zeros(*s, device="cuda")
    out = Placed2D(M, N)
    with rejected():
        o.gemm_fused(z(M, K), K, 1, z(K, N), N, 1, out.view, N, None, M, N, K, splits=1, workspace=z(M * N), mode=mode,
                     ep_a=z(M, 1), lda=1, ep_b=z(M, N), ep_y=z(M, N), inv_norm=z(M), f=1.0)
    sync("rejected gemm_fused")
    assert bool(torch.isnan(out.view).all())
    intact(out)


# ---- l2norm ------------------------------------------------------------------------------------------------------------

def l2norm_data(rows, D, kind):
    g = R.gen(rows, D, kind == "int")
    if kind == "int":
        x = R.unit_rows(rows, D, R.nnz_for(D), g) * 2.0 ** (torch.arange(rows) % 3).double()[:, None]
        if rows >= 3:
            x[1] = 0
        return x, R.ints((rows, D), -3, 3, g)
    return torch.randn(rows, D, generator=g).double(), torch.randn(rows, D, generator=g).double()


@pytest.mark.parametrize("rows,D", H.L2NORM, ids=["%dx%d" % c for c in H.L2NORM])
def test_l2norm(rows, D):
    o = ops()
    eps = float(torch.tensor(1e-12, dtype=torch.float32))
    for kind in ("int", "randn"):
        x, dy = l2norm_data(rows, D, kind)
        inv_ref = f32t(1 / torch.clamp(x.norm(dim=1), min=eps))
        y_ref = x * inv_ref[:, None]
        with_inv = D != 63                                  # inv_norm = None on the D = 63 rows
        outs = []
        for _ in range(2):
            y, inv = Placed2D(rows, D), Placed2D(1, rows)
            o.l2norm_fwd(source2d(x), y.view, inv.view[0] if with_inv else None)
            sync("l2norm_fwd")
            outs.append((y.view.clone(), inv.view[0].clone()))
            if not with_inv:
                assert bool(torch.isnan(inv.view).all())
            intact(y, inv)
        assert torch.equal(outs[0][0], outs[1][0])
        compare(kind, outs[0][0], y_ref, "l2norm y %s" % kind)
        if with_inv:
            compare(kind, outs[0][1] if kind == "int" else outs[0][1].cpu().double() / inv_ref,
                    inv_ref if kind == "int" else torch.ones(rows, dtype=torch.float64), "l2norm inv %s" % kind)
        # backward from the forward's (reference) outputs
        yv = f32t(y_ref)
        dot = (dy * yv).sum(1, keepdim=True)
        dx_ref = (dy - yv * dot) * inv_ref[:, None]
        if kind == "int":
            assert R.is_fp32(y_ref) and R.is_fp32(dy - yv * dot)
            dx_ref = f32t(dx_ref)                           # one rounding, by the zero row's inv = fp32(1e12)
        dxs = []
        for _ in range(2):
            dx = Placed2D(rows, D)
            o.l2norm_bwd(source2d(dy), source2d(yv), row(inv_ref), dx.view)
            sync("l2norm_bwd")
            dxs.append(dx.view.clone())
            intact(dx)
        assert torch.equal(dxs[0], dxs[1])
        if kind == "int":
            exact(dxs[0], dx_ref, "l2norm dx int")
        else:
            # dx is a difference of two terms of size |dy| * inv that cancel (completely for D = 1): the roundings
            # are relative to the terms, so that is the scale of the bound, not max|dx|
            scale = float((dy.abs().max(1).values * inv_ref).max())
            err = float((dxs[0].cpu().double() - dx_ref).abs().max())
            print("l2norm dx randn: max abs err %.3e, bound %.3e" % (err, RTOL_BWD * scale))
            assert err <= RTOL_BWD * scale


# ---- logits ------------------------------------------------------------------------------------------------------------

def logits_data(B, K, D, kind):
    g = R.gen(B, K, D, kind == "int")
    if kind == "int":
        return R.head_features(B, K, D, g)
    return (f32t(F.normalize(torch.randn(B, D, generator=g).double(), dim=1)),
            f32t(F.normalize(torch.randn(B, D, generator=g).double(), dim=1)),
            f32t(F.normalize(torch.randn(D, K, generator=g).double(), dim=0)))


def logits_run(q, k, queue, T, shift):
    B, K = q.shape[0], queue.shape[1]
    out = Placed2D(B, 1 + K)
    qd = source2d(q, shift=shift)
    assert qd.data_ptr() % 16 == 4 * shift
    ops().nce_logits_fwd(qd, source2d(k), source2d(queue), out.view, T)
    sync("nce_logits_fwd")
    got = out.view.clone()
    intact(out)
    return got


LOGITS_IDS = ["B%d-K%d-D%d-T%g" % c for c in H.LOGITS + H.LOGITS_OTHER_D]


@pytest.mark.parametrize("B,K,D,T", H.LOGITS + H.LOGITS_OTHER_D, ids=LOGITS_IDS)
def test_logits_forward(B, K, D, T):
    for kind in ("int", "randn"):
        q, k, queue = logits_data(B, K, D, kind)
        if kind == "int":
            ref, _ = R.logits_reference(q, k, queue, T)
        else:
            ref = torch.cat([(q * k).sum(1, keepdim=True), q @ queue], 1) * R.inv_T_of(T)
        paths = [logits_run(q, k, queue, T, 0), logits_run(q, k, queue, T, 1)]     # D = 128: fused, fallback
        again = [logits_run(q, k, queue, T, 0), logits_run(q, k, queue, T, 1)]
        assert torch.equal(paths[0], again[0]) and torch.equal(paths[1], again[1]), "two runs differ"
        for got, what in zip(paths, ("aligned q", "q one float off")):
            compare(kind, got, ref, "logits %s %s" % (kind, what))
            if kind == "int":
                for r in sorted({0, min(32, B - 1), B - 1}):                        # the positive column, by row tile
                    assert float(got[r, 0]) == float(ref[r, 0]), (what, r)
        if kind == "int":
            assert torch.equal(paths[0], paths[1]), "fused kernel and fallback differ"


BWD_IDS = ["B%d-K%d-D%d-s%d" % c for c in H.LOGITS_BWD]


@pytest.mark.parametrize("B,K,D,splits", H.LOGITS_BWD, ids=BWD_IDS)
def test_logits_backward(B, K, D, splits):
    o, T = ops(), 0.125
    for kind in ("int", "randn"):
        _, k, queue = logits_data(B, K, D, kind)
        g = R.gen(B, K, splits, 5)
        dl = R.ints((B, 1 + K), -3, 3, g) if kind == "int" else torch.randn(B, 1 + K, generator=g).double()
        ref = (dl[:, 1:] @ queue.t() + dl[:, :1] * k) / T
        outs = []
        for _ in range(2):
            dq = Placed2D(B, D)
            ws = Placed2D(1, max(1, o.gemm_workspace(B, D, K, splits)))
            o.nce_logits_bwd(source2d(dl), source2d(k), source2d(queue), dq.view, ws.view, T, splits)
            sync("nce_logits_bwd")
            outs.append(dq.view.clone())
            intact(dq, ws)
        assert torch.equal(outs[0], outs[1])
        compare(kind, outs[0], ref, "dq %s" % kind)


# ---- queue -------------------------------------------------------------------------------------------------------------

def enqueue_case(D, K, BW, ptr, writes):
    g = R.gen(D, K, BW)
    queue, keys = R.ints((D, K), -9, 9, g), R.ints((BW, D), 10, 30, g)
    qd = Placed2D(D, K)
    qd.put(queue)
    ops().queue_enqueue(qd.view, source2d(keys), row(torch.tensor([ptr])))
    sync("queue_enqueue")
    if writes:
        queue[:, ptr:ptr + BW] = keys.t()
    exact(qd.view, queue, "queue after enqueue at %d" % ptr)
    intact(qd)


def test_queue_enqueue_every_pointer():
    D, K, BW = H.ENQUEUE_SMALL
    for ptr in range(0, K, BW):
        enqueue_case(D, K, BW, ptr, True)
    enqueue_case(D, K, BW, K - BW + 1, False)       # not a multiple of the batch: the kernel's guard writes nothing
    enqueue_case(D, K, BW, -1, False)


def test_queue_enqueue_grid_stride():
    D, K, BW = H.ENQUEUE_LARGE
    enqueue_case(D, K, BW, BW, True)
    enqueue_case(D, K, BW, K - BW + 1, False)


@pytest.mark.parametrize("K,BW,ptr", H.FILL_I64, ids=["K%d-BW%d-p%d" % c for c in H.FILL_I64])
def test_queue_fill_i64(K, BW, ptr):
    o = ops()
    vals = torch.arange(BW) * 3 + 100
    for v, const in ((vals, 0), (None, 41)):
        q = Placed2D(1, K, fill=-1, dtype=torch.int64)
        want = torch.full((K,), -1, dtype=torch.int64)
        if ptr + BW <= K:
            want[ptr:ptr + BW] = vals if v is not None else const
        o.queue_fill_i64(q.view[0], row(v) if v is not None else None, const, BW, row(torch.tensor([ptr])))
        sync("queue_fill_i64")
        assert torch.equal(q.view[0].cpu(), want)
        intact(q)


@pytest.mark.parametrize("K,BW,ptr,want", H.ADVANCE, ids=["K%d-BW%d-p%d" % c[:3] for c in H.ADVANCE])
def test_queue_advance(K, BW, ptr, want):
    p = Placed2D(1, 1, fill=ptr, dtype=torch.int64)
    ops().queue_advance(p.view[0], BW, K)
    sync("queue_advance")
    assert int(p.view[0, 0]) == want
    intact(p)


# ---- gather / pull -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", H.GATHER, ids=[c.name for c in H.GATHER])
def test_gather_rows(c):
    n, idx = c.row_elems, torch.tensor(H.GATHER_INDEX)
    t = torch.arange(6 * n, dtype=torch.float64).reshape(6, n)
    src = source2d(t, c.stride_extra, c.shift_in)
    out = Placed2D(len(idx), n, 0, c.shift_out)
    assert src.data_ptr() % 16 == 4 * c.shift_in and out.view.data_ptr() % 16 == 4 * c.shift_out
    ops().gather_rows(src, row(idx), out.view)
    sync("gather_rows " + c.name)
    assert torch.equal(out.view.cpu(), t[idx].float())
    intact(out)


@pytest.mark.parametrize("c", H.PULL, ids=[c.name for c in H.PULL])
def test_pull_rows(c):
    n = c.row_elems
    ta = torch.arange(3 * n, dtype=torch.float64).reshape(3, n)
    tb = ta + 3 * n
    a, b = source2d(ta, 4, c.shift_in), source2d(tb, 0, 0)          # two tensors; the rows of one may be off 16 bytes
    picks = [(a, 2), (b, 0), (a, 0), (b, 2), (a, 2)]
    ptrs = torch.tensor([s[i].data_ptr() for s, i in picks], dtype=torch.int64)
    if n % 4 == 0:
        assert any(p % 16 for p in ptrs.tolist()) == bool(c.shift_in)
    out = Placed2D(len(picks), n)
    ops().pull_rows(row(ptrs), out.view, keep=(a, b))
    sync("pull_rows " + c.name)
    want = torch.stack([(ta if s is a else tb)[i] for s, i in picks]).float()
    assert torch.equal(out.view.cpu(), want)
    intact(out)


# ---- relu, colsum ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", H.ELEMENTWISE_N)
def test_relu(n):
    o, g = ops(), R.gen(n)
    x, dy = R.ints((1, n), -3, 3, g), R.ints((1, n), -3, 3, g)
    y, dx = Placed2D(1, n), Placed2D(1, n)
    o.relu_fwd(source2d(x), y.view)
    o.relu_bwd(source2d(dy), source2d(torch.relu(x)), dx.view)
    sync("relu")
    exact(y.view, torch.relu(x), "relu")
    exact(dx.view, dy * (x > 0), "relu backward")
    intact(y, dx)


@pytest.mark.parametrize("rows,cols", H.COLSUM, ids=["%dx%d" % c for c in H.COLSUM])
def test_colsum(rows, cols):
    x = R.ints((rows, cols), -3, 3, R.gen(rows, cols))
    out = Placed2D(1, cols)
    ops().colsum(source2d(x), out.view[0])
    sync("colsum")
    exact(out.view[0], x.sum(0), "colsum")
    intact(out)


# ---- positives ---------------------------------------------------------------------------------------------------------

def new_mask(B, K):
    return Placed2D(B, 1 + K, fill=7, around=200, dtype=torch.uint8)


@pytest.mark.parametrize("c", H.MASK, ids=[c.name for c in H.MASK])
def test_positive_mask_and_mining(c):
    o = ops()
    q, _, queue = R.head_features(c.B, c.K, 128, R.gen(c.B, c.K, c.topk), H.TIE_GROUPS[c.ties])
    sim = q @ queue
    assert R.is_fp32(sim)
    tied = R.tie_columns(H.TIE_GROUPS[c.ties], c.K)
    assert bool((sim[0, tied] == sim[0].max()).all())
    kf, queue2 = source2d(q), source2d(queue)
    workspace = o.mine_workspace(c.B, c.K, c.topk, "cuda")
    for variant in ("mixed", "sparse", "full"):
        src, names = R.names_variant(variant, c.B, c.K, R.gen(c.B, c.K))
        ref = R.mask_reference(sim, src, names, c.topk)
        if variant != "mixed":
            free = (src[:, None] != names[None, :]).sum(1)
            assert int(free[0]) == (min(3, c.K) if variant == "sparse" else 0)
        srcd, namesd = row(src), row(names)
        mask = new_mask(c.B, c.K)
        o.positive_mask(source2d(sim) if c.topk or variant == "mixed" else None, srcd, namesd, mask.view, c.topk)
        sync("positive_mask " + c.name)
        assert torch.equal(mask.view.cpu(), ref), "positive_mask, %s names" % variant
        intact(mask)
        for launch in range(2):                     # twice on one workspace: the counters are left at zero
            mask, sim_out = new_mask(c.B, c.K), Placed2D(c.B, c.K)
            o.mine_positives(kf, queue2, srcd, namesd, mask.view, c.topk, workspace, sim_out=sim_out.view)
            sync("mine_positives " + c.name)
            assert int(workspace[2].abs().sum()) == 0, "row-tile counters not reset"
            exact(sim_out.view, sim, "mined similarities")
            assert torch.equal(mask.view.cpu(), ref), "mine_positives, %s names, launch %d" % (variant, launch)
            intact(mask, sim_out)


@pytest.mark.parametrize("B,D,K,topk", H.MINE_REJECTED, ids=["B%d-D%d-K%d-top%d" % c for c in H.MINE_REJECTED])
def test_mine_positives_rejects(B, D, K, topk):
    o = ops()
    mask = new_mask(B, K)
    z = torch.zeros
    with rejected():
        o.mine_positives(z(B, D, device="cuda"), z(D, K, device="cuda"), z(B, dtype=torch.int64, device="cuda"),
                         z(K, dtype=torch.int64, device="cuda"), mask.view, topk, o.mine_workspace(B, K, topk, "cuda"))
    sync("rejected mine_positives")
    assert bool((mask.view == 7).all())


def test_positive_mask_lds_bound():
    o, B, K = ops(), 2, H.MASK_LDS_K
    g = R.gen(K)
    src = torch.tensor([1, 3])
    names = torch.randint(0, 4, (K,), generator=g)
    mask = new_mask(B, K)
    with rejected():
        o.positive_mask(torch.zeros(B, K, device="cuda"), row(src), row(names), mask.view, 5)
    sync("rejected positive_mask")
    assert bool((mask.view == 7).all())
    o.positive_mask(None, row(src), row(names), mask.view, 0)
    sync("positive_mask without top-k")
    assert torch.equal(mask.view.cpu(), R.mask_reference(None, src, names, 0))
    intact(mask)


# ---- retrieval ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", H.RETRIEVAL, ids=[c.name for c in H.RETRIEVAL])
def test_retrieval_hits(c):
    sim, train, test = R.retrieval_inputs(c.B, c.N, c.ks, R.gen(c.B, c.N, len(c.ks)))
    hits_ref, idx_ref = R.retrieval_reference(sim, train, test, c.ks)
    i = c.ks.index(c.ks[len(c.ks) // 2])
    assert float(hits_ref[0, i]) == 1 and float(hits_ref[1, i]) == 0          # a match at rank k, one at rank k + 1
    hits = Placed2D(c.B, len(c.ks))
    topidx = Placed2D(c.B, c.ks[-1], fill=-7, dtype=torch.int32)
    ops().retrieval_hits(source2d(sim), row(train), row(test), row(torch.tensor(c.ks, dtype=torch.int32)), hits.view,
                         topidx.view)
    sync("retrieval_hits " + c.name)
    assert torch.equal(topidx.view.cpu(), idx_ref), "ordered top-k columns"
    exact(hits.view, hits_ref.double(), "hits")
    intact(hits, topidx)


@pytest.mark.parametrize("rows,cols", H.COLSTATS, ids=["%dx%d" % c for c in H.COLSTATS])
def test_center_rows_and_bn1d_stats(rows, cols):
    o = ops()
    x = R.ints((rows, cols), -4, 4, R.gen(rows, cols, 2))
    x[0] -= x.sum(0) % rows                          # column sums are multiples of `rows`: the mean is an integer
    assert bool((x.sum(0) % rows == 0).all())
    xd = source2d(x)
    out, ws = Placed2D(rows, cols), Placed2D(1, o.colstats_workspace(rows, cols))
    o.center_rows(xd, out.view, ws.view)
    sync("center_rows")
    exact(out.view, x - x.sum(0, keepdim=True) / rows, "centred rows")
    intact(out, ws)
    stats, ws = Placed2D(2, cols), Placed2D(1, o.colstats_workspace(rows, cols))
    o.bn1d_stats(xd, stats.view, ws.view)
    sync("bn1d_stats")
    exact(stats.view, torch.stack([x.sum(0), (x * x).sum(0)]), "column sums and sums of squares")
    intact(stats, ws)
