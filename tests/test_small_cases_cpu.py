"""The case tables of the exact optimiser / global-pool / self-gating tests (tests/_small_cases.py) reach every launcher
branch those kernels have, and the references those tests rely on are right -- without a GPU.

The branch of a row is re-derived with the host predicates of coclr_amd/csrc/optim.hip (16-byte lanes or the scalar loop,
the `cnt & 3` tail, the passes of each loop), pool.hip (a wave per plane; the capped grid of the backward) and nce.hip
(grid1d; four planes per workgroup), restated in tests/_small_cases.py.  Deleting a row that was the only one on a branch
fails here.  Every reference is checked against an independent float64 formulation: autograd for the average pool and
the gating chain, a plain Adam loop written from torch's documented recurrence."""
import math

import torch

import _small_cases as S
from _exact import f32

CHUNK = S.CHUNK


def test_names_are_unique_and_the_chunk_is_the_librarys():
    for table in (S.MOMENTUM, S.ADAM, S.BOUNDED, S.POOL_FWD, S.POOL_BWD, S.PLANES):
        names = [c.name for c in table]
        assert len(set(names)) == len(names), names
    from coclr_amd import optim
    from coclr_amd.model import pretrain
    assert optim._CHUNK == pretrain._CHUNK == CHUNK
    assert S.chunks(CHUNK) == [(0, CHUNK)] and S.chunks(CHUNK + 1) == [(0, CHUNK), (CHUNK, 1)]
    assert S.chunks(2 * CHUNK + 4) == [(0, CHUNK), (CHUNK, CHUNK), (2 * CHUNK, 4)]


# ---- branches ------------------------------------------------------------------------------------------------------------

def test_momentum_rows_reach_every_branch():
    single = [c for c in S.MOMENTUM if len(c.tensors) == 1 and c.tensors[0].count <= CHUNK]
    for n in (1, 3, 4, 5, 255, 1027, CHUNK - 1, CHUNK):
        mine = [c for c in single if c.tensors[0].count == n]
        assert {(c.tensors[0].dst_shift, c.tensors[0].src_shift) for c in mine} == set(S.SHIFTS2), n
        assert {c.m for c in mine} == {0.999, 0.5}, n
    rows = [(c, b) for c in S.MOMENTUM for b in S.momentum_branches(c)]
    for vector in (False, True):
        assert {c.m for c, b in rows if b["vector"] == vector} == {0.999, 0.5}
    # an unaligned dst alone, an unaligned src alone: each sends the row to the scalar loop
    for c in single:
        t, b = c.tensors[0], S.momentum_branches(c)[0]
        assert b["vector"] == (t.dst_shift == 0 and t.src_shift == 0)
    assert any(b["vector"] and b["n4"] == 0 and b["tail"] > 0 for _, b in rows)         # fewer than four elements
    assert {b["tail"] for _, b in rows if b["vector"] and b["n4"] > 0} == {0, 1, 3}     # the cnt & 3 tail
    assert any(b["vector"] and b["vector_passes"] > 1 for _, b in rows)
    assert any(not b["vector"] and b["tail_passes"] > 1 for _, b in rows)
    assert any(not b["vector"] and b["tail"] == 1 for _, b in rows)
    mixed = [c for c in S.MOMENTUM if len({b["vector"] for b in S.momentum_branches(c)}) == 2]
    assert mixed and len(mixed[0].tensors) >= 4                                         # one table, both kinds of row
    assert any(len(S.chunks(t.count)) == 3 for c in S.MOMENTUM for t in c.tensors)
    assert any(len(S.chunks(t.count)) == 3 and t.dst_shift and t.src_shift for c in S.MOMENTUM for t in c.tensors)


def test_adam_rows_reach_every_branch():
    rows = [(c, b) for c in S.ADAM for b in S.adam_branches(c)]
    aligned = [c for c in S.ADAM if len(c.params) == 1 and S.adam_vector(c.params[0])]
    assert {c.params[0].count for c in aligned} == {1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 3, 2 * CHUNK + 4}
    vec = [b for _, b in rows if b["vector"]]
    assert {b["tail"] for b in vec if b["n4"] > 0} == {0, 1, 3}                         # the cnt & 3 tail
    assert {b["tail"] for b in vec if b["n4"] == 0} == {1, 3}
    assert {4 * b["n4"] + b["tail"] for b in vec} >= {CHUNK - 1, CHUNK, 1, 3, 4}        # rows of CHUNK - 1, CHUNK, 1 more, 3 more
    assert any(b["vector_passes"] > 1 for b in vec) and any(b["chunk"] == 2 for b in vec)
    # each of p, g, m, v, k alone off a 16-byte boundary: the scalar loop, at a size the float4 loop would take and at
    # one that needs several passes and a second table row
    for name in S.POINTERS:
        mine = [c for c in S.ADAM if len(c.params) == 1 and c.params[0].shifts == S.alone(name)]
        assert {c.params[0].count for c in mine} == {4, CHUNK + 3}, name
        for c in mine:
            assert not S.adam_vector(c.params[0]) and (name != "k" or c.params[0].key)
            assert all(not b["vector"] and b["n4"] == 0 for b in S.adam_branches(c))
    assert any(not b["vector"] and b["tail_passes"] > 1 for _, b in rows)
    # an unaligned k of a row that has NO key tensor is not looked at: the table holds 0 there
    assert S.adam_vector(S.AdamP(4, 0, S.alone("k"), False, 0.0))
    # hyper rows and step counters: slots other than 0, three learning rates in one launch, slot 0 among them
    assert all(p.slot != 0 for c in S.ADAM if len(c.params) == 1 for p in c.params)
    many = [c for c in S.ADAM if len({S.lr_of(p.slot) for p in c.params}) >= 3]
    assert many and any(p.slot == 0 for c in many for p in c.params)
    assert len({S.lr_of(s) for s in range(8)}) == 8
    # every launch names a strict subset of the slots, and never only a leading run of them
    for c in S.ADAM:
        out = S.outside_slots(c)
        assert out and len(out) < c.nslots, c.name
        assert len({p.slot for p in c.params}) == len(c.params)
    assert any(min(S.outside_slots(c)) < max(p.slot for p in c.params) for c in S.ADAM)
    # the folded key update: present and absent in ONE launch, on both loops, with an unaligned key
    assert any({p.key for p in c.params} == {False, True} for c in S.ADAM)
    for vector in (False, True):
        assert any(b["key"] and b["vector"] == vector for _, b in rows)
        assert any(not b["key"] and b["vector"] == vector for _, b in rows)
        assert any(b["wd"] and b["vector"] == vector for _, b in rows)
    assert any({p.wd != 0 for p in c.params} == {False, True} for c in S.ADAM)           # both sides of wd != 0, one launch
    # bounded rows: a step counter other than the first, both loops, the lr change, with and without decay
    assert {bp.count for bp in S.BOUNDED_PARAMS} == {5, CHUNK + 3}
    assert {all(v == 0 for v in bp.shifts) for bp in S.BOUNDED_PARAMS} == {False, True}
    assert any(bp.start_step == 7 for bp in S.BOUNDED_PARAMS) and any(bp.start_step == 0 for bp in S.BOUNDED_PARAMS)
    assert [(c.lr, c.betas, c.eps, c.wd) for c in S.BOUNDED] == [
        (1e-3, (0.9, 0.999), 1e-8, 1e-5), (1e-3, (0.9, 0.999), 1e-8, 0.0), (3e-2, (0.8, 0.95), 1e-3, 1e-2)]
    assert S.BOUNDED_STEPS == 10 and S.bounded_lr(S.BOUNDED[0], 4) == 1e-3 != S.bounded_lr(S.BOUNDED[0], 5)


def test_pool_rows_reach_every_branch():
    exact = [c for c in S.POOL_FWD if not c.random]
    assert {(c.planes, c.S) for c in exact} == {(p, s) for p in (1, 3, 4, 5, 9) for s in (1, 2, 63, 64, 65, 98, 128, 1000)}
    b = [S.wave_per_plane_branch(c.planes, c.S) for c in exact]
    assert {x["last_waves"] for x in b} == {1, 3, 4} and {x["blocks"] for x in b} == {1, 2, 3}
    assert any(x["idle_lanes"] for x in b) and any(x["per_lane"] == 1 and not x["ragged"] for x in b)
    assert any(x["per_lane"] > 1 and x["ragged"] for x in b) and any(x["per_lane"] == 2 and not x["ragged"] for x in b)
    assert [(c.planes, c.S) for c in S.POOL_FWD if c.random] == [(5, 1000)]
    small = [c for c in S.POOL_BWD if c.planes < 100]
    assert {c.S for c in small} == {1, 3, 64, 98} and {c.planes for c in small} >= {1, 3, 5}
    assert all(not S.pool_bwd_branch(c.planes, c.S)["strided"] for c in small)
    assert any(S.pool_bwd_branch(c.planes, c.S)["blocks"] > 1 for c in small)
    big = [c for c in S.POOL_BWD if S.pool_bwd_branch(c.planes, c.S)["strided"]]
    assert [(c.planes, c.S) for c in big] == [(1030, 513)] and 1030 * 513 == 528390 > 2048 * 256
    x = S.pool_bwd_branch(1030, 513)
    assert x["crosses"] and x["blocks"] == 2048 and x["partial_last"]


def test_gating_rows_reach_every_branch():
    assert {(c.N, c.C, c.S) for c in S.PLANES} == {(n, ch, s) for n, ch in ((1, 1), (1, 3), (2, 2), (1, 5), (3, 3))
                                                   for s in (1, 63, 64, 65, 70)}
    assert {c.N * c.C for c in S.PLANES} == {1, 3, 4, 5, 9}
    b = [S.wave_per_plane_branch(c.N * c.C, c.S) for c in S.PLANES]
    assert {x["last_waves"] for x in b} == {1, 3, 4}                  # a last workgroup of fewer than four planes
    assert any(x["blocks"] == 3 for x in b)
    assert any(x["idle_lanes"] for x in b) and any(x["per_lane"] == 2 and x["ragged"] for x in b)
    assert any(x["per_lane"] == 1 and not x["ragged"] for x in b)
    assert any(c.N > 1 and c.C > 1 for c in S.PLANES)                 # a padded sample stride is only seen with N > 1
    assert len(set(S.SCALE_VARIANTS)) == 16 and len(set(S.DOT_VARIANTS)) == 4
    assert any(v.accumulate and v.bias and v.out_slice and v.a_slice for v in S.SCALE_VARIANTS)
    assert S.SLICE["extra"] >= 2 and S.SLICE["pad"] % 4 != 0
    # sigmoid: the sizes around one workgroup; 70 000 elements do NOT reach the grid-stride loop (grid1d caps at 2048
    # workgroups of 256), the last row does
    assert set(S.SIGMOID_N) >= {1, 255, 256, 257, 70000}
    assert S.grid1d(1) == 1 and S.grid1d(256) == 1 and S.grid1d(257) == 2 and S.grid1d(10 ** 7) == 2048
    assert S.grid1d(70000) == 274 and not S.elementwise_branch(70000)["strided"]
    strided = [n for n in S.SIGMOID_N if S.elementwise_branch(n)["strided"]]
    assert len(strided) == 1 and S.elementwise_branch(strided[0])["partial_last"] and 4 * strided[0] < 2.2e6
    for n in S.SIGMOID_N:
        s = S.sigmoid_args(n)
        assert S.is_fp32(s[s == s]) and s.numel() == n
        if n >= 255:
            for v in S.SIGMOID_FIXED:
                assert bool((s != s).any()) if v != v else bool((s == v).any()), (n, v)
            assert float(s[s == s].abs().clamp(max=20).max()) > 19 and bool(((s > -20) & (s < -10)).any())


def test_print_the_branches(capsys):
    """The list docs/history.md quotes."""
    def count(rows, **want):
        return sum(all(b[k] == v for k, v in want.items()) for b in rows)
    mom = [b for c in S.MOMENTUM for b in S.momentum_branches(c)]
    adam = [b for c in S.ADAM for b in S.adam_branches(c)]
    with capsys.disabled():
        print()
        for name, rows in (("momentum", mom), ("adam", adam)):
            print("%s: %d table rows; float4 loop %d (tail 0/1/2/3: %s, several passes %d), scalar loop %d (several "
                  "passes %d)" % (name, len(rows), count(rows, vector=True),
                                  "/".join(str(sum(b["vector"] and b["tail"] == t for b in rows)) for t in range(4)),
                                  sum(b["vector_passes"] > 1 for b in rows), count(rows, vector=False),
                                  sum(not b["vector"] and b["tail_passes"] > 1 for b in rows)))
        print("adam: key rows %d, weight-decay rows %d, slots named %s" % (
            count(adam, key=True), count(adam, wd=True), sorted({b["slot"] for b in adam})))
        for name, rows in (("avgpool fwd", [(c.planes, c.S) for c in S.POOL_FWD]),
                           ("plane_scale / plane_dot", [(c.N * c.C, c.S) for c in S.PLANES])):
            b = [S.wave_per_plane_branch(p, s) for p, s in rows]
            print("%s: %d rows; waves in the last workgroup %s, elements per lane %s, S %% 64 != 0 in %d" % (
                name, len(b), sorted({x["last_waves"] for x in b}), sorted({x["per_lane"] for x in b}),
                sum(x["ragged"] for x in b)))
        b = [S.pool_bwd_branch(c.planes, c.S) for c in S.POOL_BWD]
        print("avgpool bwd: %d rows; grid-stride loop %d (plane boundary inside a stride %d)" % (
            len(b), sum(x["strided"] for x in b), sum(x["crosses"] for x in b)))
        print("sigmoid: n %s; workgroups %s; grid-stride loop at n = %s" % (
            list(S.SIGMOID_N), [S.grid1d(n) for n in S.SIGMOID_N],
            [n for n in S.SIGMOID_N if S.elementwise_branch(n)["strided"]]))


# ---- references ----------------------------------------------------------------------------------------------------------

def test_momentum_reference_is_the_fp32_tensor_expression():
    for c in S.MOMENTUM:
        for d, s in S.momentum_inputs(c):
            assert S.is_fp32(d) and S.is_fp32(s)
            assert torch.equal(S.momentum_reference(d, s, c.m).float(), S.momentum_cpu32(d, s, c.m)), c.name


def test_adam_exact_rows_are_exact():
    """The closed form of the exact rows IS the float64 recurrence, every value an fp32 value: no rounding anywhere."""
    seen = set()
    for c in S.ADAM:
        for i, p_ in enumerate(c.params):
            p, g, k = S.adam_exact_inputs(c, i)
            lr = S.lr_of(p_.slot)
            assert all(S.is_fp32(t) for t in (p, g, k)) and math.log2(lr) == round(math.log2(lr))
            assert bool((g != 0).all()) and bool((torch.log2(g.abs()) == torch.log2(g.abs()).round()).all())
            assert bool(((p / lr) == (p / lr).round()).all()) and float((p / lr).abs().max()) <= 2 ** 18
            pn, m, v, kn = S.adam_exact_expected(c, i, p, g, k)
            g2 = g + p_.wd * p
            assert bool((g2 != 0).all()) and bool((torch.log2(g2.abs()) == torch.log2(g2.abs()).round()).all())
            rp, rm, rv = S.adam_reference(p, g, torch.zeros_like(p), torch.zeros_like(p), 0, lr, S.EXACT_BETAS,
                                          S.EXACT_EPS, p_.wd)
            assert torch.equal(rp, pn) and torch.equal(rm, m) and torch.equal(rv, v), c.name
            assert all(S.is_fp32(t) for t in (pn, m, v, kn))
            assert torch.equal(pn, p - lr * torch.sign(g2)) and bool((pn != p).all())
            assert torch.equal(kn.float(), S.momentum_cpu32(k, pn, S.FOLD_M))
            if p_.wd != 0:
                seen |= {float(x) for x in (g2 / g).unique()}
            elif p_.count >= 255:
                assert {float(x) for x in torch.sign(g).unique()} == {-1.0, 1.0}
    assert seen == {2.0, 0.5, -1.0}         # the decayed gradient doubles, halves, changes sign


def _documented_adam(p, g, m, v, t, lr, betas, eps, wd):
    """torch.optim.Adam's documented recurrence, step t (1-based), float64 throughout."""
    b1, b2 = betas
    if wd != 0:
        g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    mhat, vhat = m / (1 - b1 ** t), v / (1 - b2 ** t)
    return p - lr * mhat / (vhat.sqrt() + eps), m, v


def test_adam_reference_is_the_documented_recurrence():
    """The two differ by the seven scalars the reference rounds to fp32 (2^-24 relative each); the recurrence is linear
    in all of them, so ten steps stay far inside 1e-6 of each tensor's maximum."""
    for c in S.BOUNDED:
        ref = S.bounded_reference(c)
        for bp, (p0, m0, v0, grads), traj in zip(S.BOUNDED_PARAMS, S.bounded_inputs(c), ref):
            p, m, v = p0.double(), m0.double(), v0.double()
            if bp.start_step:
                assert float(m.abs().max()) > 0 and float(v.min()) > 0
            for step in range(S.BOUNDED_STEPS):
                p, m, v = _documented_adam(p, grads[step].double(), m, v, bp.start_step + step + 1,
                                           S.bounded_lr(c, step), c.betas, c.eps, c.wd)
                for got, want in zip(traj[step], (p, m, v)):
                    assert S.relative_error(got, want) <= 1e-6, (c.name, step)
            assert not torch.equal(traj[-1][0], p0.double())
    # and against torch's own implementation in float64 on the host
    c = S.BOUNDED[2]
    (_, _, _, _), (p0, m0, v0, grads) = S.bounded_inputs(c)
    w = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([w], lr=c.lr, betas=c.betas, eps=c.eps, weight_decay=c.wd, foreach=False)
    for step in range(S.BOUNDED_STEPS):
        opt.param_groups[0]["lr"] = S.bounded_lr(c, step)
        w.grad = grads[step].double()
        opt.step()
    assert S.relative_error(w.detach(), S.bounded_reference(c)[1][-1][0]) <= 1e-6


def test_pool_references_are_the_mean_and_its_gradient():
    for c in S.POOL_FWD:
        x = S.pool_fwd_inputs(c)
        assert S.is_fp32(x) and x.shape == (1, c.planes, 1, 1, c.S)
        if not c.random:
            assert float(x.abs().max()) <= 8 and bool((x == x.round()).all())
            # CPU fp32: the exact sum, one division
            assert torch.equal(S.pool_fwd_reference(x).float(), x.float().sum((2, 3, 4), keepdim=True) / float(c.S))
        xa = x.clone().requires_grad_(True)
        y = xa.mean((2, 3, 4), keepdim=True)
        assert S.relative_error(S.pool_fwd_reference(x), y.detach()) <= 2.0 ** -24
    for c in S.POOL_BWD:
        dy = S.pool_bwd_inputs(c)
        xa = torch.zeros(1, c.planes, 1, 1, c.S, dtype=torch.float64, requires_grad=True)
        xa.mean((2, 3, 4), keepdim=True).backward(dy)
        ref = S.pool_bwd_reference(dy, c.S)
        assert ref.shape == xa.grad.shape and S.is_fp32(ref)
        assert S.relative_error(ref, xa.grad) <= 2.0 ** -23          # two roundings
        assert torch.equal(ref[..., :1].float(), dy.float() * (torch.tensor(1.0) / float(c.S)))   # CPU fp32


def test_gating_references_compose_to_the_reference_module():
    """out = x * sigmoid(fc(mean x)) (backbone/s3dg.py:68-78) and its gradients, assembled from the references the way
    engine.self_gating assembles the kernels, against float64 autograd."""
    g = S.gen(7)
    for c in S.PLANES:
        if c.S < 63:
            continue
        N, C, Sp = c.N, c.C, c.S
        x, _, _, dout = S.plane_scale_inputs(c)
        Wt, bias = S.grid64((C, C), g) / 4, S.grid64((C,), g) / 4
        a = S.pool_fwd_reference(x).view(N, C)
        s = f32(a @ Wt.t() + bias)
        w = f32(S.sigmoid_reference(s))
        out = S.plane_scale_reference(x, w, None, None, S.ScaleV(False, False, False, False))
        dw = S.plane_dot_reference(f32(dout), x)
        ds = S.sigmoid_bwd_reference(f32(dw), w)
        back = f32((ds @ Wt) / Sp)
        dx = S.plane_scale_reference(dout, w, back, None, S.ScaleV(False, False, True, False))
        xa, Wa, ba = (t.clone().requires_grad_(True) for t in (x, Wt, bias))
        ref = xa * torch.sigmoid(xa.mean((2, 3, 4)) @ Wa.t() + ba)[:, :, None, None, None]
        ref.backward(dout)
        for got, want in ((out, ref.detach()), (dx, xa.grad), (ds.t() @ a, Wa.grad), (ds.sum(0), ba.grad)):
            assert S.relative_error(got, want) <= 1e-5, c.name


def test_plane_inputs_are_exact():
    for c in S.PLANES:
        a, gain, bias, out0 = S.plane_scale_inputs(c)
        for t in (a, gain, bias, out0):
            assert bool(((t * 64) == (t * 64).round()).all()) and float(t.abs().max()) <= 4
        for v in S.SCALE_VARIANTS:
            exact = a * gain[:, :, None, None, None] + (bias[:, :, None, None, None] if v.bias else 0)
            exact = exact + out0 if v.accumulate else exact
            assert torch.equal(S.plane_scale_reference(a, gain, bias, out0, v), exact)      # nothing is rounded away
        a, b = S.plane_dot_inputs(c)
        assert float((a.abs() * b.abs()).sum((2, 3, 4)).max()) < 2 ** 24 and S.is_fp32(S.plane_dot_reference(a, b))


def test_sigmoid_reference_classes_and_ulps():
    s = torch.tensor(S.SIGMOID_FIXED, dtype=torch.float64)
    nan, one, tiny, rest = S.sigmoid_classes(s)
    assert s[tiny].tolist() == [-88.0, -89.0, -104.0, -S.INF] and s[one].tolist() == [S.INF] and int(nan.sum()) == 1
    assert s[rest].tolist() == [0.0, 1.0, -1.0, 16.5, -16.5, 88.0, 89.0, 104.0]
    fin = s[rest]
    textbook = 1 / (1 + torch.exp(-fin))
    assert float(((S.sigmoid_reference(fin) - textbook).abs() / textbook).max()) <= 1e-15
    assert float(S.sigmoid_reference(torch.tensor([-87.0], dtype=torch.float64))) > S.TINY
    # the unit: the fp32 spacing at the reference
    ref = torch.tensor([1.0, 0.75, 0.5, 2.0 ** -126, 1.5 * 2.0 ** -100], dtype=torch.float64)
    nxt = torch.nextafter(ref.float(), torch.tensor(2.0)).double()
    assert S.ulp_error(nxt, ref).tolist() == [1.0] * 5 and S.ulp_error(ref, ref).tolist() == [0.0] * 5
    # the backward against autograd
    for n in (255, 257):
        args = S.sigmoid_args(n)
        args = args[torch.isfinite(args)]
        w = f32(S.sigmoid_reference(args))
        dw = S.sigmoid_bwd_inputs(args.numel())
        sa = args.clone().requires_grad_(True)
        torch.sigmoid(sa).backward(dw)
        # w is rounded (2^-25 near 1, where 1 - w loses its relative accuracy): absolute, against the largest gradient
        assert S.relative_error(S.sigmoid_bwd_reference(dw, w), sa.grad) <= 1e-6
