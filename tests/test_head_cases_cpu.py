"""The case tables of the exact contrastive-head tests (tests/_head_cases.py) reach every launcher branch the head has, and
the references and input generators those tests rely on (tests/_head_ref.py) are right -- without a GPU.

The branch of a row is re-derived with the host predicates of coclr_amd/csrc/nce.hip (launch_gemm, coclr_nce_logits_fwd,
coclr_gather_rows, coclr_pull_rows, coclr_positive_mask), loss.hip and retrieval.hip, restated in tests/_head_ref.py.
Deleting a row that was the only one on a branch fails here."""
import pytest
import torch
import torch.nn.functional as F

import _head_cases as H
import _head_ref as R
import fake_backend
from oracle import coclr_oracle as orc


def gemm_branches():
    out = []
    for c in H.GEMM:
        sam, sak = R.operand_strides(c.M, c.K, c.pad, c.ta)
        sbk, sbn = R.operand_strides(c.K, c.N, c.pad, c.tb)
        out.append((c, R.gemm_branch(c.M, c.N, c.K, sam, sak, sbk, sbn, c.splits)))
    return out


def fused_branches():
    out = []
    for c in H.FUSED:
        sam, sak = R.operand_strides(c.M, c.K, c.pad, c.ta)
        sbk, sbn = R.operand_strides(c.K, c.N, c.pad, c.tb)
        out.append((c, R.gemm_branch(c.M, c.N, c.K, sam, sak, sbk, sbn, c.splits, c.mode, fused=True)))
    return out


def test_names_are_unique():
    for table in (H.GEMM, H.FUSED, H.GATHER, H.PULL, H.MASK, H.RETRIEVAL, H.LOSS):
        names = [c.name for c in table]
        assert len(set(names)) == len(names), names


def test_gemm_rows_reach_every_branch():
    rows = gemm_branches()
    for ta in (False, True):
        for tb in (False, True):
            mine = [(c, b) for c, b in rows if (b["TA"], b["TB"]) == (ta, tb)]
            assert {c.M for c, _ in mine} >= {1, 31, 32, 33, 65}, (ta, tb)
            assert {c.N for c, _ in mine} >= {1, 127, 128, 129, 300}, (ta, tb)
            assert any(c.pad > 0 for c, _ in mine) and any(b["grid"][0] > 1 and b["grid"][1] > 1 for _, b in mine)
    assert {c.K for c, _ in rows} >= {1, 31, 32, 33, 70, 515}
    assert {c.alpha for c, _ in rows} == {1.0, 0.5, 0.125} and all(c.K <= 16384 for c, _ in rows)
    # split-K: a last partial slice, requests that shrink to 2 and to 1, the large-K row
    assert any(b["splits"] > 1 and b["partial_last"] and c.K == 515 and c.splits == 4 for c, b in rows)
    assert any(b["splits"] == 2 and b["partial_last"] and c.K == 70 for c, b in rows)
    assert any(c.K == 40 and c.splits == 4 and b["splits"] == 2 for c, b in rows)
    assert any(c.K == 20 and c.splits == 4 and b["splits"] == 1 and not b["folded"] for c, b in rows)
    assert any((c.M, c.N, c.K, c.splits) == (32, 128, 16384, 128) and b["splits"] == 128 for c, b in rows)
    # accumulate: direct and folded, ReLU on and off
    for folded in (False, True):
        for relu in (False, True):
            assert any(c.accumulate and b["folded"] == folded and c.relu == relu for c, b in rows), (folded, relu)
    assert any(b["fold"] == "plain" and c.bias and c.relu for c, b in rows)


def test_fused_rows_reach_every_branch():
    rows = fused_branches()
    direct = [(c, b) for c, b in rows if c.mode == 0]
    assert all(not b["folded"] and b["splits"] == 1 for _, b in direct)
    assert {(c.M, c.K) for c, _ in direct} >= {(M, K) for M in (31, 33, 65) for K in (5, 70)}
    assert any(b["TA"] for _, b in direct) and any(not b["TA"] for _, b in direct)
    assert any(b["grid"][0] > 1 for _, b in direct)               # only the first tile column writes the row sums
    assert any(c.mode == 1 and b["fold"] == "plain" and c.pad > 0 for c, b in rows)
    assert {c.S for c, b in rows if c.mode == 4 and b["fold"] == "expand"} >= {1, 12}
    for mode in (2, 3):
        mine = [(c, b) for c, b in rows if c.mode == mode]
        assert {c.N for c, _ in mine} >= {64, 128, 129, 200, 512}
        assert {b["RC"] for _, b in mine} == {2, 8} and all(b["fold"] == "rows" for _, b in mine)
        assert any(b["splits"] > 1 and b["partial_last"] for _, b in mine)
    assert {c.T for c, _ in rows if c.mode == 3} == {0.125, 0.0625}
    assert any(c.mode in (1, 2, 4) and b["splits"] == 1 and b["folded"] for c, b in rows)     # fold of ONE partial
    assert H.FUSED_REJECTED_N == 513


def test_logits_and_norm_rows():
    assert {r for r, _ in H.L2NORM} == {1, 3, 4, 5, 33} and {d for _, d in H.L2NORM} == {1, 63, 64, 65, 128, 200}
    assert {(B, K) for B, K, _, _ in H.LOGITS} == {(B, K) for B in (1, 7, 8, 9, 32, 33, 40)
                                                  for K in (1, 63, 64, 65, 640)}
    assert {T for _, _, _, T in H.LOGITS} == {0.07, 0.5}
    assert all(R.logits_branch(D, 0) == "fused" and R.logits_branch(D, 1) == "fallback" for _, _, D, _ in H.LOGITS)
    assert {D for _, _, D, _ in H.LOGITS_OTHER_D} == {64, 96, 256}
    assert all(R.logits_branch(D, 0) == "fallback" for _, _, D, _ in H.LOGITS_OTHER_D)
    assert any(B > 32 for B, _, _, _ in H.LOGITS_OTHER_D)
    assert {(B, K, s) for B, K, _, s in H.LOGITS_BWD} == {(B, K, s) for B in (6, 33) for K in (65, 640) for s in (1, 5)}
    for B, K, D, s in H.LOGITS_BWD:          # the backward's product: A = dlogits[:, 1:], B = queue^T, reduction over K
        b = R.gemm_branch(B, D, K, 1 + K, 1, 1, K, s)
        assert (b["TA"], b["TB"]) == (False, True)
    assert any(R.gemm_branch(B, D, K, 1 + K, 1, 1, K, s)["partial_last"] for B, K, D, s in H.LOGITS_BWD)


def test_queue_and_copy_rows():
    D, K, BW = H.ENQUEUE_SMALL
    assert K % BW == 0 and (K - BW + 1) % BW != 0
    D, K, BW = H.ENQUEUE_LARGE
    assert K % BW == 0 and D * BW > 2048 * 256
    assert any(K % BW != 0 for K, BW, _ in H.FILL_I64) and any(p + BW > K for K, BW, p in H.FILL_I64)
    assert any(BW > 256 for _, BW, _ in H.FILL_I64)
    assert all((p + BW) % K == want for K, BW, p, want in H.ADVANCE) and any(p + BW >= K for K, BW, p, _ in H.ADVANCE)
    g = [(c, R.copy_branch(c.row_elems, c.row_elems + c.stride_extra, c.shift_in, c.shift_out)) for c in H.GATHER]
    assert {c.row_elems for c, _ in g} >= set(H.COPY_SIZES)
    for vector in (False, True):
        for loops in (False, True):
            assert any(b["vector"] == vector and b["loops"] == loops for _, b in g), (vector, loops)
    # sizes that would take the 16-byte path but for the pointers, each pointer alone and both
    sized = [(c, b) for c, b in g if (c.row_elems | (c.row_elems + c.stride_extra)) % 4 == 0]
    assert any(c.shift_in and not c.shift_out and not b["vector"] for c, b in sized)
    assert any(c.shift_out and not c.shift_in and not b["vector"] for c, b in sized)
    assert any(c.shift_in and c.shift_out and not b["vector"] for c, b in sized)
    assert any(c.stride_extra and b["vector"] for c, b in g) and any(c.stride_extra % 4 and c.row_elems % 4 == 0
                                                                     for c, b in g)
    assert len(set(H.GATHER_INDEX)) < len(H.GATHER_INDEX) and list(H.GATHER_INDEX) != sorted(H.GATHER_INDEX)
    p = [(c, R.pull_branch(c.row_elems, c.shift_in)) for c in H.PULL]
    assert {c.row_elems for c, _ in p} >= set(H.COPY_SIZES)
    for vector in (False, True):
        for loops in (False, True):
            assert any(b["vector"] == vector and b["loops"] == loops for _, b in p), (vector, loops)
    assert any(c.shift_in and c.row_elems % 4 == 0 for c, _ in p)
    assert set(H.ELEMENTWISE_N) == {1, 255, 600000} and {c for _, c in H.COLSUM} == {1, 255, 257}


def test_positive_and_retrieval_rows():
    assert {c.B for c in H.MASK} >= {1, 5, 32, 33, 40} and {c.K for c in H.MASK} >= {5, 63, 64, 65, 300, 1030}
    assert {c.topk for c in H.MASK} == {0, 1, 5, 16} and all(c.topk <= min(16, c.K) for c in H.MASK)
    assert {c.ties for c in H.MASK} == set(H.TIE_GROUPS)
    for c in H.MASK:
        cols = R.tie_columns(H.TIE_GROUPS[c.ties], c.K)
        if c.ties == "tiles":
            assert len({x // 64 for x in cols}) == 2
        if c.ties == "octets":
            assert len({x // 64 for x in cols}) == 1 and len({x // 8 for x in cols}) == 2
        if c.ties == "wave":
            assert cols == [255, 256]
        if c.ties == "ends":
            assert cols == [0, c.K - 1]
    assert any(len(R.tie_columns(H.TIE_GROUPS[c.ties], c.K)) > c.topk > 0 for c in H.MASK)
    assert any(c.B > 32 and c.topk > 0 for c in H.MASK) and any(c.K % 64 != 0 and c.K > 64 for c in H.MASK)
    assert sorted(H.MINE_REJECTED) == sorted([(5, 128, 300, 17), (5, 128, 5, 6), (5, 64, 300, 5)])
    assert not R.mask_lds_ok(H.MASK_LDS_K, 5) and R.mask_lds_ok(H.MASK_LDS_K, 0) and R.mask_lds_ok(H.MASK_LDS_K - 1, 5)
    assert {c.N for c in H.RETRIEVAL} == {50, 257, 1000, 38401} and {c.ks for c in H.RETRIEVAL} == {H.KS_FULL, (1,)}
    assert {R.retrieval_use_lds(c.N) for c in H.RETRIEVAL} == {False, True}
    assert all(c.B == 2 for c in H.RETRIEVAL if not R.retrieval_use_lds(c.N))
    assert {r for r, _ in H.COLSTATS} == {1, 63, 64, 65, 300} and {c for _, c in H.COLSTATS} == {1, 257}


def test_loss_rows():
    assert {(c.mode, c.drop_self) for c in H.LOSS} == set(H.LOSS_MODES)
    for m, d in H.LOSS_MODES:
        mine = [c for c in H.LOSS if (c.mode, c.drop_self) == (m, d)]
        assert {c.N1 for c in mine} >= {1, 2, 77, 255, 256, 257, 1025, 2049} and {c.B for c in mine} >= {1, 9, 257}
    assert any(R.cdiv(c.N1, 1024) > 1 and c.N1 > 1024 for c in H.LOSS)        # the backward's grid and stride loop
    # what the generated rows contain
    seen = set()
    for c in H.LOSS:
        lg, pos, target = R.loss_inputs(c.mode, c.drop_self, c.B, c.N1, R.gen(c.mode, c.B, c.N1))
        assert R.is_fp32(lg) and bool(pos.any(1).all())
        r = R.loss_reference(lg, pos, c.mode, c.drop_self)
        if c.mode == 0:
            seen |= {"t0"} if bool((target == 0).any()) else set()
            seen |= {"tlast"} if bool((target == c.N1 - 1).any()) and c.N1 > 256 else set()
            seen |= {"t256"} if bool(((target >= 256) & (target < c.N1 - 1)).any()) else set()
        else:
            n = pos.sum(1)
            seen |= {"lastonly"} if bool(((n == 1) & pos[:, -1]).any()) and c.N1 > 1 else set()
            seen |= {"nomask0"} if bool((~pos[:, 0]).any()) else set()
            if c.drop_self:
                seen |= {"dropped"} if bool(r["drop"].any()) else set()
                seen |= {"kept-single"} if bool(((n == 1) & pos[:, 0] & ~r["drop"]).any()) else set()
                assert not bool((r["drop"] & (n == 1)).any())
        if c.B >= 9:
            assert not bool(R.tie_free(lg).all()) or c.N1 == 1
            assert float(lg.abs().max()) > 500 or c.N1 == 1
    assert seen == {"t0", "tlast", "t256", "lastonly", "nomask0", "dropped", "kept-single"}, seen


# ---- references -------------------------------------------------------------------------------------------------------

def test_ordered_topk_is_topk_without_ties_and_the_stable_sort_with_them():
    g = R.gen(1)
    s = torch.randn(7, 300, generator=g).double()
    for k in (1, 5, 16):
        assert torch.equal(R.ordered_topk(s, k), torch.topk(s, k, dim=1).indices)
    src, names = R.names_variant("mixed", 7, 300, g)
    mask = torch.zeros(7, 301, dtype=torch.uint8)
    fake_backend.positive_mask(s, src, names, mask, 5)
    assert torch.equal(mask, R.mask_reference(s, src, names, 5))
    # tied fixtures: the retrieval double is the stable sort; the mask double uses torch.topk, whose tie order is
    # unspecified, so it must select the same VALUES and the same sibling columns
    for c in H.RETRIEVAL[:3]:
        sim, train, test = R.retrieval_inputs(c.B, c.N, c.ks, R.gen(c.B, c.N, len(c.ks)))
        assert not bool(R.tie_free(sim).any())
        hits, idx = R.retrieval_reference(sim, train, test, c.ks)
        fh, fi = torch.empty_like(hits), torch.empty_like(idx)
        fake_backend.retrieval_hits(sim.float(), train, test, torch.tensor(c.ks), fh, fi)
        assert torch.equal(fh, hits) and torch.equal(fi, idx)
    for c in H.MASK:
        if c.topk == 0 or c.B > 5:
            continue
        q, _, queue = R.head_features(c.B, c.K, 128, R.gen(c.B, c.K, c.topk), H.TIE_GROUPS[c.ties])
        sim = q @ queue
        src, names = R.names_variant("mixed", c.B, c.K, R.gen(c.B, c.K))
        ref = R.mask_reference(sim, src, names, c.topk)
        fake = torch.zeros_like(ref)
        fake_backend.positive_mask(sim, src, names, fake, c.topk)
        assert torch.equal(fake.sum(1), ref.sum(1)), c.name
        same = src[:, None] == names[None, :]
        picked = lambda m: torch.sort(torch.where((m[:, 1:] != 0) & ~same, sim, torch.zeros_like(sim)), 1).values
        assert torch.equal(picked(fake), picked(ref)), c.name


def test_retrieval_fixture_pins_rank_k_and_k_plus_one():
    for c in H.RETRIEVAL:
        if c.N > 1000:
            continue
        sim, train, test = R.retrieval_inputs(c.B, c.N, c.ks, R.gen(c.B, c.N, len(c.ks)))
        hits, idx = R.retrieval_reference(sim, train, test, c.ks)
        kstar = c.ks[len(c.ks) // 2]
        i = c.ks.index(kstar)
        assert hits[0, i] == 1 and (i == 0 or hits[0, i - 1] == 0)
        assert hits[1, i] == 0 and (i + 1 == len(c.ks) or hits[1, i + 1] == 1)
        for k in c.ks:                        # ties across the pick boundary of every k, in some row
            if k < c.N:
                v = torch.sort(sim, 1, descending=True).values
                assert bool((v[:, k - 1] == v[:, k]).any()), (c.name, k)


def test_loss_reference_is_the_reference_losses():
    for c in H.LOSS:
        if c.B > 9:
            continue
        lg, pos, target = R.loss_inputs(c.mode, c.drop_self, c.B, c.N1, R.gen(c.mode, c.B, c.N1))
        small = lg.abs().max(1).values < 100           # the softmax forms underflow to log(0) on the scaled rows
        r = R.loss_reference(lg, pos, c.mode, c.drop_self)
        if c.mode == 0:
            want = F.cross_entropy(lg, target, reduction="none")
            assert torch.allclose(r["loss"], want, rtol=1e-12, atol=1e-12)
            acc = orc.calc_topk_accuracy(lg, target, (1, 5)) if c.N1 >= 5 else None
        elif c.mode == 2:
            want = -(F.log_softmax(lg, 1) * pos).sum(1) / pos.sum(1)
            assert torch.allclose(r["loss"], want, rtol=1e-12, atol=1e-12)
            assert abs(float(orc.ubernce_loss(lg, pos.double())) - float(r["loss"].mean())) < 1e-9
            acc = None
        else:
            want = -torch.log((F.softmax(lg, 1) * r["eff"]).sum(1))
            assert torch.allclose(r["loss"][small], want[small], rtol=1e-12, atol=1e-12)
            if bool(small.all()):
                assert abs(float(orc.multi_nce_loss(lg, r["eff"].double())) - float(r["loss"].mean())) < 1e-9
            acc = None
        # on tie-free rows the rank rule is the reference's top-k accuracy
        free = R.tie_free(lg)
        if c.N1 >= 5 and bool(free.any()):
            x = lg[free]
            if c.mode == 0:
                a1, a5 = orc.calc_topk_accuracy(x, target[free], (1, 5))
            else:
                a1, a5 = orc.calc_mask_accuracy(x, pos[free].long(), (1, 5))
            assert abs(float(a1) - float(r["hits"][free, 0].mean())) < 1e-6
            assert abs(float(a5) - float(r["hits"][free, 1].mean())) < 1e-6
            s1, s5 = orc.calc_topk_accuracy(x, torch.zeros(len(x), dtype=torch.long), (1, 5))
            assert abs(float(s1) - float(r["hits"][free, 2].mean())) < 1e-6
            assert abs(float(s5) - float(r["hits"][free, 3].mean())) < 1e-6
        del acc


def test_rank_rule_on_tie_free_rows():
    """The grid rows all tie; the rank rule against the reference's accuracies on random rows of the same shapes."""
    g = R.gen(3)
    for N1 in (5, 77, 257):
        lg = torch.randn(9, N1, generator=g).double()
        pos = torch.rand(9, N1, generator=g) < 0.05
        pos[:, 0] = True
        r = R.loss_reference(lg, pos, 1, False)
        a1, a5 = orc.calc_mask_accuracy(lg, pos.long(), (1, 5))
        s1, s5 = orc.calc_topk_accuracy(lg, torch.zeros(9, dtype=torch.long), (1, 5))
        got = r["hits"].mean(0)
        assert torch.allclose(got, torch.stack([a1, a5, s1, s5]).double(), atol=1e-6)


def test_exact_inputs_are_exact():
    for c in H.GEMM:
        g = R.gen(c.M, c.N, c.K)
        A, Bm = R.ints((c.M, c.K), -3, 3, g), R.ints((c.K, c.N), -3, 3, g)
        assert float((A.abs() @ Bm.abs()).max()) < 2 ** 24
        ref = c.alpha * (A @ Bm)
        assert R.is_fp32(ref)
    for B, K, D, T in H.LOGITS + H.LOGITS_OTHER_D:
        q, k, queue = R.head_features(B, K, D, R.gen(B, K, D))
        n = R.nnz_for(D)
        ref, s = R.logits_reference(q, k, queue, T)
        assert R.is_fp32(q) and R.is_fp32(queue) and R.is_fp32(s) and R.is_fp32(ref)
        assert bool(((s * n).round() == s * n).all()) and bool(((q * q).sum(1) == 1).all())
        if K >= 63:
            assert not bool(R.tie_free(s[:, 1:]).any())
    for c in H.RETRIEVAL[:3]:
        assert R.is_fp32(R.retrieval_inputs(c.B, c.N, c.ks, R.gen(c.B, c.N, len(c.ks)))[0])
