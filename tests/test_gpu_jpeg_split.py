"""Intra-frame parallel Huffman decoding (csrc/jpeg.hip: jpeg_entropy_split_kernel; coclr_jpeg_decode_split) on one
MI355X against the committed PIL fixture and against the serial kernel, with ZERO tolerance: the chunked decode
relaxes to the serial decoder's own states, so every coefficient, status word and output byte is determined.  No test
imports PIL; only well-formed streams reach the GPU (damaged ones are the host check's:
tests/test_jpeg_split_cpu.py)."""
import pytest
import torch

import _jpeg_cases as J

pytestmark = pytest.mark.gpu

SIZES = (8, 16, 64, 128, 65536)
MIXED = (40, 56, 3, (2, 2))


def _packed(c):
    from coclr_amd import jpeg
    return jpeg.pack([J.raw(c)])[0].numpy()


def _straddling_pairs(chunk_bytes):
    """FF 00 pairs whose FF is a chunk's last byte, over the fixtures without restart markers."""
    count = 0
    for c in J.cases():
        if c["restart_interval"]:
            continue
        b = _packed(c)
        for at in range(chunk_bytes - 1, len(b) - 1, chunk_bytes):
            count += int(b[at] == 0xFF and b[at + 1] == 0)
    return count


@pytest.mark.parametrize("chunk_bytes", SIZES)
def test_every_group_equals_the_fixtures(chunk_bytes):
    """One call per geometry group: frames with and without restart markers side by side (the serial kernel decodes
    the former in the same call), different tables and lengths in one launch."""
    from coclr_amd import jpeg
    for group in J.groups().values():
        got, status = jpeg.decode(*jpeg.pack([J.raw(c) for c in group]), return_status=True, chunk_bytes=chunk_bytes)
        assert status.tolist() == [0] * len(group)
        got = got.cpu()
        for k, c in enumerate(group):
            assert torch.equal(got[k], c["rgb"]), (c["name"], chunk_bytes)
    mixed = {c["name"]: c["restart_interval"] for c in J.groups()[MIXED]}
    assert mixed["56x40_420_rst1"] and mixed["56x40_420_rstrow"]
    assert not mixed["56x40_420_optimize"] and not mixed["56x40_420_q100_noise"]


def test_the_named_edges_are_in_the_fixtures():
    """FF 00 pairs straddle chunk boundaries at the small sizes, and 65536 bytes hold every frame in one chunk (the
    serial case inside the new kernel)."""
    assert _straddling_pairs(8) > 0 and _straddling_pairs(16) > 0 and _straddling_pairs(128) > 0
    assert max(len(_packed(c)) for c in J.cases()) < 65536


def test_mixed_group_equals_one_by_one_decodes():
    from coclr_amd import jpeg
    group = J.groups()[MIXED]
    want = torch.cat([jpeg.decode(*jpeg.pack([J.raw(c)]), chunk_bytes=0).cpu() for c in group])
    for chunk_bytes in (8, 128):
        got = jpeg.decode(*jpeg.pack([J.raw(c) for c in group]), chunk_bytes=chunk_bytes)
        assert torch.equal(got.cpu(), want)
        joined = jpeg.decode(*jpeg.cat([jpeg.pack([J.raw(c)]) for c in group]), chunk_bytes=chunk_bytes)
        assert torch.equal(joined.cpu(), want)


def _coefficients(raws, chunk_bytes):
    """Stage 1 alone into a workspace that sits inside a larger buffer -> (coefficients, guards, status) on the host."""
    from coclr_amd import jpeg, ops
    data, meta = jpeg.pack(raws)
    H, W, ncomp, hs, vs = jpeg.check_meta(data, meta)
    F = meta.shape[0]
    cb, pb = ops.jpeg_workspace(H, W, ncomp, hs, vs)
    n, guard = F * cb // 2, 64
    buf = torch.full((guard + n + guard,), 0x5A5A, dtype=torch.int16, device="cuda")
    coefs = buf[guard:guard + n]
    planes = torch.empty(F * pb, dtype=torch.uint8, device="cuda")
    out = torch.empty(F, H, W, 3, dtype=torch.uint8, device="cuda")
    status = torch.full((F,), -1, dtype=torch.int32, device="cuda")
    host = meta[:, 8:].contiguous()
    ops.jpeg_decode(data.cuda(), host.cuda(), host, H, W, ncomp, hs, vs, coefs, planes, out, status, stages=1,
                    chunk_bytes=chunk_bytes)
    buf = buf.cpu()
    return buf[guard:guard + n], torch.cat([buf[:guard], buf[guard + n:]]), status.cpu()


@pytest.mark.parametrize("which", ["320x240_420_q75 x 64", "56x40 444 group"])
def test_coefficients_equal_the_serial_kernel(which):
    """The inverse DCT's range table could hide a wrong coefficient: compare the int16 workspaces themselves."""
    if which.startswith("320"):
        raws = [J.raw(J.case("320x240_420_q75"))] * 64
    else:
        raws = [J.raw(c) for c in J.groups()[(40, 56, 3, (1, 1))]]
        assert len(raws) >= 2
    want, guards, status = _coefficients(raws, 0)
    assert bool((guards == 0x5A5A).all()) and not status.any() and bool(want.any())
    for chunk_bytes in (128, 16):
        got, guards, st = _coefficients(raws, chunk_bytes)
        assert torch.equal(got, want), chunk_bytes
        assert torch.equal(st, status) and bool((guards == 0x5A5A).all()), chunk_bytes


def test_more_chunks_than_lanes():
    """56x40_444_q100_noise at 8 bytes per chunk has more chunks than a 1024-lane workgroup has lanes: the hand-over
    between windows and the slowest convergence of the fixture set, alone and as frame 2 of 3."""
    from coclr_amd import jpeg
    noise, ramp = J.case("56x40_444_q100_noise"), J.case("56x40_444_q50_ramp")
    assert -(-len(_packed(noise)) // 8) > 1024 >= -(-len(_packed(ramp)) // 8)
    got, status = jpeg.decode(*jpeg.pack([J.raw(noise)]), return_status=True, chunk_bytes=8)
    assert status.tolist() == [0] and torch.equal(got[0].cpu(), noise["rgb"])
    three, status = jpeg.decode(*jpeg.pack([J.raw(ramp), J.raw(noise), J.raw(ramp)]), return_status=True, chunk_bytes=8)
    assert status.tolist() == [0, 0, 0]
    assert torch.equal(three.cpu(), torch.stack([ramp["rgb"], noise["rgb"], ramp["rgb"]]))


def test_small_stage_budget_and_repeatability():
    from coclr_amd import jpeg, ops
    group = J.groups()[MIXED]
    raws = [J.raw(c) for c in group] * 2
    want = torch.cat([c["rgb"][None] for c in group] * 2)
    cb, pb = ops.jpeg_workspace(40, 56, 3, 2, 2)
    assert -(-len(raws) // 3) >= 3
    first = jpeg.decode(*jpeg.pack(raws), max_stage_bytes=3 * (cb + pb), chunk_bytes=16)
    again = jpeg.decode(*jpeg.pack(raws), max_stage_bytes=3 * (cb + pb), chunk_bytes=16)
    assert torch.equal(first.cpu(), want) and torch.equal(again, first)
    assert torch.equal(jpeg.decode_frames(raws, chunk_bytes=64).cpu(), want)


def test_out_into_a_larger_buffer_leaves_the_rest_untouched():
    from coclr_amd import jpeg
    c = J.case("45x37_420_q100_noise")
    H, W = c["height"], c["width"]
    n = 2 * H * W * 3
    buf = (torch.arange(64 + n + 64, dtype=torch.int32) % 251).to(torch.uint8).cuda()
    before = buf.cpu().clone()
    out = buf[64:64 + n].view(2, H, W, 3)
    got = jpeg.decode(*jpeg.pack([J.raw(c)] * 2), out=out, chunk_bytes=64)
    assert got.data_ptr() == out.data_ptr()
    after = buf.cpu()
    assert torch.equal(after[:64], before[:64]) and torch.equal(after[64 + n:], before[64 + n:])
    assert torch.equal(after[64:64 + n].view(2, H, W, 3), torch.stack([c["rgb"], c["rgb"]]))


def test_policy_from_the_environment(monkeypatch):
    """COCLR_JPEG_SPLIT is read per call; which entropy kernel ran shows in nothing but the launch, so the policy is
    observed through ops.jpeg_decode's argument."""
    from coclr_amd import jpeg, ops
    c = J.case("320x240_420_q75")
    data, meta = jpeg.pack([J.raw(c)] * 2)
    seen = []
    real = ops.jpeg_decode

    def spy(*args, **kwargs):
        seen.append(kwargs.get("chunk_bytes"))
        return real(*args, **kwargs)

    monkeypatch.setattr(ops, "jpeg_decode", spy)
    for value, want in (("128", 128), ("0", 0), (None, jpeg.DEFAULT_SPLIT), ("64", 64)):
        if value is None:
            monkeypatch.delenv("COCLR_JPEG_SPLIT", raising=False)
        else:
            monkeypatch.setenv("COCLR_JPEG_SPLIT", value)
        got, status = jpeg.decode(data, meta, return_status=True)
        assert seen[-1] == want
        assert not status.any() and torch.equal(got[0].cpu(), c["rgb"]) and torch.equal(got[1].cpu(), c["rgb"])
        assert jpeg.decode.last_status is not None
    assert torch.equal(jpeg.decode(data, meta, chunk_bytes=0)[1].cpu(), c["rgb"]) and seen[-1] == 0
