"""The JPEG decoder (csrc/jpeg.hip: coclr_jpeg_decode; coclr_amd/jpeg.py) on one MI355X against the committed PIL
fixture (tests/golden/jpeg_frames.pt, tools/make_jpeg_golden.py) with ZERO tolerance: Huffman decoding, the inverse
DCT, the upsampling and the colour conversion are integer arithmetic, so every byte is determined.  No test imports
PIL; only well-formed streams reach the GPU (damaged ones are the host check's, tests/test_jpeg_cpu.py)."""
import pytest
import torch

import _jpeg_cases as J

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def alone():
    """Every fixture decoded in a call of its own, once: name -> (frame on the host, status)."""
    from coclr_amd import jpeg
    out = {}
    for c in J.cases():
        data, meta = jpeg.pack([J.raw(c)])
        frames, status = jpeg.decode(data, meta, return_status=True)
        out[c["name"]] = (frames.cpu(), status.cpu())
    return out


@pytest.mark.parametrize("name", J.names())
def test_fixture_bit_identical(alone, name):
    c = J.case(name)
    frames, status = alone[name]
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (1, c["height"], c["width"], 3)
    assert status.tolist() == [0]
    assert torch.equal(frames[0], c["rgb"])


def test_groups_in_one_call_equal_one_by_one(alone):
    """All fixtures of one (H, W, sampling) -- different tables, quality and restart interval -- in one call,
    once through pack and once through cat of single packs."""
    from coclr_amd import jpeg
    seen = 0
    for group in J.groups().values():
        if len(group) < 2:
            continue
        want = torch.cat([alone[c["name"]][0] for c in group])
        got, status = jpeg.decode(*jpeg.pack([J.raw(c) for c in group]), return_status=True)
        assert torch.equal(got.cpu(), want) and not status.any()
        joined = jpeg.decode(*jpeg.cat([jpeg.pack([J.raw(c)]) for c in group]))
        assert torch.equal(joined.cpu(), want)
        assert torch.equal(jpeg.decode_frames([J.raw(c) for c in group]).cpu(), want)
        seen += 1
    assert seen >= 15
    mixed = [c["name"] for c in J.groups()[(40, 56, 3, (2, 2))]]
    assert "56x40_420_rst1" in mixed and "56x40_420_optimize" in mixed and "56x40_420_q100_noise" in mixed


def test_small_stage_budget_gives_the_same_frames(alone):
    from coclr_amd import jpeg, ops
    group = J.groups()[(40, 56, 3, (2, 2))]
    raws = [J.raw(c) for c in group] * 2
    cb, pb = ops.jpeg_workspace(40, 56, 3, 2, 2)
    budget = 3 * (cb + pb)                                # three frames at a time
    assert -(-len(raws) // 3) >= 3
    got = jpeg.decode(*jpeg.pack(raws), max_stage_bytes=budget)
    want = torch.cat([alone[c["name"]][0] for c in group] * 2)
    assert torch.equal(got.cpu(), want)
    one = jpeg.decode(*jpeg.pack(raws), max_stage_bytes=1)  # less than one frame: still a frame at a time
    assert torch.equal(one.cpu(), want)


@pytest.mark.parametrize("name", ["45x37_420_q100_noise", "16x16_444_q50_ramp"])
def test_out_into_a_larger_buffer_leaves_the_rest_untouched(alone, name):
    from coclr_amd import jpeg
    c = J.case(name)
    H, W = c["height"], c["width"]
    n = 2 * H * W * 3
    buf = (torch.arange(64 + n + 64, dtype=torch.int32) % 251).to(torch.uint8).cuda()
    before = buf.cpu().clone()
    out = buf[64:64 + n].view(2, H, W, 3)
    got = jpeg.decode(*jpeg.pack([J.raw(c)] * 2), out=out)
    assert got.data_ptr() == out.data_ptr()
    after = buf.cpu()
    assert torch.equal(after[:64], before[:64]) and torch.equal(after[64 + n:], before[64 + n:])
    assert torch.equal(after[64:64 + n].view(2, H, W, 3), torch.stack([c["rgb"], c["rgb"]]))
    # an odd offset takes the byte-store path of the 16-pixel groups
    odd = buf[3:3 + n // 2].view(1, H, W, 3)
    jpeg.decode(*jpeg.pack([J.raw(c)]), out=odd)
    again = buf.cpu()
    assert torch.equal(again[:3], before[:3]) and torch.equal(again[3:3 + n // 2].view(H, W, 3), c["rgb"])
    assert torch.equal(again[3 + n // 2:], after[3 + n // 2:])


def test_decoded_frames_feed_stage_crops():
    from coclr_amd import jpeg, staging
    c = J.case("320x240_420_q75")
    F, T = 64, 8
    frames, status = jpeg.decode(*jpeg.pack([J.raw(c)] * F), return_status=True)
    assert tuple(frames.shape) == (F, 240, 320, 3) and not status.any()
    index = torch.arange(F).view(F // T, T)
    boxes = staging.five_crop_boxes(320, 240, 224, where=(5,))
    got = staging.stage_crops(frames, index, boxes, [0], 224, 128)
    want = staging.stage_crops(c["rgb"][None].expand(F, -1, -1, -1).contiguous(), index, boxes, [0], 224, 128)
    assert torch.equal(got, want)
