"""The five/ten-crop staging kernel (csrc/staging.hip: coclr_stage_crops) on one MI355X: against the committed
PIL fixture (tests/golden/stage_crops.pt, tools/make_stage_crops_golden.py) and the CPU integer restatement of
tests/crops_harness.py, with ZERO tolerance -- the resampling is integer arithmetic and the float step is two
correctly rounded divisions and a subtraction per element, so every bit is determined -- and
VideoEvaluator.add_frames against staging the same crops by hand.  No test imports PIL."""
import numpy as np
import pytest
import torch

import crops_harness as CH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return CH.golden()


@pytest.fixture(scope="module")
def big():
    """One 256 x 340 frame and its ten 224 -> 128 crops from the CPU restatement, computed once."""
    from coclr_amd import staging
    frame = np.random.RandomState(3).randint(0, 256, size=(1, 256, 340, 3)).astype(np.uint8)
    frame[0, ::2, 100:200] = 255
    frame[0, 1::2, 100:200] = 0
    boxes = staging.five_crop_boxes(340, 256, 224) * 2
    flips = [0] * 5 + [1] * 5
    want = CH.reference(frame, [[0]], [(x0, y0, f) for (x0, y0), f in zip(boxes, flips)], 224, 224, 128)
    return torch.from_numpy(frame), boxes, flips, want


@pytest.mark.parametrize("name", ["A", "B_rect", "B_identity"])
def test_fixture_cases_bit_identical(golden, name):
    from coclr_amd import staging
    c = golden[name]
    want = CH.golden_expected(c, golden["levels"])
    boxes, flips = c["boxes"].tolist(), c["flips"].tolist()
    host = staging.stage_crops(c["frames"], c["frame_index"], boxes, flips, c["crop"], c["S"])
    dev = staging.stage_crops(c["frames"].cuda(), c["frame_index"], boxes, flips, c["crop"], c["S"])
    assert host.is_cuda and host.dtype == torch.float32 and host.shape == want.shape
    assert torch.equal(host.cpu(), want)
    assert torch.equal(dev, host)
    if name == "B_identity":                     # a 16 -> 16 resize returns the source bytes
        x0, y0 = boxes[0]
        src = CH.normalise(c["frames"][0, y0:y0 + 16, x0:x0 + 16].numpy()).permute(2, 0, 1)
        assert torch.equal(host[0, 0, :, 0].cpu(), src)


def test_production_size_equals_the_restatement(big):
    from coclr_amd import staging
    frame, boxes, flips, want = big
    got = staging.stage_crops(frame, [[0]], boxes, flips, 224, 128)
    assert got.shape == (10, 1, 3, 1, 128, 128) and torch.equal(got.cpu(), want)


def test_flip_is_the_mirrored_frame(golden):
    from coclr_amd import staging
    c = golden["A"]
    boxes = c["boxes"].tolist()[:5]
    flipped = staging.stage_crops(c["frames"], c["frame_index"], boxes, [1] * 5, 28, 16)
    mirrored = staging.stage_crops(c["frames"].flip(2).contiguous(), c["frame_index"], boxes, [0] * 5, 28, 16)
    plain = staging.stage_crops(c["frames"], c["frame_index"], boxes, [0] * 5, 28, 16)
    assert torch.equal(flipped, mirrored) and not torch.equal(flipped, plain)


def test_one_launch_equals_single_crop_launches(big):
    from coclr_amd import staging
    frame, boxes, flips, want = big
    dev = frame.cuda()
    single = torch.cat([staging.stage_crops(dev, [[0]], [b], [f], 224, 128) for b, f in zip(boxes, flips)])
    assert torch.equal(single.cpu(), want)
    # and with several slots per crop: clips of T = 2 over three frames of the fixture, odd output size
    frames = CH.golden()["A"]["frames"].cuda()
    idx = [[0, 1], [1, 2], [5, 0]]
    bx = staging.five_crop_boxes(52, 40, 28) * 2
    fl = [0] * 5 + [1] * 5
    together = staging.stage_crops(frames, idx, bx, fl, 28, 18)
    apart = torch.cat([staging.stage_crops(frames, idx, [b], [f], 28, 18) for b, f in zip(bx, fl)])
    assert torch.equal(together, apart)
    assert torch.equal(together.cpu(), CH.reference(frames, idx, [(x, y, f) for (x, y), f in zip(bx, fl)], 28, 28, 18))


def test_out_of_range_frame_index_raises_on_the_host(golden):
    from coclr_amd import staging
    c = golden["A"]
    out = torch.full((1, 1, 3, 4, 16, 16), 7.0, device="cuda")
    for bad in ([[0, 1, 2, 6]], [[0, -1, 2, 3]]):
        with pytest.raises(IndexError):
            staging.stage_crops(c["frames"], bad, [(0, 0)], [0], 28, 16, out=out)
    with pytest.raises(ValueError):
        staging.stage_crops(c["frames"], [[0, 1, 2, 3]], [(25, 0)], [0], 28, 16, out=out)       # 25 + 28 > 52
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                  # nothing was launched


def test_add_frames_equals_manual_staging_on_s3d():
    """add_frames against stage_crops + add() by hand through a real LinearClassifier at the smallest S3D input
    of tests/test_gpu_video_scores.py (3 x 8 x 64 x 64): the same crops in the same order fill the same batches,
    so the scores are bit-identical."""
    from coclr_amd import staging
    from coclr_amd.eval.video import VideoEvaluator
    from coclr_amd.model.classifier import LinearClassifier
    torch.manual_seed(0)
    model = LinearClassifier(num_class=51, network='s3d').cuda().eval()
    rng = np.random.RandomState(5)
    W, H, size, S, T = 100, 84, 72, 64, 8
    videos = [torch.from_numpy(rng.randint(0, 256, size=(F, H, W, 3)).astype(np.uint8)) for F in (5, 14, 9)]
    index = [staging.test_frame_index(v.shape[0], T) for v in videos]
    assert [i.shape[0] for i in index] == [1, 3, 1]
    labels = [3, 17, 40]
    ev = VideoEvaluator(model, batch_clips=8)
    for v, idx, l in zip(videos, index, labels):
        # two whole crops at a time: the chunking must not show in the result
        ev.add_frames(v, idx, label=l, crops="five", crop_size=size, out_size=S,
                      max_stage_bytes=2 * idx.shape[0] * 3 * T * S * S * 4)
    got = ev.finish()
    manual = VideoEvaluator(model, batch_clips=8)
    boxes = staging.five_crop_boxes(W, H, size)
    for v, idx, l in zip(videos, index, labels):
        staged = staging.stage_crops(v, idx, boxes, [0] * 5, size, S)
        vid = None
        for clips in staged:
            vid = manual.add(clips, label=l if vid is None else None, video=vid)
    want = manual.finish()
    torch.cuda.synchronize()
    assert ev.passes == manual.passes == -(-5 * 5 // 8)
    assert torch.equal(got.probs, want.probs) and torch.equal(got.features, want.features)
    assert torch.equal(got.labels, want.labels)
    assert torch.equal(got.top1, want.top1) and torch.equal(got.top5, want.top5)
    assert bool(torch.isfinite(got.probs).all()) and float(got.probs.sum(1).sub(1).abs().max()) < 1e-4
