"""The colour-jitter kernel (csrc/staging.hip: coclr_color_jitter_clips) and the uint8 resize next to it
(coclr_resize_crops_u8) on one MI355X: against the committed fixture of the reference's own ColorJitter / RandomGray
classes (tests/golden/color_jitter.pt, tools/make_color_jitter_golden.py) and the numpy restatement of
tests/jitter_harness.py (itself held against PIL over every input in tests/test_jitter_cpu.py), with ZERO
tolerance: PIL's arithmetic is integers plus a fixed sequence of individually rounded fp32 / double operations,
so every bit is determined.  No test imports PIL."""
import random

import numpy as np
import pytest
import torch

import crops_harness as CH
import jitter_harness as JH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return JH.golden()


@pytest.fixture(scope="module")
def cases(gold):
    return JH.fixture_cases(gold)


def _frames(n, H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n, H, W, 3)).astype(np.uint8)


@pytest.mark.parametrize("letter", ["A", "B", "C", "D", "E"])
def test_fixture_cases_bit_identical(gold, cases, letter):
    from coclr_amd import staging
    picked = [c for c in cases if c[0][0] == letter]
    assert picked
    for name, frames, progs, gs, want, _ in picked:
        T = 3 if letter != "E" else 2
        got = staging.color_jitter(torch.from_numpy(frames), progs, gs, T)
        assert got.is_cuda and got.dtype == torch.float32
        assert torch.equal(got.cpu(), JH.levels_expected(want, gold["levels"], T)), name
        assert torch.equal(got, staging.color_jitter(torch.from_numpy(frames).cuda(), progs, gs, T)), name


@pytest.fixture(scope="module")
def big():
    from coclr_amd import staging
    frame = torch.from_numpy(_frames(1, 256, 340, 3))
    boxes = staging.five_crop_boxes(340, 256, 224) * 2
    return frame.cuda(), boxes, [0] * 5 + [1] * 5


def test_no_jitter_equals_plain_staging(big):
    from coclr_amd import staging
    none = staging.ColorJitter(0.2, 0.2, 0.2, 0.1, p=0).draw(random.Random(1), 1)
    assert none == [[]]
    c = CH.golden()["A"]
    boxes, flips = c["boxes"].tolist(), c["flips"].tolist()
    plain = staging.stage_crops(c["frames"], c["frame_index"], boxes, flips, c["crop"], c["S"])
    for progs in ([[]] * 10, none * 10, [[(0, 0.0)] * 8] * 10):
        assert torch.equal(staging.stage_crops(c["frames"], c["frame_index"], boxes, flips, c["crop"], c["S"],
                                               jitter=progs), plain)
    frame, boxes, flips = big
    plain = staging.stage_crops(frame, [[0]], boxes, flips, 224, 128)
    assert torch.equal(staging.stage_crops(frame, [[0]], boxes, flips, 224, 128, jitter=none * 10), plain)


@pytest.mark.parametrize("H,W", [(18, 22), (128, 128)])
def test_each_op_alone(H, W):
    """Odd sizes take the scalar store path (W % 4 != 0), 128 x 128 the 16-byte one.  The contrast frames put the
    mean of L exactly on k + 0.5 (rounds up to k + 1) and one pixel's worth below it (rounds down to k)."""
    from coclr_amd import staging
    rnd = _frames(1, H, W, 4)[0]
    rnd[::2, 3:9] = 255
    rnd[1::2, 3:9] = 0
    todo = [(rnd, [(JH.BRIGHTNESS, a)]) for a in (0.0, 1.0, 1.4)] + \
           [(rnd, [(JH.SATURATION, a)]) for a in (0.0, 2.0)] + \
           [(rnd, [(JH.CONTRAST, a)]) for a in (0.6, 1.4)] + \
           [(JH.half_mean_frame(H, W, k, nudge)[0], [(JH.CONTRAST, a)])
            for k in (100, 37) for nudge in (False, True) for a in (0.6, 1.4)] + \
           [(rnd, [(JH.GRAY, ch)]) for ch in (0, 1, 2)] + [(rnd, [(JH.HUE, s)]) for s in (0, 17, 244)]
    assert JH.contrast_mean(JH.half_mean_frame(H, W, 100, False)[0]) == 101
    assert JH.contrast_mean(JH.half_mean_frame(H, W, 100, True)[0]) == 100
    frames = np.stack([f for f, _ in todo])
    progs = [p for _, p in todo]
    got = staging.color_jitter(torch.from_numpy(frames), progs, 1, 1).cpu()
    want = JH.reference(frames, progs, 1, 1)
    for n, (_, p) in enumerate(todo):
        assert torch.equal(got[n], want[n]), (n, p)
    assert torch.equal(got[1], JH.reference(frames[1:2], [[]], 1, 1)[0])          # brightness 1 is the identity
    # the half rounds up, the nudge down: at 1.4 a pixel of value 100 goes to 99 under mean 101 and stays under mean 100
    assert float(got[8][0, 0, 0, 0]) < float(got[10][0, 0, 0, 0])


@pytest.mark.parametrize("lo", [0, 64, 128, 192])
@pytest.mark.parametrize("what", ["hue", "saturation"])
def test_rgb_cube(gold, what, lo):
    """Every RGB value: 64 red values x 256 x 256 as 256 frames of 128 x 128 per slab -- the smallest input that
    reaches every division and rounding case of the HSV round trip (the cases are scattered: no subsample does)."""
    from coclr_amd import staging
    r = np.arange(256, dtype=np.uint8)
    cube = np.ascontiguousarray(np.stack(np.meshgrid(r[lo:lo + 64], r, r, indexing="ij"), -1).reshape(256, 128, 128, 3))
    dev = torch.from_numpy(cube).cuda()
    levels = gold["levels"].cuda()
    for prog in ([(JH.HUE, 17)], [(JH.HUE, 244)]) if what == "hue" else ([(JH.SATURATION, 0.63)], [(JH.SATURATION, 1.37)]):
        got = staging.color_jitter(dev, [prog], 256, 1)                           # (256, 3, 1, 128, 128)
        want_u8 = torch.from_numpy(JH.jitter_u8(cube, [prog], 256)).cuda().long()
        want = torch.stack([levels[c][want_u8[..., c]] for c in range(3)], 1).unsqueeze(2)      # the fixture's byte table
        assert torch.equal(got, want), prog


def test_all_orders_of_the_four_ops():
    from coclr_amd import staging
    frames, progs = JH.order_case()
    got = staging.color_jitter(torch.from_numpy(frames), progs, 1, 1).cpu()
    want = JH.reference(frames, progs, 1, 1)
    for g in range(24):
        assert torch.equal(got[g], want[g]), progs[g]
    assert len({got[g].numpy().tobytes() for g in range(24)}) >= 20


@pytest.mark.parametrize("group_size,T", [(1, 1), (1, 3), (3, 3), (3, 2), (6, 2), (6, 6)])
def test_group_sizes(group_size, T):
    from coclr_amd import staging
    frames = np.repeat(_frames(1, 18, 22, 6), 6, 0)                  # the same frame six times: only the program differs
    progs = [[(1, 1.3), (2, 0.7), (3, 1.37), (4, 17)], [(4, 244), (2, 1.4), (5, 1), (1, 0.5)], [], [(2, 0.6), (2, 1.2)],
             [(5, 2)], [(3, 0.0)]][:6 // group_size]
    got = staging.color_jitter(torch.from_numpy(frames), progs, group_size, T).cpu()
    assert got.shape == (6 // T, 3, T, 18, 22) and torch.equal(got, JH.reference(frames, progs, group_size, T))
    per = got.permute(0, 2, 1, 3, 4).reshape(6, 3, 18, 22)
    for a in range(6):
        for b in range(a):
            assert torch.equal(per[a], per[b]) == (a // group_size == b // group_size), (a, b)
    # more programs than groups are allowed; fewer are refused
    more = staging.color_jitter(torch.from_numpy(frames), progs + [[(1, 0.1)]], group_size, T).cpu()
    assert torch.equal(more, got)


def test_largest_frame_and_refusal():
    """224 x 224 x 3 bytes is 147 KiB of the 160 KiB of LDS; the contrast ops sit in the middle of the program."""
    from coclr_amd import _lib, ops, staging
    frames = _frames(2, 224, 224, 8)
    progs = [[(1, 1.2), (2, 1.3), (4, 100)], [(3, 0.3), (2, 0.5), (2, 1.5), (1, 0.9)]]
    got = staging.color_jitter(torch.from_numpy(frames), progs, 1, 1)
    assert torch.equal(got.cpu(), JH.reference(frames, progs, 1, 1))
    too_big = torch.zeros(1, 225, 224, 3, dtype=torch.uint8, device="cuda")
    out = torch.full((1, 3, 1, 225, 224), 7.0, device="cuda")
    with pytest.raises(ValueError):
        staging.color_jitter(too_big, [[(2, 1.3)]], 1, 1, out=out)
    kinds, params = staging.program_tables([[(2, 1.3)]])
    with pytest.raises(_lib.HipLibraryError):                                     # and by the entry point itself
        ops.color_jitter_clips(too_big, kinds.cuda(), params.cuda(), 1, 1, CH.IMAGENET_MEAN, CH.IMAGENET_STD, out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                               # nothing was launched


def test_stage_crops_with_jitter(gold, cases, big):
    from coclr_amd import ops, staging
    # fixture D: the reference's own chain flip -> FiveCrop(28) -> Scale(16) -> ColorJitter on two crops
    sc = CH.golden()["A"]
    runs = gold["D"]
    d = [c for c in cases if c[0][0] == "D"]
    boxes = [staging.five_crop_boxes(52, 40, 28, (r["where"],))[0] for r in runs]
    flips = [r["flip"] for r in runs]
    idx = [[0, 1, 2], [3, 4, 5]]
    got = staging.stage_crops(sc["frames"], idx, boxes, flips, 28, 16, jitter=[c[2][0] for c in d])
    want = torch.stack([JH.levels_expected(c[4], gold["levels"], 3) for c in d])
    assert got.shape == (2, 2, 3, 3, 16, 16) and torch.equal(got.cpu(), want)
    # by hand: resize_crops_u8, then color_jitter
    frame, boxes, flips = big
    progs = [staging.ColorJitter(0.2, 0.2, 0.2, 0.1).draw(r, 1)[0] for r in [random.Random(9)] for _ in range(10)]
    together = staging.stage_crops(frame, [[0]], boxes, flips, 224, 128, jitter=progs)
    crops = staging.check_crops(boxes, flips, 224, 224, 340, 256)
    u8 = torch.empty(10, 1, 128, 128, 3, dtype=torch.uint8, device="cuda")
    ops.resize_crops_u8(frame, torch.zeros(1, 1, dtype=torch.int32, device="cuda"), crops, 224, 224, 128,
                        *staging._device_tables(224, 224, 128, frame.device), u8)
    want_u8 = np.stack(CH.crop_resized_u8(frame.cpu().numpy(), crops, 224, 224, 128))
    assert torch.equal(u8.cpu(), torch.from_numpy(want_u8))
    by_hand = staging.color_jitter(u8.view(10, 128, 128, 3), progs, 1, 1)
    assert torch.equal(together.view(10, 3, 1, 128, 128), by_hand)
    assert not torch.equal(together, staging.stage_crops(frame, [[0]], boxes, flips, 224, 128))
    # one launch over ten crops equals ten single-crop launches
    apart = torch.cat([staging.stage_crops(frame, [[0]], [b], [f], 224, 128, jitter=[p])
                       for b, f, p in zip(boxes, flips, progs)])
    assert torch.equal(together, apart)


def test_add_frames_with_jitter_on_s3d():
    """add_frames(jitter=J, rng=Random(5)) against drawing the same programs and staging by hand, through a real
    LinearClassifier at the smallest S3D input (3 x 8 x 64 x 64, as tests/test_gpu_stage_crops.py)."""
    from coclr_amd import staging
    from coclr_amd.eval.video import VideoEvaluator
    from coclr_amd.model.classifier import LinearClassifier
    torch.manual_seed(0)
    model = LinearClassifier(num_class=51, network='s3d').cuda().eval()
    rng = np.random.RandomState(5)
    W, H, size, S, T = 100, 84, 72, 64, 8
    videos = [torch.from_numpy(rng.randint(0, 256, size=(F, H, W, 3)).astype(np.uint8)) for F in (5, 14)]
    index = [staging.test_frame_index(v.shape[0], T) for v in videos]
    labels = [3, 17]
    J = staging.ColorJitter(0.2, 0.2, 0.2, 0.1, p=0.7)
    ev = VideoEvaluator(model, batch_clips=8)
    r = random.Random(5)
    for v, idx, l in zip(videos, index, labels):
        ev.add_frames(v, idx, label=l, crops="five", crop_size=size, out_size=S, jitter=J, rng=r,
                      max_stage_bytes=2 * idx.shape[0] * 3 * T * S * S * 4)
    got = ev.finish()
    manual = VideoEvaluator(model, batch_clips=8)
    boxes = staging.five_crop_boxes(W, H, size)
    r2 = random.Random(5)
    for v, idx, l in zip(videos, index, labels):
        progs = [J.draw(r2, 1)[0] for _ in boxes]
        staged = staging.stage_crops(v, idx, boxes, [0] * 5, size, S, jitter=progs)
        vid = None
        for clips in staged:
            vid = manual.add(clips, label=l if vid is None else None, video=vid)
    want = manual.finish()
    plain = VideoEvaluator(model, batch_clips=8)
    for v, idx, l in zip(videos, index, labels):
        plain.add_frames(v, idx, label=l, crops="five", crop_size=size, out_size=S)
    base = plain.finish()
    torch.cuda.synchronize()
    assert r.random() == r2.random()
    assert torch.equal(got.probs, want.probs) and torch.equal(got.features, want.features)
    assert torch.equal(got.labels, want.labels)
    # (the freshly initialised head scores every class alike to the last bit: the jitter shows in the features)
    assert not (torch.equal(got.features, base.features) and torch.equal(got.probs, base.probs))
    assert bool(torch.isfinite(got.probs).all()) and float(got.probs.sum(1).sub(1).abs().max()) < 1e-4
