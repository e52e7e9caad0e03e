"""The classifier-clip staging on one MI355X (csrc/staging.hip: coclr_resize2_boxes -- RandomSizedCrop(consistent=True)
with its fallback and Scale(img_dim) in one launch; coclr_amd/staging.py: stage_classifier_clips): against the committed
fixture of the reference's own classifier transform (tests/golden/cls_transform.pt,
tools/make_cls_transform_golden.py), the numpy restatement of tests/cls_harness.py (itself held against PIL in
tests/test_cls_stage_cpu.py) and the entry points the project had before, with ZERO tolerance: every byte is integer
arithmetic, every float an individually rounded fp32 operation.  No test imports PIL; every refusal is stopped on the
host."""
import random

import numpy as np
import pytest
import torch

import cls_harness as CL
import crops_harness as CH
import jitter_harness as JH

pytestmark = pytest.mark.gpu

WHOLE = ((24, 24), (0, 0))


@pytest.fixture(scope="module")
def gold():
    return CL.golden()


@pytest.fixture(scope="module")
def plans(gold):
    return CL.fixture_plans(gold)


def _launch(frames, clips, T, size, S, form, pad=1, fill=0x5a):
    """One coclr_resize2_boxes launch by hand: clip k reads frames [first, first + T).  `pad` more clips of `fill`
    (bytes) / 7.0 (fp32) behind the output.  Returns the whole buffer."""
    from coclr_amd import ops
    dev = frames.device
    desc, xtab, ytab, tab2 = CL.descriptors(clips, T, size, S)
    n = len(clips)
    if form == "u8":
        buf = torch.full(((n + pad) * T, S, S, 3), fill, dtype=torch.uint8, device=dev)
        ops.resize2_boxes(frames, desc.to(dev), desc, xtab.to(dev), ytab.to(dev), tab2.to(dev), T, size, S, buf[:n * T])
    else:
        buf = torch.full((n + pad, 3, T, S, S), 7.0, dtype=torch.float32, device=dev)
        ops.resize2_boxes(frames, desc.to(dev), desc, xtab.to(dev), ytab.to(dev), tab2.to(dev), T, size, S, buf[:n],
                          CH.IMAGENET_MEAN, CH.IMAGENET_STD)
    return buf


def _check_launch(H, W, size, S, T, geo):
    """`geo`: [(region, resample, window)], clip k on its own T frames, all in one launch: the byte form and the fp32
    form against the restatement, nothing written behind the output, every byte of the range written."""
    n = len(geo)
    src = CL.frames(n * T, H, W, 7)
    frames = torch.from_numpy(src).cuda()
    clips = [(k * T, region, resample, window) for k, (region, resample, window) in enumerate(geo)]
    want = [CL.resized_u8(src[k * T:(k + 1) * T], region, resample, window, size, S)
            for k, (region, resample, window) in enumerate(geo)]
    buf = _launch(frames, clips, T, size, S, "u8")
    torch.cuda.synchronize()
    assert bool((buf[n * T:] == 0x5a).all())                          # nothing written behind the last image
    got = buf[:n * T].cpu()
    for k in range(n):
        assert torch.equal(got[k * T:(k + 1) * T], torch.from_numpy(want[k])), geo[k]
    again = _launch(frames, clips, T, size, S, "u8", pad=0, fill=0xa5)      # the launch alone writes every byte
    assert torch.equal(again.cpu(), got)
    f32 = _launch(frames, clips, T, size, S, "f32")
    torch.cuda.synchronize()
    assert bool((f32[n:] == 7.0).all())
    for k in range(n):
        assert torch.equal(f32[k].cpu(), JH.to_clips(want[k], T)[0]), geo[k]
    return frames, got


def test_fixture_bit_identical(gold, plans):
    from coclr_amd import staging
    size, T = gold["size"], gold["seq_len"]
    for run, plan, _ in plans:
        S = run["img_dim"]
        want = JH.levels_expected(run["out"].numpy(), gold["levels"], T)
        got = staging.stage_classifier_clips(run["frames"], plan, S, size=size)                  # host frames
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == (1, 3, T, S, S)
        assert torch.equal(got.cpu(), want), (run["seed"], run["set"])
        packed = staging.pack_cls_plan(plan)[None]
        assert torch.equal(staging.stage_classifier_clips(run["frames"].cuda(), packed, S, size=size), got)


def test_kernel_small_geometry():
    """40 x 52 frames, size 24, S 16: the whole frame, w == size, h == size, a box one pixel wide, one a pixel high, and
    a fallback window in the middle of a 288-wide resample, in ONE launch."""
    geo = [((0, 0, 52, 40),) + WHOLE, ((3, 8, 24, 25),) + WHOLE, ((5, 2, 30, 24),) + WHOLE, ((51, 0, 1, 40),) + WHOLE,
           ((0, 39, 52, 1),) + WHOLE, ((0, 0, 52, 40), (288, 24), (132, 0))]
    _check_launch(40, 52, 24, 16, 2, geo)


@pytest.mark.parametrize("S", [128, 224, 18])
def test_kernel_full_geometry(S):
    """240 x 320 frames to 224 and on to S: the real LDS footprint at 128; the identity second stage at 224; at 18
    (S % 4 != 0) the scalar stores and a band of one output row over the 64 KiB that need the opt-in."""
    from coclr_amd import staging
    assert staging.fallback_geometry(320, 240, 224) == ((298, 224), (37, 0))
    full = ((224, 224), (0, 0))
    geo = [((0, 0, 320, 240),) + full, ((17, 5, 128, 231),) + full, ((100, 60, 201, 128),) + full,
           ((0, 0, 320, 240), (298, 224), (37, 0))]
    _check_launch(240, 320, 224, S, 2, geo)


@pytest.mark.parametrize("H,W,size,S,boxes", [
    (40, 52, 24, 16, [(0, 0, 52, 40), (9, 3, 35, 36), (3, 8, 24, 25), (36, 0, 16, 16)]),
    (240, 320, 224, 128, [(0, 0, 320, 240), (17, 5, 128, 231), (100, 60, 201, 128)])])
def test_fused_equals_the_chained_entry_points(H, W, size, S, boxes, monkeypatch):
    """Box-form plans: the fused bytes equal coclr_resize_boxes_u8 box -> size followed by coclr_resize_boxes_u8
    whole -> S, and COCLR_CLS_FUSED=0 and 1 give equal tensors."""
    from coclr_amd import ops, staging
    T = 2
    full = ((size, size), (0, 0))
    src = CL.frames(len(boxes) * T, H, W, 9)
    frames = torch.from_numpy(src).cuda()
    fused = _launch(frames, [(k * T, b) + full for k, b in enumerate(boxes)], T, size, S, "u8", pad=0)

    def chained(frames, boxes, n_out):
        desc = torch.zeros(len(boxes), 10, dtype=torch.int32)
        bufs, fill = ([], []), [0, 0]
        for k, (x0, y0, w, h) in enumerate(boxes):
            desc[k, :6] = torch.tensor([k * T, T, x0, y0, w, h], dtype=torch.int32)
            for axis, n_in in ((0, w), (1, h)):
                lo, K = CH.kernel_layout(n_in, n_out)
                desc[k, 6 + axis], desc[k, 8 + axis] = fill[axis], K.shape[0]
                bufs[axis].append(torch.cat([lo[None], K]).reshape(-1))
                fill[axis] += bufs[axis][-1].numel()
        out = torch.empty(len(boxes) * T, n_out, n_out, 3, dtype=torch.uint8, device="cuda")
        ops.resize_boxes_u8(frames, desc.cuda(), desc, torch.cat(bufs[0]).cuda(), torch.cat(bufs[1]).cuda(), T, n_out, out)
        return out
    mid = chained(frames, boxes, size)
    assert torch.equal(chained(mid, [(0, 0, size, size)] * len(boxes), S), fused)
    # the switch, through the public function: a training batch (programs, a flip) and a validation batch
    each = [{"form": "box", "region": b, "resample": full[0], "window": full[1],
             "program": [(1, 1.2), (2, 0.7), (4, 23), (3, 1.3)] if k % 2 else []} for k, b in enumerate(boxes)]
    fr = frames.view(len(boxes), T, H, W, 3)
    for plans_, flip in ((each, True), ([dict(p, program=[]) for p in each], False)):
        monkeypatch.setenv("COCLR_CLS_FUSED", "1")
        one = staging.stage_classifier_clips(fr, plans_, S, flip=flip, size=size)
        monkeypatch.setenv("COCLR_CLS_FUSED", "0")
        two = staging.stage_classifier_clips(fr, plans_, S, flip=flip, size=size)
        assert torch.equal(one, two)
    with pytest.raises(ValueError):                                   # with 0 the fallback form cannot be expressed
        (ow, oh), win = staging.fallback_geometry(W, H, size)
        staging.stage_classifier_clips(fr[:1], [{"form": "fallback", "region": (0, 0, W, H), "resample": (ow, oh),
                                                 "window": win, "program": []}], S, size=size)


def test_batch_equals_single_samples(monkeypatch):
    """B = 3, T = 4, 60 x 80 -> 48 -> 32, plans drawn as a loader would, one of them the fallback, with the batch flip."""
    from coclr_amd import staging
    monkeypatch.delenv("COCLR_CLS_FUSED", raising=False)
    ct = staging.ClassifierTransform(32, 4, size=48)
    rng = random.Random(3)
    each = [ct.draw(80, 60, rng=rng) for _ in range(3)]
    each[1]["program"] = [(1, 1.2), (2, 0.7), (4, 23), (3, 1.3)]
    (ow, oh), win = staging.fallback_geometry(80, 60, 48)
    assert ((ow, oh), win) == ((64, 48), (8, 0))
    each[2] = {"form": "fallback", "region": (0, 0, 80, 60), "resample": (ow, oh), "window": win, "program": each[2]["program"]}
    frames = torch.from_numpy(CL.frames(3 * 4, 60, 80, 2)).view(3, 4, 60, 80, 3)
    batch = staging.stage_classifier_clips(frames, each, 32, flip=True, size=48)
    assert batch.shape == (3, 3, 4, 32, 32)
    assert torch.equal(batch.cpu(), CL.chain_reference(frames.numpy(), each, 48, 32, flip=True))
    for b in range(3):
        assert torch.equal(staging.stage_classifier_clips(frames[b], each[b], 32, flip=True, size=48)[0], batch[b]), b
    plain = staging.stage_classifier_clips(frames, each, 32, size=48)
    assert torch.equal(batch, plain.flip(-1)) and not torch.equal(batch, plain)
    out = torch.empty_like(batch)
    packed = torch.stack([staging.pack_cls_plan(p) for p in each])
    assert staging.stage_classifier_clips(frames.cuda(), packed, 32, flip=True, size=48, out=out) is out
    assert torch.equal(out, batch)
    # validation (one launch, fp32 from the resize kernel) equals training with empty programs and a flip undone
    val = [dict(p, program=[]) for p in each]
    direct = staging.stage_classifier_clips(frames, val, 32, size=48)
    assert staging.classifier_tables(val, 3, 4, 80, 60, 32, size=48)[6] is True
    assert torch.equal(direct, staging.stage_classifier_clips(frames, val, 32, flip=True, size=48).flip(-1))
    assert torch.equal(direct.cpu(), CL.chain_reference(frames.numpy(), val, 48, 32))


def test_size_limit_refused_before_any_launch():
    from coclr_amd import _lib, ops, staging
    frames = torch.zeros(2, 240, 320, 3, dtype=torch.uint8, device="cuda")
    out = torch.full((1, 3, 2, 16, 16), 7.0, device="cuda")
    plan = {"form": "box", "region": (0, 0, 320, 240), "resample": (225, 225), "window": (0, 0), "program": []}
    with pytest.raises(ValueError):
        staging.stage_classifier_clips(frames, plan, 16, size=225, out=out)
    with pytest.raises(ValueError):
        staging.ClassifierTransform(16, 2, size=225)
    desc, xtab, ytab, tab2 = CL.descriptors([(0, (0, 0, 320, 240), (225, 225), (0, 0))], 2, 225, 16)
    with pytest.raises(_lib.HipLibraryError):                                     # and by the entry point itself
        ops.resize2_boxes(frames, desc.cuda(), desc, xtab.cuda(), ytab.cuda(), tab2.cuda(), 2, 225, 16, out,
                          CH.IMAGENET_MEAN, CH.IMAGENET_STD)
    big = torch.full((1, 3, 2, 225, 225), 7.0, device="cuda")
    d2, x2, y2, t2 = CL.descriptors([(0, (0, 0, 320, 240), (225, 225), (0, 0))], 2, 225, 225)
    with pytest.raises(_lib.HipLibraryError):
        ops.resize2_boxes(frames, d2.cuda(), d2, x2.cuda(), y2.cuda(), t2.cuda(), 2, 225, 225, big,
                          CH.IMAGENET_MEAN, CH.IMAGENET_STD)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((big == 7.0).all())                  # nothing was launched
