"""The training-clip staging on one MI355X (csrc/staging.hip: coclr_augment_clips -- the jitter kernel with PIL's
GaussianBlur and the flip -- and coclr_resize_boxes_u8; coclr_amd/staging.py: stage_train_clips): against the
committed fixture of the reference's own training transform (tests/golden/train_transform.pt,
tools/make_train_transform_golden.py) and the numpy restatement of tests/train_harness.py (itself held against PIL
in tests/test_train_stage_cpu.py), with ZERO tolerance: every byte is integer arithmetic, every float an
individually rounded fp32 operation.  No test imports PIL."""
import math

import numpy as np
import pytest
import torch

import crops_harness as CH
import jitter_harness as JH
import train_harness as TH

pytestmark = pytest.mark.gpu

ROOT2 = float(np.float32(math.sqrt(2.0)))          # in PIL's floats the box radius reaches 1 here (1.4142: still 0)
BLUR_SIGMAS = (0.1, 0.5, 1.0, 1.4142, ROOT2, 2.0, 3.0, 9.0)


@pytest.fixture(scope="module")
def gold():
    return TH.golden()


@pytest.fixture(scope="module")
def plans(gold):
    return TH.fixture_plans(gold)


def _edges(H, W, seed):
    """A random frame with hard 0 / 255 edges and a single bright pixel in a dark patch."""
    f = TH.frames(1, H, W, seed)[0]
    f[::2, W // 3:W // 3 + 3] = 255
    f[1::2, W // 3:W // 3 + 3] = 0
    f[H // 2:, :max(W // 4, 1)] = 0
    f[min(H // 2 + 1, H - 1), 0] = (255, 200, 255)
    return f


@pytest.mark.parametrize("H,W", [(18, 22), (128, 128), (9, 1), (3, 3)])
def test_blur_alone(H, W):
    """18 x 22 takes the byte path of the vertical passes and the scalar stores (W % 4 != 0), 128 x 128 the dword
    path and 16-byte stores; 9 x 1 and 3 x 3 have lines shorter than r + 1 at sigma 3 and 9."""
    from coclr_amd import staging
    radii = [staging.blur_box_radius(s) for s in BLUR_SIGMAS]
    assert [int(r) for r in radii[:6]] == [0, 0, 0, 0, 1, 1] and int(radii[6]) >= 2 and int(radii[7]) >= 4
    frame = _edges(H, W, 4)
    frames = np.stack([frame] * len(radii))
    progs = [[(TH.BLUR, r)] for r in radii]
    got = staging.augment(torch.from_numpy(frames), progs, 1, 1).cpu()
    want = TH.reference(frames, progs, 1, 1)
    for n, r in enumerate(radii):
        assert torch.equal(got[n], want[n]), (n, r)
    plain = staging.color_jitter(torch.from_numpy(frames[:1]), [[]], 1, 1).cpu()
    assert torch.equal(staging.augment(torch.from_numpy(frames[:1]), [[(TH.BLUR, 0.0)]], 1, 1).cpu(), plain)
    if H * W > 9:
        assert not torch.equal(got[5], plain[0])


def test_largest_frame_blur_between_contrasts():
    """224 x 224 x 3 bytes is 147 KiB of the 160 KiB of LDS: the blur runs in place on the parked frame."""
    from coclr_amd import _lib, ops, staging
    frames = np.stack([_edges(224, 224, 8), TH.frames(1, 224, 224, 9)[0]])
    progs = [[(JH.CONTRAST, 1.3), (TH.BLUR, staging.blur_box_radius(1.7)), (JH.CONTRAST, 0.6)],
             [(JH.BRIGHTNESS, 1.1), (JH.CONTRAST, 0.5), (TH.BLUR, staging.blur_box_radius(0.8)), (TH.FLIP, 0),
              (JH.CONTRAST, 1.5), (TH.BLUR, staging.blur_box_radius(2.0))]]
    got = staging.augment(torch.from_numpy(frames), progs, 1, 1)
    assert torch.equal(got.cpu(), TH.reference(frames, progs, 1, 1))
    too_big = torch.zeros(1, 225, 224, 3, dtype=torch.uint8, device="cuda")
    out = torch.full((1, 3, 1, 225, 224), 7.0, device="cuda")
    with pytest.raises(ValueError):
        staging.augment(too_big, [[(TH.BLUR, 0.25)]], 1, 1, out=out)
    kinds, params = staging.augment_tables([[(TH.BLUR, 0.25)]])
    with pytest.raises(_lib.HipLibraryError):                                     # and by the entry point itself
        ops.augment_clips(too_big, kinds.cuda(), params.cuda(), 1, 1, CH.IMAGENET_MEAN, CH.IMAGENET_STD, out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                               # nothing was launched


@pytest.mark.parametrize("H,W", [(18, 22), (20, 24)])
def test_flip_at_each_position(H, W):
    from coclr_amd import staging
    base = [(JH.BRIGHTNESS, 1.2), (JH.CONTRAST, 0.7), (TH.BLUR, 1.375), (JH.HUE, 23), (JH.SATURATION, 1.3)]
    frame = _edges(H, W, 5)
    progs = [base] + [base[:i] + [(TH.FLIP, 0)] + base[i:] for i in range(len(base) + 1)]
    progs += [[(TH.FLIP, 0)] + base + [(TH.FLIP, 0)], [(TH.FLIP, 0)], []]
    frames = np.stack([frame] * len(progs))
    got = staging.augment(torch.from_numpy(frames), progs, 1, 1).cpu()
    assert torch.equal(got, TH.reference(frames, progs, 1, 1))
    for n in range(1, len(base) + 2):
        assert torch.equal(got[n], got[1]) and torch.equal(got[n], got[0].flip(-1)), n
    assert torch.equal(got[len(base) + 2], got[0])                                # two flips: none
    assert torch.equal(got[-2], got[-1].flip(-1)) and not torch.equal(got[1], got[0])


@pytest.mark.parametrize("group_size,T", [(1, 3), (3, 3), (6, 3)])
def test_group_sizes(group_size, T):
    from coclr_amd import staging
    frames = np.repeat(_edges(18, 22, 6)[None], 6, 0)                # the same frame six times: only the program differs
    progs = [[(1, 1.3), (2, 0.7), (TH.BLUR, 1.375), (4, 17)], [(TH.FLIP, 0), (2, 1.4), (5, 1), (TH.BLUR, 0.25)], [],
             [(TH.BLUR, 0.6), (TH.BLUR, 1.2)], [(TH.FLIP, 0)], [(3, 0.0), (TH.BLUR, 2.5), (TH.FLIP, 0)]][:6 // group_size]
    got = staging.augment(torch.from_numpy(frames), progs, group_size, T).cpu()
    assert got.shape == (6 // T, 3, T, 18, 22) and torch.equal(got, TH.reference(frames, progs, group_size, T))
    per = got.permute(0, 2, 1, 3, 4).reshape(6, 3, 18, 22)
    for a in range(6):
        for b in range(a):
            assert torch.equal(per[a], per[b]) == (a // group_size == b // group_size), (a, b)


def _launch_boxes(frames, boxes, T, S, pad=0):
    """One coclr_resize_boxes_u8 launch by hand: clip k reads frames [k*T, (k+1)*T).  `pad` more images of 0x5a
    behind the output.  Returns the whole buffer."""
    from coclr_amd import ops, staging
    dev = frames.device
    desc = torch.zeros(len(boxes), 10, dtype=torch.int32)
    bufs, fill = ([], []), [0, 0]
    for k, (x0, y0, w, h) in enumerate(boxes):
        desc[k, :6] = torch.tensor([k * T, T, x0, y0, w, h], dtype=torch.int32)
        for axis, n_in in ((0, w), (1, h)):
            lo, K = CH.kernel_layout(n_in, S)
            t = torch.cat([lo[None], K]).reshape(-1)
            desc[k, 6 + axis], desc[k, 8 + axis] = fill[axis], K.shape[0]
            bufs[axis].append(t)
            fill[axis] += t.numel()
    buf = torch.full((len(boxes) * T + pad, S, S, 3), 0x5a, dtype=torch.uint8, device=dev)
    ops.resize_boxes_u8(frames, desc.to(dev), desc, torch.cat(bufs[0]).to(dev), torch.cat(bufs[1]).to(dev), T, S,
                        buf[:len(boxes) * T])
    return buf


@pytest.mark.parametrize("H,W,S,boxes", [
    (40, 52, 16, [(0, 0, 52, 40), (9, 3, 35, 36), (3, 8, 16, 25), (36, 0, 16, 16), (0, 39, 52, 1), (51, 0, 1, 40)]),
    (240, 320, 128, [(0, 0, 320, 240), (17, 5, 128, 231), (100, 60, 201, 128), (192, 112, 128, 128), (3, 1, 97, 140),
                     (0, 0, 253, 189)])])
def test_resize_boxes(H, W, S, boxes):
    """Boxes of several sizes in one launch, the whole frame and boxes with w == S (and h == S) among them, up- and
    down-sampling: against the restatement per box and against one coclr_resize_crops_u8 launch per box."""
    from coclr_amd import ops, staging
    T = 2
    frames = torch.from_numpy(TH.frames(len(boxes) * T, H, W, 7)).cuda()
    buf = _launch_boxes(frames, boxes, T, S, pad=1)
    torch.cuda.synchronize()
    assert bool((buf[len(boxes) * T:] == 0x5a).all())                   # nothing written behind the last image
    got = buf[:len(boxes) * T].cpu()
    src = frames.cpu().numpy()
    for k, (x0, y0, w, h) in enumerate(boxes):
        want = CH.crop_resized_u8(src[k * T:(k + 1) * T], [(x0, y0, 0)], w, h, S)[0]
        assert torch.equal(got[k * T:(k + 1) * T], torch.from_numpy(want)), boxes[k]
        one = torch.empty(1, T, S, S, 3, dtype=torch.uint8, device="cuda")
        idx = torch.arange(k * T, (k + 1) * T, dtype=torch.int32, device="cuda").view(1, T)
        ops.resize_crops_u8(frames, idx, [(x0, y0, 0)], w, h, S, *staging._device_tables(w, h, S, frames.device), one)
        assert torch.equal(one[0].cpu(), got[k * T:(k + 1) * T]), boxes[k]
    # the launch alone writes every byte of its range
    again = _launch_boxes(frames, boxes, T, S)
    assert torch.equal(again.cpu(), got)


def test_fixture_bit_identical(gold, plans):
    from coclr_amd import staging
    S, T = gold["img_dim"], gold["seq_len"]
    for run, plan, _ in plans:
        got = staging.stage_train_clips(run["frames"], plan, S)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == (1, 2, 3, T, S, S)
        assert torch.equal(got[0].cpu(), TH.levels_expected(run["out"].numpy(), gold["levels"], T)), run["seed"]
        assert torch.equal(got, staging.stage_train_clips(run["frames"].cuda(), staging.pack_plan(plan, T)[None], S))


def test_batch_equals_single_samples(gold, plans):
    """B = 3 at the flagship's geometry in small: 2 x 4 frames of 60 x 80 to 32 x 32, plans drawn as a loader would."""
    import random
    from coclr_amd import staging
    tt = staging.TrainTransform(32, 4)
    rng, nrng = random.Random(3), np.random.RandomState(3)
    each = [tt.draw(80, 60, rng=rng, np_rng=nrng) for _ in range(3)]
    each[1]["programs"] = ([[(JH.GRAY, t % 3), (TH.BLUR, 1.375), (TH.FLIP, 0)] for t in range(4)], each[1]["programs"][1])
    frames = torch.from_numpy(TH.frames(3 * 8, 60, 80, 2)).view(3, 8, 60, 80, 3)
    batch = staging.stage_train_clips(frames, each, 32)
    assert batch.shape == (3, 2, 3, 4, 32, 32) and torch.equal(batch.cpu(), TH.chain_reference(frames.numpy(), each, 32))
    for b in range(3):
        assert torch.equal(staging.stage_train_clips(frames[b], each[b], 32)[0], batch[b]), b
    out = torch.empty_like(batch)
    packed = torch.stack([staging.pack_plan(p, 4) for p in each])
    assert staging.stage_train_clips(frames.cuda(), packed, 32, out=out) is out and torch.equal(out, batch)


def test_old_entry_points_unchanged(gold):
    """coclr_color_jitter_clips after the kernel became one of two instantiations: its own fixture, and the new
    entry point gives the same on the old kinds."""
    from coclr_amd import staging
    jg = JH.golden()
    picked = [c for c in JH.fixture_cases(jg) if c[0][0] == "A"]
    assert len(picked) == 4
    for name, frames, progs, gs, want, _ in picked:
        got = staging.color_jitter(torch.from_numpy(frames), progs, gs, 3)
        assert torch.equal(got.cpu(), JH.levels_expected(want, jg["levels"], 3)), name
        assert torch.equal(staging.augment(torch.from_numpy(frames), progs, gs, 3), got), name
    with pytest.raises(ValueError):
        staging.color_jitter(torch.from_numpy(picked[0][1]), [[(TH.BLUR, 0.25)]], 6, 3)
