"""Batches whose videos differ in frame size on one MI355X (csrc/jpeg.hip: coclr_jpeg_decode_ragged; csrc/staging.hip:
coclr_resize_boxes_ragged_u8, coclr_resize2_boxes_ragged; coclr_amd/jpeg.py: cat_ragged, decode_ragged;
coclr_amd/staging.py: RaggedFrames, stage_train_clips_ragged, stage_classifier_clips_ragged): one mixed batch per call
against PIL's own bytes (tests/golden/jpeg_frames.pt), the reference's own transforms (tests/golden/cls_transform.pt,
train_transform.pt), the numpy restatements of tests/train_harness.py and tests/cls_harness.py, and the one-size entry
points on each sample alone, with ZERO tolerance: every comparison is torch.equal.  No test imports PIL, and no
damaged stream is sent to the GPU (those belong to the host programs: tests/test_ragged_cpu.py)."""
import os
import random

import numpy as np
import pytest
import torch

import _jpeg_cases as J
import cls_harness as CL
import jitter_harness as JH
import ragged_harness as RH
import train_harness as TH

pytestmark = pytest.mark.gpu

FILL = 0x5a


@pytest.fixture(scope="module")
def whole():
    """All 54 cases of the fixture as one ragged pack, in fixture order."""
    from coclr_amd import jpeg
    cases = J.cases()
    packs = [jpeg.pack([J.raw(c)]) for c in cases]
    return cases, packs, jpeg.cat_ragged(packs)


def _check_frames(frames, cases):
    assert len(frames) == len(cases)
    for i, c in enumerate(cases):
        assert frames.height[i] == c["height"] and frames.width[i] == c["width"]
        assert torch.equal(frames.frame(i).cpu(), c["rgb"]), c["name"]


def _decode_into_filled(data, meta, tail=64):
    """One coclr_jpeg_decode_ragged call by hand into an output filled with 0x5a, `tail` more bytes behind it."""
    from coclr_amd import jpeg, ops, staging
    geo = jpeg.check_meta_ragged(data, meta)
    offset, total, stages, blocks = jpeg.ragged_plan(geo, 256 << 20)
    (_, _, geom, prefix), = stages
    host = meta[:, 8:].contiguous()
    pixels = torch.full((((total + 15) & ~15) + tail,), FILL, dtype=torch.uint8, device="cuda")
    coefs = torch.empty(blocks * 64, dtype=torch.int16, device="cuda")
    planes = torch.empty(blocks * 64, dtype=torch.uint8, device="cuda")
    status = torch.empty(meta.shape[0], dtype=torch.int32, device="cuda")
    ops.jpeg_decode_ragged(data.cuda(), host.cuda(), host, geom.cuda(), geom, prefix.cuda(), prefix, coefs, planes,
                           pixels, status, chunk_bytes=jpeg.split_policy())
    assert not bool(status.any())
    return staging.RaggedFrames(pixels, offset, geo[:, 0], geo[:, 1])


def _untouched(frames):
    """The bytes of `pixels` that belong to no frame."""
    keep = torch.ones(frames.pixels.numel(), dtype=torch.bool)
    for o, H, W in zip(frames.offset.tolist(), frames.height.tolist(), frames.width.tolist()):
        keep[o:o + 3 * H * W] = False
    return frames.pixels.cpu()[keep]


def test_whole_fixture_in_one_call(whole):
    from coclr_amd import jpeg, ops
    cases, packs, (data, meta) = whole
    assert len(cases) == 54
    geo = jpeg.check_meta_ragged(data, meta)
    assert len({tuple(g) for g in geo.tolist()}) == 21                  # every size, gray and YCbCr, three samplings
    assert {int(m[0, 10]) > 0 for _, m in packs} == {True, False}        # restart intervals and none
    # the longest restart-less scan takes several windows of 1024 chunks at 8 bytes while its neighbours take one
    scans = {c["name"]: int(m[0, 9]) for c, (_, m) in zip(cases, packs) if int(m[0, 11]) == 1}
    name = max(scans, key=scans.get)
    assert name == "56x40_444_q100_noise" and -(-scans[name] // 8) > 1024
    assert sum(-(-n // 8) <= 1024 for n in scans.values()) == len(scans) - 1
    # workgroups of the inverse DCT and the colour stage straddle frame boundaries
    _, _, stages, blocks = jpeg.ragged_plan(geo, 256 << 20)
    assert len(stages) == 1 and blocks % 256 != 0 and int(stages[0][3][1, -1]) % 256 != 0
    got = []
    for chunk_bytes in (0, 8, 64):
        frames, status = jpeg.decode_ragged(data, meta, return_status=True, chunk_bytes=chunk_bytes)
        assert not bool(status.any()) and status.shape == (54,) and jpeg.decode_ragged.last_status is status
        _check_frames(frames, cases)
        got.append(frames)
    for other in got[1:]:
        assert torch.equal(other.offset, got[0].offset)
        for i in range(54):
            assert torch.equal(other.frame(i), got[0].frame(i))
    assert ops.JR_FIELDS == 8


@pytest.mark.parametrize("order", ["largest", "smallest", "single"])
def test_order_and_count(whole, order):
    from coclr_amd import jpeg
    cases, packs, _ = whole
    size = lambda i: cases[i]["height"] * cases[i]["width"]               # noqa: E731
    if order == "single":
        idx = [cases.index(J.case("45x37_422_q100_noise"))]
    else:
        idx = sorted(range(len(cases)), key=size, reverse=order == "largest")
    data, meta = jpeg.cat_ragged([packs[i] for i in idx])
    frames = jpeg.decode_ragged(data, meta)
    _check_frames(frames, [cases[i] for i in idx])
    assert not bool(jpeg.decode_ragged.last_status.any())
    filled = _decode_into_filled(data, meta)
    _check_frames(filled, [cases[i] for i in idx])
    rest = _untouched(filled)
    assert rest.numel() >= 64 and bool((rest == FILL).all())             # padding between frames and behind the last


def test_stage_budget(whole):
    from coclr_amd import jpeg, ops
    cases, _, (data, meta) = whole
    small = sum(ops.jpeg_workspace(16, 16, 3, 1, 1))                      # 12 blocks of 192 bytes
    geo = jpeg.check_meta_ragged(data, meta)
    assert len(jpeg.ragged_plan(geo, 3 * small)[2]) > 20 and len(jpeg.ragged_plan(geo, 1)[2]) == 54
    for budget in (3 * small, 1):
        _check_frames(jpeg.decode_ragged(data, meta, max_stage_bytes=budget), cases)
        assert not bool(jpeg.decode_ragged.last_status.any())


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("img_dim", [16, 24])
def test_classifier_batch(img_dim, fused, monkeypatch):
    from coclr_amd import staging
    gold = CL.golden()
    size, T = gold["size"], gold["seq_len"]
    batch = RH.cls_batches()[img_dim]
    if fused == "0":
        # the chained form takes box plans only, and every box plan of the fixture is on a 40 x 52 frame: two seeded
        # samples of other sizes join them, held against the restatement
        batch = [(run, plan) for run, plan in batch if plan["form"] == "box"]
        for seed, (H, W), region in ((21, (8, 96), (40, 1, 56, 7)), (22, (57, 41), (20, 30, 21, 27))):
            fr = torch.from_numpy(CL.frames(T, H, W, seed))
            plan = {"form": "box", "region": region, "resample": (size, size), "window": (0, 0),
                    "program": [(1, 1.2), (3, 0.8)] if seed == 21 else []}
            want = CL.chain_u8(fr.numpy(), plan, size, img_dim)
            batch.insert(1, ({"frames": fr, "out": torch.from_numpy(want), "seed": seed, "set": "seeded"}, plan))
    assert {tuple(run["frames"].shape[1:3]) for run, _ in batch} >= {(40, 52), (8, 96)}
    monkeypatch.setenv("COCLR_CLS_FUSED", fused)
    frames = staging.ragged_from_frames([run["frames"] for run, _ in batch])
    plans = [plan for _, plan in batch]
    out = staging.stage_classifier_clips_ragged(frames, plans, img_dim, size=size)
    assert out.is_cuda and out.shape == (len(batch), 3, T, img_dim, img_dim)
    for b, (run, plan) in enumerate(batch):
        want = JH.levels_expected(run["out"].numpy(), gold["levels"], T)
        assert torch.equal(out[b:b + 1].cpu(), want), (run["seed"], run["set"])
        alone = staging.stage_classifier_clips(run["frames"], plan, img_dim, size=size)
        assert torch.equal(out[b:b + 1], alone), (run["seed"], run["set"])
    # with the batch flip, and the validation form (one launch writes fp32)
    flipped = staging.stage_classifier_clips_ragged(frames, plans, img_dim, flip=True, size=size)
    assert torch.equal(flipped, out.flip(-1))
    plain = [dict(p, program=[]) for p in plans]
    direct = staging.stage_classifier_clips_ragged(frames, plain, img_dim, size=size)
    for b, (run, _) in enumerate(batch):
        assert torch.equal(direct[b:b + 1], staging.stage_classifier_clips(run["frames"], plain[b], img_dim, size=size))


def test_training_batch():
    from coclr_amd import staging
    batch, S, T = RH.train_batch()
    shapes = [tuple(f.shape[1:3]) for f, _ in batch]
    k = shapes.index(RH.EDGE)
    x0, y0, w, h = batch[k][1]["box"][0]
    assert x0 + w == RH.EDGE[1] and y0 + h == RH.EDGE[0]                 # touches its own right and bottom edge
    assert shapes[k + 1][0] * shapes[k + 1][1] > RH.EDGE[0] * RH.EDGE[1]  # and a larger frame follows in the buffer
    frames = staging.ragged_from_frames([f for f, _ in batch])
    plans = [p for _, p in batch]
    out = staging.stage_train_clips_ragged(frames, plans, S)
    assert out.is_cuda and out.shape == (len(batch), 2, 3, T, S, S)
    for b, (f, plan) in enumerate(batch):
        assert torch.equal(out[b:b + 1].cpu(), TH.chain_reference(f[None].numpy(), [plan], S)), b
        assert torch.equal(out[b:b + 1], staging.stage_train_clips(f, plan, S)), b
    gold = TH.golden()
    for b, run in enumerate(gold["runs"]):
        assert torch.equal(out[b].cpu(), TH.levels_expected(run["out"].numpy(), gold["levels"], T)), run["seed"]
    order = [8, 0, 7, 3]
    again = staging.stage_train_clips_ragged(frames, [plans[b] for b in order], S, first=[b * 2 * T for b in order])
    assert torch.equal(again, out[order])


END_TO_END = ((40, 56, 3, (2, 2)), (37, 45, 3, (2, 1)), (33, 17, 1, (1, 1)), (16, 16, 3, (1, 1)), (240, 320, 3, (2, 2)))


def test_end_to_end():
    """T = 1: a sample is two frames of one fixture group; pack per sample, cat_ragged, decode_ragged,
    stage_train_clips_ragged -- against the same staging of the fixtures' own `rgb`."""
    from coclr_amd import jpeg, staging
    groups = J.groups()
    samples = [(groups[key] * 2)[:2] for key in END_TO_END]              # the 320 x 240 frame twice
    assert [(s[0]["width"], s[0]["height"]) for s in samples] == [(56, 40), (45, 37), (17, 33), (16, 16), (320, 240)]
    S = 32
    tt = staging.TrainTransform(S, 1)
    rng, np_rng = random.Random(5), np.random.RandomState(5)
    plans = [tt.draw(s[0]["width"], s[0]["height"], rng=rng, np_rng=np_rng) for s in samples]
    data, meta = jpeg.cat_ragged([jpeg.pack([J.raw(c) for c in s]) for s in samples])
    frames = jpeg.decode_ragged(data, meta)
    assert not bool(jpeg.decode_ragged.last_status.any())
    got = staging.stage_train_clips_ragged(frames, plans, S)
    known = staging.ragged_from_frames([torch.stack([c["rgb"] for c in s]) for s in samples])
    assert torch.equal(frames.offset, known.offset) and torch.equal(frames.height, known.height)
    want = staging.stage_train_clips_ragged(known, plans, S)
    assert got.shape == (5, 2, 3, 1, S, S) and torch.equal(got, want)
    for b, s in enumerate(samples):
        rgb = torch.stack([c["rgb"] for c in s])
        assert torch.equal(got[b:b + 1].cpu(), TH.chain_reference(rgb[None].numpy(), [plans[b]], S)), b


def test_single_size_equivalence():
    from coclr_amd import jpeg
    group = J.groups()[(40, 56, 3, (2, 2))]                              # five frames, with and without restart markers
    data, meta = jpeg.pack([J.raw(c) for c in group])
    for chunk_bytes in (0, 64):
        want, st = jpeg.decode(data, meta, return_status=True, chunk_bytes=chunk_bytes)
        frames, status = jpeg.decode_ragged(data, meta, return_status=True, chunk_bytes=chunk_bytes)
        assert torch.equal(status, st)
        n = want[0].numel()
        assert frames.offset.tolist() == [i * n for i in range(len(group))]
        assert torch.equal(frames.pixels[:want.numel()], want.reshape(-1))          # byte for byte


def test_kinetics_sizes_in_one_call():
    """tests/golden/jpeg_ragged.pt (tools/make_ragged_golden.py): four frames at kinetics400-256's sizes and the
    320 x 240 fixture in ONE ragged call against the one-size decode of each."""
    from coclr_amd import jpeg
    gold = torch.load(os.path.join(J.ROOT, "tests", "golden", "jpeg_ragged.pt"))
    cases = gold["cases"] + [J.case("320x240_420_q75")]
    assert [(c["width"], c["height"]) for c in cases[:4]] == [(340, 256), (454, 256), (256, 340), (320, 256)]
    packs = [jpeg.pack([J.raw(c)]) for c in cases]
    frames = jpeg.decode_ragged(*jpeg.cat_ragged(packs))
    assert not bool(jpeg.decode_ragged.last_status.any())
    for i, (d, m) in enumerate(packs):
        assert torch.equal(frames.frame(i), jpeg.decode(d, m)[0]), cases[i]["name"]
    assert torch.equal(frames.frame(4).cpu(), cases[4]["rgb"])
