"""Test clips of many videos in one launch on one MI355X (csrc/staging.hip: coclr_stage_crops_ragged;
staging.stage_crops_ragged; VideoEvaluator.add_videos / add_stored): every clip against the per-video kernel
(staging.stage_crops, which the existing tests hold to PIL bit for bit), the committed PIL fixture staged as mixed
batches, one launch against several, and the evaluator against a per-video add_frames loop.  ZERO tolerance: every
comparison is torch.equal -- the resampling is integer arithmetic and the float step is shared.  No test imports PIL."""
import random

import numpy as np
import pytest
import torch

import _jpeg_cases as J
import crops_harness as CH

pytestmark = pytest.mark.gpu

T, CROP = 4, 40
SIZES = ((57, 43, 3), (64, 48, 9), (48, 64, 10), (43, 57, 17), (80, 45, 17))          # W, H, frames
FILL = 7.0


@pytest.fixture(scope="module")
def videos():
    rng = np.random.RandomState(17)
    return [torch.from_numpy(rng.randint(0, 256, size=(F, H, W, 3)).astype(np.uint8)).cuda() for W, H, F in SIZES]


@pytest.fixture(scope="module")
def ragged(videos):
    from coclr_amd import staging
    frames = staging.ragged_from_frames(videos)
    assert (3 * 57 * 43) % 16 != 0 and int(frames.offset[1]) == (3 * 57 * 43 + 15) // 16 * 16        # padded
    return frames


def _ten(W, H, size=CROP):
    from coclr_amd import staging
    return staging.five_crop_boxes(W, H, size) * 2, [0] * 5 + [1] * 5


def _clips(index, firsts, sizes=SIZES, size=CROP):
    """Every (video, crop, clip) in the evaluator's order -> [(ids, box, flip)] and the video of each."""
    clips, owner = [], []
    for v, ((W, H, _), idx, first) in enumerate(zip(sizes, index, firsts)):
        boxes, flips = _ten(W, H, size)
        for box, fl in zip(boxes, flips):
            for row in idx:
                clips.append((row + first, box, fl))
                owner.append(v)
    return clips, owner


@pytest.fixture(scope="module")
def per_video(videos):
    """staging.stage_crops per video, the reference, once per (ds, S): fp32 (10 * n_clips, 3, T, S, S) per video."""
    from coclr_amd import staging
    memo = {}

    def get(ds, S):
        if (ds, S) not in memo:
            index = [staging.test_frame_index(F, T, ds) for _, _, F in SIZES]
            want = []
            for v, (W, H, _) in enumerate(SIZES):
                boxes, flips = _ten(W, H)
                want.append(staging.stage_crops(videos[v], index[v], boxes, flips, CROP, S).flatten(0, 1))
            memo[ds, S] = (index, want)
        return memo[ds, S]

    return get


# ---- (a) against the per-video kernel ---------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [16, 30, 40])
@pytest.mark.parametrize("ds", [1, 2])
def test_all_clips_of_all_videos_in_one_call(videos, ragged, per_video, ds, S):
    from coclr_amd import ops, staging
    index, want = per_video(ds, S)
    assert index[0].shape[0] == 1 and len(set(index[0][0].tolist())) < T             # shorter than a clip: left-padded
    firsts = np.cumsum([0] + [F for _, _, F in SIZES])[:-1]
    clips, owner = _clips(index, firsts)
    n = len(clips)
    assert n == 10 * sum(i.shape[0] for i in index) and n * T <= 65535              # ONE launch
    before = ragged.pixels.clone()
    big = torch.full((n + 2, 3, T, S, S), FILL, device="cuda")
    got = staging.stage_crops_ragged(ragged, clips, CROP, S, out=big[1:n + 1])
    assert got.data_ptr() == big[1].data_ptr()
    torch.cuda.synchronize()
    assert bool((big[0] == FILL).all()) and bool((big[n + 1] == FILL).all())        # rows beyond n: untouched
    assert torch.equal(ragged.pixels, before)                                         # and so are the frames
    at = 0
    for v in range(len(SIZES)):
        m = want[v].shape[0]
        assert owner[at] == v and owner[at + m - 1] == v
        assert torch.equal(got[at:at + m], want[v]), (v, ds, S)
        at += m
    assert at == n
    assert torch.equal(staging.stage_crops_ragged(ragged, clips, CROP, S), got)      # without `out`
    # the byte form: the same launch up to the second clamp, the input of coclr_color_jitter_clips
    desc, off = staging.crops_tables_ragged(ragged, clips, CROP)
    xmin, xk, ymin, yk = staging._device_tables(CROP, CROP, S, ragged.pixels.device)
    u8 = torch.full(((n + 2) * T, S, S, 3), 0x5a, dtype=torch.uint8, device="cuda")
    ops.stage_crops_ragged(ragged.pixels, desc.cuda(), desc, off.cuda(), off, CROP, CROP, S, xmin, xk, ymin, yk,
                           u8[T:(n + 1) * T])
    torch.cuda.synchronize()
    assert bool((u8[:T] == 0x5a).all()) and bool((u8[(n + 1) * T:] == 0x5a).all())
    at = 0
    for v, (W, H, _) in enumerate(SIZES):
        boxes, flips = _ten(W, H)
        crops = [(x0, y0, f) for (x0, y0), f in zip(boxes, flips)]
        k = index[v].shape[0]
        ref = torch.empty(10, k * T, S, S, 3, dtype=torch.uint8, device="cuda")
        ops.resize_crops_u8(videos[v], torch.as_tensor(index[v]).to(torch.int32).cuda(), crops, CROP, CROP, S, xmin,
                            xk, ymin, yk, ref)
        assert torch.equal(u8[T + at * T:T + (at + 10 * k) * T], ref.flatten(0, 1)), (v, ds, S)
        at += 10 * k
    # the bytes are what the fp32 form normalises: ToTensor + Normalize of them is the fp32 result
    levels = CH.golden()["levels"].cuda()
    b = u8[T:(n + 1) * T].view(n, T, S, S, 3).long()
    assert torch.equal(torch.stack([levels[c][b[..., c]] for c in range(3)], 1), got)


# ---- (b) against PIL's own bytes ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["A", "B_rect", "B_identity"])
def test_fixture_cases_in_a_mixed_batch(name):
    """A fixture case's clips interleaved with clips of the OTHER fixture video (another frame size) in one launch:
    the case's clips are PIL's bytes, the others the per-video kernel's."""
    from coclr_amd import staging
    golden = CH.golden()
    c = golden[name]
    other = golden["B_rect" if name == "A" else "A"]
    frames = staging.ragged_from_frames([c["frames"], other["frames"]])
    assert len({(int(h), int(w)) for h, w in zip(frames.height, frames.width)}) == 2
    cw, ch = c["crop"]
    S, Tc = c["S"], c["frame_index"].shape[1]
    want = CH.golden_expected(c, golden["levels"]).flatten(0, 1)
    mine = [(np.asarray(row), box, fl) for box, fl in zip(c["boxes"].tolist(), c["flips"].tolist())
            for row in c["frame_index"].tolist()]
    oF, oH, oW = other["frames"].shape[:3]
    theirs_idx = [[k % oF for k in range(j, j + Tc)] for j in range(2)]
    theirs_box = [(oW - cw, 0), (0, oH - ch)]
    theirs = [(np.asarray(row) + c["frames"].shape[0], box, fl) for box, fl in zip(theirs_box, (1, 0)) for row in theirs_idx]
    theirs_want = staging.stage_crops(other["frames"], theirs_idx, theirs_box, [1, 0], (cw, ch), S).flatten(0, 1)
    clips, src = [], []
    for k in range(max(len(mine), len(theirs))):                                      # interleaved
        for which, part in ((0, mine), (1, theirs)):
            if k < len(part):
                clips.append(part[k])
                src.append((which, k))
    got = staging.stage_crops_ragged(frames, clips, (cw, ch), S).cpu()
    for j, (which, k) in enumerate(src):
        assert torch.equal(got[j], (want, theirs_want.cpu())[which][k]), (name, which, k)


# ---- (c) one launch against several; permutation --------------------------------------------------------------------------

def test_one_launch_equals_several_and_permutes(ragged, per_video):
    from coclr_amd import staging
    index, _ = per_video(1, 30)
    firsts = np.cumsum([0] + [F for _, _, F in SIZES])[:-1]
    clips, _ = _clips(index, firsts)
    whole = staging.stage_crops_ragged(ragged, clips, CROP, 30)
    cuts = [0, 1, 7, 8, 150, len(clips) - 1, len(clips)]
    parts = torch.cat([staging.stage_crops_ragged(ragged, clips[a:b], CROP, 30) for a, b in zip(cuts, cuts[1:])])
    assert torch.equal(parts, whole)
    perm = random.Random(4).sample(range(len(clips)), len(clips))
    assert perm != sorted(perm)
    shuffled = staging.stage_crops_ragged(ragged, [clips[p] for p in perm], CROP, 30)
    assert torch.equal(shuffled, whole[torch.tensor(perm).cuda()])
    # with a jitter program per clip: two launches, the clip's own program, as stage_crops jitters a crop
    jit = staging.ColorJitter(0.2, 0.2, 0.2, 0.1, p=0.7)
    rng = random.Random(9)
    W, H, F = SIZES[3]
    boxes, flips = _ten(W, H)
    drawn = [jit.draw(rng, 1)[0] for _ in boxes]
    assert any(drawn) and len({len(p) for p in drawn}) > 1
    k = index[3].shape[0]
    sub = [(row + int(firsts[3]), box, fl) for box, fl in zip(boxes, flips) for row in index[3]]
    got = staging.stage_crops_ragged(ragged, sub, CROP, 30, jitter=[p for p in drawn for _ in range(k)])
    video = torch.stack([ragged.frame(int(firsts[3]) + f) for f in range(F)])
    want = staging.stage_crops(video, index[3], boxes, flips, CROP, 30, jitter=drawn).flatten(0, 1)
    assert torch.equal(got, want)


# ---- (d) the evaluator -------------------------------------------------------------------------------------------------------

class _TableModel(torch.nn.Module):
    """Stands in for the classifier: a clip -> the row of fixed tables that its first red byte names."""

    def __init__(self, num_class=11, width=6, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.logits = torch.nn.Parameter(torch.randn(256, num_class, generator=g) * 3, requires_grad=False)
        self.feats = torch.nn.Parameter(torch.randn(256, width, generator=g), requires_grad=False)

    def forward(self, block):
        from coclr_amd import staging
        x = block[:, 0, 0, 0, 0].double() * staging.IMAGENET_STD[0] + staging.IMAGENET_MEAN[0]
        idx = (x * 255).round().long().clamp(0, 255)
        return self.logits[idx], self.feats[idx]


def _same(got, want):
    assert torch.equal(got.probs, want.probs) and torch.equal(got.features, want.features)
    assert torch.equal(got.labels, want.labels)
    assert torch.equal(got.top1, want.top1) and torch.equal(got.top5, want.top5)
    assert bool(torch.isfinite(got.probs).all()) and float(got.probs.sum(1).sub(1).abs().max()) < 1e-4


@pytest.fixture(scope="module")
def stored():
    """A store whose videos are the fixtures of one frame size each, every fixture its own pack: four sizes (H x W)
    -> (store, [(first id, PIL's frames (F, H, W, 3))])."""
    from coclr_amd import jpeg
    store = jpeg.Store(1 << 20, 64)
    out = []
    for H, W in ((37, 45), (40, 56), (33, 17), (16, 16)):
        cases = [c for c in J.cases() if (c["height"], c["width"]) == (H, W)]
        ids = [store.add(jpeg.pack([J.raw(c)])) for c in cases]
        assert ids == list(range(ids[0], ids[0] + len(cases))) and len(cases) >= 8
        out.append((ids[0], torch.stack([c["rgb"] for c in cases])))
    return store, out


def _loop(model, vids, index, labels, jitter, seed, **kw):
    from coclr_amd.eval.video import VideoEvaluator
    ev = VideoEvaluator(model, batch_clips=8)
    rng = random.Random(seed)
    for v, idx, l in zip(vids, index, labels):
        ev.add_frames(v, idx, label=l, jitter=jitter, rng=rng, **kw)
    return ev.finish(), ev.passes


@pytest.mark.parametrize("jittered", [False, True])
def test_add_videos_and_add_stored_equal_the_add_frames_loop(stored, jittered):
    from coclr_amd import staging
    from coclr_amd.eval.video import VideoEvaluator
    store, vids = stored
    jitter = staging.ColorJitter(0.2, 0.2, 0.2, 0.1, p=0.7) if jittered else None
    kw = dict(crops="ten", crop_size=16, out_size=12)
    frames = [v for _, v in vids]
    index = [staging.test_frame_index(v.shape[0], T) for v in frames]
    labels = [2, 9, 4, 0]
    n_clips = 10 * sum(i.shape[0] for i in index)
    assert n_clips % 8 and any(i.shape[0] % 8 for i in index)                       # crops straddle the flushes
    model = _TableModel().cuda().eval()
    want, passes = _loop(model, frames, index, labels, jitter, 21, **kw)
    assert passes == -(-n_clips // 8) and passes > 8
    # from decoded frames
    rag = staging.ragged_from_frames(frames)
    firsts = np.cumsum([0] + [v.shape[0] for v in frames])
    ev = VideoEvaluator(model, batch_clips=8)
    ids = ev.add_videos(rag, [(int(firsts[k]), frames[k].shape[0], index[k], labels[k]) for k in range(4)], jitter=jitter,
                        rng=random.Random(21), **kw)
    assert ids == [0, 1, 2, 3]
    _same(ev.finish(), want)
    assert ev.passes == passes
    # from the store: all videos in one decode call, then cut into groups by max_stage_bytes
    for limit, calls in ((256 << 20, 1), (60000, 3)):
        seen, inner = [], store.decode
        store.decode = lambda ids, *a, **k: (seen.append(torch.as_tensor(ids).tolist()), inner(ids, *a, **k))[1]
        try:
            ev = VideoEvaluator(model, batch_clips=8)
            ids = ev.add_stored(store, [(vids[k][0], frames[k].shape[0], index[k], labels[k]) for k in range(4)],
                                jitter=jitter, rng=random.Random(21), max_stage_bytes=limit, **kw)
        finally:
            del store.decode
        assert ids == [0, 1, 2, 3] and len(seen) == calls
        assert sorted(i for s in seen for i in s) == list(range(vids[0][0], vids[-1][0] + frames[-1].shape[0]))
        _same(ev.finish(), want)
        assert ev.passes == passes


def test_add_stored_decodes_only_what_the_clips_read(stored):
    from coclr_amd.eval.video import VideoEvaluator
    store, vids = stored
    model = _TableModel().cuda().eval()
    rows = [[[3, 5, 5, 9]], [[12, 0, 0, 1]]]                                         # one clip each, train-mode style
    seen, inner = [], store.decode
    store.decode = lambda ids, *a, **k: (seen.append(torch.as_tensor(ids).tolist()), inner(ids, *a, **k))[1]
    try:
        ev = VideoEvaluator(model, batch_clips=8)
        ev.add_stored(store, [(vids[k][0], vids[k][1].shape[0], rows[k], k) for k in range(2)], crops="center",
                      crop_size=16, out_size=12)
    finally:
        del store.decode
    assert seen == [[vids[0][0] + f for f in (3, 5, 9)] + [vids[1][0] + f for f in (0, 1, 12)]]
    got = ev.finish()
    loop = VideoEvaluator(model, batch_clips=8)
    for k in range(2):
        loop.add_frames(vids[k][1], rows[k], label=k, crops="center", crop_size=16, out_size=12)
    _same(got, loop.finish())


def test_add_videos_equals_the_add_frames_loop_on_s3d():
    """Through a real LinearClassifier at the smallest S3D input (3 x 8 x 64 x 64), three videos of three frame sizes:
    the same clips fill the same rows of the same batches, so the scores are bit-identical."""
    from coclr_amd import staging
    from coclr_amd.eval.video import VideoEvaluator
    from coclr_amd.model.classifier import LinearClassifier
    torch.manual_seed(0)
    model = LinearClassifier(num_class=51, network='s3d').cuda().eval()
    rng = np.random.RandomState(5)
    size, S, T8 = 72, 64, 8
    shapes = ((5, 84, 100), (14, 100, 84), (9, 90, 96))
    vids = [torch.from_numpy(rng.randint(0, 256, size=s + (3,)).astype(np.uint8)) for s in shapes]
    index = [staging.test_frame_index(v.shape[0], T8) for v in vids]
    assert [i.shape[0] for i in index] == [1, 3, 1]
    labels = [3, 17, 40]
    kw = dict(crops="five", crop_size=size, out_size=S)
    want, passes = _loop(model, vids, index, labels, None, 0, **kw)
    rag = staging.ragged_from_frames(vids)
    firsts = np.cumsum([0] + [v.shape[0] for v in vids])
    ev = VideoEvaluator(model, batch_clips=8)
    ev.add_videos(rag, [(int(firsts[k]), vids[k].shape[0], index[k], labels[k]) for k in range(3)], **kw)
    got = ev.finish()
    torch.cuda.synchronize()
    assert ev.passes == passes == -(-5 * 5 // 8)
    _same(got, want)
