"""CoCLR's two-stream staging on one MI355X (coclr_amd/staging.py: stage_two_stream_clips and its ragged and cropped
forms, two_stream_frames, TwoStreamClips; the kernels are stage_train_clips' own: coclr_resize_boxes_u8,
coclr_resize_boxes_ragged_u8, coclr_augment_clips, and the store's decode): the fixture of the reference's own transform
under main_coclr.py's chain (tests/golden/two_stream_transform.pt) staged as one batch through all three forms; a batch
of mixed frame sizes; the cropped form on a JPEG store against full-frame decode; the three-clip results against the
four-clip one; CoCLR.forward on three-clip blocks against four-clip blocks.  ZERO tolerance: every comparison is
torch.equal."""
import random

import numpy as np
import pytest
import torch

import _jpeg_cases as J
import two_stream_harness as TS

pytestmark = pytest.mark.gpu

REVERSES = (None, False, True)


@pytest.fixture(scope="module")
def gold():
    return TS.golden()


def _stored(batch):
    """The batch's frames in a TS.Frames on the device and its (ids_rgb, ids_flow)."""
    store = TS.Frames("cuda")
    ids = [store.add(f) for f, _, _ in batch]
    return store, torch.tensor([a for a, _ in ids]), torch.tensor([b for _, b in ids])


def _all_forms(batch, S, T, one_size):
    """Every form and every `reverse` on the batch [(frames, plan, want (4, 3, T, S, S))] against `want`; the three-clip
    tensors against the four-clip ones."""
    from coclr_amd import staging
    B = len(batch)
    each = [p for _, p, _ in batch]
    want = torch.stack([w for _, _, w in batch], 1)                                  # (4, B, 3, T, S, S)
    whole = staging.ragged_from_frames([f for f, _, _ in batch])
    store, ids_rgb, ids_flow = _stored(batch)
    four = None
    for reverse in REVERSES:
        n = len(TS.SLOTS[reverse])
        got = []
        if one_size:
            got.append(staging.stage_two_stream_clips(torch.stack([f for f, _, _ in batch]), each, S, reverse=reverse))
        got.append(staging.stage_two_stream_clips_ragged(whole, each, S, reverse=reverse))
        sel, first = staging.two_stream_frames(ids_rgb, ids_flow, each, T, reverse=reverse, boxes=False,
                                               frame_size=store.frame_size)
        assert sel.numel() < 4 * T * B
        got.append(staging.stage_two_stream_clips_ragged(store.decode(sel), each, S, first=first, reverse=reverse))
        sel, boxes = staging.two_stream_frames(ids_rgb, ids_flow, each, T, reverse=reverse)
        assert sel.shape == (n * B * T,)
        got.append(staging.stage_two_stream_clips_cropped(store.decode(sel, boxes), each, S, reverse=reverse))
        for clips in got:
            assert clips.out.is_cuda and clips.out.dtype == torch.float32 and clips.out.is_contiguous()
            assert clips.out.shape == ((2, 2, B, 3, T, S, S) if reverse is None else (3, B, 3, T, S, S))
            TS.check(clips, want, reverse)
            assert torch.equal(clips.out, got[0].out)
            if four is None:
                four = clips
            for name in TS.SLOTS[reverse]:                                           # three clips against four
                assert torch.equal(getattr(clips, name), getattr(four, name)), (name, reverse)
            block1, block2 = clips.blocks()
            read = {"x1": block1[:, 0], "f1": block1[:, 1], "x2": block2[:, 0], "f2": block2[:, 1]}
            for name in TS.SLOTS[reverse]:
                assert read[name].is_contiguous() and read[name].data_ptr() == getattr(clips, name).data_ptr()


def test_fixture_batch_in_every_form(gold):
    """All seeds of the fixture as ONE batch, 40 x 52 to 16 x 16 at T = 3, against the reference's bytes."""
    S, T = gold["img_dim"], gold["seq_len"]
    batch = [(run["frames"], plan, TS.expected(run, gold)) for run, plan, _ in TS.fixture_plans(gold)]
    assert len(batch) == len(gold["runs"]) >= 6 and {c for run in gold["runs"] for c in run["covers"]} >= TS.COVERS
    _all_forms(batch, S, T, True)


def test_mixed_sizes(gold):
    """40 x 52 next to 8 x 96, 57 x 41 (frames that are no multiple of 16 bytes) and 24 x 192 in one batch."""
    S, T = gold["img_dim"], gold["seq_len"]
    batch = TS.mixed_batch(gold)
    assert len({tuple(f.shape[1:3]) for f, _, _ in batch}) == 4
    _all_forms(batch, S, T, False)


def test_cropped_form_on_a_jpeg_store():
    """RGB and flow videos in ONE jpeg.Store under different ids, each one fixture geometry repeated to 2 T frames and
    more: two_stream_frames + decode(sel, boxes) + the cropped form equal full-frame decode + the ragged form, and the
    ragged form on all 4 T frames decoded in the dataset's order."""
    from coclr_amd import jpeg, staging
    T, S, B = 2, 16, 6
    groups = J.groups()
    geoms = [(40, 56, 3, (2, 2)), (37, 45, 3, (2, 1))]
    store = jpeg.Store(1 << 20, 128)
    videos = []                                                   # per geometry (first rgb id, first flow id, length)
    for key in geoms:
        g = groups[key]
        rgb = (g * 3)[:max(2 * T + 1, len(g))]
        flow = (g[::-1] * 3)[:len(rgb)]
        videos.append((store.add(jpeg.pack([J.raw(c) for c in rgb])), store.add(jpeg.pack([J.raw(c) for c in flow])),
                       len(rgb)))
        assert len(rgb) >= 2 * T
    tt = staging.TrainTransform(S, 2 * T)
    rng, np_rng, pick = random.Random(0), np.random.RandomState(0), random.Random(1)
    ids_rgb, ids_flow, plans = [], [], []
    for b in range(B):
        r0, f0, n = videos[b % 2]
        index = [pick.randrange(n) for _ in range(2 * T)]        # the SAME frame indices of both videos
        ids_rgb.append([r0 + i for i in index])
        ids_flow.append([f0 + i for i in index])
        assert store.frame_size(ids_rgb[-1][0]) == store.frame_size(ids_flow[-1][0])
        plans.append(tt.draw(*store.frame_size(ids_rgb[-1][0]), rng=rng, np_rng=np_rng))
    ids_rgb, ids_flow = torch.tensor(ids_rgb), torch.tensor(ids_flow)
    assert {p["half"] for p in plans} == {(0, 1), (0, 0), (1, 1)}
    order = torch.cat([ids_rgb[:, :T], ids_flow[:, :T], ids_rgb[:, T:], ids_flow[:, T:]], 1)     # the dataset's order
    everything = store.decode(order.reshape(-1))
    assert not bool(store.decode.last_status.any())
    four = staging.stage_two_stream_clips_ragged(everything, plans, S)
    for reverse in REVERSES:
        n = len(TS.SLOTS[reverse])
        sel, boxes = staging.two_stream_frames(ids_rgb, ids_flow, plans, T, reverse=reverse, frame_size=store.frame_size)
        assert sel.shape == (n * B * T,) and boxes.shape == (n * B * T, 4)
        cropped = staging.stage_two_stream_clips_cropped(store.decode(sel, boxes), plans, S, reverse=reverse)
        assert not bool(store.decode.last_status.any())
        sel, first = staging.two_stream_frames(ids_rgb, ids_flow, plans, T, reverse=reverse, boxes=False)
        assert sel.numel() < 4 * T * B
        full = staging.stage_two_stream_clips_ragged(store.decode(sel), plans, S, first=first, reverse=reverse)
        assert cropped.out.shape == ((2, 2, B, 3, T, S, S) if reverse is None else (3, B, 3, T, S, S))
        assert torch.equal(cropped.out, full.out)
        for name in TS.SLOTS[reverse]:
            assert torch.equal(getattr(cropped, name), getattr(four, name)), (name, reverse)
    # a flow video of another size than its RGB video is refused on the host
    bad_flow = ids_flow.clone()
    bad_flow[0] = ids_flow[1]
    with pytest.raises(ValueError):
        staging.two_stream_frames(ids_rgb, bad_flow, plans, T, frame_size=store.frame_size)
    sel, first = staging.two_stream_frames(ids_rgb, bad_flow, plans, T, boxes=False)
    with pytest.raises(ValueError):
        staging.stage_two_stream_clips_ragged(store.decode(sel), plans, S, first=first)


@pytest.mark.parametrize("queue", ["cold", "full"])
@pytest.mark.parametrize("reverse", [False, True])
def test_coclr_forward_reads_three_clips(reverse, queue):
    """On the clip of the small CoCLR cases (tests/_cases.py: 3 x 16 x 64 x 64, B = 4, K = 32): a training forward on
    the three-clip blocks gives the logits and the mask of one on the four-clip blocks, bit for bit -- the stream of
    block1 that aliases a neighbouring slot is never read."""
    import model.pretrain as product
    from _cases import build_model, load_golden
    from coclr_amd import staging
    cfg = dict(load_golden("coclr_s3d_small")["cfg"], reverse=reverse)
    if queue == "cold":
        del cfg["prefill"]
    B, (_, T, S, _) = cfg["B"], cfg["clip"]
    H, W = 72, 88
    frames = torch.from_numpy(np.random.RandomState(3).randint(0, 256, size=(B, 4 * T, H, W, 3)).astype(np.uint8)).cuda()
    tt = staging.TrainTransform(S, 2 * T)
    rng, np_rng = random.Random(2), np.random.RandomState(2)
    plans = [tt.draw(W, H, rng=rng, np_rng=np_rng) for _ in range(B)]
    vname = torch.randint(0, cfg["n_sources"], (B,), generator=torch.Generator().manual_seed(1)).cuda()
    four = staging.stage_two_stream_clips(frames, plans, S)
    three = staging.stage_two_stream_clips(frames, plans, S, reverse=reverse)
    unread = "f1" if reverse is False else "x1"
    assert getattr(three, unread) is None and not torch.equal(getattr(four, unread), getattr(four, "x2" if not reverse else "f2"))
    results = []
    for clips in (four, three):
        model = build_model(cfg, product).cuda()                   # the same weights and queues from the case's seeds
        model.train()
        model.sampler.eval()                                       # main_coclr.py:363
        assert model.reverse is reverse
        torch.manual_seed(cfg["perm_seed"])
        logits, mask = model(*clips.blocks(), vname)
        torch.cuda.synchronize()
        assert model.queue_is_full == (queue == "full")
        results.append((logits.detach().clone(), mask.clone(), int(model.queue_ptr)))
    (l4, m4, p4), (l3, m3, p3) = results
    assert l4.shape == (B, 1 + cfg["K"]) and m4.shape == (B, 1 + cfg["K"]) and p4 == p3 == B
    assert torch.equal(l3, l4) and torch.equal(m3, m4)
    assert bool(torch.isfinite(l4).all()) and bool(m4[:, 0].all())
    if queue == "full":
        assert int(m4[:, 1:].sum()) > 0                            # the mined positives
