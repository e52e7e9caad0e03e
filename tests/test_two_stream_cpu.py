"""CPU tier of CoCLR's two-stream staging (coclr_amd/staging.py: two_stream_slots, TwoStreamClips,
stage_two_stream_clips, stage_two_stream_clips_ragged, stage_two_stream_clips_cropped, two_stream_frames): the draws of
TrainTransform(img_dim, 2 * T) against the reference's use of both generators under main_coclr.py's chain
(tests/golden/two_stream_transform.pt); the three entry forms on the kernel doubles of tests/train_harness.py and
tests/ragged_harness.py against the reference's four clips; the selections of two_stream_frames by hand; every
refusal; the views of blocks().  Every comparison is torch.equal."""
import random

import numpy as np
import pytest
import torch

import ragged_harness as RH
import train_harness as TH
import two_stream_harness as TS
from coclr_amd import staging

REVERSES = (None, False, True)


@pytest.fixture(scope="module")
def gold():
    return TS.golden()


@pytest.fixture(scope="module")
def plans(gold):
    return TS.fixture_plans(gold)


class CountedRandom:
    """Counts the calls `draw` makes, as the fixture's tool counted the reference's module-level calls."""

    def __init__(self, inner, names, count):
        for name in names:
            setattr(self, name, self._counted(getattr(inner, name), name, count))

    @staticmethod
    def _counted(fn, name, count):
        def call(*a, **kw):
            count[name] += 1
            return fn(*a, **kw)
        return call


def test_fixture_has_every_case(gold, plans):
    assert {c for run in gold["runs"] for c in run["covers"]} >= TS.COVERS
    S, T = gold["img_dim"], gold["seq_len"]
    assert (S, T) == (16, 3)
    for run in gold["runs"]:
        assert tuple(run["frames"].shape) == (4 * T, 40, 52, 3) and tuple(run["clips"].shape) == (4, T, S, S, 3)
    assert {plan["half"] for _, plan, _ in plans} == {(0, 1), (0, 0), (1, 1)}
    assert any(plan["box"][c] == (0, 0, 52, 40) for _, plan, _ in plans for c in range(2))
    # a gray clip whose channel differs between the RGB and the flow frame of one time step
    gray = [[op[1] for p in plan["programs"][c] for op in p if op[0] == staging.JITTER_GRAY]
            for _, plan, _ in plans for c in range(2)]
    assert any(len(ch) == 2 * T and any(ch[j] != ch[T + j] for j in range(T)) for ch in gray)


def test_draws_reproduce_the_fixture(gold, plans):
    """TrainTransform(img_dim, 2 T).draw under the run's seeds makes the reference's calls of both generators and
    leaves both where main_coclr.py's chain left them; the restated chain on its plan gives the reference's bytes."""
    S, T = gold["img_dim"], gold["seq_len"]
    tt = staging.TrainTransform(S, 2 * T)
    for run, plan, after in plans:
        assert after == (run["next"], run["np_next"]), run["seed"]
        count = {k: 0 for k in run["draws"]}
        random.seed(run["seed"])
        np.random.seed(run["seed"])
        again = tt.draw(52, 40, rng=CountedRandom(random, ("random", "uniform", "shuffle", "randint", "choices"), count),
                        np_rng=CountedRandom(np.random, ("choice",), count))
        assert count == run["draws"] and again == plan, run["seed"]
        assert all(len(plan["programs"][c]) == 2 * T for c in range(2))
        assert torch.equal(TS.chain_expected(run["frames"], plan, T, S), TS.expected(run, gold)), run["seed"]
        packed = staging.pack_plan(plan, 2 * T)
        assert packed.shape == (2, 5 + 16 * 2 * T)
        back = staging.unpack_plan(packed)
        assert back["half"] == tuple(plan["half"]) and [list(x) for x in back["programs"]] == \
            [list(x) for x in plan["programs"]]


def test_slots():
    name = {(0, 0): "x1", (0, 1): "f1", (1, 0): "x2", (1, 1): "f2"}
    for reverse in REVERSES:
        assert tuple(name[s] for s in staging.two_stream_slots(reverse)) == TS.SLOTS[reverse]
    for bad in (0, 1, "False", np.bool_(False), (False,)):
        with pytest.raises(ValueError):
            staging.two_stream_slots(bad)


def _batch(gold, plans):
    frames = torch.stack([run["frames"] for run, _, _ in plans])
    want = torch.stack([TS.expected(run, gold) for run, _, _ in plans], 1)          # (4, B, 3, T, S, S)
    return frames, [p for _, p, _ in plans], want


@pytest.mark.parametrize("reverse", REVERSES)
def test_one_size_form_on_the_doubles(monkeypatch, gold, plans, reverse):
    RH.install(monkeypatch)
    S, T = gold["img_dim"], gold["seq_len"]
    frames, each, want = _batch(gold, plans)
    B, n = len(each), len(TS.SLOTS[reverse])
    clips = staging.stage_two_stream_clips(frames, each, S, reverse=reverse, device="cpu")
    assert [c[0] for c in TH.CALLS] == ["boxes", "augment"] and TH.CALLS[0][1:] == (n * B, T)      # n B clips of T frames
    assert TH.CALLS[1][1:3] == (n * B * T, 1)                                                    # a gray clip: per frame
    assert isinstance(clips, staging.TwoStreamClips) and clips.reverse is reverse
    assert clips.out.shape == ((2, 2, B, 3, T, S, S) if reverse is None else (3, B, 3, T, S, S))
    assert clips.out.dtype == torch.float32
    TS.check(clips, want, reverse)
    # one sample alone, as a dict and 4-d frames; the packed plans through the default collate; `out`
    for b, (run, plan, _) in enumerate(plans):
        one = staging.stage_two_stream_clips(run["frames"], plan, S, reverse=reverse, device="cpu")
        TS.check(one, want[:, b:b + 1], reverse)
    packed = torch.stack([staging.pack_plan(p, 2 * T) for p in each])
    again = staging.stage_two_stream_clips(frames, packed, S, reverse=reverse, device="cpu")
    assert torch.equal(again.out, clips.out)
    out = torch.empty_like(clips.out)
    into = staging.stage_two_stream_clips(frames, each, S, reverse=reverse, out=out, device="cpu")
    assert into.out is out and torch.equal(out, clips.out)


@pytest.mark.parametrize("reverse", REVERSES)
def test_ragged_and_cropped_forms_on_the_doubles(monkeypatch, gold, reverse):
    """A mixed batch (four frame sizes): the ragged form on all 4 T frames in the dataset's order, on a full-frame
    selection without the quarters nothing reads, and the cropped form, each against the reference's bytes (fixture
    samples) or the restated chain (the others)."""
    RH.install(monkeypatch)
    S, T = gold["img_dim"], gold["seq_len"]
    batch = TS.mixed_batch(gold)
    B, n = len(batch), len(TS.SLOTS[reverse])
    assert len({tuple(f.shape[1:3]) for f, _, _ in batch}) == 4
    each = [p for _, p, _ in batch]
    want = torch.stack([w for _, _, w in batch], 1)
    whole = staging.ragged_from_frames([f for f, _, _ in batch], device="cpu")
    clips = staging.stage_two_stream_clips_ragged(whole, each, S, reverse=reverse)
    assert RH.CALLS == [("boxes", n * B, T)] and [c[0] for c in TH.CALLS] == ["augment"]
    TS.check(clips, want, reverse)
    store = TS.Frames("cpu")
    ids = [store.add(f) for f, _, _ in batch]
    ids_rgb, ids_flow = torch.tensor([a for a, _ in ids]), torch.tensor([b for _, b in ids])
    sel, first = staging.two_stream_frames(ids_rgb, ids_flow, each, T, reverse=reverse, boxes=False,
                                           frame_size=store.frame_size)
    assert sel.numel() < 4 * T * B and bool((first == -1).any())                  # something is not decoded
    part = staging.stage_two_stream_clips_ragged(store.decode(sel), each, S, first=first, reverse=reverse)
    assert torch.equal(part.out, clips.out)
    sel, boxes = staging.two_stream_frames(ids_rgb, ids_flow, each, T, reverse=reverse)
    assert sel.shape == (n * B * T,) and boxes.shape == (n * B * T, 4)
    del RH.CALLS[:], TH.CALLS[:]
    cropped = staging.stage_two_stream_clips_cropped(store.decode(sel, boxes), each, S, reverse=reverse)
    assert RH.CALLS == [("boxes", n * B, T)] and [c[0] for c in TH.CALLS] == ["augment"]
    assert torch.equal(cropped.out, clips.out)
    out = torch.empty_like(clips.out)
    assert staging.stage_two_stream_clips_cropped(store.decode(sel, boxes), each, S, reverse=reverse, out=out).out is out
    assert torch.equal(out, clips.out)
    # another order of samples through `first`
    order = [B - 1, 0, 3]
    full = torch.tensor([[4 * T * b + T * q for q in range(4)] for b in order])
    again = staging.stage_two_stream_clips_ragged(whole, [each[b] for b in order], S, first=full, reverse=reverse)
    TS.check(again, want[:, order], reverse)


# ---- two_stream_frames by hand -----------------------------------------------------------------------------------

def _plan(half, box, T):
    return {"half": half, "box": box, "programs": ([[]] * (2 * T), [[(staging.AUGMENT_FLIP, 0.0)]] * (2 * T))}


def test_two_stream_frames_by_hand():
    T = 2
    A, Bx = (4, 5, 20, 10), (0, 0, 52, 40)
    two, lo, hi = _plan((0, 1), (A, Bx), T), _plan((0, 0), (A, Bx), T), _plan((1, 1), (A, Bx), T)
    rgb = torch.tensor([[10, 11, 12, 13], [20, 21, 22, 23], [30, 31, 32, 33]])
    flow = rgb + 100
    each = [two, lo, hi]
    # per sample the ids of its quarters 0..3 under its plan's halves, per tensor
    q = {"x1": [[10, 11], [20, 21], [32, 33]], "f1": [[110, 111], [120, 121], [132, 133]],
         "x2": [[12, 13], [20, 21], [32, 33]], "f2": [[112, 113], [120, 121], [132, 133]]}
    box = {"x1": A, "f1": A, "x2": Bx, "f2": Bx}
    for reverse in REVERSES:
        sel, boxes = staging.two_stream_frames(rgb, flow, each, T, reverse=reverse)
        assert sel.dtype == torch.int64 and boxes.dtype == torch.int64
        assert sel.tolist() == [i for name in TS.SLOTS[reverse] for b in range(3) for i in q[name][b]]
        assert boxes.tolist() == [list(box[name]) for name in TS.SLOTS[reverse] for b in range(3) for _ in range(T)]
    # full frames: per sample the quarters read, once each, in the dataset's order; the others are absent
    sel, first = staging.two_stream_frames(rgb, flow, each, T, boxes=False)
    assert sel.tolist() == [10, 11, 110, 111, 12, 13, 112, 113, 20, 21, 120, 121, 32, 33, 132, 133]
    assert first.tolist() == [[0, 2, 4, 6], [8, 10, -1, -1], [-1, -1, 12, 14]] and first.dtype == torch.int64
    sel, first = staging.two_stream_frames(rgb, flow, each, T, reverse=False, boxes=False)       # f1 is not read
    assert sel.tolist() == [10, 11, 12, 13, 112, 113, 20, 21, 120, 121, 32, 33, 132, 133]
    assert first.tolist() == [[0, -1, 2, 4], [6, 8, -1, -1], [-1, -1, 10, 12]]
    sel, first = staging.two_stream_frames(rgb, flow, each, T, reverse=True, boxes=False)        # x1 is not read
    assert sel.tolist() == [110, 111, 12, 13, 112, 113, 20, 21, 120, 121, 32, 33, 132, 133]
    assert first.tolist() == [[-1, 0, 2, 4], [6, 8, -1, -1], [-1, -1, 10, 12]]
    # lists and the packed tensor will do
    packed = torch.stack([staging.pack_plan(p, 2 * T) for p in each])
    sel2, first2 = staging.two_stream_frames(rgb.tolist(), flow.tolist(), packed, T, reverse=True, boxes=False)
    assert torch.equal(sel2, sel) and torch.equal(first2, first)
    # refusals
    for bad_rgb, bad_flow, bad_plans, kw in (
            (rgb[:, :3], flow, each, {}), (rgb, flow[:, :3], each, {}), (rgb.float(), flow, each, {}),
            (rgb, flow.double(), each, {}), (rgb.view(-1), flow, each, {}), (rgb, flow[:2], each[:2], {}),
            (rgb[:2], flow, each, {}), (rgb, flow, each[:2], {}), (rgb, flow, each, {"reverse": 1}),
            (rgb, flow, [two, lo, _plan((0, 2), (A, Bx), T)], {}),
            (rgb, flow, each, {"frame_size": lambda i: (52, 40) if i < 100 or i >= 130 else (52, 41)})):
        with pytest.raises(ValueError):
            staging.two_stream_frames(bad_rgb, bad_flow, bad_plans, T, **kw)
    staging.two_stream_frames(rgb, flow, each, T, frame_size=lambda i: (52, 40))


# ---- refusals, before any launch ------------------------------------------------------------------------------------

def test_refusals(monkeypatch, gold, plans):
    RH.install(monkeypatch)
    S, T = gold["img_dim"], gold["seq_len"]
    run, plan, _ = plans[0]
    fr = run["frames"]
    one_stream = staging.TrainTransform(S, T).draw(52, 40, rng=random.Random(1), np_rng=np.random.RandomState(1))
    short = dict(plan, programs=(plan["programs"][0], plan["programs"][1][:2 * T - 1]))
    stage = staging.stage_two_stream_clips
    for frames, p, kw in ((fr, one_stream, {}),                                     # programs T long, not 2 T
                          (fr, short, {}),
                          (fr[:4 * T - 1], plan, {}), (fr[:2 * T], plan, {}),       # not 4 T frames
                          (torch.cat([fr, fr[:4]]), plan, {}),                      # 4 (T + 1) frames: the plan is for T
                          (fr.float(), plan, {}), (fr, [plan, plan], {}),
                          (fr, plan, {"reverse": 0}), (fr, plan, {"reverse": "yes"}),
                          (fr, plan, {"out": torch.empty(1, 2, 3, T, S, S)}),       # the one-stream shape
                          (fr, plan, {"out": torch.empty(3, 1, 3, T, S, S)}),       # a three-clip out, four clips
                          (fr, plan, {"reverse": False, "out": torch.empty(2, 2, 1, 3, T, S, S)}),
                          (fr, plan, {"reverse": True, "out": torch.empty(3, 1, 3, T, S, S + 1)}),
                          (fr, dict(plan, half=(0, 2)), {}),
                          (fr, dict(plan, box=(plan["box"][0], (40, 0, 16, 16))), {})):
        with pytest.raises(ValueError):
            stage(frames, p, S, device="cpu", **kw)
    with pytest.raises(ValueError):
        stage(fr, plan, 225, device="cpu")
    # the ragged form: frames, first, missing quarters, mixed sizes
    ragged = staging.stage_two_stream_clips_ragged
    whole = staging.ragged_from_frames([fr], device="cpu")
    two = [p for _, p, _ in plans if p["half"] == (0, 1)][0]
    lo = [p for _, p, _ in plans if p["half"] == (0, 0)][0]
    for frames, p, kw in ((whole, one_stream, {}), (whole.pixels, plan, {}),
                          (whole, plan, {"first": [0, T, 2 * T, 3 * T]}),           # not (B, 4)
                          (whole, plan, {"first": torch.tensor([[0.0, T, 2 * T, 3 * T]])}),
                          (whole, plan, {"first": [[0, T, 2 * T, 3 * T + 1]]}),      # leaves the frames
                          (whole, plan, {"first": [[0, T, 2 * T, -2]]}),
                          (whole, plan, {"first": [[-1, -1, -1, -1]]}),
                          (whole, two, {"first": [[0, -1, 2 * T, 3 * T]]}),          # f1's quarter is missing, f1 staged
                          (whole, two, {"first": [[0, -1, 2 * T, 3 * T]], "reverse": True}),
                          (whole, two, {"first": [[-1, T, 2 * T, 3 * T]], "reverse": False}),
                          (whole, lo, {"first": [[0, -1, 2 * T, 3 * T]], "reverse": True}),    # half 0 twice: f2 reads quarter 1
                          (whole, plan, {"reverse": 2}),
                          (whole, plan, {"out": torch.empty(1, 2, 3, T, S, S)})):
        with pytest.raises(ValueError):
            ragged(frames, p, S, **kw)
    # a missing quarter nothing reads is fine: f1 with reverse=False, x1 with reverse=True, the abandoned half
    ragged(whole, two, S, first=[[0, -1, 2 * T, 3 * T]], reverse=False)
    ragged(whole, two, S, first=[[-1, T, 2 * T, 3 * T]], reverse=True)
    ragged(whole, lo, S, first=[[0, T, -1, -1]])
    del RH.CALLS[:], TH.CALLS[:]
    # RGB and flow of different sizes inside one sample; frames of one quarter that differ; a quarter off the stride
    T4 = [fr[k * T:(k + 1) * T] for k in range(4)]
    mixed = staging.ragged_from_frames([T4[0], T4[1][:, :39], T4[2], T4[3][:, :39]], device="cpu")
    inside = staging.ragged_from_frames([T4[0][:2], T4[0][2:, :, :51], T4[1], T4[2], T4[3]], device="cpu")
    n = 3 * 40 * 52
    spread = staging.RaggedFrames(torch.zeros(13 * n, dtype=torch.uint8), [k * n + (16 if k else 0) for k in range(12)],
                                  [40] * 12, [52] * 12)
    for bad in (mixed, inside, spread):
        with pytest.raises(ValueError):
            ragged(bad, two, S)
    # the cropped form: the frames are the slots' clips, each of its box's size
    store = TS.Frames("cpu")
    a, b = store.add(fr)
    for reverse in REVERSES:
        sel, boxes = staging.two_stream_frames([a], [b], [two], T, reverse=reverse)
        good = store.decode(sel, boxes)
        other = None if reverse is not None else False
        wrong = boxes.clone()
        wrong[T:2 * T, 2] -= 1                                                      # the second slot's clip: not its box
        for frames, p, kw in ((good, two, {"reverse": other}),                      # three clips' frames for four, or back
                              (store.decode(sel[:-1], boxes[:-1]), two, {"reverse": reverse}),
                              (store.decode(sel, wrong), two, {"reverse": reverse}),
                              (good, one_stream, {"reverse": reverse}),
                              (good.pixels, two, {"reverse": reverse}),
                              (good, two, {"reverse": reverse, "out": torch.empty(1, 2, 3, T, S, S)})):
            with pytest.raises(ValueError):
                staging.stage_two_stream_clips_cropped(frames, p, S, **kw)
    assert not RH.CALLS and not TH.CALLS                                            # refused before any call


# ---- blocks() ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reverse", REVERSES)
def test_blocks_are_views(reverse):
    B, T, S = 3, 2, 4
    n = len(TS.SLOTS[reverse])
    out = torch.arange(n * B * 3 * T * S * S, dtype=torch.float32).view(
        (2, 2, B, 3, T, S, S) if reverse is None else (3, B, 3, T, S, S))
    clips = staging.TwoStreamClips(out, reverse)
    assert clips.out is out
    step = B * 3 * T * S * S * 4
    for k, name in enumerate(TS.SLOTS[reverse]):
        t = getattr(clips, name)
        assert t.shape == (B, 3, T, S, S) and t.is_contiguous() and t.data_ptr() == out.data_ptr() + k * step
    for name in set(TS.NAMES) - set(TS.SLOTS[reverse]):
        assert getattr(clips, name) is None
    block1, block2 = clips.blocks()
    assert block1.shape == block2.shape == (B, 2, 3, T, S, S)
    # what CoCLR.forward reads of the blocks (model/pretrain.py: _split_pair, then the swap under `reverse`)
    x1, f1, x2, f2 = block1[:, 0], block1[:, 1], block2[:, 0], block2[:, 1]
    read = {"x1": x1, "f1": f1, "x2": x2, "f2": f2}
    for name in TS.SLOTS[reverse]:
        t = getattr(clips, name)
        assert read[name].is_contiguous() and read[name].data_ptr() == t.data_ptr() and torch.equal(read[name], t), name
    # the aliasing of the three-clip forms, as the docstring states it
    if reverse is False:
        assert f1.data_ptr() == clips.x2.data_ptr()
    if reverse is True:
        assert x1.data_ptr() == clips.f2.data_ptr()
    for bad in (out[..., :-1], out.view(-1), out.view((n * B, 3, T, S, S))):
        with pytest.raises(ValueError):
            staging.TwoStreamClips(bad, reverse)
    with pytest.raises(ValueError):
        staging.TwoStreamClips(out, None if reverse is not None else False)
