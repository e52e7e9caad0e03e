"""CPU tier of the five/ten-crop staging (coclr_amd/staging.py: stage_crops and its host helpers;
coclr_amd/eval/video.py: VideoEvaluator.add_frames; csrc/staging.hip: coclr_stage_crops): the integer restatement
of tests/crops_harness.py against PIL itself and against the committed fixture, the product's host-side tables,
boxes and frame sampling against the reference's formulas, the evaluator's host logic on the doubles, and the C
ABI of the new entry point."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import crops_harness as CH
from coclr_amd import _lib, ops, staging
from coclr_amd.eval.video import VideoEvaluator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return CH.golden()


def _ten(W, H, size):
    boxes = staging.five_crop_boxes(W, H, size)
    return [(x0, y0, f) for f in (0, 1) for x0, y0 in boxes]


def _pil_u8(frames, crops, cw, ch, S):
    from PIL import Image
    out = []
    for x0, y0, flip in crops:
        per = []
        for f in frames:
            img = Image.fromarray(f)
            if flip:
                img = img.transpose(Image.FLIP_LEFT_RIGHT)
            per.append(np.asarray(img.crop((x0, y0, x0 + cw, y0 + ch)).resize((S, S), Image.BICUBIC)))
        out.append(np.stack(per))
    return out


def test_restatement_equals_pil(golden):
    pytest.importorskip("PIL")
    cases = []
    for name in ("A", "B_rect", "B_identity"):
        c = golden[name]
        cases.append((name, c["frames"].numpy(), CH.case_crops(c), c["crop"][0], c["crop"][1], c["S"]))
    big = np.random.RandomState(3).randint(0, 256, size=(1, 256, 340, 3)).astype(np.uint8)
    big[0, ::2, 100:200] = 255                         # hard edges: the clamp is live at the production size too
    big[0, 1::2, 100:200] = 0
    cases.append(("256x340", big, _ten(340, 256, 224), 224, 224, 128))
    for name, frames, crops, cw, ch, S in cases:
        want = _pil_u8(frames, crops, cw, ch, S)
        got = CH.crop_resized_u8(frames, crops, cw, ch, S)
        for k, (w, g) in enumerate(zip(want, got)):
            assert np.array_equal(w, g), "%s crop %d %s" % (name, k, crops[k])
        if any(f for _, _, f in crops):
            # the flip comes BEFORE the crop: cropping first and mirroring the box is another picture
            wrong = CH.crop_resized_u8(frames, crops, cw, ch, S, flip_after_crop=True)
            assert any(not np.array_equal(w, g) for w, g in zip(want, wrong)), name
    # the clamp is reached at both ends, and the identity resize returns the source bytes
    a = np.stack(CH.crop_resized_u8(golden["A"]["frames"].numpy(), CH.case_crops(golden["A"]), 28, 28, 16))
    assert a.min() == 0 and a.max() == 255
    c = golden["B_identity"]
    x0, y0, _ = CH.case_crops(c)[0]
    assert torch.equal(c["resized"][0, 0], c["frames"][0, y0:y0 + 16, x0:x0 + 16])
    assert torch.equal(c["resized"][1, 0], c["frames"][0].flip(1)[y0:y0 + 16, x0:x0 + 16])


@pytest.mark.parametrize("name", ["A", "B_rect", "B_identity"])
def test_fixture_equals_restatement(golden, name):
    c = golden[name]
    want = CH.golden_expected(c, golden["levels"])
    got = CH.reference(c["frames"], c["frame_index"], CH.case_crops(c), c["crop"][0], c["crop"][1], c["S"])
    assert want.dtype == torch.float32 and want.shape == got.shape and torch.equal(want, got)
    # `levels` is ToTensor + Normalize of every byte
    assert torch.equal(golden["levels"], CH.normalise(np.arange(256, dtype=np.uint8)[:, None].repeat(3, 1)).t())


def test_fixture_covers_the_cases(golden):
    a = golden["A"]
    assert tuple(a["frames"].shape) == (6, 40, 52, 3) and a["frame_index"].tolist() == [[0, 1, 2, 3], [2, 3, 4, 5],
                                                                                       [0, 0, 0, 1]]
    assert set(a["frames"][5].unique().tolist()) == {0, 255}
    assert CH.case_crops(a) == _ten(52, 40, 28) and a["crop"] == (28, 28) and a["S"] == 16
    assert {(x0 + 28, y0 + 28) for x0, y0, _ in CH.case_crops(a)} >= {(52, 40)}       # the frame's far corner
    assert golden["B_rect"]["crop"] == (12, 20) and golden["B_identity"]["crop"] == (16, 16)
    assert os.path.getsize(CH.GOLDEN) < 200 * 1024


@pytest.mark.parametrize("n_in,n_out,taps", [(224, 128, 9), (28, 16, 9), (12, 16, 5), (16, 16, 5), (20, 16, 7)])
def test_resample_tables(n_in, n_out, taps):
    lo, K = staging.resample_tables(n_in, n_out)
    want_lo, want_K = CH.tables(n_in, n_out)
    assert lo.dtype == np.int32 and K.dtype == np.int32 and K.shape == (n_out, taps)
    assert np.array_equal(lo, want_lo) and np.array_equal(K, want_K)
    assert int(np.abs(K.sum(1) - (1 << 22)).max()) <= taps            # rows sum to one, up to the rounding
    assert int(np.abs(K.astype(np.int64)).sum(1).max()) * 255 < 2 ** 31 - 2 ** 21      # int32 cannot overflow
    assert int((lo + (K != 0).cumsum(1).argmax(1)).max()) < n_in      # the last live tap is inside the source
    if n_in == n_out:
        assert all(K[i, j] == ((1 << 22) if lo[i] + j == i else 0) for i in range(n_out) for j in range(taps))


def test_five_crop_boxes():
    assert staging.five_crop_boxes(340, 256, 224) == [(58, 16), (0, 0), (116, 0), (0, 32), (116, 32)]
    # Python's round: halves to even -- (53-28)/2 = 12.5 -> 12, (55-28)/2 = 13.5 -> 14
    assert staging.five_crop_boxes(53, 40, 28, where=(5,)) == [(12, 6)]
    assert staging.five_crop_boxes(55, 43, 28, where=(5,)) == [(14, 8)]
    assert staging.five_crop_boxes(52, 40, 28, where=(4, 1)) == [(24, 12), (0, 0)]
    assert staging.five_crop_boxes(28, 28, 28) == [(0, 0)] * 5
    for W, H in ((27, 40), (40, 27)):
        with pytest.raises(ValueError):
            staging.five_crop_boxes(W, H, 28)
    with pytest.raises(ValueError):
        staging.five_crop_boxes(52, 40, 28, where=(6,))


def test_test_frame_index():
    idx = staging.test_frame_index(100, 32, 1)
    assert idx.dtype == np.int64 and idx.shape == (5, 32)
    assert idx[:, 0].tolist() == [0, 15, 30, 45, 60] and np.array_equal(idx[3], np.arange(45, 77))
    assert staging.test_frame_index(32, 32, 1).tolist() == [list(range(32))]
    assert staging.test_frame_index(20, 32, 1).tolist() == [[0] * 12 + list(range(20))]
    idx = staging.test_frame_index(40, 8, 2)              # stride 2: windows of 16 frames every 7
    assert idx[:, 0].tolist() == [0, 7, 14, 21] and idx[1].tolist() == list(range(7, 23, 2))
    assert staging.test_frame_index(5, 4, 3).tolist() == [[0, 0, 0, 3]]       # 0, 3 kept of 0, 3, 6, 9
    with pytest.raises(ValueError):
        staging.test_frame_index(10, 2, 1)                # window step 2*1//2 - 1 = 0


def _video(F=7, H=24, W=30, seed=0):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, size=(F, H, W, 3)).astype(np.uint8))


def test_stage_crops_host_logic(monkeypatch):
    CH.install(monkeypatch)
    frames = _video()
    idx = [[0, 1, 2, 3], [3, 4, 5, 6], [0, 0, 5, 6]]
    boxes = [(2, 1), (14, 8), (0, 0)]
    out = staging.stage_crops(frames, idx, boxes, [0, 1, 1], 16, 8, device="cpu")
    want = CH.reference(frames, idx, [(2, 1, 0), (14, 8, 1), (0, 0, 1)], 16, 16, 8)
    assert out.shape == (3, 3, 3, 4, 8, 8) and torch.equal(out, want)
    rect = staging.stage_crops(frames, np.asarray(idx), [(5, 3)], [0], (12, 20), 6, device="cpu")     # S % 4 != 0
    assert torch.equal(rect, CH.reference(frames, idx, [(5, 3, 0)], 12, 20, 6))
    many = staging.stage_crops(frames, idx, [(i, 0) for i in range(14)] + boxes, [0] * 17, 16, 8, device="cpu")
    assert [n for n, _ in CH.CALLS[-2:]] == [16, 1] and torch.equal(many[14:], staging.stage_crops(
        frames, idx, boxes, [0] * 3, 16, 8, device="cpu"))
    calls = len(CH.CALLS)
    for bad in ([[0, 7]], [[-1, 0]]):
        with pytest.raises(IndexError):
            staging.stage_crops(frames, bad, boxes, [0, 1, 1], 16, 8, device="cpu")
    with pytest.raises(ValueError):
        staging.stage_crops(frames, idx, [(15, 0)], [0], 16, 8, device="cpu")          # 15 + 16 > 30
    with pytest.raises(ValueError):
        staging.stage_crops(frames, idx, [(0, 9)], [0], 16, 8, device="cpu")           # 9 + 16 > 24
    with pytest.raises(ValueError):
        staging.stage_crops(frames, idx, [(0, 0)], [2], 16, 8, device="cpu")
    with pytest.raises(ValueError):
        staging.stage_crops(frames, idx, boxes, [0], 16, 8, device="cpu")
    with pytest.raises(ValueError):
        staging.stage_crops(frames.float(), idx, boxes, [0, 0, 0], 16, 8, device="cpu")
    with pytest.raises(ValueError):
        staging.stage_crops(frames, [0, 1], boxes, [0, 0, 0], 16, 8, device="cpu")
    assert len(CH.CALLS) == calls                                                      # nothing was launched


@pytest.mark.parametrize("mode,n_crops", [("center", 1), ("five", 5), ("ten", 10)])
def test_add_frames_on_the_doubles(monkeypatch, mode, n_crops):
    CH.install(monkeypatch)
    W, H, size, S, T = 30, 24, 16, 8, 4
    videos = [(_video(7, H, W, 1), staging.test_frame_index(7, T)), (_video(3, H, W, 2), staging.test_frame_index(3, T)),
              (_video(13, H, W, 3), staging.test_frame_index(13, T))]
    assert [v[1].shape[0] for v in videos] == [4, 1, 10]
    where, flips = {"center": ((5,), (0,)), "five": ((5, 1, 2, 3, 4), (0,)), "ten": ((5, 1, 2, 3, 4), (0, 1))}[mode]
    boxes = staging.five_crop_boxes(W, H, size, where) * len(flips)
    flip = [f for f in flips for _ in where]
    seen = []
    inner = VideoEvaluator.add
    monkeypatch.setattr(VideoEvaluator, "add", lambda self, clips, label=None, video=None: (
        seen.append((clips.clone(), label, video)), inner(self, clips, label=label, video=video))[1])
    per_crop = lambda n: n * 3 * T * S * S * 4
    model = CH.ToyClassifier().eval()
    ev = VideoEvaluator(model, batch_clips=8)
    ids = []
    for v, (frames, idx) in enumerate(videos):
        first = len(CH.CALLS)
        ids.append(ev.add_frames(frames, idx, label=v, crops=mode, crop_size=size, out_size=S,
                                 max_stage_bytes=3 * per_crop(idx.shape[0]) + 5))     # three whole crops at a time
        sizes = [n for n, _ in CH.CALLS[first:]]
        assert sizes == [3] * (n_crops // 3) + ([n_crops % 3] if n_crops % 3 else [])
        assert all(b <= 3 * per_crop(idx.shape[0]) + 5 for _, b in CH.CALLS[first:])
    assert ids == [0, 1, 2] and len(ev) == 3
    got = ev.finish()
    # one add() per crop, in the reference's order (centre first, the flipped five last), one video index each
    assert len(seen) == 3 * n_crops
    for v, (frames, idx) in enumerate(videos):
        want = CH.reference(frames, idx, [(x0, y0, f) for (x0, y0), f in zip(boxes, flip)], size, size, S)
        for k in range(n_crops):
            clips, label, video = seen[v * n_crops + k]
            assert torch.equal(clips, want[k]), (v, k)
            assert (label, video) == ((v, None) if k == 0 else (None, v))
    # the same scores as staging the crops and calling add() by hand
    monkeypatch.setattr(VideoEvaluator, "add", inner)
    ev2 = VideoEvaluator(CH.ToyClassifier().eval(), batch_clips=8)
    for v, (frames, idx) in enumerate(videos):
        staged = staging.stage_crops(frames, idx, boxes, flip, size, S, device="cpu")
        vid = None
        for clips in staged:
            vid = ev2.add(clips, label=v if vid is None else None, video=vid)
    want = ev2.finish()
    assert ev.passes == ev2.passes == -(-15 * n_crops // 8)
    assert torch.equal(got.probs, want.probs) and torch.equal(got.features, want.features)
    assert torch.equal(got.labels, want.labels) and got.labels.tolist() == [0, 1, 2]
    assert float(got.top1) == float(want.top1) and float(got.top5) == float(want.top5)


def test_add_frames_refusals(monkeypatch):
    CH.install(monkeypatch)
    ev = VideoEvaluator(CH.ToyClassifier().eval(), batch_clips=8)
    frames, idx = _video(), staging.test_frame_index(7, 4)
    with pytest.raises(ValueError):
        ev.add_frames(frames, idx, crops="three", crop_size=16, out_size=8)
    with pytest.raises(ValueError):
        ev.add_frames(frames, idx, crop_size=25, out_size=8)                  # FiveCrop: bigger than the frame
    with pytest.raises(IndexError):
        ev.add_frames(frames, [[0, 1, 2, 7]], crop_size=16, out_size=8)
    with pytest.raises(ValueError):
        ev.add_frames(frames, idx, crop_size=16, out_size=8, max_stage_bytes=1000)      # not even one crop
    assert len(ev) == 0 and not CH.CALLS                                      # refused before anything changed
    assert ev.add_frames(frames, idx, crops="center", crop_size=16, out_size=8) == 0
    with pytest.raises(ValueError):
        ev.add_frames(frames, idx, crops="center", crop_size=16, out_size=12)  # another clip size
    assert len(ev) == 1


def test_abi_of_stage_crops():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "coclr_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+coclr_stage_crops\s*\(", src)
    assert "coclr_stage_crops" in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 26
    lib = _lib.load()
    assert lib.coclr_abi_version() == 26
    # everything is validated on the host before anything is launched: no GPU is needed to be refused
    p = C.c_void_p(4096)
    ok = dict(frames=p, F=6, H=40, W=52, slot_frame=p, n_clips=3, T=4, crops=[0, 0, 0, 24, 12, 1], cw=28, ch=28, S=16,
              xmin=p, xk=p, xtaps=9, ymin=p, yk=p, ytaps=9, mean=[0.5, 0.5, 0.5], std=[0.2, 0.2, 0.2], out=p)

    def call(**kw):
        a = dict(ok, **kw)
        crops = None if a["crops"] is None else (C.c_int32 * len(a["crops"]))(*a["crops"])
        mean = None if a["mean"] is None else (C.c_float * 3)(*a["mean"])
        std = None if a["std"] is None else (C.c_float * 3)(*a["std"])
        n_crops = a.get("n_crops", 0 if a["crops"] is None else len(a["crops"]) // 3)
        return lib.coclr_stage_crops(a["frames"], a["F"], a["H"], a["W"], a["slot_frame"], a["n_clips"], a["T"], crops,
                                     n_crops, a["cw"], a["ch"], a["S"], a["xmin"], a["xk"], a["xtaps"], a["ymin"],
                                     a["yk"], a["ytaps"], mean, std, a["out"], None)
    for name in ("frames", "slot_frame", "xmin", "xk", "ymin", "yk", "out", "mean", "std"):
        assert call(**{name: None}) == 1, name
    assert call(crops=None, n_crops=2) == 1
    for name in ("F", "H", "W", "T", "n_clips", "S"):
        assert call(**{name: 0}) == 1 and call(**{name: -3}) == 1, name
    assert call(n_crops=0) == 1 and call(crops=[0, 0, 0] * 17) == 1
    assert call(S=513) == 1
    for name in ("xtaps", "ytaps"):
        assert call(**{name: 0}) == 1 and call(**{name: 65}) == 1, name
    assert call(crops=[-1, 0, 0]) == 1 and call(crops=[0, -1, 0]) == 1
    assert call(crops=[25, 0, 0]) == 1 and call(crops=[0, 13, 0]) == 1          # 25 + 28 > 52, 13 + 28 > 40
    assert call(crops=[0, 0, 0, 24, 12, 2]) == 1 and call(crops=[0, 0, -1]) == 1
    assert call(std=[0.2, 0.0, 0.2]) == 1
    assert call(n_clips=16384, T=4) == 1                                        # 65536 slots: over the grid limit
    assert call(S=512, ytaps=64, cw=600, ch=8000, H=8000, W=600, crops=[0, 0, 0]) == 1      # one row's taps > 64 KiB
    with pytest.raises(_lib.HipLibraryError):                                   # and the binding has no CPU path
        staging.stage_crops(_video(), [[0, 1]], [(0, 0)], [0], 16, 8, device="cpu")
