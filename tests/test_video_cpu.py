"""CPU tier of the video-level evaluator (coclr_amd/eval/video.py) on the doubles of tests/video_harness.py:
batching and segment bookkeeping against a plain per-video loop (eval/main_classifier.py:482-494,533,624-640),
and the C ABI of the two segmented-accumulate entry points."""
import ctypes as C
import os
import re

import pytest
import torch

import video_harness as VH
from coclr_amd import _lib, ops
from coclr_amd.eval.video import VideoEvaluator, extract_features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _doubles(monkeypatch):
    VH.install(monkeypatch)


def _videos(lengths, crops, seed=0, clip=(3, 4, 6, 6)):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(n, *clip, generator=g) for _ in range(crops)] for n in lengths]


def _per_video_loop(model, videos):
    """The reference's loops: one model call per video and crop."""
    probs, feats = [], []
    with torch.no_grad():
        for crops in videos:
            outs = [model(c.double()) for c in crops]
            probs.append(torch.stack([torch.softmax(l, -1).mean(0) for l, _ in outs], 0).mean(0))
            feats.append(torch.stack([f.mean(0) for _, f in outs], 0).mean(0))
    return torch.stack(probs), torch.stack(feats)


@pytest.mark.parametrize("crops", [1, 2])
def test_batching_matches_the_per_video_loop(monkeypatch, crops):
    lengths = [1, 3, 11, 2, 5, 8, 1, 9, 19, 4]        # 11, 9 and 19 exceed batch_clips; several span two batches
    videos = _videos(lengths, crops)
    labels = [i % 11 for i in range(len(lengths))]
    model = VH.ToyClassifier().eval()
    seen = []
    inner = ops.segment_accum
    monkeypatch.setattr(ops, "segment_accum", lambda x, segs, w, out: (seen.append((list(segs), list(w))),
                                                                     inner(x, segs, w, out))[1])
    ev = VideoEvaluator(model, batch_clips=8)
    ids = [ev.add(v[0], label=l) for v, l in zip(videos, labels)]      # first crop of every video ...
    assert ids == list(range(len(lengths))) and len(ev) == len(lengths)
    for c in range(1, crops):                                          # ... then the further ones (`video=`)
        for i, v in enumerate(videos):
            assert ev.add(v[c], video=i) == i
    total = sum(lengths) * crops
    assert ev.passes == total // 8                                     # full batches ran as they filled up
    res = ev.finish()
    assert ev.passes == -(-total // 8) and len(ev) == 0
    assert all(s == (8, 3, 4, 6, 6) for s in model.shapes)             # ONE shape, the tail batch included
    # every clip row belongs to exactly one segment, pad rows of the tail to none
    rows = 0
    for b, (segs, w) in enumerate(seen):
        used = sorted(r for first, n, _ in segs for r in range(first, first + n))
        fill = 8 if b < len(seen) - 1 or total % 8 == 0 else total % 8
        assert used == list(range(fill))
        rows += len(used)
    assert rows == total
    # weights: 1/n of the crop the rows came from; a video that spans batches contributes several segments
    per_video = {}
    for segs, w in seen:
        for (first, n, v), wi in zip(segs, w):
            assert wi == 1.0 / lengths[v]
            per_video[v] = per_video.get(v, 0) + n
    assert per_video == {i: n * crops for i, n in enumerate(lengths)}
    assert sum(len(s) for s, _ in seen) > len(lengths) * crops         # some crop was cut by a batch boundary
    want_p, want_f = _per_video_loop(model.double(), videos)
    assert res.probs.shape == (len(lengths), 11) and res.features.shape == (len(lengths), 16)
    assert float((res.probs.double() - want_p).abs().max()) < 1e-6
    assert float((res.features.double() - want_f).abs().max()) < 1e-6
    assert res.labels.tolist() == labels
    pred = want_p.topk(5, 1).indices
    tgt = torch.tensor(labels)
    assert float(res.top1) == pytest.approx(float((pred[:, 0] == tgt).float().mean()))
    assert float(res.top5) == pytest.approx(float((pred == tgt[:, None]).any(1).float().mean()))


def test_extract_features_and_unlabelled_videos():
    videos = _videos([2, 7, 1], 1, seed=3)
    model = VH.ToyClassifier().eval()
    feats, labels = extract_features(model, [(v[0], i) for i, v in enumerate(videos)], batch_clips=4)
    _, want = _per_video_loop(model.double(), videos)
    assert labels.tolist() == [0, 1, 2] and float((feats.double() - want).abs().max()) < 1e-6
    feats, labels = extract_features(model.float(), [v[0] for v in videos], batch_clips=4)
    assert labels is None and feats.shape == (3, 16)


def test_argument_errors():
    model = VH.ToyClassifier().eval()
    with pytest.raises(ValueError):
        VideoEvaluator(model, batch_clips=0)
    ev = VideoEvaluator(model, batch_clips=4)
    with pytest.raises(ValueError):
        ev.finish()                                         # nothing added
    with pytest.raises(ValueError):
        ev.add(torch.zeros(3, 4, 6, 6))                     # not (n, 3, T, H, W)
    with pytest.raises(ValueError):
        ev.add(torch.zeros(0, 3, 4, 6, 6))                  # no clip
    with pytest.raises(IndexError):
        ev.add(torch.zeros(1, 3, 4, 6, 6), video=0)         # no such video yet
    v = ev.add(torch.zeros(1, 3, 4, 6, 6), label=2)
    with pytest.raises(ValueError):
        ev.add(torch.zeros(1, 3, 4, 8, 8))                  # another clip size
    with pytest.raises(ValueError):
        ev.add(torch.zeros(1, 3, 4, 6, 6), label=3, video=v)
    with pytest.raises(_lib.HipLibraryError):
        ops.segment_accum(torch.zeros(4, 5), [(3, 2, 0)], [1.0], torch.zeros(1, 5))
    model.train()
    with pytest.raises(RuntimeError):
        ev.finish()                                         # the model has to be in eval() mode


def test_abi_declares_the_segment_entries():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "coclr_hip.h")).read(), flags=re.S)
    for name in ("coclr_segment_softmax_accum", "coclr_segment_accum"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 26
    assert re.search(r"return\s+26\s*;", open(os.path.join(ROOT, "coclr_amd", "csrc", "version.hip")).read())
    lib = _lib.load()
    assert lib.coclr_abi_version() == 26
    # the segments are validated on the host, before anything is launched: no GPU is needed to be refused
    x = C.c_void_p(4096)
    w = (C.c_float * 2)(1.0, 1.0)

    def call(fn, segs, R=8, C_=101, V=4):
        arr = (C.c_int32 * len(segs))(*segs)
        return fn(x, arr, w, x, R, C_, len(segs) // 3, V, None)
    for fn in (lib.coclr_segment_softmax_accum, lib.coclr_segment_accum):
        assert call(fn, [0, 0, 0]) == 1                      # empty segment
        assert call(fn, [0, 4, 0, 6, 3, 1]) == 1             # rows 6..8 of 8
        assert call(fn, [-1, 2, 0]) == 1
        assert call(fn, [0, 2, 4]) == 1                      # out row 4 of 4
        assert call(fn, [0, 2, 0], C_=0) == 1
        assert call(fn, [0, 2, 0], C_=ops.SEGMENT_MAX_C + 1) == 1
        assert fn(x, None, w, x, 8, 101, 0, 4, None) == 1
    with pytest.raises(ValueError):
        ops._segment_call("segment_accum", torch.zeros(2, ops.SEGMENT_MAX_C + 4), [(0, 1, 0)], [1.0],
                          torch.zeros(1, ops.SEGMENT_MAX_C + 4))      # the binding states the bound too
