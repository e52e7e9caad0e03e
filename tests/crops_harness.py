"""An independent restatement of the five/ten-crop staging (csrc/staging.hip: coclr_stage_crops) in numpy integer
arithmetic on the CPU -- flip, crop, PIL's 8-bit bicubic `Image.resize`, ToTensor, Normalize -- and a TEST DOUBLE
of ops.stage_crops built on it, so that the HOST logic of staging.stage_crops and VideoEvaluator.add_frames runs
in the CPU tier.  Installed only by tests, on top of tests/video_harness.py; the product has no CPU path and
never imports this file.  Nothing here shares code with coclr_amd/staging.py: the tables are computed
vectorised in float64, and tests/test_crops_cpu.py holds both against PIL itself."""
import os

import numpy as np
import torch

import video_harness
from coclr_amd import ops
from coclr_amd.staging import IMAGENET_MEAN, IMAGENET_STD

ToyClassifier = video_harness.ToyClassifier
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage_crops.pt")


def tables(n_in, n_out):
    """(xmin int32 (n_out,), K int32 (n_out, taps)): PIL's precompute_coeffs + normalize_coeffs_8bpc, BICUBIC."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support, ss = 2.0 * fs, 1.0 / fs
    taps = int(np.ceil(support)) * 2 + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    lo = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    hi = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n_in)
    i = np.arange(taps, dtype=np.int64)[None, :]
    x = np.abs((i + lo[:, None] - center[:, None] + 0.5) * ss)
    a = -0.5
    w = np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0,
                 np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))
    w = np.where(i < (hi - lo)[:, None], w, 0.0)
    ww = np.zeros(n_out, dtype=np.float64)
    for t in range(taps):                       # left to right, as PIL sums (np.sum adds pairwise)
        ww = ww + w[:, t]
    k = w / np.where(ww != 0.0, ww, 1.0)[:, None]
    K = np.trunc(np.where(k >= 0, k * 4194304.0 + 0.5, k * 4194304.0 - 0.5)).astype(np.int32)
    return lo.astype(np.int32), K


def resample_last_axis(src, n_out):
    """src uint8 (..., n_in) -> uint8 (..., n_out): one pass of PIL's resize along the last axis."""
    n_in = src.shape[-1]
    lo, K = tables(n_in, n_out)
    acc = np.full(src.shape[:-1] + (n_out,), 1 << 21, dtype=np.int64)
    for t in range(K.shape[1]):
        col = np.minimum(lo.astype(np.int64) + t, n_in - 1)         # padded taps have K = 0
        acc += K[:, t].astype(np.int64) * src[..., col].astype(np.int64)
    return np.clip(acc >> 22, 0, 255).astype(np.uint8)


def resize_u8(box, S):
    """box uint8 (F, ch, cw, 3) -> (F, S, S, 3): horizontal pass first, rounded and clamped after each pass."""
    h = resample_last_axis(np.ascontiguousarray(box.transpose(0, 1, 3, 2)), S)        # (F, ch, 3, S)
    v = resample_last_axis(np.ascontiguousarray(h.transpose(0, 2, 3, 1)), S)          # (F, 3, S(x), S(y))
    return np.ascontiguousarray(v.transpose(0, 3, 2, 1))                              # (F, S(y), S(x), 3)


def normalise(u8, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """uint8 (..., 3) -> fp32: ToTensor's /255, then Normalize, in torch fp32 (channel last here)."""
    x = torch.from_numpy(np.ascontiguousarray(u8)).to(torch.float32) / 255
    m = torch.tensor(list(mean), dtype=torch.float32)
    s = torch.tensor(list(std), dtype=torch.float32)
    return (x - m) / s


def crop_resized_u8(frames, crops, cw, ch, S, flip_after_crop=False):
    """[(F, S, S, 3) uint8 per crop]: flip the whole frame, THEN crop (`flip_after_crop` is the wrong order a
    test must be able to tell apart)."""
    frames = np.asarray(frames)
    out = []
    for x0, y0, flip in crops:
        src = frames[:, :, ::-1] if flip and not flip_after_crop else frames
        box = src[:, y0:y0 + ch, x0:x0 + cw]
        if flip and flip_after_crop:
            box = box[:, :, ::-1]
        out.append(resize_u8(box, S))
    return out


def gather_clips(per_frame, slot_frame):
    """(F, S, S, 3) fp32 per frame -> (n_clips, 3, T, S, S) for slot_frame (n_clips, T)."""
    idx = torch.as_tensor(np.asarray(slot_frame)).long()
    return per_frame[idx].permute(0, 4, 1, 2, 3).contiguous()


def reference(frames, slot_frame, crops, cw, ch, S, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """frames uint8 (F, H, W, 3), slot_frame (n_clips, T), crops [(x0, y0, flip)] -> (n_crops, n_clips, 3, T, S, S)."""
    if torch.is_tensor(frames):
        frames = frames.cpu().numpy()
    return torch.stack([gather_clips(normalise(u8, mean, std), slot_frame)
                        for u8 in crop_resized_u8(frames, crops, cw, ch, S)])


def kernel_layout(n_in, S):
    """The tables as the kernel takes them: (Sp,), (taps, Sp), Sp = S rounded up to a multiple of 4."""
    lo, K = tables(n_in, S)
    Sp = (S + 3) & ~3
    lo_p = np.zeros(Sp, dtype=np.int32)
    lo_p[:S] = lo
    K_p = np.zeros((K.shape[1], Sp), dtype=np.int32)
    K_p[:, :S] = K.T
    return torch.from_numpy(lo_p), torch.from_numpy(K_p)


CALLS = []      # (n_crops, bytes written) of every call of the double


def stage_crops(frames, slot_frame, crops, cw, ch, S, xmin, xk, ymin, yk, mean, std, out):
    """Double of ops.stage_crops: the tables handed over must be the harness's own, in the kernel's layout."""
    for got, want in zip((xmin, xk), kernel_layout(cw, S)):
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)
    for got, want in zip((ymin, yk), kernel_layout(ch, S)):
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)
    assert frames.dtype == torch.uint8 and slot_frame.dtype == torch.int32 and 1 <= len(crops) <= 16
    assert int(slot_frame.min()) >= 0 and int(slot_frame.max()) < frames.shape[0]
    CALLS.append((len(crops), out.numel() * 4))
    out.copy_(reference(frames, slot_frame.cpu(), [tuple(int(v) for v in c) for c in crops], cw, ch, S, mean, std))


def install(monkeypatch):
    video_harness.install(monkeypatch)
    monkeypatch.setattr(ops, "stage_crops", stage_crops)
    del CALLS[:]


def golden():
    """tests/golden/stage_crops.pt (tools/make_stage_crops_golden.py): per case the inputs and PIL's resized
    bytes per crop and frame, plus `levels` (3, 256): ((v / 255) - mean[c]) / std[c] in torch fp32 for every byte
    v.  The expected fp32 output is levels[c][byte], gathered per clip."""
    return torch.load(GOLDEN)


def golden_expected(case, levels):
    """(n_crops, n_clips, 3, T, S, S) fp32 of a fixture case."""
    res = case["resized"].long()                                       # (n_crops, F, S, S, 3)
    per = torch.stack([levels[c][res[..., c]] for c in range(3)], -1)  # fp32, channel last
    return torch.stack([gather_clips(p, case["frame_index"]) for p in per])


def case_crops(case):
    return [(int(x0), int(y0), int(f)) for (x0, y0), f in zip(case["boxes"].tolist(), case["flips"].tolist())]
