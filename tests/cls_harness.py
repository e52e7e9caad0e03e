"""An independent restatement of the classifier-clip staging (csrc/staging.hip: coclr_resize2_boxes;
coclr_amd/staging.py: ClassifierTransform, stage_classifier_clips) in numpy on the CPU -- RandomSizedCrop(size,
consistent=True) as a crop and a bicubic resize or, in its fallback, Scale(size) of the whole frame and CenterCrop;
Scale(img_dim) as a second bicubic resize; ColorJitter, the batch flip, ToTensor and Normalize -- on top of
tests/crops_harness.py, tests/jitter_harness.py and tests/train_harness.py, and a TEST DOUBLE of ops.resize2_boxes
built on it, so that the HOST logic of staging.stage_classifier_clips runs in the CPU tier.  Installed only by tests;
the product has no CPU path and never imports this file.  Nothing here shares code with coclr_amd/staging.py or the
kernel text; tests/test_cls_stage_cpu.py holds the restatement against PIL itself."""
import os
import random

import numpy as np
import torch

import crops_harness as CH
import jitter_harness as JH
import train_harness as TH
from coclr_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cls_transform.pt")
FLIP = 7
FIELDS = 14         # first, frames, x0, y0, w, h, ow, oh, cx, cy, x offset, y offset, xtaps, ytaps


def resize_wh_u8(box, ow, oh):
    """box uint8 (F, h, w, 3) -> (F, oh, ow, 3): PIL's Image.resize((ow, oh), BICUBIC), horizontal pass first, rounded
    and clamped after each pass (CH.resize_u8 with two sizes)."""
    h = CH.resample_last_axis(np.ascontiguousarray(box.transpose(0, 1, 3, 2)), ow)        # (F, h, 3, ow)
    v = CH.resample_last_axis(np.ascontiguousarray(h.transpose(0, 2, 3, 1)), oh)          # (F, 3, ow, oh)
    return np.ascontiguousarray(v.transpose(0, 3, 2, 1))                                  # (F, oh, ow, 3)


def geometry(frames, region, resample, window, size):
    """RandomSizedCrop's output: the region of every frame resampled to `resample` (left as it is when that is its own
    size: Scale and Image.resize both return their input then), of which the size x size window is kept."""
    frames = frames.cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
    x0, y0, w, h = region
    (ow, oh), (cx, cy) = resample, window
    box = frames[:, y0:y0 + h, x0:x0 + w]
    if (ow, oh) == (size, size) and (cx, cy) == (0, 0):
        return CH.crop_resized_u8(frames, [(x0, y0, 0)], w, h, size)[0]
    full = box if (ow, oh) == (w, h) else resize_wh_u8(box, ow, oh)
    return np.ascontiguousarray(full[:, cy:cy + size, cx:cx + size])


def scaled(sq, S):
    """Scale(S) of square images uint8 (F, size, size, 3): untouched when S == size."""
    return sq if sq.shape[1] == S else CH.resize_u8(sq, S)


def resized_u8(frames, region, resample, window, size, S):
    return scaled(geometry(frames, region, resample, window, size), S)


def chain_u8(frames, plan, size, S, flip=False):
    """One sample: frames uint8 (T, H, W, 3) and a plan of ClassifierTransform.draw -> uint8 (T, S, S, 3)."""
    u8 = resized_u8(frames, plan["region"], plan["resample"], plan["window"], size, S)
    prog = list(plan["program"]) + ([(FLIP, 0)] if flip else [])
    return np.stack([TH.apply_program(f, prog) for f in u8])


def chain_reference(frames, plans, size, S, flip=False, mean=CH.IMAGENET_MEAN, std=CH.IMAGENET_STD):
    """frames (B, T, H, W, 3) -> fp32 (B, 3, T, S, S)."""
    T = frames.shape[1]
    return torch.cat([JH.to_clips(chain_u8(f, p, size, S, flip), T, mean, std) for f, p in zip(frames, plans)])


def window_layout(n_in, n_out, c0, size):
    """Columns c0 .. c0 + size - 1 of the n_in -> n_out tables as the kernel takes them: (P,), (taps, P), P = size
    rounded up to a multiple of 4."""
    lo, K = CH.tables(n_in, n_out)
    P = (size + 3) & ~3
    lo_p = np.zeros(P, dtype=np.int32)
    lo_p[:size] = lo[c0:c0 + size]
    K_p = np.zeros((K.shape[1], P), dtype=np.int32)
    K_p[:, :size] = K[c0:c0 + size].T
    return torch.from_numpy(lo_p), torch.from_numpy(K_p)


def descriptors(clips, T, size, S):
    """[(first, (x0, y0, w, h), (ow, oh), (cx, cy))] -> (desc int32 (n, 14), xtab, ytab, tab2 (1 + taps, Sp)) from the
    harness's own tables, every clip with tables of its own."""
    desc = torch.zeros(len(clips), FIELDS, dtype=torch.int32)
    bufs, fill = ([], []), [0, 0]
    for k, (first, (x0, y0, w, h), (ow, oh), (cx, cy)) in enumerate(clips):
        desc[k, :10] = torch.tensor([first, T, x0, y0, w, h, ow, oh, cx, cy], dtype=torch.int32)
        for axis, (n_in, n_out, c0) in enumerate(((w, ow, cx), (h, oh, cy))):
            lo, K = window_layout(n_in, n_out, c0, size)
            t = torch.cat([lo[None], K]).reshape(-1)
            desc[k, 10 + axis], desc[k, 12 + axis] = fill[axis], K.shape[0]
            bufs[axis].append(t)
            fill[axis] += t.numel()
    lo2, K2 = CH.kernel_layout(size, S)
    return desc, torch.cat(bufs[0]), torch.cat(bufs[1]), torch.cat([lo2[None], K2]).contiguous()


# ---- test doubles ------------------------------------------------------------------------------------------------

CALLS = []      # ("resize2", n_clips, T, "u8" | "f32") of every call of the double


def resize2_boxes(frames, desc, desc_host, xtab, ytab, tab2, T, size, S, out, mean=None, std=None):
    """Double of ops.resize2_boxes: the tables at every descriptor's offsets must be the harness's own."""
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3
    assert desc.dtype == torch.int32 and desc_host.dtype == torch.int32 and torch.equal(desc.cpu(), desc_host)
    assert tuple(desc_host.shape[1:]) == (FIELDS,)
    assert xtab.dtype == torch.int32 and ytab.dtype == torch.int32 and xtab.dim() == 1 and ytab.dim() == 1
    n_clips = desc_host.shape[0]
    F, H, W = frames.shape[:3]
    P, Sp = (size + 3) & ~3, (S + 3) & ~3
    lo2, K2 = CH.kernel_layout(size, S)
    assert tab2.dtype == torch.int32 and torch.equal(tab2.cpu(), torch.cat([lo2[None], K2]))
    src = frames.cpu().numpy()
    u8 = []
    for first, n, x0, y0, w, h, ow, oh, cx, cy, xo, yo, xt, yt in desc_host.tolist():
        assert n == T and 0 <= first and first + T <= F and 0 <= x0 and 0 <= y0 and x0 + w <= W and y0 + h <= H
        assert 0 <= cx and 0 <= cy and cx + size <= ow and cy + size <= oh
        for tab, off, taps, (n_in, n_out, c0) in ((xtab, xo, xt, (w, ow, cx)), (ytab, yo, yt, (h, oh, cy))):
            lo, K = window_layout(n_in, n_out, c0, size)
            assert off % 4 == 0 and taps == K.shape[0] and off + P * (1 + taps) <= tab.numel()
            assert torch.equal(tab[off:off + P].cpu(), lo)
            assert torch.equal(tab[off + P:off + P * (1 + taps)].cpu().view(taps, P), K)
        u8.append(resized_u8(src[first:first + T], (x0, y0, w, h), (ow, oh), (cx, cy), size, S))
    u8 = np.concatenate(u8)
    if out.dtype == torch.uint8:
        assert tuple(out.shape) == (n_clips * T, S, S, 3) and mean is None and std is None
        CALLS.append(("resize2", n_clips, T, "u8"))
        out.copy_(torch.from_numpy(u8))
    else:
        assert out.dtype == torch.float32 and tuple(out.shape) == (n_clips, 3, T, S, S)
        CALLS.append(("resize2", n_clips, T, "f32"))
        out.copy_(JH.to_clips(u8, T, mean, std))


def install(monkeypatch):
    TH.install(monkeypatch)
    monkeypatch.setattr(ops, "resize2_boxes", resize2_boxes)
    del CALLS[:]


def golden():
    """tests/golden/cls_transform.pt (tools/make_cls_transform_golden.py): what the reference's own classifier
    transform made of 3 small frames under fixed seeds, as bytes, with its use of the generator."""
    return torch.load(GOLDEN)


def fixture_plans(gold):
    """Per recorded run (run, plan, random.random() right after the draw): the plan staging.ClassifierTransform.draw
    yields with the generator seeded as the run was."""
    from coclr_amd import staging
    out = []
    for run in gold["runs"]:
        ct = staging.ClassifierTransform(run["img_dim"], gold["seq_len"], size=gold["size"], mode=run["mode"])
        random.seed(run["seed"])
        H, W = run["frames"].shape[1:3]
        plan = ct.draw(W, H)
        out.append((run, plan, random.random()))
    return out


def frames(n, H, W, seed):
    return TH.frames(n, H, W, seed)
