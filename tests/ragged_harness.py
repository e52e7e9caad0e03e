"""The ragged staging on the CPU (csrc/staging.hip: coclr_resize_boxes_ragged_u8, coclr_resize2_boxes_ragged;
coclr_amd/staging.py: stage_train_clips_ragged, stage_classifier_clips_ragged): TEST DOUBLES of the two ragged resize
wrappers that cut each clip's frames out of the flat byte buffer, as its descriptor names them, and hand them to the
per-size restatements of tests/train_harness.py and tests/cls_harness.py, so that the HOST logic of the ragged staging
runs in the CPU tier.  Installed only by tests; the product has no CPU path and never imports this file.  Also the two
mixed batches the CPU and the GPU tier share."""
import random

import numpy as np
import torch

import cls_harness as CL
import train_harness as TH
from coclr_amd import ops

ALIGN = 16
CALLS = []      # ("boxes", n_clips, T) / ("resize2", n_clips, T, "u8" | "f32") of every call of the doubles


def clip_frames(pixels, rag, T):
    """The T frames a ragged descriptor's trailing words (offset low, offset high, W, H) name: (T, H, W, 3)."""
    lo, hi, W, H = rag
    off = (hi << 32) | (lo & 0xffffffff)
    n = 3 * H * W
    step = (n + ALIGN - 1) // ALIGN * ALIGN
    assert off % ALIGN == 0 and W >= 1 and H >= 1 and 0 <= off and off + step * (T - 1) + n <= pixels.numel()
    return torch.stack([pixels[off + t * step:off + t * step + n].view(H, W, 3) for t in range(T)]).cpu()


def _common(pixels, desc, desc_host, fields):
    assert pixels.dtype == torch.uint8 and pixels.dim() == 1
    assert desc.dtype == torch.int32 and desc_host.dtype == torch.int32 and torch.equal(desc.cpu(), desc_host)
    assert tuple(desc_host.shape[1:]) == (fields,)


def resize_boxes_ragged_u8(pixels, desc, desc_host, xtab, ytab, T, S, out):
    """Double of ops.resize_boxes_ragged_u8: clip by clip through the double of ops.resize_boxes_u8, which holds the
    box against the clip's OWN frame and the tables against the harness's."""
    _common(pixels, desc, desc_host, 14)
    n_clips = desc_host.shape[0]
    assert out.dtype == torch.uint8 and tuple(out.shape) == (n_clips * T, S, S, 3)
    CALLS.append(("boxes", n_clips, T))
    for k, row in enumerate(desc_host.tolist()):
        one = torch.tensor([[0] + row[1:10]], dtype=torch.int32)
        TH.resize_boxes_u8(clip_frames(pixels, row[10:], T), one, one, xtab, ytab, T, S, out[k * T:(k + 1) * T])
        TH.CALLS.pop()


def resize2_boxes_ragged(pixels, desc, desc_host, xtab, ytab, tab2, T, size, S, out, mean=None, std=None):
    """Double of ops.resize2_boxes_ragged: clip by clip through the double of ops.resize2_boxes."""
    _common(pixels, desc, desc_host, 18)
    n_clips = desc_host.shape[0]
    u8 = out.dtype == torch.uint8
    assert tuple(out.shape) == ((n_clips * T, S, S, 3) if u8 else (n_clips, 3, T, S, S))
    CALLS.append(("resize2", n_clips, T, "u8" if u8 else "f32"))
    for k, row in enumerate(desc_host.tolist()):
        one = torch.tensor([[0] + row[1:14]], dtype=torch.int32)
        dst = out[k * T:(k + 1) * T] if u8 else out[k:k + 1]
        CL.resize2_boxes(clip_frames(pixels, row[14:], T), one, one, xtab, ytab, tab2, T, size, S, dst, mean, std)
        CL.CALLS.pop()


def install(monkeypatch):
    CL.install(monkeypatch)
    monkeypatch.setattr(ops, "resize_boxes_ragged_u8", resize_boxes_ragged_u8)
    monkeypatch.setattr(ops, "resize2_boxes_ragged", resize2_boxes_ragged)
    del CALLS[:]


# ---- the mixed batches ---------------------------------------------------------------------------------------------

def cls_batches():
    """tests/golden/cls_transform.pt as one ragged batch per img_dim, in golden order: {img_dim: [(run, plan)]}.  Three
    frame sizes: 40 x 52, 8 x 96, 24 x 192."""
    out = {}
    for run, plan, _ in CL.fixture_plans(CL.golden()):
        out.setdefault(run["img_dim"], []).append((run, plan))
    return out


EDGE = (57, 41)      # H, W of the sample whose box touches its own right and bottom edge; a larger frame follows it


def train_batch():
    """The runs of tests/golden/train_transform.pt (40 x 52) followed by seeded samples of 8 x 96, 57 x 41 and 24 x 192
    (H x W) whose plans come from TrainTransform.draw: [(frames uint8 (2T, H, W, 3), plan)], and (img_dim, T).  The
    57 x 41 sample's first box is moved to the right and bottom edge of its own frame; its 7011-byte frames are not a
    multiple of 16, so the container pads between them."""
    from coclr_amd import staging
    gold = TH.golden()
    S, T = gold["img_dim"], gold["seq_len"]
    batch = [(run["frames"], plan) for run, plan, _ in TH.fixture_plans(gold)]
    tt = staging.TrainTransform(S, T)
    for seed, (H, W) in ((11, (8, 96)), (12, EDGE), (13, (24, 192))):
        rng, np_rng = random.Random(seed), np.random.RandomState(seed)
        plan = tt.draw(W, H, rng=rng, np_rng=np_rng)
        if (H, W) == EDGE:
            (x0, y0, w, h), other = plan["box"]
            plan["box"] = ((W - w, H - h, w, h), other)
        batch.append((torch.from_numpy(TH.frames(2 * T, H, W, seed)), plan))
    return batch, S, T
