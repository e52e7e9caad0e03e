"""An independent restatement of the training-clip staging (csrc/staging.hip: coclr_resize_boxes_u8,
coclr_augment_clips; coclr_amd/staging.py: stage_train_clips) in numpy on the CPU -- PIL's 8-bit
`ImageFilter.GaussianBlur` (three extended box blurs per direction, rounded to bytes after each), the flip, and the
whole chain crop -> bicubic resize -> ColorJitter -> RandomGray -> blur -> flip -> ToTensor -> Normalize on top of
tests/crops_harness.py and tests/jitter_harness.py -- and TEST DOUBLES of ops.resize_boxes_u8 and ops.augment_clips
built on it, so that the HOST logic of staging.stage_train_clips runs in the CPU tier.  Installed only by tests; the
product has no CPU path and never imports this file.  Nothing here shares code with coclr_amd/staging.py or the
kernel text; tests/test_train_stage_cpu.py holds the blur against PIL itself."""
import os

import numpy as np
import torch

import crops_harness as CH
import jitter_harness as JH
from coclr_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_transform.pt")
BLUR, FLIP = 6, 7
f32 = np.float32


def box_radius(sigma):
    """PIL's _gaussian_blur_radius(sigma, passes=3) as its C computes it: sigma and every variable a `float`, the
    square root and the floor taken in double.  (Evaluated in doubles throughout and rounded at the end, the
    radius differs in the last bit for many sigmas and the blurred bytes for a few, 1.4 among them:
    tests/test_train_stage_cpu.py.)"""
    radius = np.asarray(sigma, dtype=f32)
    sigma2 = radius * radius / f32(3)
    L = np.sqrt(np.float64(12.0) * sigma2.astype(np.float64) + 1.0).astype(f32)
    l = np.floor((L.astype(np.float64) - 1.0) / 2.0).astype(f32)
    l1 = l + f32(1)
    num = (f32(2) * l + f32(1)) * (l * l1 - f32(3) * sigma2)
    den = f32(6) * (sigma2 - l1 * l1)
    out = l + num / den
    assert out.dtype == f32
    return f32(out)


def box_weights(rf):
    """(r, ww, fw) of PIL's ImagingLineBoxBlur for the fp32 radius rf: the division is a float32 one."""
    rf = f32(rf)
    r = int(rf)
    ww = int(np.uint32(f32(16777216.0) / (rf * f32(2.0) + f32(1.0))))
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return r, ww, fw


def box_line(x, rf):
    """One line pass along the LAST axis of uint8 x: edge pixels replicated, (acc + 2^23) >> 24."""
    r, ww, fw = box_weights(rf)
    n = x.shape[-1]
    i = np.arange(n)
    X = x.astype(np.int64)
    near = sum(X[..., np.clip(i + d, 0, n - 1)] for d in range(-r, r + 1))
    far = X[..., np.clip(i - r - 1, 0, n - 1)] + X[..., np.clip(i + r + 1, 0, n - 1)]
    acc = ww * near + fw * far + (1 << 23)
    assert int(acc.max()) < (1 << 32)
    return (acc >> 24).astype(np.uint8)


def blur_u8(img, rf):
    """uint8 (H, W, C) -> uint8 (H, W, C): three line passes along x, then three along y."""
    a = np.ascontiguousarray(np.asarray(img).transpose(0, 2, 1))          # (H, C, W)
    for _ in range(3):
        a = box_line(a, rf)
    a = np.ascontiguousarray(a.transpose(1, 2, 0))                        # (C, W, H)
    for _ in range(3):
        a = box_line(a, rf)
    return np.ascontiguousarray(a.transpose(2, 1, 0))


def apply_op(rgb, kind, param):
    kind = int(kind)
    if kind == BLUR:
        return blur_u8(rgb, param)
    if kind == FLIP:
        return np.ascontiguousarray(np.asarray(rgb)[:, ::-1])
    return JH.apply_op(rgb, kind, param)


def apply_program(rgb, program):
    for kind, param in program:
        rgb = apply_op(rgb, kind, param)
    return np.ascontiguousarray(rgb)


def augment_u8(frames, programs, group_size):
    frames = frames.cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
    return np.stack([apply_program(f, programs[n // group_size]) for n, f in enumerate(frames)])


def reference(frames, programs, group_size, T, mean=CH.IMAGENET_MEAN, std=CH.IMAGENET_STD):
    """uint8 (N, H, W, 3) -> fp32 (N/T, 3, T, H, W), frame n running programs[n // group_size]."""
    return JH.to_clips(augment_u8(frames, programs, group_size), T, mean, std)


def chain_u8(frames, plan, S):
    """One sample: frames uint8 (2T, H, W, 3) and a plan of TrainTransform.draw -> uint8 (2T, S, S, 3), clip 0
    then clip 1: crop the box, resize, run each frame's program."""
    frames = frames.cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
    T = frames.shape[0] // 2
    out = []
    for c in range(2):
        x0, y0, w, h = plan["box"][c]
        src = frames[plan["half"][c] * T:(plan["half"][c] + 1) * T]
        resized = CH.crop_resized_u8(src, [(x0, y0, 0)], w, h, S)[0]
        out.append(np.stack([apply_program(f, prog) for f, prog in zip(resized, plan["programs"][c])]))
    return np.concatenate(out)


def chain_reference(frames, plans, S, mean=CH.IMAGENET_MEAN, std=CH.IMAGENET_STD):
    """frames (B, 2T, H, W, 3) -> fp32 (B, 2, 3, T, S, S)."""
    T = frames.shape[1] // 2
    return torch.stack([JH.to_clips(chain_u8(f, p, S), T, mean, std) for f, p in zip(frames, plans)])


# ---- test doubles ------------------------------------------------------------------------------------------------

CALLS = []      # ("boxes", n_clips, T) / ("augment", N, group_size, programs) of every call of the doubles


def resize_boxes_u8(frames, desc, desc_host, xtab, ytab, T, S, out):
    """Double of ops.resize_boxes_u8: the tables at every box's offsets must be the harness's own."""
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3
    assert desc.dtype == torch.int32 and desc_host.dtype == torch.int32 and torch.equal(desc.cpu(), desc_host)
    assert xtab.dtype == torch.int32 and ytab.dtype == torch.int32 and xtab.dim() == 1 and ytab.dim() == 1
    n_clips = desc_host.shape[0]
    assert out.dtype == torch.uint8 and tuple(out.shape) == (n_clips * T, S, S, 3)
    F, H, W = frames.shape[:3]
    Sp = (S + 3) & ~3
    CALLS.append(("boxes", n_clips, T))
    src = frames.cpu().numpy()
    for k, (first, n, x0, y0, w, h, xo, yo, xt, yt) in enumerate(desc_host.tolist()):
        assert n == T and 0 <= first and first + T <= F and 0 <= x0 and 0 <= y0 and x0 + w <= W and y0 + h <= H
        for tab, off, taps, n_in in ((xtab, xo, xt, w), (ytab, yo, yt, h)):
            lo, K = CH.kernel_layout(n_in, S)
            assert off % 4 == 0 and taps == K.shape[0] and off + Sp * (1 + taps) <= tab.numel()
            assert torch.equal(tab[off:off + Sp].cpu(), lo)
            assert torch.equal(tab[off + Sp:off + Sp * (1 + taps)].cpu().view(taps, Sp), K)
        out[k * T:(k + 1) * T].copy_(torch.from_numpy(
            CH.crop_resized_u8(src[first:first + T], [(x0, y0, 0)], w, h, S)[0]))


def augment_clips(frames, kinds, params, group_size, T, mean, std, out, host_tables=None):
    """Double of ops.augment_clips."""
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3
    assert kinds.dtype == torch.int32 and params.dtype == torch.float32 and kinds.shape == params.shape
    N = frames.shape[0]
    assert N % T == 0 and kinds.shape[0] * group_size >= N and kinds.shape[1] <= 8
    assert host_tables is None or (torch.equal(host_tables[0], kinds.cpu()) and torch.equal(host_tables[1], params.cpu()))
    progs = JH.table_programs(kinds, params)
    CALLS.append(("augment", N, int(group_size), progs))
    out.copy_(reference(frames, progs, group_size, T, mean, std))


def install(monkeypatch):
    JH.install(monkeypatch)
    monkeypatch.setattr(ops, "resize_boxes_u8", resize_boxes_u8)
    monkeypatch.setattr(ops, "augment_clips", augment_clips)
    del CALLS[:]


def golden():
    """tests/golden/train_transform.pt (tools/make_train_transform_golden.py): what the reference's own training
    transform made of 2 x 3 small frames under fixed seeds, as bytes, with its use of both generators."""
    return torch.load(GOLDEN)


def fixture_plans(gold):
    """Per recorded run (run, plan, (random.random(), np.random.random()) right after the draw): the plan
    staging.TrainTransform.draw yields with both generators seeded as the run was."""
    import random
    from coclr_amd import staging
    tt = staging.TrainTransform(gold["img_dim"], gold["seq_len"])
    out = []
    for run in gold["runs"]:
        random.seed(run["seed"])
        np.random.seed(run["seed"])
        H, W = run["frames"].shape[1:3]
        plan = tt.draw(W, H)
        out.append((run, plan, (random.random(), float(np.random.random()))))
    return out


def levels_expected(u8, levels, T):
    """One sample's uint8 (2T, S, S, 3) -> fp32 (2, 3, T, S, S) through the fixture's byte table."""
    return JH.levels_expected(u8, levels, T)


def frames(n, H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n, H, W, 3)).astype(np.uint8)
