"""An independent restatement of the colour-jitter kernel (csrc/staging.hip: coclr_color_jitter_clips) in numpy
on the CPU -- PIL's 8-bit `ImageEnhance.Brightness/Contrast/Color`, `convert('L')`, `convert('HSV')` and back, the
reference's `RandomGray.grayscale`, then ToTensor and Normalize -- and TEST DOUBLES of ops.resize_crops_u8 and
ops.color_jitter_clips built on it, so that the HOST logic of staging.stage_crops(jitter=) and
VideoEvaluator.add_frames(jitter=) runs in the CPU tier.  Installed only by tests, on top of
tests/crops_harness.py; the product has no CPU path and never imports this file.  Nothing here shares code with
coclr_amd/staging.py or the kernel text; tests/test_jitter_cpu.py holds every function against PIL itself.

Every float32 step below is a numpy float32 operation of its own (numpy never contracts), every other step is
float64 or integer."""
import os

import numpy as np
import torch

import crops_harness as CH
from coclr_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_jitter.pt")
NOP, BRIGHTNESS, CONTRAST, SATURATION, HUE, GRAY = range(6)
f32, f64 = np.float32, np.float64


def lum(rgb):
    """uint8 (..., 3) -> int64 (...): PIL's convert('L')."""
    c = np.asarray(rgb).astype(np.int64)
    return (c[..., 0] * 19595 + c[..., 1] * 38470 + c[..., 2] * 7471 + 0x8000) >> 16


def blend(d, i, a):
    """PIL's Image.blend(degenerate d, image i, alpha a) on bytes (any broadcastable integer arrays)."""
    a = f32(a)
    d, i = np.asarray(d).astype(np.int32), np.asarray(i).astype(np.int32)
    t = d.astype(f32) + a * (i - d).astype(f32)
    assert t.dtype == f32
    if f32(0) <= a <= f32(1):
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def contrast_mean(rgb):
    """int(mean of L over the frame + 0.5), in doubles as ImageStat does."""
    L = lum(rgb)
    return int(float(L.sum()) / float(L.size) + 0.5)


def rgb_to_hsv(rgb):
    """uint8 (..., 3) -> uint8 (..., 3): PIL's convert('HSV')."""
    c = np.asarray(rgb).astype(np.int32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    maxc, minc = c.max(-1), c.min(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(f32)
        s = cr / maxc.astype(f32)
        rc, gc, bc = ((maxc - r).astype(f32) / cr, (maxc - g).astype(f32) / cr, (maxc - b).astype(f32) / cr)
        h = np.where(r == maxc, bc - gc,
                     np.where(g == maxc, (2.0 + rc.astype(f64) - bc.astype(f64)).astype(f32),
                              (4.0 + gc.astype(f64) - rc.astype(f64)).astype(f32)))
        h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
        uh = np.clip(np.nan_to_num(h.astype(f64) * 255.0).astype(np.int64), 0, 255)
        us = np.clip(np.nan_to_num(s.astype(f64) * 255.0).astype(np.int64), 0, 255)
    grey = minc == maxc
    return np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), maxc], -1).astype(np.uint8)


def _round_away(x):
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5))


def hsv_to_rgb(hsv):
    """uint8 (..., 3) -> uint8 (..., 3): PIL's convert('RGB') of an HSV image."""
    c = np.asarray(hsv)
    h, s, v = c[..., 0], c[..., 1], c[..., 2]
    h6 = h.astype(f32).astype(f64) * 6.0 / 255.0
    i = np.floor(h6)
    f = (h6 - i.astype(f32).astype(f64)).astype(f32)
    fs = (s.astype(f32).astype(f64) / 255.0).astype(f32)
    vd, fsd, fd = v.astype(f32).astype(f64), fs.astype(f64), f.astype(f64)
    p = np.clip(_round_away(vd * (1.0 - fsd)), 0, 255).astype(np.uint8)
    q = np.clip(_round_away(vd * (1.0 - fsd * fd)), 0, 255).astype(np.uint8)
    t = np.clip(_round_away(vd * (1.0 - fsd * (1.0 - fd))), 0, 255).astype(np.uint8)
    k = i.astype(np.int64) % 6
    pick = lambda *six: np.choose(k, six)            # noqa: E731
    rgb = np.stack([pick(v, q, p, p, t, v), pick(t, v, v, q, p, p), pick(p, p, t, v, v, q)], -1)
    return np.where((s == 0)[..., None], np.stack([v, v, v], -1), rgb).astype(np.uint8)


def apply_op(rgb, kind, param):
    """One op on one frame, uint8 (H, W, 3) -> uint8 (H, W, 3)."""
    rgb = np.asarray(rgb)
    kind = int(kind)
    if kind == NOP:
        return rgb.copy()
    if kind == BRIGHTNESS:
        return blend(0, rgb, param)
    if kind == CONTRAST:
        return blend(contrast_mean(rgb), rgb, param)
    if kind == SATURATION:
        return blend(lum(rgb)[..., None], rgb, param)
    if kind == HUE:
        hsv = rgb_to_hsv(rgb)
        hsv[..., 0] = ((hsv[..., 0].astype(np.int64) + int(param)) & 255).astype(np.uint8)
        return hsv_to_rgb(hsv)
    if kind == GRAY:
        return np.repeat(rgb[..., int(param)][..., None], 3, -1)
    raise ValueError("no op kind %r" % (kind,))


def apply_program(rgb, program):
    """program: [(kind, param)] in order."""
    for kind, param in program:
        rgb = apply_op(rgb, kind, param)
    return np.ascontiguousarray(rgb)


def jitter_u8(frames, programs, group_size):
    """frames uint8 (N, H, W, 3), frame n runs programs[n // group_size] -> uint8 (N, H, W, 3)."""
    frames = frames.cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
    return np.stack([apply_program(f, programs[n // group_size]) for n, f in enumerate(frames)])


def to_clips(u8, T, mean=CH.IMAGENET_MEAN, std=CH.IMAGENET_STD):
    """uint8 (N, H, W, 3) -> fp32 (N/T, 3, T, H, W): ToTensor, Normalize, frame n at clip n // T, position n % T."""
    x = CH.normalise(u8, mean, std)
    N, H, W, _ = x.shape
    return x.view(N // T, T, H, W, 3).permute(0, 4, 1, 2, 3).contiguous()


def reference(frames, programs, group_size, T, mean=CH.IMAGENET_MEAN, std=CH.IMAGENET_STD):
    return to_clips(jitter_u8(frames, programs, group_size), T, mean, std)


def table_programs(kinds, params):
    """The (G, P) tables as the kernel takes them -> [[(kind, param)]] per group."""
    kinds, params = kinds.cpu().numpy(), params.cpu().numpy()
    return [list(zip(kinds[g].tolist(), params[g].tolist())) for g in range(kinds.shape[0])]


# ---- test doubles ------------------------------------------------------------------------------------------------

CALLS = []      # ("resize", n_crops) / ("jitter", N, group_size, programs) of every call of the doubles


def resize_crops_u8(frames, slot_frame, crops, cw, ch, S, xmin, xk, ymin, yk, out):
    """Double of ops.resize_crops_u8."""
    for got, want in zip((xmin, xk), CH.kernel_layout(cw, S)):
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)
    for got, want in zip((ymin, yk), CH.kernel_layout(ch, S)):
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)
    assert frames.dtype == torch.uint8 and slot_frame.dtype == torch.int32 and 1 <= len(crops) <= 16
    assert out.dtype == torch.uint8 and tuple(out.shape) == (len(crops), slot_frame.numel(), S, S, 3)
    CALLS.append(("resize", len(crops)))
    idx = slot_frame.cpu().reshape(-1).long().numpy()
    per = CH.crop_resized_u8(frames.cpu().numpy(), [tuple(int(v) for v in c) for c in crops], cw, ch, S)
    out.copy_(torch.from_numpy(np.stack([p[idx] for p in per])))


def color_jitter_clips(frames, kinds, params, group_size, T, mean, std, out, host_tables=None):
    """Double of ops.color_jitter_clips."""
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3
    assert kinds.dtype == torch.int32 and params.dtype == torch.float32 and kinds.shape == params.shape
    N = frames.shape[0]
    assert N % T == 0 and kinds.shape[0] * group_size >= N and kinds.shape[1] <= 8
    assert host_tables is None or (torch.equal(host_tables[0], kinds.cpu()) and torch.equal(host_tables[1], params.cpu()))
    progs = table_programs(kinds, params)
    CALLS.append(("jitter", N, int(group_size), progs))
    out.copy_(reference(frames, progs, group_size, T, mean, std))


def install(monkeypatch):
    CH.install(monkeypatch)
    monkeypatch.setattr(ops, "resize_crops_u8", resize_crops_u8)
    monkeypatch.setattr(ops, "color_jitter_clips", color_jitter_clips)
    del CALLS[:]


def golden():
    """tests/golden/color_jitter.pt (tools/make_color_jitter_golden.py): what the reference's own ColorJitter and
    RandomGray classes made of small frames under fixed seeds, as bytes."""
    return torch.load(GOLDEN)


def fixture_cases(gold):
    """Every recorded run of the fixture as (id, frames uint8 (N, H, W, 3), programs, group_size, want uint8
    (N, H, W, 3), next): the programs are what staging.ColorJitter.draw yields under the run's seed (RandomGray:
    the recorded channels), `next` is what the generator must return afterwards (None where it does not apply)."""
    import random
    from coclr_amd import staging
    frames = gold["frames"].numpy()
    out = []
    for name, jit, n_groups, gs in (("A", staging.ColorJitter(0.4, 0.4, 0.4, 0.1), 1, 6),
                                    ("B", staging.ColorJitter(0.4, 0.4, 0.4, 0.1), 2, 3),
                                    ("C", staging.ColorJitter(0.2, 0.2, 0.2, 0.1, p=0.3), 1, 6)):
        for run in gold[name]:
            random.seed(run["seed"])
            progs = jit.draw(random, n_groups)
            out.append(("%s%d" % (name, run["seed"]), frames, progs, gs, run["out"].numpy(), (random.random(), run["next"])))
    sc = CH.golden()["A"]
    for run in gold["D"]:
        (x0, y0), = _five_crop_box(52, 40, 28, run["where"])
        resized = CH.crop_resized_u8(sc["frames"].numpy(), [(x0, y0, run["flip"])], 28, 28, 16)[0]
        random.seed(run["seed"])
        random.random()                                  # RandomHorizontalFlip's draw comes first in the chain
        progs = staging.ColorJitter(0.2, 0.2, 0.2, 0.1).draw(random, 1)
        out.append(("D%d" % run["where"], resized, progs, resized.shape[0], run["out"].numpy(),
                    (random.random(), run["next"])))
    for run in gold["E"]:
        out.append(("E%d" % run["seed"], frames, [[(GRAY, ch)] for ch in run["channels"]], 1, run["out"].numpy(), None))
    return out


def _five_crop_box(W, H, size, where):
    return [{1: (0, 0), 2: (W - size, 0), 3: (0, H - size), 4: (W - size, H - size),
             5: (int(round((W - size) / 2.)), int(round((H - size) / 2.)))}[where]]


def levels_expected(u8, levels, T):
    """uint8 (N, H, W, 3) -> fp32 (N/T, 3, T, H, W) through the fixture's byte table."""
    b = torch.from_numpy(np.ascontiguousarray(u8)).long()
    per = torch.stack([levels[c][b[..., c]] for c in range(3)], -1)
    N, H, W, _ = per.shape
    return per.view(N // T, T, H, W, 3).permute(0, 4, 1, 2, 3).contiguous()


def order_case():
    """All 24 orders of brightness, contrast, saturation and hue as 24 groups of one frame each, the SAME 16 x 16
    random frame, so that only the order tells the results apart: (frames (24, 16, 16, 3), programs)."""
    import itertools
    frame = np.random.RandomState(11).randint(0, 256, size=(1, 16, 16, 3)).astype(np.uint8)
    ops4 = [(BRIGHTNESS, 1.3), (CONTRAST, 0.7), (SATURATION, 1.4), (HUE, 23)]
    return np.repeat(frame, 24, 0), [list(p) for p in itertools.permutations(ops4)]


def half_mean_frame(H, W, k, nudge):
    """A grey frame whose L mean is exactly k + 0.5 (half the pixels k, half k + 1; H * W even), or, with `nudge`,
    k + 0.5 - 1 / (H * W): one pixel of the upper half one lower.  A third colour channel pattern keeps contrast
    from being the identity on it."""
    n = H * W
    g = np.full(n, k, dtype=np.uint8)
    g[n // 2:] = k + 1
    if nudge:
        g[-1] = k
    return np.repeat(g.reshape(1, H, W, 1), 3, -1)
