"""Writes tests/golden/train_transform.pt: small frames and what the reference's OWN training transform -- the
classes of its utils/augmentation.py chained with the settings of main_nce.py:366-390 -- makes of them under
fixed seeds.

    python tools/make_train_transform_golden.py --reference <checkout of the reference project>

utils/augmentation.py is imported UNMODIFIED through tools/make_color_jitter_golden.py (which see for the
torchvision / joblib stand-ins), plus one more stand-in, torchvision 0.5's

    transforms.RandomApply(transforms, p):  if p < random.random(): return img;  else apply them in order

Everything random -- random.choices / random / uniform / randint / shuffle, np.random.choice -- and every decision
is the reference's; PIL does the crop, the resize, the enhancements, the blur and the flip.

Samples are 2 x 3 frames of 40 rows x 52 columns, img_dim 16, seq_len 3.  The seeds are the first ones (in
order) that each add something to this list, all of which the script asserts it found: both branches of the
TransformController; the base and the null transform on either clip; either half kept by OneClipTransform;
ColorJitter applied and skipped; a gray clip; a blur whose box radius truncates to 0 and one to 1; a flip; a crop
box that does not fit (the frame is resized whole).  What a seed does is read off coclr_amd.staging.TrainTransform
under the same seed, and counts only where that leaves both generators exactly where the reference left them.

Per seed the fixture holds the frames (one tensor shared by all seeds), the reference's output as BYTES
(6, 16, 16, 3): clip 0 then clip 1), how often the reference called each generator function (`draws`), and the
values random.random() and np.random.random() return right afterwards (`next`, `np_next`).  `levels` is the byte
table of color_jitter.pt."""
import argparse
import os
import random
import sys

import numpy as np
import PIL
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_color_jitter_golden as G      # noqa: E402  (puts the repository root on sys.path too)
from coclr_amd import staging             # noqa: E402

IMG_DIM, SEQ_LEN, H, W = 16, 3, 40, 52


class RandomApply:
    def __init__(self, transforms, p=0.5):
        self.transforms, self.p = transforms, p

    def __call__(self, img):
        if self.p < random.random():
            return img
        for t in self.transforms:
            img = t(img)
        return img


def chain(A, seq_len=SEQ_LEN):
    """get_transform('train', args) of main_nce.py with args.img_dim, args.seq_len = IMG_DIM, SEQ_LEN; main_coclr.py:447-473
    is the same text with `seq_len = args.seq_len * 2` (tools/make_two_stream_golden.py)."""
    null = G.Compose([
        A.RandomSizedCrop(size=IMG_DIM, consistent=False, seq_len=seq_len, bottom_area=0.2),
        A.RandomHorizontalFlip(consistent=False, seq_len=seq_len),
        A.ToTensor()])
    base = G.Compose([
        A.RandomSizedCrop(size=IMG_DIM, consistent=False, seq_len=seq_len, bottom_area=0.2),
        RandomApply([A.ColorJitter(0.4, 0.4, 0.4, 0.1, p=1.0, consistent=False, seq_len=seq_len)], p=0.8),
        A.RandomGray(p=0.2, seq_len=seq_len),
        RandomApply([A.GaussianBlur([.1, 2.], seq_len=seq_len)], p=0.5),
        A.RandomHorizontalFlip(consistent=False, seq_len=seq_len),
        A.ToTensor()])
    return A.TransformController([A.TwoClipTransform(base, null, seq_len=seq_len, p=0.3),
                                  A.OneClipTransform(base, null, seq_len=seq_len)], weights=[0.5, 0.5])


class Draws:
    """Counts the reference's calls of the generator functions while it runs."""
    NAMES = (("random", random), ("uniform", random), ("shuffle", random), ("randint", random), ("choices", random),
             ("choice", np.random))

    def __enter__(self):
        self.count = {k: 0 for k, _ in self.NAMES}
        self.saved = [(k, mod, getattr(mod, k)) for k, mod in self.NAMES]
        for k, mod, fn in self.saved:
            setattr(mod, k, self.wrap(k, fn))
        return self

    def wrap(self, k, fn):
        def counted(*a, **kw):
            self.count[k] += 1
            return fn(*a, **kw)
        return counted

    def __exit__(self, *exc):
        for k, mod, fn in self.saved:
            setattr(mod, k, fn)


def run(transform, frames, seed):
    random.seed(seed)
    np.random.seed(seed)
    with Draws() as d:
        out = transform([Image.fromarray(f) for f in frames.numpy()])
    nxt, np_nxt = random.random(), float(np.random.random())
    x = torch.stack(out)                                                  # (6, 3, 16, 16) fp32 = byte / 255
    u8 = (x * 255).round().to(torch.uint8)
    assert torch.equal(u8.float().div(255), x)
    return {"seed": seed, "frames": frames, "out": u8.permute(0, 2, 3, 1).contiguous(), "draws": dict(d.count),
            "next": nxt, "np_next": np_nxt}


def features(seed, r):
    """What the seed exercises, from the project's own draw -- only if it follows the reference's generators."""
    random.seed(seed)
    np.random.seed(seed)
    plan = staging.TrainTransform(IMG_DIM, SEQ_LEN).draw(W, H)
    assert (random.random(), float(np.random.random())) == (r["next"], r["np_next"]), seed
    got = set()
    got.add("two clips" if _two(seed) else "one clip")
    if not _two(seed):
        got.add("one clip, half %d" % plan["half"][0])
    for c in range(2):
        progs = plan["programs"][c]
        kinds = [k for k, _ in progs[0]]
        base = _is_base(seed, c)
        got.add("%s on clip %d" % ("base" if base else "null", c))
        if base:
            got.add("jitter applied" if any(k in (1, 2, 3, 4) for k in kinds) else "jitter skipped")
        if 5 in kinds:
            got.add("gray")
            if len({p[kinds.index(5)][1] for p in progs}) > 1:
                got.add("gray, channels differ")
        for k, v in progs[0]:
            if k == 6:
                got.add("blur r = %d" % int(v))
        if 7 in kinds:
            got.add("flip")
        if plan["box"][c] == (0, 0, W, H):
            got.add("box does not fit")
    return got


def _decisions(seed):
    rng = random.Random(seed)
    two = rng.choices(range(2), weights=[0.5, 0.5])[0] == 0
    if two:
        return two, (rng.random() < 0.3, rng.random() < 0.3)
    first = rng.random() < 0.5
    return two, (first, not first)


def _two(seed):
    return _decisions(seed)[0]


def _is_base(seed, c):
    return _decisions(seed)[1][c]


WANTED = {"two clips", "one clip", "one clip, half 0", "one clip, half 1", "base on clip 0", "null on clip 0",
          "base on clip 1", "null on clip 1", "jitter applied", "jitter skipped", "gray", "gray, channels differ",
          "blur r = 0", "blur r = 1", "flip", "box does not fit"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("COCLR_REFERENCE"), required="COCLR_REFERENCE" not in os.environ)
    args = ap.parse_args()
    A = G.load_reference(args.reference)
    transform = chain(A)
    rng = np.random.RandomState(17)
    frames = rng.randint(0, 256, size=(2 * SEQ_LEN, H, W, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    frames[1] = (((yy // 5 + xx // 6) & 1) * 255).astype(np.uint8)[:, :, None]       # hard edges for the blur
    frames[4, 10:30, 12:40] = np.array([250, 30, 90], dtype=np.uint8)
    frames = torch.from_numpy(frames)
    fix = {"pil": PIL.__version__, "img_dim": IMG_DIM, "seq_len": SEQ_LEN, "runs": []}
    seen = set()
    for seed in range(400):
        r = run(transform, frames, seed)
        new = features(seed, r) - seen
        if new:
            r["covers"] = sorted(new)
            fix["runs"].append(r)
            seen |= new
        if seen >= WANTED:
            break
    assert seen >= WANTED, WANTED - seen
    levels = torch.arange(256, dtype=torch.float32)[None, :].expand(3, 256) / 255
    levels = (levels - torch.tensor(staging.IMAGENET_MEAN)[:, None]) / torch.tensor(staging.IMAGENET_STD)[:, None]
    fix["levels"] = levels.contiguous()
    out = os.path.join(G.ROOT, "tests", "golden", "train_transform.pt")
    torch.save(fix, out)
    print("wrote %s (%d bytes, seeds %s)" % (out, os.path.getsize(out), [r["seed"] for r in fix["runs"]]))
    for r in fix["runs"]:
        print(r["seed"], r["draws"], r["covers"])
    assert os.path.getsize(out) <= 200000


if __name__ == "__main__":
    main()
