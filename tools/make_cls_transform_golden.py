"""Writes tests/golden/cls_transform.pt: small frames and what the reference's OWN classifier transform -- the
classes of its utils/augmentation.py chained as get_transform of eval/main_classifier.py:729-744 chains them -- makes
of them under fixed seeds.

    python tools/make_cls_transform_golden.py --reference <checkout of the reference project>

utils/augmentation.py is imported UNMODIFIED through tools/make_color_jitter_golden.py (which see for the
torchvision / joblib stand-ins).  The chain is

    A.RandomSizedCrop(size=24, consistent=True, bottom_area=0.2)     # crop -> bicubic resize, ten tries, else fallback
    A.Scale(16)                                                      # a second bicubic resize
    A.ColorJitter(0.4, 0.4, 0.4, 0.1, p=0.3, consistent=True)        # mode "train" only
    A.ToTensor()

on seq_len = 3 frames.  Everything random -- random.random / uniform / randint / shuffle -- and every decision is the
reference's; PIL does the crops, the resizes and the enhancements.

Three sets of frames: 40 rows x 52 columns, where the box fits on some attempt; 8 x 96, where it never can (the
smaller side of any draw is at least sqrt(0.2 * 768 * 0.75) = 10.7 > 8), so that the fallback resamples the frame to
288 x 24 and keeps the window at x = 132; and 24 x 192, where it never can either (at least 26.3 > 24) and the
fallback's Scale(24) leaves the frame as it is.  The seeds on the first set are the first ones (in order) that each
add something to the list the script asserts it found: a box on the first attempt, a box after at least one miss, a
swapped box, jitter applied and jitter skipped.  One more run has img_dim == size (Scale returns its input) and one is
the validation chain (no ColorJitter).  What a seed does is read off a loop written out below under the same seed.

Per run the fixture holds the frames (one tensor per set, shared), the reference's output as BYTES (3, S, S, 3), how
often the reference called each generator function (`draws`) and the value random.random() returns right afterwards
(`next`).  `levels` is the byte table of color_jitter.pt."""
import argparse
import math
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

SIZE, IMG_DIM, SEQ_LEN = 24, 16, 3
SETS = {"main": (40, 52), "wide8": (8, 96), "wide24": (24, 192)}           # rows, columns


def chain(A, mode, img_dim):
    """get_transform(mode, args) of eval/main_classifier.py with 224 -> SIZE and args.img_dim = img_dim."""
    steps = [A.RandomSizedCrop(size=SIZE, consistent=True, bottom_area=0.2), A.Scale(img_dim)]
    if mode == "train":
        steps.append(A.ColorJitter(0.4, 0.4, 0.4, 0.1, p=0.3, consistent=True))
    return G.Compose(steps + [A.ToTensor()])


class Draws:
    """Counts the reference's calls of the generator functions while it runs."""
    NAMES = ("random", "uniform", "shuffle", "randint")

    def __enter__(self):
        self.count = {k: 0 for k in self.NAMES}
        self.saved = [(k, getattr(random, k)) for k in self.NAMES]
        for k, fn in self.saved:
            setattr(random, k, self.wrap(k, fn))
        return self

    def wrap(self, k, fn):
        def counted(*a, **kw):
            self.count[k] += 1
            return fn(*a, **kw)
        return counted

    def __exit__(self, *exc):
        for k, fn in self.saved:
            setattr(random, k, fn)


def run(A, frames, which, seed, mode="train", img_dim=IMG_DIM):
    random.seed(seed)
    with Draws() as d:
        out = chain(A, mode, img_dim)([Image.fromarray(f) for f in frames[which].numpy()])
    nxt = random.random()
    x = torch.stack(out)                                                  # (3, 3, S, S) fp32 = byte / 255
    u8 = (x * 255).round().to(torch.uint8)
    assert torch.equal(u8.float().div(255), x) and tuple(u8.shape) == (SEQ_LEN, 3, img_dim, img_dim)
    return {"seed": seed, "set": which, "mode": mode, "img_dim": img_dim, "frames": frames[which],
            "out": u8.permute(0, 2, 3, 1).contiguous(), "draws": dict(d.count), "next": nxt}


def features(r):
    """What the run exercises, from the reference's loop written out -- only if it follows the reference's generator."""
    H, W = SETS[r["set"]]
    rng = random.Random(r["seed"])
    rng.random()
    got, misses, fitted = set(), 0, False
    for _ in range(10):
        area = rng.uniform(0.2, 1) * (W * H)
        ar = rng.uniform(3. / 4, 4. / 3)
        w, h = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
        swap = rng.random() < 0.5
        if swap:
            w, h = h, w
        if w <= W and h <= H:
            rng.randint(0, W - w), rng.randint(0, H - h)
            fitted = True
            got.add("box on the first attempt" if misses == 0 else "box after a miss")
            if swap:
                got.add("swapped box")
            break
        misses += 1
    if not fitted:
        (ow, oh), _ = staging.fallback_geometry(W, H, SIZE)
        got.add("fallback with a resample" if (ow, oh) != (W, H) else "fallback without a resample")
    if r["mode"] == "train":
        if rng.random() < 0.3:
            got.add("jitter applied")
            for lo, hi in ((0.6, 1.4), (0.6, 1.4), (0.6, 1.4), (-0.1, 0.1)):
                rng.uniform(lo, hi)
            rng.shuffle([0, 1, 2, 3])
        else:
            got.add("jitter skipped")
    else:
        got.add("validation")
    if r["img_dim"] == SIZE:
        got.add("img_dim == size")
    assert rng.random() == r["next"], (r["seed"], r["set"])
    return got


WANTED = {"box on the first attempt", "box after a miss", "swapped box", "jitter applied", "jitter skipped",
          "fallback with a resample", "fallback without a resample", "img_dim == size", "validation"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("COCLR_REFERENCE"), required="COCLR_REFERENCE" not in os.environ)
    args = ap.parse_args()
    A = G.load_reference(args.reference)
    rng = np.random.RandomState(23)
    frames = {}
    for name, (H, W) in SETS.items():
        f = rng.randint(0, 256, size=(SEQ_LEN, H, W, 3)).astype(np.uint8)
        yy, xx = np.mgrid[0:H, 0:W]
        f[1] = (((yy // 3 + xx // 5) & 1) * 255).astype(np.uint8)[:, :, None]          # hard edges for the bicubic
        f[2, H // 4:H // 2, W // 4:W // 2] = np.array([250, 30, 90], dtype=np.uint8)
        frames[name] = torch.from_numpy(f)
    fix = {"pil": PIL.__version__, "size": SIZE, "img_dim": IMG_DIM, "seq_len": SEQ_LEN, "runs": []}
    seen = set()

    def keep(r, always=False):
        new = features(r) - seen
        if new or always:
            r["covers"] = sorted(features(r))
            fix["runs"].append(r)
            seen.update(new)
    main_wanted = {"box on the first attempt", "box after a miss", "swapped box", "jitter applied", "jitter skipped"}
    for seed in range(400):
        keep(run(A, frames, "main", seed))
        if seen >= main_wanted:
            break
    for which in ("wide8", "wide24"):
        for seed in (0, 1):                                   # one with jitter drawn either way where it happens
            keep(run(A, frames, which, seed), always=True)
    keep(run(A, frames, "main", 5, img_dim=SIZE), always=True)
    keep(run(A, frames, "wide8", 2, img_dim=SIZE), always=True)
    keep(run(A, frames, "main", 6, mode="val"), always=True)
    keep(run(A, frames, "wide24", 3, mode="val"), always=True)
    assert seen >= WANTED, WANTED - seen
    # the two fallback geometries are the ones the tests name
    assert staging.fallback_geometry(96, 8, SIZE) == ((288, 24), (132, 0))
    assert staging.fallback_geometry(192, 24, SIZE) == ((192, 24), (84, 0))
    levels = torch.arange(256, dtype=torch.float32)[None, :].expand(3, 256) / 255
    levels = (levels - torch.tensor(staging.IMAGENET_MEAN)[:, None]) / torch.tensor(staging.IMAGENET_STD)[:, None]
    fix["levels"] = levels.contiguous()
    out = os.path.join(G.ROOT, "tests", "golden", "cls_transform.pt")
    torch.save(fix, out)
    print("wrote %s (%d bytes, %d runs)" % (out, os.path.getsize(out), len(fix["runs"])))
    for r in fix["runs"]:
        print(r["seed"], r["set"], r["mode"], r["img_dim"], r["draws"], r["covers"])
    assert os.path.getsize(out) <= 200000


if __name__ == "__main__":
    main()
