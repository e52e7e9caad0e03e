"""Writes tests/golden/two_stream_transform.pt: small RGB and flow frames and what the reference's OWN two-stream
training transform -- the classes of its utils/augmentation.py chained with the settings of main_coclr.py:447-473,
that is main_nce.py's chain at `seq_len = args.seq_len * 2` -- makes of them under fixed seeds.

    python tools/make_two_stream_golden.py --reference <checkout of the reference project>

utils/augmentation.py is imported UNMODIFIED through tools/make_color_jitter_golden.py, the chain and the
RandomApply stand-in are those of tools/make_train_transform_golden.py (which see).

A sample is 4 x 3 frames of 40 rows x 52 columns in the dataset's order (dataset/lmdb_dataset.py:503-504):
rgb(clip 1), flow(clip 1), rgb(clip 2), flow(clip 2); img_dim 16, seq_len 3, so the chain runs at seq_len 6 and an
RGB clip shares its crop box, its jitter draw, its blur sigma and its flip with its flow clip, while a gray clip
draws a channel per frame across all 6.  The transform's 12 tensors are split and stacked as
lmdb_dataset.py:506-509 and the training loop's tr() (main_coclr.py:365-367) do -- two (2, 3, T, S, S) blocks
[rgb, flow] -- and stored as BYTES, `clips` (4, 3, 16, 16, 3): x1, f1, x2, f2.

The seeds are the first ones (in order) that each add something to this list, all of which the script asserts it
found: both branches of the TransformController; the base and the null transform on either clip; either half kept
by OneClipTransform; ColorJitter applied and skipped; a gray clip whose drawn channel differs between an RGB frame
and the flow frame of the same time step; a blur whose box radius truncates to 0 and one to 1; a flip; a crop box
that does not fit.  What a seed does is read off coclr_amd.staging.TrainTransform(16, 2 * 3) under the same seed, and
counts only where that leaves both generators exactly where the reference left them.

Per seed the fixture holds the frames (one tensor shared by all seeds), `clips`, how often the reference called
each generator function (`draws`), and the values random.random() and np.random.random() return right afterwards
(`next`, `np_next`).  `levels` is the byte table of color_jitter.pt."""
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
import make_train_transform_golden as TT  # noqa: E402
from coclr_amd import staging             # noqa: E402

IMG_DIM, SEQ_LEN, H, W = 16, 3, 40, 52
CHAIN_LEN = 2 * SEQ_LEN                    # main_coclr.py:448


def run(transform, frames, seed):
    T, S = SEQ_LEN, IMG_DIM
    random.seed(seed)
    np.random.seed(seed)
    with TT.Draws() as d:
        seq = transform([Image.fromarray(f) for f in frames.numpy()])
    nxt, np_nxt = random.random(), float(np.random.random())
    assert len(seq) == 4 * T
    blocks = []
    for half in (seq[0:2 * T], seq[2 * T:]):                              # lmdb_dataset.py:506-509
        x = torch.stack(half, 1)                                          # (3, 2T, S, S): rgb, flow
        blocks.append(x.view(3, 2, T, S, S).transpose(0, 1).contiguous())  # tr(): (2, 3, T, S, S)
    x = torch.cat(blocks)                                                 # x1, f1, x2, f2
    u8 = (x * 255).round().to(torch.uint8)
    assert torch.equal(u8.float().div(255), x)
    return {"seed": seed, "frames": frames, "clips": u8.permute(0, 2, 3, 4, 1).contiguous(), "draws": dict(d.count),
            "next": nxt, "np_next": np_nxt}


def features(seed, r):
    """What the seed exercises, from the project's own draw -- only if it follows the reference's generators."""
    T = SEQ_LEN
    random.seed(seed)
    np.random.seed(seed)
    plan = staging.TrainTransform(IMG_DIM, CHAIN_LEN).draw(W, H)
    assert (random.random(), float(np.random.random())) == (r["next"], r["np_next"]), seed
    two, base = TT._decisions(seed)
    got = {"two clips" if two else "one clip"}
    if not two:
        got.add("one clip, half %d" % plan["half"][0])
    for c in range(2):
        progs = plan["programs"][c]
        assert len(progs) == CHAIN_LEN
        kinds = [k for k, _ in progs[0]]
        got.add("%s on clip %d" % ("base" if base[c] else "null", c))
        if base[c]:
            got.add("jitter applied" if any(k in (1, 2, 3, 4) for k in kinds) else "jitter skipped")
        if 5 in kinds:
            got.add("gray")
            ch = [p[kinds.index(5)][1] for p in progs]
            if any(ch[j] != ch[T + j] for j in range(T)):
                got.add("gray, rgb and flow channels differ")
        for k, v in progs[0]:
            if k == 6:
                got.add("blur r = %d" % int(v))
        if 7 in kinds:
            got.add("flip")
        if plan["box"][c] == (0, 0, W, H):
            got.add("box does not fit")
    return got


WANTED = {"two clips", "one clip", "one clip, half 0", "one clip, half 1", "base on clip 0", "null on clip 0",
          "base on clip 1", "null on clip 1", "jitter applied", "jitter skipped", "gray",
          "gray, rgb and flow channels differ", "blur r = 0", "blur r = 1", "flip", "box does not fit"}


def make_frames():
    """4 x 3 frames: noise for the RGB quarters, smoother fields around mid-gray (what flow looks like) for the flow
    quarters, and hard edges in one frame of each for the blur."""
    T = SEQ_LEN
    rng = np.random.RandomState(23)
    frames = rng.randint(0, 256, size=(4 * T, H, W, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for q in (1, 3):
        for t in range(T):
            field = 128 + 60 * np.sin((yy + 3 * t + 11 * q) / 7.0)[:, :, None] * \
                np.cos((xx - 5 * t)[:, :, None] / (5.0 + np.arange(3)))
            noise = rng.randint(-12, 13, size=(H, W, 3))
            frames[q * T + t] = np.clip(np.round(field + noise), 0, 255).astype(np.uint8)
    frames[1] = (((yy // 5 + xx // 6) & 1) * 255).astype(np.uint8)[:, :, None]
    frames[T + 1, 10:30, 12:40] = np.array([250, 30, 90], dtype=np.uint8)
    frames[2 * T + 2, 5:20, 30:50] = np.array([10, 240, 200], dtype=np.uint8)
    return torch.from_numpy(frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("COCLR_REFERENCE"), required="COCLR_REFERENCE" not in os.environ)
    args = ap.parse_args()
    A = G.load_reference(args.reference)
    transform = TT.chain(A, CHAIN_LEN)
    frames = make_frames()
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
    out = os.path.join(G.ROOT, "tests", "golden", "two_stream_transform.pt")
    torch.save(fix, out)
    print("wrote %s (%d bytes, seeds %s)" % (out, os.path.getsize(out), [r["seed"] for r in fix["runs"]]))
    for r in fix["runs"]:
        print(r["seed"], r["draws"], r["covers"])
    assert os.path.getsize(out) <= 200000


if __name__ == "__main__":
    main()
