"""Feeding VideoEvaluator from a device-resident JPEG store: one call for many videos (VideoEvaluator.add_stored)
against the per-video loop a user of the store writes without it, on one MI355X.

    python tools/eval_store_step.py [--rounds 3] [--workloads one,ten] [--models table,s3d]
                                    [--out profiles/eval_store.json]

The frames are copies of the 320 x 240, 4:2:0, quality-75 frame of tests/golden/jpeg_frames.pt (3 W H is a multiple of
16 there, so the per-video path has its zero-copy (F, H, W, 3) view of the decoded batch and is at its best).
T = 32, crop 224, S = 128, batch_clips = 32.  The workloads:
  one   64 videos of 32 frames, ONE centre-crop clip each: the retrieval protocol's train split
        (eval/main_classifier.py:574-606)
  ten   16 videos of 96 frames, five clips each, ten crops: the --ten_crop test
The models: `table`, a look-up that isolates the feeding, and `s3d`, the LinearClassifier on S3D.  The legs:
  loop    per video `store.decode(ids of the video)`, then `add_frames` on the view.  This is the baseline; it is never
          the new code.
  stored  `add_stored` once with all videos.
Every round runs every leg of every (workload, model) once, each in a fresh child process, so the legs alternate
within one command and drift of the machine hits them alike.  A child builds the store, runs --warmup whole passes,
then --reps timed ones and reports, as medians over them, the milliseconds of
  device   the whole pass -- every video fed and finish() -- between device events
  host     wall time until finish() returns, without waiting for the device
and a digest of the scores, which the parent requires to be the same in both legs.  The parent reports per leg the
rows, their medians and the spread (largest minus smallest) between rounds, and for every (workload, model) whether
`stored` is above `loop` by more than the larger of the two spreads.  One frame copied many times, one geometry, one
machine: PROVISIONAL.  Kernel times are not taken here.  `--child` runs one leg of one round."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "jpeg_frames.pt")
CASE = "320x240_420_q75"
T, CROP, S, BATCH = 32, 224, 128, 32
WORKLOADS = {"one": (64, 32, "center"), "ten": (16, 96, "ten")}          # videos, frames per video, crops


def median(v):
    return sorted(v)[len(v) // 2]


def child(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from coclr_amd import jpeg, staging
    from coclr_amd.eval.video import VideoEvaluator
    c = next(c for c in torch.load(FIXTURE)["cases"] if c["name"] == CASE)
    raw, (H, W) = c["raw"].numpy().tobytes(), c["rgb"].shape[:2]
    videos, length, crops = WORKLOADS[args.workload]
    pack = jpeg.pack([raw] * length)
    store = jpeg.Store(videos * pack[0].numel(), videos * length)
    first = [store.add(pack) for _ in range(videos)]
    index = np.arange(T, dtype=np.int64)[None] if args.workload == "one" else staging.test_frame_index(length, T)
    used = sorted(set(index.reshape(-1).tolist()))
    dev = torch.device("cuda")

    if args.model == "table":
        class Table(torch.nn.Module):
            def __init__(self):
                super().__init__()
                g = torch.Generator().manual_seed(0)
                self.logits = torch.nn.Parameter(torch.randn(256, 101, generator=g) * 3, requires_grad=False)
                self.feats = torch.nn.Parameter(torch.randn(256, 1024, generator=g), requires_grad=False)

            def forward(self, block):
                x = block[:, 0, 0, 0, 0].double() * staging.IMAGENET_STD[0] + staging.IMAGENET_MEAN[0]
                idx = (x * 255).round().long().clamp(0, 255)
                return self.logits[idx], self.feats[idx]
        model = Table().to(dev).eval()
    else:
        from coclr_amd.model.classifier import LinearClassifier
        torch.manual_seed(0)
        model = LinearClassifier(num_class=101, network='s3d').to(dev).eval()
    kw = dict(crops=crops, crop_size=CROP, out_size=S)

    def loop():
        ev = VideoEvaluator(model, batch_clips=BATCH)
        for v in range(videos):
            frames = store.decode(torch.arange(first[v], first[v] + length))
            view = frames.pixels[:length * H * W * 3].view(length, H, W, 3)
            ev.add_frames(view, index, label=v % 101, **kw)
        return ev.finish()

    def stored():
        ev = VideoEvaluator(model, batch_clips=BATCH)
        ev.add_stored(store, [(first[v], length, index, v % 101) for v in range(videos)], **kw)
        return ev.finish()

    step = {"loop": loop, "stored": stored}[args.leg]
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    rows = {"device": [], "host": []}
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t = time.perf_counter()
        res = step()
        host = 1e3 * (time.perf_counter() - t)
        b.record()
        torch.cuda.synchronize()
        rows["device"].append(a.elapsed_time(b))
        rows["host"].append(host)
    digest = hashlib.sha256(res.probs.cpu().numpy().tobytes() + res.features.cpu().numpy().tobytes()).hexdigest()[:16]
    out = {"workload": args.workload, "model": args.model, "leg": args.leg, "videos": videos, "frames": length,
           "clips": videos * index.shape[0] * {"center": 1, "ten": 10}[crops], "digest": digest,
           "decoded_frames": videos * (length if args.leg == "loop" else len(used))}
    out.update({k: median(v) for k, v in rows.items()})
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--leg", default="loop")
    ap.add_argument("--workload", default="one")
    ap.add_argument("--model", default="table")
    ap.add_argument("--workloads", default="one,ten")
    ap.add_argument("--models", default="table,s3d")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    cells = [(w, m) for w in args.workloads.split(",") for m in args.models.split(",")]
    legs = ("loop", "stored")
    rows = {(w, m, leg): [] for w, m in cells for leg in legs}
    for r in range(args.rounds):
        for w, m in cells:
            for leg in legs:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--leg", leg, "--workload", w, "--model", m,
                       "--warmup", str(args.warmup), "--reps", str(args.reps)]
                out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.timeout)
                if out.returncode != 0:
                    sys.stderr.write(out.stderr[-4000:])
                    raise SystemExit("round %d, %s / %s / %s failed with exit status %d" % (r, w, m, leg, out.returncode))
                rows[w, m, leg].append(json.loads(out.stdout.strip().splitlines()[-1]))
                print(json.dumps(rows[w, m, leg][-1]), flush=True)
    keys = ("device", "host")
    table = []
    for w, m in cells:
        cell = {"workload": w, "model": m}
        for leg in legs:
            rs = rows[w, m, leg]
            cell[leg] = {"rows": rs, "median": {k: median([r[k] for r in rs]) for k in keys},
                         "spread": {k: max(r[k] for r in rs) - min(r[k] for r in rs) for k in keys}}
        if len({r["digest"] for leg in legs for r in rows[w, m, leg]}) != 1:
            raise SystemExit("%s / %s: the two legs' scores differ" % (w, m))
        gap = cell["stored"]["median"]["device"] - cell["loop"]["median"]["device"]
        spread = max(cell["stored"]["spread"]["device"], cell["loop"]["spread"]["device"])
        cell["stored_minus_loop"] = {"device": gap, "larger_spread": spread, "not_slower": gap <= spread}
        table.append(cell)
        print(json.dumps({"workload": w, "model": m, "loop": cell["loop"]["median"], "stored": cell["stored"]["median"],
                          "stored_minus_loop": cell["stored_minus_loop"]}), flush=True)
    result = {"case": CASE, "T": T, "crop": CROP, "S": S, "batch_clips": BATCH, "cells": table,
              "units": "ms per whole pass: every video fed and finish()",
              "note": "one frame copied many times, one geometry, one machine: PROVISIONAL; kernel times not taken"}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
