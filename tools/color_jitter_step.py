"""The test-clip staging of one video on one MI355X with and without the reference's ColorJitter.

    python tools/color_jitter_step.py [--rounds 5] [--out profiles/color_jitter.json]

One video's ten 224 -> 128 crops of one clip of 32 frames (256 x 340 frames on the device):
  plain   staging.stage_crops_on_device(...): the single `coclr_stage_crops` launch
  jitter  the same call with jitter= ten programs drawn from ColorJitter(0.2, 0.2, 0.2, 0.1) at p = 1 (all four ops,
          shuffled): `coclr_resize_crops_u8`, then `coclr_color_jitter_clips`, and the uint8 buffer between them
The two alternate within a round; each figure is device-event time per call over `--iters` calls after a warm-up,
and the medians over the rounds are reported with the spread, next to the time the fp32 output alone would take
to write at `--hbm_gbps` (the part's nominal HBM rate).  No threshold: the plain launch on the same box is the
yardstick.  A GPU-only measurement; there is no CPU path."""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _event_ms(fn, iters):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=340)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--hbm_gbps", type=float, default=8000.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from coclr_amd import staging
    if not torch.cuda.is_available():
        raise SystemExit("color_jitter_step: no GPU; this is a measurement and has no CPU path")
    dev = torch.device("cuda")
    T, S = args.frames, args.size
    fr = torch.from_numpy(np.random.RandomState(0).randint(0, 256, size=(T, args.height, args.width, 3))
                          .astype(np.uint8)).to(dev)
    idx = staging.check_frame_index(np.arange(T)[None, :], T).to(dev)
    boxes = staging.five_crop_boxes(args.width, args.height, args.crop) * 2
    crops = staging.check_crops(boxes, [0] * 5 + [1] * 5, args.crop, args.crop, args.width, args.height)
    rng = random.Random(0)
    jit = staging.ColorJitter(0.2, 0.2, 0.2, 0.1)
    programs = [jit.draw(rng, 1)[0] for _ in crops]
    out = torch.empty(len(crops), 1, 3, T, S, S, dtype=torch.float32, device=dev)
    out_bytes = out.numel() * 4

    def plain():
        staging.stage_crops_on_device(fr, idx, crops, args.crop, args.crop, S, out=out)

    def jitter():
        staging.stage_crops_on_device(fr, idx, crops, args.crop, args.crop, S, out=out, jitter=programs)
    for fn in (plain, jitter):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rows = []
    for r in range(args.rounds):
        order = (("plain", plain), ("jitter", jitter)) if r % 2 == 0 else (("jitter", jitter), ("plain", plain))
        row = {"round": r}
        for name, fn in order:
            row[name + "_ms"] = _event_ms(fn, args.iters)
        rows.append(row)
        print(json.dumps(row), flush=True)
    med = {k: sorted(r[k] for r in rows)[len(rows) // 2] for k in ("plain_ms", "jitter_ms")}
    write_ms = out_bytes / args.hbm_gbps / 1e6
    res = {"video": {"frames": T, "height": args.height, "width": args.width, "crops": len(crops), "crop": args.crop,
                     "size": S},
           "programs": programs, "output_bytes": out_bytes, "hbm_gbps": args.hbm_gbps, "output_write_ms": write_ms,
           "plain_ms": med["plain_ms"], "jitter_ms": med["jitter_ms"], "jitter_over_plain": med["jitter_ms"] / med["plain_ms"],
           "plain_over_write": med["plain_ms"] / write_ms, "jitter_over_write": med["jitter_ms"] / write_ms,
           "plain_spread_ms": [min(r["plain_ms"] for r in rows), max(r["plain_ms"] for r in rows)],
           "jitter_spread_ms": [min(r["jitter_ms"] for r in rows), max(r["jitter_ms"] for r in rows)],
           "device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
