"""The training-clip staging of one batch on one MI355X, beside its write-stream floor and the loader's PIL chain.

    python tools/train_stage_step.py [--rounds 5] [--out profiles/train_stage.json]

One batch: 32 samples of 2 x 32 frames of 240 x 320 uint8 (on the device), plans drawn by
staging.TrainTransform(128, 32) from Random(0) / RandomState(0), staged to (32, 2, 3, 32, 128, 128) fp32:
  train   staging.stage_train_clips(...): `coclr_resize_boxes_u8`, then `coclr_augment_clips`, with the host work
          of the call (unpacking the plans, tables of the boxes, descriptors, programs, five small uploads)
  launch  the same with staging.train_tables(...) computed ahead: the uploads and the two launches alone
  floor   staging.tr(...) = `coclr_stage_clips` from (32, 3, 64, 128, 128) uint8: the same number of fp32 bytes
          written from already cropped and resized frames -- the write stream alone
  pil     the same plans applied with PIL itself on `--threads` CPU threads (crop, resize, ImageEnhance, the HSV
          round trip, GaussianBlur, transpose, / 255), where PIL is installed: what the reference's loader spends
The three alternate within a round; each figure is device-event time per call over `--iters` calls after a
warm-up, medians over the rounds with the spread; `train_wall_ms` is the same call timed on the host with a
synchronize at the end.  No threshold: nobody has measured either side.  A GPU measurement; there is no CPU path."""
import argparse
import json
import os
import random
import sys
import time

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


def _pil_clip(frames, box, programs, S):
    """One clip with PIL: frames uint8 (T, H, W, 3) -> fp32 (T, 3, S, S) in [0, 1] (the loader's ToTensor)."""
    import numpy as np
    from PIL import Image, ImageEnhance, ImageFilter
    x0, y0, w, h = box
    enh = {1: ImageEnhance.Brightness, 2: ImageEnhance.Contrast, 3: ImageEnhance.Color}
    out = []
    for f, prog in zip(frames, programs):
        img = Image.fromarray(f).crop((x0, y0, x0 + w, y0 + h)).resize((S, S), Image.BICUBIC)
        for kind, v in prog:
            if kind in enh:
                img = enh[kind](img).enhance(v)
            elif kind == 4:
                hh, ss, vv = img.convert('HSV').split()
                hh = Image.fromarray((np.array(hh, dtype=np.uint8) + np.uint8(int(v))).astype(np.uint8), 'L')
                img = Image.merge('HSV', (hh, ss, vv)).convert('RGB')
            elif kind == 5:
                g = np.array(img)[:, :, int(v)]
                img = Image.fromarray(np.dstack([g, g, g]), 'RGB')
            elif kind == 6:
                img = img.filter(ImageFilter.GaussianBlur(radius=v))          # v: the sigma kept beside the plan
            elif kind == 7:
                img = img.transpose(Image.FLIP_LEFT_RIGHT)
        out.append(np.asarray(img).transpose(2, 0, 1).astype(np.float32) / 255)
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--hbm_gbps", type=float, default=8000.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from coclr_amd import staging
    if not torch.cuda.is_available():
        raise SystemExit("train_stage_step: no GPU; this is a measurement and has no CPU path")
    dev = torch.device("cuda")
    B, T, S, H, W = args.batch, args.frames, args.size, args.height, args.width
    one = torch.from_numpy(np.random.RandomState(0).randint(0, 256, size=(2 * T, H, W, 3)).astype(np.uint8))
    host = torch.stack([one.roll(b, 0) for b in range(B)])
    fr = host.to(dev)
    tt = staging.TrainTransform(S, T)
    rng, nrng = random.Random(0), np.random.RandomState(0)
    plans = [tt.draw(W, H, rng=rng, np_rng=nrng) for _ in range(B)]
    packed = torch.stack([staging.pack_plan(p, T) for p in plans])
    out = torch.empty(B, 2, 3, T, S, S, dtype=torch.float32, device=dev)
    out_bytes = out.numel() * 4
    small = torch.from_numpy(np.random.RandomState(1).randint(0, 256, size=(B, 3, 2 * T, S, S)).astype(np.uint8)).to(dev)

    def train():
        staging.stage_train_clips(fr, packed, S, out=out)

    tables = staging.train_tables(packed, B, T, W, H, S)

    def launch():
        staging.stage_train_clips(fr, None, S, out=out, tables=tables)

    def floor():
        staging.tr(small, 2, T, out=out)
    for fn in (train, launch, floor):
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    rows = []
    for r in range(args.rounds):
        order = (("train", train), ("launch", launch), ("floor", floor))
        order = order if r % 2 == 0 else order[::-1]
        row = {"round": r}
        for name, fn in order:
            row[name + "_ms"] = _event_ms(fn, args.iters)
        t0 = time.perf_counter()
        for _ in range(args.iters):
            train()
        torch.cuda.synchronize()
        row["train_wall_ms"] = (time.perf_counter() - t0) * 1e3 / args.iters
        rows.append(row)
        print(json.dumps(row), flush=True)
    med = {k: sorted(r[k] for r in rows)[len(rows) // 2] for k in ("train_ms", "launch_ms", "floor_ms", "train_wall_ms")}
    res = {"batch": {"samples": B, "frames": 2 * T, "height": H, "width": W, "size": S}, "output_bytes": out_bytes,
           "hbm_gbps": args.hbm_gbps, "output_write_ms": out_bytes / args.hbm_gbps / 1e6,
           "train_ms": med["train_ms"], "launch_ms": med["launch_ms"], "floor_ms": med["floor_ms"],
           "train_wall_ms": med["train_wall_ms"], "launch_over_floor": med["launch_ms"] / med["floor_ms"],
           "clips_per_s": 2 * B / (med["train_ms"] * 1e-3), "clips_per_s_launch": 2 * B / (med["launch_ms"] * 1e-3),
           "train_spread_ms": [min(r["train_ms"] for r in rows), max(r["train_ms"] for r in rows)],
           "floor_spread_ms": [min(r["floor_ms"] for r in rows), max(r["floor_ms"] for r in rows)],
           "pil_ms": None, "pil_threads": args.threads, "device": torch.cuda.get_device_name(0), "rows": rows}
    try:
        import PIL                                                    # noqa: F401
    except ImportError:
        PIL = None
    if PIL is not None:
        from concurrent.futures import ThreadPoolExecutor
        # the plans again with the sigma in place of the box radius: PIL takes the sigma
        rng, nrng = random.Random(0), np.random.RandomState(0)
        saved, staging.blur_box_radius = staging.blur_box_radius, lambda sigma: sigma
        try:
            pil_plans = [tt.draw(W, H, rng=rng, np_rng=nrng) for _ in range(B)]
        finally:
            staging.blur_box_radius = saved
        src = host.numpy()
        jobs = [(src[b, p["half"][c] * T:(p["half"][c] + 1) * T], p["box"][c], p["programs"][c], S)
                for b, p in enumerate(pil_plans) for c in range(2)]
        with ThreadPoolExecutor(args.threads) as pool:
            t0 = time.perf_counter()
            done = list(pool.map(lambda j: _pil_clip(*j), jobs))
            res["pil_ms"] = (time.perf_counter() - t0) * 1e3
        assert len(done) == 2 * B
        res["pil_over_train"] = res["pil_ms"] / med["train_ms"]
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
