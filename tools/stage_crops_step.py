"""The five/ten-crop staging kernel on one MI355X against a plain streaming write of the same size, and (where
PIL is importable) the reference's CPU chain for the same video.

    python tools/stage_crops_step.py [--rounds 5] [--out profiles/stage_crops.json]

One realistic test video: 60 frames of 256 x 340, five overlapping clips of T = 32 with evenly spaced starts
(0, 7, 14, 21, 28; `--clips 0` takes the reference's own sampling, staging.test_frame_index, instead: two clips at
60 frames, five at 100), ten crops 224 -> 128.
  a  `coclr_stage_crops` alone: frames, indices and tables on the device, one launch per round of `--iters`
  b  `coclr_stage_clips` from uint8 writing the SAME number of fp32 output bytes in the same process: one byte
     read and four written per element, no resampling -- the write stream the crop kernel cannot beat
  c  the reference chain on the CPU for the same video (Image.transpose / crop / resize(BICUBIC), /255, Normalize)
     over the ten passes the reference makes, on `--threads` threads; skipped where PIL is absent
a and b alternate within a round; each figure is device-event time per launch over `--iters` launches after a
warm-up, and the medians over the rounds are reported with the spread."""
import argparse
import json
import os
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


def _pil_chain(args, frames, index, boxes, flips):
    try:
        from PIL import Image
    except ImportError:
        return None
    import numpy as np
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from coclr_amd.staging import IMAGENET_MEAN, IMAGENET_STD
    mean = torch.tensor(IMAGENET_MEAN).view(3, 1, 1)
    std = torch.tensor(IMAGENET_STD).view(3, 1, 1)
    torch.set_num_threads(1)

    def one(job):
        f, (x0, y0), flip = job
        img = Image.fromarray(frames[f])
        if flip:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        img = img.crop((x0, y0, x0 + args.crop, y0 + args.crop)).resize((args.size, args.size), Image.BICUBIC)
        x = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).float() / 255
        return (x - mean) / std
    # the reference transforms every frame of every clip anew for each of its ten passes over the test set
    jobs = [(int(f), b, fl) for b, fl in zip(boxes, flips) for f in index.reshape(-1)]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(args.threads) as pool:
        n = sum(1 for _ in pool.map(one, jobs, chunksize=32))
    return {"ms": 1e3 * (time.perf_counter() - t0), "frames_resampled": n, "threads": args.threads}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--clips", type=int, default=5, help="0: the reference's test-mode sampling")
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=340)
    ap.add_argument("--seq_len", type=int, default=32)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from coclr_amd import staging
    if not torch.cuda.is_available():
        raise SystemExit("stage_crops_step: no GPU; this is a measurement and has no CPU path")
    rng = np.random.RandomState(0)
    frames = rng.randint(0, 256, size=(args.frames, args.height, args.width, 3)).astype(np.uint8)
    if args.clips:
        starts = np.linspace(0, args.frames - args.seq_len, args.clips).astype(np.int64)
        index = starts[:, None] + np.arange(args.seq_len, dtype=np.int64)[None, :]
    else:
        index = staging.test_frame_index(args.frames, args.seq_len)
    boxes = staging.five_crop_boxes(args.width, args.height, args.crop) * 2
    flips = [0] * 5 + [1] * 5
    n_clips, T, S = index.shape[0], args.seq_len, args.size
    dev = torch.device("cuda")
    fr = torch.from_numpy(frames).to(dev)
    idx = staging.check_frame_index(index, args.frames).to(dev)
    crops = staging.check_crops(boxes, flips, args.crop, args.crop, args.width, args.height)
    out = torch.empty(len(crops), n_clips, 3, T, S, S, dtype=torch.float32, device=dev)
    out_bytes = out.numel() * 4
    # b: the same output bytes through stage_clips from uint8: (B, 3, 1*T, S, S) with B = crops * clips
    src_b = torch.randint(0, 256, (len(crops) * n_clips, 3, T, S, S), dtype=torch.uint8, device=dev)
    out_b = torch.empty(len(crops) * n_clips, 1, 3, T, S, S, dtype=torch.float32, device=dev)
    assert out_b.numel() == out.numel()

    def run_a():
        staging.stage_crops_on_device(fr, idx, crops, args.crop, args.crop, S, out=out)

    def run_b():
        staging.tr(src_b, 1, T, out=out_b)
    for fn in (run_a, run_b):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rows = []
    for r in range(args.rounds):
        order = (("a", run_a), ("b", run_b)) if r % 2 == 0 else (("b", run_b), ("a", run_a))
        row = {"round": r}
        for name, fn in order:
            row[name + "_ms"] = _event_ms(fn, args.iters)
        rows.append(row)
        print(json.dumps(row), flush=True)
    med = {k: sorted(r[k] for r in rows)[len(rows) // 2] for k in ("a_ms", "b_ms")}
    res = {"video": {"frames": args.frames, "height": args.height, "width": args.width, "clips": n_clips, "T": T,
                     "crops": len(crops), "crop": args.crop, "size": S},
           "output_bytes": out_bytes, "frame_bytes": int(frames.nbytes),
           "a_stage_crops_ms": med["a_ms"], "b_stage_clips_u8_ms": med["b_ms"],
           "a_over_b": med["a_ms"] / med["b_ms"],
           "a_output_GBps": out_bytes / med["a_ms"] / 1e6, "b_output_GBps": out_bytes / med["b_ms"] / 1e6,
           "a_spread_ms": [min(r["a_ms"] for r in rows), max(r["a_ms"] for r in rows)],
           "b_spread_ms": [min(r["b_ms"] for r in rows), max(r["b_ms"] for r in rows)],
           "rows": rows, "c_pil_chain": _pil_chain(args, frames, index, boxes, flips)}
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
