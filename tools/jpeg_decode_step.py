"""JPEG decoding of one loader batch (coclr_amd/jpeg.py) on one MI355X, per stage.

    python tools/jpeg_decode_step.py [--frames 2048] [--rounds 3] [--out profiles/jpeg_decode.json]

The batch is --frames copies of the 320 x 240, 4:2:0, quality-75 frame of tests/golden/jpeg_frames.pt (its BYTES: PIL is
not needed), i.e. 64 clips of 32 frames.  Every round is a fresh child process: warm-up decodes, then --reps timed
ones.  A child reports, as medians over its repetitions, the milliseconds of
  pack      the host side of a worker: parse the headers, derive the tables (per batch; not GPU time)
  upload    compressed bytes + descriptors to the device
  entropy   Huffman decoding -> coefficients (one lane per frame: the fixture has no restart markers)
  idct      coefficients -> sample planes
  colour    upsampling, YCbCr -> RGB, crop
  decode    jpeg.decode as a caller runs it (upload + the three stages, chunked by max_stage_bytes)
and frames/s of `decode`.  Stages are timed with device events around coclr_jpeg_decode(stages = 1 / 2 / 4) on one
chunk of frames that fits the default stage budget.  Where PIL is importable the parent also times PIL's
`Image.open(BytesIO(raw)).convert('RGB')` of the same bytes on --threads threads (the loader's side of the trade).
`--child` runs one round (what the parent starts)."""
import argparse
import io
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "jpeg_frames.pt")
CASE = "320x240_420_q75"


def fixture_bytes():
    import torch
    c = next(c for c in torch.load(FIXTURE)["cases"] if c["name"] == CASE)
    return c["raw"].numpy().tobytes(), c["rgb"]


def median(v):
    return sorted(v)[len(v) // 2]


def child(args):
    sys.path.insert(0, ROOT)
    import torch
    from coclr_amd import jpeg, ops
    raw, rgb = fixture_bytes()
    raws = [raw] * args.frames
    t = time.perf_counter()
    data, meta = jpeg.pack(raws)
    pack_ms = 1e3 * (time.perf_counter() - t)
    H, W, ncomp, hs, vs = jpeg.check_meta(data, meta)
    dev = torch.device("cuda")
    out = torch.empty(args.frames, H, W, 3, dtype=torch.uint8, device=dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), r

    for _ in range(args.warmup):
        jpeg.decode(data, meta, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out[0].cpu(), rgb) and torch.equal(out[-1].cpu(), rgb) and not jpeg.decode.last_status.any()
    rows = {k: [] for k in ("upload", "entropy", "idct", "colour", "decode")}
    # the stages alone, on the frames of one chunk of the default budget
    cb, pb = ops.jpeg_workspace(H, W, ncomp, hs, vs)
    n = max(1, min(args.frames, (256 << 20) // (cb + pb)))
    host = meta[:n, 8:].contiguous()
    coefs = torch.empty(n * cb // 2, dtype=torch.int16, device=dev)
    planes = torch.empty(n * pb, dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    pinned = (data.pin_memory(), host.pin_memory())
    for _ in range(args.reps):
        ms, (d_data, d_meta) = timed(lambda: (pinned[0].to(dev, non_blocking=True), pinned[1].to(dev, non_blocking=True)))
        rows["upload"].append(ms * args.frames / n if n < args.frames else ms)
        for name, stage in (("entropy", 1), ("idct", 2), ("colour", 4)):
            ms, _ = timed(lambda: ops.jpeg_decode(d_data, d_meta, host, H, W, ncomp, hs, vs, coefs, planes, out[:n],
                                                  status, stages=stage))
            rows[name].append(ms * args.frames / n)
        t = time.perf_counter()
        jpeg.decode(data, meta, out=out)
        torch.cuda.synchronize()
        rows["decode"].append(1e3 * (time.perf_counter() - t))
    res = {k: median(v) for k, v in rows.items()}
    res.update(pack=pack_ms, frames=args.frames, stage_frames=n, frames_per_s=args.frames / (res["decode"] / 1e3),
               compressed_bytes=data.numel(), frame_bytes=args.frames * H * W * 3)
    print(json.dumps(res))


def pil_leg(args):
    try:
        from PIL import Image
    except ImportError:
        return None
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    raw, _ = fixture_bytes()

    def one(_):
        return np.asarray(Image.open(io.BytesIO(raw)).convert("RGB")).shape

    times = []
    with ThreadPoolExecutor(args.threads) as pool:
        list(pool.map(one, range(args.threads * 4)))
        for _ in range(max(3, args.rounds)):
            t = time.perf_counter()
            list(pool.map(one, range(args.frames), chunksize=16))
            times.append(time.perf_counter() - t)
    dt = median(times)
    return {"threads": args.threads, "ms": 1e3 * dt, "frames_per_s": args.frames / dt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = []
    for r in range(args.rounds):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--frames", str(args.frames), "--warmup",
               str(args.warmup), "--reps", str(args.reps)]
        out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.timeout)
        if out.returncode != 0:
            sys.stderr.write(out.stderr[-4000:])
            raise SystemExit("round %d failed with exit status %d" % (r, out.returncode))
        rows.append(json.loads(out.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), flush=True)
    summary = {k: median([r[k] for r in rows]) for k in rows[0]}
    result = {"case": CASE, "rows": rows, "median": summary, "pil": pil_leg(args),
              "units": "ms per batch of `frames` frames; frames_per_s of jpeg.decode (upload included)"}
    print(json.dumps({"median": summary, "pil": result["pil"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
