"""JPEG decoding of one loader batch (coclr_amd/jpeg.py) on one MI355X, per stage and per entropy path.

    python tools/jpeg_decode_step.py [--frames 2048] [--rounds 3] [--legs 0,64,128,256,512]
                                     [--out profiles/jpeg_decode_split.json]

The batch is --frames copies of the 320 x 240, 4:2:0, quality-75 frame of tests/golden/jpeg_frames.pt (its BYTES: PIL is
not needed), i.e. 64 clips of 32 frames.  A leg is one value of `chunk_bytes`: 0 the serial entropy kernel (one lane
per frame: the fixture has no restart markers), n the split kernel with a lane per chunk of n bytes.  Every round
runs every leg once, each in a fresh child process, so the legs alternate within one command and drift of the machine
hits them alike.  A child does warm-up decodes, asserts that EVERY frame equals the fixture's `rgb`, then --reps timed
repetitions, and reports, as medians over them, the milliseconds of
  pack      the host side of a worker: parse the headers, derive the tables (per batch; not GPU time)
  upload    compressed bytes + descriptors to the device
  entropy   Huffman decoding -> coefficients, on the leg's path
  idct      coefficients -> sample planes
  colour    upsampling, YCbCr -> RGB, crop
  decode    jpeg.decode as a caller runs it (upload + the three stages, chunked by max_stage_bytes)
and frames/s of `decode`.  Stages are timed with device events around the entry point (stages = 1 / 2 / 4) on one
chunk of frames that fits the default stage budget.  The parent reports per leg the rows, their medians and the
spread (largest minus smallest) of `entropy` and `decode` between rounds, and applies the rule for the default of
COCLR_JPEG_SPLIT: the split leg with the lowest median `decode`, if that median is below the serial leg's by more
than the spread between rounds of either of the two legs; otherwise 0.  All copies of one frame decode in lockstep on
the serial path (its lanes never diverge) while a split wave's lanes decode different chunks: the comparison is the
serial path's best case.  With one leg (--legs 0) the output has the form of profiles/jpeg_decode.json.
Where PIL is importable the parent also times PIL's `Image.open(BytesIO(raw)).convert('RGB')` of the same bytes on
--threads threads (the loader's side of the trade).  `--child` runs one leg of one round (what the parent starts)."""
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

    cbytes = args.chunk_bytes
    for _ in range(args.warmup):
        jpeg.decode(data, meta, out=out, chunk_bytes=cbytes)
    torch.cuda.synchronize()
    assert bool((out == rgb.to(dev)[None]).all()) and not jpeg.decode.last_status.any()
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
                                                  status, stages=stage, chunk_bytes=cbytes))
            rows[name].append(ms * args.frames / n)
        t = time.perf_counter()
        jpeg.decode(data, meta, out=out, chunk_bytes=cbytes)
        torch.cuda.synchronize()
        rows["decode"].append(1e3 * (time.perf_counter() - t))
    assert bool((out == rgb.to(dev)[None]).all()) and not jpeg.decode.last_status.any()
    res = {k: median(v) for k, v in rows.items()}
    res.update(chunk_bytes=cbytes, pack=pack_ms, frames=args.frames, stage_frames=n,
               frames_per_s=args.frames / (res["decode"] / 1e3),
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


def choose_default(legs):
    """The rule of the module docstring over {chunk_bytes: {"median", "spread"}} -> (chunk size, the reason)."""
    split = [c for c in legs if c != 0]
    if 0 not in legs or not split:
        return None, "needs the serial leg and a split leg"
    best = min(split, key=lambda c: legs[c]["median"]["decode"])
    gain = legs[0]["median"]["decode"] - legs[best]["median"]["decode"]
    spread = max(legs[0]["spread"]["decode"], legs[best]["spread"]["decode"])
    if gain > spread:
        return best, "decode at %d bytes is %.3f ms below serial; spread between rounds %.3f ms" % (best, gain, spread)
    return 0, "the best split leg (%d bytes) is %.3f ms below serial, within the spread between rounds of %.3f ms" % (
        best, gain, spread)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--chunk-bytes", type=int, default=0)
    ap.add_argument("--legs", default="0,64,128,256,512")
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
    legs = [int(v) for v in args.legs.split(",")]
    rows = {c: [] for c in legs}
    for r in range(args.rounds):
        for c in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--chunk-bytes", str(c), "--frames",
                   str(args.frames), "--warmup", str(args.warmup), "--reps", str(args.reps)]
            out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.timeout)
            if out.returncode != 0:
                sys.stderr.write(out.stderr[-4000:])
                raise SystemExit("round %d, leg %d failed with exit status %d" % (r, c, out.returncode))
            rows[c].append(json.loads(out.stdout.strip().splitlines()[-1]))
            print(json.dumps(rows[c][-1]), flush=True)
    units = "ms per batch of `frames` frames; frames_per_s of jpeg.decode (upload included)"
    if len(legs) == 1:
        summary = {k: median([r[k] for r in rows[legs[0]]]) for k in rows[legs[0]][0]}
        result = {"case": CASE, "rows": rows[legs[0]], "median": summary, "pil": pil_leg(args), "units": units}
        print(json.dumps({"median": summary, "pil": result["pil"]}), flush=True)
    else:
        table = {}
        for c in legs:
            table[c] = {"rows": rows[c], "median": {k: median([r[k] for r in rows[c]]) for k in rows[c][0]},
                        "spread": {k: max(r[k] for r in rows[c]) - min(r[k] for r in rows[c])
                                   for k in ("entropy", "decode")}}
        chosen, why = choose_default(table)
        result = {"case": CASE, "legs": {str(c): table[c] for c in legs},
                  "default": {"COCLR_JPEG_SPLIT": chosen, "why": why}, "pil": pil_leg(args), "units": units,
                  "note": "one frame copied `frames` times: the serial kernel's lanes never diverge, a split wave's "
                          "lanes decode different chunks; host frames, other frame sizes and a training step with "
                          "the decode in the loop are not measured here"}
        print(json.dumps({"median": {str(c): {k: table[c]["median"][k] for k in ("entropy", "decode", "frames_per_s")}
                                     for c in legs}, "spread": {str(c): table[c]["spread"] for c in legs},
                          "default": result["default"], "pil": result["pil"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
