"""One CoCLR two-stream batch (RGB + flow) decoded from a device-resident store and staged, on one MI355X: the route
through the one-stream functions plus copies against coclr_amd/staging.py's stage_two_stream_clips_ragged,
stage_two_stream_clips_cropped and two_stream_frames.

    python tools/two_stream_step.py [--samples 32] [--rounds 3] [--out profiles/two_stream.json]

The batch: --samples samples of 4 x 32 frames -- per sample an RGB and a flow video of 2 x 32 frames under different
ids of ONE jpeg.Store, copies of the 320 x 240, 4:2:0, quality-75 frame of tests/golden/jpeg_frames.pt -- staged to
128 x 128; the plans come from a seeded TrainTransform(128, 2 * 32).  The model is CoCLR(reverse=False), which reads x1,
x2 and f2.  The legs:
  baseline       store.decode of all 4 T frames in the dataset's order, stage_train_clips_ragged at T' = 2 T, then the
                 view / transpose and the three `.contiguous()` tensors the model reads.  It uses only functions that
                 exist without the two-stream staging, so this file runs it on a checkout from before as well.
  four           the same decode, stage_two_stream_clips_ragged(reverse=None).
  three          two_stream_frames(reverse=False, boxes=False), a full-frame decode of what is read,
                 stage_two_stream_clips_ragged(first=, reverse=False).
  three_cropped  two_stream_frames(reverse=False), store.decode(sel, boxes), stage_two_stream_clips_cropped.
Every round runs every leg once, each in a fresh child process, so the legs alternate within one command and drift of
the machine hits them alike.  A child does warm-up steps, asserts (new legs) that its x1, x2 and f2 equal the
baseline route's bit for bit, then --reps timed repetitions and reports, as medians over them, the milliseconds
between device events of `decode`, `stage` (for the baseline: the staging AND the copies; `copies` alone beside it) and
`step`, their sum per repetition, with the frames decoded.  The parent reports per leg the rows, their medians and the
spread (largest minus smallest) between rounds, and says whether the three-clip full-frame leg's `step` is above the
baseline's by more than the larger spread.  One frame copied, one geometry, one table set: PROVISIONAL.  `--child` runs
one leg of one round."""
import argparse
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "jpeg_frames.pt")
CASE = "320x240_420_q75"
T, S = 32, 128
LEGS = ("baseline", "four", "three", "three_cropped")
KEYS = ("decode", "stage", "copies", "step")


def median(v):
    return sorted(v)[len(v) // 2]


def child(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from coclr_amd import jpeg, staging
    c = next(c for c in torch.load(FIXTURE)["cases"] if c["name"] == CASE)
    raw = c["raw"].numpy().tobytes()
    H, W = c["height"], c["width"]
    B, leg = args.samples, args.leg
    packs = [jpeg.pack([raw] * (2 * T)) for _ in range(2 * B)]              # per sample an RGB and a flow video
    store = jpeg.Store(sum(d.numel() for d, _ in packs), 4 * B * T)
    first = [store.add(p) for p in packs]
    order = random.Random(1).sample(range(2 * B), 2 * B)
    ids_rgb = torch.tensor([[first[order[2 * b]] + i for i in range(2 * T)] for b in range(B)])
    ids_flow = torch.tensor([[first[order[2 * b + 1]] + i for i in range(2 * T)] for b in range(B)])
    tt = staging.TrainTransform(S, 2 * T)
    rng, np_rng = random.Random(7), np.random.RandomState(7)
    plans = [tt.draw(W, H, rng=rng, np_rng=np_rng) for _ in range(B)]
    everything = torch.cat([ids_rgb[:, :T], ids_flow[:, :T], ids_rgb[:, T:], ids_flow[:, T:]], 1).reshape(-1)

    def baseline_stage(frames):
        return staging.stage_train_clips_ragged(frames, plans, S)           # (B, 2, 3, 2T, S, S)

    def baseline_copies(out):
        v = out.view(B, 2, 3, 2, T, S, S)                                   # [sample, clip, channel, stream, t]
        return v[:, 0, :, 0].contiguous(), v[:, 1, :, 0].contiguous(), v[:, 1, :, 1].contiguous()       # x1, x2, f2

    if leg == "baseline":
        sel, decode = everything, lambda: store.decode(everything)
        stage = lambda fr: baseline_copies(baseline_stage(fr))              # noqa: E731
    elif leg == "four":
        sel, decode = everything, lambda: store.decode(everything)

        def stage(fr):
            r = staging.stage_two_stream_clips_ragged(fr, plans, S)
            return r.x1, r.x2, r.f2
    elif leg == "three":
        sel, quarters = staging.two_stream_frames(ids_rgb, ids_flow, plans, T, reverse=False, boxes=False)
        decode = lambda: store.decode(sel)                                  # noqa: E731

        def stage(fr):
            r = staging.stage_two_stream_clips_ragged(fr, plans, S, first=quarters, reverse=False)
            return r.x1, r.x2, r.f2
    else:
        sel, boxes = staging.two_stream_frames(ids_rgb, ids_flow, plans, T, reverse=False)
        decode = lambda: store.decode(sel, boxes)                           # noqa: E731

        def stage(fr):
            r = staging.stage_two_stream_clips_cropped(fr, plans, S, reverse=False)
            return r.x1, r.x2, r.f2

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), r

    for _ in range(args.warmup):
        out = stage(decode())
    assert not bool(store.decode.last_status.any())
    if leg != "baseline":
        want = baseline_copies(baseline_stage(store.decode(everything)))
        assert all(torch.equal(a, b) for a, b in zip(out, want))            # every leg stages the same three tensors
        del want
    assert all(t.is_contiguous() and t.shape == (B, 3, T, S, S) for t in out)
    del out
    rows = {key: [] for key in KEYS}
    for _ in range(args.reps):
        d_ms, fr = timed(decode)
        if leg == "baseline":
            s_ms, staged = timed(lambda: baseline_stage(fr))
            c_ms, _ = timed(lambda: baseline_copies(staged))
            del staged
        else:
            (s_ms, _), c_ms = timed(lambda: stage(fr)), 0.0
        rows["decode"].append(d_ms)
        rows["stage"].append(s_ms + c_ms)
        rows["copies"].append(c_ms)
        rows["step"].append(d_ms + s_ms + c_ms)
        del fr
    res = {"leg": leg, "samples": B, "frames": int(sel.numel())}
    res.update({key: median(v) for key, v in rows.items()})
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--leg", default="baseline", choices=LEGS)
    ap.add_argument("--legs", default=",".join(LEGS), help="the legs of a round, e.g. `baseline` alone on an older checkout")
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    legs = tuple(args.legs.split(","))
    rows = {c: [] for c in legs}
    for r in range(args.rounds):
        for c in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--leg", c, "--samples", str(args.samples),
                   "--warmup", str(args.warmup), "--reps", str(args.reps)]
            out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.timeout)
            if out.returncode != 0:
                sys.stderr.write(out.stderr[-4000:])
                raise SystemExit("round %d, leg %s failed with exit status %d" % (r, c, out.returncode))
            rows[c].append(json.loads(out.stdout.strip().splitlines()[-1]))
            print(json.dumps(rows[c][-1]), flush=True)
    table = {}
    for c in legs:
        table[c] = {"rows": rows[c], "frames": rows[c][0]["frames"],
                    "median": {k: median([r[k] for r in rows[c]]) for k in KEYS},
                    "spread": {k: max(r[k] for r in rows[c]) - min(r[k] for r in rows[c]) for k in KEYS}}
    result = {"case": CASE, "samples": args.samples, "T": T, "S": S, "reverse": False, "legs": table,
              "units": "ms per batch between device events, medians over the repetitions of a child, then over the rounds",
              "note": "PROVISIONAL: one frame copied, one geometry, one table set; a training step with the decode in the "
                      "loop is not measured here"}
    if "baseline" in table and "three" in table:
        over = table["three"]["median"]["step"] - table["baseline"]["median"]["step"]
        spread = max(table["baseline"]["spread"]["step"], table["three"]["spread"]["step"])
        result["verdict"] = {"three_minus_baseline_ms": over, "spread_ms": spread, "not_slower": over <= spread}
    print(json.dumps({"median": {c: table[c]["median"] for c in legs}, "spread": {c: table[c]["spread"] for c in legs},
                      "frames": {c: table[c]["frames"] for c in legs}, "verdict": result.get("verdict")}), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
