"""Decoding and staging ONE loader batch whose videos differ in frame size (kinetics400-256) on one MI355X: the ragged
entry points against what a caller had to do without them.

    python tools/ragged_step.py [--samples 32] [--seq-len 32] [--img-dim 128] [--rounds 3]
                                [--out profiles/ragged_step.json]

The batch is --samples samples of 2 x --seq-len frames; every sample is one of five frames copied -- 340 x 256,
454 x 256, 256 x 340, 320 x 256 (tests/golden/jpeg_ragged.pt) and 320 x 240 (tests/golden/jpeg_frames.pt), all 4:2:0,
quality 75, their BYTES: PIL is not needed -- assigned in a seeded mix.  Plans come from TrainTransform.draw under a
fixed seed.  Legs, each run in a fresh child process, alternating within one command, --rounds times:
  grouped      through the one-size API: group the samples by size; per group jpeg.cat, jpeg.decode and
               stage_train_clips; copy every group's result into batch order
  ragged       jpeg.decode_ragged, then stage_train_clips_ragged
  one_decode   jpeg.decode of samples * 2 * seq_len copies of the 320 x 240 frame alone
  one_ragged   jpeg.decode_ragged of the same pack: the price of the per-lane frame search on a one-size batch
A child first asserts that its pair's two results are equal, warms up, and then reports the medians over --reps
repetitions of `decode`, `stage` and `sum` (the one-size pair: `decode` alone) in milliseconds between device events,
upload and host-side table building included; packing and cat / cat_ragged (the worker's and the collate's work) are
not.  The parent reports per leg the rows, their medians and the spread (largest minus smallest) between rounds, and
the acceptance: the ragged `sum` may not be above the grouped `sum` by more than the larger of the two spreads.
`--child LEG` runs one leg of one round (what the parent starts)."""
import argparse
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = os.path.join(ROOT, "tests", "golden", "jpeg_ragged.pt")
FRAMES = os.path.join(ROOT, "tests", "golden", "jpeg_frames.pt")
ONE = "320x240_420_q75"
LEGS = ("grouped", "ragged", "one_decode", "one_ragged")


def median(v):
    return sorted(v)[len(v) // 2]


def fixtures():
    import torch
    cases = list(torch.load(RAGGED)["cases"])
    cases.append(next(c for c in torch.load(FRAMES)["cases"] if c["name"] == ONE))
    return [(c["name"], c["width"], c["height"], c["raw"].numpy().tobytes()) for c in cases]


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def child(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from coclr_amd import jpeg, staging
    fix = fixtures()
    B, T, S = args.samples, args.seq_len, args.img_dim
    n = 2 * T
    rows = {}
    if args.child in ("one_decode", "one_ragged"):
        raw = fix[-1][3]
        data, meta = jpeg.pack([raw] * (B * n))
        one, rag = jpeg.decode(data, meta), jpeg.decode_ragged(data, meta)
        assert torch.equal(rag.pixels[:one.numel()], one.reshape(-1)) and not jpeg.decode_ragged.last_status.any()
        del one, rag
        fn = (lambda: jpeg.decode(data, meta)) if args.child == "one_decode" else (lambda: jpeg.decode_ragged(data, meta))
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        rows["decode"] = [timed(fn)[0] for _ in range(args.reps)]
        res = {k: median(v) for k, v in rows.items()}
        res.update(leg=args.child, frames=B * n, compressed_bytes=data.numel())
        print(json.dumps(res))
        return
    mix = random.Random(args.seed)
    which = [mix.randrange(len(fix)) for _ in range(B)]
    packed = [jpeg.pack([f[3]] * n) for f in fix]                                # per video, as a worker would
    tt = staging.TrainTransform(S, T)
    rng, np_rng = random.Random(args.seed + 1), np.random.RandomState(args.seed + 1)
    plans = [tt.draw(fix[k][1], fix[k][2], rng=rng, np_rng=np_rng) for k in which]
    groups = {}
    for b, k in enumerate(which):
        groups.setdefault(k, []).append(b)
    cats = {k: jpeg.cat([packed[k]] * len(idx)) for k, idx in groups.items()}    # the collate's work, per leg's form
    ragged = jpeg.cat_ragged([packed[k] for k in which])
    dev = torch.device("cuda")
    out = torch.empty(B, 2, 3, T, S, S, dtype=torch.float32, device=dev)

    def grouped_decode():
        return {k: jpeg.decode(*cats[k]) for k in groups}

    def grouped_stage(frames):
        for k, idx in groups.items():
            H, W = fix[k][2], fix[k][1]
            part = staging.stage_train_clips(frames[k].view(len(idx), n, H, W, 3), [plans[b] for b in idx], S)
            out[torch.tensor(idx, device=dev)] = part
        return out

    def ragged_decode():
        return jpeg.decode_ragged(*ragged)

    def ragged_stage(frames):
        return staging.stage_train_clips_ragged(frames, plans, S, out=out)

    want = grouped_stage(grouped_decode()).clone()
    got = ragged_stage(ragged_decode())
    assert torch.equal(got, want) and not jpeg.decode_ragged.last_status.any()
    del want, got
    decode, stage = (grouped_decode, grouped_stage) if args.child == "grouped" else (ragged_decode, ragged_stage)
    for _ in range(args.warmup):
        stage(decode())
    torch.cuda.synchronize()
    rows = {"decode": [], "stage": [], "sum": []}
    for _ in range(args.reps):
        d, frames = timed(decode)
        s, _ = timed(lambda: stage(frames))
        del frames
        rows["decode"].append(d)
        rows["stage"].append(s)
        rows["sum"].append(d + s)
    res = {k: median(v) for k, v in rows.items()}
    res.update(leg=args.child, frames=B * n, sizes=sorted({(fix[k][1], fix[k][2]) for k in which}),
               groups=len(groups), compressed_bytes=int(ragged[0].numel()))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, choices=LEGS)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--seq-len", type=int, default=32)
    ap.add_argument("--img-dim", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = {leg: [] for leg in LEGS}
    for r in range(args.rounds):
        for leg in LEGS:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--samples", str(args.samples),
                   "--seq-len", str(args.seq_len), "--img-dim", str(args.img_dim), "--seed", str(args.seed),
                   "--warmup", str(args.warmup), "--reps", str(args.reps)]
            out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.timeout)
            if out.returncode != 0:
                sys.stderr.write(out.stderr[-4000:])
                raise SystemExit("round %d, leg %s failed with exit status %d" % (r, leg, out.returncode))
            rows[leg].append(json.loads(out.stdout.strip().splitlines()[-1]))
            print(json.dumps(rows[leg][-1]), flush=True)
    table = {}
    for leg in LEGS:
        keys = [k for k in ("decode", "stage", "sum") if k in rows[leg][0]]
        table[leg] = {"rows": rows[leg], "median": {k: median([r[k] for r in rows[leg]]) for k in keys},
                      "spread": {k: max(r[k] for r in rows[leg]) - min(r[k] for r in rows[leg]) for k in keys}}
    over = table["ragged"]["median"]["sum"] - table["grouped"]["median"]["sum"]
    spread = max(table["ragged"]["spread"]["sum"], table["grouped"]["spread"]["sum"])
    price = table["one_ragged"]["median"]["decode"] - table["one_decode"]["median"]["decode"]
    result = {"legs": table, "units": "ms per batch between device events; medians over the rounds",
              "acceptance": {"ragged_minus_grouped_sum_ms": over, "larger_spread_ms": spread, "holds": over <= spread},
              "one_size": {"ragged_minus_decode_ms": price,
                           "larger_spread_ms": max(table["one_ragged"]["spread"]["decode"],
                                                   table["one_decode"]["spread"]["decode"])},
              "note": "PROVISIONAL: one mix of five sizes, every sample one frame copied, one machine"}
    print(json.dumps({k: result[k] for k in ("acceptance", "one_size")}), flush=True)
    print(json.dumps({leg: table[leg]["median"] for leg in LEGS}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
