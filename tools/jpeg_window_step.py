"""One training batch decoded from a device-resident store and staged, whole frames against crop boxes only
(coclr_amd/jpeg.py: Store.decode(ids, boxes); coclr_amd/staging.py: clip_frames, stage_train_clips_cropped), on one
MI355X.

    python tools/jpeg_window_step.py [--samples 32] [--rounds 3] [--out profiles/jpeg_window.json]

The batch is the store table's (tools/jpeg_store_step.py): --samples samples of 2 x 32 frames, copies of the 320 x 240,
4:2:0, quality-75 frame of tests/golden/jpeg_frames.pt, in a Store of the default chunk size; the plans come from a
seeded TrainTransform(128, 32).  The legs:
  full     store.decode(ids) + stage_train_clips_ragged: the path without this feature, which it leaves untouched.
           This is the baseline; it is never the new code.
  window   clip_frames + store.decode(sel, boxes) + stage_train_clips_cropped.
Every round runs both legs once, each in a fresh child process, so the legs alternate within one command and drift of
the machine hits them alike.  A child does warm-up steps, asserts that the staged batch of its leg equals the full
route's bit for bit, then --reps timed repetitions and reports, as medians over them, the milliseconds between device
events of
  decode, stage   the two calls of a step, and `step`, their sum per repetition
  entropy, idct, colour   the three decode stages alone (stages = 1, 2, 4) on the frames of the first stage of the
                  default budget, scaled to the batch
and, derived rather than timed: the pixel bytes the decode writes (sum 3 w h against sum 3 W H), the blocks the inverse
DCT runs on, and the share of entropy lanes that return without decoding (from the store's rows, read back once).
The parent reports per leg the rows, their medians and the spread (largest minus smallest) between rounds, and says
whether the window leg's `step` is below the full leg's by more than the larger spread.  One frame copied, one
geometry, one table set: PROVISIONAL.  `--child` runs one leg of one round."""
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
KEYS = ("decode", "stage", "step", "entropy", "idct", "colour")


def median(v):
    return sorted(v)[len(v) // 2]


def child(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from coclr_amd import jpeg, ops, staging
    c = next(c for c in torch.load(FIXTURE)["cases"] if c["name"] == CASE)
    raw = c["raw"].numpy().tobytes()
    H, W = c["height"], c["width"]
    B = args.samples
    packs = [jpeg.pack([raw] * T) for _ in range(2 * B)]
    store = jpeg.Store(sum(d.numel() for d, _ in packs), 2 * B * T)
    first = [store.add(p) for p in packs]
    order = random.Random(1).sample(range(2 * B), 2 * B)
    ids = torch.tensor([[first[v] + i for v in order[2 * b:2 * b + 2] for i in range(T)] for b in range(B)])
    tt = staging.TrainTransform(S, T)
    rng, np_rng = random.Random(7), np.random.RandomState(7)
    plans = [tt.draw(W, H, rng=rng, np_rng=np_rng) for _ in range(B)]
    sel, boxes = staging.clip_frames(ids, plans, T)
    dev = torch.device("cuda")
    window = args.leg == "window"

    def decode():
        return store.decode(sel, boxes) if window else store.decode(ids.view(-1))

    def stage(frames):
        return (staging.stage_train_clips_cropped if window else staging.stage_train_clips_ragged)(frames, plans, S)

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
    want = staging.stage_train_clips_ragged(store.decode(ids.view(-1)), plans, S)
    assert torch.equal(out, want)                                            # either leg stages the same batch
    del want

    # the decode stages alone, on the first stage of the default budget
    if window:
        p_sel, geo, offset, total, stages, blocks, win = store.plan(sel, boxes=boxes)
    else:
        p_sel, geo, offset, total, stages, blocks = store.plan(ids.view(-1))
    k, e, geom, prefix = stages[0]
    n, frames = e - k, p_sel.numel()
    d_sel, d_geom, d_prefix = p_sel[k:e].to(dev), geom.to(dev), prefix.to(dev)
    pixels = torch.empty((total + 15) & ~15, dtype=torch.uint8, device=dev)
    coefs = torch.empty(blocks * 64, dtype=torch.int16, device=dev)
    planes = torch.empty(blocks * 64, dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    if window:
        d_win = win[k:e].to(dev)
        part = lambda st: ops.jpeg_decode_store_window(store._buffers(), d_sel, p_sel[k:e].contiguous(), d_geom, geom,   # noqa: E731
                                                       d_win, win[k:e].contiguous(), d_prefix, prefix, coefs, planes,
                                                       pixels, status, stages=st)
    else:
        part = lambda st: ops.jpeg_decode_store(store._buffers(), d_sel, p_sel[k:e].contiguous(), d_geom, geom, d_prefix,   # noqa: E731
                                                prefix, coefs, planes, pixels, status, stages=st)
    part(7)
    rows = {key: [] for key in KEYS}
    for _ in range(args.reps):
        for key, st in (("entropy", 1), ("idct", 2), ("colour", 4)):
            ms, _ = timed(lambda: part(st))
            rows[key].append(ms * frames / n)
        d_ms, fr = timed(decode)
        s_ms, _ = timed(lambda: stage(fr))
        rows["decode"].append(d_ms)
        rows["stage"].append(s_ms)
        rows["step"].append(d_ms + s_ms)
        del fr
    res = {"leg": args.leg, "samples": B, "frames": frames, "stage_frames": n}
    res.update({key: median(v) for key, v in rows.items()})
    # derived, not timed
    mb = 6
    mcux = -(-W // 16)
    full_blocks = mcux * -(-H // 16) * mb
    res["pixel_bytes"] = int((3 * boxes[:, 2] * boxes[:, 3]).sum()) if window else 3 * W * H * frames
    res["idct_blocks"] = full_blocks * frames
    res["entropy_lanes"] = int(store._lanes[p_sel].sum())
    res["entropy_lanes_skipped"] = 0
    if window:
        blocks_w, skipped = 0, 0
        counts = {}
        for f, box in zip(p_sel.tolist(), boxes.tolist()):
            mx0, my0, mx1, my1 = jpeg.window_mcus(H, W, 3, 2, 2, *box)
            blocks_w += (mx1 - mx0) * (my1 - my0) * mb
            lo, hi = (my0 * mcux + mx0) * mb, ((my1 - 1) * mcux + mx1) * mb
            if f not in counts:                                              # blocks completed before every chunk
                rec = store._host[0][f].tolist()
                r = store._rows[rec[6]:rec[6] + int(store._lanes[f])].cpu()
                nxt = [full_blocks if i + 1 == len(r) or int(r[i + 1, 0]) < 0 else int(r[i + 1, 1]) for i in range(len(r))]
                counts[f] = (r[:, 1].tolist(), nxt)
            own, nxt = counts[f]
            skipped += sum(1 for a, b in zip(own, nxt) if b < lo or a >= hi)
        res.update(idct_blocks=blocks_w, entropy_lanes_skipped=skipped)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--leg", default="full")
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    legs = ("full", "window")
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
        table[c] = {"rows": rows[c], "median": {k: median([r[k] for r in rows[c]]) for k in KEYS},
                    "spread": {k: max(r[k] for r in rows[c]) - min(r[k] for r in rows[c]) for k in KEYS}}
    gain = table["full"]["median"]["step"] - table["window"]["median"]["step"]
    spread = max(table["full"]["spread"]["step"], table["window"]["spread"]["step"])
    w = rows["window"][0]
    f = rows["full"][0]
    result = {"case": CASE, "samples": args.samples, "T": T, "S": S, "legs": table,
              "derived": {"pixel_bytes": {"full": f["pixel_bytes"], "window": w["pixel_bytes"]},
                          "idct_blocks": {"full": f["idct_blocks"], "window": w["idct_blocks"]},
                          "entropy_lanes": w["entropy_lanes"], "entropy_lanes_skipped": w["entropy_lanes_skipped"]},
              "verdict": {"gain_ms": gain, "spread_ms": spread, "faster": gain > spread},
              "units": "ms per batch, medians over the repetitions of a child, then over the rounds",
              "note": "PROVISIONAL: one frame copied, one geometry, one table set; a training step with the decode in the "
                      "loop is not measured here"}
    print(json.dumps({"median": {c: table[c]["median"] for c in legs}, "spread": {c: table[c]["spread"] for c in legs},
                      "derived": result["derived"], "verdict": result["verdict"]}), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
