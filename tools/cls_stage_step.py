"""The classifier-clip staging of one batch on one MI355X: the fused double resample beside the chained one, the
launches alone, the write-stream floor and the loader's PIL chain.

    python tools/cls_stage_step.py [--rounds 5] [--out profiles/cls_stage_step.json]

One batch: 32 samples of 32 frames of 240 x 320 uint8 (on the device), plans drawn by
staging.ClassifierTransform(128, 32) from Random(0) (a fallback plan, should one be drawn, is replaced by the box of
the whole frame so that both legs can run it), staged to (32, 3, 32, 128, 128) fp32:
  fused    staging.stage_classifier_clips(...) with COCLR_CLS_FUSED=1: `coclr_resize2_boxes`, then
           `coclr_augment_clips`, with the host work of the call (unpacking the plans, tables, descriptors, uploads)
  chained  the same call with COCLR_CLS_FUSED=0: `coclr_resize_boxes_u8` twice through a (1024, 224, 224, 3) byte
           buffer, then `coclr_augment_clips` -- entry points the project had before the fused kernel: the yardstick
  launch   the fused call with staging.classifier_tables(...) computed ahead: the uploads and the two launches alone
  floor    staging.tr(...) = `coclr_stage_clips` from (32, 3, 32, 128, 128) uint8: the same number of fp32 bytes
           written from already cropped and resized frames -- the write stream alone
  pil      the same plans applied with PIL itself on `--threads` CPU threads (crop, two resizes, ImageEnhance, the
           HSV round trip, / 255), where PIL is installed: what the reference's loader spends
Every round is a fresh process under its own time limit; inside it the four GPU legs alternate (the order reverses from
round to round), each figure device-event time per call over `--iters` calls after a warm-up.  Reported: medians over
the rounds with the spread.  The default of COCLR_CLS_FUSED follows from `fused` against `chained` plus the chained
leg's own round-to-round spread (`fused_keeps_default`).  A GPU measurement; there is no CPU path."""
import argparse
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("fused", "chained", "launch", "floor")
GEOMETRY = ("batch", "frames", "height", "width", "size", "iters")


def _event_ms(fn, iters):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def _plans(args):
    sys.path.insert(0, ROOT)
    from coclr_amd import staging
    ct = staging.ClassifierTransform(args.size, args.frames)
    rng = random.Random(0)
    plans = [ct.draw(args.width, args.height, rng=rng) for _ in range(args.batch)]
    for p in plans:
        if p["form"] != "box":
            p.update(form="box", region=(0, 0, args.width, args.height), resample=(ct.size, ct.size), window=(0, 0))
    return ct, plans


def _frames(args):
    import numpy as np
    import torch
    one = torch.from_numpy(np.random.RandomState(0).randint(0, 256, size=(args.frames, args.height, args.width, 3))
                           .astype(np.uint8))
    return torch.stack([one.roll(b, 0) for b in range(args.batch)])


def child(args):
    """One round: the four GPU legs in this process, in the order of `--order`."""
    import numpy as np
    import torch
    ct, plans = _plans(args)
    from coclr_amd import staging
    if not torch.cuda.is_available():
        raise SystemExit("cls_stage_step: no GPU; this is a measurement and has no CPU path")
    dev = torch.device("cuda")
    B, T, S, H, W = args.batch, args.frames, args.size, args.height, args.width
    fr = _frames(args).to(dev)
    packed = torch.stack([staging.pack_cls_plan(p) for p in plans])
    out = torch.empty(B, 3, T, S, S, dtype=torch.float32, device=dev)
    small = torch.from_numpy(np.random.RandomState(1).randint(0, 256, size=(B, 3, T, S, S)).astype(np.uint8)).to(dev)
    tables = staging.classifier_tables(packed, B, T, W, H, S, size=ct.size)

    def staged(fused, **kw):
        def fn():
            os.environ["COCLR_CLS_FUSED"] = fused
            staging.stage_classifier_clips(fr, packed, S, out=out, size=ct.size, **kw)
        return fn
    legs = {"fused": staged("1"), "chained": staged("0"), "launch": staged("1", tables=tables),
            "floor": lambda: staging.tr(small, 1, T, out=out.view(B, 1, 3, T, S, S))}
    results = {}
    for name in LEGS:                                        # every leg's shapes warm, and the two legs agree
        for _ in range(2):
            legs[name]()
        torch.cuda.synchronize()
        if name in ("fused", "chained"):
            results[name] = out.clone()
    if not torch.equal(results["fused"], results["chained"]):
        raise SystemExit("cls_stage_step: the fused and the chained leg disagree")
    row = {}
    for name in (LEGS if args.order == 0 else LEGS[::-1]):
        row[name + "_ms"] = _event_ms(legs[name], args.iters)
    t0 = time.perf_counter()
    for _ in range(args.iters):
        legs["fused"]()
    torch.cuda.synchronize()
    row["fused_wall_ms"] = (time.perf_counter() - t0) * 1e3 / args.iters
    row["device"] = torch.cuda.get_device_name(0)
    row["jittered_clips"] = sum(1 for p in plans if p["program"])
    print(json.dumps(row), flush=True)


def _pil_clip(frames, plan, size, S):
    """One clip with PIL: frames uint8 (T, H, W, 3) -> fp32 (T, 3, S, S) in [0, 1] (the loader's ToTensor)."""
    import numpy as np
    from PIL import Image, ImageEnhance
    x0, y0, w, h = plan["region"]
    enh = {1: ImageEnhance.Brightness, 2: ImageEnhance.Contrast, 3: ImageEnhance.Color}
    out = []
    for f in frames:
        img = Image.fromarray(f).crop((x0, y0, x0 + w, y0 + h)).resize((size, size), Image.BICUBIC)
        img = img.resize((S, S), Image.BICUBIC)
        for kind, v in plan["program"]:
            if kind in enh:
                img = enh[kind](img).enhance(v)
            elif kind == 4:
                hh, ss, vv = img.convert('HSV').split()
                hh = Image.fromarray((np.array(hh, dtype=np.uint8) + np.uint8(int(v))).astype(np.uint8), 'L')
                img = Image.merge('HSV', (hh, ss, vv)).convert('RGB')
        out.append(np.asarray(img).transpose(2, 0, 1).astype(np.float32) / 255)
    return np.stack(out)


def _median(values):
    return sorted(values)[len(values) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--order", type=int, default=0)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--timeout", type=float, default=180.0)
    ap.add_argument("--hbm_gbps", type=float, default=8000.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = []
    for r in range(args.rounds):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--order=%d" % (r % 2)] + [
            "--%s=%s" % (k, getattr(args, k)) for k in GEOMETRY]
        done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.timeout,
                              env=dict(os.environ, COCLR_QUIET="1"))
        if done.returncode != 0:                                # a round that failed ends the measurement
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit("cls_stage_step: round %d failed with exit status %d" % (r, done.returncode))
        row = json.loads(done.stdout.strip().splitlines()[-1])
        row["round"] = r
        rows.append(row)
        print(json.dumps(row), flush=True)
    B, T, S = args.batch, args.frames, args.size
    out_bytes = B * 3 * T * S * S * 4
    res = {"batch": {"samples": B, "frames": T, "height": args.height, "width": args.width, "size": S},
           "output_bytes": out_bytes, "hbm_gbps": args.hbm_gbps, "output_write_ms": out_bytes / args.hbm_gbps / 1e6,
           "device": rows[0]["device"], "jittered_clips": rows[0]["jittered_clips"], "pil_ms": None,
           "pil_threads": args.threads}
    for name in LEGS + ("fused_wall",):
        v = [r[name + "_ms"] for r in rows]
        res[name + "_ms"], res[name + "_spread_ms"] = _median(v), [min(v), max(v)]
    chained_spread = res["chained_spread_ms"][1] - res["chained_spread_ms"][0]
    res["fused_over_chained"] = res["fused_ms"] / res["chained_ms"]
    res["launch_over_floor"] = res["launch_ms"] / res["floor_ms"]
    res["clips_per_s"] = B / (res["fused_ms"] * 1e-3)
    # the rule of the default: fused stays on unless its median exceeds the chained median by more than the chained
    # leg's own round-to-round spread
    res["fused_keeps_default"] = res["fused_ms"] <= res["chained_ms"] + chained_spread
    try:
        import PIL                                                    # noqa: F401
    except ImportError:
        PIL = None
    if PIL is not None:
        from concurrent.futures import ThreadPoolExecutor
        ct, plans = _plans(args)
        src = _frames(args).numpy()
        with ThreadPoolExecutor(args.threads) as pool:
            t0 = time.perf_counter()
            done = list(pool.map(lambda j: _pil_clip(*j), [(src[b], p, ct.size, S) for b, p in enumerate(plans)]))
            res["pil_ms"] = (time.perf_counter() - t0) * 1e3
        assert len(done) == B
        res["pil_over_fused"] = res["pil_ms"] / res["fused_ms"]
    res["rows"] = rows
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
