"""Gradient-free consumers of the classifier backbone on one MI355X: inference launch plans (COCLR_PLAN_INFER=1)
against the interpreted pass (=0), and the video-level evaluator against the reference's per-video loop.

    python tools/eval_step.py [--legs a,b,c,d] [--rounds 3] [--out profiles/eval_step.json]

Legs, each in a fresh child process, alternating planned / interpreted within a round:
  a  linear-probe training step, B = 32: `_classifier_loop.train_step` with `--train_what last` (backbone frozen
     and in eval(), final_bn + final_fc trained; eval/main_classifier.py:125-130,319-351)
  b  validation pass, B = 32 (:385-402): transform, forward under no_grad, loss, top-k, the three `.item()` reads
  c  the test loop (:482-494): one video per pass, 10 clips, the permuted view of :448 as input, then
     `F.softmax(logit).mean(0)`
  d  the same videos through coclr_amd.eval.video.VideoEvaluator (batch_clips = 32): one add() per video, finish()
Every leg reports ms per pass (host clock over a window that ends in a synchronise; a pass of c / d is one VIDEO),
the host milliseconds spent inside the model call per model pass, and clips/s.  Clips are 3x32x128x128, staged on
the device once (the loader and the crop transforms are not what is measured).
`--child a|b|c|d` runs one leg with the environment as it is (also the command to put under rocprofv3)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(args):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    import torch.nn.functional as F
    import model.classifier as product
    import _classifier_loop as L
    from coclr_amd import engine
    from coclr_amd.eval.video import VideoEvaluator
    from oracle import coclr_oracle as orc
    leg = args.child
    torch.manual_seed(0)
    bare, call, opt, crit = L.build_classifier(product, train_what="last", optim="sgd", gpu=0)
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(1)
    host, calls = [0.0], [0]
    inner = bare.forward

    def timed_forward(block):
        t = time.perf_counter()
        out = inner(block)
        host[0] += time.perf_counter() - t
        calls[0] += 1
        return out
    bare.forward = timed_forward
    T_, S_ = args.seq_len, args.img_dim
    if leg in ("a", "b"):
        clips = torch.rand(args.batch, 3, T_, S_, S_, generator=g).cuda()
        target = torch.randint(0, 101, (args.batch,), generator=g).cuda()
        per_pass = args.batch
        if leg == "a":
            L.begin_epoch(call, bare, "last")

            def step():
                L.train_step(call, opt, crit, clips, target, dev, T_, S_, orc.calc_topk_accuracy)
        else:
            call.eval()

            def step():
                with torch.no_grad():
                    x = L._tr(clips, False, 1, T_, S_).squeeze(1)
                    logit, _ = call(x)
                    loss = crit(logit, target)
                    top1, top5 = orc.calc_topk_accuracy(logit, target, (1, 5))
                    loss.item(), top1.item(), top5.item()
    else:
        call.eval()
        n = args.clips_per_video
        # a video as the loader's transform leaves it: (3, n, T, H, W), handed to the model as the permuted view
        videos = [torch.randn(3, n, T_, S_, S_, generator=g).cuda() for _ in range(args.videos)]
        per_pass = n
        state = {"i": 0, "ev": None}
        if leg == "c":
            def step():
                with torch.no_grad():
                    v = videos[state["i"] % len(videos)]
                    state["i"] += 1
                    logit, _ = call(v.permute(1, 0, 2, 3, 4))
                    return F.softmax(logit, dim=-1).mean(0, keepdim=True)
        else:
            def step():
                if state["ev"] is None:
                    state["ev"] = VideoEvaluator(call, batch_clips=args.batch)
                state["ev"].add(videos[state["i"] % len(videos)].permute(1, 0, 2, 3, 4))
                state["i"] += 1
                if state["i"] % len(videos) == 0:
                    res = state["ev"].finish()
                    state["ev"] = None
                    return res
    warm = args.warmup if leg in ("a", "b") else max(args.warmup, 2) * args.videos
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    host[0], calls[0] = 0.0, 0
    stats0 = dict(engine.PLAN_STATS)
    unit = 1 if leg in ("a", "b") else args.videos       # c / d: whole rounds over the videos
    n_, t0 = 0, time.perf_counter()
    while True:
        for _ in range(unit):
            step()
        n_ += unit
        if n_ >= args.min_steps and time.perf_counter() - t0 >= args.window:
            break
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({
        "leg": leg, "plan_infer": bool(engine.PLAN_INFER), "passes": n_, "model_passes": calls[0],
        "ms_per_pass": 1e3 * dt / n_, "clips_per_s": per_pass * n_ / dt,
        "host_ms_in_model": 1e3 * host[0] / max(calls[0], 1),
        "infer_replayed": engine.PLAN_STATS["infer_replayed"] - stats0["infer_replayed"],
        "clips_per_pass": per_pass}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["a", "b", "c", "d"])
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq_len", type=int, default=32)
    ap.add_argument("--img_dim", type=int, default=128)
    ap.add_argument("--videos", type=int, default=16)
    ap.add_argument("--clips_per_video", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--min_steps", type=int, default=10)
    ap.add_argument("--window", type=float, default=2.0)
    ap.add_argument("--timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = []
    keys = ("ms_per_pass", "clips_per_s", "host_ms_in_model")
    for leg in args.legs.split(","):
        for r in range(args.rounds):
            for plan in (("1", "0") if r % 2 == 0 else ("0", "1")):
                env = dict(os.environ, COCLR_QUIET="1", COCLR_PLAN_INFER=plan)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", leg] + [
                    "--%s=%s" % (k, getattr(args, k)) for k in (
                        "batch", "seq_len", "img_dim", "videos", "clips_per_video", "warmup", "min_steps", "window")]
                out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=args.timeout)
                if out.returncode != 0:
                    sys.stderr.write(out.stderr[-4000:])
                    raise SystemExit("leg %s (COCLR_PLAN_INFER=%s) failed with exit status %d"
                                     % (leg, plan, out.returncode))
                row = json.loads(out.stdout.strip().splitlines()[-1])
                row["round"] = r
                rows.append(row)
                print(json.dumps(row), flush=True)
    summary = {}
    for leg in args.legs.split(","):
        for plan in (True, False):
            sel = [r for r in rows if r["leg"] == leg and r["plan_infer"] == plan]
            summary["%s_%s" % (leg, "planned" if plan else "interpreted")] = {
                k: sorted(r[k] for r in sel)[len(sel) // 2] for k in keys}
    print(json.dumps({"median": summary}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"rows": rows, "median": summary, "batch": args.batch,
                       "clip": [3, args.seq_len, args.img_dim, args.img_dim], "videos": args.videos,
                       "clips_per_video": args.clips_per_video}, f, indent=1)


if __name__ == "__main__":
    main()
