"""Fine-tuning step of eval/main_classifier.py (restated by tests/_classifier_loop.py: `--train_what ft`, the
backbone at lr/10, one param group per tensor) on one MI355X: native optimisers against torch's.

    python tools/finetune_step.py [--optims sgd,adam] [--rounds 2] [--batch 32] [--out profiles/x.json]

runs, for each optimiser, legs alternating native / torch (COCLR_PATCH_SGD=0 / COCLR_PATCH_ADAM=0), each in
a fresh child process: warm-up steps, then a timed window of at least --window seconds.  Every leg reports
ms/step, clips/s and the host milliseconds spent inside `optimizer.step()`.  The batch is staged on the
device once (the loader is not what is measured); each step is `_classifier_loop.train_step`: transform,
forward, CrossEntropyLoss, top-k accuracy, the three `.item()` reads, zero_grad, backward, step.
`--child native|torch` runs one leg (what the parent starts; also the command to put under rocprofv3)."""
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
    import model.classifier as product      # the shim: install() unless COCLR_PATCH_* = 0
    import _classifier_loop as L
    from oracle import coclr_oracle as orc
    torch.manual_seed(0)
    _, call, opt, crit = L.build_classifier(product, train_what="ft", optim=args.optim, gpu=0)
    L.begin_epoch(call, call.module, "ft")
    g = torch.Generator().manual_seed(1)
    clips = torch.rand(args.batch, 3, args.seq_len, args.img_dim, args.img_dim, generator=g).cuda()
    target = torch.randint(0, 101, (args.batch,), generator=g).cuda()
    inner = opt.step
    host = [0.0]

    def timed_step(closure=None):
        t = time.perf_counter()
        inner()
        host[0] += time.perf_counter() - t
    opt.step = timed_step

    def step():
        return L.train_step(call, opt, crit, clips, target, torch.device("cuda"), args.seq_len, args.img_dim,
                            orc.calc_topk_accuracy)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    host[0] = 0.0
    n, t0 = 0, time.perf_counter()
    while True:
        loss = step()
        n += 1
        if n >= args.min_steps and time.perf_counter() - t0 >= args.window:
            break
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    native = type(opt).__module__ == "coclr_amd.optim" and opt._plan is not None
    print(json.dumps({"optim": args.optim, "leg": args.child, "native": native, "steps": n,
                      "ms_per_step": 1e3 * dt / n, "clips_per_s": args.batch * n / dt,
                      "host_ms_in_step": 1e3 * host[0] / n, "loss": loss, "batch": args.batch}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["native", "torch"])
    ap.add_argument("--optim", default="sgd")
    ap.add_argument("--optims", default="sgd,adam")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq_len", type=int, default=32)
    ap.add_argument("--img_dim", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--min_steps", type=int, default=10)
    ap.add_argument("--window", type=float, default=2.0)
    ap.add_argument("--timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = []
    for optim in args.optims.split(","):
        for r in range(args.rounds):
            for leg in (("native", "torch") if r % 2 == 0 else ("torch", "native")):
                env = dict(os.environ, COCLR_QUIET="1")
                if leg == "torch":
                    env.update(COCLR_PATCH_SGD="0", COCLR_PATCH_ADAM="0")
                cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--optim", optim,
                       "--batch", str(args.batch), "--seq_len", str(args.seq_len), "--img_dim", str(args.img_dim),
                       "--warmup", str(args.warmup), "--min_steps", str(args.min_steps),
                       "--window", str(args.window)]
                out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=args.timeout)
                if out.returncode != 0:
                    sys.stderr.write(out.stderr[-4000:])
                    raise SystemExit("leg %s/%s failed with exit status %d" % (optim, leg, out.returncode))
                row = json.loads(out.stdout.strip().splitlines()[-1])
                row["round"] = r
                rows.append(row)
                print(json.dumps(row), flush=True)
    summary = {}
    for optim in args.optims.split(","):
        for leg in ("native", "torch"):
            sel = [r for r in rows if r["optim"] == optim and r["leg"] == leg]
            summary["%s_%s" % (optim, leg)] = {
                k: sorted(r[k] for r in sel)[len(sel) // 2] for k in ("ms_per_step", "clips_per_s", "host_ms_in_step")}
    print(json.dumps({"median": summary}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"rows": rows, "median": summary, "batch": args.batch, "clip": [3, args.seq_len, args.img_dim,
                                                                                    args.img_dim]}, f, indent=1)


if __name__ == "__main__":
    main()
