"""What the shard gather costs: one loader batch decoded from a jpeg.ShardedStore of two in-process device shards
against the same batch from ONE device Store, on one MI355X.

    python tools/jpeg_shard_step.py [--frames 2048] [--rounds 3] [--legs 64,host,shards] [--baseline-root DIR]
                                    [--out profiles/jpeg_shard.json]

The batch is that of tools/jpeg_store_step.py: --frames copies of the 320 x 240, 4:2:0, quality-75 frame of
tests/golden/jpeg_frames.pt, as 64 packs (videos) of 32 frames, the videos in a seeded order.  The legs:
  64       Store.decode on one device store at chunk_bytes = 64: the child of tools/jpeg_store_step.py.  With
           --baseline-root that tool is run from DIR, a built checkout of the commit BEFORE the sharded store, so the
           baseline is never the new code; without it, from this tree.
  host     the same tool's Store(bytes_on="host") leg, from the same place: the other route that gathers first.
  shards   this tree: the videos dealt alternately to two device Stores, jpeg.ShardedStore([a, b]).decode(ids).
Every round runs every leg once, each in a fresh child process, so the legs alternate within one command.  A child does
warm-up decodes, asserts that EVERY frame equals the fixture's `rgb`, then --reps timed repetitions and reports, as
medians over them, the milliseconds of `entropy`, `decode` and `host` as tools/jpeg_store_step.py defines them, and for
`shards` also `gather`, the gather launch alone between device events, `plan`, the host time of gather_plan, and
`copied_bytes`, what the launch copies (hulls and rows).  The parent reports medians over the rounds and the spread
(largest minus smallest).  One frame copied --frames times, one geometry, one table set: PROVISIONAL.  Both shards lie
in ONE device's memory: what a peer's memory over xGMI costs is unmeasured (no multi-GPU node).  `--child` runs the
`shards` leg of one round."""
import argparse
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "jpeg_frames.pt")
CASE = "320x240_420_q75"
CLIP = 32


def median(v):
    return sorted(v)[len(v) // 2]


def child(args):
    sys.path.insert(0, ROOT)
    import torch
    from coclr_amd import jpeg, ops
    c = next(c for c in torch.load(FIXTURE)["cases"] if c["name"] == CASE)
    raw, rgb = c["raw"].numpy().tobytes(), c["rgb"]
    videos = args.frames // CLIP
    packs = [jpeg.pack([raw] * CLIP) for _ in range(videos)]
    dev = torch.device("cuda")
    want = rgb.to(dev)[None]
    H, W = rgb.shape[:2]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t = time.perf_counter()
        r = fn()
        host = 1e3 * (time.perf_counter() - t)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), host, r

    nbytes = sum(d.numel() for d, _ in packs)
    shards = [jpeg.Store(nbytes, args.frames, chunk_bytes=64) for _ in range(2)]
    first = [shards[v % 2].add(p) for v, p in enumerate(packs)]
    store = jpeg.ShardedStore(shards)
    order = random.Random(1).sample(range(videos), videos)
    ids = torch.tensor([int(store.bases[v % 2]) + first[v] + i for v in order for i in range(CLIP)])
    state = {}

    def step():
        state["frames"] = store.decode(ids)
        return state["frames"]

    for _ in range(args.warmup):
        step()
    check = lambda: bool((state["frames"].pixels.view(args.frames, H, W, 3) == want).all()) and \
        not store.decode.last_status.any()                                                # noqa: E731
    assert check()
    sel, geo, offset, total, stages, blocks = store.plan(ids)
    k, e, geom, prefix = stages[0]
    n = e - k
    plan = store.gather_plan(sel)
    d_plan = torch.cat([plan[0].reshape(-1), plan[2].reshape(-1), plan[5]]).to(dev)
    gather = lambda: store._gather(plan, d_plan)               # noqa: E731
    view = gather()
    sel = torch.arange(args.frames)
    d_sel, d_geom, d_prefix = sel[k:e].to(dev), geom.to(dev), prefix.to(dev)
    pixels = state["frames"].pixels
    coefs = torch.empty(blocks * 64, dtype=torch.int16, device=dev)
    planes = torch.empty(blocks * 64, dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    entropy = lambda: ops.jpeg_decode_store(view, d_sel, sel[k:e].contiguous(), d_geom, geom, d_prefix, prefix,   # noqa: E731
                                            coefs, planes, pixels, status, stages=1)
    rows = {k: [] for k in ("entropy", "decode", "host", "gather", "plan")}
    for _ in range(args.reps):
        rows["gather"].append(timed(gather)[0])
        rows["entropy"].append(timed(entropy)[0] * args.frames / n)
        ms, host_ms, _ = timed(step)
        rows["decode"].append(ms)
        rows["host"].append(host_ms)
        t = time.perf_counter()
        store.gather_plan(ids)
        rows["plan"].append(1e3 * (time.perf_counter() - t))
    assert check()
    res = {"leg": "shards", "frames": args.frames, "shards": 2, "copied_bytes": plan[3] + 16 * plan[4],
           "compressed_bytes": store.nbytes, "table_sets": store.table_sets, "stage_frames": n}
    res.update({k: median(v) for k, v in rows.items()})
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--legs", default="64,host,shards")
    ap.add_argument("--baseline-root", default=None)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.frames < CLIP or args.frames % CLIP:
        raise SystemExit("--frames is a multiple of %d" % CLIP)
    if args.child:
        return child(args)
    base = os.path.abspath(args.baseline_root) if args.baseline_root else ROOT
    legs = args.legs.split(",")
    rows = {c: [] for c in legs}
    common = ["--frames", str(args.frames), "--warmup", str(args.warmup), "--reps", str(args.reps)]
    for r in range(args.rounds):
        for c in legs:
            if c == "shards":
                cmd, cwd = [sys.executable, os.path.abspath(__file__), "--child"] + common, ROOT
            else:
                cmd, cwd = [sys.executable, os.path.join(base, "tools", "jpeg_store_step.py"), "--child", "--leg",
                            c] + common, base
            out = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=args.timeout)
            if out.returncode != 0:
                sys.stderr.write(out.stderr[-4000:])
                raise SystemExit("round %d, leg %s failed with exit status %d" % (r, c, out.returncode))
            rows[c].append(json.loads(out.stdout.strip().splitlines()[-1]))
            print(json.dumps(rows[c][-1]), flush=True)
    table = {}
    for c in legs:
        keys = [k for k, v in rows[c][0].items() if isinstance(v, float)]
        table[c] = {"rows": rows[c], "median": {k: median([r[k] for r in rows[c]]) for k in keys},
                    "spread": {k: max(r[k] for r in rows[c]) - min(r[k] for r in rows[c]) for k in keys}}
    result = {"case": CASE, "frames": args.frames, "legs": table,
              "baseline": "a checkout of the parent commit" if args.baseline_root else "this tree",
              "units": "ms per batch of `frames` frames",
              "note": "PROVISIONAL: one frame copied `frames` times, one geometry, one table set; both shards in one "
                      "device's memory; across peer GPUs unmeasured: no multi-GPU node"}
    if "shards" in table and "64" in table:
        result["overhead_ms"] = {k: table["shards"]["median"][k] - table["64"]["median"][k]
                                 for k in ("entropy", "decode", "host")}
    print(json.dumps({"median": {c: table[c]["median"] for c in legs}, "spread": {c: table[c]["spread"] for c in legs},
                      "overhead_ms": result.get("overhead_ms")}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
