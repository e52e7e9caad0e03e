"""One loader batch decoded by index from a device-resident store (coclr_amd/jpeg.py: class Store) against the path a
batch takes without one, on one MI355X.

    python tools/jpeg_store_step.py [--frames 2048] [--rounds 3] [--legs parent,64,128,256,host]
                                    [--out profiles/jpeg_store.json]

The batch is that of tools/jpeg_decode_step.py: --frames copies of the 320 x 240, 4:2:0, quality-75 frame of
tests/golden/jpeg_frames.pt, as 64 packs (videos) of 32 frames.  The legs:
  parent   what a step does without a store: jpeg.cat of the packs, upload, jpeg.decode at chunk_bytes = 64 (the
           default of COCLR_JPEG_SPLIT).  This is the baseline; it is never the new code.
  n        a Store built once with chunk_bytes = n, then store.decode(ids) per step, the videos in a seeded order.
  host     the same with Store(bytes_on="host") at chunk_bytes = 64: bytes and rows in pinned host memory, every step's
           frames gathered to the device arena first (coclr_jpeg_store_gather).  Its baselines are `parent` and `64`.
Every round runs every leg once, each in a fresh child process, so the legs alternate within one command and drift of
the machine hits them alike.  A child does warm-up decodes, asserts that EVERY frame equals the fixture's `rgb`, then
--reps timed repetitions and reports, as medians over them, the milliseconds of
  entropy   the entropy stage alone (stages = 1) between device events, on the frames of the first stage of the
            default budget, scaled to the batch
  decode    the whole call between device events (the parent's cat and upload included: they are in its step)
  host      wall time until the call returns, without waiting for the device
and for a store leg `add`, the one-off cost per frame of building the store (host and device, synchronised at the
end).  The host leg adds `gather`, the gather launch alone between device events, `bus_bytes`, what it copies (hulls
and rows), and `save` / `load`, the milliseconds per frame of Store.save to a temporary directory and of Store.load
from it as a host store, to be held against `add`.  The parent reports per leg the rows, their medians and the spread (largest minus smallest) between rounds, and
applies the rule for Store's default chunk size: the store leg with the lowest median `decode`, if it is below every
other store leg by more than the spread between rounds of either; otherwise 64.  One frame copied --frames times, one
geometry: PROVISIONAL, as COCLR_JPEG_SPLIT's default is.  `--child` runs one leg of one round."""
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

    rows = {k: [] for k in ("entropy", "decode", "host")}
    res = {"leg": args.leg, "frames": args.frames}
    if args.leg == "parent":
        out = torch.empty(args.frames, H, W, 3, dtype=torch.uint8, device=dev)

        def step():
            data, meta = jpeg.cat(packs)
            return jpeg.decode(data, meta, out=out, chunk_bytes=64)

        for _ in range(args.warmup):
            step()
        assert bool((out == want).all()) and not jpeg.decode.last_status.any()
        data, meta = jpeg.cat(packs)
        geo = jpeg.check_meta(data, meta)
        cb, pb = ops.jpeg_workspace(*geo)
        n = max(1, min(args.frames, (256 << 20) // (cb + pb)))
        host = meta[:n, 8:].contiguous()
        d_data, d_meta = data.to(dev), host.to(dev)
        coefs = torch.empty(n * cb // 2, dtype=torch.int16, device=dev)
        planes = torch.empty(n * pb, dtype=torch.uint8, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        entropy = lambda: ops.jpeg_decode(d_data, d_meta, host, *geo, coefs, planes, out[:n], status, stages=1,   # noqa: E731
                                          chunk_bytes=64)
        check = lambda: bool((out == want).all()) and not jpeg.decode.last_status.any()      # noqa: E731
        res["compressed_bytes"] = data.numel()
    else:
        on_host = args.leg == "host"
        chunk = 64 if on_host else int(args.leg)
        nbytes = sum(d.numel() for d, _ in packs)
        store = jpeg.Store(nbytes, args.frames, chunk_bytes=chunk, bytes_on="host" if on_host else "device")
        torch.cuda.synchronize()
        t = time.perf_counter()
        first = [store.add(p) for p in packs]
        torch.cuda.synchronize()
        res["add"] = 1e3 * (time.perf_counter() - t) / args.frames
        order = random.Random(1).sample(range(videos), videos)
        ids = torch.tensor([first[v] + i for v in order for i in range(CLIP)])
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
        d_sel, d_geom, d_prefix = sel[k:e].to(dev), geom.to(dev), prefix.to(dev)
        buffers = store._buffers
        if on_host:                                            # the entropy stage runs on the arena's frames
            plan = store.gather_plan(sel)
            d_plan = torch.cat([plan[0].reshape(-1), plan[2].reshape(-1)]).to(dev)
            gather = lambda: store._gather(plan, d_plan)       # noqa: E731
            view = gather()
            buffers = lambda: view                             # noqa: E731
            sel = torch.arange(args.frames)
            d_sel = sel[k:e].to(dev)
            rows["gather"] = []
            res["bus_bytes"] = plan[3] + 16 * plan[4]
            import tempfile
            with tempfile.TemporaryDirectory() as tmp:
                t = time.perf_counter()
                store.save(tmp)
                res["save"] = 1e3 * (time.perf_counter() - t) / args.frames
                t = time.perf_counter()
                loaded = jpeg.Store.load(tmp, bytes_on="host")
                torch.cuda.synchronize()
                res["load"] = 1e3 * (time.perf_counter() - t) / args.frames
            assert len(loaded) == args.frames and torch.equal(loaded._rows[:loaded.chunk_rows],
                                                              store._rows[:store.chunk_rows])
            del loaded
        pixels = state["frames"].pixels
        coefs = torch.empty(blocks * 64, dtype=torch.int16, device=dev)
        planes = torch.empty(blocks * 64, dtype=torch.uint8, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        entropy = lambda: ops.jpeg_decode_store(buffers(), d_sel, sel[k:e].contiguous(), d_geom, geom, d_prefix,   # noqa: E731
                                                prefix, coefs, planes, pixels, status, stages=1)
        res.update(compressed_bytes=store.nbytes, chunk_rows=store.chunk_rows, table_sets=store.table_sets)
    for _ in range(args.reps):
        if "gather" in rows:
            rows["gather"].append(timed(gather)[0])
        ms, _, _ = timed(entropy)
        rows["entropy"].append(ms * args.frames / n)
        ms, host_ms, _ = timed(step)
        rows["decode"].append(ms)
        rows["host"].append(host_ms)
    assert check()
    res.update({k: median(v) for k, v in rows.items()}, stage_frames=n)
    print(json.dumps(res))


def choose_default(legs):
    """The rule of the module docstring over {leg: {"median", "spread"}} -> (chunk size, the reason)."""
    sizes = [c for c in legs if c.isdigit()]
    if len(sizes) < 2:
        return 64, "needs two store legs"
    best = min(sizes, key=lambda c: legs[c]["median"]["decode"])
    for c in sizes:
        gain = legs[c]["median"]["decode"] - legs[best]["median"]["decode"]
        spread = max(legs[c]["spread"]["decode"], legs[best]["spread"]["decode"])
        if c != best and gain <= spread:
            return 64, "%s bytes is lowest, but only %.3f ms below %s bytes with %.3f ms between rounds" % (
                best, gain, c, spread)
    return int(best), "decode at %s bytes is below every other store leg by more than the spread between rounds" % best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--leg", default="parent")
    ap.add_argument("--legs", default="parent,64,128,256,host")
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
    legs = args.legs.split(",")
    rows = {c: [] for c in legs}
    for r in range(args.rounds):
        for c in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--leg", c, "--frames", str(args.frames),
                   "--warmup", str(args.warmup), "--reps", str(args.reps)]
            out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.timeout)
            if out.returncode != 0:
                sys.stderr.write(out.stderr[-4000:])
                raise SystemExit("round %d, leg %s failed with exit status %d" % (r, c, out.returncode))
            rows[c].append(json.loads(out.stdout.strip().splitlines()[-1]))
            print(json.dumps(rows[c][-1]), flush=True)
    keys = ("entropy", "decode", "host")
    extra = {"parent": (), "host": ("gather", "add", "save", "load", "bus_bytes")}
    table = {}
    for c in legs:
        table[c] = {"rows": rows[c],
                    "median": {k: median([r[k] for r in rows[c]]) for k in keys + extra.get(c, ("add",))},
                    "spread": {k: max(r[k] for r in rows[c]) - min(r[k] for r in rows[c])
                               for k in keys + extra.get(c, ())[:1]}}
    chosen, why = choose_default(table)
    result = {"case": CASE, "frames": args.frames, "legs": table, "default": {"chunk_bytes": chosen, "why": why},
              "units": "ms per batch of `frames` frames; `add` ms per frame, once",
              "note": "one frame copied `frames` times, one geometry; a training step with the decode in the loop is "
                      "not measured here"}
    if "host" in table and "parent" in table:
        # the host store is recommended for a dataset that does not fit the device only if it beats the route such a
        # dataset takes today by more than the rounds differ
        gain = table["parent"]["median"]["decode"] - table["host"]["median"]["decode"]
        spread = max(table["parent"]["spread"]["decode"], table["host"]["spread"]["decode"])
        result["host_store"] = {"recommended": gain > spread, "gain_ms": gain, "spread_ms": spread,
                                "note": "PROVISIONAL: one geometry, one frame copied, no training step in the loop"}
    print(json.dumps({"median": {c: table[c]["median"] for c in legs}, "spread": {c: table[c]["spread"] for c in legs},
                      "default": result["default"], "host_store": result.get("host_store")}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
