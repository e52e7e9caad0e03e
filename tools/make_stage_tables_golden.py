"""Writes tests/golden/stage_tables.pt: what the HOST side of the staging and of the JPEG path returns -- descriptor
rows, axis tables, program tables, concatenated packs, checked geometry, decode stages -- for the batches the CPU and the
GPU tier share, so that a change of that host code is held to the bytes it returned before.

    python tools/make_stage_tables_golden.py        # run on the commit whose results are to be kept

Public names of coclr_amd.staging, coclr_amd.jpeg and coclr_amd.ops only; the batches are those of tests/train_harness.py,
tests/ragged_harness.py, tests/_jpeg_cases.py and the MIXED list of tests/test_ragged_cpu.py.
tests/test_stage_tables_cpu.py calls `entries()` again and compares every element.  A tensor of more than KEEP elements
is recorded as its shape, dtype and the SHA-256 of its bytes, which keeps the file the size of its neighbours; a call
that refuses is recorded as the name of its exception."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

import _jpeg_cases as J                     # noqa: E402
import ragged_harness as RH                 # noqa: E402
import train_harness as TH                  # noqa: E402
from coclr_amd import jpeg, ops, staging    # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "stage_tables.pt")
MIXED = ("16x16_444_q50_ramp", "56x40_420_rst1", "17x33_gray_q50_ramp", "45x37_420_q100_noise")
ONE_SIZE = (40, 56, 3, (2, 2))
KEEP = 64


def freeze(x):
    """A result as plain data: tuples and lists as lists, small tensors as they are, large ones as a digest."""
    if torch.is_tensor(x):
        x = x.contiguous()
        if x.numel() <= KEEP:
            return x.clone()
        return {"shape": tuple(x.shape), "dtype": str(x.dtype), "sha256": hashlib.sha256(x.numpy().tobytes()).hexdigest()}
    if isinstance(x, (tuple, list)):
        return [freeze(v) for v in x]
    assert isinstance(x, (bool, int, str)), type(x)
    return x


def attempt(fn, *args):
    try:
        return freeze(fn(*args))
    except ValueError as e:
        return "raises " + type(e).__name__


def samples_of(frames, n):
    """[(byte offset, W, H)] of samples of n frames each, from the container's own tables."""
    return [(int(frames.offset[f]), int(frames.width[f]), int(frames.height[f])) for f in range(0, len(frames), n)]


def entries():
    out = {}
    # the training transform: the recorded runs as one one-size batch, then the mixed batch
    gold = TH.golden()
    S, T = gold["img_dim"], gold["seq_len"]
    runs = TH.fixture_plans(gold)
    H, W = runs[0][0]["frames"].shape[1:3]
    plans = [plan for _, plan, _ in runs]
    out["train_tables"] = freeze(staging.train_tables(plans, len(plans), T, W, H, S))
    batch, S, T = RH.train_batch()
    frames = staging.ragged_from_frames([f for f, _ in batch], device="cpu")
    plans = [p for _, p in batch]
    out["train_tables_ragged"] = freeze(staging.train_tables_ragged(plans, samples_of(frames, 2 * T), T, S))
    flat = [list(p) for plan in plans for progs in plan["programs"] for p in progs]
    out["augment_tables/train"] = freeze(staging.augment_tables(flat))
    out["program_tables/train"] = freeze(staging.program_tables([[op for op in p if op[0] < 6] for p in flat]))
    # the classifier's transform: every img_dim group as one ragged batch, and each run of one frame size on its own
    size, T = RH.CL.golden()["size"], RH.CL.golden()["seq_len"]
    for img_dim, group in sorted(RH.cls_batches().items()):
        frames = staging.ragged_from_frames([run["frames"] for run, _ in group], device="cpu")
        plans = [plan for _, plan in group]
        shapes = [tuple(run["frames"].shape[1:3]) for run, _ in group]
        for flip in (False, True):
            key = "%d/flip%d" % (img_dim, flip)
            out["classifier_tables_ragged/" + key] = freeze(
                staging.classifier_tables_ragged(plans, samples_of(frames, T), T, img_dim, size, flip))
            for H, W in sorted(set(shapes)):
                own = [p for p, s in zip(plans, shapes) if s == (H, W)]
                out["classifier_tables/%s/%dx%d" % (key, H, W)] = freeze(
                    staging.classifier_tables(own, len(own), T, W, H, img_dim, size, flip))
        programs = [list(plan["program"]) for plan in plans]
        out["program_tables/cls%d" % img_dim] = freeze(staging.program_tables(programs))
        out["augment_tables/cls%d" % img_dim] = freeze(staging.augment_tables(programs))
    # the JPEG host path: packs of one geometry, then the mixed list
    for name, cases in (("one_size", J.groups()[ONE_SIZE]), ("mixed", [J.case(n) for n in MIXED])):
        packs = [jpeg.pack([J.raw(c)]) for c in cases]
        data, meta = jpeg.cat_ragged(packs)
        out["cat/" + name] = attempt(jpeg.cat, packs)
        out["cat_ragged/" + name] = freeze((data, meta))
        out["check_meta/" + name] = attempt(jpeg.check_meta, data, meta)
        out["check_meta_ragged/" + name] = attempt(jpeg.check_meta_ragged, data, meta)
    geo = jpeg.check_meta_ragged(data, meta)
    nb = [ops.jpeg_workspace(*g)[1] // 64 for g in geo.tolist()]
    out["ragged_plan/256MiB"] = freeze(jpeg.ragged_plan(geo, 256 << 20))
    out["ragged_plan/two_stages"] = freeze(jpeg.ragged_plan(geo, (nb[0] + nb[1]) * 192))
    return out


def main():
    torch.save(entries(), OUT)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) <= 100000


if __name__ == "__main__":
    main()
