"""The case table of the exact segmented-accumulate tests (tests/_segment_cases.py) reaches every branch the launcher of
coclr_segment_softmax_accum / coclr_segment_accum has (coclr_amd/csrc/retrieval.hip, segment_accum<>), its restated host
predicates are the library's, and the references the GPU tests rely on are right -- without a GPU.

The launcher decides four things on the host: whether a call is refused, the 16-byte or the scalar form (C % 4, the bases
of x and out), how often a thread goes round the column loop, and which segments share a launch (64 at most, no output
row twice).  Deleting a row that was the only one on a branch fails here, naming the branch.  The validation runs before
any launch and needs no device: the table's shapes go through the raw entry points in a child process that sees no
device, where an accepted call ends in hipErrorNoDevice and a refused one in COCLR_EINVAL."""
import json
import os
import re
import subprocess
import sys

import torch

import _segment_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BRANCHES = [
    ("16-byte form", lambda r, b: b["vec"]),
    ("scalar form", lambda r, b: not b["vec"]),
    ("scalar form because of C % 4 alone", lambda r, b: b["scalar_why"] == {"C % 4"}),
    ("scalar form because of the base of x alone", lambda r, b: b["scalar_why"] == {"x base"}),
    ("scalar form because of the base of out alone", lambda r, b: b["scalar_why"] == {"out base"}),
    ("scalar form because of both bases", lambda r, b: b["scalar_why"] == {"x base", "out base"}),
    ("one pass, 16-byte form", lambda r, b: b["vec"] and b["passes"] == 1),
    ("one pass, scalar form", lambda r, b: not b["vec"] and b["passes"] == 1),
    ("two passes, 16-byte form", lambda r, b: b["vec"] and b["passes"] == 2),
    ("two passes, scalar form", lambda r, b: not b["vec"] and b["passes"] == 2),
    ("four passes or more, 16-byte form", lambda r, b: b["vec"] and b["passes"] >= 4),
    ("four passes or more, scalar form", lambda r, b: not b["vec"] and b["passes"] >= 4),
    ("exactly one full pass (tail 0)", lambda r, b: b["tail"] == 0 and b["passes"] == 1),
    ("full passes only, several (tail 0)", lambda r, b: b["tail"] == 0 and b["passes"] > 1),
    ("a partly filled last pass above 256 units", lambda r, b: b["tail"] != 0 and b["passes"] > 1),
    ("a last pass of one unit", lambda r, b: b["tail"] == 1 and b["passes"] > 1),
    ("idle waves: two", lambda r, b: b["idle_waves"] == 2),
    ("idle waves: three", lambda r, b: b["idle_waves"] == 3),
    ("only lane 0 works, 16-byte form (C = 4)", lambda r, b: b["vec"] and b["CV"] == 1),
    ("only lane 0 works, scalar form (C = 1)", lambda r, b: not b["vec"] and b["CV"] == 1),
    ("the widest row, 32 KiB of LDS", lambda r, b: r.C == S.MAX_C and b["lds_bytes"] == 32768),
    ("one launch", lambda r, b: len(b["launches"]) == 1),
    ("one launch of 64 segments", lambda r, b: [len(l) for l in b["launches"]] == [64]),
    ("one segment", lambda r, b: b["launches"] == [[0]]),
    ("two launches", lambda r, b: len(b["launches"]) == 2),
    ("three launches", lambda r, b: len(b["launches"]) == 3),
    ("cut because the block is full, alone", lambda r, b: {"full"} in b["cuts"]),
    ("cut because of the same output row, alone", lambda r, b: {"same row"} in b["cuts"]),
    ("cut for both reasons at once", lambda r, b: {"full", "same row"} in b["cuts"]),
    ("the same output row in adjacent segments", lambda r, b: any(
        r.segs[s][2] == r.segs[s + 1][2] for s in range(len(r.segs) - 1))),
    ("the same output row ten segments later", lambda r, b: any(
        r.segs[s][2] == r.segs[s + 10][2] for s in range(len(r.segs) - 10))),
    ("one output row named three times", lambda r, b: max(
        [o for _, _, o in r.segs].count(o) for _, _, o in r.segs) == 3),
    ("a segment ending on row R - 1", lambda r, b: any(f + n == r.R for f, n, _ in r.segs)),
    ("output row V - 1", lambda r, b: any(o == r.V - 1 for _, _, o in r.segs)),
    ("the first segment starts past row 0", lambda r, b: r.segs[0][0] > 0),
    ("segments out of row order", lambda r, b: any(
        r.segs[s + 1][0] < r.segs[s][0] for s in range(len(r.segs) - 1))),
    ("two segments read the same rows into different output rows", lambda r, b: any(
        a[:2] == c[:2] and a[2] != c[2] for i, a in enumerate(r.segs) for c in r.segs[i + 1:])),
    ("an output row named by no segment", lambda r, b: bool(S.unnamed_outputs(r))),
    ("a row of x in no segment", lambda r, b: bool(S.unread_rows(r))),
    ("a segment of one row", lambda r, b: any(n == 1 for _, n, _ in r.segs)),
    ("a segment of 64 rows", lambda r, b: any(n == 64 for _, n, _ in r.segs)),
    ("weight 1 / rows", lambda r, b: any(w == 1.0 / n and n > 1 for (_, n, _), w in zip(r.segs, r.weights))),
    ("weight 0", lambda r, b: 0.0 in r.weights),
    ("a negative weight", lambda r, b: any(w < 0 for w in r.weights)),
]


def _reached(cases):
    table = [(r, S.branches(r)) for r in cases]
    return {name: [r.name for r, b in table if hit(r, b)] for name, hit in BRANCHES}


def test_names_are_unique_and_the_table_is_what_it_says():
    names = [c.name for c in S.CASES]
    assert len(set(names)) == len(names)
    assert {c.C for c in S.of("width") if S.branches(c)["vec"]} == set(S.VEC_WIDTHS) == {4, 252, 256, 1024, 1028, 2048,
                                                                                       4092, 4096}
    assert {c.C for c in S.of("width") if not S.branches(c)["vec"]} == set(S.SCALAR_WIDTHS) == {1, 3, 63, 65, 255, 257,
                                                                                              513, 4093}
    for C in (8, 1028):
        aligned, shifted = S.twins(C, "rand3")
        assert S.branches(aligned)["vec"] and aligned.C % 4 == 0
        assert sorted((c.x_shift, c.out_shift) for c in shifted) == [(0, 2), (1, 0), (1, 2)]
        assert all(not S.branches(c)["vec"] and c.segs == aligned.segs for c in shifted)
    for C in (12, 257):
        part = {c.name.split("-", 2)[2].rsplit("-", 1)[0]: S.branches(c) for c in S.of("partition", "sum") if c.C == C}
        assert [len(l) for l in part["s64"]["launches"]] == [64]
        assert [len(l) for l in part["s65"]["launches"]] == [64, 1]
        assert [len(l) for l in part["s129"]["launches"]] == [64, 64, 1]
        assert part["dup-adjacent"]["launches"] == [[0, 1], [2, 3, 4, 5]]
        assert part["dup-ten-later"]["launches"] == [list(range(12)), [12, 13]]
        assert part["triple"]["launches"] == [[0, 1], [2, 3], [4, 5]]
        assert part["dup-as-65th"]["launches"] == [list(range(64)), [64, 65]]
        assert part["dup-as-65th"]["cuts"] == [{"full", "same row"}]
        assert part["s1"]["launches"] == [[0]]
    assert all(c.R <= 200 and c.V <= 140 and c.C <= S.MAX_C for c in S.CASES)
    assert all(n <= 64 for c in S.CASES for _, n, _ in c.segs)
    assert all(S.accepted(c.R, c.C, len(c.segs), c.V, c.segs) and len(c.weights) == len(c.segs) for c in S.CASES)
    # both kernels get every shape: an exact class and a random one each
    shapes = {}
    for c in S.CASES:
        shapes.setdefault((c.C, c.x_shift, c.out_shift, c.R, c.V, c.segs), set()).add(c.cls)
    assert all({"sum", "softmax", "rand3"} <= v for v in shapes.values())
    assert {c.cls for c in S.of("width")} == {c.cls for c in S.of("geometry")} == set(S.EXACT + S.RANDOM)


def test_rows_reach_every_branch(capsys):
    """Per class of data, since each class is one kernel's exact test (or both kernels' bounded one)."""
    for cls in ("sum", "softmax", "rand3"):
        reached = _reached(S.of(cls=cls))
        for name, _ in BRANCHES:
            if cls == "rand3" and name in ("weight 0", "a negative weight"):
                continue                               # the random class carries the evaluator's weights only
            assert reached[name], "no %s row reaches: %s" % (cls, name)
    reached = _reached(S.CASES)
    with capsys.disabled():
        print()
        print("segmented accumulate: %d rows (%s)" % (len(S.CASES), ", ".join(
            "%s %d" % (cls, len(S.of(cls=cls))) for cls in S.EXACT + S.RANDOM)))
        for name, _ in BRANCHES:
            print("  %-58s %3d rows, e.g. %s" % (name, len(reached[name]), reached[name][0]))


def test_removing_a_row_names_its_branch():
    """The coverage test is not vacuous: without the only rows on a branch, that branch comes up empty."""
    for gone, branch in ((("dup-as-65th",), "cut for both reasons at once"), (("s129", "triple"), "three launches"),
                         (("width-C1-",), "only lane 0 works, scalar form (C = 1)"),
                         (("x0-out2",), "scalar form because of the base of out alone"),
                         (("width-C4096",), "the widest row, 32 KiB of LDS"), (("width-C65-",), "idle waves: two")):
        kept = [c for c in S.of(cls="sum") if not any(g in c.name for g in gone)]
        assert len(kept) < len(S.of(cls="sum")) and _reached(S.of(cls="sum"))[branch]
        assert not _reached(kept)[branch], branch


def test_constants_are_the_librarys():
    from coclr_amd import ops
    assert S.MAX_C == ops.SEGMENT_MAX_C == 4096
    hip = open(os.path.join(ROOT, "coclr_amd", "csrc", "retrieval.hip")).read()
    assert int(re.search(r"#define\s+COCLR_SEG_MAX\s+(\d+)", hip).group(1)) == S.SEG_MAX == 64
    assert int(re.search(r"#define\s+COCLR_SEG_MAX_C\s+(\d+)", hip).group(1)) == S.MAX_C
    assert re.search(r"__launch_bounds__\(256\)\s*segment_accum_kernel", hip) and S.THREADS == 256
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "coclr_hip.h")).read())
    assert "1 <= C <= %d" % S.MAX_C in header[header.index("Video-level scores"):header.index("coclr_segment_accum(")]


_CHILD = r"""
import ctypes as C, json, sys
import _segment_cases as S
from coclr_amd import _lib
lib = _lib.load()
n = C.c_int(-1)
err = C.CDLL("libamdhip64.so").hipGetDeviceCount(C.byref(n))
if err == 0 and n.value > 0:
    print(json.dumps({"devices": n.value}))          # a device is visible: nothing may be launched at dummy addresses
    sys.exit(0)
x = C.c_void_p(4096)
out = {}
seen = set()
for c in S.CASES:
    key = (c.R, c.C, c.V, c.segs)
    if key in seen:
        continue
    seen.add(key)
    arr = (C.c_int32 * (3 * len(c.segs)))(*[v for sg in c.segs for v in sg])
    w = (C.c_float * len(c.segs))(*c.weights)
    end, top = max(f + k for f, k, _ in c.segs), max(o for _, _, o in c.segs)
    codes = []
    for fn in (lib.coclr_segment_softmax_accum, lib.coclr_segment_accum):
        call = lambda R, C_, V: fn(x, arr, w, x, R, C_, len(c.segs), V, None)
        codes.append({"row": call(c.R, c.C, c.V), "tight": call(end, c.C, top + 1), "R": call(end - 1, c.C, c.V),
                      "V": call(c.R, c.C, top), "C0": call(c.R, 0, c.V), "Cmax": call(c.R, S.MAX_C + 1, c.V),
                      "S0": fn(x, arr, w, x, c.R, c.C, 0, c.V, None)})
    out[c.name] = codes
print(json.dumps({"devices": 0, "codes": out}))
"""


def test_the_restated_validation_is_the_librarys():
    """Every shape of the table through both raw entry points with dummy addresses, in a child process that is shown no
    device: what `accepted` accepts gets as far as the launch (hipErrorNoDevice, 100), and the same call with R one
    short of the furthest segment, V equal to the highest output row, C = 0, C = 4097 or S = 0 is COCLR_EINVAL."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + sys.path))
    res = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    assert got["devices"] == 0, "the child process saw a device and launched nothing"
    assert len(got["codes"]) == len({(c.R, c.C, c.V, c.segs) for c in S.CASES})
    for name, codes in got["codes"].items():
        c = S.BY_NAME[name]
        end, top = max(f + k for f, k, _ in c.segs), max(o for _, _, o in c.segs)
        assert S.accepted(end, c.C, len(c.segs), top + 1, c.segs)
        assert not S.accepted(end - 1, c.C, len(c.segs), c.V, c.segs)
        assert not S.accepted(c.R, c.C, len(c.segs), top, c.segs)
        assert not S.accepted(c.R, 0, len(c.segs), c.V, c.segs) and not S.accepted(c.R, S.MAX_C + 1, 1, c.V, c.segs)
        assert not S.accepted(c.R, c.C, 0, c.V, c.segs)
        for k in codes:
            assert k["row"] == k["tight"] == 100, (name, k)       # hipErrorNoDevice: validated, then the launch
            assert k["R"] == k["V"] == k["C0"] == k["Cmax"] == k["S0"] == 1, (name, k)


# ---- references -------------------------------------------------------------------------------------------------------------

def test_exact_rows_are_exact():
    """Every value a kernel can hold on an exact row -- the table after each segment -- is an fp32 value, whichever way
    `o += w * acc` is rounded: a sum row stays in whole units of the smallest weight below 2^24 of them."""
    for c in S.of(cls="sum") + S.of(cls="softmax"):
        x, prior = S.inputs(c)
        assert all(w == 0 or abs(w) >= S.SMALLEST_WEIGHT and float(torch.tensor(abs(w)).log2()) % 1 == 0
                   for w in c.weights), c.name
        units = prior / S.SMALLEST_WEIGHT
        assert torch.equal(units, units.round()) and float(units.abs().max()) <= 32
        if c.cls == "sum":
            assert torch.equal(x, x.round()) and float(x.abs().max()) <= 8
            for first, rows, _ in c.segs:
                assert float(x[first:first + rows].abs().sum(0).max()) < 2 ** 10      # every partial sum
        steps = list(S.exact_steps(c))
        for t in steps:
            assert torch.equal(t.float().double(), t), c.name
            assert torch.equal(t / 2.0 ** -9, (t / 2.0 ** -9).round()) and float(t.abs().max()) < 2 ** 14
        assert torch.equal(steps[-1], S.reference(c, c.cls == "softmax"))
        for o in S.unnamed_outputs(c):
            assert torch.equal(steps[-1][o], prior[o])


def test_softmax_rows_put_the_maximum_where_a_reduction_can_miss_it():
    for c in S.of(cls="softmax"):
        b = S.branches(c)
        x, _ = S.inputs(c)
        hit, ks, last = set(), set(), False
        for r in sorted(set(range(c.R)) - set(S.unread_rows(c))):
            cols = S.max_columns(c, r)
            v = S.ROW_MAXIMA[r % len(S.ROW_MAXIMA)]
            assert len(set(cols)) == len(cols) in (1, 2, 4, 8) and 0 <= min(cols) and max(cols) < c.C
            assert len({S.owner(c, col) for col in cols}) == 1             # one wave of one pass holds them all
            mask = torch.zeros(c.C, dtype=torch.bool)
            mask[cols] = True
            assert bool((x[r][mask] == v).all()) and (c.C == len(cols) or float(x[r][~mask].max()) <= v - 200)
            hit.add(S.owner(c, cols[0]))
            ks.add(len(cols))
            last |= cols == [c.C - 1]
        if c.group in ("width", "base"):
            waves = 4 - b["idle_waves"]
            assert {w for _, w in hit} == set(range(waves)), c.name
            assert {p for p, _ in hit} == {0, min(1, b["passes"] - 1), b["passes"] - 1}, c.name
            assert last and S.owner(c, c.C - 1)[0] == b["passes"] - 1, c.name
            assert ks == {k for k in (1, 2, 4, 8) if k <= c.C}, c.name
    every = torch.cat([S.inputs(c)[0].reshape(-1) for c in S.of("width", "softmax")])
    assert bool((every == -S.INF).any()) and {87.0, -1000.0, 3.0e4} <= set(S.ROW_MAXIMA)


def test_references_are_the_per_video_expression():
    """softmax(x[first:first + rows].double(), -1).sum(0) * w added into the prior, segments in list order.  On the
    exact softmax rows the closed form (1/k and 0, no exponential) differs from it by the exp(-200) a float64 softmax
    keeps: below 1e-80, and nothing once rounded to fp32."""
    for c in S.CASES:
        x, prior = S.inputs(c)
        for softmax in S.kernels_of(c):
            want = prior.clone()
            for (first, rows, o), w in zip(c.segs, c.weights):
                part = x[first:first + rows].double()
                want[o] += (torch.softmax(part, -1) if softmax else part).sum(0) * w
            ref = S.reference(c, softmax)
            if c.cls == "softmax":
                assert float((ref - want).abs().max()) < 1e-80 and torch.equal(ref.float(), want.float()), c.name
            else:
                assert torch.equal(ref, want), c.name
            assert ref.shape == (c.V, c.C) and bool(torch.isfinite(ref).all())


def test_the_random_bar_is_not_tuned_to_the_kernels(capsys):
    """The bar of the random rows is the project's 1e-6 of the largest reference element (tests/_cases.check_close).  A
    plain fp32 restatement -- F.softmax in fp32, rows added in ascending order, times the weight -- stays at or below
    5e-7 on every random row, so an fp32 kernel that sums in this order has the room it needs and no more than twice."""
    worst = {True: (0.0, None), False: (0.0, None)}
    for c in S.of(cls="rand3") + S.of(cls="rand30"):
        assert all(w == 1.0 / n for (_, n, _), w in zip(c.segs, c.weights))
        for softmax in (True, False):
            ref = S.reference(c, softmax)
            err = float((S.restated_fp32(c, softmax).double() - ref).abs().max() / ref.abs().max())
            assert err <= 5e-7, (c.name, softmax, err)
            worst[softmax] = max(worst[softmax], (err, c.name))
    with capsys.disabled():
        print()
        print("fp32 restatement against float64, largest error relative to the largest reference element (bar 1e-6): "
              "softmax sum %.2e (%s), plain sum %.2e (%s)" % (worst[True] + worst[False]))
