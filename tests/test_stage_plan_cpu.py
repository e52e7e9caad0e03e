"""CPU tier for the staging dispatch: the plan queries of coclr_amd/csrc/staging.hip (coclr_stage_crops_plan,
coclr_stage_crops_ragged_plan, coclr_resize_boxes_plan, coclr_resize2_boxes_plan, coclr_stage_clips_plan,
coclr_jitter_plan: the structs the launchers themselves launch from, nothing launched) say what every row of
tests/_stage_cases.py reaches, and this module asserts that the table covers all fourteen kernel instantiations and
every edge in EDGES below, and that every row is the only cover of something.  tests/test_gpu_stage_exact.py runs the
same rows against the restatements bit for bit, so a row cannot be dropped or moved without this module failing.

Also here: the band bounds of the three resampling launchers against the real tables over a fixed sweep, the queries'
refusals, and the restatements the GPU tier uses as references against PIL itself on the rows' own inputs.
"""
import ctypes as C

import numpy as np
import pytest

import _stage_cases as SC
import crops_harness as CH
from coclr_amd import _lib, ops, staging


def _plan(row):
    try:
        return SC.plan(row)
    except _lib.HipLibraryError:
        return None


PLANS = [(r, _plan(r)) for r in SC.ALL]
RESIZE = [r for r in SC.CROPS + SC.BOXES + SC.TWOS if not r.refuse]


def test_rows_are_small():
    for r in SC.ALL:
        assert SC.row_bytes(r) <= SC.MAX_BYTES, r.name


def test_rows_reach_what_they_claim():
    for r, pl in PLANS:
        if getattr(r, "refuse", False):
            assert pl is None, r.name
            continue
        assert pl is not None, r.name
        for k, v in r.want.items():
            assert pl[k] == v, (r.name, k, pl)
        fam = SC.family(r)
        if fam in ("crop", "box"):
            S = r.S
            assert pl["bands"] == -(-S // pl["R"]) and pl["lds"] == pl["cap_rows"] * 3 * ((S + 3) & ~3), r.name
            assert pl["lds"] <= (32768 if pl["R"] > 1 else 65536), r.name
        if fam == "crop":
            assert pl["u8out"] == r.form.endswith("u8") and pl["ragged"] == r.form.startswith("rag"), r.name
            assert pl["vec"] == (not pl["u8out"] and r.S % 4 == 0 and r.out_off % 4 == 0), r.name
        if fam == "box":
            assert pl["u8out"] and pl["ragged"] == r.ragged and not pl["vec"], r.name
        if fam == "two":
            P, Sp = (r.size + 3) & ~3, (r.S + 3) & ~3
            h1, h2 = pl["cap1"] * 3 * P, pl["capA"] * 3 * Sp
            assert pl["one"] == ("h1" if h1 > h2 else "h2"), r.name
            assert pl["lds"] == max(h1, h2) + pl["capA"] * 3 * P and pl["optin"] == (pl["lds"] > 65536), r.name
            assert pl["lds"] <= (80 << 10 if pl["R"] > 1 else 160 << 10) and pl["bands"] == -(-r.S // pl["R"]), r.name
            assert pl["u8out"] == r.form.endswith("u8") and pl["ragged"] == r.form.startswith("rag"), r.name
            assert pl["vec"] == (not pl["u8out"] and r.S % 4 == 0), r.name
        if fam == "clips":
            per = 16 if r.u8 else 4
            assert pl["u8"] == r.u8 and pl["gx"] == min(max((r.thw // per + 255) // 256, 1), 64), r.name
            assert pl["vec"] == (r.thw % per == 0 and r.src_off == 0 and r.out_off == 0), r.name
        if fam == "prog":
            nt = 1024 if r.aug else 512
            items = (r.H * r.W + 3) // 4
            cuts = max(sum(k in (SC.CON, SC.BLUR) for k, _ in p) for p in r.programs)
            assert pl["aug"] == r.aug and pl["items"] == items and pl["per_lane"] == -(-items // nt), r.name
            assert pl["cuts"] == cuts and pl["use_lds"] == (cuts > 0) and pl["lds"] == (items * 12 if cuts else 0), r.name
            assert pl["vec"] == (r.W % 4 == 0), r.name


# ---- the fourteen instantiations ----------------------------------------------------------------------------------------

def instantiation(r, pl):
    fam = SC.family(r)
    if fam == "crop":
        return "stage_crops_kernel<U8OUT=%d, RAGGED=%d>" % (pl["u8out"], pl["ragged"])
    if fam == "box":
        return "resize_boxes_kernel<RAGGED=%d>" % pl["ragged"]
    if fam == "two":
        return "resize2_boxes_kernel<U8OUT=%d, RAGGED=%d>" % (pl["u8out"], pl["ragged"])
    if fam == "clips":
        return "stage_clips_kernel<U8=%d>" % pl["u8"]
    return "color_jitter_kernel<AUG=%d>" % pl["aug"]


INSTANTIATIONS = (["stage_crops_kernel<U8OUT=%d, RAGGED=%d>" % (u, g) for u in (0, 1) for g in (0, 1)] +
                  ["resize_boxes_kernel<RAGGED=%d>" % g for g in (0, 1)] +
                  ["resize2_boxes_kernel<U8OUT=%d, RAGGED=%d>" % (u, g) for u in (0, 1) for g in (0, 1)] +
                  ["stage_clips_kernel<U8=%d>" % u for u in (0, 1)] + ["color_jitter_kernel<AUG=%d>" % a for a in (0, 1)])
UNREACHABLE = {}        # instantiation or edge -> why no geometry can reach it; none turned out to be


def test_table_reaches_every_instantiation():
    assert len(INSTANTIATIONS) == 14
    got = {}
    for r, pl in PLANS:
        if pl is not None:
            got.setdefault(instantiation(r, pl), []).append(r.name)
    print()
    for k in INSTANTIATIONS:
        print("  %-48s %s" % (k, ", ".join(got.get(k, [])) or "-"))
    assert set(got) == set(INSTANTIATIONS) - set(UNREACHABLE)


# ---- the edges ------------------------------------------------------------------------------------------------------------

def _is(fam):
    return lambda r: SC.family(r) == fam


def _one_stage(r):
    return SC.family(r) in ("crop", "box")


def _boxes_of(r):
    """(w, h) of every box a one-stage row resizes."""
    return [(r.cw, r.ch)] if SC.family(r) == "crop" else [c[1][2:] for c in r.clips]


def _frames_of_clip(r, k):
    return r.slots[k] if SC.family(r) == "crop" else (r.clips[k][0],)


def _touches_before_larger(r):
    """A ragged row: some clip's box ends on its own frame's right and bottom edge, and the next frame in the buffer
    is larger."""
    for k in range(len(r.slots if SC.family(r) == "crop" else r.clips)):
        i = _frames_of_clip(r, k)[0]
        H, W = r.sizes[i]
        if SC.family(r) == "crop":
            x0, y0, _ = r.crops[k]
            w, h = r.cw, r.ch
        else:
            x0, y0, w, h = r.clips[k][1][:4]
        if x0 + w == W and y0 + h == H and i + 1 < len(r.sizes) and r.sizes[i + 1][0] * r.sizes[i + 1][1] > H * W:
            return True
    return False


def _box_row_split(r, pl):
    """Box form: the tallest box and the most-tapped box are different clips, tables at non-zero offsets."""
    if SC.family(r) != "box" or pl is None:
        return False
    desc = SC.box_descriptors(r)[0]
    h, yt = desc[:, 5], desc[:, 9]
    return int(h.argmax()) != int(yt.argmax()) and int(yt.max()) > int(yt[h.argmax()]) and \
        bool((desc[1:, 6] > 0).all()) and bool((desc[1:, 7] > 0).all())


EDGES = {}
for _R in (32, 16, 8, 4, 2, 1):
    EDGES["one-stage band height R = %d" % _R] = lambda r, pl, R=_R: _one_stage(r) and pl and pl["R"] == R
    EDGES["two-stage band height R = %d" % _R] = lambda r, pl, R=_R: _is("two")(r) and pl and pl["R"] == R
for _k in (16, 8, 4, 2, 1):
    EDGES["crop kernel, R = %d" % _k] = lambda r, pl, R=_k: _is("crop")(r) and pl and pl["R"] == R
    EDGES["box kernel, R = %d" % _k] = lambda r, pl, R=_k: _is("box")(r) and pl and pl["R"] == R
EDGES.update({
    "crop kernel: R = 1 within 32 KiB of LDS": lambda r, pl: _is("crop")(r) and pl and pl["R"] == 1 and
    pl["lds"] <= 32768,
    "crop kernel: R = 1 with more than 32 KiB of LDS": lambda r, pl: _is("crop")(r) and pl and pl["R"] == 1 and
    pl["lds"] > 32768,
    "box kernel: R = 1 with more than 32 KiB of LDS": lambda r, pl: _is("box")(r) and pl and pl["R"] == 1 and
    pl["lds"] > 32768,
    "crop form refuses: one row's taps do not fit": lambda r, pl: _is("crop")(r) and r.refuse and
    SC.ntaps(r.ch, r.S) <= 64,
    "crop form refuses: taps > 64": lambda r, pl: _is("crop")(r) and r.refuse and SC.ntaps(r.ch, r.S) > 64,
    "box form refuses: one row's taps do not fit": lambda r, pl: _is("box")(r) and r.refuse and
    max(SC.ntaps(h, r.S) for _, h in _boxes_of(r)) <= 64,
    "box form refuses: taps > 64": lambda r, pl: _is("box")(r) and r.refuse and
    max(SC.ntaps(h, r.S) for _, h in _boxes_of(r)) > 64,
    "crop kernel: a partial last band": lambda r, pl: _is("crop")(r) and pl and r.S % pl["R"] != 0 and pl["bands"] > 1,
    "box kernel: a partial last band": lambda r, pl: _is("box")(r) and pl and r.S % pl["R"] != 0 and pl["bands"] > 1,
    "crop kernel: a single band, S < R": lambda r, pl: _is("crop")(r) and pl and pl["bands"] == 1 and r.S < pl["R"],
    "box kernel: a single band, S < R": lambda r, pl: _is("box")(r) and pl and pl["bands"] == 1 and r.S < pl["R"],
    "crop kernel: R < 32 behind a horizontal pass that resamples (cw != S)": lambda r, pl: _is("crop")(r) and pl and
    pl["R"] < 32 and r.cw != r.S,
    "crop kernel: cap_rows clipped to the box height": lambda r, pl: _is("crop")(r) and pl and pl["clipped"],
    "box kernel: cap_rows clipped to the tallest box": lambda r, pl: _is("box")(r) and pl and pl["clipped"],
    "crop kernel, bytes out: S % 4 != 0": lambda r, pl: _is("crop")(r) and pl and pl["u8out"] and r.S % 4 != 0,
    "crop kernel, fp32 out: S % 4 != 0 (guarded stores)": lambda r, pl: _is("crop")(r) and pl and not pl["u8out"] and
    r.S % 4 != 0,
    "box kernel: S % 4 != 0": lambda r, pl: _is("box")(r) and pl and r.S % 4 != 0,
    "box kernel: S % 4 == 0": lambda r, pl: _is("box")(r) and pl and r.S % 4 == 0,
    "crop kernel, fp32 one-size: 16-byte stores": lambda r, pl: _is("crop")(r) and pl and pl["vec"] and
    not pl["ragged"],
    "crop kernel, fp32 one-size: S % 4 == 0 and out one float off": lambda r, pl: _is("crop")(r) and pl and
    r.form == "f32" and r.S % 4 == 0 and r.out_off == 1 and not pl["vec"],
    "crop kernel, fp32 ragged: S % 4 == 0 and out one float off": lambda r, pl: _is("crop")(r) and pl and
    r.form == "rag_f32" and r.S % 4 == 0 and r.out_off == 1 and not pl["vec"],
    "crop kernel: up-sampling a box of more than one pixel on both axes (5 taps)": lambda r, pl: _is("crop")(r) and pl and r.cw < r.S and
    r.ch < r.S and r.cw > 1,
    "box kernel: up-sampling on both axes (5 taps)": lambda r, pl: _is("box")(r) and pl and
    any(1 < w < r.S and 1 < h < r.S for w, h in _boxes_of(r)),
    "crop kernel: identity, cw == ch == S": lambda r, pl: _is("crop")(r) and pl and r.cw == r.ch == r.S,
    "box kernel: identity, w == h == S": lambda r, pl: _is("box")(r) and pl and (r.S, r.S) in _boxes_of(r),
    "crop kernel: a box of one pixel": lambda r, pl: _is("crop")(r) and pl and r.cw == r.ch == 1,
    "box kernel: a box one pixel wide and a box one pixel high": lambda r, pl: _is("box")(r) and pl and
    any(w == 1 for w, _ in _boxes_of(r)) and any(h == 1 for _, h in _boxes_of(r)),
    "crop kernel, one-size: flush right and bottom, with and without flip, and flip at x0 = 0":
        lambda r, pl: _is("crop")(r) and pl and not pl["ragged"] and
        all((r.sizes[0][1] - r.cw, r.sizes[0][0] - r.ch, f) in r.crops for f in (0, 1)) and
        any(x0 == 0 and f for x0, _, f in r.crops) and r.sizes[0][1] > r.cw,
    "crop kernel: n_crops = 16": lambda r, pl: _is("crop")(r) and pl and not pl["ragged"] and len(r.crops) == 16,
    "crop kernel, one-size: slots repeat and share frames": lambda r, pl: _is("crop")(r) and pl and
    not pl["ragged"] and any(len(set(s)) < len(s) for s in r.slots) and
    len({i for s in r.slots for i in s}) < sum(len(set(s)) for s in r.slots),
    "box kernel: tallest and most-tapped box are different clips, non-zero table offsets": _box_row_split,
    "crop kernel, ragged fp32: three frame sizes, shared slot offsets, own edge before a larger frame":
        lambda r, pl: _is("crop")(r) and pl and r.form == "rag_f32" and len(set(r.sizes)) >= 3 and
        len({s for s in r.slots}) < len(r.slots) and _touches_before_larger(r),
    "crop kernel, ragged bytes: three frame sizes, shared slot offsets, own edge before a larger frame":
        lambda r, pl: _is("crop")(r) and pl and r.form == "rag_u8" and len(set(r.sizes)) >= 3 and
        len({s for s in r.slots}) < len(r.slots) and _touches_before_larger(r),
    "box kernel, ragged: three frame sizes, shared frames, own edge before a larger frame, T > 1":
        lambda r, pl: _is("box")(r) and pl and r.ragged and len(set(r.sizes)) >= 3 and r.T > 1 and
        len({c[0] for c in r.clips}) < len(r.clips) and _touches_before_larger(r),
    # ---- two-stage ----
    "two-stage: fallback window with cx, cy != 0": lambda r, pl: _is("two")(r) and pl and
    any(cx > 0 and cy > 0 for _, _, _, (cx, cy) in r.clips),
    "two-stage: size == S (identity second stage)": lambda r, pl: _is("two")(r) and pl and r.size == r.S,
    "two-stage: size % 4 != 0 and S % 4 != 0": lambda r, pl: _is("two")(r) and pl and r.size % 4 and r.S % 4,
    "two-stage: S > size (second stage up-samples)": lambda r, pl: _is("two")(r) and pl and r.S > r.size,
    "two-stage: `one` sized by H1's rows": lambda r, pl: _is("two")(r) and pl and pl["one"] == "h1",
    "two-stage: `one` sized by H2's rows, small": lambda r, pl: _is("two")(r) and pl and pl["one"] == "h2" and
    not pl["optin"],
    "two-stage: `one` sized by H2's rows, above 64 KiB": lambda r, pl: _is("two")(r) and pl and pl["one"] == "h2" and
    pl["optin"],
    **{"two-stage <U8OUT=%d, RAGGED=%d>: LDS above 64 KiB, the instantiation's dynamic-LDS opt-in" % (u, g):
       (lambda r, pl, u=u, g=g: _is("two")(r) and pl and pl["optin"] and (pl["u8out"], pl["ragged"]) == (bool(u), bool(g)))
       for u in (0, 1) for g in (0, 1)},
    "two-stage: R = 32 above 64 KiB, the whole size x size image staged": lambda r, pl: _is("two")(r) and pl and
    pl["R"] == 32 and pl["optin"] and pl["capA"] == r.size,
    "two-stage: R > 1 below 64 KiB": lambda r, pl: _is("two")(r) and pl and 1 < pl["R"] < 32 and not pl["optin"],
    "two-stage refuses: one row's halo does not fit": lambda r, pl: _is("two")(r) and r.refuse,
    "two-stage, ragged: three frame sizes": lambda r, pl: _is("two")(r) and pl and pl["ragged"] and
    len(set(r.sizes)) >= 3,
    "two-stage: T > 1": lambda r, pl: _is("two")(r) and pl and r.T > 1,
    # ---- stage_clips ----
    "stage_clips uint8: vector path with idle lanes (THW / 16 < 256)": lambda r, pl: _is("clips")(r) and pl and
    pl["u8"] and pl["vec"] and r.thw // 16 < 256,
    "stage_clips uint8: scalar by length (THW % 16), one sweep of the grid": lambda r, pl: _is("clips")(r) and pl and
    pl["u8"] and r.thw % 16 != 0 and r.thw <= pl["gx"] * 256,
    "stage_clips uint8: scalar by a source one byte off": lambda r, pl: _is("clips")(r) and pl and pl["u8"] and
    r.thw % 16 == 0 and r.src_off == 1 and not pl["vec"],
    "stage_clips uint8: scalar by a destination one float off": lambda r, pl: _is("clips")(r) and pl and pl["u8"] and
    r.thw % 16 == 0 and r.src_off == 0 and r.out_off == 1 and not pl["vec"],
    "stage_clips fp32: vector path": lambda r, pl: _is("clips")(r) and pl and not pl["u8"] and pl["vec"],
    "stage_clips fp32: scalar by length (THW % 4)": lambda r, pl: _is("clips")(r) and pl and not pl["u8"] and
    r.thw % 4 != 0,
    "stage_clips fp32: scalar by a source one float off": lambda r, pl: _is("clips")(r) and pl and not pl["u8"] and
    r.thw % 4 == 0 and r.src_off == 1 and not pl["vec"],
    "stage_clips fp32: scalar by a destination one float off": lambda r, pl: _is("clips")(r) and pl and
    not pl["u8"] and r.thw % 4 == 0 and r.src_off == 0 and r.out_off == 1 and not pl["vec"],
    "stage_clips: the vector loop past the 64-workgroup clamp, with a tail": lambda r, pl: _is("clips")(r) and pl and
    pl["vec"] and pl["gx"] == 64 and 0 < r.thw // 16 - 64 * 256 < 256,
    "stage_clips: the scalar loop runs more than once": lambda r, pl: _is("clips")(r) and pl and not pl["vec"] and
    r.thw > pl["gx"] * 256 and r.thw % 256 != 0,
    "stage_clips: C = 1": lambda r, pl: _is("clips")(r) and pl and r.C == 1,
    "stage_clips: C = 4": lambda r, pl: _is("clips")(r) and pl and r.C == 4,
    "stage_clips refuses B * C * S > 65535": lambda r, pl: _is("clips")(r) and r.refuse and r.B * r.C * r.S == 65536,
})


def _progs(r):
    return [[k for k, _ in p] for p in r.programs]


def _has_run(kinds, *want):
    body = [k for k in kinds if k != SC.NOP]
    return any(tuple(body[i:i + len(want)]) == want for i in range(len(body)))


EDGES.update({
    "jitter: H * W % 4 != 0, frames 1.. off a 4-byte boundary": lambda r, pl: _is("prog")(r) and not r.aug and
    (r.H * r.W) % 4 != 0 and (r.H * r.W * 3) % 4 != 0 and r.N > 1,
    "augment: frames 1.. off a 4-byte boundary": lambda r, pl: _is("prog")(r) and r.aug and
    (r.H * r.W * 3) % 4 != 0 and r.N > 1,
    "augment: W % 4 != 0 with flip and with blur (byte paths)": lambda r, pl: _is("prog")(r) and r.aug and
    r.W % 4 != 0 and any(SC.BLUR in p and p.count(SC.FLIP) % 2 == 1 for p in _progs(r)),
    "contrast first": lambda r, pl: _is("prog")(r) and any(p[0] == SC.CON and len(p) > 1 and p[1] != SC.CON
                                                            for p in _progs(r)),
    "contrast last": lambda r, pl: _is("prog")(r) and any(len(p) > 1 and p[-1] == SC.CON and p[-2] != SC.CON
                                                           for p in _progs(r)),
    "contrast twice in a row": lambda r, pl: _is("prog")(r) and any(_has_run(p, SC.CON, SC.CON) for p in _progs(r)),
    "contrast on both sides of a blur": lambda r, pl: _is("prog")(r) and
    any(_has_run(p, SC.CON, SC.BLUR, SC.CON) for p in _progs(r)),
    "blur radius below 1": lambda r, pl: _is("prog")(r) and any(k == SC.BLUR and 0 < v < 1 for p in r.programs
                                                                  for k, v in p),
    "blur radius 16, larger than either side": lambda r, pl: _is("prog")(r) and max(r.H, r.W) < 16 and
    any(k == SC.BLUR and v == 16 for p in r.programs for k, v in p),
    "P = 8 with no NOP": lambda r, pl: _is("prog")(r) and any(len(p) == 8 and SC.NOP not in p for p in _progs(r)),
    "augment: W % 4 == 0, mirrored 16-byte stores behind a blur": lambda r, pl: _is("prog")(r) and r.aug and
    pl["vec"] and any(SC.BLUR in p and p.count(SC.FLIP) % 2 == 1 for p in _progs(r)),
    "group_size does not divide N": lambda r, pl: _is("prog")(r) and r.N % r.group_size != 0,
    "224 x 224: 13 items a lane, the whole LDS": lambda r, pl: _is("prog")(r) and r.H == r.W == 224 and
    pl["per_lane"] == 13,
    "jitter: no whole-frame op, no LDS": lambda r, pl: _is("prog")(r) and not r.aug and not pl["use_lds"],
    "augment: no whole-frame op, no LDS, flip": lambda r, pl: _is("prog")(r) and r.aug and not pl["use_lds"] and
    any(p.count(SC.FLIP) % 2 == 1 for p in _progs(r)),
    "T > 1 in a program launch": lambda r, pl: _is("prog")(r) and r.T > 1,
})


def _hits(pred):
    return [r.name for r, pl in PLANS if pred(r, pl)]


@pytest.mark.parametrize("edge", list(EDGES))
def test_table_hits_edge(edge):
    hit = _hits(EDGES[edge])
    print("\n%s: %s" % (edge, hit))
    assert hit or edge in UNREACHABLE, "no row hits: %s" % edge


def test_every_row_is_the_only_cover_of_something():
    """Deleting any single row must lose an instantiation or an edge: test_table_hits_edge /
    test_table_reaches_every_instantiation then name it."""
    sole = {}
    for edge, pred in EDGES.items():
        hit = _hits(pred)
        if len(hit) == 1:
            sole.setdefault(hit[0], []).append(edge)
    inst = {}
    for r, pl in PLANS:
        if pl is not None:
            inst.setdefault(instantiation(r, pl), []).append(r.name)
    for k, names in inst.items():
        if len(names) == 1:
            sole.setdefault(names[0], []).append(k)
    print()
    for r in SC.ALL:
        print("  %-22s %s" % (r.name, "; ".join(sole.get(r.name, [])) or "-"))
    assert [r.name for r in SC.ALL if r.name not in sole] == []


# ---- the band bounds against the real tables -----------------------------------------------------------------------------

def _last_tap(K):
    """Per output sample the index of its last non-zero tap (0 for an all-zero row)."""
    nz = K != 0
    return np.where(nz.any(1), K.shape[1] - 1 - np.argmax(nz[:, ::-1], 1), 0)


def _check_one_stage(ymin, K, ch, S, pl):
    """Every band of the kernel's own arithmetic stages the last non-zero tap of every one of its rows."""
    last = ymin.astype(np.int64) + _last_tap(K)
    ytaps, R = K.shape[1], pl["R"]
    for r0 in range(0, S, R):
        r1 = min(r0 + R, S)
        ylo = min(max(int(ymin[r0]), 0), ch - 1)
        rows = min(min(max(int(ymin[r1 - 1]) + ytaps, ylo + 1), ch) - ylo, pl["cap_rows"])
        assert int(ymin[r0:r1].min()) >= ylo and int(last[r0:r1].max()) < ylo + rows, (ch, S, r0, pl)


ONE_STAGE_S = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 16, 18, 20, 22, 24, 27, 31, 32, 37, 40, 48, 52, 61, 64, 75, 90,
               97, 112, 128, 137, 200, 224, 337, 512)


def one_stage_sweep():
    """(box height, S) pairs the launchers can be asked about (at most 64 taps): for every S a ladder of heights from
    S / 8 to 15.5 S -- every band height and the refusal lie inside it -- in steps of S / 8 with both neighbours (S / 2
    for S >= 200), and the heights of the table's rows."""
    pairs = set()
    for S in ONE_STAGE_S:
        dense = S <= 140
        for j in range(1, 125 if dense else 32):
            for d in ((-1, 0, 1) if dense else (0,)):
                h = max((S * j) // (8 if dense else 2) + d, 1)
                if SC.ntaps(h, S) <= 64:
                    pairs.add((h, S))
    pairs.update((r.ch, r.S) for r in SC.CROPS if SC.ntaps(r.ch, r.S) <= 64)
    return sorted(pairs)


@pytest.mark.parametrize("builder", ["staging.resample_tables", "crops_harness.tables"])
def test_one_stage_band_bound(builder):
    """The whole sweep with each builder on its own: the product's tables are the ones the kernels receive."""
    tables = staging.resample_tables if builder.startswith("staging") else CH.tables
    pairs = one_stage_sweep()
    assert len(pairs) >= 7090
    seen, refused, checked = set(), 0, 0
    for h, S in pairs:
        ymin, K = tables(h, S)
        assert K.shape[1] == SC.ntaps(h, S) <= 64
        try:
            pl = ops.stage_crops_plan(1, h, 1, 1, 1, [(0, 0, 0)], 1, h, S, 5, K.shape[1], u8=True)
        except _lib.HipLibraryError:
            refused += 1
            continue
        seen.add(pl["R"])
        _check_one_stage(ymin, K, h, S, pl)
        checked += 1
    assert seen == {32, 16, 8, 4, 2, 1} and refused > 0 and checked + refused == len(pairs)


def _window(n_in, n_out, c0, size, tables):
    lo, K = tables(n_in, n_out)
    return lo[c0:c0 + size], K[c0:c0 + size]


def two_stage_sweep():
    """(h, oh, cy, size, S) draws the launcher can be asked about (at most 64 taps in either stage), seeded."""
    rng = np.random.RandomState(26)
    draws = []
    for size in (224, 200, 128, 112, 64, 33, 18, 16):
        for S in (32, 31, 24, 16, 13, 8, 4, 2, 224, 128, 16 + size % 16):
            if SC.ntaps(size, S) > 64:
                continue
            for _ in range(52):
                h = int(rng.choice([rng.randint(1, 33), rng.randint(33, 251), 250, 200, size]))
                oh = size + int(rng.choice([0, 0, rng.randint(0, 80)]))
                cy = int(rng.randint(0, oh - size + 1))
                if SC.ntaps(h, oh) <= 64:
                    draws.append((h, oh, cy, size, S))
    for r in SC.TWOS:
        if not r.refuse:
            draws += [(reg[3], res[1], win[1], r.size, r.S) for _, reg, res, win in r.clips]
    return draws


@pytest.mark.parametrize("builder", ["staging.resample_tables", "crops_harness.tables"])
def test_two_stage_band_bound(builder):
    """Every draw with each builder on its own (the tables of an axis are computed once per (n_in, n_out))."""
    import functools
    tables = functools.lru_cache(None)(staging.resample_tables if builder.startswith("staging") else CH.tables)
    draws = two_stage_sweep()
    assert len(draws) >= 3115
    seen, optin, checked = set(), 0, 0
    for n, (h, oh, cy, size, S) in enumerate(draws):
        min2, K2 = tables(size, S)
        ymin, K1 = _window(h, oh, cy, size, tables)
        assert K2.shape[1] <= 64 and K1.shape[1] <= 64
        P = (size + 3) & ~3
        desc = [[0, 1, 0, 0, 1, h, size, oh, 0, cy, 0, 0, 5, K1.shape[1]]]
        try:
            pl = ops.resize2_boxes_plan(desc, 1, size, S, P * 6, P * (1 + K1.shape[1]), K2.shape[1], u8=True,
                                        shape=(1, h, 1))
        except _lib.HipLibraryError:
            continue
        seen.add(pl["R"])
        optin += pl["optin"]
        checked += 1
        last2 = min2.astype(np.int64) + _last_tap(K2)
        last1 = ymin.astype(np.int64) + _last_tap(K1)
        taps2, ytaps, R = K2.shape[1], K1.shape[1], pl["R"]
        for r0 in range(0, S, R):
            r1 = min(r0 + R, S)
            alo = min(max(int(min2[r0]), 0), size - 1)
            arows = min(min(max(int(min2[r1 - 1]) + taps2, alo + 1), size) - alo, pl["capA"])
            assert int(min2[r0:r1].min()) >= alo and int(last2[r0:r1].max()) < alo + arows, (draws[n], r0, pl)
            ylo = min(max(int(ymin[alo]), 0), h - 1)
            rows1 = min(min(max(int(ymin[alo + arows - 1]) + ytaps, ylo + 1), h) - ylo, pl["cap1"])
            assert int(ymin[alo:alo + arows].min()) >= ylo, (draws[n], r0, pl)
            assert int(last1[alo:alo + arows].max()) < ylo + rows1, (draws[n], r0, pl)
    assert seen == {32, 16, 8, 4, 2, 1} and optin > 0 and checked >= 3115


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_queries_refuse_what_the_launchers_refuse():
    lib = _lib.load()
    a = ops.PLAN_ADDR
    f3 = (C.c_float * 3)(1, 1, 1)
    box = (C.c_int32 * 3)(0, 0, 0)
    o8, o10 = (C.c_int32 * 8)(), (C.c_int32 * 10)()
    # crop form: the query's own answer, then a null plan, null pointers, both outputs, and the two refusal geometries
    # through the launcher itself (it returns before it launches: no device is touched)
    crops = lambda *t: lib.coclr_stage_crops_plan(*t)                                   # noqa: E731
    ok = [a, 1, 40, 52, a, 1, 1, box, 1, 28, 28, 16, a, a, 7, a, a, 7, f3, f3, None, a, o8]
    assert crops(*ok) == 0
    for i in (0, 4, 7, 12, 13, 15, 16, 22):
        assert crops(*(ok[:i] + [None] + ok[i + 1:])) == 1, i
    assert crops(*(ok[:20] + [a, a, o8])) == 1 and crops(*(ok[:20] + [None, None, o8])) == 1
    assert crops(*(ok[:18] + [None, None, None, a, o8])) == 1                       # fp32 without mean / std
    assert crops(*(ok[:18] + [None, None, a, None, o8])) == 0                       # bytes need none
    # c_refuse_lds: launcher and query refuse, and for the LDS bound: 61 taps instead of 63 in the same frame fit
    r = SC.BY_NAME["c_refuse_lds"]
    H, W = r.sizes[0]
    args = [a, 1, H, W, a, 1, 1, box, 1, r.cw, r.ch, r.S, a, a, SC.ntaps(r.cw, r.S), a, a, SC.ntaps(r.ch, r.S)]
    assert SC.ntaps(r.ch, r.S) == 63 and (63 + 2) * 3 * ((r.S + 3) & ~3) > 65536
    assert lib.coclr_resize_crops_u8(*(args + [a, None])) == 1
    assert crops(*(args + [f3, f3, a, None, o8])) == 1
    fits = args[:10] + [r.ch - 7, r.S] + args[12:17] + [SC.ntaps(r.ch - 7, r.S)]
    assert SC.ntaps(r.ch - 7, r.S) == 61 and crops(*(fits + [f3, f3, a, None, o8])) == 0 and o8[0] == 1
    # c_refuse_taps (ragged): launcher and query refuse, and for the tap count: the same call with 64 taps is planned
    r = SC.BY_NAME["c_refuse_taps"]
    desc, slot_off, nbytes = SC.crop_descriptors(r)
    dp, sp = C.cast(desc.data_ptr(), C.POINTER(C.c_int32)), C.cast(slot_off.data_ptr(), C.POINTER(C.c_int64))
    yt = SC.ntaps(r.ch, r.S)
    rag = [a, nbytes, a, dp, 1, 1, a, sp, r.cw, r.ch, r.S, a, a, SC.ntaps(r.cw, r.S), a, a, yt, f3, f3, None, a]
    assert yt == 67
    assert lib.coclr_stage_crops_ragged(*(rag + [None])) == 1
    assert lib.coclr_stage_crops_ragged_plan(*(rag + [o8])) == 1
    rag[16] = 64
    assert lib.coclr_stage_crops_ragged_plan(*(rag + [o8])) == 0 and o8[6] == 1
    assert lib.coclr_stage_crops_ragged_plan(*(rag + [None])) == 1                  # a null plan
    for i in (0, 2, 3, 6, 7, 11, 12, 14, 15):
        assert lib.coclr_stage_crops_ragged_plan(*(rag[:i] + [None] + rag[i + 1:] + [o8])) == 1, i
    assert lib.coclr_stage_crops_ragged_plan(*(rag[:19] + [a, a, o8])) == 1         # both outputs
    assert lib.coclr_stage_crops_ragged_plan(*(rag[:19] + [None, None, o8])) == 1   # neither
    assert lib.coclr_stage_crops_ragged_plan(*(rag[:17] + [None, None, None, a, o8])) == 1      # fp32, no mean / std
    assert lib.coclr_stage_crops_ragged_plan(*(rag[:11] + [a + 4] + rag[12:] + [o8])) == 1      # xmin off 16 bytes
    # stage_clips
    o3 = (C.c_int32 * 3)()
    assert lib.coclr_stage_clips_plan(a, 1, a, 1, 3, 1, 16, f3, f3, o3) == 0
    assert lib.coclr_stage_clips_plan(a, 1, a, 1, 3, 1, 16, f3, f3, None) == 1
    assert lib.coclr_stage_clips_plan(None, 1, a, 1, 3, 1, 16, f3, f3, o3) == 1
    assert lib.coclr_stage_clips_plan(a, 1, None, 1, 3, 1, 16, f3, f3, o3) == 1
    assert lib.coclr_stage_clips_plan(a, 1, a, 1, 5, 1, 16, f3, f3, o3) == 1
    r = SC.BY_NAME["s_refuse"]
    f4 = (C.c_float * 4)(1, 1, 1, 1)
    assert lib.coclr_stage_clips_plan(a, 0, a, r.B, r.C, r.S, r.thw, f4, f4, o3) == 1
    assert lib.coclr_stage_clips(a, 0, a, r.B, r.C, r.S, r.thw, f4, f4, None) == 1
    assert lib.coclr_stage_clips_plan(a, 0, a, r.B, r.C, r.S - 1, r.thw, f4, f4, o3) == 0
    # box and two-stage forms: null plan, null descriptors, and the refusal rows through the launchers
    for r in (SC.BY_NAME["b_refuse_lds"], SC.BY_NAME["b_refuse_taps"]):
        desc, xtab, ytab = SC.box_descriptors(r)
        dp = C.cast(desc.data_ptr(), C.POINTER(C.c_int32))
        F, H, W = (0, 0, 0) if r.ragged else (len(r.sizes) * r.T,) + r.sizes[0]
        nbytes = SC.ragged_offsets(r.sizes, r.T)[1] if r.ragged else 0
        tail = [dp, len(r.clips), r.T, r.S, a, xtab.numel(), a, ytab.numel(), a]
        assert lib.coclr_resize_boxes_plan(int(r.ragged), a, nbytes, F, H, W, a, *tail, o8) == 1, r.name
        launch = lib.coclr_resize_boxes_ragged_u8(a, nbytes, a, *tail, None) if r.ragged else \
            lib.coclr_resize_boxes_u8(a, F, H, W, a, *tail, None)
        assert launch == 1, r.name
        if r.name == "b_refuse_taps":            # for the tap count: the same descriptor with 64 y taps is planned
            assert int(desc[0, 9]) == 67
            desc[0, 9] = 64
            assert lib.coclr_resize_boxes_plan(int(r.ragged), a, nbytes, F, H, W, a, *tail, o8) == 0
        else:                                    # for the LDS bound: 63 taps are admitted, seven rows fewer (61) fit
            assert int(desc[0, 9]) == 63
            desc[0, 5], desc[0, 9] = r.clips[0][1][3] - 7, 61
            assert lib.coclr_resize_boxes_plan(int(r.ragged), a, nbytes, F, H, W, a, *tail, o8) == 0 and o8[0] == 1
    r = SC.BY_NAME["b_r16"]
    desc, xtab, ytab = SC.box_descriptors(r)
    dp = C.cast(desc.data_ptr(), C.POINTER(C.c_int32))
    good = [0, a, 0, 1, 286, 37, a, dp, 2, 1, 37, a, xtab.numel(), a, ytab.numel(), a, o8]
    assert lib.coclr_resize_boxes_plan(*good) == 0
    for i in (1, 6, 7, 11, 13, 15, 16):
        assert lib.coclr_resize_boxes_plan(*(good[:i] + [None] + good[i + 1:])) == 1, i
    assert lib.coclr_resize_boxes_plan(*(good[:11] + [a + 4] + good[12:])) == 1           # a misaligned table
    r = SC.BY_NAME["t_refuse"]
    desc, xtab, ytab, tab2 = SC.two_descriptors(r)
    dp = C.cast(desc.data_ptr(), C.POINTER(C.c_int32))
    H, W = r.sizes[0]
    body = [a, dp, 1, r.T, r.size, r.S, a, xtab.numel(), a, ytab.numel(), a, tab2.numel(), tab2.shape[0] - 1]
    assert lib.coclr_resize2_boxes_plan(0, a, 0, 1, H, W, *body, None, None, a, None, o10) == 1
    assert lib.coclr_resize2_boxes(a, 1, H, W, *body, None, None, a, None, None) == 1
    body[4] = 32                                                                           # S = 32 fits
    body[11:] = [len(CH.kernel_layout(224, 32)[1]) * 32 + 32, len(CH.kernel_layout(224, 32)[1])]
    assert lib.coclr_resize2_boxes_plan(0, a, 0, 1, H, W, *body, None, None, a, None, o10) == 0
    assert lib.coclr_resize2_boxes_plan(0, a, 0, 1, H, W, *body, None, None, a, None, None) == 1
    assert lib.coclr_resize2_boxes_plan(0, a, 0, 1, H, W, *body, None, None, a, a, o10) == 1      # both outputs
    assert lib.coclr_resize2_boxes_plan(0, a, 0, 1, H, W, *body, None, None, None, a, o10) == 1   # fp32, no mean / std
    # programs: a blur in the jitter form, a radius above 16, too large a frame, G * group_size < N
    with pytest.raises(_lib.HipLibraryError):
        ops.jitter_plan(False, 1, 4, 4, 1, [[SC.BLUR]], [[1.0]], 1)
    with pytest.raises(_lib.HipLibraryError):
        ops.jitter_plan(True, 1, 4, 4, 1, [[SC.BLUR]], [[16.5]], 1)
    with pytest.raises(_lib.HipLibraryError):
        ops.jitter_plan(True, 1, 225, 224, 1, [[SC.CON]], [[1.0]], 1)
    with pytest.raises(_lib.HipLibraryError):
        ops.jitter_plan(True, 5, 4, 4, 1, [[SC.CON], [SC.NOP]], [[1.0], [0.0]], 2)
    assert ops.jitter_plan(True, 4, 4, 4, 1, [[SC.CON], [SC.NOP]], [[1.0], [0.0]], 2)["cuts"] == 1
    o7 = (C.c_int32 * 7)()
    k1, p1 = (C.c_int32 * 1)(0), (C.c_float * 1)(0)
    assert lib.coclr_jitter_plan(0, a, 1, 4, 4, 1, a, a, k1, p1, 1, 1, 1, f3, f3, a, o7) == 0
    assert lib.coclr_jitter_plan(0, a, 1, 4, 4, 1, a, a, k1, p1, 1, 1, 1, f3, f3, a, None) == 1
    assert lib.coclr_jitter_plan(0, a, 1, 4, 4, 1, a, a, None, p1, 1, 1, 1, f3, f3, a, o7) == 1
    assert lib.coclr_jitter_plan(0, a, 1, 4, 4, 1, a, a, k1, p1, 1, 1, 1, f3, f3, None, o7) == 1
    # ragged crops: a misaligned x table, a box that leaves its own frame
    r = SC.BY_NAME["c_rag_u8_identity"]
    desc, slot_off, nbytes = SC.crop_descriptors(r)
    assert ops.stage_crops_ragged_plan(nbytes, desc, slot_off, 12, 12, 12, 5, 5, u8=True)["ragged"]
    desc[0, 0] += 1
    with pytest.raises(_lib.HipLibraryError):
        ops.stage_crops_ragged_plan(nbytes, desc, slot_off, 12, 12, 12, 5, 5, u8=True)


def test_stage_clips_takes_the_scalar_path_for_a_misaligned_destination():
    """Before ABI 26 stage_clips_kernel tested the source's alignment only and stored float4 through `out`."""
    a = ops.PLAN_ADDR
    for u8, thw in ((True, 32), (False, 8)):
        assert ops.stage_clips_plan(2, 3, 2, thw, u8)["vec"]
        for off in (4, 8, 12):
            assert not ops.stage_clips_plan(2, 3, 2, thw, u8, out_addr=a + off)["vec"]
        assert not ops.stage_clips_plan(2, 3, 2, thw, u8, src_addr=a + (1 if u8 else 4))["vec"]
        assert ops.stage_clips_plan(2, 3, 2, thw, u8, src_addr=a + 16, out_addr=a + 32)["vec"]


# ---- the references against PIL ----------------------------------------------------------------------------------------------

def _pil_resize(Image, img, size):
    """Image.resize(size, BICUBIC, box=the whole of `img`).  The reference crops first and resizes the crop; box= on
    the uncropped frame would let taps at the box's edge read pixels outside it, which neither it nor the kernel does."""
    return img.resize(size, Image.BICUBIC, box=(0, 0) + img.size)


@pytest.mark.parametrize("name", [r.name for r in RESIZE])
def test_resize_reference_equals_pil(name):
    Image = pytest.importorskip("PIL.Image")
    r = SC.BY_NAME[name]
    src = SC.sources(r)
    want = SC.resize_reference(r, src)
    fam = SC.family(r)

    def one(frame, x0, y0, w, h, flip=0):
        img = Image.fromarray(frame)
        if flip:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        return img.crop((x0, y0, x0 + w, y0 + h))

    if fam == "crop":
        rag = r.form.startswith("rag")
        for k, s in enumerate(r.slots):
            for c, (x0, y0, flip) in enumerate([r.crops[k]] if rag else r.crops):
                for t, i in enumerate(s):
                    got = np.asarray(_pil_resize(Image, one(src[i][0], x0, y0, r.cw, r.ch, flip), (r.S, r.S)))
                    assert np.array_equal(got, want[k, t] if rag else want[c, k, t]), (k, c, t)
    elif fam == "box":
        for k, clip in enumerate(r.clips):
            for t in range(r.T):
                got = np.asarray(_pil_resize(Image, one(src[clip[0]][t], *clip[1]), (r.S, r.S)))
                assert np.array_equal(got, want[k, t]), (k, t)
    else:
        for k, (s, region, (ow, oh), (cx, cy)) in enumerate(r.clips):
            for t in range(r.T):
                img = _pil_resize(Image, one(src[s][t], *region), (ow, oh))
                img = img.crop((cx, cy, cx + r.size, cy + r.size))
                got = np.asarray(_pil_resize(Image, img, (r.S, r.S)))
                assert np.array_equal(got, want[k, t]), (k, t)


def test_pil_differs_from_the_restatement_by_pass_order_only():
    """Why the band-height rows keep their boxes S wide.  The restatement, the kernels and the reference's Pillow 6.1
    resample horizontally first; Pillow 12 was seen to resample a tall thin box vertically first, which rounds the
    intermediate bytes differently.  Whatever this Pillow does on such a box, its result is one of the two orders of
    the restatement's own passes, and where the box is S wide (one pass) the two agree."""
    Image = pytest.importorskip("PIL.Image")
    S = 37
    for h, w in ((450, 4), (526, 4), (526, 8), (526, S)):
        f = SC.edges(h, w, 5)
        pil = np.asarray(_pil_resize(Image, Image.fromarray(f), (S, S)))
        hv = CH.resize_u8(f[None], S)[0]
        v = CH.resample_last_axis(np.ascontiguousarray(f.transpose(1, 2, 0)), S)                  # (w, 3, S(y))
        vh = CH.resample_last_axis(np.ascontiguousarray(v.transpose(2, 1, 0)), S).transpose(0, 2, 1)   # (S(y), S(x), 3)
        assert np.array_equal(pil, hv) or np.array_equal(pil, vh), (h, w)
        if w == S:
            assert np.array_equal(hv, vh) and np.array_equal(pil, hv)
        if (h, w) == (526, 8):
            assert np.array_equal(pil, hv)               # c_u8_r8's geometry: horizontally first in every Pillow seen


def _pil_op(Image, img, kind, v):
    from PIL import ImageEnhance
    if kind == SC.NOP:
        return img
    if kind in (SC.BRI, SC.CON, SC.SAT):
        E = {SC.BRI: ImageEnhance.Brightness, SC.CON: ImageEnhance.Contrast, SC.SAT: ImageEnhance.Color}[kind]
        return E(img).enhance(v)
    if kind == SC.HUE:
        h, s, val = img.convert("HSV").split()
        h = Image.fromarray(((np.asarray(h).astype(np.int64) + int(v)) & 255).astype(np.uint8), "L")
        return Image.merge("HSV", (h, s, val)).convert("RGB")
    if kind == SC.GRAY:
        ch = img.split()[int(v)]
        return Image.merge("RGB", (ch, ch, ch))
    if kind == SC.BLUR:          # ImageFilter.GaussianBlur is box_blur(its radius for sigma, 3 passes): the radius itself
        return img._new(img.im.box_blur((float(v), float(v)), 3)) if v > 0 else img
    return img.transpose(Image.FLIP_LEFT_RIGHT)


@pytest.mark.parametrize("name", [r.name for r in SC.PROGS])
def test_program_reference_equals_pil(name):
    Image = pytest.importorskip("PIL.Image")
    r = SC.BY_NAME[name]
    frames = SC.program_frames(r)
    want = SC.program_reference_u8(r, frames)
    for n, f in enumerate(frames):
        img = Image.fromarray(f)
        for kind, v in r.programs[n // r.group_size]:
            img = _pil_op(Image, img, kind, float(np.float32(v)))
        assert np.array_equal(np.asarray(img), want[n]), n
