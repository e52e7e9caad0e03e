"""CPU tier of the windowed store decode (coclr_amd/jpeg.py: Store.plan / Store.decode with `boxes`; include/coclr_hip.h:
coclr_jpeg_decode_store_window; coclr_amd/staging.py: clip_frames, train_tables_cropped): the host tables on a store
whose buffers are host tensors and whose launches are recording doubles, the refusals of `decode` and of the entry point
without a device, the staging tables against the full-frame ones, and the window arithmetic of csrc/jpeg_core.h
compiled for the host under AddressSanitizer and UBSan (tools/jpeg_window_check.cpp).  Nothing here needs a GPU and
nothing is preloaded into Python."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _jpeg_cases as J
import _jpeg_window_cases as WC
from coclr_amd import _lib, jpeg, ops, staging

ROOT = J.ROOT


@pytest.fixture
def launches(monkeypatch):
    """The three launching ops replaced by doubles that record their name."""
    calls = []
    monkeypatch.setattr(ops, "jpeg_store_index", lambda *a, **k: calls.append("index"))
    monkeypatch.setattr(ops, "jpeg_decode_store", lambda *a, **k: calls.append("store"))
    monkeypatch.setattr(ops, "jpeg_decode_store_window", lambda *a, **k: calls.append("window"))
    return calls


def _store(chunk_bytes=None):
    store = jpeg.Store(1 << 20, 64, chunk_bytes=chunk_bytes, device="cpu")
    for c in J.cases():
        store.add(jpeg.pack([J.raw(c)]))
    return store


def _lanes(c, chunk_bytes):
    info = jpeg.parse(J.raw(c))
    n = len(info["segments"])
    return n if n > 1 else max(1, -(-(info["scan"][1] - info["scan"][0]) // chunk_bytes))


@pytest.mark.parametrize("budget", [256 << 20, 400000, 1])
def test_plan_with_boxes(launches, budget):
    store = _store()
    cases = J.cases()
    picks = WC.all_boxes()[::7] + WC.all_boxes()[-30:]
    ids = [i for i, _ in picks]
    boxes = [b for _, b in picks]
    plain = store.plan(ids, budget)
    assert len(plain) == 6 and len(store.plan(ids, budget, boxes=None)) == 6
    sel, geo, offset, total, stages, blocks, window = store.plan(ids, budget, boxes)
    assert torch.equal(sel, plain[0]) and torch.equal(geo, plain[1]) and blocks == plain[5]
    assert window.dtype == torch.int64 and window.tolist() == [list(b) for b in boxes]
    # the output: every box at 3 w h bytes, 16-byte aligned, in order
    at, want = 0, []
    for _, _, w, h in boxes:
        want.append(at)
        at = (at + 3 * w * h + 15) & ~15
    assert offset.tolist() == want and total == want[-1] + 3 * boxes[-1][2] * boxes[-1][3]
    assert len(stages) == len(plain[4]) and (budget != 1 or len(stages) == len(ids)) and \
        (budget != 400000 or len(stages) > 2)
    nblocks, groups, lanes = [], [], []
    for i, box in picks:
        c = cases[i]
        hs, vs = c["sampling"]
        mx0, my0, mx1, my1 = WC.mcu_rect(c["height"], c["width"], c["ncomp"], hs, vs, box)
        nblocks.append((mx1 - mx0) * (my1 - my0) * WC.mcu_blocks(c["ncomp"], hs, vs))
        groups.append(box[3] * -(-box[2] // 16))
        lanes.append(_lanes(c, 64))
    for (k, e, geom, prefix), (pk, pe, p_geom, p_prefix) in zip(stages, plain[4]):
        assert (k, e) == (pk, pe)                                            # staged by the full-frame workspace
        assert torch.equal(geom[:, :6], p_geom[:, :6]) and geom[:, 6].tolist() == want[k:e]
        assert prefix.shape == (3, e - k + 1) and prefix.dtype == torch.int64
        assert prefix[0].tolist() == [sum(nblocks[k:k + n]) for n in range(e - k + 1)]
        assert prefix[1].tolist() == [sum(groups[k:k + n]) for n in range(e - k + 1)]
        assert prefix[2].tolist() == [sum(lanes[k:k + n]) for n in range(e - k + 1)]
        assert torch.equal(prefix[2], p_prefix[2])
    # a whole-frame box counts the whole frame
    whole = [(0, 0, cases[i]["width"], cases[i]["height"]) for i in range(len(cases))]
    a, b = store.plan(list(range(len(cases))), budget, whole), store.plan(list(range(len(cases))), budget)
    assert torch.equal(a[2], b[2]) and a[3] == b[3]
    assert all(torch.equal(x[2], y[2]) and torch.equal(x[3], y[3]) for x, y in zip(a[4], b[4]))
    # jpeg.window_mcus is the rectangle counted above
    for i, box in picks:
        c = cases[i]
        args = (c["height"], c["width"], c["ncomp"]) + tuple(c["sampling"])
        assert jpeg.window_mcus(*args, *box) == WC.mcu_rect(*args, box)
    assert launches == ["index"] * len(cases)


def test_decode_refuses_bad_boxes_before_any_launch(launches):
    store = _store()
    n = len(launches)
    name = "56x40_420_q50_ramp"
    i = J.names().index(name)
    good = [[0, 0, 56, 40], [10, 5, 8, 8]]
    for bad in ([[0, 0, 56, 40]],                                            # one box for two frames
                [0, 0, 56, 40, 10, 5, 8, 8],                                 # flat
                [[0, 0, 56], [10, 5, 8]],                                    # three words
                [[[0, 0, 56, 40], [10, 5, 8, 8]]],                           # a third dimension
                torch.tensor(good, dtype=torch.float32), torch.tensor(good, dtype=torch.float64),
                torch.tensor(good) > 0,                                      # bool
                [[0.0, 0.0, 56.0, 40.0], [10.0, 5.0, 8.0, 8.0]],
                "boxes",
                [[0, 0, 0, 40], good[1]], [[0, 0, 56, 0], good[1]], [[0, 0, -3, 4], good[1]],
                [good[0], [-1, 5, 8, 8]], [good[0], [10, -1, 8, 8]],
                [good[0], [49, 5, 8, 8]], [good[0], [10, 33, 8, 8]],        # one past the right / bottom edge
                [good[0], [56, 0, 1, 1]], [good[0], [0, 40, 1, 1]],
                [[0, 0, 57, 40], good[1]], [[0, 0, 56, 41], good[1]],
                [good[0], [1 << 40, 0, 1, 1]], [good[0], [0, 0, 1 << 40, 1]]):
        with pytest.raises(ValueError):
            store.decode([i, i], bad)
        with pytest.raises(ValueError):
            store.plan([i, i], boxes=bad)
    # a box is measured against ITS frame: 45 x 37 does not hold what 56 x 40 holds
    small = J.names().index("45x37_420_q50_ramp")
    with pytest.raises(ValueError):
        store.decode([i, small], [good[0], good[0]])
    with pytest.raises(ValueError):
        store.decode([i, 99], good)                                          # ids are still checked
    assert launches[n:] == []
    assert len(store.plan([i, i], boxes=torch.tensor(good, dtype=torch.int32))) == 7       # any integer type will do
    assert len(store.plan([i, i], boxes=[[48, 32, 8, 8], [55, 39, 1, 1]])) == 7           # flush with the edges


def test_entry_point_is_declared_exported_and_bound():
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "coclr_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\bint\s+(coclr_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (coclr_[a-z0-9_]+)", out))
    name = "coclr_jpeg_decode_store_window"
    assert name in declared and name in exported and name in _lib.EXPORTED_SYMBOLS
    assert declared == exported == set(_lib.EXPORTED_SYMBOLS)
    assert lib.coclr_abi_version() == _lib.ABI_VERSION == 26
    assert callable(ops.jpeg_decode_store_window) and ops.JW_FIELDS == 4
    # the window entry is the store entry with the window table, device and host, in front of the prefix
    sig, base = _lib._SIGNATURES[name], _lib._SIGNATURES["coclr_jpeg_decode_store"]
    assert sig == base[:6] + [_lib.vp, C.POINTER(_lib.i64)] + base[6:]


def test_entry_point_rejects_before_any_launch(launches):
    """COCLR_EINVAL from the host copies alone: no call below reaches a device (there is none here; the stand-in
    device pointers are never dereferenced)."""
    lib = _lib.load()
    store = jpeg.Store(1 << 20, 64, device="cpu")
    for c in J.cases()[:8]:
        store.add(jpeg.pack([J.raw(c)]))
    a = store.add(jpeg.pack([J.raw(J.case("56x40_420_rst1"))]))
    b = store.add(jpeg.pack([J.raw(J.case("45x37_422_q100_noise"))]))
    fake = 0x10000                                            # a non-null, 16-byte aligned stand-in
    frames_host, tables_host, segs_host = store._host
    desc = _lib.JpegStore(data=fake, data_bytes=store.nbytes, frames=fake, frames_host=frames_host.data_ptr(),
                          nframes=len(store), tables=fake, tables_host=tables_host.data_ptr(),
                          table_sets=store.table_sets, segs=fake, segs_host=segs_host.data_ptr(), nsegs=store._segs,
                          rows=fake, nrows=store._rows.shape[0], chunk_bytes=64)
    picks = [a, b, b, 2]
    boxes = [[3, 2, 40, 30], [0, 0, 45, 37], [17, 9, 16, 5], [1, 1, 2, 2]]
    sel, geo, offset, total, stages, blocks, window = store.plan(picks, boxes=boxes)
    (_, _, geom, prefix), = stages
    hp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_int64))   # noqa: E731

    def decode(s=sel, g=geom, w=window, p=prefix, F=len(picks), stages=7, blocks=blocks, out_bytes=(total + 15) & ~15,
               ptrs=None, st=desc):
        d = {"sel": fake, "geom": fake, "window": fake, "prefix": fake, "coefs": fake, "planes": fake, "out": fake,
             "status": fake}
        d.update(ptrs or {})
        return lib.coclr_jpeg_decode_store_window(
            C.byref(st) if st is not None else None, d["sel"], hp(s) if s is not None else None, F, d["geom"],
            hp(g) if g is not None else None, d["window"], hp(w) if w is not None else None, d["prefix"],
            hp(p) if p is not None else None, stages, d["coefs"], d["planes"], blocks, d["out"], out_bytes, d["status"],
            None)

    def edit(t, at, value):
        t = t.clone()
        t[at] = value
        return t

    # null tables and pointers
    assert decode(st=None) == 1
    for name in ("sel", "geom", "window", "prefix", "coefs", "planes", "out", "status"):
        assert decode(ptrs={name: None}) == 1, name
    assert decode(s=None) == 1 and decode(g=None) == 1 and decode(w=None) == 1 and decode(p=None) == 1
    assert decode(F=0) == 1 and decode(stages=0) == 1 and decode(stages=8) == 1
    assert decode(ptrs={"window": fake + 4}) == 1 and decode(ptrs={"out": fake + 8}) == 1
    # a box leaving its frame, or empty
    for f, col, value in ((0, 0, 17), (0, 1, 11), (0, 2, 54), (0, 3, 39), (1, 2, 46), (1, 3, 38), (1, 0, 1), (3, 0, -1),
                          (3, 1, -1), (2, 2, 0), (2, 3, 0), (2, 2, -16), (3, 2, 1 << 40), (3, 0, 1 << 40)):
        assert decode(w=edit(window, (f, col), value)) == 1, (f, col, value)
    # the prefixes are the window's, not the frame's
    full = store.plan(picks)[4][0][3]
    assert not torch.equal(full[:2], prefix[:2]) and torch.equal(full[2], prefix[2])
    assert decode(p=full) == 1
    for row in range(3):
        assert decode(p=edit(prefix, (row, 0), 1)) == 1
        assert decode(p=edit(prefix, (row, 2), int(prefix[row, 2]) + 1)) == 1
        assert decode(p=edit(prefix, (row, 2), int(prefix[row, 2]) - 1)) == 1
    # output frames: in order, 16-byte aligned, no overlap, inside out_bytes
    assert decode(g=edit(geom, (2, 6), int(geom[2, 6]) + 8)) == 1            # off its 16 bytes
    assert decode(g=edit(geom, (2, 6), int(geom[2, 6]) - 16)) == 1           # overlaps frame 1
    assert decode(g=edit(geom, (1, 6), int(geom[2, 6]))) == 1                # frame 1 where frame 2 lies
    assert decode(g=edit(geom, (3, 6), (total + 15) & ~15)) == 1             # behind the end
    assert decode(g=edit(geom, (0, 6), -16)) == 1
    assert decode(out_bytes=total - 1) == 1
    # the coefficient blocks keep the full-frame layout
    assert decode(blocks=blocks - 1) == 1
    assert decode(g=edit(geom, (2, 5), int(geom[2, 5]) - 1)) == 1
    # the selection and the geometry, as coclr_jpeg_decode_store
    for bad in (-1, len(store), 1 << 40):
        assert decode(s=edit(sel, 1, bad)) == 1, bad
    assert decode(s=edit(sel, 1, 3)) == 1
    assert decode(g=edit(geom, (1, 0), int(geom[1, 0]) + 1)) == 1


def _plan(half, box, programs):
    return {"half": half, "box": box, "programs": programs}


def test_clip_frames_by_hand():
    T = 3
    flip = [(staging.AUGMENT_FLIP, 0.0)]
    two = _plan((0, 1), ((4, 5, 20, 10), (0, 0, 56, 40)), ([flip] * T, [[]] * T))
    one = _plan((1, 1), ((1, 2, 3, 4), (7, 8, 9, 10)), ([[]] * T, [flip] * T))
    ids = torch.tensor([[10, 11, 12, 13, 14, 15], [20, 20, 21, 22, 23, 23]])
    sel, boxes = staging.clip_frames(ids, [two, one], T)
    assert sel.dtype == torch.int64 and boxes.dtype == torch.int64
    assert sel.tolist() == [10, 11, 12, 13, 14, 15, 22, 23, 23, 22, 23, 23]             # ids 20, 21 are never decoded
    assert boxes.tolist() == [[4, 5, 20, 10]] * 3 + [[0, 0, 56, 40]] * 3 + [[1, 2, 3, 4]] * 3 + [[7, 8, 9, 10]] * 3
    first = _plan((0, 0), one["box"], one["programs"])
    sel, boxes = staging.clip_frames(ids[1:], [first], T)
    assert sel.tolist() == [20, 20, 21, 20, 20, 21] and boxes.tolist() == [[1, 2, 3, 4]] * 3 + [[7, 8, 9, 10]] * 3
    # the packed tensor, and a list of ids, will do
    packed = torch.stack([staging.pack_plan(two, T), staging.pack_plan(one, T)])
    sel2, boxes2 = staging.clip_frames(ids.tolist(), packed, T)
    assert sel2.tolist() == [10, 11, 12, 13, 14, 15, 22, 23, 23, 22, 23, 23] and boxes2.shape == (12, 4)
    for bad_ids, plans in ((ids[:, :5], [two, one]), (ids.to(torch.float32), [two, one]), (ids, [two]),
                           (ids.view(-1), [two, one]), (ids, [two, _plan((0, 2), one["box"], one["programs"])])):
        with pytest.raises(ValueError):
            staging.clip_frames(bad_ids, plans, T)


def test_cropped_tables_against_the_ragged_ones():
    T, S = 2, 16
    tt = staging.TrainTransform(S, T)
    rng, np_rng = random.Random(0), np.random.RandomState(0)
    sizes = [(56, 40), (45, 37)] * 3
    plans = [tt.draw(W, H, rng=rng, np_rng=np_rng) for W, H in sizes]
    assert {p["half"] for p in plans} == {(0, 1), (0, 0), (1, 1)}
    # the full frames, laid out as decode lays them out; the boxes, laid out as decode(boxes=) does
    samples, at = [], 0
    for W, H in sizes:
        samples.append((at, W, H))
        at += 2 * T * ((3 * W * H + 15) & ~15)
    clips, at = [], 0
    for p in plans:
        for c in range(2):
            w, h = p["box"][c][2:]
            clips.append((at, w, h))
            at += T * ((3 * w * h + 15) & ~15)
    want = staging.train_tables_ragged(plans, samples, T, S)
    got = staging.train_tables_cropped(plans, clips, T, S)
    for a, b in zip(got[1:], want[1:]):                                      # axis tables, programs, group size
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
    assert got[5] == 1                                                       # a gray clip: per-frame programs
    d, w = got[0], want[0]
    assert d.shape == w.shape == (12, 14) and d.dtype == torch.int32
    same = [0, 1, 4, 5, 6, 7, 8, 9]                                          # first frame, T, w, h and the table words
    assert torch.equal(d[:, same], w[:, same])
    k = 0
    for p, (_, W, H) in zip(plans, samples):
        for c in range(2):
            x0, y0, bw, bh = p["box"][c]
            assert w[k, 2:6].tolist() == [x0, y0, bw, bh] and w[k, 12:].tolist() == [W, H]
            assert d[k, 2:6].tolist() == [0, 0, bw, bh] and d[k, 12:].tolist() == [bw, bh]
            assert d[k, 10:12].tolist() == [clips[k][0], 0]
            k += 1
    # a clip that is not its box's size, and a clip too few
    with pytest.raises(ValueError):
        staging.train_tables_cropped(plans, [(o, w + 1, h) for o, w, h in clips], T, S)
    with pytest.raises(ValueError):
        staging.train_tables_cropped(plans, clips[:-1], T, S)
    # stage_train_clips_cropped checks the layout on the host before it touches the pixels
    def layout(gap, sizes_of):
        offs, hs, ws, at = [], [], [], 0
        for k, (_, w_, h_) in enumerate(clips):
            for t in range(T):
                w2, h2 = sizes_of(k, t, w_, h_)
                offs.append(at)
                hs.append(h2)
                ws.append(w2)
                at += ((3 * w2 * h2 + 15) & ~15) + gap
        return staging.RaggedFrames(torch.zeros(at, dtype=torch.uint8), offs, hs, ws)

    keep = lambda k, t, w_, h_: (w_, h_)                                     # noqa: E731
    spread = layout(16, keep)                                                # not at the ragged stride
    mixed = layout(0, lambda k, t, w_, h_: (w_, h_ - 1) if (k, t) == (3, 1) else (w_, h_))   # a clip of two sizes
    other = layout(0, lambda k, t, w_, h_: (w_ + 1, h_) if k == 5 else (w_, h_))             # a clip that is not its box
    good = layout(0, keep)
    short = staging.RaggedFrames(good.pixels, good.offset[:-1], good.height[:-1], good.width[:-1])
    for bad in (spread, mixed, other, short, good.pixels):
        with pytest.raises(ValueError):
            staging.stage_train_clips_cropped(bad, plans, S)
    assert [(int(o), int(w_), int(h_)) for o, w_, h_ in zip(good.offset[::T], good.width[::T], good.height[::T])] == clips


@pytest.fixture(scope="module")
def window_check(tmp_path_factory):
    """tools/jpeg_window_check.cpp built with the sanitizers, run once on every fixture and its boxes."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("jpeg_window")
    exe, cases, boxes = str(tmp / "jpeg_window_check"), str(tmp / "cases.bin"), str(tmp / "boxes.bin")
    # the sanitizer runtimes are linked statically: the program then does not care what else a host preloads
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "jpeg_window_check.cpp"), "-o", exe])
    J.write_core_check_cases(cases)
    WC.write_boxes(boxes)
    return subprocess.run([exe, cases, boxes], stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_host_build_windows_equal_the_golden_crops(window_check):
    out, err = window_check.stdout.decode(), window_check.stderr.decode()
    assert window_check.returncode == 0 and "ERROR" not in err and "runtime error" not in err, out + err
    line = next(l for l in out.splitlines() if "windows:" in l)
    windows, lanes, skipped, blocks, pixels, reads, failed = [int(v) for v in re.findall(r"\d+", line)]
    picks = WC.all_boxes()
    cases = J.cases()
    assert windows == 2 * len(picks) and failed == 0 and "differs" not in out
    assert lanes == sum(_lanes(cases[i], cb) for cb in (8, 64) for i, _ in picks)
    assert 0 < skipped < lanes and skipped > lanes // 4                      # skipping is real, and not everything
    assert pixels == 2 * sum(b[2] * b[3] for _, b in picks) and reads > pixels
    want = 0
    for i, box in picks:
        c = cases[i]
        hs, vs = c["sampling"]
        mx0, my0, mx1, my1 = WC.mcu_rect(c["height"], c["width"], c["ncomp"], hs, vs, box)
        want += (mx1 - mx0) * (my1 - my0) * WC.mcu_blocks(c["ncomp"], hs, vs)
    assert blocks == 2 * want
    assert "10 of 10 bad boxes refused" in out
