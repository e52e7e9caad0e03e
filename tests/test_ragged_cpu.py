"""CPU tier of the ragged path -- batches whose videos differ in frame size: jpeg.cat_ragged / decode_ragged's host
side, staging.RaggedFrames, the three additive entry points' refusals before any launch, the host logic of
stage_train_clips_ragged / stage_classifier_clips_ragged against the reference's own fixtures through the doubles of
tests/ragged_harness.py, and the kernels' frame search and ragged addressing (csrc/jpeg_core.h) compiled for the host
under AddressSanitizer and UBSan (tools/jpeg_ragged_check.cpp).  Nothing here needs a GPU, nothing is preloaded into
Python, and the pointers that stand for device memory are never dereferenced: only refused calls are made."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

import _jpeg_cases as J
import cls_harness as CL
import jitter_harness as JH
import ragged_harness as RH
import train_harness as TH
from coclr_amd import _lib, jpeg, ops, staging

ROOT = J.ROOT
FAKE = 0x10000                                                # a non-null, 16-byte aligned stand-in, never dereferenced
NAMES = ("coclr_jpeg_decode_ragged", "coclr_resize_boxes_ragged_u8", "coclr_resize2_boxes_ragged")
MIXED = ("16x16_444_q50_ramp", "56x40_420_rst1", "17x33_gray_q50_ramp", "45x37_420_q100_noise")


def hp(t, ty=C.c_int32):
    return C.cast(t.data_ptr(), C.POINTER(ty))


def _mixed():
    packs = [jpeg.pack([J.raw(J.case(n))]) for n in MIXED]
    return packs, jpeg.cat_ragged(packs)


# ---- pack and container layout ----------------------------------------------------------------------------------------

def test_cat_ragged_layout():
    packs, (data, meta) = _mixed()
    assert data.dtype == torch.uint8 and meta.dtype == torch.int32 and meta.shape[0] == len(MIXED)
    width = max(m.shape[1] for _, m in packs)
    assert meta.shape[1] == width == 8 + jpeg.META_SEG + 12   # the rst1 frame has 12 restart segments
    at = 0
    for k, (d, m) in enumerate(packs):
        c = J.case(MIXED[k])
        hs, vs = c["sampling"]
        assert meta[k, :8].tolist() == [width, c["height"], c["width"], c["ncomp"], hs, vs, 0, 0]       # its own head
        assert int(meta[k, 8]) == at and int(meta[k, 9]) == d.numel()
        assert torch.equal(data[at:at + d.numel()], d)
        assert torch.equal(meta[k, 9:m.shape[1]], m[0, 9:]) and not bool(meta[k, m.shape[1]:].any())
        at += d.numel()
    assert at == data.numel()
    geo = jpeg.check_meta_ragged(data, meta)
    assert geo.tolist() == [[16, 16, 3, 1, 1], [40, 56, 3, 2, 2], [33, 17, 1, 1, 1], [37, 45, 3, 2, 2]]
    with pytest.raises(jpeg.Unsupported, match="differ"):     # the one-size functions keep refusing
        jpeg.cat(packs)
    with pytest.raises(ValueError):
        jpeg.check_meta(data, meta)
    with pytest.raises(ValueError):
        jpeg.cat_ragged([])


def test_cat_ragged_of_one_size_equals_cat():
    group = J.groups()[(40, 56, 3, (2, 2))]
    packs = [jpeg.pack([J.raw(c)]) for c in group]
    a, b = jpeg.cat(packs), jpeg.cat_ragged(packs)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _laid_out(offset, height, width, total):
    end = offset + 3 * height.to(torch.int64) * width.to(torch.int64)
    assert offset.dtype == torch.int64 and int(offset[0]) == 0
    assert bool((offset % 16 == 0).all())                     # aligned
    assert bool((offset[1:] >= end[:-1]).all())               # increasing, not overlapping
    assert bool((offset[1:] - end[:-1] < 16).all())           # and packed: only alignment padding between frames
    assert int(end[-1]) <= total


def test_ragged_frames_offsets():
    sizes = [(2, 57, 41), (1, 8, 96), (3, 40, 52), (1, 7, 9)]
    parts = [torch.from_numpy(TH.frames(n, H, W, 3 + k)) for k, (n, H, W) in enumerate(sizes)]
    rf = staging.ragged_from_frames(parts, device="cpu")
    assert len(rf) == 7 and rf.pixels.dim() == 1 and rf.pixels.dtype == torch.uint8
    assert rf.height.dtype == rf.width.dtype == torch.int32 and not rf.offset.is_cuda
    assert rf.height.tolist() == [57, 57, 8, 40, 40, 40, 7] and rf.width.tolist() == [41, 41, 96, 52, 52, 52, 9]
    _laid_out(rf.offset, rf.height, rf.width, rf.pixels.numel())
    assert int(rf.offset[1]) == (3 * 57 * 41 + 15) // 16 * 16            # 7011 bytes: padded to 7024
    flat = [f for p in parts for f in p]
    for i, want in enumerate(flat):
        assert torch.equal(rf.frame(i), want)
    with pytest.raises(IndexError):
        rf.frame(7)
    # the constructor holds what the kernels rely on
    for bad in ((rf.offset + 8, "misaligned"), (rf.offset.flip(0), "decreasing"),
                (torch.cat([rf.offset[:1], rf.offset[:-1]]), "overlapping")):
        with pytest.raises(ValueError):
            staging.RaggedFrames(rf.pixels, bad[0], rf.height, rf.width)
    with pytest.raises(ValueError):
        staging.RaggedFrames(rf.pixels[:-1], rf.offset, rf.height, rf.width)
    # decode_ragged's own layout, and its stages: whole frames by cumulative workspace bytes, the same output layout
    _, (data, meta) = _mixed()
    geo = jpeg.check_meta_ragged(data, meta)
    offset, total, stages, blocks = jpeg.ragged_plan(geo, 256 << 20)
    _laid_out(offset, geo[:, 0], geo[:, 1], total)
    assert [(k, e) for k, e, _, _ in stages] == [(0, 4)]
    nb = [ops.jpeg_workspace(*g)[1] // 64 for g in geo.tolist()]
    assert blocks == sum(nb) and stages[0][3][0].tolist() == [0, nb[0], sum(nb[:2]), sum(nb[:3]), sum(nb)]
    assert stages[0][2][:, 5].tolist() == stages[0][3][0, :-1].tolist() and stages[0][2][:, 6].tolist() == offset.tolist()
    small = jpeg.ragged_plan(geo, (nb[0] + nb[1]) * 192)
    assert [(k, e) for k, e, _, _ in small[2]] == [(0, 2), (2, 4)] and torch.equal(small[0], offset)
    assert small[2][1][2][:, 5].tolist() == [0, nb[2]] and small[2][1][2][:, 6].tolist() == offset[2:].tolist()
    assert small[3] == nb[0] + nb[1] and small[2][1][3].tolist()[0] == [0, nb[2], nb[2] + nb[3]]
    assert [(k, e) for k, e, _, _ in jpeg.ragged_plan(geo, (nb[0] + nb[1]) * 192 - 1)[2]] == [(0, 1), (1, 2), (2, 4)]
    one = jpeg.ragged_plan(geo, 1)
    assert [(k, e) for k, e, _, _ in one[2]] == [(0, 1), (1, 2), (2, 3), (3, 4)] and one[3] == max(nb)


# ---- host refusals -------------------------------------------------------------------------------------------------------

def test_decode_ragged_refuses_a_bad_meta_on_the_host():
    """The list of test_decode_refuses_a_bad_meta_on_the_host, with the bad word in row 1 (56 x 40, 4:2:0, restart
    interval 1), whose geometry differs from row 0's (16 x 16, 4:4:4)."""
    _, (data, meta) = _mixed()
    lo, n = int(meta[1, 8]), int(meta[1, 9])
    for word, value, why in ((8, data.numel(), "leave the buffer"), (9, data.numel() - lo + 1, "leave the buffer"),
                             (10, 5, "restart segments"), (11, 3, "restart segments"),
                             (8 + jpeg.META_SEG + 3, 1 << 20, "offset"), (8 + jpeg.META_QUANT, 256, "quantiser"),
                             (3, 4, "geometry"), (0, 7, "wide")):
        bad = meta.clone()
        bad[1, word] = value
        with pytest.raises(ValueError):                           # `why`, and before any device is touched
            jpeg.decode_ragged(data, bad)
    assert n > 0
    # a row whose geometry head is itself invalid: a sampling, a size and a component count the kernels do not take,
    # and the two spare words
    for word, value in ((4, 4), (5, 3), (1, 0), (2, 8193), (3, 2), (6, 1), (7, -1)):
        bad = meta.clone()
        bad[1, word] = value
        with pytest.raises(ValueError):
            jpeg.decode_ragged(data, bad)
    # a head that is valid but not the row's own: read as 16 x 16 4:4:4, row 1 has 4 MCUs and so not 12 segments
    bad = meta.clone()
    bad[1, 1:6] = meta[0, 1:6]
    with pytest.raises(ValueError, match="restart segments"):
        jpeg.decode_ragged(data, bad)
    with pytest.raises(ValueError):
        jpeg.decode_ragged(data[:-1].to(torch.int8), meta)
    with pytest.raises(ValueError):
        jpeg.decode_ragged(data, meta, chunk_bytes=7)


# ---- entry-point refusals before any launch ----------------------------------------------------------------------------

def test_jpeg_entry_point_rejects_before_any_launch():
    lib = _lib.load()
    _, (data, meta) = _mixed()
    geo = jpeg.check_meta_ragged(data, meta)
    offset, total, stages, blocks = jpeg.ragged_plan(geo, 256 << 20)
    _, _, geom, prefix = stages[0]
    host = meta[:, 8:].contiguous()
    F = host.shape[0]

    def call(m=host, g=geom, p=prefix, F=F, n=data.numel(), width=host.shape[1], stages=7, blocks=blocks,
             out_bytes=(total + 15) & ~15, chunk=0, ptrs=None):
        q = {"data": FAKE, "meta": FAKE, "geom": FAKE, "prefix": FAKE, "coefs": FAKE, "planes": FAKE, "out": FAKE,
             "status": FAKE}
        q.update(ptrs or {})
        return lib.coclr_jpeg_decode_ragged(
            q["data"], n, q["meta"], hp(m) if m is not None else None, F, width, q["geom"],
            hp(g, C.c_int64) if g is not None else None, q["prefix"], hp(p, C.c_int64) if p is not None else None,
            stages, q["coefs"], q["planes"], blocks, q["out"], out_bytes, q["status"], chunk, None)

    for name in ("data", "meta", "geom", "prefix", "coefs", "planes", "out", "status"):
        assert call(ptrs={name: None}) == 1, name
    assert call(m=None) == 1 and call(g=None) == 1 and call(p=None) == 1
    for name, by in (("coefs", 8), ("planes", 8), ("out", 8), ("geom", 4), ("prefix", 4), ("meta", 2)):
        assert call(ptrs={name: FAKE + by}) == 1, name          # misaligned
    assert call(F=0) == 1 and call(stages=0) == 1 and call(stages=8) == 1
    assert call(n=-1) == 1 and call(n=1 << 31) == 1 and call(width=jpeg.META_SEG) == 1
    assert call(chunk=7) == 1 and call(chunk=65537) == 1
    assert call(n=data.numel() - 1) == 1                        # the last frame's bytes leave the buffer
    assert call(blocks=blocks - 1) == 1                         # the last frame's blocks leave the workspace
    assert call(out_bytes=total - 1) == 1                       # its pixels leave the output

    def table(row, col, value):
        g = geom.clone()
        g[row, col] = value
        return g

    assert call(g=table(1, 4, 1)) == 1                          # 2x1 is no geometry of a 12-segment frame: per frame
    assert call(g=table(1, 3, 4)) == 1 and call(g=table(2, 2, 3)) == 1 and call(g=table(0, 0, 0)) == 1
    assert call(g=table(3, 1, 8193)) == 1
    assert call(g=table(2, 5, int(geom[2, 5]) - 1)) == 1        # coefficients overlap the frame before
    assert call(g=table(2, 5, int(geom[1, 5]))) == 1
    assert call(g=table(1, 5, int(geom[3, 5]))) == 1            # decreasing: frame 2 starts below frame 1's end
    assert call(g=table(2, 6, int(geom[2, 6]) - 16)) == 1       # output overlaps the frame before
    assert call(g=table(2, 6, int(geom[2, 6]) + 8)) == 1        # misaligned first byte
    assert call(g=table(1, 6, int(geom[3, 6]))) == 1            # decreasing
    assert call(g=table(3, 6, int(geom[3, 6]) + 16)) == 1       # the last frame leaves the output
    assert call(g=table(0, 5, -1)) == 1 and call(g=table(0, 6, -16)) == 1

    def pre(row, col, value):
        p = prefix.clone()
        p[row, col] = value
        return p

    assert call(p=pre(0, 0, 1)) == 1 and call(p=pre(1, 0, 16)) == 1            # a prefix starts at 0
    assert call(p=pre(0, 2, int(prefix[0, 2]) + 1)) == 1                      # disagrees with the geometry table
    assert call(p=pre(1, 3, int(prefix[1, 3]) - 1)) == 1
    assert call(p=pre(0, F, int(prefix[0, F]) + 64)) == 1 and call(p=pre(1, F, int(prefix[1, F]) + 64)) == 1

    def changed(row, word, value):
        m = host.clone()
        m[row, word] = value
        return m

    lo = int(host[1, 0])
    assert call(m=changed(1, 0, data.numel())) == 1 and call(m=changed(1, 1, data.numel() - lo + 1)) == 1
    assert call(m=changed(1, 2, 5)) == 1 and call(m=changed(1, 3, 13)) == 1 and call(m=changed(1, 3, 0)) == 1
    assert call(m=changed(0, 3, 2)) == 1                        # two segments without an interval
    assert call(m=changed(1, jpeg.META_SEG + 5, 0)) == 1        # offsets must not decrease
    assert call(m=changed(2, jpeg.META_QUANT + 3, 256)) == 1 and call(m=changed(3, jpeg.META_HUFF + 3, 70000)) == 1


def _train_case():
    """Two samples, T = 1: 8 x 96 frames then 24 x 192 frames (H x W), as stage_train_clips_ragged lays them out."""
    frames = staging.ragged_from_frames([torch.zeros(2, 8, 96, 3, dtype=torch.uint8),
                                         torch.zeros(2, 24, 192, 3, dtype=torch.uint8)], device="cpu")
    plans = [{"half": (0, 1), "box": ((0, 0, 96, 8), (10, 1, 50, 6)), "programs": ([[]], [[]])},
             {"half": (0, 1), "box": ((0, 0, 192, 24), (100, 4, 80, 20)), "programs": ([[]], [[]])}]
    samples = staging._ragged_samples(frames, 2, 2, None)
    return frames, plans, samples


def test_boxes_entry_point_rejects_before_any_launch():
    lib = _lib.load()
    frames, plans, samples = _train_case()
    desc, xtab, ytab, _, _, _ = staging.train_tables_ragged(plans, samples, 1, 16)
    assert tuple(desc.shape) == (4, 14) and desc[:, 10].tolist() == [0, 2304, 4608, 4608 + 13824]
    assert desc[:, 12:].tolist() == [[96, 8]] * 2 + [[192, 24]] * 2
    nbytes = frames.pixels.numel()

    def call(d=desc, nbytes=nbytes, n=4, T=1, S=16, xlen=xtab.numel(), ylen=ytab.numel(), ptrs=None):
        q = {"frames": FAKE, "desc": FAKE, "xtab": FAKE, "ytab": FAKE, "out": FAKE}
        q.update(ptrs or {})
        return lib.coclr_resize_boxes_ragged_u8(q["frames"], nbytes, q["desc"], hp(d) if d is not None else None, n, T,
                                                S, q["xtab"], xlen, q["ytab"], ylen, q["out"], None)

    def changed(row, col, value):
        d = desc.clone()
        d[row, col] = value
        return d

    for name in ("frames", "desc", "xtab", "ytab", "out"):
        assert call(ptrs={name: None}) == 1, name
    assert call(d=None) == 1
    for name, by in (("frames", 8), ("xtab", 8), ("ytab", 4), ("desc", 2)):
        assert call(ptrs={name: FAKE + by}) == 1, name          # misaligned
    assert call(nbytes=0) == 1 and call(n=0) == 1 and call(T=0) == 1 and call(S=0) == 1 and call(S=513) == 1
    assert call(nbytes=nbytes - 1) == 1                         # the last clip's frame leaves the buffer
    assert call(d=changed(1, 10, 2304 + 8)) == 1                # a misaligned offset
    assert call(d=changed(0, 10, -16)) == 1 and call(d=changed(0, 11, -1)) == 1
    assert call(d=changed(3, 10, nbytes)) == 1 and call(d=changed(3, 11, 1)) == 1          # offsets past the end
    assert call(d=changed(0, 12, 0)) == 1 and call(d=changed(0, 13, 0)) == 1
    assert call(T=2) == 1 and call(d=changed(2, 1, 2)) == 1     # frames != T
    # a box inside the batch's largest frame (192 x 24) and outside its own (96 x 8)
    assert call(d=changed(0, 4, 97)) == 1 and call(d=changed(0, 2, 1)) == 1
    assert call(d=changed(1, 5, 8)) == 1 and call(d=changed(1, 3, 3)) == 1 and call(d=changed(0, 5, 9)) == 1
    assert call(d=changed(1, 2, 96)) == 1 and call(d=changed(1, 2, -1)) == 1
    # the frame taken for a larger one than the buffer holds
    assert call(d=changed(3, 13, 25)) == 1
    assert call(d=changed(0, 8, 65)) == 1 and call(d=changed(0, 6, 2)) == 1 and call(xlen=16) == 1


def test_resize2_entry_point_rejects_before_any_launch():
    lib = _lib.load()
    size, S, T = 24, 16, 2
    frames = staging.ragged_from_frames([torch.zeros(2, 40, 52, 3, dtype=torch.uint8),
                                         torch.zeros(2, 24, 192, 3, dtype=torch.uint8)], device="cpu")
    (ow, oh), win = staging.fallback_geometry(192, 24, size)
    plans = [{"form": "box", "region": (3, 8, 24, 25), "resample": (size, size), "window": (0, 0), "program": []},
             {"form": "fallback", "region": (0, 0, 192, 24), "resample": (ow, oh), "window": win, "program": []}]
    samples = staging._ragged_samples(frames, 2, T, None)
    desc, xtab, ytab, tab2, _, _, direct = staging.classifier_tables_ragged(plans, samples, T, S, size)
    assert tuple(desc.shape) == (2, 18) and direct and desc[:, 14:].tolist() == [[0, 0, 52, 40], [12480, 0, 192, 24]]
    nbytes = frames.pixels.numel()
    mean = (C.c_float * 3)(0.5, 0.5, 0.5)

    def call(d=desc, nbytes=nbytes, n=2, T=T, size=size, S=S, taps2=tab2.shape[0] - 1, ptrs=None):
        q = {"frames": FAKE, "desc": FAKE, "xtab": FAKE, "ytab": FAKE, "tab2": FAKE, "out8": FAKE, "out": None}
        q.update(ptrs or {})
        return lib.coclr_resize2_boxes_ragged(q["frames"], nbytes, q["desc"], hp(d) if d is not None else None, n, T,
                                              size, S, q["xtab"], xtab.numel(), q["ytab"], ytab.numel(), q["tab2"],
                                              tab2.numel(), taps2, mean, mean, q["out8"], q["out"], None)

    def changed(row, col, value):
        d = desc.clone()
        d[row, col] = value
        return d

    for name in ("frames", "desc", "xtab", "ytab", "tab2", "out8"):
        assert call(ptrs={name: None}) == 1, name
    assert call(d=None) == 1 and call(ptrs={"out": FAKE}) == 1                # both outputs
    for name, by in (("frames", 8), ("xtab", 8), ("ytab", 4), ("tab2", 8), ("desc", 2)):
        assert call(ptrs={name: FAKE + by}) == 1, name
    assert call(nbytes=0) == 1 and call(n=0) == 1 and call(T=0) == 1 and call(size=225) == 1 and call(taps2=0) == 1
    assert call(nbytes=nbytes - 1) == 1
    assert call(d=changed(1, 14, 12480 + 8)) == 1 and call(d=changed(0, 14, -16)) == 1 and call(d=changed(0, 15, -1)) == 1
    assert call(d=changed(1, 14, nbytes)) == 1 and call(d=changed(1, 15, 1)) == 1
    assert call(d=changed(0, 16, 0)) == 1 and call(d=changed(0, 17, 0)) == 1 and call(d=changed(1, 17, 25)) == 1
    assert call(T=1) == 1
    # a region inside the batch's largest frame (192 wide) and outside its own (52 x 40)
    assert call(d=changed(0, 4, 52)) == 1 and call(d=changed(0, 2, 30)) == 1 and call(d=changed(0, 5, 33)) == 1
    assert call(d=changed(1, 5, 25)) == 1                        # 40 rows would fit frame 0, not its own 24
    assert call(d=changed(1, 8, int(desc[1, 8]) + 200)) == 1     # the window leaves the resample


# ---- ABI -----------------------------------------------------------------------------------------------------------------

def test_abi_is_additive_and_exported():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "coclr_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\bint\s+(coclr_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (coclr_[a-z0-9_]+)", out))
    for name in NAMES:
        assert name in declared and name in exported and name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(ops, name[len("coclr_"):])
    assert lib.coclr_abi_version() == _lib.ABI_VERSION == 26
    assert text.count("Additive: the ABI number stays 25") >= 3 + 3


# ---- reference parity through the CPU harness ----------------------------------------------------------------------------

@pytest.mark.parametrize("img_dim", [16, 24])
def test_classifier_fixture_as_one_ragged_batch(img_dim, monkeypatch):
    RH.install(monkeypatch)
    monkeypatch.delenv("COCLR_CLS_FUSED", raising=False)
    gold = CL.golden()
    size, T = gold["size"], gold["seq_len"]
    batch = RH.cls_batches()[img_dim]
    sizes = {tuple(run["frames"].shape[1:3]) for run, _ in batch}
    assert sizes == ({(40, 52), (8, 96), (24, 192)} if img_dim == 16 else {(40, 52), (8, 96)})
    frames = staging.ragged_from_frames([run["frames"] for run, _ in batch], device="cpu")
    plans = [plan for _, plan in batch]
    out = staging.stage_classifier_clips_ragged(frames, plans, img_dim, size=size)
    assert out.shape == (len(batch), 3, T, img_dim, img_dim)
    assert RH.CALLS == [("resize2", len(batch), T, "u8")] and [c[0] for c in TH.CALLS] == ["augment"]
    for b, (run, _) in enumerate(batch):
        want = JH.levels_expected(run["out"].numpy(), gold["levels"], T)
        assert torch.equal(out[b:b + 1], want), (run["seed"], run["set"])
    packed = torch.stack([staging.pack_cls_plan(p) for p in plans])
    assert torch.equal(staging.stage_classifier_clips_ragged(frames, packed, img_dim, size=size, T=T), out)
    # validation-like batch: no programs, one launch writes fp32
    del RH.CALLS[:], TH.CALLS[:]
    plain = [dict(p, program=[]) for p in plans]
    direct = staging.stage_classifier_clips_ragged(frames, plain, img_dim, size=size)
    assert RH.CALLS == [("resize2", len(batch), T, "f32")] and TH.CALLS == []
    for b, (run, _) in enumerate(batch):
        assert torch.equal(direct[b:b + 1], CL.chain_reference(run["frames"][None].numpy(), [plain[b]], size, img_dim))
    # `first`: the samples in another order
    order = list(reversed(range(len(batch))))
    again = staging.stage_classifier_clips_ragged(frames, [plans[b] for b in order], img_dim, size=size, T=T,
                                                  first=[b * T for b in order])
    assert torch.equal(again, out[order])
    shapes = [tuple(run["frames"].shape[1:3]) for run, _ in batch]
    k = next(b for b in range(1, len(batch)) if shapes[b] != shapes[b - 1])
    with pytest.raises(ValueError, match="differ in size"):      # a sample across two videos
        staging.stage_classifier_clips_ragged(frames, plans[:1], img_dim, size=size, T=T, first=[k * T - 1])
    with pytest.raises(ValueError, match="leaves"):              # a plan drawn for another sample's frame
        staging.stage_classifier_clips_ragged(frames, [plans[0]] * len(batch), img_dim, size=size)
    monkeypatch.setenv("COCLR_CLS_FUSED", "0")                   # the chained form cannot express the fallback
    with pytest.raises(ValueError, match="fallback"):
        staging.stage_classifier_clips_ragged(frames, plans, img_dim, size=size)


def test_training_batch_ragged(monkeypatch):
    RH.install(monkeypatch)
    batch, S, T = RH.train_batch()
    assert [tuple(f.shape[1:3]) for f, _ in batch[-3:]] == [(8, 96), (57, 41), (24, 192)]
    (x0, y0, w, h) = batch[-2][1]["box"][0]
    assert x0 + w == 41 and y0 + h == 57                         # touches its own right and bottom edge
    frames = staging.ragged_from_frames([f for f, _ in batch], device="cpu")
    plans = [p for _, p in batch]
    out = staging.stage_train_clips_ragged(frames, plans, S)
    assert out.shape == (len(batch), 2, 3, T, S, S)
    assert RH.CALLS == [("boxes", 2 * len(batch), T)] and [c[0] for c in TH.CALLS] == ["augment"]
    for b, (f, plan) in enumerate(batch):
        assert torch.equal(out[b:b + 1], TH.chain_reference(f[None].numpy(), [plan], S)), b
    gold = TH.golden()
    for b, run in enumerate(gold["runs"]):                       # and the reference's own recorded bytes
        assert torch.equal(out[b], TH.levels_expected(run["out"].numpy(), gold["levels"], T)), run["seed"]
    packed = torch.stack([staging.pack_plan(p, T) for p in plans])
    assert torch.equal(staging.stage_train_clips_ragged(frames, packed, S), out)
    order = [8, 0, 7, 3]
    again = staging.stage_train_clips_ragged(frames, [plans[b] for b in order], S, first=[b * 2 * T for b in order])
    assert torch.equal(again, out[order])
    with pytest.raises(ValueError, match="differ in size"):
        staging.stage_train_clips_ragged(frames, plans[:1], S, first=[6 * 2 * T - 1])
    with pytest.raises(ValueError, match="leaves"):
        staging.stage_train_clips_ragged(frames, [plans[0]] * len(batch), S)
    with pytest.raises(ValueError):
        staging.stage_train_clips_ragged(frames, plans + plans[:1], S)       # more samples than frames
    with pytest.raises(ValueError):
        staging.stage_train_clips_ragged(torch.zeros(6, 8, 8, 3, dtype=torch.uint8), plans[:1], S)


# ---- the host program under sanitizers -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ragged_check(tmp_path_factory):
    """tools/jpeg_ragged_check.cpp built with the sanitizers, run once on every fixture as one mixed batch."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("jpeg_ragged")
    exe, cases = str(tmp / "jpeg_ragged_check"), str(tmp / "cases.bin")
    # the sanitizer runtimes are linked statically: the program then does not care what else a host preloads
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "jpeg_ragged_check.cpp"), "-o", exe])
    J.write_core_check_cases(cases)
    return subprocess.run([exe, cases], stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_host_build_finds_every_lanes_frame(ragged_check):
    out, err = ragged_check.stdout.decode(), ragged_check.stderr.decode()
    m = re.search(r"(\d+) searches, (\d+) wrong", out)
    assert m and int(m.group(1)) == 4 and int(m.group(2)) == 0, out + err


def test_host_build_decodes_the_mixed_batch_exactly(ragged_check):
    out, err = ragged_check.stdout.decode(), ragged_check.stderr.decode()
    assert ragged_check.returncode == 0 and "ERROR" not in err and "runtime error" not in err, out + err
    m = re.search(r"(\d+) frames in one batch, (\d+) failed, (\d+) skipped, status (\d+); (\d+) bytes between frames, "
                  r"(\d+) touched", out)
    assert m and int(m.group(1)) == len(J.cases()) and [int(m.group(k)) for k in (2, 3, 4, 6)] == [0, 0, 0, 0], out
    assert int(m.group(5)) > 0                                   # there was padding to leave alone
