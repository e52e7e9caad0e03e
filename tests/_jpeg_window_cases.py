"""Shared by the windowed-decode tests (tests/test_gpu_jpeg_window.py, tests/test_jpeg_window_cpu.py): the fixed list of
pixel boxes every fixture of tests/golden/jpeg_frames.pt is decoded with, the boxes file tools/jpeg_window_check.cpp
reads, and the window arithmetic written out once more, independently of coclr_amd.jpeg, to count lanes with."""
import random
import struct

import _jpeg_cases as J

EDGES = (0, 1, 7, 8, 15, 16, 17)         # around the 8- and 16-pixel MCU and block boundaries
WIDTHS = (16, 32, 15, 17)                # the 16-byte store path of the colour stage, and just off it


def _clip(W, H, x0, y0, w, h):
    """The box cut to the frame; None when its corner lies outside."""
    if x0 < 0 or y0 < 0 or x0 >= W or y0 >= H:
        return None
    return (x0, y0, min(w, W - x0), min(h, H - y0))


def boxes(W, H, seed):
    """The boxes of one W x H fixture, (x0, y0, w, h), all inside the frame, in a fixed order."""
    out = [(0, 0, W, H)]
    out += [(0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1), (W // 2, H // 2, 1, 1)]
    for v in EDGES:
        out += [_clip(W, H, v, v, 11, 9), _clip(W, H, v, 0, 11, 9), _clip(W, H, 0, v, 11, 9)]
    for wd in WIDTHS:
        out += [_clip(W, H, 0, 2, wd, 6), _clip(W, H, 5, 1, wd, 7)]
    # ending at the right and bottom edges: the partial last MCU
    out += [_clip(W, H, max(0, W - 5), max(0, H - 3), 5, 3), _clip(W, H, max(0, W - 19), max(0, H - 18), 19, 18),
            (0, H - 1, W, 1), (W - 1, 0, 1, H)]
    rng = random.Random(seed)
    for _ in range(20):
        w, h = rng.randint(1, W), rng.randint(1, H)
        out.append((rng.randint(0, W - w), rng.randint(0, H - h), w, h))
    out = [b for b in out if b is not None]
    assert all(x0 >= 0 and y0 >= 0 and w >= 1 and h >= 1 and x0 + w <= W and y0 + h <= H for x0, y0, w, h in out)
    return out


def all_boxes():
    """[(fixture index, box)] over every fixture, in fixture order."""
    return [(i, b) for i, c in enumerate(J.cases()) for b in boxes(c["width"], c["height"], 1000 + i)]


def write_boxes(path):
    """The boxes of every fixture in the format tools/jpeg_window_check.cpp reads, in the cases file's order."""
    with open(path, "wb") as f:
        f.write(struct.pack("<ii", 0x4A505742, len(J.cases())))
        for i, c in enumerate(J.cases()):
            bs = boxes(c["width"], c["height"], 1000 + i)
            f.write(struct.pack("<i", len(bs)))
            for b in bs:
                f.write(struct.pack("<4i", *b))


def mcu_rect(H, W, ncomp, hs, vs, box):
    """(mx0, my0, mx1, my1), ends exclusive: the MCUs of the box's luma samples and of the chroma samples fancy
    upsampling reads for them, found by listing the samples."""
    x0, y0, w, h = box
    if ncomp == 1:
        hs = vs = 1
    cols, rows = set(), set()
    for x in (x0, x0 + w - 1):
        cols.add(x // (8 * hs))
        if ncomp == 3 and hs == 2:
            dw = -(-W // 2)
            cols |= {min(max(c, 0), dw - 1) // 8 for c in ((x >> 1) - 1, x >> 1, (x >> 1) + 1)}
    for y in (y0, y0 + h - 1):
        rows.add(y // (8 * vs))
        if ncomp == 3 and vs == 2:
            dh = -(-H // 2)
            rows |= {min(max(r, 0), dh - 1) // 8 for r in ((y >> 1) - 1, y >> 1, (y >> 1) + 1)}
    return min(cols), min(rows), max(cols) + 1, max(rows) + 1


def mcu_blocks(ncomp, hs, vs):
    return 1 if ncomp == 1 else hs * vs + 2


def block_mcus(H, W, ncomp, hs, vs):
    """Per block of a frame's coefficient storage (csrc/jpeg_core.h: jc_geom -- the luma plane row by row, then Cb,
    then Cr, each in whole MCUs) the linear index of the MCU it belongs to."""
    if ncomp == 1:
        hs = vs = 1
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    out = [(by // vs) * mcux + bx // hs for by in range(mcuy * vs) for bx in range(mcux * hs)]
    for _ in range(ncomp - 1):
        out += list(range(mcux * mcuy))
    return out
