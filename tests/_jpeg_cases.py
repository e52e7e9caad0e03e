"""Shared by the JPEG tests: the golden fixture (tests/golden/jpeg_frames.pt, written by tools/make_jpeg_golden.py),
loaded once, and the cases file tools/jpeg_core_check.cpp reads."""
import functools
import os
import struct

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_frames.pt")

CORRUPTED = ("45x37_420_q100_noise", "56x40_420_rst1", "17x33_gray_q50_ramp")     # damaged by the host check


@functools.lru_cache(maxsize=None)
def golden():
    return torch.load(GOLDEN)


def cases():
    return golden()["cases"]


def case(name):
    return next(c for c in cases() if c["name"] == name)


def names():
    return [c["name"] for c in cases()]


def raw(c):
    return c["raw"].numpy().tobytes()


def groups():
    """The fixtures of one (H, W, components, sampling): what one decode call can take together."""
    out = {}
    for c in cases():
        out.setdefault((c["height"], c["width"], c["ncomp"], tuple(c["sampling"])), []).append(c)
    return out


def write_core_check_cases(path):
    """Every fixture, packed as coclr_amd.jpeg.pack packs it, in the format of tools/jpeg_core_check.cpp."""
    from coclr_amd import jpeg
    with open(path, "wb") as f:
        f.write(struct.pack("<ii", 0x4A504731, len(cases())))
        for c in cases():
            data, meta = jpeg.pack([raw(c)])
            row = meta[0, 8:].contiguous()
            hs, vs = c["sampling"]
            f.write(struct.pack("<8i", c["height"], c["width"], c["ncomp"], hs, vs, row.numel(), data.numel(),
                                int(c["name"] in CORRUPTED)))
            f.write(row.numpy().tobytes())
            f.write(data.numpy().tobytes())
            f.write(c["rgb"].contiguous().numpy().tobytes())
