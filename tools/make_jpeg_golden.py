"""Writes tests/golden/jpeg_frames.pt: small JPEG files as PIL (libjpeg-turbo) encodes them and the bytes
`Image.open(BytesIO(raw)).convert('RGB')` returns for each -- what dataset/lmdb_dataset.py:37-38 of the reference
hands to its transforms, and what coclr_amd.jpeg.decode must reproduce exactly.

    python tools/make_jpeg_golden.py

PIL is needed here only: no GPU test imports it to read the fixture.  Per case the fixture also records what PIL
itself reports about the file (size, sampling, table counts) and the restart interval asked of the encoder, for the
parser's test (the Huffman table counts are libjpeg's: one DC / AC pair for luma, one for chroma).  `refusals` are
files the decoder must refuse, each with a word of the reason.

The cases are the smallest at which each piece can go wrong: whole and partial MCUs both ways, a frame smaller
than one MCU, every sampling, quality 50 and 100 (quantiser 1, 16-bit codes, the range table's wrap), smooth and
noise content (noise reaches the 63rd coefficient and the 16-zero run symbol), per-image Huffman tables, restart
intervals of one MCU (12 segments: the marker number wraps) and of one MCU row, and one 320 x 240 frame."""
import io
import os

import numpy as np
import PIL
import torch
from PIL import Image, JpegImagePlugin, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "jpeg_frames.pt")

SIZES = ((16, 16), (7, 9), (45, 37), (56, 40), (17, 33))            # W x H
MODES = (("444", "4:4:4", (1, 1)), ("422", "4:2:2", (2, 1)), ("420", "4:2:0", (2, 2)), ("gray", None, (1, 1)))


def content(kind, W, H, seed):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ramp = np.stack([xx * 255 / max(W - 1, 1), yy * 255 / max(H - 1, 1), (xx + yy) * 255 / max(W + H - 2, 1)], -1)
    rng = np.random.RandomState(seed)
    if kind == "ramp":
        img = ramp
    elif kind == "noise":
        img = rng.randint(0, 256, size=(H, W, 3)).astype(np.float64)
    else:                                                             # smooth content plus mild noise
        img = 0.5 * ramp + 64 + 40 * np.sin(xx / 17.0)[:, :, None] + rng.normal(0, 6, size=(H, W, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def decoded(raw):
    return np.array(Image.open(io.BytesIO(raw)).convert("RGB"))


def encode(pixels, sub, **kw):
    im = Image.fromarray(pixels if sub is not None else pixels[:, :, 1])
    buf = io.BytesIO()
    if sub is not None:
        kw["subsampling"] = sub
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


def case(name, pixels, sub, sampling, restart=0, **kw):
    raw = encode(pixels, sub, **kw)
    im = Image.open(io.BytesIO(raw))
    im.load()
    H, W = pixels.shape[:2]
    if sub is not None:
        assert JpegImagePlugin.get_sampling(im) == {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}[sub]
    return {"name": name, "raw": torch.frombuffer(bytearray(raw), dtype=torch.uint8), "rgb": torch.from_numpy(decoded(raw)),
            "width": W, "height": H, "ncomp": 1 if sub is None else 3, "sampling": sampling,
            "restart_interval": restart, "quant_tables": len(im.quantization),
            "dc_tables": 1 if sub is None else 2, "ac_tables": 1 if sub is None else 2}     # libjpeg: luma + chroma


def patch_sampling(raw, value):
    """The same file with the luma sampling byte of its SOF0 set to `value` (PIL cannot encode h1v2 or h4v1)."""
    at = raw.index(b"\xff\xc0")
    assert raw[at + 9] == 3                                           # three components; luma's factors at +11
    return raw[:at + 11] + bytes([value]) + raw[at + 12:]


def main():
    assert features.check_feature("libjpeg_turbo"), "the golden is libjpeg-turbo's decoder"
    cases, seed = [], 0
    for W, H in SIZES:
        for tag, sub, sampling in MODES:
            kinds = ((50, "ramp"), (100, "noise")) + (((50, "noise"), (100, "ramp")) if (W, H) == (45, 37) else ())
            for quality, kind in kinds:
                seed += 1
                cases.append(case("%dx%d_%s_q%d_%s" % (W, H, tag, quality, kind), content(kind, W, H, seed), sub,
                                  sampling, quality=quality))
    W, H = 56, 40
    noise = content("noise", W, H, 1001)
    cases.append(case("56x40_420_optimize", noise, "4:2:0", (2, 2), quality=75, optimize=True))
    cases.append(case("56x40_420_rst1", noise, "4:2:0", (2, 2), restart=1, quality=75, restart_marker_blocks=1))
    cases.append(case("56x40_444_rst1", noise, "4:4:4", (1, 1), restart=1, quality=90, restart_marker_blocks=1))
    cases.append(case("56x40_420_rstrow", noise, "4:2:0", (2, 2), restart=4, quality=50, restart_marker_rows=1))
    cases.append(case("56x40_422_rst2", noise, "4:2:2", (2, 1), restart=2, quality=75, restart_marker_blocks=2))
    cases.append(case("320x240_420_q75", content("mild", 320, 240, 2001), "4:2:0", (2, 2), quality=75))
    assert sum(c["raw"][:].numpy().tobytes().count(b"\xff\xd0") for c in cases if c["name"] == "56x40_420_rst1") >= 1

    good = encode(content("mild", 32, 24, 3001), "4:2:0", quality=75)
    sos = good.index(b"\xff\xda")
    cmyk = io.BytesIO()
    Image.fromarray(content("noise", 16, 16, 3002)).convert("CMYK").save(cmyk, "JPEG", quality=75)
    refusals = [
        ("progressive", encode(content("mild", 32, 24, 3003), "4:2:0", quality=75, progressive=True), "progressive"),
        ("cmyk", cmyk.getvalue(), "4 components"),
        ("cut_before_sos", good[:sos], "past the buffer"),
        ("cut_in_segment", good[:sos - 7], "past the buffer"),
        ("no_eoi", good[:-2], "no EOI"),
        ("h1v2", patch_sampling(good, 0x12), "sampling"),
        ("h4v1", patch_sampling(good, 0x41), "sampling"),
    ]
    fix = {"pil": PIL.__version__, "libjpeg_turbo": features.version_feature("libjpeg_turbo"), "cases": cases,
           "refusals": [{"name": n, "raw": torch.frombuffer(bytearray(r), dtype=torch.uint8), "reason": why}
                        for n, r, why in refusals]}
    torch.save(fix, OUT)
    print("wrote %s (%d bytes, %d cases)" % (OUT, os.path.getsize(OUT), len(cases)))
    assert os.path.getsize(OUT) <= 600000


if __name__ == "__main__":
    main()
