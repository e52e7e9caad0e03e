"""CPU tier of the JPEG decoder: the host-side parser and its refusals, the C ABI's device-free entry points, and
the kernels' own arithmetic (coclr_amd/csrc/jpeg_core.h) compiled for the host under AddressSanitizer and UBSan --
every fixture to exactly PIL's bytes, and damaged streams in bounds (tools/jpeg_core_check.cpp).  Nothing here
needs a GPU, nothing is preloaded into Python, and no damaged stream is ever sent to a GPU."""
import ctypes as C
import io
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _jpeg_cases as J
from coclr_amd import _lib, jpeg, ops

ROOT = J.ROOT


@pytest.mark.parametrize("name", J.names())
def test_parse_reports_what_the_golden_records(name):
    c = J.case(name)
    info = jpeg.parse(J.raw(c))
    assert (info["width"], info["height"], info["ncomp"]) == (c["width"], c["height"], c["ncomp"])
    assert tuple(info["sampling"]) == tuple(c["sampling"])
    assert info["restart_interval"] == c["restart_interval"]
    assert (len(info["quant_tables"]), len(info["dc_tables"]), len(info["ac_tables"])) == \
        (c["quant_tables"], c["dc_tables"], c["ac_tables"])
    hs, vs = c["sampling"]
    mcus = -(-c["width"] // (8 * hs)) * -(-c["height"] // (8 * vs))
    ri = c["restart_interval"]
    assert len(info["segments"]) == (-(-mcus // ri) if ri else 1)
    start, end = info["scan"]
    raw = J.raw(c)
    assert raw[end:end + 2] == b"\xff\xd9" and raw[start - 3:start] == b"\x00\x3f\x00"
    for k, at in enumerate(info["segments"][1:]):          # each segment starts behind RST(k mod 8)
        assert raw[start + at - 2:start + at] == bytes([0xFF, 0xD0 + k % 8])
    for bits, vals in info["dc"] + info["ac"]:
        assert len(bits) == 16 and int(sum(bits)) == len(vals)
    assert all(q.shape == (64,) and q.min() >= 1 for q in info["quant"])


def test_restart_fixture_wraps_the_marker_number():
    info = jpeg.parse(J.raw(J.case("56x40_420_rst1")))
    assert len(info["segments"]) == 12 and info["restart_interval"] == 1


def test_quality_100_has_unit_quantisers_and_optimize_its_own_tables():
    assert all(int(q.max()) == 1 for q in jpeg.parse(J.raw(J.case("45x37_420_q100_noise")))["quant"])
    std = jpeg.parse(J.raw(J.case("56x40_420_q50_ramp")))
    opt = jpeg.parse(J.raw(J.case("56x40_420_optimize")))
    assert len(opt["ac"][0][1]) < len(std["ac"][0][1]) == 162


@pytest.mark.parametrize("k", range(7))
def test_refusals_name_their_reason(k):
    r = J.golden()["refusals"][k]
    with pytest.raises(jpeg.Unsupported, match=re.escape(r["reason"])):
        jpeg.parse(r["raw"].numpy().tobytes())
    with pytest.raises(ValueError):                           # Unsupported is a ValueError; pack refuses alike
        jpeg.pack([r["raw"].numpy().tobytes()])


def test_refusal_fixture_covers_the_issue_list():
    assert [r["name"] for r in J.golden()["refusals"]] == ["progressive", "cmyk", "cut_before_sos", "cut_in_segment",
                                                           "no_eoi", "h1v2", "h4v1"]


def _with_segment(raw, marker, payload, before=b"\xff\xdb"):
    at = raw.index(before)
    return raw[:at] + b"\xff" + bytes([marker]) + (len(payload) + 2).to_bytes(2, "big") + payload + raw[at:]


def test_header_refusals_built_from_a_good_file():
    good = J.raw(J.case("16x16_444_q50_ramp"))
    jpeg.parse(good)
    adobe = b"Adobe" + bytes([0, 100, 0, 0, 0, 0])
    with pytest.raises(jpeg.Unsupported, match="transform 0"):
        jpeg.parse(_with_segment(good, 0xEE, adobe + b"\x00"))
    jpeg.parse(_with_segment(good, 0xEE, adobe + b"\x01"))       # transform 1 is YCbCr
    sof = good.index(b"\xff\xc0")
    with pytest.raises(jpeg.Unsupported, match="12-bit"):
        jpeg.parse(good[:sof + 4] + b"\x0c" + good[sof + 5:])
    with pytest.raises(jpeg.Unsupported, match="arithmetic"):
        jpeg.parse(good[:sof + 1] + b"\xc9" + good[sof + 2:])
    with pytest.raises(jpeg.Unsupported, match="DNL"):
        jpeg.parse(_with_segment(good, 0xDC, b"\x00\x10"))
    dht = good.index(b"\xff\xc4")
    ln = int.from_bytes(good[dht + 2:dht + 4], "big")
    with pytest.raises(jpeg.Unsupported, match="missing DC Huffman table"):
        jpeg.parse(good[:dht] + good[dht + 2 + ln:])
    eoi = len(good) - 2
    sos = good.index(b"\xff\xda")
    with pytest.raises(jpeg.Unsupported, match="several scans"):
        jpeg.parse(good[:eoi] + good[sos:])
    with pytest.raises(jpeg.Unsupported, match="no SOI"):
        jpeg.parse(good[2:])


def test_pack_and_cat_layout():
    group = J.groups()[(40, 56, 3, (2, 2))]
    packs = [jpeg.pack([J.raw(c)]) for c in group]
    data, meta = jpeg.cat(packs)
    both = jpeg.pack([J.raw(c) for c in group])
    assert torch.equal(data, both[0]) and torch.equal(meta, both[1])
    assert meta.dtype == torch.int32 and data.dtype == torch.uint8 and meta.shape[0] == len(group)
    assert meta.shape[1] == 8 + jpeg.META_SEG + 12               # the widest frame has 12 restart segments
    assert meta[:, 1:6].unique(dim=0).tolist() == [[40, 56, 3, 2, 2]]
    assert int(meta[-1, 8] + meta[-1, 9]) == data.numel()
    assert jpeg.check_meta(data, meta) == (40, 56, 3, 2, 2)
    with pytest.raises(jpeg.Unsupported, match="differ"):
        jpeg.pack([J.raw(group[0]), J.raw(J.case("16x16_444_q50_ramp"))])
    with pytest.raises(jpeg.Unsupported, match="differ"):
        jpeg.cat([packs[0], jpeg.pack([J.raw(J.case("56x40_444_rst1"))])])


def test_decode_refuses_a_bad_meta_on_the_host():
    data, meta = jpeg.pack([J.raw(J.case("56x40_420_rst1"))])
    for word, value, why in ((8, data.numel(), "leave the buffer"), (9, data.numel() + 1, "leave the buffer"),
                             (10, 5, "restart segments"), (11, 3, "restart segments"),
                             (8 + jpeg.META_SEG + 3, 1 << 20, "offset"), (8 + jpeg.META_QUANT, 256, "quantiser"),
                             (3, 4, "geometry"), (0, 7, "wide")):
        bad = meta.clone()
        bad[0, word] = value
        with pytest.raises(ValueError):                           # `why`, and before any device is touched
            jpeg.decode(data, bad)
    with pytest.raises(ValueError):
        jpeg.decode(data[:-1].to(torch.int8), meta)


def test_abi_is_additive_and_exported():
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "coclr_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\bint\s+(coclr_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (coclr_[a-z0-9_]+)", out))
    for name in ("coclr_jpeg_workspace", "coclr_jpeg_decode"):
        assert name in declared and name in exported and name in _lib.EXPORTED_SYMBOLS
    assert declared == exported == set(_lib.EXPORTED_SYMBOLS)
    assert lib.coclr_abi_version() == _lib.ABI_VERSION == 26


def test_workspace_without_a_device():
    assert ops.jpeg_workspace(240, 320, 3, 2, 2) == (1800 * 128, 1800 * 64)
    assert ops.jpeg_workspace(9, 7, 3, 2, 2) == (6 * 128, 6 * 64)
    assert ops.jpeg_workspace(37, 45, 3, 2, 1) == ((30 + 15 + 15) * 128, 60 * 64)
    assert ops.jpeg_workspace(33, 17, 1, 1, 1) == (15 * 128, 15 * 64)
    lib = _lib.load()
    a, b = C.c_int64(0), C.c_int64(0)
    assert lib.coclr_jpeg_workspace(16, 16, 3, 2, 2, None, C.byref(b)) == 1
    for bad in ((0, 16, 3, 2, 2), (16, 8193, 3, 2, 2), (16, 16, 4, 1, 1), (16, 16, 3, 1, 2), (16, 16, 3, 4, 1),
                (16, 16, 1, 2, 2), (16, 16, 2, 1, 1)):
        assert lib.coclr_jpeg_workspace(*bad, C.byref(a), C.byref(b)) == 1, bad
        with pytest.raises(ValueError):
            ops.jpeg_workspace(*bad)


def test_decode_entry_point_rejects_before_any_launch():
    """COCLR_EINVAL for a null pointer, F < 1 and a descriptor whose ranges leave the buffer: the host copy of the
    descriptors is validated first, so none of these calls reaches a device (there is none here; the pointers that
    stand for device memory are never dereferenced)."""
    lib = _lib.load()
    data, meta = jpeg.pack([J.raw(J.case("56x40_420_rst1"))])
    host = meta[:, 8:].contiguous()
    fake = 0x10000                                            # a non-null, 16-byte aligned stand-in
    hp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_int32))   # noqa: E731

    def call(m=host, F=1, n=data.numel(), width=host.shape[1], geo=(40, 56, 3, 2, 2), stages=7, ptrs=None):
        p = {"data": fake, "meta": fake, "coefs": fake, "planes": fake, "out": fake, "status": fake}
        p.update(ptrs or {})
        return lib.coclr_jpeg_decode(p["data"], n, p["meta"], hp(m) if m is not None else None, F, width, *geo, stages,
                                     p["coefs"], p["planes"], p["out"], p["status"], None)

    for name in ("data", "meta", "coefs", "planes", "out", "status"):
        assert call(ptrs={name: None}) == 1, name
    assert call(m=None) == 1
    assert call(F=0) == 1 and call(F=-3) == 1
    assert call(ptrs={"coefs": fake + 8}) == 1                # misaligned workspace
    assert call(stages=0) == 1 and call(stages=8) == 1
    assert call(geo=(40, 56, 3, 1, 2)) == 1 and call(geo=(40, 56, 4, 1, 1)) == 1
    assert call(width=jpeg.META_SEG) == 1 and call(n=-1) == 1 and call(n=1 << 31) == 1
    assert call(n=data.numel() - 1) == 1                      # the frame's bytes leave the buffer

    def changed(word, value):
        m = host.clone()
        m[0, word] = value
        return m

    assert call(m=changed(0, 1)) == 1                         # offset + length past the end
    assert call(m=changed(0, -1)) == 1
    assert call(m=changed(1, data.numel() + 1)) == 1
    assert call(m=changed(2, 5)) == 1                         # 12 segments do not fit an interval of 5
    assert call(m=changed(3, 13)) == 1                        # more segments than the descriptor is wide
    assert call(m=changed(3, 0)) == 1
    assert call(m=changed(jpeg.META_SEG + 5, data.numel() + 9)) == 1      # a segment outside its frame
    assert call(m=changed(jpeg.META_SEG + 5, 0)) == 1                     # offsets must not decrease
    assert call(m=changed(jpeg.META_QUANT + 70, 256)) == 1
    assert call(m=changed(jpeg.META_HUFF + 3, 70000)) == 1                # a code limit past 2^16


def test_regenerated_outputs_reproduce_the_golden():
    Image = pytest.importorskip("PIL.Image")
    features = pytest.importorskip("PIL.features")
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("PIL without libjpeg-turbo")
    for c in J.cases():
        got = np.array(Image.open(io.BytesIO(J.raw(c))).convert("RGB"))
        assert np.array_equal(got, c["rgb"].numpy()), c["name"]


@pytest.fixture(scope="module")
def core_check(tmp_path_factory):
    """tools/jpeg_core_check.cpp built with the sanitizers, run once on every fixture."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("jpeg_core")
    exe, cases = str(tmp / "jpeg_core_check"), str(tmp / "cases.bin")
    # the sanitizer runtimes are linked statically: the program then does not care what else a host preloads
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "jpeg_core_check.cpp"), "-o", exe])
    J.write_core_check_cases(cases)
    return subprocess.run([exe, cases], stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_host_build_decodes_every_fixture_exactly(core_check):
    out = core_check.stdout.decode()
    assert core_check.returncode == 0, out + core_check.stderr.decode()
    m = re.search(r"(\d+) cases, (\d+) failed", out)
    assert m and int(m.group(1)) == len(J.cases()) and int(m.group(2)) == 0, out


def test_host_build_survives_damaged_streams(core_check):
    """Three fixtures, each cut at five points, overwritten at 32 seeded places and once given sixteen one bits:
    exit 0 without a sanitizer report, and the invalid code raises the status flag."""
    out, err = core_check.stdout.decode(), core_check.stderr.decode()
    assert core_check.returncode == 0 and "ERROR" not in err and "runtime error" not in err, out + err
    m = re.search(r"(\d+) damaged streams decoded in bounds, (\d+) of them flagged", out)
    assert m and int(m.group(1)) == len(J.CORRUPTED) * (5 + 32 + 1), out
    assert int(m.group(2)) >= len(J.CORRUPTED) and "did not raise" not in out
