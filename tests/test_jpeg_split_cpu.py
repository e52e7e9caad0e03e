"""CPU tier of intra-frame parallel Huffman decoding (coclr_jpeg_decode_split; csrc/jpeg_core.h: jc_chunk_scan /
jc_chunk_write): the additive entry point and its refusals without a device, the host-side policy, and the chunk
arithmetic compiled for the host under AddressSanitizer and UBSan (tools/jpeg_split_check.cpp), driven in the kernel's
order and compared with the serial decoder byte for byte -- every fixture and restart segment at nine chunk sizes, and
damaged streams, which are never sent to a GPU.  Nothing here needs a GPU and nothing is preloaded into Python."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import _jpeg_cases as J
from coclr_amd import _lib, jpeg

ROOT = J.ROOT
SIZES = (1, 2, 3, 5, 8, 16, 64, 128, 4096)


def test_split_entry_point_is_declared_exported_and_bound():
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "coclr_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\bint\s+(coclr_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (coclr_[a-z0-9_]+)", out))
    name = "coclr_jpeg_decode_split"
    assert name in declared and name in exported and name in _lib.EXPORTED_SYMBOLS
    assert declared == exported == set(_lib.EXPORTED_SYMBOLS)
    assert len(getattr(lib, name).argtypes) == len(lib.coclr_jpeg_decode.argtypes) + 1
    assert lib.coclr_abi_version() == _lib.ABI_VERSION == 26


def test_split_entry_point_rejects_before_any_launch():
    """COCLR_EINVAL for a chunk size outside {0} and 8..65536 and for the descriptors coclr_jpeg_decode refuses: the
    host copy is validated first, so no call reaches a device (there is none here; the stand-in pointers are never
    dereferenced)."""
    lib = _lib.load()
    data, meta = jpeg.pack([J.raw(J.case("56x40_420_rst1"))])
    host = meta[:, 8:].contiguous()
    fake = 0x10000                                            # a non-null, 16-byte aligned stand-in
    hp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_int32))   # noqa: E731

    def call(chunk_bytes, m=host, F=1, n=data.numel(), width=host.shape[1], geo=(40, 56, 3, 2, 2), stages=7,
             ptrs=None):
        p = {"data": fake, "meta": fake, "coefs": fake, "planes": fake, "out": fake, "status": fake}
        p.update(ptrs or {})
        return lib.coclr_jpeg_decode_split(p["data"], n, p["meta"], hp(m) if m is not None else None, F, width, *geo,
                                           stages, p["coefs"], p["planes"], p["out"], p["status"], chunk_bytes, None)

    for bad in (-1, 1, 7, 65537):
        assert call(bad) == 1, bad

    def changed(word, value):
        m = host.clone()
        m[0, word] = value
        return m

    for cb in (0, 128):                                       # the same bad descriptors, whatever the chunk size
        for name in ("data", "meta", "coefs", "planes", "out", "status"):
            assert call(cb, ptrs={name: None}) == 1, name
        assert call(cb, m=None) == 1
        assert call(cb, F=0) == 1 and call(cb, F=-3) == 1
        assert call(cb, ptrs={"coefs": fake + 8}) == 1
        assert call(cb, stages=0) == 1 and call(cb, stages=8) == 1
        assert call(cb, geo=(40, 56, 3, 1, 2)) == 1 and call(cb, geo=(40, 56, 4, 1, 1)) == 1
        assert call(cb, width=jpeg.META_SEG) == 1 and call(cb, n=-1) == 1 and call(cb, n=1 << 31) == 1
        assert call(cb, n=data.numel() - 1) == 1
        assert call(cb, m=changed(0, 1)) == 1
        assert call(cb, m=changed(0, -1)) == 1
        assert call(cb, m=changed(1, data.numel() + 1)) == 1
        assert call(cb, m=changed(2, 5)) == 1
        assert call(cb, m=changed(3, 13)) == 1
        assert call(cb, m=changed(3, 0)) == 1
        assert call(cb, m=changed(jpeg.META_SEG + 5, data.numel() + 9)) == 1
        assert call(cb, m=changed(jpeg.META_SEG + 5, 0)) == 1
        assert call(cb, m=changed(jpeg.META_QUANT + 70, 256)) == 1
        assert call(cb, m=changed(jpeg.META_HUFF + 3, 70000)) == 1


def test_bad_chunk_size_is_a_value_error_without_a_device(monkeypatch):
    data, meta = jpeg.pack([J.raw(J.case("16x16_444_q50_ramp"))])
    monkeypatch.delenv("COCLR_JPEG_SPLIT", raising=False)
    for bad in (3, -1, 7, 65537, 2.5, "x"):
        with pytest.raises(ValueError, match="chunk_bytes"):
            jpeg.decode(data, meta, chunk_bytes=bad)
    with pytest.raises(ValueError, match="chunk_bytes"):
        jpeg.decode_frames([b"not looked at"], chunk_bytes=3)
    for bad in ("5", "65537", "-8", "many"):
        monkeypatch.setenv("COCLR_JPEG_SPLIT", bad)
        with pytest.raises(ValueError, match="COCLR_JPEG_SPLIT"):
            jpeg.decode(data, meta)
        assert jpeg.split_policy(64) == 64                     # an explicit size does not consult the environment
    monkeypatch.setenv("COCLR_JPEG_SPLIT", "128")
    assert jpeg.split_policy() == 128 and jpeg.split_policy(0) == 0
    monkeypatch.setenv("COCLR_JPEG_SPLIT", "0")
    assert jpeg.split_policy() == 0
    monkeypatch.delenv("COCLR_JPEG_SPLIT")
    assert jpeg.split_policy() == jpeg.DEFAULT_SPLIT
    assert jpeg.DEFAULT_SPLIT == 0 or 8 <= jpeg.DEFAULT_SPLIT <= 65536


@pytest.fixture(scope="module")
def split_check(tmp_path_factory):
    """tools/jpeg_split_check.cpp built with the sanitizers, run once on every fixture."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("jpeg_split")
    exe, cases = str(tmp / "jpeg_split_check"), str(tmp / "cases.bin")
    # the sanitizer runtimes are linked statically: the program then does not care what else a host preloads
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "jpeg_split_check.cpp"), "-o", exe])
    J.write_core_check_cases(cases)
    return subprocess.run([exe, cases], stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_host_build_equals_the_serial_decoder_at_every_chunk_size(split_check):
    out, err = split_check.stdout.decode(), split_check.stderr.decode()
    assert split_check.returncode == 0 and "ERROR" not in err and "runtime error" not in err, out + err
    m = re.search(r"(\d+) units x sizes, (\d+) failed", out)
    segments = sum(len(jpeg.parse(J.raw(c))["segments"]) for c in J.cases())
    assert m and int(m.group(1)) == segments * len(SIZES) and int(m.group(2)) == 0, out
    assert segments > len(J.cases())                           # restart segments are units of their own


def test_host_build_equals_the_serial_decoder_on_damaged_streams(split_check):
    """Per CORRUPTED fixture and chunk size 8, 16, 128: five cuts, 32 seeded overwrites, sixteen one bits, a planted
    FF D0 and a cut inside an FF 00 pair, all in exact heap blocks under the sanitizers."""
    out, err = split_check.stdout.decode(), split_check.stderr.decode()
    assert split_check.returncode == 0 and "ERROR" not in err and "runtime error" not in err, out + err
    m = re.search(r"(\d+) damaged streams equal to the serial decoder", out)
    assert all(J.case(n)["raw"].numel() > 64 for n in J.CORRUPTED)
    assert m and int(m.group(1)) == len(J.CORRUPTED) * 3 * (5 + 32 + 1 + 1 + 1), out
    assert "differs" not in out


def test_the_inputs_exercise_the_mechanism(split_check):
    """Relaxation really runs for several rounds, and chunks that own no symbol start really occur."""
    out = split_check.stdout.decode()
    rows = {int(a): (int(b), int(c)) for a, b, c in
            re.findall(r"chunk size (\d+): at most (\d+) rounds, (\d+) chunks owned no symbol start", out)}
    assert sorted(rows) == sorted(SIZES), out
    assert rows[16][0] >= 3, out
    assert rows[1][1] > 0, out
    assert rows[4096][0] <= rows[128][0] <= rows[16][0]
