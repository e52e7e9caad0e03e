"""CPU tier of the device-resident JPEG store (coclr_amd/jpeg.py: class Store; include/coclr_hip.h:
coclr_jpeg_store_index, coclr_jpeg_decode_store): the host side of `add` and `decode` on a store whose buffers are
host tensors and whose indexing launch is a recording double, the two entry points' refusals without a device, and the
store arithmetic of csrc/jpeg_core.h compiled for the host under AddressSanitizer and UBSan
(tools/jpeg_store_check.cpp) -- rows against a serial walk, the one-pass decode against the serial decoder, damaged
streams and rows of random words, none of which is ever sent to a GPU.  Nothing here needs a GPU and nothing is
preloaded into Python."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

import _jpeg_cases as J
from coclr_amd import _lib, jpeg, ops

ROOT = J.ROOT
SIZES = (8, 16, 64, 128, 65536)
DAMAGED_SIZES = (8, 64, 128)


@pytest.fixture
def indexed(monkeypatch):
    """ops.jpeg_store_index replaced by a double that records (frames filled, f0, f1) of every call."""
    calls = []
    monkeypatch.setattr(ops, "jpeg_store_index", lambda store, f0, f1: calls.append((store[3], f0, f1)))
    return calls


def _pack(*names):
    return jpeg.pack([J.raw(J.case(n)) for n in names])


def _group(key):
    return jpeg.pack([J.raw(c) for c in J.groups()[key]])


def _chunks(meta, chunk_bytes):
    """sum of jc_chunk_count over the restart-less frames of a pack"""
    return sum(max(1, -(-int(r[9]) // chunk_bytes)) for r in meta if int(r[11]) == 1)


def test_ids_are_consecutive_and_sizes_are_kept(indexed):
    store = jpeg.Store(1 << 20, 64, device="cpu")
    assert len(store) == 0 and store.nbytes == 0 and store.table_sets == 0 and store.chunk_bytes == 64
    first, total, sizes = [], 0, []
    for key, group in J.groups().items():
        data, meta = jpeg.pack([J.raw(c) for c in group])
        first.append(store.add((data, meta)))
        total += data.numel()
        sizes += [(key[1], key[0])] * len(group)
        assert indexed[-1] == (len(sizes), first[-1], len(sizes))            # one indexing call for the new frames
    assert first[0] == 0 and len(store) == len(J.cases()) == 54 and store.nbytes == total
    assert first == [sum(len(g) for g in list(J.groups().values())[:i]) for i in range(len(first))]
    assert [store.frame_size(i) for i in range(54)] == sizes
    for bad in (-1, 54):
        with pytest.raises(ValueError):
            store.frame_size(bad)
    # the bytes lie where the 64-bit bases say
    data, meta = _pack("45x37_422_q100_noise")
    at = store.add((data, meta))
    base = int(store._host[0][at, 0])
    assert base == total and torch.equal(store._data[base:base + data.numel()], data)


def test_refusals_write_nothing(indexed):
    data, meta = _group((40, 56, 3, (2, 2)))                                 # five frames, some with restart markers
    assert meta.shape[0] == 5 and int((meta[:, 11] > 1).sum()) >= 1

    def snapshot(store):
        return (len(store), store.nbytes, store.table_sets, store.chunk_rows, store._segs, store._data.clone(),
                [t.clone() for t in store._host], [t.clone() for t in store._dev], len(indexed))

    def unchanged(store, was):
        now = snapshot(store)
        assert now[:5] == was[:5] and now[8] == was[8] and torch.equal(now[5], was[5])
        assert all(torch.equal(a, b) for a, b in zip(now[6] + now[7], was[6] + was[7]))

    n = data.numel()
    for kwargs, what in ((dict(capacity_bytes=2 * n - 1, capacity_frames=64), "bytes"),
                         (dict(capacity_bytes=1 << 20, capacity_frames=9), "frames"),
                         (dict(capacity_bytes=1 << 20, capacity_frames=64, capacity_segments=int(meta[:, 11][
                             meta[:, 11] > 1].sum()) * 2 - 1), "restart segments")):
        store = jpeg.Store(device="cpu", **kwargs)
        store._data.fill_(0x5a)
        assert store.add((data, meta)) == 0
        was = snapshot(store)
        with pytest.raises(ValueError, match=what):
            store.add((data, meta))
        unchanged(store, was)
    store = jpeg.Store(1 << 20, 64, device="cpu", capacity_table_sets=1)
    store.add(_pack("16x16_444_q50_ramp"))
    was = snapshot(store)
    with pytest.raises(ValueError, match="table sets"):
        store.add(_pack("45x37_420_q100_noise"))
    unchanged(store, was)
    # what check_meta refuses
    bad = meta.clone()
    bad[2, 8 + jpeg.META_QUANT + 3] = 256
    for pack in ((data, bad), (data[:-1], meta), (data, meta[:, :-1].contiguous()), (data.to(torch.int16), meta)):
        with pytest.raises(ValueError):
            store.add(pack)
        unchanged(store, was)
    # ids: refused on the host, before any launch (there is no device here to launch on)
    store = jpeg.Store(1 << 20, 64, device="cpu")
    store.add((data, meta))
    for ids in ([5], [-1], [0, 1, 7], torch.tensor([[0, 5]]), [], [0.5]):
        with pytest.raises(ValueError):
            store.decode(ids)
    for bad in (0, 7, 65537, 2.5):
        with pytest.raises(ValueError, match="chunk_bytes"):
            jpeg.Store(1 << 20, 64, chunk_bytes=bad, device="cpu")


def test_table_sets_are_shared(indexed):
    store = jpeg.Store(1 << 20, 128, device="cpu")
    cases = J.cases()
    keys = []
    for c in cases:
        _, meta = jpeg.pack([J.raw(c)])
        keys.append(meta[0, 8 + jpeg.META_QUANT:8 + jpeg.META_SEG].numpy().tobytes())
        store.add(jpeg.pack([J.raw(c)]))
    distinct = list(dict.fromkeys(keys))
    assert 1 < len(distinct) < len(cases)                                    # some fixtures share tables, some do not
    assert store.table_sets == len(distinct)
    ids = store._host[0][:len(cases), 4].tolist()
    assert ids == [distinct.index(k) for k in keys]
    for k, i in zip(keys, ids):                                              # and the words are the frame's own
        at = ops.JS_TABLE_PAD + i * ops.JS_TABLE_WORDS
        assert store._host[1][at:at + ops.JS_TABLE_WORDS].numpy().tobytes() == k
    # the same fixture again: no new set
    store.add(jpeg.pack([J.raw(cases[0])] * 3))
    assert store.table_sets == len(distinct) and store._host[0][len(cases):len(cases) + 3, 4].tolist() == [ids[0]] * 3


@pytest.mark.parametrize("chunk_bytes", [8, 64, 65536])
def test_chunk_rows_and_records(indexed, chunk_bytes):
    store = jpeg.Store(1 << 20, 64, chunk_bytes=chunk_bytes, device="cpu")
    want_rows = want_segs = at = 0
    for c in J.cases():
        data, meta = jpeg.pack([J.raw(c)])
        f = store.add((data, meta))
        rec = store._host[0][f].tolist()
        ln, ri, nseg = int(meta[0, 9]), int(meta[0, 10]), int(meta[0, 11])
        hs, vs = c["sampling"]
        assert rec[:4] == [at, ln, ri, nseg]
        assert rec[7] == c["height"] | c["width"] << 16 | c["ncomp"] << 32 | hs << 36 | vs << 40
        if nseg == 1:
            assert rec[6] == want_rows
            want_rows += max(1, -(-ln // chunk_bytes))
        else:
            assert rec[5] == want_segs
            assert store._host[2][want_segs:want_segs + nseg].tolist() == meta[0, 8 + jpeg.META_SEG:].tolist()[:nseg]
            want_segs += nseg
        at += ln
        assert torch.equal(store._dev[0][f], store._host[0][f])
    assert store.chunk_rows == want_rows == sum(_chunks(jpeg.pack([J.raw(c)])[1], chunk_bytes) for c in J.cases())
    assert store._segs == want_segs > 0
    assert store._rows.shape[0] >= want_rows
    if chunk_bytes == 65536:
        assert want_rows == sum(len(jpeg.parse(J.raw(c))["segments"]) == 1 for c in J.cases())


@pytest.mark.parametrize("budget", [256 << 20, 40000, 1])
def test_per_call_tables_equal_decode_raggeds(indexed, budget):
    cases = J.cases()
    store = jpeg.Store(1 << 20, 64, device="cpu")
    g = torch.Generator().manual_seed(7)
    order = torch.randperm(len(cases), generator=g).tolist()
    where = {}
    for i in order:
        where[i] = store.add(jpeg.pack([J.raw(cases[i])]))
    picks = torch.randperm(len(cases), generator=g).tolist() + [3, 3, 17, 0, 3]      # a permutation, then repeats
    ids = [where[i] for i in picks]
    sel, geo, offset, total, stages, blocks = store.plan(ids, budget)
    data, meta = jpeg.cat_ragged([jpeg.pack([J.raw(cases[i])]) for i in picks])
    want_geo = jpeg.check_meta_ragged(data, meta)
    w_offset, w_total, w_stages, w_blocks = jpeg.ragged_plan(want_geo, budget)
    assert sel.tolist() == ids and torch.equal(geo, want_geo)
    assert torch.equal(offset, w_offset) and total == w_total and blocks == w_blocks and len(stages) == len(w_stages)
    assert len(stages) == {256 << 20: 1, 1: len(picks)}.get(budget, len(stages)) and (budget != 40000 or len(stages) > 2)
    lanes = [max(1, -(-int(r[9]) // 64)) if int(r[11]) == 1 else int(r[11]) for r in meta]
    for (k, e, geom, prefix), (wk, we, w_geom, w_prefix) in zip(stages, w_stages):
        assert (k, e) == (wk, we) and torch.equal(geom, w_geom) and torch.equal(prefix[:2], w_prefix)
        assert prefix.shape == (3, e - k + 1) and prefix.dtype == torch.int64
        assert prefix[2].tolist() == [sum(lanes[k:k + i]) for i in range(e - k + 1)]


def test_entry_points_are_declared_exported_and_bound():
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "coclr_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\bint\s+(coclr_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (coclr_[a-z0-9_]+)", out))
    for name in ("coclr_jpeg_store_index", "coclr_jpeg_decode_store"):
        assert name in declared and name in exported and name in _lib.EXPORTED_SYMBOLS
    assert declared == exported == set(_lib.EXPORTED_SYMBOLS)
    assert lib.coclr_abi_version() == _lib.ABI_VERSION == 26
    fields = re.search(r"typedef struct \{([^}]*)\} coclr_jpeg_store;", header).group(1)
    assert re.findall(r"(\w+);", fields) == [n for n, _ in _lib.JpegStore._fields_]


def test_entry_points_reject_before_any_launch(indexed):
    """COCLR_EINVAL from the host copies alone: no call below reaches a device (there is none here; the stand-in
    device pointers are never dereferenced)."""
    lib = _lib.load()
    store = jpeg.Store(1 << 20, 64, device="cpu")
    for c in J.cases()[:8]:
        store.add(jpeg.pack([J.raw(c)]))
    store.add(_pack("56x40_420_rst1"))
    n = len(store)
    fake = 0x10000                                            # a non-null, 16-byte aligned stand-in
    frames_host, tables_host, segs_host = (t.clone() for t in store._host)

    def desc(**over):
        d = dict(data=fake, data_bytes=store.nbytes, frames=fake, frames_host=frames_host.data_ptr(), nframes=n,
                 tables=fake, tables_host=tables_host.data_ptr(), table_sets=store.table_sets, segs=fake,
                 segs_host=segs_host.data_ptr(), nsegs=store._segs, rows=fake, nrows=store._rows.shape[0],
                 chunk_bytes=64)
        d.update(over)
        return _lib.JpegStore(**d)

    def index(f0=0, f1=n, **over):
        return lib.coclr_jpeg_store_index(C.byref(desc(**over)), f0, f1, None)

    assert lib.coclr_jpeg_store_index(None, 0, n, None) == 1
    for over in (dict(data=None), dict(frames=None), dict(frames_host=None), dict(tables=None), dict(tables_host=None),
                 dict(rows=None), dict(segs=None), dict(segs_host=None), dict(chunk_bytes=7), dict(chunk_bytes=65537),
                 dict(nframes=0), dict(table_sets=0), dict(nrows=0), dict(rows=fake + 4), dict(data_bytes=-1),
                 dict(data_bytes=store.nbytes - 1),             # the last frame's bytes leave the store
                 dict(nrows=store.chunk_rows - 1), dict(nsegs=store._segs - 1), dict(table_sets=1)):
        assert index(**over) == 1, over
    assert index(f0=-1) == 1 and index(f0=3, f1=3) == 1 and index(f1=n + 1) == 1

    def changed(t, at, value):
        was = t[at].clone()
        t[at] = value
        rc = index()
        t[at] = was
        return rc

    last = n - 1                                                # the frame with restart markers
    assert int(frames_host[last, 3]) > 1 and int(frames_host[0, 3]) == 1
    for at, value in (((0, 0), -1), ((0, 1), -1), ((0, 1), 1 << 31), ((0, 2), -1), ((0, 3), 0), ((0, 3), 2),
                      ((0, 4), -1), ((0, 4), store.table_sets), ((0, 6), -1), ((0, 6), store._rows.shape[0]),
                      ((0, 7), 0), ((0, 7), int(frames_host[0, 7]) | 3 << 36), ((last, 5), -1),
                      ((last, 5), store._segs), ((last, 2), 5)):
        assert changed(frames_host, at, value) == 1, (at, value)
    first_seg = int(frames_host[last, 5])
    assert changed(segs_host, first_seg + 2, 0) == 1                          # decreasing
    assert changed(segs_host, first_seg + 2, int(frames_host[last, 1]) + 1) == 1
    tset = ops.JS_TABLE_PAD + int(frames_host[0, 4]) * ops.JS_TABLE_WORDS
    assert changed(tables_host, tset + 3, 256) == 1                           # a quantiser
    assert changed(tables_host, tset + (jpeg.META_HUFF - jpeg.META_QUANT) + 3, 70000) == 1      # a code limit

    # coclr_jpeg_decode_store: the selection and the per-call tables
    picks = [last, 2, 2, 0]
    sel, geo, offset, total, stages, blocks = store.plan(picks)
    (_, _, geom, prefix), = stages
    hp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_int64))   # noqa: E731

    def decode(s=sel, g=geom, p=prefix, F=len(picks), stages=7, blocks=blocks, out_bytes=(total + 15) & ~15, ptrs=None,
               **over):
        a = {"sel": fake, "geom": fake, "prefix": fake, "coefs": fake, "planes": fake, "out": fake, "status": fake}
        a.update(ptrs or {})
        return lib.coclr_jpeg_decode_store(C.byref(desc(**over)), a["sel"], hp(s) if s is not None else None, F,
                                           a["geom"], hp(g) if g is not None else None, a["prefix"],
                                           hp(p) if p is not None else None, stages, a["coefs"], a["planes"], blocks,
                                           a["out"], out_bytes, a["status"], None)

    for name in ("sel", "geom", "prefix", "coefs", "planes", "out", "status"):
        assert decode(ptrs={name: None}) == 1, name
    assert decode(s=None) == 1 and decode(g=None) == 1 and decode(p=None) == 1
    assert decode(F=0) == 1 and decode(stages=0) == 1 and decode(stages=8) == 1
    assert decode(ptrs={"coefs": fake + 8}) == 1 and decode(ptrs={"out": fake + 8}) == 1
    assert decode(blocks=blocks - 1) == 1 and decode(out_bytes=total - 1) == 1
    assert decode(chunk_bytes=7) == 1 and decode(rows=None) == 1 and decode(nframes=last) == 1
    assert int(frames_host[2, 3]) == 1 and int(frames_host[2, 1]) > 8
    assert decode(chunk_bytes=8) == 1                            # the lanes are no longer the frames' chunk counts

    def edit(t, at, value):
        t = t.clone()
        t[at] = value
        return t

    for bad in (-1, n, 1 << 40):
        assert decode(s=edit(sel, 1, bad)) == 1, bad
    assert decode(s=edit(sel, 1, 3)) == 1                        # another frame: its geometry is not the table's
    assert decode(g=edit(geom, (1, 0), int(geom[1, 0]) + 1)) == 1
    assert decode(g=edit(geom, (2, 5), int(geom[2, 5]) - 1)) == 1            # overlapping coefficient blocks
    assert decode(g=edit(geom, (2, 6), int(geom[2, 6]) + 8)) == 1            # an output frame off its 16 bytes
    assert decode(g=edit(geom, (3, 6), (total + 15) & ~15)) == 1
    for row in range(3):
        assert decode(p=edit(prefix, (row, 0), 1)) == 1
        assert decode(p=edit(prefix, (row, 2), int(prefix[row, 2]) + 1)) == 1


@pytest.fixture(scope="module")
def store_check(tmp_path_factory):
    """tools/jpeg_store_check.cpp built with the sanitizers, run once on every fixture."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("jpeg_store")
    exe, cases = str(tmp / "jpeg_store_check"), str(tmp / "cases.bin")
    # the sanitizer runtimes are linked statically: the program then does not care what else a host preloads
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "jpeg_store_check.cpp"), "-o", exe])
    J.write_core_check_cases(cases)
    return subprocess.run([exe, cases], stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def _counts(line):
    return [int(v) for v in re.findall(r"\d+", line)]


def test_host_build_rows_are_the_serial_decoders_states(store_check):
    out, err = store_check.stdout.decode(), store_check.stderr.decode()
    assert store_check.returncode == 0 and "ERROR" not in err and "runtime error" not in err, out + err
    line = next(l for l in out.splitlines() if "frames x sizes" in l)
    frames, rows, segments, garbage, failed = _counts(line)
    single = [c for c in J.cases() if len(jpeg.parse(J.raw(c))["segments"]) == 1]
    assert frames == len(J.cases()) * len(SIZES) and failed == 0
    want = sum(_chunks(jpeg.pack([J.raw(c)])[1], cb) for c in single for cb in SIZES)
    assert rows == want and garbage == 2 * rows and rows > 50 * len(single)
    multi = sum(len(jpeg.parse(J.raw(c))["segments"]) for c in J.cases() if c not in single)
    assert segments == multi * len(SIZES) > 0
    assert "differs" not in out


def test_host_build_holds_on_damaged_streams(store_check):
    """Per CORRUPTED fixture and chunk size 8, 64, 128: 24 flipped bytes, 5 cuts and 16 inserted bytes, each checked as
    the clean frames are, rows of random words included, all in exact heap blocks under the sanitizers."""
    out, err = store_check.stdout.decode(), store_check.stderr.decode()
    assert store_check.returncode == 0 and "ERROR" not in err and "runtime error" not in err, out + err
    line = next(l for l in out.splitlines() if "damaged frames" in l)
    frames, rows, segments, garbage, failed = _counts(line)
    assert frames == len(J.CORRUPTED) * len(DAMAGED_SIZES) * (24 + 5 + 16) and failed == 0
    assert rows > 0 and segments > 0 and garbage == 2 * rows
