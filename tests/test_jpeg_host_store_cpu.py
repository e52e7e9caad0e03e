"""CPU tier of the host-resident JPEG store (coclr_amd/jpeg.py: Store(bytes_on="host"), Store.save / Store.load;
include/coclr_hip.h: coclr_jpeg_store_gather): the bookkeeping of a host store against a device-kind store on the
`device="cpu"` double, the gather's host tables, the save / load round trip with its refusals, and the gather arithmetic
of csrc/jpeg_core.h compiled for the host under AddressSanitizer and UBSan (tools/jpeg_gather_check.cpp).
ops.jpeg_store_index and ops.jpeg_store_gather are recording doubles; the gather double is a numpy restatement of the
copy.  Nothing here needs a GPU and nothing is preloaded into Python."""
import ctypes as C
import json
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


def _numpy_gather(store, plan, plan_host, slot_host, frames_host, arena, arena_rows):
    """What jpeg_store_gather_kernel copies, restated: per plan row the 16-byte words of the hull, then the rows."""
    data, rows = store[0].numpy(), store[10].numpy().reshape(-1, 4)
    out, out_rows = arena.numpy(), arena_rows.numpy().reshape(-1, 4)
    for frame, src, ln, dst, srow, nrows, drow, lane in plan_host.tolist():
        if ln:
            w0, w1 = src >> 4, (src + ln + 15) >> 4
            have = min(w1 * 16, data.size) - w0 * 16             # (the room behind the bytes is never read back)
            out[(dst >> 4) * 16:(dst >> 4) * 16 + have] = data[w0 * 16:w0 * 16 + have]
        out_rows[drow:drow + nrows] = rows[srow:srow + nrows]


@pytest.fixture
def doubles(monkeypatch):
    """The two launches replaced: `index` records (frames of the view, its records, f0, f1), `gather` records the plan
    and copies as the kernel does."""
    calls = {"index": [], "gather": [], "refuse": False}

    def index(store, f0, f1):
        if calls["refuse"]:
            raise _lib.HipLibraryError("coclr_amd: jpeg_store_index failed with hipError 1")
        calls["index"].append((store[3], store[2][:store[3]].clone(), f0, f1))

    def gather(store, plan, plan_host, slot_host, frames_host, arena, arena_rows):
        calls["gather"].append((plan_host.clone(), slot_host.clone(), frames_host.clone()))
        _numpy_gather(store, plan, plan_host, slot_host, frames_host, arena, arena_rows)

    monkeypatch.setattr(ops, "jpeg_store_index", index)
    monkeypatch.setattr(ops, "jpeg_store_gather", gather)
    return calls


def _packs():
    return [jpeg.pack([J.raw(c) for c in group]) for group in J.groups().values()]


def _both(**kw):
    return (jpeg.Store(1 << 20, 64, device="cpu", bytes_on="host", **kw), jpeg.Store(1 << 20, 64, device="cpu", **kw))


def _same_books(a, b):
    assert (len(a), a.nbytes, a.table_sets, a.chunk_rows, a._segs) == (len(b), b.nbytes, b.table_sets, b.chunk_rows,
                                                                      b._segs)
    assert [a.frame_size(i) for i in range(len(a))] == [b.frame_size(i) for i in range(len(b))]
    assert all(torch.equal(x, y) for x, y in zip(a._host + a._dev, b._host + b._dev))
    assert torch.equal(a._data[:a.nbytes], b._data[:b.nbytes])
    assert torch.equal(a._geo, b._geo) and torch.equal(a._lanes, b._lanes) and a._sets == b._sets


def test_the_keyword_is_last_and_defaults_to_device(doubles):
    import inspect
    names = list(inspect.signature(jpeg.Store.__init__).parameters)
    assert names[-1] == "bytes_on" and inspect.signature(jpeg.Store.__init__).parameters["bytes_on"].default == "device"
    assert jpeg.Store(1 << 10, 4, device="cpu").bytes_on == "device"
    with pytest.raises(ValueError, match="bytes_on"):
        jpeg.Store(1 << 10, 4, device="cpu", bytes_on="disk")


@pytest.mark.parametrize("chunk_bytes", [None, 8, 65536])
def test_bookkeeping_is_a_device_stores(doubles, chunk_bytes):
    host, dev = _both(chunk_bytes=chunk_bytes)
    assert host.bytes_on == "host" and not host._data.is_cuda and not host._rows.is_cuda
    for data, meta in _packs():
        rows0, n0 = host.chunk_rows, len(doubles["index"])
        assert host.add((data, meta)) == dev.add((data, meta))
        _same_books(host, dev)
        # the host store indexed a view of the pack alone, its records rebased to the scratch
        (F, rec, f0, f1), (Fd, _, d0, d1) = doubles["index"][n0:]
        assert (F, f0, f1) == (meta.shape[0], 0, meta.shape[0]) and (Fd, d1 - d0) == (len(dev), F)
        want = host._host[0][len(host) - F:len(host)].clone()
        want[:, 0] -= host.nbytes - data.numel()
        want[:, 6] -= rows0
        assert torch.equal(rec, want) and torch.equal(rec[:, 0], meta[:, 8].to(torch.int64))
        assert torch.equal(host._scratch[:data.numel()], data)
    assert len(host) == 54 and host._rows.shape == dev._rows.shape


def test_refusals_and_rollback_write_nothing(doubles):
    data, meta = jpeg.pack([J.raw(c) for c in J.groups()[(40, 56, 3, (2, 2))]])
    n, nseg = data.numel(), int(meta[:, 11][meta[:, 11] > 1].sum())
    assert nseg > 0

    def snapshot(s):
        return (len(s), s.nbytes, s.table_sets, s.chunk_rows, s._segs, dict(s._sets), s._data.clone(), s._rows.clone(),
                [t.clone() for t in s._host + s._dev])

    def unchanged(s, was):
        now = snapshot(s)
        assert now[:6] == was[:6] and torch.equal(now[6], was[6]) and torch.equal(now[7], was[7])
        assert all(torch.equal(a, b) for a, b in zip(now[8], was[8]))

    for kw, what in ((dict(capacity_bytes=2 * n - 1, capacity_frames=64), "bytes"),
                     (dict(capacity_bytes=1 << 20, capacity_frames=9), "frames"),
                     (dict(capacity_bytes=1 << 20, capacity_frames=64, capacity_segments=2 * nseg - 1),
                      "restart segments"),
                     (dict(capacity_bytes=1 << 20, capacity_frames=64, capacity_table_sets=1), "table sets")):
        store = jpeg.Store(device="cpu", bytes_on="host", **kw)
        store._data.fill_(0x5a)
        store._rows.fill_(0x5a5a5a5a)
        sets = what == "table sets"
        assert store.add(jpeg.pack([J.raw(J.case("16x16_444_q50_ramp"))]) if sets else (data, meta)) == 0
        was = snapshot(store)
        other = jpeg.pack([J.raw(J.case("45x37_420_q100_noise"))]) if sets else (data, meta)
        with pytest.raises(ValueError, match=what):
            store.add(other)
        unchanged(store, was)
    # the indexing entry point refuses: the frames are not kept, and the next pack takes their ids
    host, dev = _both()
    host.add((data, meta)), dev.add((data, meta))
    was = snapshot(host)
    doubles["refuse"] = True
    with pytest.raises(_lib.HipLibraryError):
        host.add(jpeg.pack([J.raw(J.case("45x37_420_q100_noise"))]))
    assert snapshot(host)[:6] == was[:6] and torch.equal(host._rows, was[7])
    doubles["refuse"] = False
    pack = jpeg.pack([J.raw(J.case("17x33_gray_q50_ramp"))])
    assert host.add(pack) == dev.add(pack) == meta.shape[0]
    _same_books(host, dev)


def _filled_store(doubles, chunk_bytes=None, seed=3):
    """Every fixture as a pack of its own, in a seeded order, with rows that say whose they are."""
    store = jpeg.Store(1 << 20, 64, chunk_bytes=chunk_bytes, device="cpu", bytes_on="host")
    order = torch.randperm(54, generator=torch.Generator().manual_seed(seed)).tolist()
    where = {i: store.add(jpeg.pack([J.raw(J.cases()[i])])) for i in order}
    store._rows[:store.chunk_rows] = torch.arange(store.chunk_rows * 4, dtype=torch.int32).view(-1, 4)
    return store, where


@pytest.mark.parametrize("chunk_bytes", [None, 8])
def test_rebased_records_of_a_selection(doubles, chunk_bytes):
    store, where = _filled_store(doubles, chunk_bytes)
    g = torch.Generator().manual_seed(11)
    picks = torch.randperm(54, generator=g).tolist()[:40] + [5, 5, 17]
    picks.insert(3, picks[0]), picks.insert(20, picks[0])                     # picks[0] three times
    sel = torch.tensor([where[i] for i in picks])
    plan, slot, records, nbytes, nrows = store.gather_plan(sel)
    rec = store._host[0]
    m = plan.shape[0]
    assert m == len(set(picks)) and plan.shape == (m, ops.JG_FIELDS) and records.shape == (len(picks), ops.JS_FIELDS)
    assert plan[:, 0].tolist() == sorted(set(sel.tolist())) and torch.equal(plan[:, 0][slot], sel)
    src, ln, dst = plan[:, 1], plan[:, 2], plan[:, 3]
    assert torch.equal(src, rec[plan[:, 0], 0]) and torch.equal(ln, rec[plan[:, 0], 1])
    assert bool(((dst - src) % 16 == 0).all())                                # the congruence
    hull0, hull1 = dst & ~15, (dst + ln + 15) & ~15
    assert int(hull0[0]) == 0 and torch.equal(hull0[1:], hull1[:-1]) and int(hull1[-1]) == nbytes      # no overlap, no gap
    assert bool((dst + ln <= nbytes).all()) and bool((dst - hull0 < 16).all()) and bool((hull1 - dst - ln < 16).all())
    single = rec[plan[:, 0], 3] == 1
    assert bool(single.any()) and not bool(single.all())
    assert torch.equal(plan[:, 5], torch.where(single, store._lanes[plan[:, 0]], 0))     # restart markers: no rows
    assert torch.equal(plan[:, 6], plan[:, 5].cumsum(0) - plan[:, 5]) and int(plan[:, 5].sum()) == nrows
    lanes = (hull1 - hull0) // 16 + plan[:, 5]
    assert torch.equal(plan[:, 7], lanes.cumsum(0) - lanes)
    # the records: the store's own, moved; a frame chosen three times is once in the arena and three times here
    want = rec[sel].clone()
    want[:, 0], want[:, 6] = dst[slot], plan[:, 6][slot]
    assert torch.equal(records, want)
    thrice = [i for i, p in enumerate(picks) if p == picks[0]]
    assert len(thrice) >= 3 and len(set(slot[thrice].tolist())) == 1 and len(set(map(tuple, records[thrice].tolist()))) == 1
    assert int((plan[:, 0] == where[picks[0]]).sum()) == 1
    # and the copy: every selected frame's bytes and rows lie in the arena where its record says
    d_tables = torch.cat([plan.reshape(-1), records.reshape(-1)])
    view = store._gather((plan, slot, records, nbytes, nrows), d_tables)
    arena, d_rec, h_rec, n, tables, h_tables, sets, segs, h_segs, nsegs, arena_rows, cb = view
    assert arena.numel() == nbytes and arena_rows.shape[0] == nrows and n == len(picks) and cb == store.chunk_bytes
    assert torch.equal(d_rec, records) and h_rec is records and tables is store._dev[1] and segs is store._dev[2]
    for i, f in enumerate(sel.tolist()):
        b, l, a = int(rec[f, 0]), int(rec[f, 1]), int(records[i, 0])
        assert torch.equal(arena[a:a + l], store._data[b:b + l])
        if int(rec[f, 3]) == 1:
            k, r = int(store._lanes[f]), int(records[i, 6])
            assert torch.equal(arena_rows[r:r + k], store._rows[int(rec[f, 6]):int(rec[f, 6]) + k])
    # the arena is kept: a smaller call allocates nothing
    kept = store._arena.data_ptr(), store._arena_rows.data_ptr()
    one = store.gather_plan(sel[:1])
    assert one[0].shape[0] == 1 and one[1].tolist() == [0] and int(one[0][0, 3]) == int(rec[sel[0], 0]) % 16
    assert one[3] == ((int(one[0][0, 3]) + int(one[0][0, 2]) + 15) & ~15)
    store._gather(one, torch.cat([one[0].reshape(-1), one[2].reshape(-1)]))
    assert (store._arena.data_ptr(), store._arena_rows.data_ptr()) == kept


def _saved(doubles, tmp_path, bytes_on):
    store = jpeg.Store(1 << 20, 64, device="cpu", bytes_on=bytes_on)
    packs = _packs()
    for p in packs[:-2]:
        store.add(p)
    store._rows[:store.chunk_rows] = torch.arange(store.chunk_rows * 4, dtype=torch.int32).view(-1, 4)
    path = str(tmp_path / ("store_" + bytes_on))
    store.save(path)
    return store, path, packs[-2:]


@pytest.mark.parametrize("kinds", [("host", "device"), ("device", "host"), ("host", "host")])
def test_save_load_round_trip(doubles, tmp_path, kinds):
    store, path, rest = _saved(doubles, tmp_path, kinds[0])
    assert sorted(os.listdir(path)) == sorted(["header.json"] + [n + ".npy" for n in jpeg.Store._FILES])
    head = json.load(open(os.path.join(path, "header.json")))
    assert head["version"] == 1 and head["chunk_bytes"] == 64 and head["frames"] == len(store)
    assert head["bytes"] == store.nbytes and head["rows"] == store.chunk_rows and head["table_sets"] == store.table_sets
    assert head["constants"] == {"JS_FIELDS": 8, "JS_TABLE_WORDS": 768, "JS_TABLE_PAD": 16, "JS_ROW_WORDS": 4}
    calls = len(doubles["index"])
    loaded = jpeg.Store.load(path, device="cpu", bytes_on=kinds[1])
    assert loaded.bytes_on == kinds[1] and len(doubles["index"]) == calls           # nothing was indexed
    assert (loaded.capacity_bytes, loaded.capacity_frames) == (store.nbytes, len(store))
    nf, sets = len(store), ops.JS_TABLE_PAD + store.table_sets * ops.JS_TABLE_WORDS
    for k, n in ((0, nf), (1, sets), (2, store._segs)):
        assert torch.equal(loaded._host[k][:n], store._host[k][:n]) and torch.equal(loaded._dev[k][:n], store._host[k][:n])
    assert torch.equal(loaded._data[:store.nbytes], store._data[:store.nbytes])
    assert torch.equal(loaded._rows[:store.chunk_rows], store._rows[:store.chunk_rows])
    assert torch.equal(loaded._geo[:nf], store._geo[:nf]) and torch.equal(loaded._lanes[:nf], store._lanes[:nf])
    assert loaded._sets == store._sets and loaded.chunk_rows == store.chunk_rows and loaded._segs == store._segs
    with pytest.raises(ValueError, match="bytes"):                                   # full: the file's own capacities
        loaded.add(rest[0])
    # larger capacities: add carries on where the saved store would, sharing the table sets it holds
    roomy = jpeg.Store.load(path, device="cpu", bytes_on=kinds[1], capacity_bytes=1 << 20, capacity_frames=64,
                            capacity_table_sets=64)
    for p in rest:
        assert roomy.add(p) == store.add(p)
    assert roomy.add(_packs()[0]) == store.add(_packs()[0]) == 54          # tables the file held: no new set
    assert roomy.table_sets == store.table_sets
    _same_books(roomy, store)


def _edit_header(path, **fields):
    name = os.path.join(path, "header.json")
    head = json.load(open(name))
    for k, v in fields.items():
        if k in head["constants"]:
            head["constants"][k] = v
        else:
            head[k] = v
    json.dump(head, open(name, "w"))


@pytest.mark.parametrize("what", ["version", "JS_FIELDS", "JS_TABLE_WORDS", "JS_TABLE_PAD", "JS_ROW_WORDS", "frames",
                                  "bytes", "segments", "rows", "table_sets", "chunk_bytes", "truncated",
                                  "capacity_bytes", "capacity_frames", "capacity_table_sets", "capacity_segments"])
def test_load_refuses_before_any_buffer(doubles, tmp_path, monkeypatch, what):
    store, path, _ = _saved(doubles, tmp_path, "host")
    kw = {}
    if what == "truncated":
        name = os.path.join(path, "data.npy")
        with open(name, "r+b") as f:
            f.truncate(os.path.getsize(name) - 1)
    elif what.startswith("capacity"):
        kw[what] = {"capacity_bytes": store.nbytes, "capacity_frames": len(store),
                    "capacity_table_sets": store.table_sets, "capacity_segments": store._segs}[what] - 1
    elif what == "chunk_bytes":
        _edit_header(path, chunk_bytes=7)
    else:
        was = json.load(open(os.path.join(path, "header.json")))
        _edit_header(path, **{what: (was["constants"] if what in was["constants"] else was)[what] + 1})
    made = []
    init = jpeg.Store.__init__
    monkeypatch.setattr(jpeg.Store, "__init__", lambda self, *a, **k: (made.append(1), init(self, *a, **k))[1])
    for bytes_on in ("host", "device"):
        with pytest.raises(ValueError):
            jpeg.Store.load(path, device="cpu", bytes_on=bytes_on, **kw)
    assert not made                                                                  # no buffer was ever allocated
    monkeypatch.setattr(jpeg.Store, "__init__", init)


def test_gather_entry_point_is_declared_exported_and_bound():
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "coclr_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\bint\s+(coclr_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (coclr_[a-z0-9_]+)", out))
    assert "coclr_jpeg_store_gather" in declared & exported & set(_lib.EXPORTED_SYMBOLS)
    assert lib.coclr_abi_version() == _lib.ABI_VERSION
    args = re.search(r"int coclr_jpeg_store_gather\(([^)]*)\)", header).group(1).split(",")
    assert len(args) == len(_lib._SIGNATURES["coclr_jpeg_store_gather"]) == 12


def test_gather_entry_point_refuses_without_a_device(doubles):
    """COCLR_EINVAL from the host copies, and at the latest from the pointer query: plain host memory (here, with no
    device at all, any memory) is never launched on.  The stand-in pointers are never dereferenced."""
    lib = _lib.load()
    store, where = _filled_store(doubles)
    sel = torch.tensor([where[3], where[9], where[3]])
    plan, slot, records, nbytes, nrows = store.gather_plan(sel)
    fake = 0x10000
    hp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_int64))   # noqa: E731

    def call(data=store._data.data_ptr(), rows=store._rows.data_ptr(), p=plan, s=slot, r=records, arena=fake,
             arena_bytes=nbytes, arena_rows=fake, arena_nrows=nrows, plan_dev=fake):
        desc = _lib.JpegStore(data, store.nbytes, fake, store._host[0].data_ptr(), len(store), fake,
                              store._host[1].data_ptr(), store.table_sets, fake, store._host[2].data_ptr(), store._segs,
                              rows, store._rows.shape[0], store.chunk_bytes)
        return lib.coclr_jpeg_store_gather(C.byref(desc), plan_dev, hp(p), p.shape[0], hp(s), hp(r), s.numel(), arena,
                                           arena_bytes, arena_rows, arena_nrows, None)

    assert call() == 1                                           # the store's bytes are plain host memory
    assert lib.coclr_jpeg_store_gather(None, fake, hp(plan), 2, hp(slot), hp(records), 3, fake, nbytes, fake, nrows,
                                       None) == 1
    for kw in (dict(data=None), dict(rows=None), dict(arena=None), dict(arena_rows=None), dict(plan_dev=None),
               dict(arena=fake + 8), dict(arena_bytes=nbytes - 1), dict(arena_nrows=nrows - 1)):
        assert call(**kw) == 1, kw
    bad = plan.clone()
    bad[1, 0] = len(store)                                       # a selection of nframes
    assert call(p=bad) == 1


@pytest.fixture(scope="module")
def gather_check(tmp_path_factory):
    """tools/jpeg_gather_check.cpp built with the sanitizers and run once."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("jpeg_gather") / "jpeg_gather_check")
    # the sanitizer runtimes are linked statically: the program then does not care what else a host preloads
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "jpeg_gather_check.cpp"), "-o", exe])
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_host_build_gather_arithmetic_holds(gather_check):
    out, err = gather_check.stdout.decode(), gather_check.stderr.decode()
    assert gather_check.returncode == 0 and "ERROR" not in err and "runtime error" not in err, out + err
    far, copies, garbage, refusals, failed = [int(v) for v in re.findall(r"\d+", out.splitlines()[-1])]
    assert failed == 0 and "differs" not in out
    assert far == 14 * 13 and copies == 16 * 49 * 3 and garbage == 8 * copies and refusals >= 14
