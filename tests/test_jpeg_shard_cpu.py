"""CPU tier of the sharded JPEG store (coclr_amd/jpeg.py: class ShardedStore; include/coclr_hip.h:
coclr_jpeg_store_gather_shards): the books of a store sealed from 1, 2, 3 and 8 shards against ONE Store given the same
packs in global order, the shard gather's host tables against a brute-force placement, decode through recording doubles,
the refusals, the entry point's host refusals through ctypes, and the gather arithmetic of csrc/jpeg_core.h compiled for
the host under AddressSanitizer and UBSan (tools/jpeg_shard_check.cpp).  The launches are doubles; the shard gather's is
a numpy restatement of the copy.  `join`'s agreed failure runs as two CPU processes over gloo.  Nothing here needs a GPU
and nothing is preloaded into Python."""
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
SHARDS = (1, 2, 3, 8)


def _numpy_gather_shards(shards, plan, plan_host, shard, shard_host, slot_host, frames_host, arena, arena_rows):
    """What jpeg_store_gather_kernel<shard_sources> copies, restated: per plan row, from the row's own source, the
    16-byte words of the hull, then the rows."""
    out, out_rows = arena.numpy(), arena_rows.numpy().reshape(-1, 4)
    for (frame, src, ln, dst, srow, nrows, drow, lane), s in zip(plan_host.tolist(), shard_host.tolist()):
        data, rows = shards[s][0].numpy(), shards[s][1].numpy().reshape(-1, 4)
        if ln:
            w0, w1 = src >> 4, (src + ln + 15) >> 4
            have = min(w1 * 16, data.size) - w0 * 16             # (the room behind the bytes is never read back)
            out[(dst >> 4) * 16:(dst >> 4) * 16 + have] = data[w0 * 16:w0 * 16 + have]
        out_rows[drow:drow + nrows] = rows[srow:srow + nrows]


@pytest.fixture
def doubles(monkeypatch):
    """Every launch replaced: the two gathers copy as the kernels do and record their host tables; the decode entries
    record the store they were given (the arena's bytes and rows cloned)."""
    calls = {"gather": [], "shards": [], "decode": []}

    def gather(store, plan, plan_host, slot_host, frames_host, arena, arena_rows):
        calls["gather"].append((plan_host.clone(), slot_host.clone(), frames_host.clone()))
        _numpy_gather_shards([(store[0], store[10])], plan, plan_host, None, torch.zeros(plan_host.shape[0],
                             dtype=torch.int64), slot_host, frames_host, arena, arena_rows)

    def gather_shards(shards, plan, plan_host, shard, shard_host, slot_host, frames_host, arena, arena_rows):
        assert torch.equal(plan, plan_host) and torch.equal(shard, shard_host)          # the device copies
        calls["shards"].append((plan_host.clone(), shard_host.clone(), slot_host.clone(), frames_host.clone(),
                                len(shards)))
        _numpy_gather_shards(shards, plan, plan_host, shard, shard_host, slot_host, frames_host, arena, arena_rows)

    def decode(store, sel, sel_host, geom, geom_host, *rest):
        window = rest[1].clone() if len(rest) == 8 else None                            # (the windowed entry)
        data, frames, frames_host, n, tables, tables_host, sets, segs, segs_host, nsegs, rows, cb = store
        calls["decode"].append(dict(data=data.clone(), records=frames_host.clone(), dev_records=frames.clone(), n=n,
                                    tables=tables_host[:ops.JS_TABLE_PAD + sets * ops.JS_TABLE_WORDS].clone(),
                                    dev_tables=tables.clone(), segs=segs_host[:nsegs].clone(),
                                    dev_segs=segs[:nsegs].clone(), rows=rows.clone(), chunk_bytes=cb,
                                    sel=sel_host.clone(), geom=geom_host.clone(), window=window))
        rest[-1].zero_()                                                                # status

    monkeypatch.setattr(ops, "jpeg_store_index", lambda store, f0, f1: None)
    monkeypatch.setattr(ops, "jpeg_store_gather", gather)
    monkeypatch.setattr(ops, "jpeg_store_gather_shards", gather_shards)
    monkeypatch.setattr(ops, "jpeg_decode_store", decode)
    monkeypatch.setattr(ops, "jpeg_decode_store_window", decode)
    return calls


def _packs():
    return [jpeg.pack([J.raw(c) for c in group]) for group in J.groups().values()]


def _dealt(nshards, chunk_bytes=None, single_on="host"):
    """The packs dealt round-robin to `nshards` stores -- at 8 to seven, shard 2 staying EMPTY; kinds alternate, every
    shard's write cursor starts at another residue mod 16 and its rows say whose they are -> (the shards, ONE store
    given the same packs in global order, its rows copied frame by frame from the shards')."""
    packs = _packs()
    empty = 2 if nshards == 8 else None
    filled = [s for s in range(nshards) if s != empty]
    stores, order = [], []
    for s in range(nshards):
        st = jpeg.Store(1 << 19, 64, chunk_bytes=chunk_bytes, device="cpu", bytes_on=("device", "host")[s % 2])
        if s != empty:
            st._advance_cursor(3 * s + 1)
            for p in packs[filled.index(s)::len(filled)]:
                st.add(p)
            order += packs[filled.index(s)::len(filled)]
            st._rows[:st.chunk_rows] = torch.arange(st.chunk_rows * 4, dtype=torch.int32).view(-1, 4) + (s << 20)
        stores.append(st)
    single = jpeg.Store(1 << 20, 64, chunk_bytes=chunk_bytes, device="cpu", bytes_on=single_on)
    for p in order:
        single.add(p)
    g = 0
    for st in stores:
        for f in range(len(st)):
            if int(st._host[0][f, 3]) == 1:
                k, a, b = int(st._lanes[f]), int(single._host[0][g, 6]), int(st._host[0][f, 6])
                assert k == int(single._lanes[g])
                single._rows[a:a + k] = st._rows[b:b + k]
            g += 1
    assert g == len(single) == 54
    return stores, single


@pytest.mark.parametrize("nshards", SHARDS)
def test_books_are_one_stores(doubles, nshards):
    stores, single = _dealt(nshards)
    before = [(len(s), s.nbytes, [t.clone() for t in s._host]) for s in stores]
    sh = jpeg.ShardedStore(stores)
    n = len(single)
    assert len(sh) == n == 54 and sh.chunk_bytes == single.chunk_bytes == 64
    assert sh.nbytes == sum(s.nbytes for s in stores) and sh.table_sets == single.table_sets
    lens = torch.tensor([len(s) for s in stores])
    assert torch.equal(sh.bases, lens.cumsum(0) - lens)
    if nshards == 8:
        assert len(stores[2]) == 0 and int(sh.bases[2]) == int(sh.bases[3])             # the empty shard
    ids = torch.arange(n)
    assert torch.equal(sh.shard_of(ids), torch.repeat_interleave(torch.arange(nshards), lens))
    assert [sh.frame_size(i) for i in range(n)] == [single.frame_size(i) for i in range(n)]
    assert torch.equal(sh._geo, single._geo[:n]) and torch.equal(sh._lanes, single._lanes[:n])
    # the union: each distinct set once, and the remapped records name the same 768 words
    rec, tables, segs = sh._host
    W, T = ops.JS_TABLE_WORDS, ops.JS_TABLE_PAD
    assert tables.numel() == T + sh.table_sets * W and torch.equal(sh._dev_tables, tables)
    sets = [tables[T + i * W:T + (i + 1) * W].numpy().tobytes() for i in range(sh.table_sets)]
    assert len(set(sets)) == len(sets)
    for g in range(n):
        s = int(sh.shard_of(g))
        own = stores[s]._host[0][g - int(sh.bases[s])]
        a = T + int(own[4]) * W
        assert sets[int(rec[g, 4])] == stores[s]._host[1][a:a + W].numpy().tobytes()
    one = single._host[0][:n]
    # the records: the single store's, but for the first byte and the first row, which count inside the shard
    assert torch.equal(rec[:, [1, 2, 3, 4, 5, 7]], one[:, [1, 2, 3, 4, 5, 7]])
    assert torch.equal(tables, single._host[1][:tables.numel()])
    # the shifted segment words are those of the single store
    assert sh._segs == single._segs > 0 and torch.equal(segs[:sh._segs], single._host[2][:single._segs])
    assert torch.equal(sh._dev_segs, segs)
    own = torch.cat([s._host[0][:len(s)] for s in stores])
    assert torch.equal(rec[:, [0, 6]], own[:, [0, 6]])
    # the stores passed in are untouched and stay usable; what they take later is not seen
    for s, (ln, nb, host) in zip(stores, before):
        assert (len(s), s.nbytes) == (ln, nb) and all(torch.equal(a, b) for a, b in zip(s._host, host))
    stores[0].add(_packs()[0])
    assert len(sh) == 54 and torch.equal(sh._host[0], rec)


def _brute_force(sh, stores, sel):
    """The placement written out frame by frame: distinct (shard, frame) pairs in order, each hull after the last."""
    pairs = sorted({(int(sh.shard_of(g)), g - int(sh.bases[int(sh.shard_of(g))])) for g in sel})
    plan, shard, end, rows, lanes, where = [], [], 0, 0, 0, {}
    for s, f in pairs:
        base, ln, _, nseg, _, _, row, _ = stores[s]._host[0][f].tolist()
        words = ((base + ln + 15) // 16 - base // 16) if ln else 0
        nrows = int(stores[s]._lanes[f]) if nseg == 1 else 0
        dst = end + base % 16
        plan.append([f, base, ln, dst, row, nrows, rows, lanes])
        shard.append(s)
        where[(s, f)] = (len(plan) - 1, dst, rows)
        end, rows, lanes = end + 16 * words, rows + nrows, lanes + words + nrows
    return plan, shard, end, rows, where


@pytest.mark.parametrize("nshards", SHARDS)
@pytest.mark.parametrize("chunk_bytes", [None, 8])
def test_gather_plan_against_brute_force(doubles, nshards, chunk_bytes):
    stores, single = _dealt(nshards, chunk_bytes)
    sh = jpeg.ShardedStore(stores)
    g = torch.Generator().manual_seed(11 + nshards)
    picks = torch.randperm(54, generator=g).tolist()[:40] + [5, 5, 17]
    picks.insert(3, picks[0]), picks.insert(20, picks[0])                     # picks[0] three times
    for sel in (picks, list(range(54)), [53], [7, 7, 7]):
        plan, slot, records, nbytes, nrows, shard = sh.gather_plan(torch.tensor(sel))
        want_plan, want_shard, end, rows, where = _brute_force(sh, stores, sel)
        assert plan.tolist() == want_plan and shard.tolist() == want_shard and (nbytes, nrows) == (end, rows)
        m = plan.shape[0]
        assert m == len(set(sel)) and plan.dtype == shard.dtype == torch.int64 and shard.shape == (m,)
        src, ln, dst = plan[:, 1], plan[:, 2], plan[:, 3]
        assert bool(((dst - src) % 16 == 0).all())                             # congruent to the SHARD byte
        hull0, hull1 = dst & ~15, (dst + ln + 15) & ~15
        assert int(hull0[0]) == 0 and torch.equal(hull0[1:], hull1[:-1]) and int(hull1[-1]) == nbytes     # no gaps
        assert torch.equal(plan[:, 6], plan[:, 5].cumsum(0) - plan[:, 5])      # rows consecutive
        key = shard * (1 << 32) + plan[:, 0]
        assert bool((key[1:] > key[:-1]).all())                                # ordered by (shard, frame)
        assert torch.equal(sh.bases[shard] + plan[:, 0], torch.tensor(sorted(set(sel))))
        # repeats share one slot; the records are the sealed ones moved to the arena
        for i, gid in enumerate(sel):
            s = int(sh.shard_of(gid))
            j, d, r = where[(s, gid - int(sh.bases[s]))]
            assert int(slot[i]) == j
            want = sh._host[0][gid].clone()
            want[0], want[6] = d, r
            assert torch.equal(records[i], want)
    if len(set(picks)) < len(picks):
        thrice = [i for i, p in enumerate(picks) if p == picks[0]]
        slot = sh.gather_plan(torch.tensor(picks))[1]
        assert len(thrice) >= 3 and len(set(slot[thrice].tolist())) == 1


def test_one_shard_tables_equal_the_stores(doubles):
    stores, single = _dealt(1)
    sh = jpeg.ShardedStore(stores)
    sel = torch.tensor([9, 3, 3, 50, 0, 9])
    got, want = sh.gather_plan(sel), stores[0].gather_plan(sel)
    assert len(got) == 6 and len(want) == 5 and got[5].tolist() == [0] * 4
    assert all(torch.equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3:5] == want[3:5]
    a, b = sh.plan(sel, 40000), stores[0].plan(sel, 40000)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[3] == b[3] and a[5] == b[5]
    assert all(x[:2] == y[:2] and torch.equal(x[2], y[2]) and torch.equal(x[3], y[3]) for x, y in zip(a[4], b[4]))


@pytest.mark.parametrize("nshards", SHARDS)
@pytest.mark.parametrize("boxed", [False, True])
def test_decode_through_the_doubles(doubles, nshards, boxed):
    """The arena a ShardedStore decodes from holds what the single HOST store's arena holds, frame by frame, under
    records that differ in nothing but the residue of the first byte; tables and segment words are the single store's."""
    stores, single = _dealt(nshards)
    sh = jpeg.ShardedStore(stores)
    g = torch.Generator().manual_seed(5)
    ids = torch.randperm(54, generator=g).tolist() + [4, 4, 31, 0]
    boxes = None
    if boxed:
        boxes = [[0, 0, *sh.frame_size(i)] for i in ids]
        boxes[1] = [1, 1, 3, 2]
    for budget in (256 << 20, 40000):
        doubles["decode"].clear()
        got, status = sh.decode(ids, boxes, return_status=True, max_stage_bytes=budget)
        assert sh.decode.last_status is status and jpeg.Store.decode.last_status is status
        ours = list(doubles["decode"])
        doubles["decode"].clear()
        want = single.decode(ids, boxes, max_stage_bytes=budget)
        theirs = list(doubles["decode"])
        assert len(ours) == len(theirs) >= (1 if budget > 40000 else 3)
        assert torch.equal(got.offset, want.offset) and torch.equal(got.height, want.height)
        assert torch.equal(got.width, want.width)
        for a, b in zip(ours, theirs):
            assert a["n"] == b["n"] == len(ids) and a["chunk_bytes"] == b["chunk_bytes"]
            assert torch.equal(a["sel"], b["sel"]) and torch.equal(a["geom"], b["geom"])
            assert (a["window"] is None) == (not boxed) and (not boxed or torch.equal(a["window"], b["window"]))
            assert torch.equal(a["tables"], b["tables"]) and torch.equal(a["segs"], b["segs"])
            assert torch.equal(a["dev_tables"], a["tables"]) and torch.equal(a["dev_segs"], a["segs"])
            assert torch.equal(a["dev_records"], a["records"])
            ra, rb = a["records"], b["records"]
            assert torch.equal(ra[:, 1:], rb[:, 1:]) and not torch.equal(ra[:, 0], rb[:, 0])
            assert bool(((ra[:, 0] - sh._host[0][ids, 0]) % 16 == 0).all())
            for i in range(len(ids)):
                x, y, ln = int(ra[i, 0]), int(rb[i, 0]), int(ra[i, 1])
                assert torch.equal(a["data"][x:x + ln], b["data"][y:y + ln])
                if int(ra[i, 3]) == 1:
                    k, r = int(sh._lanes[ids[i]]), int(ra[i, 6])
                    assert k > 0 and torch.equal(a["rows"][r:r + k], b["rows"][r:r + k])
    plan, shard, slot, records, n = doubles["shards"][-1]
    assert n == nshards and plan.shape[0] == 54 and set(shard.tolist()) == {s for s in range(nshards) if len(stores[s])}
    # the arena is kept: a smaller call allocates nothing
    kept = sh._arena.data_ptr(), sh._arena_rows.data_ptr()
    sh.decode(ids[:5])
    assert (sh._arena.data_ptr(), sh._arena_rows.data_ptr()) == kept


def test_refusals(doubles):
    stores, single = _dealt(2)
    sh = jpeg.ShardedStore(stores)
    with pytest.raises(ValueError, match="sealed"):
        sh.add(_packs()[0])
    other = jpeg.Store(1 << 10, 4, chunk_bytes=8, device="cpu")
    with pytest.raises(ValueError, match="chunk_bytes"):
        jpeg.ShardedStore([stores[0], other])
    nine = [jpeg.Store(1 << 10, 4, device="cpu") for _ in range(9)]
    with pytest.raises(ValueError, match="1..8"):
        jpeg.ShardedStore(nine)
    with pytest.raises(ValueError, match="1..8"):
        jpeg.ShardedStore([])
    assert len(jpeg.ShardedStore(nine[:8])) == 0                                # eight, all empty: legal, and no id is
    for bad in ([54], [-1], [], [0.5], [True]):
        with pytest.raises(ValueError):
            sh.decode(bad)
        with pytest.raises(ValueError):
            jpeg.ShardedStore(nine[:8]).decode(bad)
    with pytest.raises(ValueError):
        sh.shard_of([54])
    with pytest.raises(ValueError):
        sh.frame_size(54)
    W, H = sh.frame_size(3)
    for boxes in ([[0, 0, W + 1, H]], [[0, 0, 0, 1]], [[0, 0, 1]], [[0.5, 0, 1, 1]], [[0, 0, 1, 1], [0, 0, 1, 1]]):
        with pytest.raises(ValueError):
            sh.decode([3], boxes)
    assert not doubles["shards"] and not doubles["decode"]                      # refused before any launch
    with pytest.raises(ValueError, match="host"):                               # before anything collective
        jpeg.ShardedStore.join(stores[1])
    sh.close()
    with pytest.raises(ValueError, match="closed"):
        sh.decode([0])
    sh.close()                                                                  # twice is harmless
    assert stores[0].decode([0]) is not None                                    # the shard is its owner's again


def test_shard_entry_point_is_declared_exported_and_bound():
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "coclr_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\bint\s+(coclr_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (coclr_[a-z0-9_]+)", out))
    assert "coclr_jpeg_store_gather_shards" in declared & exported & set(_lib.EXPORTED_SYMBOLS)
    assert lib.coclr_abi_version() == _lib.ABI_VERSION == 26
    args = re.search(r"int coclr_jpeg_store_gather_shards\(([^)]*)\)", header).group(1).split(",")
    assert len(args) == len(_lib._SIGNATURES["coclr_jpeg_store_gather_shards"]) == 15
    assert ops.JG_MAX_SHARDS == 8 and "JG_MAX_SHARDS = 8" in open(os.path.join(ROOT, "coclr_amd", "csrc",
                                                                                 "jpeg_core.h")).read()


def test_shard_entry_point_refuses_without_a_device(doubles):
    """Every refusal the header lists, from the host copies and at the latest from the pointer query: with no device
    at all, any memory is refused, so the call as planned returns 1 as well.  Return code 1 (COCLR_EINVAL) before
    any launch; the stand-in device pointers are never dereferenced."""
    lib = _lib.load()
    stores, _ = _dealt(3)
    sh = jpeg.ShardedStore(stores)
    sel = torch.tensor([3, 30, 9, 3, 50])
    plan, slot, records, nbytes, nrows, shard = sh.gather_plan(sel)
    assert shard.tolist() == sorted(shard.tolist()) and len(set(shard.tolist())) == 3
    fake = 0x10000
    hp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_int64))   # noqa: E731

    def call(descs=None, nshards=None, p=plan, sc=shard, s=slot, r=records, arena=fake, arena_bytes=nbytes,
             arena_rows=fake, arena_nrows=nrows, plan_dev=fake, shard_dev=fake, shard_host=True, null=None, **edit):
        descs = [ops.jpeg_shard_desc(*src) for src in sh._sources] if descs is None else descs
        for k, v in edit.items():
            setattr(descs[1], k, v)
        ptrs = [None if i == null else C.pointer(d) for i, d in enumerate(descs)]
        table = (C.POINTER(_lib.JpegStore) * len(descs))(*ptrs)
        return lib.coclr_jpeg_store_gather_shards(table, len(descs) if nshards is None else nshards, plan_dev, hp(p),
                                                  shard_dev, hp(sc) if shard_host else None, p.shape[0], hp(s), hp(r),
                                                  s.numel(), arena, arena_bytes, arena_rows, arena_nrows, None)

    assert call() == 1                                           # the shards' bytes are plain host memory
    one = [ops.jpeg_shard_desc(*sh._sources[0])]
    assert call(nshards=0) == 1 and call(nshards=9) == 1 and call(nshards=-1) == 1
    assert call(descs=one * 9) == 1                              # nine sources
    assert lib.coclr_jpeg_store_gather_shards(None, 3, fake, hp(plan), fake, hp(shard), plan.shape[0], hp(slot),
                                              hp(records), slot.numel(), fake, nbytes, fake, nrows, None) == 1
    for i in range(3):
        assert call(null=i) == 1                                 # a null shard
    for kw in (dict(chunk_bytes=8), dict(chunk_bytes=7), dict(data=None), dict(rows=None), dict(tables_host=None),
               dict(frames_host=None), dict(data=stores[1]._data.data_ptr() + 8), dict(data_bytes=0), dict(nrows=0),
               dict(nframes=-1), dict(nframes=0), dict(table_sets=0)):
        assert call(**kw) == 1, kw                               # chunk sizes that differ, and a shard's own fields
    for kw in (dict(arena=None), dict(arena_rows=None), dict(plan_dev=None), dict(shard_dev=None),
               dict(shard_host=False), dict(arena=fake + 8), dict(shard_dev=fake + 4), dict(arena_bytes=nbytes - 1),
               dict(arena_nrows=nrows - 1)):
        assert call(**kw) == 1, kw
    for value in (3, -1, 8, 1 << 40):                            # a shard index outside [0, nshards)
        bad = shard.clone()
        bad[-1] = value
        assert call(sc=bad) == 1, value
    swapped = torch.cat([shard[1:2], shard[:1], shard[2:]])      # rows not ordered by (shard, frame)
    assert call(sc=swapped) == 1
    same = shard.clone()
    same[1] = same[0]                                            # row 1 now claims row 0's shard: its frame is not there
    assert call(sc=same) == 1
    bad = plan.clone()
    bad[0, 0] = len(stores[int(shard[0])])                       # a frame of nframes
    assert call(p=bad) == 1
    bad = plan.clone()
    bad[1, 3] += 1                                               # the congruence
    assert call(p=bad) == 1
    bad = slot.clone()
    bad[0] = plan.shape[0]
    assert call(s=bad) == 1
    bad = records.clone()
    bad[2, 4] += 1                                               # a rebased record that is not the shard's, moved
    assert call(r=bad) == 1


@pytest.fixture(scope="module")
def shard_check(tmp_path_factory):
    """tools/jpeg_shard_check.cpp built with the sanitizers and run once."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("jpeg_shard") / "jpeg_shard_check")
    # the sanitizer runtimes are linked statically: the program then does not care what else a host preloads
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "jpeg_shard_check.cpp"), "-o", exe])
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_host_build_shard_gather_arithmetic_holds(shard_check):
    out, err = shard_check.stdout.decode(), shard_check.stderr.decode()
    assert shard_check.returncode == 0 and "ERROR" not in err and "runtime error" not in err, out + err
    copies, garbage, far, orders, failed = [int(v) for v in re.findall(r"\d+", out.splitlines()[-1])]
    assert failed == 0 and "differs" not in out
    # 16 residues x 49 lengths x {1, 2, 3, 8 shards, 8 with one empty}; 8 plans and 8 shard columns of random words each
    assert copies == 16 * 49 * 5 and garbage == 16 * copies and far == 14 * 13 and orders >= 12


def _join_worker(rank, port, q):
    """One rank of test_join_fails_on_every_rank_together: rank 1 cannot export its buffers."""
    try:
        import datetime
        import torch.distributed as dist
        import torch.multiprocessing.reductions as reductions
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=2, timeout=datetime.timedelta(seconds=60))

        def export(t):
            if rank == 1:
                raise RuntimeError("no handle for you")
            return (torch.zeros, (1,))                           # never opened: the peer failed first
        reductions.reduce_tensor = export
        ops.jpeg_store_index = lambda store, f0, f1: None
        store = jpeg.Store(1 << 16, 16, device="cpu")
        for p in _packs()[rank:rank + 2]:
            store.add(p)
        try:
            jpeg.ShardedStore.join(store)
            q.put((rank, "joined"))
        except RuntimeError as e:
            q.put((rank, "RuntimeError: %s" % e))
        assert store.add(_packs()[5]) > 0                        # nothing was sealed: the store is its owner's
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "FAIL: %s\n%s" % (e, traceback.format_exc())))


def test_join_fails_on_every_rank_together():
    """A rank that cannot export makes EVERY rank raise the same RuntimeError: none is left sharded, none waits.  Two
    CPU processes over gloo; the export is a double, nothing is mapped."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_join_worker, args=(r, 29743, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        results = dict(q.get(timeout=120) for _ in procs)
    finally:
        for p in procs:
            p.join(20)
        for p in procs:
            if p.is_alive():
                p.terminate()
    assert set(results) == {0, 1} and len(set(results.values())) == 1, results
    assert results[0].startswith("RuntimeError: coclr_amd: ShardedStore.join") and "no rank is sharded" in results[0]
