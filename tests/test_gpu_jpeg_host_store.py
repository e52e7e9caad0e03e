"""The host-resident JPEG store on one MI355X (coclr_amd/jpeg.py: Store(bytes_on="host"), Store.save / Store.load;
csrc/jpeg.hip: coclr_jpeg_store_gather): the compressed bytes and the chunk rows in pinned host memory, the selection's
distinct frames copied to a device arena in one launch and decoded there.  Every fixture of tests/golden/jpeg_frames.pt
is added as its own pack in a shuffled order to a host store and to a device store; rows, frames, offsets and status
must be equal with ZERO tolerance (every comparison is torch.equal), and the frames PIL's own bytes.  Pinned allocations
stay below 1 MiB.  No pageable pointer ever reaches a kernel: the refusals below are refused on the host."""
import random

import numpy as np
import pytest
import torch

import _jpeg_cases as J

pytestmark = pytest.mark.gpu

FILL = 0x5a
CHUNKS = (None, 8, 65536)
CAPACITY = 1 << 17           # bytes: at chunk_bytes 8 the rows take twice that


def _picks():
    """A seeded permutation of all 54 fixtures, then some of them again."""
    order = random.Random(11).sample(range(54), 54)
    return order + [order[5], order[5], 0, order[40], 53, 0]


def _filled(store):
    from coclr_amd import jpeg
    order = random.Random(3).sample(range(54), 54)
    where = {i: store.add(jpeg.pack([J.raw(J.cases()[i])])) for i in order}
    assert [where[i] for i in order] == list(range(54))
    return where


@pytest.fixture(scope="module")
def stores():
    """Per chunk size (host store, device store, fixture -> id), filled alike."""
    from coclr_amd import jpeg
    out = {}
    for chunk_bytes in CHUNKS:
        host = jpeg.Store(CAPACITY, 64, chunk_bytes=chunk_bytes, bytes_on="host")
        dev = jpeg.Store(CAPACITY, 64, chunk_bytes=chunk_bytes)
        where = _filled(host)
        assert _filled(dev) == where
        assert host._data.is_pinned() and host._rows.is_pinned() and not host._data.is_cuda and dev._data.is_cuda
        assert all(t.is_cuda for t in host._dev)
        assert host._data.numel() + 16 <= 1 << 20 and host._rows.numel() * 4 <= 1 << 20
        out[chunk_bytes] = (host, dev, where)
    return out


@pytest.fixture(scope="module")
def reference(stores):
    """The device store's decode of _picks(), once."""
    _, dev, where = stores[None]
    return dev.decode([where[i] for i in _picks()], return_status=True)


def _same_frames(got, want, n):
    assert len(got) == len(want) == n and torch.equal(got.offset, want.offset)
    assert torch.equal(got.height, want.height) and torch.equal(got.width, want.width)
    assert all(torch.equal(got.frame(k), want.frame(k)) for k in range(n))


@pytest.mark.parametrize("chunk_bytes", CHUNKS)
def test_rows_are_the_device_stores(stores, chunk_bytes):
    host, dev, _ = stores[chunk_bytes]
    assert host.chunk_rows == dev.chunk_rows > 0 and host.nbytes == dev.nbytes
    assert torch.equal(host._rows[:host.chunk_rows], dev._rows[:dev.chunk_rows].cpu())
    assert torch.equal(host._data[:host.nbytes], dev._data[:dev.nbytes].cpu())
    assert all(torch.equal(a, b) for a, b in zip(host._host, dev._host))
    assert all(torch.equal(a, b) for a, b in zip(host._dev, dev._dev))
    if chunk_bytes == 8:
        assert host.chunk_rows > 1024 * 2                                              # several windows of the indexer


@pytest.mark.parametrize("chunk_bytes", CHUNKS)
def test_decode_equals_pil_and_the_device_store(stores, reference, chunk_bytes):
    host, dev, where = stores[chunk_bytes]
    cases, picks = J.cases(), _picks()
    ids = torch.tensor([where[i] for i in picks])
    want, want_status = reference
    for budget in (256 << 20, 40000):
        assert len(host.plan(ids, budget)[4]) >= (1 if budget > 40000 else 3)
        frames, status = host.decode(ids, return_status=True, max_stage_bytes=budget)
        assert host.decode.last_status is status and status.dtype == torch.int32
        assert not bool(status.any()) and torch.equal(status, want_status)
        _same_frames(frames, want, len(picks))
        for k, i in enumerate(picks):
            assert torch.equal(frames.frame(k).cpu(), cases[i]["rgb"]), cases[i]["name"]       # PIL's bytes
    # repeats crossed the bus once, and the arena is kept: the second call allocated nothing
    plan = host.gather_plan(ids)[0]
    assert plan.shape[0] == 54 < len(picks)
    kept = host._arena.data_ptr(), host._arena_rows.data_ptr()
    host.decode(ids.tolist()[:7])
    assert (host._arena.data_ptr(), host._arena_rows.data_ptr()) == kept
    for bad in ([54], [-1], []):
        with pytest.raises(ValueError):
            host.decode(bad)


def _batch(store, B=2, T=2, S=16):
    """B seeded plans over two fixture sizes, ids with repeats -> (ids (B, 2T), plans)."""
    from coclr_amd import staging
    geo = store._geo[:len(store)]
    groups = [torch.nonzero((geo[:, 0] == h) & (geo[:, 1] == w)).view(-1).tolist() for h, w in ((40, 56), (37, 45))]
    tt = staging.TrainTransform(S, T)
    rng, np_rng, pick = random.Random(0), np.random.RandomState(0), random.Random(1)
    ids, plans = [], []
    for b in range(B):
        ids.append([pick.choice(groups[b % 2]) for _ in range(2 * T)])
        plans.append(tt.draw(*store.frame_size(ids[-1][0]), rng=rng, np_rng=np_rng))
    ids[0][1] = ids[0][0]                                                              # a repeated id
    return torch.tensor(ids), plans


@pytest.mark.parametrize("chunk_bytes", CHUNKS)
def test_boxes_equal_the_device_stores_windowed_decode(stores, chunk_bytes):
    from coclr_amd import staging
    host, dev, _ = stores[chunk_bytes]
    ids, plans = _batch(host)
    sel, boxes = staging.clip_frames(ids, plans, 2)
    assert sel.shape == (8,) and len(set(sel.tolist())) < 8
    got, status = host.decode(sel, boxes, return_status=True)
    want, want_status = dev.decode(sel, boxes, return_status=True)
    assert torch.equal(status, want_status) and not bool(status.any())
    _same_frames(got, want, 8)
    assert got.height.tolist() == boxes[:, 3].tolist() and got.width.tolist() == boxes[:, 2].tolist()


def _by_hand(store, sel):
    """coclr_jpeg_store_gather called by hand into arenas filled with 0x5a, 64 more bytes behind them."""
    from coclr_amd import ops
    plan, slot, records, nbytes, nrows = store.gather_plan(torch.as_tensor(sel))
    arena = torch.full((nbytes + 64,), FILL, dtype=torch.uint8, device="cuda")
    arena_rows = torch.full((max(1, nrows) + 4, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    ops.jpeg_store_gather(store._buffers(), plan.cuda(), plan, slot, records, arena[:nbytes], arena_rows[:max(1, nrows)])
    return plan, records, nbytes, nrows, arena.cpu(), arena_rows.cpu()


def _check_arena(store, sel, got):
    plan, records, nbytes, nrows, arena, arena_rows = got
    rec, rows = store._host[0], store._rows.cpu()
    data = store._data.cpu()
    covered = torch.zeros(arena.numel(), dtype=torch.bool)
    for i, f in enumerate(torch.as_tensor(sel).tolist()):
        b, l, a = int(rec[f, 0]), int(rec[f, 1]), int(records[i, 0])
        assert a % 16 == b % 16 and torch.equal(arena[a:a + l], data[b:b + l])
        covered[a & ~15:(a + l + 15) & ~15] = True
        if int(rec[f, 3]) == 1:
            k, r = int(store._lanes[f]), int(records[i, 6])
            assert torch.equal(arena_rows[r:r + k], rows[int(rec[f, 6]):int(rec[f, 6]) + k])
    assert not bool(covered[nbytes:].any()) and bool((arena[~covered] == FILL).all()) and int((~covered).sum()) >= 64
    assert bool((arena_rows[nrows:] == 0x5a5a5a5a).all())


@pytest.mark.parametrize("chunk_bytes", CHUNKS)
def test_gather_by_hand(stores, chunk_bytes):
    host, dev, where = stores[chunk_bytes]
    sel = [where[i] for i in _picks()]
    _check_arena(host, sel, _by_hand(host, sel))
    _check_arena(dev, sel, _by_hand(dev, sel))                                         # a device store is taken alike
    _check_arena(host, sel[3:4], _by_hand(host, sel[3:4]))                             # one frame


def test_gather_at_every_residue_of_the_base():
    """A one-frame store whose cursor was moved by r = 0..15 first: the shortest fixture, whose head and tail words
    meet (its entropy-coded bytes are fewer than 16), and one of a few hundred bytes."""
    from coclr_amd import jpeg
    sizes = {c["name"]: jpeg.pack([J.raw(c)])[0].numel() for c in J.cases()}
    short = min(sizes, key=sizes.get)
    assert sizes[short] < 16
    for name in (short, "45x37_420_q100_noise"):
        c = J.case(name)
        want = None
        for r in range(16):
            store = jpeg.Store(16384, 2, chunk_bytes=8, bytes_on="host")
            store._data.fill_(0xa5)
            store._advance_cursor(r)
            assert store.add(jpeg.pack([J.raw(c)])) == 0 and int(store._host[0][0, 0]) == r
            got = _by_hand(store, [0])
            assert int(got[1][0, 0]) == r and got[2] == (r + sizes[name] + 15) & ~15
            _check_arena(store, [0], got)
            frames = store.decode([0, 0])
            assert torch.equal(frames.frame(0).cpu(), c["rgb"]) and torch.equal(frames.frame(1).cpu(), c["rgb"])
            want = store._rows[:store.chunk_rows].clone() if want is None else want
            assert torch.equal(store._rows[:store.chunk_rows], want)                   # rows do not depend on the base


def test_refusals_launch_nothing(stores):
    from coclr_amd import _lib, ops
    host, _, where = stores[None]
    sel = [where[i] for i in _picks()[:9]]
    plan, slot, records, nbytes, nrows = host.gather_plan(torch.as_tensor(sel))
    arena = torch.full((nbytes + 64,), FILL, dtype=torch.uint8, device="cuda")
    arena_rows = torch.full((nrows + 4, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    d_plan = plan.cuda()

    def refused(buffers=None, p=plan, size=nbytes):
        with pytest.raises(_lib.HipLibraryError):
            ops.jpeg_store_gather(buffers or host._buffers(), d_plan, p, slot, records, arena[:size], arena_rows[:nrows])
        torch.cuda.synchronize()                                                       # and no error was left behind
        assert bool((arena == FILL).all()) and bool((arena_rows == 0x5a5a5a5a).all())

    plain = host._data.clone()                                                         # the same bytes, not pinned
    assert not plain.is_pinned() and not plain.is_cuda
    refused(buffers=(plain,) + host._buffers()[1:])
    plain_rows = host._rows.clone()
    assert not plain_rows.is_pinned()
    refused(buffers=host._buffers()[:10] + (plain_rows,) + host._buffers()[11:])
    refused(size=nbytes - 1)                                                           # an arena one byte too small
    outside = plan.clone()
    outside[-1, 0] = len(host)                                                         # a selection of nframes
    refused(p=outside)
    # the same call, unedited, goes through
    ops.jpeg_store_gather(host._buffers(), d_plan, plan, slot, records, arena[:nbytes], arena_rows[:nrows])
    _check_arena(host, sel, (plan, records, nbytes, nrows, arena.cpu(), arena_rows.cpu()))


def test_training_staging_from_a_host_store(stores):
    from coclr_amd import staging
    host, dev, _ = stores[None]
    ids, plans = _batch(host)
    got = staging.stage_train_clips_ragged(host.decode(ids.view(-1)), plans, 16)
    want = staging.stage_train_clips_ragged(dev.decode(ids.view(-1)), plans, 16)
    assert got.shape == (2, 2, 3, 2, 16, 16) and torch.equal(got, want)
    sel, boxes = staging.clip_frames(ids, plans, 2)
    cropped = staging.stage_train_clips_cropped(host.decode(sel, boxes), plans, 16)
    assert torch.equal(cropped, staging.stage_train_clips_cropped(dev.decode(sel, boxes), plans, 16))
    assert torch.equal(cropped, want)


class _TableModel(torch.nn.Module):
    """Stands in for the classifier: a clip -> the row of fixed tables that its first red byte names."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.logits = torch.nn.Parameter(torch.randn(256, 11, generator=g) * 3, requires_grad=False)
        self.feats = torch.nn.Parameter(torch.randn(256, 6, generator=g), requires_grad=False)

    def forward(self, block):
        from coclr_amd import staging
        x = block[:, 0, 0, 0, 0].double() * staging.IMAGENET_STD[0] + staging.IMAGENET_MEAN[0]
        idx = (x * 255).round().long().clamp(0, 255)
        return self.logits[idx], self.feats[idx]


def test_evaluator_from_a_host_store():
    """VideoEvaluator.add_stored: two videos (the fixtures of one frame size each), clips of T = 2 at S = 16."""
    from coclr_amd import jpeg
    from coclr_amd.eval.video import VideoEvaluator
    model = _TableModel().cuda().eval()
    results = []
    for bytes_on in ("host", "device"):
        store = jpeg.Store(CAPACITY, 64, bytes_on=bytes_on)
        videos = []
        for label, (H, W) in enumerate(((37, 45), (40, 56))):
            cases = [c for c in J.cases() if (c["height"], c["width"]) == (H, W)]
            ids = [store.add(jpeg.pack([J.raw(c)])) for c in cases]
            assert len(cases) >= 13
            videos.append((ids[0], len(cases), [[[3, 5], [5, 9]], [[12, 0], [0, 1]]][label], label))
        ev = VideoEvaluator(model, batch_clips=8)
        assert ev.add_stored(store, videos, crops="center", crop_size=16, out_size=16) == [0, 1]
        results.append(ev.finish())
    got, want = results
    assert torch.equal(got.probs, want.probs) and torch.equal(got.features, want.features)
    assert torch.equal(got.labels, want.labels) and torch.equal(got.top1, want.top1)


@pytest.mark.parametrize("kinds", [("device", "host"), ("host", "device")])
def test_save_and_load_across_kinds(stores, reference, tmp_path, monkeypatch, kinds):
    from coclr_amd import jpeg, ops
    host, dev, where = stores[None]
    source = host if kinds[0] == "host" else dev
    source.save(str(tmp_path / "store"))

    def no_indexing(*a, **k):
        raise AssertionError("a loaded store indexes nothing")

    monkeypatch.setattr(ops, "jpeg_store_index", no_indexing)
    monkeypatch.setattr(jpeg, "pack", no_indexing)
    monkeypatch.setattr(jpeg, "parse", no_indexing)
    loaded = jpeg.Store.load(str(tmp_path / "store"), bytes_on=kinds[1])
    assert loaded.bytes_on == kinds[1] and len(loaded) == 54 and loaded.nbytes == source.nbytes
    assert loaded._data.is_pinned() == (kinds[1] == "host") and loaded._data.is_cuda == (kinds[1] == "device")
    assert torch.equal(loaded._rows[:loaded.chunk_rows].cpu(), source._rows[:source.chunk_rows].cpu())
    picks = _picks()
    frames, status = loaded.decode([where[i] for i in picks], return_status=True)
    want, want_status = reference
    assert torch.equal(status, want_status)
    _same_frames(frames, want, len(picks))
