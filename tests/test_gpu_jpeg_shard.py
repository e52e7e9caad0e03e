"""The sharded JPEG store on one MI355X, in ONE process (coclr_amd/jpeg.py: class ShardedStore; csrc/jpeg.hip:
coclr_jpeg_store_gather_shards): every fixture of tests/golden/jpeg_frames.pt is its own pack, dealt round-robin to 1,
2, 3 and 8 shards -- one shard empty at 8, one in pinned host memory at 3 -- and to ONE Store in global order, which the
existing tests hold to PIL.  Frames, offsets and status must be equal with ZERO tolerance (every comparison is
torch.equal).  Only clean plans reach the kernel: what it does with a corrupt plan or shard column is proved on the host
(tools/jpeg_shard_check.cpp), and the refusals below are refused before any launch."""
import random

import numpy as np
import pytest
import torch

import _jpeg_cases as J
import _jpeg_window_cases as WC

pytestmark = pytest.mark.gpu

FILL = 0x5a
CAPACITY = 1 << 17


def _dealt(nshards, chunk_bytes):
    """-> (the shards, the single store, fixture index -> global id)."""
    from coclr_amd import jpeg
    order = random.Random(3).sample(range(54), 54)
    empty = 2 if nshards == 8 else None
    filled = [s for s in range(nshards) if s != empty]
    shards, dealt = [], []
    for s in range(nshards):
        kind = "host" if (nshards == 3 and s == 1) else "device"
        st = jpeg.Store(CAPACITY, 64, chunk_bytes=chunk_bytes, bytes_on=kind)
        if s != empty:
            st._advance_cursor(3 * s + 1)                                              # another residue in every shard
            mine = order[filled.index(s)::len(filled)]
            for i in mine:
                st.add(jpeg.pack([J.raw(J.cases()[i])]))
            dealt += mine
        shards.append(st)
    single = jpeg.Store(CAPACITY, 64, chunk_bytes=chunk_bytes)
    where = {i: single.add(jpeg.pack([J.raw(J.cases()[i])])) for i in dealt}
    assert sorted(where.values()) == list(range(54))
    return shards, single, where


@pytest.fixture(scope="module")
def dealt():
    made = {}

    def get(nshards, chunk_bytes):
        if (nshards, chunk_bytes) not in made:
            made[(nshards, chunk_bytes)] = _dealt(nshards, chunk_bytes)
        return made[(nshards, chunk_bytes)]
    return get


def _picks():
    """A seeded permutation of all 54 fixtures, then some of them again."""
    order = random.Random(11).sample(range(54), 54)
    return order + [order[5], order[5], 0, order[40], 53, 0]


def _same_frames(got, want, n):
    assert len(got) == len(want) == n and torch.equal(got.offset, want.offset)
    assert torch.equal(got.height, want.height) and torch.equal(got.width, want.width)
    assert all(torch.equal(got.frame(k), want.frame(k)) for k in range(n))


def test_one_shard_is_its_store(dealt):
    from coclr_amd import jpeg
    (store,), single, where = dealt(1, None)
    sh = jpeg.ShardedStore([store])
    assert len(sh) == 54 and sh.bases.tolist() == [0] and sh.nbytes == store.nbytes
    ids = [where[i] for i in _picks()]
    got, status = sh.decode(ids, return_status=True)
    want, want_status = store.decode(ids, return_status=True)
    assert sh.decode.last_status is status and status.dtype == torch.int32
    assert torch.equal(status, want_status) and not bool(status.any())
    _same_frames(got, want, len(ids))
    cases = J.cases()
    for k, i in enumerate(_picks()):
        assert torch.equal(got.frame(k).cpu(), cases[i]["rgb"]), cases[i]["name"]       # PIL's bytes
    for bad in ([54], [-1], []):
        with pytest.raises(ValueError):
            sh.decode(bad)


@pytest.mark.parametrize("chunk_bytes", [8, 64])
@pytest.mark.parametrize("nshards", [2, 3, 8])
def test_shards_equal_the_single_store(dealt, nshards, chunk_bytes):
    from coclr_amd import jpeg
    shards, single, where = dealt(nshards, chunk_bytes)
    if nshards == 3:
        assert shards[1]._data.is_pinned() and not shards[1]._data.is_cuda and shards[0]._data.is_cuda
    if nshards == 8:
        assert len(shards[2]) == 0
    sh = jpeg.ShardedStore(shards)
    assert len(sh) == 54 and sh.chunk_bytes == chunk_bytes and sh.table_sets == single.table_sets
    ids = torch.tensor([where[i] for i in _picks()])
    assert set(sh.shard_of(ids).tolist()) == {s for s in range(nshards) if len(shards[s])}
    want, want_status = single.decode(ids, return_status=True)
    assert not bool(want_status.any())
    for budget in (256 << 20, 40000):
        assert len(sh.plan(ids, budget)[4]) >= (1 if budget > 40000 else 3)
        got, status = sh.decode(ids, return_status=True, max_stage_bytes=budget)
        assert sh.decode.last_status is status and torch.equal(status, want_status)
        _same_frames(got, want, len(ids))
    # repeats were copied once, and the arena is kept
    assert sh.gather_plan(ids)[0].shape[0] == 54 < len(ids)
    kept = sh._arena.data_ptr(), sh._arena_rows.data_ptr()
    sh.decode(ids.tolist()[:7])
    assert (sh._arena.data_ptr(), sh._arena_rows.data_ptr()) == kept
    # the fixed box list of the windowed decode, every fixture
    picks = WC.all_boxes()
    sel = torch.tensor([where[i] for i, _ in picks])
    boxes = torch.tensor([b for _, b in picks], dtype=torch.int64)
    got, status = sh.decode(sel, boxes, return_status=True)
    want, want_status = single.decode(sel, boxes, return_status=True)
    assert torch.equal(status, want_status) and not bool(status.any())
    assert len(got) == len(picks) and torch.equal(got.offset, want.offset)
    assert torch.equal(got.height, want.height) and torch.equal(got.width, want.width)
    assert got.height.tolist() == boxes[:, 3].tolist() and got.width.tolist() == boxes[:, 2].tolist()
    sizes = 3 * boxes[:, 2] * boxes[:, 3]
    keep = torch.zeros(got.pixels.numel(), dtype=torch.bool)
    for o, n in zip(got.offset.tolist(), sizes.tolist()):
        keep[o:o + n] = True                                                           # (the padding is not compared)
    keep = keep.cuda()
    assert torch.equal(got.pixels[keep], want.pixels[keep])


def _at_every_residue(first):
    """A store (chunk_bytes 8) of 16 one-frame packs whose first bytes lie at the residues first, first + 1, ... mod 16."""
    from coclr_amd import jpeg
    store = jpeg.Store(CAPACITY, 32, chunk_bytes=8)
    store._data.fill_(0xa5)
    sizes = sorted(range(54), key=lambda i: J.cases()[i]["raw"].numel())
    for k in range(16):
        store._advance_cursor((first + k - store.nbytes) % 16)
        f = store.add(jpeg.pack([J.raw(J.cases()[sizes[(3 * k + first) % 54]])]))
        assert int(store._host[0][f, 0]) % 16 == (first + k) % 16
    assert sorted(set((store._host[0][:16, 0] % 16).tolist())) == list(range(16))
    return store


def _by_hand(sh, sel, edit=None):
    """coclr_jpeg_store_gather_shards called by hand into arenas filled with 0x5a, 64 more bytes behind them."""
    from coclr_amd import ops
    plan, slot, records, nbytes, nrows, shard = sh.gather_plan(torch.as_tensor(sel))
    arena = torch.full((nbytes + 64,), FILL, dtype=torch.uint8, device="cuda")
    arena_rows = torch.full((max(1, nrows) + 4, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    ops.jpeg_store_gather_shards(sh._sources, plan.cuda(), plan, shard.cuda(), shard, slot, records, arena[:nbytes],
                                 arena_rows[:max(1, nrows)])
    return plan, shard, records, nbytes, nrows, arena.cpu(), arena_rows.cpu()


def _check_arena(sh, shards, sel, got):
    plan, shard, records, nbytes, nrows, arena, arena_rows = got
    covered = torch.zeros(arena.numel(), dtype=torch.bool)
    for i, g in enumerate(torch.as_tensor(sel).tolist()):
        s = int(sh.shard_of(g))
        st, f = shards[s], g - int(sh.bases[s])
        rec, data, rows = st._host[0], st._data.cpu(), st._rows.cpu()
        b, l, a = int(rec[f, 0]), int(rec[f, 1]), int(records[i, 0])
        assert a % 16 == b % 16 and torch.equal(arena[a:a + l], data[b:b + l])
        covered[a & ~15:(a + l + 15) & ~15] = True
        if int(rec[f, 3]) == 1:
            k, r = int(st._lanes[f]), int(records[i, 6])
            assert k > 0 and torch.equal(arena_rows[r:r + k], rows[int(rec[f, 6]):int(rec[f, 6]) + k])
    # hulls without a gap up to the last one; everything beyond keeps its poison
    assert bool(covered[:nbytes].all()) and not bool(covered[nbytes:].any())
    assert bool((arena[nbytes:] == FILL).all()) and arena.numel() - nbytes == 64
    assert bool((arena_rows[nrows:] == 0x5a5a5a5a).all())


def test_gather_by_hand_at_every_residue():
    from coclr_amd import jpeg
    shards = [_at_every_residue(0), _at_every_residue(5)]
    sh = jpeg.ShardedStore(shards)
    sel = random.Random(7).sample(range(32), 32) + [3, 3, 20]
    got = _by_hand(sh, sel)
    assert got[0].shape[0] == 32 and got[1].tolist() == [0] * 16 + [1] * 16
    assert sorted(set((got[0][:16, 3] % 16).tolist())) == sorted(set((got[0][16:, 3] % 16).tolist())) == list(range(16))
    _check_arena(sh, shards, sel, got)
    _check_arena(sh, shards, [17], _by_hand(sh, [17]))                                 # one frame, of the second shard
    # and decoded from there: PIL's bytes
    frames = sh.decode(sel)
    single = jpeg.Store(CAPACITY, 32, chunk_bytes=8)
    sizes = sorted(range(54), key=lambda i: J.cases()[i]["raw"].numel())
    for first in (0, 5):
        for k in range(16):
            single.add(jpeg.pack([J.raw(J.cases()[sizes[(3 * k + first) % 54]])]))
    _same_frames(frames, single.decode(sel), len(sel))


def test_refusals_launch_nothing(dealt):
    from coclr_amd import _lib, jpeg, ops
    shards, single, where = dealt(3, 64)
    sh = jpeg.ShardedStore(shards)
    sel = [where[i] for i in _picks()[:12]]
    plan, slot, records, nbytes, nrows, shard = sh.gather_plan(torch.as_tensor(sel))
    assert len(set(shard.tolist())) == 3
    arena = torch.full((nbytes + 64,), FILL, dtype=torch.uint8, device="cuda")
    arena_rows = torch.full((nrows + 4, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    d_plan, d_shard = plan.cuda(), shard.cuda()

    def refused(sources=None, p=plan, sc=shard, size=nbytes):
        with pytest.raises(_lib.HipLibraryError):
            ops.jpeg_store_gather_shards(sources or sh._sources, d_plan, p, d_shard, sc, slot, records, arena[:size],
                                         arena_rows[:nrows])
        torch.cuda.synchronize()                                                       # and no error was left behind
        assert bool((arena == FILL).all()) and bool((arena_rows == 0x5a5a5a5a).all())

    def with_source(k, **edit):
        names = ("data", "rows", "frames_host", "nframes", "tables_host", "table_sets", "segs_host", "nsegs",
                 "chunk_bytes")
        src = dict(zip(names, sh._sources[k]))
        src.update(edit)
        return sh._sources[:k] + [tuple(src[n] for n in names)] + sh._sources[k + 1:]

    for k in range(3):                                                                 # the same bytes, not pinned
        plain = shards[k]._data.cpu().clone()
        assert not plain.is_pinned() and not plain.is_cuda
        refused(sources=with_source(k, data=plain))
        plain_rows = shards[k]._rows.cpu().clone()
        assert not plain_rows.is_pinned()
        refused(sources=with_source(k, rows=plain_rows))
    refused(sources=with_source(2, chunk_bytes=8))                                     # shards that differ in chunk_bytes
    refused(size=nbytes - 1)                                                           # an arena one byte too small
    outside = shard.clone()
    outside[-1] = 3                                                                    # a shard of nshards
    refused(sc=outside)
    refused(sc=torch.cat([shard[-1:], shard[:-1]]))                                    # not ordered by (shard, frame)
    beyond = plan.clone()
    beyond[0, 0] = len(shards[0])                                                      # a frame of nframes
    refused(p=beyond)
    with pytest.raises(ValueError):
        ops.jpeg_store_gather_shards(sh._sources * 3, d_plan, plan, d_shard, shard, slot, records, arena[:nbytes],
                                     arena_rows[:nrows])                               # nine sources
    # the same call, unedited, goes through
    ops.jpeg_store_gather_shards(sh._sources, d_plan, plan, d_shard, shard, slot, records, arena[:nbytes],
                                 arena_rows[:nrows])
    got = (plan, shard, records, nbytes, nrows, arena.cpu(), arena_rows.cpu())
    _check_arena(sh, shards, sel, got)


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


def test_training_staging_from_a_sharded_store(dealt):
    from coclr_amd import jpeg, staging
    shards, single, _ = dealt(2, 64)
    sh = jpeg.ShardedStore(shards)
    ids, plans = _batch(sh)
    assert len(set(sh.shard_of(ids.view(-1)).tolist())) == 2
    want = staging.stage_train_clips_ragged(single.decode(ids.view(-1)), plans, 16)
    got = staging.stage_train_clips_ragged(sh.decode(ids.view(-1)), plans, 16)
    assert got.shape == (2, 2, 3, 2, 16, 16) and torch.equal(got, want)
    sel, boxes = staging.clip_frames(ids, plans, 2)
    cropped = staging.stage_train_clips_cropped(sh.decode(sel, boxes), plans, 16)
    assert torch.equal(cropped, staging.stage_train_clips_cropped(single.decode(sel, boxes), plans, 16))
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


def test_evaluator_from_a_sharded_store():
    """VideoEvaluator.add_stored: two videos (the fixtures of one frame size each), one per shard."""
    from coclr_amd import jpeg
    from coclr_amd.eval.video import VideoEvaluator
    model = _TableModel().cuda().eval()
    results = []
    for sharded in (True, False):
        stores = [jpeg.Store(CAPACITY, 64) for _ in range(2 if sharded else 1)]
        videos, base = [], 0
        for label, (H, W) in enumerate(((37, 45), (40, 56))):
            store = stores[label if sharded else 0]
            cases = [c for c in J.cases() if (c["height"], c["width"]) == (H, W)]
            ids = [store.add(jpeg.pack([J.raw(c)])) for c in cases]
            assert len(cases) >= 13
            videos.append((base + ids[0] if sharded else ids[0], len(cases),
                           [[[3, 5], [5, 9]], [[12, 0], [0, 1]]][label], label))
            base += len(cases)
        source = jpeg.ShardedStore(stores) if sharded else stores[0]
        ev = VideoEvaluator(model, batch_clips=8)
        assert ev.add_stored(source, videos, crops="center", crop_size=16, out_size=16) == [0, 1]
        results.append(ev.finish())
    got, want = results
    assert torch.equal(got.probs, want.probs) and torch.equal(got.features, want.features)
    assert torch.equal(got.labels, want.labels) and torch.equal(got.top1, want.top1)
