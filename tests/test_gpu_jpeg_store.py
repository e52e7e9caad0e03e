"""The device-resident JPEG store on one MI355X (coclr_amd/jpeg.py: class Store; csrc/jpeg.hip: coclr_jpeg_store_index,
coclr_jpeg_decode_store): every fixture of tests/golden/jpeg_frames.pt added as its own pack in a shuffled order and
decoded by index -- permuted, with repeats -- against PIL's own bytes and against decode_ragged on the same frames,
with ZERO tolerance: every comparison is torch.equal.  At three chunk sizes, cut into several stages, with the bytes
behind 2^31, and through stage_train_clips_ragged.  No damaged stream and no damaged row is sent to the GPU (those
belong to the host program: tests/test_jpeg_store_cpu.py)."""
import os
import random

import numpy as np
import pytest
import torch

import _jpeg_cases as J

pytestmark = pytest.mark.gpu

FILL = 0x5a
CHUNKS = (None, 8, 65536)


def _picks():
    """A seeded permutation of all 54 fixtures, then some of them again."""
    order = random.Random(11).sample(range(54), 54)
    return order + [order[5], order[5], 0, order[40], 53, 0]


@pytest.fixture(scope="module")
def stores():
    """Per chunk size a store of all 54 fixtures, each its own pack, in a shuffled order -> (store, fixture -> id)."""
    from coclr_amd import jpeg
    cases = J.cases()
    assert len(cases) == 54
    out = {}
    for chunk_bytes in CHUNKS:
        store = jpeg.Store(1 << 20, 64, chunk_bytes=chunk_bytes)
        order = random.Random(3).sample(range(54), 54)
        assert order != sorted(order)
        where = {i: store.add(jpeg.pack([J.raw(cases[i])])) for i in order}
        assert [where[i] for i in order] == list(range(54)) and len(store) == 54
        out[chunk_bytes] = (store, where)
    return out


@pytest.fixture(scope="module")
def ragged():
    """decode_ragged on the frames of _picks() in that order: the reference route, computed once."""
    from coclr_amd import jpeg
    cases = J.cases()
    data, meta = jpeg.cat_ragged([jpeg.pack([J.raw(cases[i])]) for i in _picks()])
    frames, status = jpeg.decode_ragged(data, meta, return_status=True)
    return frames, status


def _check(frames, status, ragged, picks):
    cases = J.cases()
    want, want_status = ragged
    assert len(frames) == len(picks) and status.shape == (len(picks),) and status.dtype == torch.int32
    assert not bool(status.any()) and torch.equal(status, want_status)
    assert torch.equal(frames.offset, want.offset)
    for k, i in enumerate(picks):
        c = cases[i]
        assert frames.height[k] == c["height"] and frames.width[k] == c["width"]
        assert torch.equal(frames.frame(k).cpu(), c["rgb"]), c["name"]                 # PIL's bytes
        assert torch.equal(frames.frame(k), want.frame(k)), c["name"]                  # decode_ragged's


@pytest.mark.parametrize("chunk_bytes", CHUNKS)
def test_whole_fixture_by_index(stores, ragged, chunk_bytes):
    from coclr_amd import jpeg
    store, where = stores[chunk_bytes]
    cases, picks = J.cases(), _picks()
    assert store.chunk_bytes == (chunk_bytes or jpeg.DEFAULT_STORE_CHUNK)
    geos = {(c["height"], c["width"], c["ncomp"], tuple(c["sampling"])) for c in cases}
    assert len(geos) == 21 and len({(g[0], g[1]) for g in geos}) == 6                  # sizes, gray, samplings
    kinds = {len(jpeg.parse(J.raw(c))["segments"]) > 1 for c in cases}
    assert kinds == {True, False}                                                      # restart markers and none
    single = [c for c in cases if len(jpeg.parse(J.raw(c))["segments"]) == 1]
    if chunk_bytes == 65536:
        assert store.chunk_rows == len(single)                                         # every frame is one chunk
    elif chunk_bytes == 8:
        assert store.chunk_rows > 1024 * 2                                             # several windows of the indexer
    ids = torch.tensor([where[i] for i in picks])
    frames, status = store.decode(ids, return_status=True)
    assert store.decode.last_status is status
    _check(frames, status, ragged, picks)
    again = store.decode(ids.tolist())                                                 # a sequence will do
    assert all(torch.equal(again.frame(k), frames.frame(k)) for k in range(len(picks)))
    # the bytes are the same at every chunk size
    first = stores[CHUNKS[0]]
    if chunk_bytes != CHUNKS[0]:
        other = first[0].decode([first[1][i] for i in picks])
        assert all(torch.equal(other.frame(k), frames.frame(k)) for k in range(len(picks)))


@pytest.mark.parametrize("chunk_bytes", CHUNKS)
def test_padding_between_frames_is_untouched(stores, ragged, chunk_bytes):
    """One coclr_jpeg_decode_store call by hand into an output filled with 0x5a, 64 more bytes behind it."""
    from coclr_amd import ops, staging
    store, where = stores[chunk_bytes]
    picks = _picks()
    sel, geo, offset, total, stages, blocks = store.plan([where[i] for i in picks])
    (_, _, geom, prefix), = stages
    pixels = torch.full((((total + 15) & ~15) + 64,), FILL, dtype=torch.uint8, device="cuda")
    coefs = torch.empty(blocks * 64, dtype=torch.int16, device="cuda")
    planes = torch.empty(blocks * 64, dtype=torch.uint8, device="cuda")
    status = torch.empty(len(picks), dtype=torch.int32, device="cuda")
    ops.jpeg_decode_store(store._buffers(), sel.cuda(), sel, geom.cuda(), geom, prefix.cuda(), prefix, coefs, planes,
                          pixels, status)
    frames = staging.RaggedFrames(pixels, offset, geo[:, 0].to(torch.int32), geo[:, 1].to(torch.int32))
    _check(frames, status, ragged, picks)
    keep = torch.ones(pixels.numel(), dtype=torch.bool)
    for o, H, W in zip(offset.tolist(), geo[:, 0].tolist(), geo[:, 1].tolist()):
        keep[o:o + 3 * H * W] = False
    rest = pixels.cpu()[keep]
    assert rest.numel() >= 64 and bool((rest == FILL).all())


@pytest.mark.parametrize("chunk_bytes", CHUNKS)
def test_stage_budget(stores, ragged, chunk_bytes):
    store, where = stores[chunk_bytes]
    picks = _picks()
    ids = [where[i] for i in picks]
    for budget, least in ((40000, 3), (1, len(picks))):
        assert len(store.plan(ids, budget)[4]) >= least
        frames, status = store.decode(ids, return_status=True, max_stage_bytes=budget)
        _check(frames, status, ragged, picks)


def test_rows_are_the_recorded_rows():
    """tests/golden/jpeg_store_rows.json (tools/make_jpeg_store_rows_golden.py): what coclr_jpeg_store_index stored for
    the 54 fixtures added in index order, at chunk sizes 8 and 64, as a count and a digest of the rows' bytes."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location(
        "make_jpeg_store_rows_golden", os.path.join(J.ROOT, "tools", "make_jpeg_store_rows_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(tool.OUT) as f:
        want = json.load(f)
    assert sorted(want) == ["64", "8"]
    assert want["8"]["chunk_rows"] > 1024 * 2                                          # several windows of the indexer
    assert tool.digests() == want


def test_bytes_behind_two_gib():
    """64-bit addressing: the write cursor is moved past 2^31 before the first add (Store._advance_cursor, for this
    test only); the allocation is untouched memory."""
    from coclr_amd import jpeg
    names = ("320x240_420_q75", "56x40_420_rst1", "45x37_422_q100_noise")
    cases = [J.case(n) for n in names]
    store = jpeg.Store((1 << 31) + (1 << 20), 8)
    store._advance_cursor((1 << 31) + 5)
    ids = [store.add(jpeg.pack([J.raw(c)])) for c in cases]
    assert ids == [0, 1, 2] and store.nbytes > (1 << 31) + 5
    assert all(int(b) > 1 << 31 for b in store._host[0][:3, 0])
    assert {int(n) > 1 for n in store._host[0][:3, 3]} == {True, False}
    frames, status = store.decode([2, 0, 1, 0], return_status=True)
    assert not bool(status.any())
    for k, i in enumerate((2, 0, 1, 0)):
        assert torch.equal(frames.frame(k).cpu(), cases[i]["rgb"]), names[i]


def test_kinetics_sizes_through_training_staging():
    """tests/golden/jpeg_ragged.pt: four frames at kinetics400-256's sizes; T = 1, a sample is its frame twice -- by
    index from the store, and as cat_ragged / decode_ragged of the same bytes; both staged with the same plans."""
    from coclr_amd import jpeg, staging
    cases = torch.load(os.path.join(J.ROOT, "tests", "golden", "jpeg_ragged.pt"))["cases"]
    assert [(c["width"], c["height"]) for c in cases] == [(340, 256), (454, 256), (256, 340), (320, 256)]
    S = 32
    tt = staging.TrainTransform(S, 1)
    rng, np_rng = random.Random(5), np.random.RandomState(5)
    store = jpeg.Store(1 << 20, 8)
    first = [store.add(jpeg.pack([J.raw(c)])) for c in cases]
    plans = [tt.draw(*store.frame_size(f), rng=rng, np_rng=np_rng) for f in first]
    ids = torch.tensor([[f, f] for f in first])
    frames = store.decode(ids.view(-1))
    assert not bool(store.decode.last_status.any())
    want = jpeg.decode_ragged(*jpeg.cat_ragged([jpeg.pack([J.raw(c)] * 2) for c in cases]))
    assert torch.equal(frames.offset, want.offset) and torch.equal(frames.height, want.height)
    got = staging.stage_train_clips_ragged(frames, plans, S)
    assert got.shape == (4, 2, 3, 1, S, S)
    assert torch.equal(got, staging.stage_train_clips_ragged(want, plans, S))
