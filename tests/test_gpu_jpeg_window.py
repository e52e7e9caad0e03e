"""Decoding only a pixel box of every frame from the device-resident JPEG store, on one MI355X (coclr_amd/jpeg.py:
Store.decode(ids, boxes); csrc/jpeg.hip: coclr_jpeg_decode_store_window; coclr_amd/staging.py: clip_frames,
stage_train_clips_cropped).  Every comparison is torch.equal, ZERO tolerance: a box equals the same region cut from the
full decode, which is held to PIL's own bytes here as in tests/test_gpu_jpeg_store.py.  Only clean files are sent to the
GPU (damage belongs to the host programs)."""
import random

import numpy as np
import pytest
import torch

import _jpeg_cases as J
import _jpeg_window_cases as WC

pytestmark = pytest.mark.gpu

FILL = 0x5a
CHUNKS = (8, None, 65536)


@pytest.fixture(scope="module")
def stores():
    """Per chunk size a store of all 54 fixtures in fixture order (id = fixture index) and its full decode on the host,
    computed once and left unchanged."""
    from coclr_amd import jpeg
    cases = J.cases()
    out = {}
    for chunk_bytes in CHUNKS:
        store = jpeg.Store(1 << 20, 64, chunk_bytes=chunk_bytes)
        assert [store.add(jpeg.pack([J.raw(c)])) for c in cases] == list(range(len(cases)))
        frames, status = store.decode(list(range(len(cases))), return_status=True)
        assert not bool(status.any())
        full = [frames.frame(i).cpu() for i in range(len(cases))]
        for c, f in zip(cases, full):
            assert torch.equal(f, c["rgb"]), c["name"]                                 # PIL's bytes
        out[chunk_bytes] = (store, full)
    return out


def _ids_boxes():
    picks = WC.all_boxes()
    return [i for i, _ in picks], torch.tensor([b for _, b in picks], dtype=torch.int64)


def _check(frames, status, full, ids, boxes):
    assert len(frames) == len(ids) and status.shape == (len(ids),) and status.dtype == torch.int32
    assert not bool(status.any())
    assert bool((frames.offset % 16 == 0).all())
    pixels = frames.pixels.cpu()
    for k, (i, (x0, y0, w, h)) in enumerate(zip(ids, boxes.tolist())):
        assert frames.height[k] == h and frames.width[k] == w
        o = int(frames.offset[k])
        got = pixels[o:o + 3 * h * w].view(h, w, 3)
        assert torch.equal(got, full[i][y0:y0 + h, x0:x0 + w]), (J.cases()[i]["name"], x0, y0, w, h)


@pytest.mark.parametrize("chunk_bytes", CHUNKS)
def test_every_fixture_against_the_box_list(stores, chunk_bytes):
    """All 54 fixtures x the fixed box list (tests/_jpeg_window_cases.py: boxes) in ONE call with repeated ids."""
    store, full = stores[chunk_bytes]
    ids, boxes = _ids_boxes()
    cases = J.cases()
    assert len(cases) == 54 and len(ids) > 40 * 54 and set(ids) == set(range(54))
    seen = {(cases[i]["ncomp"], tuple(cases[i]["sampling"])) for i in ids}
    assert seen == {(1, (1, 1)), (3, (1, 1)), (3, (2, 1)), (3, (2, 2))}
    big = [b for i, b in zip(ids, boxes.tolist()) if cases[i]["name"] == "320x240_420_q75"]
    assert {b[2] for b in big} >= {16, 32, 15, 17, 320, 1}                             # the 16-byte store path and off it
    frames, status = store.decode(ids, boxes, return_status=True)
    assert store.decode.last_status is status
    _check(frames, status, full, ids, boxes)
    again = store.decode(torch.tensor(ids), boxes.tolist())                            # sequences will do
    assert torch.equal(again.offset, frames.offset)
    _check(again, store.decode.last_status, full, ids, boxes)                          # (the padding is not compared)


def test_without_boxes_the_call_is_todays(stores, monkeypatch):
    from coclr_amd import jpeg, ops
    store, full = stores[None]
    ids = [5, 53, 53, 0, 20, 41]
    cases = J.cases()
    want = jpeg.decode_ragged(*jpeg.cat_ragged([jpeg.pack([J.raw(cases[i])]) for i in ids]))
    assert len(store.plan(ids)) == 6 and len(store.plan(ids, boxes=None)) == 6
    monkeypatch.setattr(ops, "jpeg_decode_store_window", None)                         # not the new entry point
    a = store.decode(ids)
    b, status = store.decode(ids, boxes=None, return_status=True)
    for got in (a, b):
        assert torch.equal(got.offset, want.offset) and torch.equal(got.height, want.height)
        assert torch.equal(got.width, want.width) and got.pixels.numel() == want.pixels.numel()
        assert all(torch.equal(got.frame(k), want.frame(k)) for k in range(len(ids)))  # (the padding is not compared)
    assert not bool(status.any())


@pytest.mark.parametrize("chunk_bytes", CHUNKS)
def test_padding_between_frames_is_untouched(stores, chunk_bytes):
    """One coclr_jpeg_decode_store_window call by hand into an output filled with 0x5a, 64 more bytes behind it."""
    from coclr_amd import ops, staging
    store, full = stores[chunk_bytes]
    ids, boxes = _ids_boxes()
    sel, geo, offset, total, stages, blocks, window = store.plan(ids, boxes=boxes)
    (_, _, geom, prefix), = stages
    pixels = torch.full((((total + 15) & ~15) + 64,), FILL, dtype=torch.uint8, device="cuda")
    coefs = torch.empty(blocks * 64, dtype=torch.int16, device="cuda")
    planes = torch.empty(blocks * 64, dtype=torch.uint8, device="cuda")
    status = torch.empty(len(ids), dtype=torch.int32, device="cuda")
    ops.jpeg_decode_store_window(store._buffers(), sel.cuda(), sel, geom.cuda(), geom, window.cuda(), window,
                                 prefix.cuda(), prefix, coefs, planes, pixels, status)
    frames = staging.RaggedFrames(pixels, offset, window[:, 3].to(torch.int32), window[:, 2].to(torch.int32))
    _check(frames, status, full, ids, boxes)
    keep = torch.ones(pixels.numel(), dtype=torch.bool)
    for o, (_, _, w, h) in zip(offset.tolist(), boxes.tolist()):
        keep[o:o + 3 * h * w] = False
    rest = pixels.cpu()[keep]
    assert rest.numel() >= 64 and bool((rest == FILL).all())


def test_stage_budget(stores):
    store, full = stores[None]
    ids, boxes = _ids_boxes()
    ids, boxes = ids[-400:], boxes[-400:]                                              # the larger fixtures
    for budget, least in ((400000, 3), (1, len(ids))):
        assert len(store.plan(ids, budget, boxes)[4]) >= least
        frames, status = store.decode(ids, boxes, return_status=True, max_stage_bytes=budget)
        _check(frames, status, full, ids, boxes)


def _entropy_only(store, ids, boxes):
    """The coefficients after stage 1 alone of the window entry point and of the existing one -> two int16
    (blocks, 64) host tensors in the full-frame layout."""
    from coclr_amd import ops
    sel, geo, offset, total, stages, blocks, window = store.plan(ids, boxes=boxes)
    (_, _, geom, prefix), = stages
    _, _, _, f_total, f_stages, _ = store.plan(ids)
    (_, _, f_geom, f_prefix), = f_stages
    out = []
    for win in (True, False):
        coefs = torch.full((blocks * 64,), 0x1234, dtype=torch.int16, device="cuda")
        planes = torch.empty(blocks * 64, dtype=torch.uint8, device="cuda")
        status = torch.empty(len(ids), dtype=torch.int32, device="cuda")
        if win:
            pixels = torch.empty((total + 15) & ~15, dtype=torch.uint8, device="cuda")
            ops.jpeg_decode_store_window(store._buffers(), sel.cuda(), sel, geom.cuda(), geom, window.cuda(), window,
                                         prefix.cuda(), prefix, coefs, planes, pixels, status, stages=1)
        else:
            pixels = torch.empty((f_total + 15) & ~15, dtype=torch.uint8, device="cuda")
            ops.jpeg_decode_store(store._buffers(), sel.cuda(), sel, f_geom.cuda(), f_geom, f_prefix.cuda(), f_prefix,
                                  coefs, planes, pixels, status, stages=1)
        assert not bool(status.any())
        out.append(coefs.cpu().view(blocks, 64))
    return out


@pytest.mark.parametrize("name,box,before", [
    ("320x240_420_q75", (100, 100, 60, 40), False),
    ("320x240_420_q75", (40, 200, 200, 40), True),                                     # in the bottom rows
    ("56x40_420_q100_noise", (20, 18, 10, 4), False),                                  # inside one MCU row
])
def test_skipping_is_real(stores, name, box, before):
    store, _ = stores[None]
    from coclr_amd import jpeg
    i = J.names().index(name)
    c = J.cases()[i]
    assert len(jpeg.parse(J.raw(c))["segments"]) == 1                                  # decoded by chunk
    H, W, ncomp, (hs, vs) = c["height"], c["width"], c["ncomp"], c["sampling"]
    mx0, my0, mx1, my1 = WC.mcu_rect(H, W, ncomp, hs, vs, box)
    mcux, mb = -(-W // (8 * hs)), WC.mcu_blocks(ncomp, hs, vs)
    first, last = my0 * mcux + mx0, (my1 - 1) * mcux + mx1
    if name.startswith("56x40"):
        assert my1 - my0 == 1
    got, want = _entropy_only(store, [i], torch.tensor([box]))
    mcu = torch.tensor(WC.block_mcus(H, W, ncomp, hs, vs))
    assert mcu.numel() == got.shape[0] == want.shape[0]
    inside = (mcu % mcux >= mx0) & (mcu % mcux < mx1) & (mcu // mcux >= my0) & (mcu // mcux < my1)
    assert int(inside.sum()) == (mx1 - mx0) * (my1 - my0) * mb
    assert torch.equal(got[inside], want[inside])
    assert bool(want[mcu >= last].any()) and not bool(got[mcu >= last].any())          # the full decode has them
    if before:
        # rows of the frame: blocks completed before every chunk; the first chunk that is not wholly before `first`
        rec = store._host[0][i].tolist()
        n = max(1, -(-rec[1] // store.chunk_bytes))
        rows = store._rows[rec[6]:rec[6] + n].cpu()
        counts = [int(r[1]) if int(r[0]) >= 0 else None for r in rows]                 # None: a past row
        total = mcux * -(-H // (8 * vs)) * mb
        nxt = [total if k + 1 == n or counts[k + 1] is None else counts[k + 1] for k in range(n)]
        k0 = next(k for k in range(n) if nxt[k] >= first * mb)
        clean = counts[k0] // mb                                                       # MCUs below lie in skipped chunks
        assert 0 < clean <= first
        assert bool(want[mcu < clean].any()) and not bool(got[mcu < clean].any())


def test_through_staging():
    """B = 6 seeded plans at T = 2, S = 16 over two fixture groups, with repeated ids: the cropped route equals the
    full-frame route bit for bit."""
    from coclr_amd import jpeg, staging
    T, S, B = 2, 16, 6
    groups = J.groups()
    packs = [groups[(40, 56, 3, (2, 2))], groups[(37, 45, 3, (2, 1))]]
    store = jpeg.Store(1 << 20, 64)
    first = [store.add(jpeg.pack([J.raw(c) for c in g])) for g in packs]
    tt = staging.TrainTransform(S, T)
    rng, np_rng, pick = random.Random(0), np.random.RandomState(0), random.Random(1)
    ids, plans, sizes = [], [], []
    for b in range(B):
        g = b % 2
        ids.append([first[g] + pick.randrange(len(packs[g])) for _ in range(2 * T)])
        sizes.append(store.frame_size(ids[-1][0]))
        assert all(store.frame_size(i) == sizes[-1] for i in ids[-1])
        plans.append(tt.draw(*sizes[-1], rng=rng, np_rng=np_rng))
    ids = torch.tensor(ids)
    assert any(len(set(row)) < 2 * T for row in ids.tolist())                          # repeated ids
    halves = {p["half"] for p in plans}
    assert halves == {(0, 1), (0, 0), (1, 1)}                                          # TwoClip and both OneClip halves
    assert any(p["box"][c] == (0, 0) + sizes[b] for b, p in enumerate(plans) for c in range(2))    # a box that did not fit
    assert any(p["box"][c] != (0, 0) + sizes[b] for b, p in enumerate(plans) for c in range(2))
    gray = [progs for p in plans for progs in p["programs"]
            if any(op[0] == staging.JITTER_GRAY for prog in progs for op in prog)]
    assert any(progs[0] != progs[1] for progs in gray)                                 # per-frame programs
    sel, boxes = staging.clip_frames(ids, plans, T)
    assert sel.shape == (2 * B * T,) and boxes.shape == (2 * B * T, 4)
    cropped = store.decode(sel, boxes)
    assert not bool(store.decode.last_status.any())
    got = staging.stage_train_clips_cropped(cropped, plans, S)
    want = staging.stage_train_clips_ragged(store.decode(ids.view(-1)), plans, S)
    assert got.shape == (B, 2, 3, T, S, S) and got.dtype == torch.float32
    assert torch.equal(got, want)
    packed = torch.stack([staging.pack_plan(p, T) for p in plans])                     # the packed tensor will do
    sel2, boxes2 = staging.clip_frames(ids, packed, T)
    assert torch.equal(sel2, sel) and torch.equal(boxes2, boxes)
    assert torch.equal(staging.stage_train_clips_cropped(cropped, packed, S), want)
