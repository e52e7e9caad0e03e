"""Every row of tests/_stage_cases.py (all fourteen instantiations of coclr_amd/csrc/staging.hip, every band height of
both band schemes, every LDS and alignment edge: tests/test_stage_plan_cpu.py says which row reaches what) on one
MI355X through the C ABI wrappers of coclr_amd/ops.py, against the CPU restatements (tests/crops_harness.py,
cls_harness.py, train_harness.py, jitter_harness.py; oracle.coclr_oracle.tr for coclr_stage_clips) with ZERO tolerance:
the resampling and the programs are integer arithmetic, and the float step is two correctly rounded divisions and a
subtraction, so every comparison is torch.equal.

Per row: the plan query, asked with the very tensors of the launch, reports the path the row is there for; the output
lies inside a larger buffer of a sentinel (0x5a bytes / 7.0) and nothing before or behind its range is touched; a second
launch over a different fill gives the same, so the launch writes every element of its range.  A refusal row raises
and writes nothing.  No test imports PIL (tests/test_stage_plan_cpu.py holds the restatements against it)."""
import numpy as np
import pytest
import torch

import _stage_cases as SC
import crops_harness as CH
import jitter_harness as JH
from oracle import coclr_oracle as orc

pytestmark = pytest.mark.gpu

GUARD = 64           # elements of sentinel on either side; keeps a 16-byte aligned range aligned
MEAN, STD = CH.IMAGENET_MEAN, CH.IMAGENET_STD


def _ids(rows):
    return [r.name for r in rows]


def _guarded(shape, dtype, off, fill):
    """A contiguous tensor of `shape` `off` elements behind a 16-byte boundary, inside a buffer of `fill`."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + off,), fill, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + off:GUARD + off + n].view(shape)


def _guards_intact(buf, out, fill):
    n, lo = out.numel(), out.storage_offset()
    return bool((buf[:lo] == fill).all()) and bool((buf[lo + n:] == fill).all())


def _run(row, shape, dtype, off, launch, want, plan_kw=None):
    """launch(out) twice over two fills, guards, equality with `want` (None: the launcher must refuse)."""
    from coclr_amd import _lib
    fills = (7.0, -3.0) if dtype == torch.float32 else (0x5a, 0xa5)
    got = []
    for fill in fills:
        buf, out = _guarded(shape, dtype, off, fill)
        if getattr(row, "refuse", False):
            with pytest.raises(_lib.HipLibraryError):
                SC.plan(row, out_addr=out.data_ptr(), **(plan_kw(out) if plan_kw else {}))
            with pytest.raises(_lib.HipLibraryError):
                launch(out)
            torch.cuda.synchronize()
            assert bool((buf == fill).all()), row.name
            return
        pl = SC.plan(row, out_addr=out.data_ptr(), **(plan_kw(out) if plan_kw else {}))
        for k, v in row.want.items():
            assert pl[k] == v, (row.name, k, pl)
        launch(out)
        torch.cuda.synchronize()
        assert _guards_intact(buf, out, fill), row.name
        got.append(out.cpu())
    assert torch.equal(got[0], want), row.name
    assert torch.equal(got[1], got[0]), row.name


def _normalised(u8):
    """uint8 (..., T, S, S, 3) -> fp32 (..., 3, T, S, S)."""
    x = CH.normalise(u8, MEAN, STD)
    return x.movedim(-1, -4).contiguous()


@pytest.mark.parametrize("row", SC.CROPS, ids=_ids(SC.CROPS))
def test_crop_form(row):
    from coclr_amd import ops
    src = SC.sources(row)
    u8, rag = row.form.endswith("u8"), row.form.startswith("rag")
    n_clips, T, S = len(row.slots), len(row.slots[0]), row.S
    xmin, xk = [t.cuda() for t in CH.kernel_layout(row.cw, S)]
    ymin, yk = [t.cuda() for t in CH.kernel_layout(row.ch, S)]
    want = None
    if not row.refuse:
        ref = torch.from_numpy(SC.resize_reference(row, src))          # (n_crops,) n_clips, T, S, S, 3
        want = ref.reshape((-1, S, S, 3) if rag else (len(row.crops), -1, S, S, 3)) if u8 else _normalised(ref.numpy())
    if rag:
        pixels = torch.from_numpy(SC.flat_buffer(row, src)).cuda()
        desc, slot_off, _ = SC.crop_descriptors(row)
        ddev, sdev = desc.cuda(), slot_off.cuda()
        shape = (n_clips * T, S, S, 3) if u8 else (n_clips, 3, T, S, S)

        def launch(out):
            ops.stage_crops_ragged(pixels, ddev, desc, sdev, slot_off, row.cw, row.ch, S, xmin, xk, ymin, yk, out,
                                   None if u8 else MEAN, None if u8 else STD)
    else:
        frames = torch.from_numpy(np.concatenate(src)).cuda()
        slot_frame = torch.tensor(row.slots, dtype=torch.int32, device="cuda")
        shape = (len(row.crops), n_clips * T, S, S, 3) if u8 else (len(row.crops), n_clips, 3, T, S, S)

        def launch(out):
            if u8:
                ops.resize_crops_u8(frames, slot_frame, list(row.crops), row.cw, row.ch, S, xmin, xk, ymin, yk, out)
            else:
                ops.stage_crops(frames, slot_frame, list(row.crops), row.cw, row.ch, S, xmin, xk, ymin, yk, MEAN, STD,
                                out)
    _run(row, shape, torch.uint8 if u8 else torch.float32, row.out_off, launch, want)


@pytest.mark.parametrize("row", SC.BOXES, ids=_ids(SC.BOXES))
def test_box_form(row):
    from coclr_amd import ops
    src = SC.sources(row)
    desc, xtab, ytab = SC.box_descriptors(row)
    ddev, xdev, ydev = desc.cuda(), xtab.cuda(), ytab.cuda()
    n, S = len(row.clips) * row.T, row.S
    want = None if row.refuse else torch.from_numpy(SC.resize_reference(row, src)).reshape(n, S, S, 3)
    if row.ragged:
        pixels = torch.from_numpy(SC.flat_buffer(row, src)).cuda()

        def launch(out):
            ops.resize_boxes_ragged_u8(pixels, ddev, desc, xdev, ydev, row.T, S, out)
    else:
        frames = torch.from_numpy(np.concatenate(src)).cuda()

        def launch(out):
            ops.resize_boxes_u8(frames, ddev, desc, xdev, ydev, row.T, S, out)
    _run(row, (n, S, S, 3), torch.uint8, 0, launch, want)


@pytest.mark.parametrize("row", SC.TWOS, ids=_ids(SC.TWOS))
def test_two_stage_form(row):
    from coclr_amd import ops
    src = SC.sources(row)
    desc, xtab, ytab, tab2 = SC.two_descriptors(row)
    ddev, xdev, ydev, t2dev = desc.cuda(), xtab.cuda(), ytab.cuda(), tab2.cuda()
    u8, rag = row.form.endswith("u8"), row.form.startswith("rag")
    n_clips, T, S = len(row.clips), row.T, row.S
    want = None
    if not row.refuse:
        ref = SC.resize_reference(row, src)                              # n_clips, T, S, S, 3
        want = torch.from_numpy(ref).reshape(-1, S, S, 3) if u8 else _normalised(ref)
    source = torch.from_numpy(SC.flat_buffer(row, src) if rag else np.concatenate(src)).cuda()
    fn = ops.resize2_boxes_ragged if rag else ops.resize2_boxes

    def launch(out):
        fn(source, ddev, desc, xdev, ydev, t2dev, T, row.size, S, out, None if u8 else MEAN, None if u8 else STD)
    shape = (n_clips * T, S, S, 3) if u8 else (n_clips, 3, T, S, S)
    _run(row, shape, torch.uint8 if u8 else torch.float32, 0, launch, want)


def _tr(frames, S, thw, mean, std):
    """oracle.coclr_oracle.tr (three channels) for C in 1..4: a window of three channels at a time."""
    Cc = frames.shape[1]
    if Cc == 3:
        return orc.tr(frames, S, thw, mean, std)
    if Cc < 3:
        pad = torch.cat([frames] + [frames[:, :1]] * (3 - Cc), 1)
        return orc.tr(pad, S, thw, tuple(mean) + (mean[0],) * (3 - Cc), tuple(std) + (std[0],) * (3 - Cc))[:, :, :Cc]
    lo = orc.tr(frames[:, :3], S, thw, mean[:3], std[:3])
    hi = orc.tr(frames[:, Cc - 3:], S, thw, mean[Cc - 3:], std[Cc - 3:])
    return torch.cat([lo, hi[:, :, 3 - (Cc - 3):]], 2).contiguous()


@pytest.mark.parametrize("row", SC.CLIPS, ids=_ids(SC.CLIPS))
def test_stage_clips(row):
    from coclr_amd import ops
    gen = torch.Generator().manual_seed(sum(map(ord, row.name)))
    shape = (row.B, row.C, row.S * row.thw, 1, 1)
    u8 = torch.randint(0, 256, shape, generator=gen, dtype=torch.uint8)
    u8.view(-1)[::7] = 255
    u8.view(-1)[3::11] = 0
    host = u8 if row.u8 else u8.float() / 255
    _, frames = _guarded(shape, host.dtype, row.src_off, 0)
    frames.copy_(host)
    mean, std = (0.485, 0.456, 0.406, 0.5)[:row.C], (0.229, 0.224, 0.225, 0.25)[:row.C]
    want = None if row.refuse else _tr(host, row.S, row.thw, mean, std)

    def launch(out):
        ops.stage_clips(frames, out, row.S, mean, std)
    _run(row, (row.B, row.S, row.C, row.thw, 1, 1), torch.float32, row.out_off, launch, want,
         plan_kw=lambda out: dict(src_addr=frames.data_ptr()))


@pytest.mark.parametrize("row", SC.PROGS, ids=_ids(SC.PROGS))
def test_program_form(row):
    from coclr_amd import ops
    frames_np = SC.program_frames(row)
    frames = torch.from_numpy(frames_np).cuda()
    kinds, params = SC.program_tables(row)
    kdev, pdev = kinds.cuda(), params.cuda()
    want = JH.to_clips(SC.program_reference_u8(row, frames_np), row.T, MEAN, STD)
    fn = ops.augment_clips if row.aug else ops.color_jitter_clips

    def launch(out):
        fn(frames, kdev, pdev, row.group_size, row.T, MEAN, STD, out, host_tables=(kinds, params))
    _run(row, (row.N // row.T, 3, row.T, row.H, row.W), torch.float32, 0, launch, want)

