"""Staging test rows: small named geometries that reach every instantiation, band height and dispatch edge of the
launchers of coclr_amd/csrc/staging.hip -- the edges are listed in tests/test_stage_plan_cpu.py.

Shared by the CPU-tier coverage test (tests/test_stage_plan_cpu.py: the launchers' own plan queries say what each row
reaches, and the restatements used as references are held against PIL on the rows' inputs) and the GPU test
(tests/test_gpu_stage_exact.py: every row against the restatement, bit for bit).  The table itself is plain data; the
builders below import numpy / torch and the harnesses when called.

The two axes of a resize are independent, so a row that is about the row axis (band height, LDS) says nothing new about
the column axis.  Its boxes are exactly S wide: PIL then runs the vertical pass alone, so the comparison with PIL does
not depend on the order of the passes -- the reference's Pillow 6.1 and the kernels resample horizontally first, while
Pillow 12 resamples tall thin boxes (450 x 4 -> 37 x 37) vertically first, which rounds the intermediate bytes
differently (tests/test_stage_plan_cpu.py: test_pil_differs_from_the_restatement_by_pass_order_only).  One band-height
row, c_u8_r8, keeps a real horizontal resample (8 -> 37 columns) in front of its R = 8 bands: at 526 x 8 every Pillow
resamples horizontally first.  `want` is what the row is there for, as the plan query words it; both
tiers assert it, so a later change of dispatch cannot quietly move a row.
"""
import collections
import math

# ---- one-stage resize, crop form: coclr_stage_crops (f32), coclr_resize_crops_u8 (u8), coclr_stage_crops_ragged -----
# sizes   (H, W) of every frame; the one-size forms take frames of one size
# slots   per output clip the T frames it reads (indices into sizes); frames may repeat and be shared
# crops   one-size forms: the launch's (x0, y0, flip) list, every clip gets every crop
#         ragged forms: one (x0, y0, flip) per clip, held to the clip's own frame (all slots of a clip share a size)
# out_off floats between a 16-byte boundary and the fp32 output
Crop = collections.namedtuple("Crop", "name form sizes slots crops cw ch S out_off refuse want")


def crop(name, form, sizes, slots, crops, cw, ch, S, out_off=0, refuse=False, **want):
    return Crop(name, form, tuple(sizes), tuple(map(tuple, slots)), tuple(crops), cw, ch, S, out_off, refuse, want)


_TEN = [(0, 0, 0), (24, 12, 0), (24, 0, 0), (0, 12, 0), (12, 6, 0), (0, 0, 1), (24, 12, 1), (24, 0, 1), (0, 12, 1),
        (12, 6, 1), (5, 3, 0), (5, 3, 1), (23, 11, 0), (1, 1, 1), (24, 11, 0), (23, 12, 1)]

CROPS = [
    # ten-crop style: 16 crops of 28 x 28 in 40 x 52 frames, flush with the right and bottom edges with and without
    # flip, flip at x0 = 0; one band (S <= R) whose cap is the box height; 16-byte stores
    crop("c_sixteen", "f32", [(40, 52)] * 3, [(0, 1), (1, 1), (2, 0)], _TEN, 28, 28, 16,
         R=32, bands=1, clipped=True, vec=True),
    # the same stores from an output one float off a 16-byte boundary: the guarded 4-byte path although S % 4 == 0
    crop("c_f32_out_off", "f32", [(40, 52)] * 2, [(1, 0)], [(24, 12, 1), (0, 0, 0)], 28, 28, 16, out_off=1,
         R=32, vec=False),
    crop("c_rag_f32_out_off", "rag_f32", [(30, 33), (28, 28), (41, 29)], [(0, 0), (1, 1), (2, 2)],
         [(5, 2, 0), (0, 0, 1), (1, 13, 0)], 28, 28, 16, out_off=1, R=32, vec=False),
    # band heights: the smallest box height found for each R, S % 4 != 0 (padded tables, guarded stores), S % R != 0
    crop("c_f32_r16", "f32", [(290, 40)], [(0,)], [(0, 2, 0), (3, 4, 1)], 37, 286, 37, R=16, bands=3, clipped=False),
    crop("c_u8_r8", "u8", [(526, 10)] * 2, [(0, 1)], [(2, 0, 1)], 8, 526, 37, R=8, bands=5),
    # three frame sizes, shared slot offsets, a box on its own frame's right and bottom edge before a larger frame
    crop("c_rag_f32_r4", "rag_f32", [(924, 61), (930, 64), (940, 70)], [(0, 0), (1, 1), (2, 2), (1, 1)],
         [(0, 0, 1), (3, 6, 0), (1, 5, 1), (3, 6, 1)], 61, 924, 61, R=4, bands=16),
    crop("c_rag_u8_r2", "rag_u8", [(1457, 97), (1460, 99), (1470, 100)], [(0,), (1,), (2,), (1,)],
         [(0, 0, 0), (2, 3, 1), (0, 13, 0), (0, 0, 0)], 97, 1457, 97, R=2, bands=49),
    crop("c_u8_r1", "u8", [(2059, 137)], [(0,)], [(0, 0, 1)], 137, 2059, 137, R=1, bands=137),
    # one output row per band and more than 32 KiB of LDS
    crop("c_f32_r1_big", "f32", [(3000, 200)], [(0,)], [(0, 0, 0)], 200, 3000, 200, R=1, bands=200, vec=True),
    # up-sampling (5 taps), identity (cw == S), one pixel
    crop("c_u8_up", "u8", [(9, 11)] * 2, [(1, 0)], [(2, 1, 0), (5, 3, 1)], 6, 5, 14, R=32),
    crop("c_rag_u8_identity", "rag_u8", [(14, 15), (12, 12), (20, 13)], [(0,), (1,), (2,)],
         [(3, 2, 0), (0, 0, 1), (1, 8, 1)], 12, 12, 12, R=32, clipped=True),
    crop("c_f32_pixel", "f32", [(5, 6)], [(0,)], [(5, 4, 0), (0, 0, 1), (2, 2, 0)], 1, 1, 8, R=32, clipped=True),
    # refused: one output row's taps do not fit 64 KiB; more than 64 taps
    crop("c_refuse_lds", "u8", [(5062, 1)], [(0,)], [(0, 0, 0)], 1, 5062, 337, refuse=True),
    crop("c_refuse_taps", "rag_f32", [(130, 4)], [(0,)], [(0, 0, 0)], 4, 130, 8, refuse=True),
]

# ---- one-stage resize, box form: coclr_resize_boxes_u8, coclr_resize_boxes_ragged_u8 --------------------------------
# sizes  (H, W) of every source clip's T frames; clips: (source, (x0, y0, w, h)) or (source, box, extra y taps: the
# box's y table is handed over with that many more zero taps than PIL needs); sources may be shared
Box = collections.namedtuple("Box", "name ragged sizes T clips S refuse want")


def box(name, ragged, sizes, T, clips, S, refuse=False, **want):
    return Box(name, ragged, tuple(sizes), T, tuple(clips), S, refuse, want)


BOXES = [
    # the tallest box (clip 1, the whole frame, 11 taps) and the most-tapped box (clip 2, 7 rows, its 5 taps padded to
    # 15) are different clips, every table at its own offset; up-sampling, identity, one pixel wide, one pixel high
    box("b_mixed", False, [(40, 30)] * 2, 2,
        [(0, (3, 2, 20, 37)), (1, (0, 0, 30, 40)), (0, (4, 5, 6, 7), 10), (1, (10, 20, 18, 18)), (1, (29, 0, 1, 40)),
         (0, (0, 39, 30, 1)), (0, (12, 22, 18, 18))], 18, R=32, bands=1, clipped=True),
    box("b_r16", False, [(286, 37)], 1, [(0, (0, 0, 37, 286)), (0, (0, 100, 37, 180))], 37, R=16, bands=3),
    box("b_rag_r8", True, [(526, 37), (530, 40), (60, 70)], 2,
        [(0, (0, 0, 37, 526)), (2, (30, 20, 40, 40)), (1, (3, 8, 37, 522)), (0, (0, 3, 37, 500))], 37, R=8, bands=5),
    box("b_r4", False, [(924, 61)], 1, [(0, (0, 0, 61, 924))], 61, R=4),
    box("b_rag_r2", True, [(1457, 97), (1458, 98), (20, 21)], 1, [(0, (0, 0, 97, 1457)), (2, (4, 0, 17, 20)),
                                                                    (1, (1, 1, 97, 1457))], 97, R=2),
    box("b_rag_r1_big", True, [(3000, 200), (16, 16), (24, 40)], 1,
        [(0, (0, 0, 200, 3000)), (1, (0, 0, 16, 16)), (2, (20, 10, 20, 14))], 200, R=1, bands=200),
    box("b_refuse_lds", True, [(5062, 1)], 1, [(0, (0, 0, 1, 5062))], 337, refuse=True),
    box("b_refuse_taps", False, [(130, 2)], 1, [(0, (0, 0, 2, 130))], 8, refuse=True),
]

# ---- two-stage resize: coclr_resize2_boxes, coclr_resize2_boxes_ragged, byte and fp32 outputs -----------------------
# clips: (source, region (x0, y0, w, h), resample (ow, oh), window (cx, cy)); a drawn box is ow = oh = size, window 0
Two = collections.namedtuple("Two", "name form sizes T clips size S refuse want")


def two(name, form, sizes, T, clips, size, S, refuse=False, **want):
    return Two(name, form, tuple(sizes), T, tuple(clips), size, S, refuse, want)


def _drawn(src, x0, y0, w, h, size):
    return (src, (x0, y0, w, h), (size, size), (0, 0))


TWOS = [
    # more than 64 KiB of LDS in each instantiation (the dynamic-LDS opt-in), at four band heights
    two("t_f32_r32_big", "f32", [(114, 6)], 1, [_drawn(0, 1, 2, 4, 112, 112)], 112, 32, R=32, optin=True, one="h1"),
    two("t_u8_r16_big", "u8", [(200, 5)], 1, [_drawn(0, 0, 0, 5, 200, 112)], 112, 32, R=16, optin=True),
    two("t_rag_f32_r8_big", "rag_f32", [(8, 9), (10, 6), (12, 12)], 1,
        [_drawn(0, 1, 0, 8, 8, 224), _drawn(1, 0, 2, 6, 8, 224), _drawn(2, 5, 3, 7, 8, 224)], 224, 24,
        R=8, optin=True, one="h2"),
    two("t_rag_u8_r1_big", "rag_u8", [(250, 4), (30, 20), (252, 5)], 1,
        [_drawn(0, 0, 0, 4, 250, 112), _drawn(1, 3, 4, 10, 20, 112), _drawn(2, 1, 2, 4, 250, 112)], 112, 8,
        R=1, optin=True),
    two("t_f32_r4", "f32", [(250, 4)], 2, [_drawn(0, 0, 0, 3, 250, 112)], 112, 16, R=4, optin=False),
    two("t_rag_u8_r2", "rag_u8", [(200, 4), (128, 3), (64, 64)], 1,
        [_drawn(0, 0, 0, 4, 200, 112), _drawn(1, 0, 0, 3, 128, 112), _drawn(2, 10, 10, 50, 50, 112)], 112, 8,
        R=2, optin=True),
    # the fallback: the whole frame resampled to (ow, oh) and a window in its middle; size % 4 != 0 and S % 4 != 0
    two("t_u8_fallback", "u8", [(20, 30)] * 2, 2, [(1, (0, 0, 30, 20), (27, 22), (4, 2)), _drawn(0, 3, 1, 20, 18, 18),
                                                    (0, (0, 0, 30, 20), (18, 27), (0, 9))], 18, 13, R=32),
    # size == S: PIL's identity as the second stage
    two("t_rag_f32_identity", "rag_f32", [(20, 30), (16, 16), (31, 17)], 1,
        [_drawn(0, 2, 1, 25, 19, 16), _drawn(1, 0, 0, 16, 16, 16), (2, (0, 0, 17, 31), (16, 29), (0, 6))], 16, 16,
        R=32),
    # S > size: the second stage up-samples, and H2's rows, not H1's, size the shared buffer
    two("t_f32_up", "f32", [(12, 14)], 1, [_drawn(0, 1, 1, 12, 10, 16)], 16, 24, R=32, one="h2", optin=False),
    # one output row's halo of intermediate and source rows does not fit the CU's LDS
    two("t_refuse", "u8", [(800, 4)], 1, [_drawn(0, 0, 0, 4, 800, 224)], 224, 16, refuse=True),
]

# ---- coclr_stage_clips ------------------------------------------------------------------------------------------------
# src_off / out_off: ELEMENTS between a 16-byte boundary and the source / the fp32 output
Clips = collections.namedtuple("Clips", "name u8 B C S thw src_off out_off refuse want")


def clips(name, u8, B, C, S, thw, src_off=0, out_off=0, refuse=False, **want):
    return Clips(name, u8, B, C, S, thw, src_off, out_off, refuse, want)


GRID_THW = 64 * 256 * 16 + 16        # uint8: one 16-byte item more than 64 workgroups take in one sweep

CLIPS = [
    clips("s_u8_vec", True, 2, 3, 2, 48, vec=True),
    clips("s_u8_len", True, 2, 3, 2, 40, vec=False),                   # THW % 16 != 0
    clips("s_u8_src_off", True, 1, 3, 2, 32, src_off=1, vec=False),
    clips("s_u8_out_off", True, 2, 3, 1, 32, out_off=1, vec=False),    # stored 16 bytes through `out` before ABI 26
    clips("s_f32_vec", False, 2, 1, 3, 12, vec=True),                  # C = 1
    clips("s_f32_len", False, 1, 4, 2, 10, vec=False),                 # C = 4, THW % 4 != 0
    clips("s_f32_src_off", False, 2, 3, 1, 8, src_off=1, vec=False),
    clips("s_f32_out_off", False, 1, 3, 2, 8, out_off=1, vec=False),
    clips("s_u8_grid", True, 1, 1, 2, GRID_THW, vec=True, gx=64),      # the grid-stride loop runs twice, a tail
    clips("s_u8_grid_scalar", True, 1, 1, 1, 64 * 256 + 5, vec=False),  # the 1-byte loop past its grid
    clips("s_refuse", False, 4, 4, 4096, 4, refuse=True),              # B * C * S = 65536
]

# ---- programs: coclr_color_jitter_clips (aug False), coclr_augment_clips ----------------------------------------------
# programs: one list of (kind, parameter) per group, padded with NOPs to the longest; frame n runs n // group_size.
# A blur's parameter is PIL's fp32 box radius itself (what the kernel takes).
Prog = collections.namedtuple("Prog", "name aug N H W T programs group_size want")
NOP, BRI, CON, SAT, HUE, GRAY, BLUR, FLIP = range(8)


def prog(name, aug, N, H, W, T, programs, group_size, **want):
    return Prog(name, aug, N, H, W, T, tuple(tuple(p) for p in programs), group_size, want)


PROGS = [
    # H * W = 35: a last item of three pixels, frames 1.. start off a 4-byte boundary; contrast first, last and twice
    # in a row; five frames in groups of two: the last group has one
    prog("p_jit_contrast", False, 5, 5, 7, 1,
         [[(CON, 1.3), (BRI, 0.8), (HUE, 23)], [(SAT, 1.4), (GRAY, 1), (CON, 0.6)], [(CON, 0.5), (CON, 1.7)]], 2,
         use_lds=True, cuts=2, vec=False),
    # no whole-frame op: one pass, global to global, no LDS
    prog("p_jit_no_lds", False, 4, 6, 5, 2, [[(BRI, 1.2), (SAT, 0.7), (HUE, 200), (GRAY, 2)]], 4,
         use_lds=False, lds=0, cuts=0),
    prog("p_aug_no_lds_flip", True, 2, 4, 6, 2, [[(FLIP, 0), (BRI, 0.9)], [(SAT, 1.5), (NOP, 0)]], 1,
         use_lds=False, vec=False),
    # W % 4 != 0 with flip and blur (the byte paths); contrast on both sides of a blur; radii below 1, 16 (more than
    # either side of the frame), and in between
    prog("p_aug_blur_bytes", True, 3, 9, 10, 1,
         [[(CON, 1.2), (BLUR, 0.5), (CON, 0.7), (FLIP, 0)], [(BLUR, 16.0), (FLIP, 0), (HUE, 77)],
          [(BRI, 1.1), (BLUR, 2.25), (FLIP, 0), (FLIP, 0)]], 1, use_lds=True, cuts=3, vec=False),
    # eight ops and no NOP; W % 4 == 0: the dword path of the vertical passes and the mirrored 16-byte stores
    prog("p_aug_eight", True, 2, 6, 8, 2,
         [[(BRI, 1.3), (CON, 0.8), (SAT, 1.2), (HUE, 250), (BLUR, 1.375), (FLIP, 0), (CON, 1.1), (GRAY, 0)]], 2,
         use_lds=True, cuts=3, vec=True),
    # the largest frame: 13 items a lane across the blur's barrier, 147 KiB of LDS
    prog("p_aug_224", True, 1, 224, 224, 1, [[(CON, 1.3), (BLUR, 1.375), (CON, 0.6), (FLIP, 0)]], 1,
         use_lds=True, per_lane=13, lds=224 * 224 * 3, vec=True),
]

FAMILIES = {"crop": CROPS, "box": BOXES, "two": TWOS, "clips": CLIPS, "prog": PROGS}
ALL = [r for rows in FAMILIES.values() for r in rows]
BY_NAME = {r.name: r for r in ALL}
assert len(BY_NAME) == len(ALL)

MAX_BYTES = 4 << 20          # inputs plus outputs of any row


def family(row):
    return {Crop: "crop", Box: "box", Two: "two", Clips: "clips", Prog: "prog"}[type(row)]


def ntaps(n_in, n_out):
    """Taps of PIL's BICUBIC tables for n_in -> n_out samples."""
    return int(math.ceil(2.0 * max(n_in / n_out, 1.0))) * 2 + 1


def ragged_offsets(sizes, T=1):
    """Byte offset of every source (T frames of its size at 3 * H * W bytes rounded up to 16) in one flat buffer, and
    the buffer's length."""
    off, at = [], 0
    for H, W in sizes:
        off.append(at)
        at += T * ((3 * H * W + 15) & ~15)
    return off, at


def row_bytes(row):
    fam = family(row)
    if fam == "clips":
        n = row.B * row.C * row.S * row.thw
        return n * (1 if row.u8 else 4) + n * 4
    if fam == "prog":
        return row.N * row.H * row.W * 3 * 5
    S = row.S
    src = sum(3 * H * W for H, W in row.sizes) * (row.T if fam != "crop" else 1)
    if fam == "crop":
        images = len(row.slots) * len(row.slots[0]) * (1 if row.form.startswith("rag") else len(row.crops))
        return src + images * S * S * 3 * (1 if row.form.endswith("u8") else 4)
    images = len(row.clips) * row.T
    return src + images * S * S * 3 * (4 if fam == "two" and row.form.endswith("f32") else 1)


# ---- what the launchers would do --------------------------------------------------------------------------------------

def crop_descriptors(row):
    """Ragged crop rows: (desc int32 (n_clips, 5), slot_off int64 (n_clips, T), nbytes)."""
    import torch
    off, nbytes = ragged_offsets(row.sizes)
    desc = torch.tensor([[x0, y0, flip, row.sizes[s[0]][1], row.sizes[s[0]][0]]
                         for (x0, y0, flip), s in zip(row.crops, row.slots)], dtype=torch.int32)
    slot_off = torch.tensor([[off[i] for i in s] for s in row.slots], dtype=torch.int64)
    return desc, slot_off, nbytes


def box_descriptors(row):
    """(desc int32 (n_clips, 10 or 14), xtab, ytab): every clip's tables at an offset of their own, from
    crops_harness.kernel_layout."""
    import torch
    import crops_harness as CH
    off, _ = ragged_offsets(row.sizes, row.T)
    desc = torch.zeros(len(row.clips), 14 if row.ragged else 10, dtype=torch.int32)
    bufs, fill = ([], []), [0, 0]
    for k, clip in enumerate(row.clips):
        src, (x0, y0, w, h) = clip[:2]
        desc[k, :6] = torch.tensor([0 if row.ragged else src * row.T, row.T, x0, y0, w, h], dtype=torch.int32)
        for axis, n_in in ((0, w), (1, h)):
            lo, K = CH.kernel_layout(n_in, row.S)
            if axis == 1 and len(clip) > 2:
                K = torch.cat([K, torch.zeros(clip[2], K.shape[1], dtype=torch.int32)])
            t = torch.cat([lo[None], K]).reshape(-1)
            desc[k, 6 + axis], desc[k, 8 + axis] = fill[axis], K.shape[0]
            bufs[axis].append(t)
            fill[axis] += t.numel()
        if row.ragged:
            H, W = row.sizes[src]
            desc[k, 10:] = torch.tensor([off[src] & 0x7fffffff, off[src] >> 32, W, H], dtype=torch.int32)
    return desc, torch.cat(bufs[0]), torch.cat(bufs[1])


def two_descriptors(row):
    """(desc int32 (n_clips, 14 or 18), xtab, ytab, tab2) from cls_harness.descriptors."""
    import torch
    import cls_harness as CL
    ragged = row.form.startswith("rag")
    off, _ = ragged_offsets(row.sizes, row.T)
    desc, xtab, ytab, tab2 = CL.descriptors([(0 if ragged else src * row.T, region, resample, window)
                                             for src, region, resample, window in row.clips], row.T, row.size, row.S)
    if ragged:
        rag = torch.tensor([[off[src] & 0x7fffffff, off[src] >> 32, row.sizes[src][1], row.sizes[src][0]]
                            for src, _, _, _ in row.clips], dtype=torch.int32)
        desc = torch.cat([desc, rag], 1).contiguous()
    return desc, xtab, ytab, tab2


def program_tables(row):
    """(kinds int32 (G, P), params fp32 (G, P)), shorter programs padded with NOPs."""
    import torch
    P = max(len(p) for p in row.programs)
    kinds = torch.zeros(len(row.programs), P, dtype=torch.int32)
    params = torch.zeros(len(row.programs), P, dtype=torch.float32)
    for g, p in enumerate(row.programs):
        for j, (kind, v) in enumerate(p):
            kinds[g, j], params[g, j] = kind, v
    return kinds, params


def plan(row, **addr):
    """The plan query of the row's launcher; `addr`: out_addr / src_addr of the tensors a launch will use (default:
    aligned, then the row's offsets added).  Raises coclr_amd._lib.HipLibraryError where the launcher refuses."""
    from coclr_amd import ops
    fam = family(row)
    if fam == "crop":
        u8, T = row.form.endswith("u8"), len(row.slots[0])
        out_addr = addr.get("out_addr", ops.PLAN_ADDR + 4 * row.out_off)
        xt, yt = ntaps(row.cw, row.S), ntaps(row.ch, row.S)
        if row.form.startswith("rag"):
            desc, slot_off, nbytes = crop_descriptors(row)
            return ops.stage_crops_ragged_plan(nbytes, desc, slot_off, row.cw, row.ch, row.S, xt, yt, u8=u8,
                                               out_addr=out_addr)
        H, W = row.sizes[0]
        return ops.stage_crops_plan(len(row.sizes), H, W, len(row.slots), T, row.crops, row.cw, row.ch, row.S, xt, yt,
                                    u8=u8, out_addr=out_addr)
    if fam == "box":
        desc, xtab, ytab = box_descriptors(row)
        if row.ragged:
            return ops.resize_boxes_plan(desc, row.T, row.S, xtab.numel(), ytab.numel(),
                                         nbytes=ragged_offsets(row.sizes, row.T)[1])
        H, W = row.sizes[0]
        return ops.resize_boxes_plan(desc, row.T, row.S, xtab.numel(), ytab.numel(),
                                     shape=(len(row.sizes) * row.T, H, W))
    if fam == "two":
        desc, xtab, ytab, tab2 = two_descriptors(row)
        kw = dict(u8=row.form.endswith("u8"), out_addr=addr.get("out_addr", ops.PLAN_ADDR))
        if row.form.startswith("rag"):
            kw["nbytes"] = ragged_offsets(row.sizes, row.T)[1]
        else:
            kw["shape"] = (len(row.sizes) * row.T,) + row.sizes[0]
        return ops.resize2_boxes_plan(desc, row.T, row.size, row.S, xtab.numel(), ytab.numel(), tab2.shape[0] - 1, **kw)
    if fam == "clips":
        esz = 1 if row.u8 else 4
        return ops.stage_clips_plan(row.B, row.C, row.S, row.thw, row.u8,
                                    src_addr=addr.get("src_addr", ops.PLAN_ADDR + esz * row.src_off),
                                    out_addr=addr.get("out_addr", ops.PLAN_ADDR + 4 * row.out_off))
    kinds, params = program_tables(row)
    return ops.jitter_plan(row.aug, row.N, row.H, row.W, row.T, kinds, params, row.group_size,
                           out_addr=addr.get("out_addr", ops.PLAN_ADDR))


# ---- inputs and references ----------------------------------------------------------------------------------------------

def edges(H, W, seed):
    """A random frame (train_harness.frames) with saturated 0 / 255 stripes along both axes and a bright pixel in a dark
    patch, so that the bicubic overshoot clips both ways whichever axis the row is about."""
    import train_harness as TH
    f = TH.frames(1, H, W, seed)[0]
    f[::2, W // 3:W // 3 + 3] = 255
    f[1::2, W // 3:W // 3 + 3] = 0
    f[H // 3:H // 3 + 3, ::2] = 0
    f[H // 3:H // 3 + 3, 1::2] = 255
    f[H // 2:, :max(W // 4, 1)] = 0
    f[min(H // 2 + 1, H - 1), 0] = (255, 200, 255)
    return f


def sources(row):
    """Resize rows: per entry of row.sizes a uint8 array (T, H, W, 3) (crop form: T = 1)."""
    import numpy as np
    T = 1 if family(row) == "crop" else row.T
    seed = sum(map(ord, row.name))
    return [np.stack([edges(H, W, seed + 31 * i + t) for t in range(T)]) for i, (H, W) in enumerate(row.sizes)]


def flat_buffer(row, src):
    """The ragged forms' flat byte buffer (numpy uint8) of `src` = sources(row): unused bytes are 0x33."""
    import numpy as np
    T = 1 if family(row) == "crop" else row.T
    off, nbytes = ragged_offsets(row.sizes, T)
    buf = np.full(nbytes, 0x33, dtype=np.uint8)
    for o, s in zip(off, src):
        step = (s[0].size + 15) & ~15
        for t in range(s.shape[0]):
            buf[o + t * step:o + t * step + s[t].size] = s[t].reshape(-1)
    return buf


def resize_reference(row, src):
    """The resized bytes of a resize row from the restatements (crops_harness, cls_harness), as uint8:
    crop form, one-size: (n_crops, n_clips, T, S, S, 3); ragged: (n_clips, T, S, S, 3); box and two-stage forms:
    (n_clips, T, S, S, 3)."""
    import numpy as np
    import cls_harness as CL
    import crops_harness as CH
    fam = family(row)
    if fam == "crop":
        if row.form.startswith("rag"):
            return np.stack([np.stack([CH.crop_resized_u8(src[i], [c], row.cw, row.ch, row.S)[0][0] for i in s])
                             for c, s in zip(row.crops, row.slots)])
        frames = np.concatenate(src)
        per = CH.crop_resized_u8(frames, list(row.crops), row.cw, row.ch, row.S)
        return np.stack([p[np.asarray(row.slots)] for p in per])
    if fam == "box":
        return np.stack([CH.crop_resized_u8(src[s], [(x0, y0, 0)], w, h, row.S)[0] for s, (x0, y0, w, h) in (c[:2] for c in row.clips)])
    return np.stack([CL.resized_u8(src[s], region, resample, window, row.size, row.S)
                     for s, region, resample, window in row.clips])


def program_frames(row):
    import numpy as np
    seed = sum(map(ord, row.name))
    return np.stack([edges(row.H, row.W, seed + n) for n in range(row.N)])


def program_reference_u8(row, frames):
    """uint8 (N, H, W, 3) from train_harness (which falls through to jitter_harness for kinds 0..5)."""
    import train_harness as TH
    return TH.augment_u8(frames, [list(p) for p in row.programs], row.group_size)
