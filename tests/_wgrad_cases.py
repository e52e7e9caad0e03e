"""Small geometries that between them reach every weight-gradient kernel instantiation the launcher of
coclr_amd/csrc/conv_wgrad.hip can select, and every dispatch edge listed in tests/test_wgrad_plan_cpu.py.

Shared by the CPU-tier coverage test (tests/test_wgrad_plan_cpu.py: the planner query says what each row reaches)
and the exact-arithmetic GPU test (tests/test_gpu_wgrad_exact.py: each row against float64).  Every row has at
most 32768 output positions and channels no wider than the edge it is there for needs.
"""
import collections

Case = collections.namedtuple("Case", "name N Cin Cout dims k s p algo odim slice_of")


def _c(name, N, Cin, Cout, dims, k, s, p, algo=0, odim=None, slice_of=None):
    return Case(name, N, Cin, Cout, dims, k, s, p, algo, odim, slice_of)


P0, S1 = (0, 0, 0), (1, 1, 1)
K1, K133, K311, K711, K177 = (1, 1, 1), (1, 3, 3), (3, 1, 1), (7, 1, 1), (1, 7, 7)

CASES = [
    # ---- first-generation kernel <BJ, PCH>: BJ 64 = pointwise, 128 = stencil ---------------------------------
    # pointwise, Cin < 8; 50 positions per sample in 64-position boxes of two samples, N odd: phantom sample
    _c("g1_pw_cin3", 3, 3, 24, (2, 5, 5), K1, S1, P0),
    # pointwise strided along T (resnet_2d3d.py downsample form): window of 7 frames per 4 outputs
    _c("g1_pw_st2", 3, 24, 40, (7, 4, 4), K1, (2, 1, 1), P0),
    # r50's (1,1,1)/(1,2,2) downsample
    _c("g1_pw_s122", 3, 40, 72, (2, 7, 7), K1, (1, 2, 2), P0),
    _c("g1_pw_s222", 3, 24, 40, (3, 6, 6), K1, (2, 2, 2), P0),
    # Cin < 48 sends a (1,3,3) layer to the first generation (Mixed_*.branch1/2 squeeze widths 16-48)
    _c("g1_133_cin16", 3, 16, 72, (3, 7, 7), K133, S1, (0, 1, 1)),
    # 104 boxes: split 26 rounded down to 24 in the first-generation kernel
    _c("g1_133_split", 1, 8, 50, (13, 32, 32), K133, S1, (0, 1, 1)),
    # Cout < 48; enough boxes for a split count in 4..15
    _c("g1_311_cout24", 2, 72, 24, (9, 6, 6), K311, S1, (1, 0, 0)),
    # strided temporal stem conv, narrow
    _c("g1_711s2_cin24", 3, 24, 72, (8, 4, 4), K711, (2, 1, 1), (3, 0, 0)),
    # r50's strided (1,3,3)/(1,2,2): its window never fits the wave-specialised kernel
    _c("g1_133s2", 2, 72, 40, (3, 13, 13), K133, (1, 2, 2), (0, 1, 1)),
    # ---- wave-specialised kernel, direct forms --------------------------------------------------------------
    _c("w1_133_pch2", 3, 72, 80, (2, 6, 6), K133, S1, (0, 1, 1)),
    _c("w1_133_pch3", 3, 72, 80, (3, 4, 4), K133, S1, (0, 1, 1)),
    # Cout*Cin*taps > 8192*64: the fold's grid-stride loop; 4 x 4 tiles
    _c("w1_133_256", 3, 256, 256, (2, 4, 4), K133, S1, (0, 1, 1)),
    _c("w2_311", 3, 72, 80, (5, 3, 3), K311, S1, (1, 0, 0)),
    # 102 boxes: split 25 rounded down to 24 (>= 16: a multiple of 8), which does not divide 102
    _c("w2_311_split", 2, 50, 50, (9, 16, 17), K311, S1, (1, 0, 0)),
    _c("w3_711s2", 3, 72, 80, (10, 3, 3), K711, (2, 1, 1), (3, 0, 0)),
    # pointwise: the fused 1x1x1 heads of an inception block (Cout = three heads side by side)
    _c("w4_pw_big", 3, 72, 100, (2, 5, 5), K1, S1, P0),             # 50 positions: no 16-byte DMA
    _c("w4_pw_big_tiles", 2, 136, 200, (2, 3, 3), K1, S1, P0),      # 2 x 2 tiles of 128 x 128
    _c("w5_pw_small", 3, 24, 100, (3, 3, 3), K1, S1, P0),           # 27 positions, box spans 2 samples
    _c("pw4_dma", 3, 72, 100, (2, 8, 8), K1, S1, P0),               # 128 positions per sample
    _c("pw5_dma", 2, 40, 100, (3, 8, 8), K1, S1, P0),
    _c("pw5_dma_split", 1, 16, 24, (4, 40, 40), K1, S1, P0),        # 100 boxes, split 24
    _c("pw4_dma_tile_order", 1, 128, 72, (2, 64, 64), K1, S1, P0),  # a 4 MiB sample: tile-fastest by default
    # ---- Winograd-domain forms -------------------------------------------------------------------------------
    _c("w6_odd_frames", 3, 72, 80, (5, 3, 3), K311, S1, (1, 0, 0), algo=1),
    _c("w6_phantom", 3, 72, 80, (3, 2, 2), K311, S1, (1, 0, 0), algo=1),   # boxes of 4 samples, N = 3
    _c("w6_f43_fwd", 2, 50, 72, (8, 8, 8), K311, S1, (1, 0, 0), algo=2),
    _c("w7_rebox", 2, 72, 72, (2, 6, 20), K133, S1, (0, 1, 1), algo=1),
    _c("w7_plain", 3, 50, 80, (2, 8, 8), K133, S1, (0, 1, 1), algo=1),
    _c("w7_pch3", 3, 72, 72, (1, 4, 4), K133, S1, (0, 1, 1), algo=1),
    _c("w7_t_overhang", 1, 72, 72, (3, 4, 4), K133, S1, (0, 1, 1), algo=1),
    _c("w7_split", 1, 64, 48, (6, 16, 16), K133, S1, (0, 1, 1), algo=1),
    # ---- (1,7,7) stem -----------------------------------------------------------------------------------------
    _c("stem", 3, 3, 24, (2, 20, 20), K177, (1, 2, 2), (0, 3, 3)),
    _c("stem_phantom", 3, 3, 24, (1, 8, 20), K177, (1, 2, 2), (0, 3, 3)),  # boxes of 2 samples, N = 3
    _c("stem_cout72", 1, 3, 72, (1, 12, 20), K177, (1, 2, 2), (0, 3, 3)),
    # temporal tap 3 of r50's (5,7,7)/(1,2,2) pad (2,3,3) stem, as the engine slices it: pad_t = 2 - 3
    _c("stem_slice_kt3", 2, 3, 40, (4, 12, 20), K177, (1, 2, 2), (-1, 3, 3), odim=(4, 6, 10),
       slice_of=((5, 7, 7), (2, 3, 3), 3)),
]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# every <family, id, PCH, BJ> the launcher's selection can name (coclr_conv3d_wgrad_plan out[0..3]); the stem's
# BatchNorm form is the same plan with out[14] set
INSTANTIATIONS = (
    [("gen1", 0, pch, bj) for bj in (64, 128) for pch in (2, 4, 8, 20)] +
    [("wave", 1, 2, 0), ("wave", 1, 3, 0), ("wave", 2, 2, 0), ("wave", 3, 4, 0), ("wave", 4, 2, 0),
     ("wave", 5, 2, 0), ("wave", 6, 2, 0), ("wave", 7, 2, 0), ("wave", 7, 3, 0)] +
    [("pwdma", 4, 0, 0), ("pwdma", 5, 0, 0)] +
    [("stem", 9, 20, 0), ("stem+bn", 9, 20, 0)])

# instantiations no accepted geometry reaches, with the planner condition that excludes them
UNREACHABLE = {
    ("gen1", 0, 2, 128):
        "BJ 128 means taps > 1; a first-generation box always holds 2^7 positions (lTW + lTH + lTT + lTN = 7, "
        "conv_pick_box) and its window has ((2^l - 1) * stride + k) >= 2^l elements per axis, strictly more on an "
        "axis with k > 1, so plane > 128 and pch = cdiv(plane, 64) >= 3: plan_wgrad never picks variant 0",
}


def geom(case):
    from coclr_amd import ops
    return ops.ConvGeom(case.N, case.Cin, case.Cout, case.dims, case.k, case.s, case.p, odim=case.odim,
                        algo=case.algo)


def instantiation(plan):
    return (plan["family"], plan["id"], plan["pch"], plan["bj"])


def family(plan):
    """The six kernel families an edge has to be hit in."""
    if plan["family"] == "wave":
        return {6: "wino6", 7: "wino7"}.get(plan["id"], "wave_direct")
    return plan["family"]


FAMILIES = ("gen1", "wave_direct", "wino6", "wino7", "pwdma", "stem")


def planned_extents(case, plan):
    """(Wo, Ho, To) as the planner boxes them: axes the stencil does not touch are flattened into W
    (conv_normalise), and the F(2,3) form counts frame PAIRS."""
    To, Ho, Wo = geom(case).odim
    free = [case.k[i] == 1 and case.s[i] == 1 and case.p[i] == 0 and case.odim is None for i in range(3)]
    if free[1] and free[2]:
        Wo, Ho = Ho * Wo, 1
        if free[0]:
            Wo, To = Wo * To, 1
    if family(plan) == "wino6":
        To = (To + 1) // 2
    return Wo, Ho, To
