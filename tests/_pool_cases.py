"""Max-pool (and pooled-BatchNorm-backward) test rows: small shapes that reach every kernel instantiation the
launchers of coclr_amd/csrc/pool.hip can select and every dispatch edge listed in tests/test_pool_plan_cpu.py.

Shared by the CPU-tier coverage test (tests/test_pool_plan_cpu.py: coclr_pool_plan says what each row reaches)
and the GPU test (tests/test_gpu_pool_exact.py: every row against float64).  No torch import here.

A row is one pool geometry plus the layout of its operands:
  x_extra / y_extra / d_extra   channels of the wider buffer x / y / (dy and dx) is a slice of (0: dense)
  x_pad / d_pad                 extra floats between the samples of x / of dy and dx (sample strides that are not
                                a multiple of 4 even where C * S is)
  aff                           in-affine applied while x is read: None, "plain" or "relu"; scales +-2^k of both
                                signs, small-integer shifts
  special                       the -inf / NaN input pattern instead of relu(randn)
  pooled                        the row also runs the pooled BatchNorm backward (y is then the unit's convolution
                                output, the pool read it through the affine)
"""
import collections

Case = collections.namedtuple(
    "Case", "name N C idim k s p x_extra y_extra d_extra x_pad d_pad aff special pooled")


def case(name, N, C, idim, k, s, p, x_extra=0, y_extra=0, d_extra=0, x_pad=0, d_pad=0, aff=None, special=False,
         pooled=False):
    return Case(name, N, C, tuple(idim), tuple(k), tuple(s), tuple(p), x_extra, y_extra, d_extra, x_pad, d_pad,
                aff, special, pooled)


K333, S1, P1 = (3, 3, 3), (1, 1, 1), (1, 1, 1)
K133, S122, P011 = (1, 3, 3), (1, 2, 2), (0, 1, 1)
S222, K222, P0 = (2, 2, 2), (2, 2, 2), (0, 0, 0)
K111 = (1, 1, 1)

CASES = [
    # ---- separable 3x3x3 / 1 / 1 forward: TT = 4, 8, 16 and the run-time form; H*W = 16, 32, 64, 256 -------------
    case("sep_t4_hw16", 2, 5, (4, 4, 4), K333, S1, P1, special=True),                   # 10 planes: gcount < PG
    case("sep_t8_hw32", 2, 3, (8, 4, 8), K333, S1, P1, x_extra=2, y_extra=1, aff="relu", pooled=True),   # 8x4 plane
    case("sep_t16_hw64", 1, 5, (16, 8, 8), K333, S1, P1),
    case("sep_t1_hw256", 2, 3, (1, 16, 16), K333, S1, P1),
    case("sep_t5_hw16_scalar", 3, 7, (5, 4, 4), K333, S1, P1, x_pad=1, aff="plain"),    # x_nstride % 4 != 0
    case("sep_t32_hw256", 1, 3, (32, 16, 16), K333, S1, P1),     # 64 KiB without indices; tiled with them
    case("sep_t4_hw64_many", 2, 1025, (4, 8, 8), K333, S1, P1, d_extra=1),   # backward: (3,3,3,1) with G = 2
    # ---- its fall-throughs to the tiled (3,3,3)/(1,1,1) template ------------------------------------------------
    case("ft_t33", 2, 2, (33, 4, 4), K333, S1, P1, d_pad=1),                # dx_nstride % 4 != 0
    case("ft_hw8", 2, 3, (3, 2, 4), K333, S1, P1),                          # backward: 3x3x3 gather with S = 24
    case("ft_32x16", 1, 2, (2, 16, 32), K333, S1, P1),
    case("ft_w6", 2, 3, (4, 4, 6), K333, S1, P1, special=True),             # Wo % WPT != 0
    case("ft_w5_scalar", 2, 3, (3, 3, 5), K333, S1, P1, aff="relu"),        # Si = 45: 4-byte staging
    # ---- 3x3x3 / 1 / 1 on maps of 1 or 2 pixels: the tiled forward with G >= 2, the gather backward ----------------
    case("g333_s1", 3, 1367, (1, 1, 1), K333, S1, P1, x_extra=1, y_extra=2, d_extra=1),  # Mixed_5b/5c at 32x32
    case("g333_s2", 3, 1367, (1, 1, 2), K333, S1, P1, d_extra=1),
    case("g333_s2_t", 2, 5, (2, 1, 1), K333, S1, P1, d_extra=3),
    case("g333_s3", 3, 1367, (3, 1, 1), K333, S1, P1, x_extra=1, d_extra=1),
    case("g333_s6", 2, 5, (3, 1, 2), K333, S1, P1, d_extra=1),
    case("g333_s8", 2, 2049, (2, 2, 2), K333, S1, P1, d_extra=1),
    case("g333_s128", 2, 3, (8, 4, 4), K333, S1, P1, d_extra=1),
    case("g333_s128_odd", 2, 3, (8, 4, 4), K333, S1, P1, x_pad=3, d_pad=1), # S % 4 == 0, dy_nstride % 4 != 0
    # ---- tiled (1,3,3)/(1,2,2): time folded into the planes -----------------------------------------------------------
    case("t133_g1", 2, 3, (3, 9, 9), K133, S122, P011, aff="relu", pooled=True),         # Si = 81, Wo = 5
    case("t133_g4", 2, 1365, (3, 4, 4), K133, S122, P011, x_extra=1, y_extra=1, d_extra=1, aff="plain",
         pooled=True),                                                      # 8190 folded planes, T = 3
    case("t133_g2", 3, 455, (3, 8, 8), K133, S122, P011, x_extra=2, aff="relu"),         # 4095 folded planes
    case("t133_pooled_g4", 2, 683, (3, 4, 4), K133, S122, P011, aff="relu", pooled=True),
    case("t133_pooled_g2", 2, 1025, (1, 4, 4), K133, S122, P011, aff="plain", pooled=True),
    case("t133_128", 1, 2, (1, 128, 128), K133, S122, P011, aff="relu", pooled=True),    # Si == 16384: fits
    case("t133_pooled_odd_y", 2, 3, (2, 8, 8), K133, S122, P011, x_pad=1, aff="relu", pooled=True),
    case("t133_g2048", 5, 419021, (1, 1, 1), K133, S122, P011),      # 2095105 one-pixel planes: the largest G
    case("t133_112", 1, 2, (2, 112, 112), K133, S122, P011, aff="relu", pooled=True),    # kq = 4: generic classes
    # ---- tiled (3,3,3)/(2,2,2) ------------------------------------------------------------------------------------
    case("t333s2_g1", 2, 3, (5, 7, 9), K333, S222, P1, aff="plain", pooled=True),
    case("t333s2_g2", 3, 1367, (2, 4, 4), K333, S222, P1, x_extra=1, y_extra=1, d_extra=1),
    # ---- tiled (2,2,2)/(2,2,2) ------------------------------------------------------------------------------------
    case("t222_g1", 2, 3, (3, 3, 7), K222, S222, P0, special=True),                      # Si = 63, Wo = 3
    case("t222_g2", 3, 1367, (2, 4, 4), K222, S222, P0, x_extra=1, y_extra=1, d_extra=1, aff="relu", pooled=True),
    case("t222_vec", 2, 3, (4, 4, 6), K222, S222, P0, aff="plain", pooled=True),
    case("t222_pooled_odd_dy", 2, 3, (4, 4, 4), K222, S222, P0, d_pad=1, aff="plain", pooled=True),
    # ---- generic forward / gather backward ---------------------------------------------------------------------------
    case("gen_132x128", 1, 2, (1, 132, 128), K133, S122, P011, aff="relu"),              # Si = 16896 > 16384
    case("gen_unlisted", 2, 3, (3, 7, 7), K111, S122, P0, aff="plain", pooled=True),     # (1,1,1)/(1,2,2)
    case("gen_unlisted_kq2", 1, 2, (2, 40, 40), K111, S122, P0),
    case("gen_unlisted_kq4", 1, 2, (1, 56, 56), K111, S122, P0),
    case("gen_planes_65540", 2, 32770, (1, 2, 2), K111, S122, P0),
]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

MAX_ELEMS = 1 << 21


def elems(c):
    return c.N * c.C * c.idim[0] * c.idim[1] * c.idim[2]


def odim(c):
    return tuple((c.idim[i] + 2 * c.p[i] - c.k[i]) // c.s[i] + 1 for i in range(3))


def strides(c):
    """Sample strides (floats) of x, y and of the backward's dy / dx as the GPU test lays them out."""
    si = c.idim[0] * c.idim[1] * c.idim[2]
    o = odim(c)
    so = o[0] * o[1] * o[2]
    return dict(x=(c.C + c.x_extra) * si + c.x_pad, y=(c.C + c.y_extra) * so,
                dy=(c.C + c.d_extra) * so + c.d_pad, dx=(c.C + c.d_extra) * si + c.d_pad)


def geom(c):
    from coclr_amd import ops
    return ops.PoolGeom(c.N, c.C, c.idim, c.k, c.s, c.p)


def plan(c, with_indices=True):
    st = strides(c)
    return geom(c).plan(with_indices, x_nstride=st["x"], y_nstride=st["y"], dy_nstride=st["dy"],
                        dx_nstride=st["dx"])


def affine(c):
    """Per-channel (scale, shift) lists of the row's in-affine: +-2^k, both signs; small integers."""
    scale = [(-1.0 if ch % 3 == 1 else 1.0) * 2.0 ** ((ch % 4) - 2) for ch in range(c.C)]
    shift = [float((ch * 5) % 7 - 3) for ch in range(c.C)]
    return scale, shift


# every instantiation the launchers can select: (kernel, template, with indices) for the forward kernels ...
FWD_INSTANTIATIONS = ([("generic", None)] + [("sep333", tt, i) for tt in (0, 4, 8, 16) for i in (False, True)] +
                      [("tiled", t, i) for t in ((1, 3, 3, 1, 2, 2, 2), (3, 3, 3, 1, 1, 1, 4), (3, 3, 3, 2, 2, 2, 2),
                                                 (2, 2, 2, 2, 2, 2, 2)) for i in (False, True)])
BWD_INSTANTIATIONS = [("generic", None), ("gather333", None)] + [
    ("classes", t) for t in ((1, 2, 2, 1), (3, 3, 3, 1), (2, 2, 2, 1), (1, 1, 1, 2), (0, 0, 0, 0))]
POOLED_INSTANTIATIONS = [(1, 2, 2, 1), (2, 2, 2, 1), (0, 0, 0, 0)]
UNREACHABLE = {}     # instantiation -> excluding condition: nothing the launchers can select is out of reach
# edges no row of at most MAX_ELEMS input elements can reach, with the condition that excludes them
UNREACHABLE_EDGES = {
    "generic gather backward: pl += gridDim.y above 65535 planes":
        "the generic backward needs Si > 16384, and 65536 such planes hold 2^30 elements",
    "colour-class G = 4096 / Si at its cap for Si == 1":
        "G is halved while ceil(planes / G) < 1024: G = 4096 needs 1023 * 4096 + 1 planes, twice the limit; "
        "G = 2048 (1023 * 2048 + 1 = 2095105 one-pixel planes) is the largest and has a row",
}
