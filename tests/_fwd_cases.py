"""Small geometries that between them reach every forward / data-gradient kernel instantiation the launcher of
coclr_amd/csrc/conv_igemm.hip can select (conv3d_fwd_impl through select_forward), every pair route of
coclr_conv3d_fwd_multi and every dispatch edge listed in tests/test_fwd_plan_cpu.py.

Shared by the CPU-tier coverage test (tests/test_fwd_plan_cpu.py: ConvGeom.fwd_plan says what each row reaches)
and the exact-arithmetic GPU test (tests/test_gpu_fwd_exact.py: each row against float64).

A row is a convolution (N, Cin, Cout, dims, k, s, p, algo, odim) plus
  op        what is launched: "fwd" the convolution itself, "dgrad" its data gradient as ConvGeom.dgrad() poses it
            (a stride-1 correlation over dy, dilated when the convolution is strided), "phase0" / "phase1" one
            phase of ConvGeom.dgrad_phases() (a destination lattice along T);
  misalign  the row is there for the 4-byte twin of a 16-byte-staged kernel: x starts one float into its
            allocation (the plan is queried with x_aligned=False);
  env       environment switches the launcher reads per call (COCLR_WINO_W8).  COCLR_WINO_X16 and COCLR_CONV_XG
            are read ONCE per process into a static, so setting them per row would only act on the first launch
            of a test session: the rows that are there for the non-X16 / non-XG kernels reach them through what
            the predicates test instead -- x one float off alignment, or W % 4 != 0;
  xa, wa    alphabets: x holds integers in [-xa, xa], the weights G * integers in [-wa, wa] (G: granule of the
            form, see granule());
  slice_of  (full stencil, full padding, temporal tap) when the row is one kt-slice of a wider stencil.

Sizes.  Every row has at most 32768 output positions and channels no wider than its edge needs.  The rows that
reach the 128-wide tiles (variants 0, 1, 10, 11, 20, 21) sit AT that limit because choose_tile's cost model only
prefers those tiles from ~512 workgroups up: 256 boxes of 128 positions times 2-3 channel tiles (Cout 72 / 380).
The persistent-grid rows need their work-item count above the grid: `hw_grid*` 96 boxes x 3 channel tiles = 288 >
kWinoGrid = 256 (24576 positions), `stem_grid` 520 boxes > kStemGrid = 512 (32500 positions: every box overhangs
W and the last row of boxes overhangs H, or it would take 65664).
"""
import collections
import functools

Case = collections.namedtuple("Case", "name N Cin Cout dims k s p algo odim op misalign env xa wa slice_of")


def _c(name, N, Cin, Cout, dims, k, s, p, algo=0, odim=None, op="fwd", misalign=False, env=None, xa=2, wa=2,
       slice_of=None):
    return Case(name, N, Cin, Cout, dims, k, s, p, algo, odim, op, misalign, env or {}, xa, wa, slice_of)


P0, S1 = (0, 0, 0), (1, 1, 1)
K1, K133, K311, K411, K711, K177 = (1, 1, 1), (1, 3, 3), (3, 1, 1), (4, 1, 1), (7, 1, 1), (1, 7, 7)
PS, PT = (0, 1, 1), (1, 0, 0)
BIG = (8, 64, 64)
W8OFF = {"COCLR_WINO_W8": "0"}

_ROWS = [
    # ---- pointwise: variants 0 / 1 / 2 (choose_tile), 3 (strided or dilated) ---------------------------------
    _c("pw0_128x128", 1, 8, 380, BIG, K1, S1, P0, xa=1, wa=1),              # ragged 128-row tile, Cin <= CC
    _c("pw1_64x128", 1, 20, 72, BIG, K1, S1, P0, xa=1, wa=1),               # ragged 16-channel chunk
    _c("pw2_64x64", 3, 20, 24, (2, 4, 4), K1, S1, P0),                      # boxes of 2 samples, N = 3
    _c("pw2_cin8", 2, 8, 72, (3, 4, 4), K1, S1, P0),                        # one chunk; 48 positions: W overhang
    _c("pw3_strided", 3, 20, 24, (3, 5, 5), K1, (1, 2, 2), P0),
    _c("pw3_dilated", 3, 24, 20, (3, 5, 5), K1, (1, 2, 2), P0, op="dgrad"),  # dy zero-upsampled by the launcher
    _c("pw3_st2", 2, 8, 72, (5, 3, 3), K1, (2, 1, 1), P0),
    # ---- (1,3,3): variants 10 / 11 / 12, 13 (window > 256 floats) ---------------------------------------------
    _c("s10_128x128", 1, 8, 380, BIG, K133, S1, PS, xa=1, wa=1),
    _c("s11_64x128", 1, 20, 72, BIG, K133, S1, PS, xa=1, wa=1),
    _c("s12_xg", 3, 20, 24, (2, 4, 4), K133, S1, PS),
    _c("s12_odd", 2, 12, 72, (3, 7, 7), K133, S1, PS),                      # W % 4 != 0: 4-byte; W, H, T overhang
    _c("s12_cin8", 1, 8, 16, (1, 8, 8), K133, S1, PS),
    _c("s12_t3", 1, 12, 24, (3, 4, 4), K133, S1, PS),                       # 4 x 4 x 4 boxes over 3 frames
    _c("s12_dgrad", 2, 24, 20, (2, 6, 8), K133, S1, PS, op="dgrad"),
    _c("s13_xg", 1, 8, 16, (16, 1, 4), K133, S1, PS),                       # 6 x 3 x 16 window = 288 floats
    _c("s13_strided", 2, 20, 24, (2, 9, 9), K133, (1, 2, 2), PS),
    _c("s13_dilated", 2, 24, 20, (2, 9, 9), K133, (1, 2, 2), PS, op="dgrad"),
    # ---- (3,1,1) direct: 20 / 21 / 22; (4,1,1) direct: 25; (7,1,1): 40 ----------------------------------------
    _c("t20_128x128", 3, 8, 380, (2, 64, 64), K311, S1, PT, xa=1, wa=1),
    _c("t21_64x128", 3, 20, 72, (2, 64, 64), K311, S1, PT, xa=1, wa=1),
    _c("t22_xv4", 3, 20, 24, (3, 2, 2), K311, S1, PT),                      # boxes of 4 samples, N = 3
    _c("t22_odd", 2, 12, 72, (5, 3, 3), K311, S1, PT),                      # 9 positions per frame: 4-byte
    _c("t22_cin8", 1, 8, 16, (4, 4, 4), K311, S1, PT),
    _c("t22_dgrad_st2", 2, 20, 24, (7, 2, 2), K311, (2, 1, 1), PT, op="dgrad"),   # dilated along T
    _c("t22_phase0", 1, 24, 20, (8, 2, 2), K711, (2, 1, 1), (3, 0, 0), op="phase0"),   # direct, T lattice
    _c("t25_dense", 1, 20, 24, (6, 2, 2), K411, S1, PT, odim=(6, 2, 2)),
    _c("t25_phase1", 1, 24, 20, (8, 2, 2), K711, (2, 1, 1), (3, 0, 0), op="phase1"),
    _c("t25_phase1_odd", 2, 24, 20, (9, 3, 3), K711, (2, 1, 1), (3, 0, 0), op="phase1"),
    _c("t40_xv4", 1, 8, 16, (8, 4, 4), K711, (2, 1, 1), (3, 0, 0)),
    _c("t40_odd", 3, 20, 72, (5, 3, 3), K711, (2, 1, 1), (3, 0, 0)),
    _c("t40_dgrad", 1, 20, 24, (6, 2, 2), K711, (2, 1, 1), (3, 0, 0), op="dgrad"),
    # ---- F(2,3) along T: 50 ---------------------------------------------------------------------------------
    _c("w50_odd_frames", 3, 20, 24, (5, 2, 2), K311, S1, PT, algo=1),
    _c("w50_cin8x", 1, 16, 72, (3, 4, 4), K311, S1, PT, algo=1),
    _c("w50_dgrad", 2, 24, 20, (4, 2, 4), K311, S1, PT, algo=1, op="dgrad"),
    _c("w50_odd_plane", 2, 16, 24, (4, 3, 3), K311, S1, PT, algo=1),        # 9 positions per frame: 4-byte
    # ---- F(4,3) along T: 51, dense and on a T lattice ------------------------------------------------------------
    _c("w51_t5", 3, 20, 24, (5, 2, 2), K311, S1, PT, algo=2),
    _c("w51_t6", 1, 16, 72, (6, 4, 4), K311, S1, PT, algo=2),
    _c("w51_t7", 2, 20, 24, (7, 2, 4), K311, S1, PT, algo=2),
    _c("w51_t7_odd_plane", 2, 20, 24, (7, 3, 3), K311, S1, PT, algo=2),
    _c("w51_dgrad", 2, 24, 20, (9, 2, 2), K311, S1, PT, algo=2, op="dgrad"),
    _c("w51_phase0_t32", 1, 24, 20, (32, 2, 2), K711, (2, 1, 1), (3, 0, 0), op="phase0"),
    _c("w51_phase0_t34", 3, 24, 20, (34, 2, 2), K711, (2, 1, 1), (3, 0, 0), op="phase0"),    # 17 frames
    _c("w51_phase0_t38_odd", 1, 24, 20, (38, 3, 3), K711, (2, 1, 1), (3, 0, 0), op="phase0"),  # 19 frames, 4-byte
    # ---- F(2,4) along T: 52, dense and on a T lattice ------------------------------------------------------------
    _c("w52_dense_odd", 3, 20, 24, (5, 2, 2), K411, S1, PT, algo=2, odim=(5, 2, 2)),
    _c("w52_dense_odd_plane", 1, 16, 72, (7, 3, 3), K411, S1, PT, algo=2, odim=(7, 3, 3)),
    _c("w52_phase1_t32", 1, 24, 20, (32, 2, 2), K711, (2, 1, 1), (3, 0, 0), op="phase1"),
    _c("w52_phase1_t34", 3, 24, 20, (34, 2, 2), K711, (2, 1, 1), (3, 0, 0), op="phase1"),    # 17 frames
    _c("w52_phase1_t38_odd", 1, 24, 20, (38, 3, 3), K711, (2, 1, 1), (3, 0, 0), op="phase1"),
    # ---- polyphase (7,1,1)/2: 41 ---------------------------------------------------------------------------------
    _c("w41_t16", 1, 20, 24, (16, 2, 2), K711, (2, 1, 1), (3, 0, 0), algo=1),
    _c("w41_t20_odd_pairs", 3, 16, 72, (20, 2, 2), K711, (2, 1, 1), (3, 0, 0), algo=1),     # 5 output pairs
    _c("w41_odd_plane", 2, 20, 24, (18, 3, 3), K711, (2, 1, 1), (3, 0, 0), algo=1),         # 9 output frames
    # ---- F(2x2,3x3): 60 ------------------------------------------------------------------------------------------
    _c("hw8", 3, 24, 72, (1, 12, 8), K133, S1, PS, algo=1),
    _c("hw8_dgrad", 1, 24, 72, (3, 4, 12), K133, S1, PS, algo=1, op="dgrad"),
    _c("hw_x16_cin20", 1, 20, 24, (2, 8, 8), K133, S1, PS, algo=1),         # Cin % 8: the two-wave kernel refuses
    _c("hw_x16_w8off", 3, 24, 72, (1, 12, 8), K133, S1, PS, algo=1, env=W8OFF),
    _c("hw_pch6_mis", 1, 20, 24, (2, 6, 20), K133, S1, PS, algo=1, misalign=True),   # 8 x 22 window, 4-byte staged
    _c("hw_pch10_w6", 2, 20, 24, (1, 6, 6), K133, S1, PS, algo=1),          # W % 4 != 0; boxes of 4 samples
    _c("hw_pch10_mis", 3, 24, 72, (1, 12, 8), K133, S1, PS, algo=1, misalign=True),
    _c("hw_pch10", 1, 20, 24, (3, 4, 4), K133, S1, PS, algo=1),             # boxes of 4 frames x 4 samples
    _c("hw8_grid", 1, 16, 130, (6, 64, 64), K133, S1, PS, algo=1, xa=1, wa=1),
    _c("hw_grid", 1, 20, 130, (6, 64, 64), K133, S1, PS, algo=1, xa=1, wa=1),
    # ---- (1,7,7): 31 (persistent stem kernel, Cin = 3), 30 -------------------------------------------------------
    _c("stem", 3, 3, 24, (1, 8, 20), K177, (1, 2, 2), (0, 3, 3)),           # boxes of 2 samples, N = 3
    _c("stem_cout72", 1, 3, 72, (2, 12, 20), K177, (1, 2, 2), (0, 3, 3)),
    _c("stem_grid", 1, 3, 8, (20, 50, 130), K177, (1, 2, 2), (0, 3, 3), xa=1, wa=1),
    # temporal tap 3 of r50's (5,7,7)/(1,2,2) pad (2,3,3) stem, as the engine slices it: pad_t = 2 - 3
    _c("stem_slice_kt3", 2, 3, 40, (4, 12, 20), K177, (1, 2, 2), (-1, 3, 3), odim=(4, 6, 10),
       slice_of=((5, 7, 7), (2, 3, 3), 3)),
    _c("stem_small", 1, 3, 24, (3, 10, 16), K177, (1, 2, 2), (0, 3, 3)),    # 8 x 8 x 2 boxes over 8 x 5 x 3 outputs
    _c("stem30_cin4", 3, 4, 24, (1, 8, 20), K177, (1, 2, 2), (0, 3, 3)),
    _c("stem30_small", 1, 4, 24, (3, 10, 16), K177, (1, 2, 2), (0, 3, 3)),
    _c("stem30_dgrad", 1, 24, 3, (1, 8, 12), K177, (1, 2, 2), (0, 3, 3), op="dgrad"),
]

# the rows that get a 4-byte twin `<name>_4b`: same geometry and data, x one float into its allocation.  The list
# is explicit; tests/test_fwd_plan_cpu.py asserts that each base row is 16-byte staged and its twin is not.
TWINS = ["pw0_128x128", "pw1_64x128", "pw2_64x64", "s10_128x128", "s11_64x128", "s12_xg", "s13_xg",
         "t20_128x128", "t21_64x128", "t22_xv4", "t25_dense", "t25_phase1", "t40_xv4", "t22_phase0",
         "w50_odd_frames", "w51_t5", "w51_phase0_t32", "w52_dense_odd", "w52_phase1_t32", "w41_t16"]

CASES = list(_ROWS)
for _n in TWINS:
    _b = next(c for c in _ROWS if c.name == _n)
    CASES.append(_b._replace(name=_n + "_4b", misalign=True))

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def base_name(case):
    """Rows that share their data: a `_4b` twin runs the problem of its base row."""
    return case.name[:-3] if case.name.endswith("_4b") and case.name[:-3] in BY_NAME else case.name


# ---- geometry ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _geoms(name):
    from coclr_amd import ops
    c = BY_NAME[name]
    g = ops.ConvGeom(c.N, c.Cin, c.Cout, c.dims, c.k, c.s, c.p, odim=c.odim, algo=c.algo)
    if c.op == "fwd":
        return g, g, None
    if c.op == "dgrad":
        return g, g.dgrad(), None
    phases = g.dgrad_phases()
    assert phases is not None, name
    pg, k0, nk, step = phases[int(c.op[-1])]
    return g, pg, (k0, nk, step)


def conv_geom(case):
    """The convolution the row is about."""
    return _geoms(case.name)[0]


def launch_geom(case):
    """The geometry handed to conv_fwd: the convolution, its dgrad() or one of its dgrad_phases()."""
    return _geoms(case.name)[1]


def phase(case):
    """(tap_base, taps, tap_step) of a phase row, None otherwise."""
    return _geoms(case.name)[2]


def positions(case):
    g = launch_geom(case)
    return g.N * g.odim[0] * g.odim[1] * g.odim[2]


def plan(case, **kw):
    kw.setdefault("x_aligned", not case.misalign)
    return launch_geom(case).fwd_plan(**kw)


INST_FIELDS = ("variant", "family", "form", "KT", "KH", "KW", "CC", "BM", "BN", "PCH", "OCC", "XV4", "XG", "X16",
               "INAFF", "lattice")


def instantiation(pl):
    """A destination lattice is a run-time mapping in the direct kernels; only variants 51 / 52 take other fields
    under it, so only there is it part of what a row reaches."""
    t = tuple(pl[f] for f in INST_FIELDS)
    return t if pl["variant"] in (51, 52) else t[:-1] + (False,)


def _i(variant, family, form, k, cc, bm, bn, pch, occ=0, xv4=False, xg=False, x16=False, inaff=False, lat=False):
    return (variant, family, form) + tuple(k) + (cc, bm, bn, pch, occ, xv4, xg, x16, inaff, lat)


# every <variant, family, form, KT KH KW CC BM BN PCH OCC, XV4 XG X16 INAFF lattice> the kernel table of
# conv_igemm.hip (kFwdTable: one row per variant and staging form) holds.
# A lattice does not change the kernel of the direct forms (it is a run-time destination mapping there), so it is
# listed only for variants 51 / 52, whose kernels read the frame count and pitch from other fields under it.
INSTANTIATIONS = (
    [_i(0, "igemm", 0, K1, 32, 128, 128, 2, xv4=v) for v in (True, False)] +
    [_i(1, "igemm", 0, K1, 16, 64, 128, 2, xv4=True), _i(1, "igemm", 0, K1, 32, 64, 128, 2)] +
    [_i(2, "igemm", 0, K1, 16, 64, 64, 1, xv4=True), _i(2, "igemm", 0, K1, 32, 64, 64, 1)] +
    [_i(3, "igemm", 0, K1, 16, 64, 64, 4)] +
    [_i(10, "igemm", 0, K133, 4, 128, 128, 3, xg=True), _i(10, "igemm", 0, K133, 4, 128, 128, 4)] +
    [_i(11, "igemm", 0, K133, 8, 64, 128, 3, xg=True), _i(11, "igemm", 0, K133, 8, 64, 128, 4)] +
    [_i(12, "igemm", 0, K133, 8, 64, 64, 3, xg=True), _i(12, "igemm", 0, K133, 8, 64, 64, 4)] +
    [_i(13, "igemm", 0, K133, 8, 64, 64, 3, xg=True), _i(13, "igemm", 0, K133, 8, 64, 64, 8)] +
    [_i(20, "igemm", 0, K311, 4, 128, 128, 4, xv4=v) for v in (True, False)] +
    [_i(21, "igemm", 0, K311, 8, 64, 128, 4, xv4=v) for v in (True, False)] +
    [_i(22, "igemm", 0, K311, 8, 64, 64, 4, xv4=v) for v in (True, False)] +
    [_i(25, "igemm", 0, K411, 8, 64, 128, 4, xv4=v) for v in (True, False)] +
    [_i(50, "wino_t", 0, K311, 8, 64, 64, 4, 4, xv4=True), _i(50, "wino_t", 0, K311, 16, 64, 64, 4, 1)] +
    [_i(51, "wino_tf", 6, K311, 8, 64, 64, 6, 3, xv4=v, lat=l) for v in (True, False) for l in (False, True)] +
    [_i(52, "wino_tf", 5, K411, 8, 64, 64, 4, 3, xv4=v, lat=l) for v in (True, False) for l in (False, True)] +
    [_i(60, "wino_hw8", 0, K133, 8, 64, 64, 3, x16=True), _i(60, "wino_hw", 0, K133, 8, 64, 64, 3, x16=True),
     _i(60, "wino_hw", 0, K133, 8, 64, 64, 6), _i(60, "wino_hw", 0, K133, 8, 64, 64, 10)] +
    [_i(30, "igemm", 0, K177, 4, 64, 128, 20), _i(31, "stem", 0, K177, 3, 64, 128, 20)] +
    [_i(41, "wino_tf", 9, K711, 8, 64, 64, 6, 2, xv4=v, inaff=a) for v in (True, False) for a in (False, True)] +
    [_i(40, "igemm", 0, K711, 4, 64, 128, 8, xv4=True), _i(40, "igemm", 0, K711, 8, 64, 128, 8)])

# instantiations no accepted geometry reaches, with the planner condition that excludes them
UNREACHABLE = {}

# ---- pair routes of coclr_conv3d_fwd_multi: (rows, route) -----------------------------------------------------------
# route: "pair" one two-problem launch of the rows' common kernel, "mixed" conv_igemm_133_mixed_kernel, "singles" two
# launches, "odd" a trailing third call
PAIRS = [
    (("s12_xg", "s12_xg"), "pair"),                     # (1,3,3) family, same kernel, equal LDS
    (("s12_xg", "s12_cin8"), "pair-lds"),               # same kernel, two LDS stages vs one: sizes differ
    (("pw2_64x64", "pw2_cin8"), "pair-lds"),            # 16-byte pointwise, two chunks vs one
    (("w50_odd_frames", "w50_cin8x"), "pair"),          # F(2,3), 16-byte
    (("w51_t5", "w51_t6"), "pair"),                     # F(4,3), 16-byte, dense
    (("s11_64x128", "s12_xg"), "mixed"),                # 64 x 128 then 64 x 64
    (("s12_xg", "s11_64x128"), "mixed"),
    (("s12_xg", "t22_xv4"), "singles"),                 # a pairable kernel next to one without a pair form
    (("s12_xg", "s12_odd"), "singles"),                 # both pairable, different kernels, no mixed form
    (("s12_xg", "s12_xg", "pw2_64x64"), "odd"),
]


# ---- data: alphabets, granules, host-side packing, float64 reference ---------------------------------------------

def granule(case):
    """Weights are G * small integers so that every transformed operand of the row's form is an integer."""
    g = launch_geom(case)
    if g.algo == 0:
        return 1
    if g.k == (1, 3, 3):
        return 4
    if g.k == (3, 1, 1):
        return 2 if g.algo == 1 else 24
    return 6            # F(2,4) of a (4,1,1) stencil, polyphase form of the (7,1,1) one


def _integers(gen, shape, amax):
    import torch
    return torch.randint(-amax, amax + 1, shape, generator=gen).double()


def _pad_back(c, i, k, p):
    """Padding behind axis i that an explicit odim implies."""
    g = conv_geom(c)
    return (g.odim[i] - 1) * c.s[i] + k[i] - c.dims[i] - p[i]


@functools.lru_cache(maxsize=None)
def problem(name, kind="int"):
    """(operand, w, ref) on the CPU in float64.  operand: what the launch reads (x, or dy for a data gradient);
    w: the FULL parameter [Cout][Cin][stencil] (the full stencil of a kt-slice row); ref: what the launch must
    produce, dense in launch_geom().odim (a phase row: its residue class of dx), from F.conv3d (+ autograd)."""
    import torch
    import torch.nn.functional as F
    c = BY_NAME[name]
    assert base_name(c) == name
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 11 + len(kind))
    k, p, t = (c.k, c.p, None) if c.slice_of is None else c.slice_of
    G = granule(c)

    def draw(shape, amax):
        if kind == "int":
            return _integers(gen, shape, amax)
        return torch.randn(shape, generator=gen).double()

    x = draw((c.N, c.Cin) + tuple(c.dims), c.xa)
    w = (_integers(gen, (c.Cout, c.Cin) + tuple(k), c.wa) * G) if kind == "int" else \
        torch.randn((c.Cout, c.Cin) + tuple(k), generator=gen).double() * 0.05
    weff = w
    if t is not None:
        weff = torch.zeros_like(w)
        weff[:, :, t] = w[:, :, t]
    ph = phase(c)
    if ph is not None:
        k0, nk, step = ph
        weff = torch.zeros_like(w)
        weff[:, :, k0::step] = w[:, :, k0::step]
    back = [_pad_back(c, i, k, p) for i in range(3)]

    def conv(xx):
        # explicit padding: an explicit odim may ask for more (or less) behind than in front, and p may be negative
        pads = []
        for i in (2, 1, 0):
            pads += [p[i], back[i]]
        return F.conv3d(F.pad(xx, pads), weff, None, c.s, 0)

    if c.op == "fwd":
        ref = conv(x)
        assert tuple(ref.shape[2:]) == conv_geom(c).odim, (name, ref.shape)
        return x, w, ref
    xr = x.clone().requires_grad_(True)
    y = conv(xr)
    dy = draw(tuple(y.shape), c.xa)
    y.backward(dy)
    ref = xr.grad
    if ph is not None:
        lat = launch_geom(c).lattice
        ref = ref[:, :, lat[1][0]::lat[0][0]].contiguous()
    return dy, w, ref


_F23 = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
_F43 = [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
        [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]
_F24 = [[.5, 0, 0, 0], [-.5, -.5, -.5, -.5], [-1 / 6, 1 / 6, -1 / 6, 1 / 6], [1 / 6, 2 / 6, 4 / 6, 8 / 6], [0, 0, 0, 1]]
_POLY7 = [[0, 1, 0, 0, 0, 0, 0], [0, .5, 0, .5, 0, .5, 0], [0, .5, 0, -.5, 0, .5, 0], [0, 0, 0, 0, 0, 1, 0],
          [.5, 0, 0, 0, 0, 0, 0], [-.5, 0, -.5, 0, -.5, 0, -.5], [-1 / 6, 0, 1 / 6, 0, -1 / 6, 0, 1 / 6],
          [1 / 6, 0, 2 / 6, 0, 4 / 6, 0, 8 / 6], [0, 0, 0, 0, 0, 0, 1]]
SOURCE_TAPS = {4: 3, 5: 4, 6: 3, 9: 7, 16: 9}


def host_pack(w, taps, tap_base=0, tap_step=1, transpose=False, wino=False, row0=0, rows_total=0, col0=0,
              cols_total=0, into=None):
    """The packed operand of coclr_conv_pack_weights in float64, in its documented layout
    (include/coclr_hip.h): dst[(tap * RP + r) * CP + c] with r the reduction channel (Cin forward, Cout for the
    data gradient, whose stencil is flipped), RP / CP padded to 32 / 128; the 16-matrix form
    dst[(r * CP + c) * 16 + xi'] with the quads of xi rotated by c >> 2.  w: [Cout][Cin][...stencil]."""
    import torch
    cout, cin = w.shape[:2]
    w = w.reshape(cout, cin, -1).double()
    nsrc = SOURCE_TAPS[taps] if wino else taps
    g = w[:, :, tap_base:tap_base + (nsrc - 1) * tap_step + 1:tap_step]
    assert g.shape[2] == nsrc
    if transpose:
        g = g.flip(-1)
    if not wino:
        U = g
    elif taps == 16:
        A = torch.tensor(_F23, dtype=torch.float64)
        U = torch.einsum("ia,ocab,jb->ocij", A, g.reshape(cout, cin, 3, 3), A).reshape(cout, cin, 16)
    else:
        A = torch.tensor({4: _F23, 5: _F24, 6: _F43, 9: _POLY7}[taps], dtype=torch.float64)
        U = torch.einsum("ta,oca->oct", A, g)
    M = U.permute(2, 0, 1) if transpose else U.permute(2, 1, 0)      # [tap][r][c]
    r, cc = M.shape[1:]
    placed = rows_total > 0 and cols_total > 0
    RP = -(-(rows_total if placed else r) // 32) * 32
    CP = -(-(cols_total if placed else cc) // 128) * 128
    if into is None:
        into = torch.zeros(taps * RP * CP, dtype=torch.float64)
    if wino and taps == 16:
        out = into.view(RP, CP, 16)
        col = torch.arange(cc)
        for tap in range(16):
            xi = ((((tap >> 2) + (col >> 2)) & 3) << 2) + (tap & 3)
            out[:r, col, xi] = M[tap]
    else:
        out = into.view(taps, RP, CP)
        out[:, row0:row0 + r, col0:col0 + cc] = M
    return into


def pack_args(case):
    """(taps, tap_base, tap_step, transpose, wino, stencil taps of the full parameter) of the row's operand, as
    engine.Run.pack chooses them."""
    g = launch_geom(case)
    k = case.k if case.slice_of is None else case.slice_of[0]
    full = k[0] * k[1] * k[2]
    transpose = case.op != "fwd"
    ph = phase(case)
    if ph is not None:
        k0, nk, step = ph
        return ({3: 6, 4: 5}[nk] if g.algo >= 1 else nk), k0, step, transpose, g.algo >= 1, full
    if g.algo >= 1:
        vt = {(3, 1, 1): 6 if g.algo == 2 else 4, (4, 1, 1): 5, (7, 1, 1): 9, (1, 3, 3): 16}[g.k]
        return vt, 0, 1, transpose, True, full
    if case.slice_of is not None:
        per = case.k[0] * case.k[1] * case.k[2]
        return per, case.slice_of[2] * per, 1, transpose, False, full
    return full, 0, 1, transpose, False, full


@functools.lru_cache(maxsize=None)
def bwd_operands(name, relu):
    """Dyadic operands of the backward-sums epilogue (coclr_conv_call.bwd_y) for a row, on the CPU in float64 and
    dense in launch_geom().odim: (by, scale, shift, mean, invstd, g, xhat) with g = relu ? (by * scale + shift > 0
    ? dz : 0) : dz and xhat = (by - mean) * invstd.  by holds integers in [-4, 4], xhat multiples of 1/2 of
    magnitude <= 12, and by * scale + shift is never zero."""
    import torch
    x, w, ref = problem(name)
    gen = torch.Generator().manual_seed(31 + sum(map(ord, name)))
    Cout = ref.shape[1]
    pick = lambda vals: torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), (Cout,), generator=gen)]
    by = torch.randint(-4, 5, ref.shape, generator=gen).double()
    scale, shift = pick([1.0, -1.0, 0.5]), pick([0.25, -1.25, 2.75])
    mean, invstd = pick([0.0, 1.0, -2.0]), pick([0.5, 1.0, 2.0])
    b = lambda v: v.view(1, -1, 1, 1, 1)
    pre = by * b(scale) + b(shift)
    assert bool((pre != 0).all())
    g = ref * (pre > 0) if relu else ref
    xhat = (by - b(mean)) * b(invstd)
    return by, scale, shift, mean, invstd, g, xhat
