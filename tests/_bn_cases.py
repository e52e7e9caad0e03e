"""BatchNorm test rows: small units that reach every route and vector / scalar instantiation the launchers of
coclr_amd/csrc/bn.hip can select and every dispatch edge listed in tests/test_bn_plan_cpu.py.

Shared by the CPU-tier coverage test (tests/test_bn_plan_cpu.py: coclr_bn_plan says what each row reaches) and the
GPU test (tests/test_gpu_bn_exact.py: every row against float64).  No torch import here.

A row is one unit [N][C][T][H][W] plus the layout of its operands:
  z / dres    the backward is given z (the mask comes from it) / writes dres: a residual unit, always streaming
  pad         operands whose sample stride is one float longer (not a multiple of 4 even where C * S is)
  extra       operands that are channel slices of a buffer one channel wider
Operand names: y, z (forward output; the backward's z), dz, dy, dres (also the forward's residual).
"""
import collections

Case = collections.namedtuple("Case", "name N C dims z dres pad extra")


def case(name, N, C, dims, z=False, dres=False, pad=(), extra=()):
    return Case(name, N, C, tuple(dims), z, dres, tuple(pad), tuple(extra))


OPERANDS = ("y", "z", "dz", "dy", "dres")

CASES = [
    # ---- one workgroup per channel ------------------------------------------------------------------------------------
    case("one_vec", 2, 3, (2, 4, 4)),
    case("one_vec_slices", 3, 5, (2, 4, 4), extra=("y", "z", "dz", "dy")),
    case("one_scalar_s15", 2, 3, (1, 3, 5)),
    case("one_odd_y", 3, 2, (1, 4, 4), pad=("y",)),
    case("one_odd_z", 3, 2, (1, 4, 4), pad=("z",)),               # forward scalar; the backward has no z: vector
    case("one_odd_dz", 3, 2, (1, 4, 4), pad=("dz",)),
    case("one_odd_dy", 3, 2, (1, 4, 4), pad=("dy",)),
    case("one_tail", 3, 2, (5, 4, 281)),                          # N*S/4 = 4215: >= 4096, not a multiple of 1024
    case("edge_32768", 2, 2, (16, 32, 32)),                       # N*S == 32768: still one workgroup
    # ---- streaming ----------------------------------------------------------------------------------------------------
    case("edge_32772", 3, 2, (1, 2731, 4)),                       # N*S == 32772
    case("z_small", 2, 3, (2, 4, 4), z=True),
    case("dres_small", 2, 3, (2, 4, 4), dres=True),
    case("z_dres_slices", 3, 5, (2, 4, 4), z=True, dres=True, extra=OPERANDS),
    case("str_scalar_s15", 2, 3, (1, 3, 5), dres=True),
    case("str_odd_y", 3, 2, (1, 4, 4), z=True, pad=("y",)),
    case("str_odd_z", 3, 2, (1, 4, 4), z=True, pad=("z",)),
    case("str_odd_dz", 3, 2, (1, 4, 4), z=True, pad=("dz",)),
    case("str_odd_dy", 3, 2, (1, 4, 4), z=True, pad=("dy",)),
    case("str_odd_dres", 3, 2, (1, 4, 4), dres=True, pad=("dres",)),
    case("groups_n70", 70, 3, (1, 8, 8), dres=True),              # S = 64: 64 samples per group and a remainder
    case("groups_s4096", 3, 2, (4, 32, 32), z=True),              # S >= 4096: one group per sample
    case("large_stream", 9, 2, (4, 32, 32)),
    case("large_scalar", 3, 2, (1, 113, 97)),                     # S = 10961: streaming 4-byte passes, gx = 3
    case("grid_gx2", 5, 3, (1, 66, 100)),                         # S/4 = 1650: gx = 2, not a multiple of 1024 / 2048
]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

MAX_ELEMS = 1 << 21

# coclr_bn_finalize_apply_multi / coclr_bn_act_backward_multi: the units of one call, by row name
MULTI = {
    "five_small": ("one_vec", "one_vec_slices", "one_tail", "one_vec", "one_vec_slices"),     # runs of 4 + 1
    "vector_width_splits_a_run": ("one_vec", "one_tail", "one_scalar_s15", "one_odd_y", "one_vec"),
    "large_unit_inside": ("one_vec", "one_vec", "edge_32772", "one_vec", "one_vec"),
}
# backward only: units with partial sums (row, tile counts of the one or two arrays); None: no partials
MULTI_PARTIALS = {
    "part_inside": (("one_vec", None), ("one_vec_slices", None), ("one_vec", (3,)), ("one_vec", None),
                    ("one_tail", None)),
}
PARTIALS = {
    "part_small_3": ("one_vec", (3,)),
    "part_scalar_300": ("one_scalar_s15", (300,)),
    "part_two_300_7": ("grid_gx2", (300, 7)),
}
FINALIZE_NTILES = (1, 3, 300)


def S(c):
    return c.dims[0] * c.dims[1] * c.dims[2]


def elems(c):
    return c.N * c.C * S(c)


def strides(c):
    """Sample strides (floats) of every operand as the GPU test lays them out."""
    return {op: (c.C + (op in c.extra)) * S(c) + (op in c.pad) for op in OPERANDS}


def plan(c, partials=False):
    from coclr_amd import ops
    st = strides(c)
    return ops.bn_plan(c.N, c.C, S(c), y_nstride=st["y"], z_nstride=st["z"], dz_nstride=st["dz"],
                       dy_nstride=st["dy"], dres_nstride=st["dres"], has_z=c.z and not partials,
                       has_dres=c.dres and not partials, has_partials=partials)


def runs(names, partials=None):
    """How the multi launchers cut a call into launches, from their own run-cutting function (coclr_bn_multi_plan,
    nothing launched): a list of tuples of row names.  partials (backward): per unit, the tile counts or None."""
    from coclr_amd import ops
    units = []
    for i, n in enumerate(names):
        c = BY_NAME[n]
        st = strides(c)
        units.append(dict(N=c.N, C=c.C, S=S(c), y_nstride=st["y"], z_nstride=st["z"], dz_nstride=st["dz"],
                          dy_nstride=st["dy"], partials=partials is not None and partials[i] is not None))
    out, at = [], 0
    for length in ops.bn_multi_plan(units, backward=partials is not None):
        out.append(tuple(names[at:at + length]))
        at += length
    assert at == len(names)
    return out
