"""CPU tier for the weight-gradient dispatch: coclr_conv3d_wgrad_plan (the launcher's own planner and kernel
selection, nothing launched) says what every row of tests/_wgrad_cases.py reaches, and this module asserts that
the table covers

  * every kernel instantiation the launcher can select, except those listed as UNREACHABLE with the planner
    condition that excludes them (and none of those is reached);
  * every dispatch edge in EDGES below.

tests/test_gpu_wgrad_exact.py runs the same rows against float64, so a row that is the only cover of an
instantiation or edge cannot be dropped without this module failing.  Also here: the argument refusals of
coclr_conv3d_wgrad_multi, which are host-side and need no GPU.
"""
import ctypes as C

import pytest

import _wgrad_cases as W
from coclr_amd import _lib, ops


def _plans():
    out = []
    for c in W.CASES:
        g = W.geom(c)
        out.append((c, g, g.wgrad_plan(True), g.wgrad_plan(False)))
    return out


PLANS = _plans()


def test_rows_are_small():
    for c, g, pl, _ in PLANS:
        assert c.N * g.odim[0] * g.odim[1] * g.odim[2] <= 32768, c.name


def test_plan_agrees_with_the_other_queries():
    """The query and the entry points that already existed answer from the same plan."""
    for c, g, pl, pu in PLANS:
        assert g.wgrad_workspace() == pl["split"] * pl["slices"] * c.Cout * c.Cin * g.taps, c.name
        assert g.wgrad_bn_ok() == pl["bn"], c.name
        assert pl["slices"] == {"stem": 4, "wino7": 2}.get(W.family(pl), 1), c.name
        assert pl["lTW"] + pl["lTH"] + pl["lTT"] + pl["lTN"] in (5, 6, 7), c.name
        # alignment only ever decides between the 16-byte-DMA pointwise kernel and ids 4 / 5
        if pu != pl:
            assert pl["family"] == "pwdma" and pu["family"] == "wave" and pu["id"] == pl["id"], c.name
            assert {k: v for k, v in pl.items() if k not in ("family", "pch")} == \
                   {k: v for k, v in pu.items() if k not in ("family", "pch")}, c.name
    d = _lib.ConvDesc.from_buffer_copy(PLANS[0][1].desc)
    out = (C.c_int32 * 16)()
    lib = _lib.load()
    assert lib.coclr_conv3d_wgrad_plan(None, 1, out) == 1
    assert lib.coclr_conv3d_wgrad_plan(C.byref(d), 1, None) == 1
    d.dt = 2
    assert lib.coclr_conv3d_wgrad_plan(C.byref(d), 1, out) == 1


def _reached():
    reached = {}
    for c, g, pl, pu in PLANS:
        for p in (pl, pu):
            names = reached.setdefault(W.instantiation(p), [])
            if c.name not in names:
                names.append(c.name)
            if p["bn"]:
                names = reached.setdefault(("stem+bn",) + W.instantiation(p)[1:], [])
                if c.name not in names:
                    names.append(c.name)
    return reached


def test_table_reaches_every_instantiation():
    reached = _reached()
    print("\ninstantiation <family, id, PCH, BJ> -> rows")
    for inst in W.INSTANTIATIONS:
        print("  %-24s %s" % (inst, ", ".join(reached.get(inst, [])) or "-"))
    print("UNREACHABLE")
    for inst, why in W.UNREACHABLE.items():
        print("  %-24s %s" % (inst, why))
    assert set(reached) <= set(W.INSTANTIATIONS), set(reached) - set(W.INSTANTIATIONS)
    assert set(W.UNREACHABLE) <= set(W.INSTANTIATIONS)
    for inst in W.INSTANTIATIONS:
        if inst in W.UNREACHABLE:
            assert inst not in reached, "%s is listed as unreachable but %s reach it" % (inst, reached[inst])
        else:
            assert reached.get(inst), "no row of the table reaches %s" % (inst,)


def _per_family(pred):
    """{family: rows} of the rows (with the plan of either alignment) that satisfy pred(case, geom, plan)."""
    hit = {}
    for c, g, pl, pu in PLANS:
        for p in (pl, pu):
            if pred(c, g, p) and c.name not in hit.setdefault(W.family(p), []):
                hit[W.family(p)].append(c.name)
    return hit


def _overhang(axis):
    def pred(c, g, p):
        return W.planned_extents(c, p)[axis] % (1 << p[("lTW", "lTH", "lTT")[axis]]) != 0
    return pred


def _grid(p):
    return p["split"] * p["ct"] * p["mt"]


def _stencil(c):
    return c.k != (1, 1, 1)


# name -> (predicate, families that must each have a row; None: one row anywhere is enough)
EDGES = {
    "ragged Cout tile": (lambda c, g, p: c.Cout % (32 if W.family(p) == "wino7" else 64) != 0 and
                         c.Cout % 64 != 0, W.FAMILIES),
    "ragged Cin tile": (lambda c, g, p: c.Cin % 64 != 0, W.FAMILIES),
    "stencil with Cin < 48": (lambda c, g, p: _stencil(c) and c.Cin < 48 <= c.Cout and c.Cin != 3, ("gen1",)),
    "stencil with Cout < 48": (lambda c, g, p: _stencil(c) and c.Cout < 48 <= c.Cin, ("gen1",)),
    "Cin < 8": (lambda c, g, p: c.Cin < 8 and c.k != (1, 7, 7), ("gen1",)),
    "phantom sample in the last box": (lambda c, g, p: p["lTN"] > 0 and c.N % (1 << p["lTN"]) != 0,
                                       ("gen1", "wave_direct", "wino6", "wino7", "stem")),
    "overhang along W": (_overhang(0), None),
    "overhang along H": (_overhang(1), None),
    "overhang along T": (_overhang(2), None),
    "odd frame count in the F(2,3) form": (lambda c, g, p: g.odim[0] % 2 == 1, ("wino6",)),
    "F(2x2,3x3) re-boxed 34x4 -> 18x6": (lambda c, g, p: p["rebox"], ("wino7",)),
    "F(2x2,3x3) not re-boxed": (lambda c, g, p: not p["rebox"], ("wino7",)),
    "split does not divide ntiles": (lambda c, g, p: p["ntiles"] % p["split"] != 0, None),
    "fold of 1 slice": (lambda c, g, p: p["split"] * p["slices"] == 1, None),
    "fold of 2-3 slices": (lambda c, g, p: 2 <= p["split"] * p["slices"] <= 3, None),
    "fold of 4-15 slices": (lambda c, g, p: 4 <= p["split"] * p["slices"] <= 15, None),
    "fold of >= 16 slices, not a multiple of 16": (lambda c, g, p: p["split"] * p["slices"] >= 16 and
                                                   (p["split"] * p["slices"]) % 16 != 0, None),
    "split >= 16 (rounded to the XCD count)": (lambda c, g, p: p["split"] >= 16 and p["split"] % 8 == 0,
                                               ("gen1", "wave_direct", "pwdma")),
    # only these families have a tile-fastest order (the GPU test forces it with COCLR_WGRAD_ORDER=tile)
    "tile-fastest remap tail: grid % 8 != 0, grid > 8": (lambda c, g, p: _grid(p) > 8 and _grid(p) % 8 != 0,
                                                         ("wino7",)),
    "tile-fastest with fewer than 8 workgroups": (lambda c, g, p: _grid(p) < 8,
                                                  ("wave_direct", "wino6", "wino7", "pwdma")),
    "tile-fastest by the default rule": (lambda c, g, p: p["tile_order"], ("pwdma",)),
    "fold's grid-stride loop": (lambda c, g, p: c.Cout * c.Cin * g.taps > 8192 * 64, None),
    "strided (1,3,3)/(1,2,2)": (lambda c, g, p: c.k == (1, 3, 3) and c.s == (1, 2, 2), None),
    "strided (7,1,1)/(2,1,1)": (lambda c, g, p: c.k == (7, 1, 1) and c.s == (2, 1, 1), ("gen1", "wave_direct")),
    "(1,7,7) kt-slice of a (5,7,7) stem, tap_base > 0, shifted padding":
        (lambda c, g, p: c.slice_of is not None and c.slice_of[0] == (5, 7, 7) and c.slice_of[2] > 0 and
         c.p[0] == c.slice_of[1][0] - c.slice_of[2], ("stem",)),
    "pointwise eligible for the 16-byte DMA": (lambda c, g, p: p["family"] == "pwdma", ("pwdma",)),
    "pointwise not eligible: Wi % 64 != 0": (lambda c, g, p: c.k == (1, 1, 1) and c.s == (1, 1, 1) and
                                             c.Cin >= 8 and W.planned_extents(c, p)[0] % 64 != 0 and
                                             g.wgrad_plan(True)["family"] == "wave", ("wave_direct",)),
}


@pytest.mark.parametrize("edge", list(EDGES))
def test_table_hits_edge(edge):
    pred, families = EDGES[edge]
    hit = _per_family(pred)
    print("\n%s: %s" % (edge, hit))
    if families is None:
        assert hit, "no row hits: %s" % edge
    else:
        for f in families:
            assert hit.get(f), "no %s row hits: %s" % (f, edge)


def test_both_pointwise_dma_kernels_have_an_unaligned_fallback_row():
    """The rows the GPU test runs at an odd channel offset: eligible by shape, ids 4 / 5 when a pointer is not
    16-byte aligned."""
    ids = {pl["id"] for c, g, pl, pu in PLANS if pl["family"] == "pwdma" and pu["family"] == "wave"}
    assert ids == {4, 5}


def test_multi_destination_argument_refusals():
    """coclr_conv3d_wgrad_multi validates on the host, before anything is launched: COCLR_EINVAL (1) without a
    GPU.  (A call that got as far as a launch here would report the missing device, not 1.)"""
    lib = _lib.load()
    g = ops.ConvGeom(2, 72, 100, (2, 5, 5), (1, 1, 1), (1, 1, 1), (0, 0, 0))
    d = _lib.ConvDesc.from_buffer_copy(g.desc)
    d.x_nstride, d.y_nstride = 72 * 50, 100 * 50
    p = C.c_void_p(4096)

    def call(ptrs, ends, nseg, desc=d):
        arr = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        end = (C.c_int32 * max(len(ends), 1))(*ends)
        return lib.coclr_conv3d_wgrad_multi(C.byref(desc), p, p, arr, end, nseg, p, 72, 1, 0, 0, None)

    v = p.value
    assert call([v], [100], 0) == 1                                       # nseg 0
    assert call([v] * 5, [10, 20, 30, 40, 100], 5) == 1                   # nseg 5
    assert call([v, None, v], [17, 64, 100], 3) == 1                      # a null destination
    assert call([v, v, v], [17, 17, 100], 3) == 1                         # row_end not strictly increasing
    assert call([v, v, v], [64, 17, 100], 3) == 1
    assert call([v, v], [0, 100], 2) == 1                                 # an empty first segment
    assert call([v, v, v], [17, 64, 99], 3) == 1                          # last row_end != Cout
    assert call([v, v, v], [17, 64, 101], 3) == 1
    dil = _lib.ConvDesc.from_buffer_copy(d)
    dil.dh = 2
    assert call([v, v, v], [17, 64, 100], 3, dil) == 1                    # input dilation
    assert lib.coclr_conv3d_wgrad_multi(C.byref(d), p, p, None, (C.c_int32 * 1)(100), 1, p, 72, 1, 0, 0,
                                        None) == 1
    assert lib.coclr_conv3d_wgrad_multi(C.byref(d), p, p, (C.c_void_p * 1)(v), None, 1, p, 72, 1, 0, 0,
                                        None) == 1
