"""CPU tier for the forward / data-gradient dispatch: coclr_conv3d_fwd_plan (ConvGeom.fwd_plan: the launcher's own
planner and select_forward(), nothing launched) says what every row of tests/_fwd_cases.py reaches, and this
module asserts that the table covers

  * every kernel instantiation the launcher's kernel table (kFwdTable, the rows select_forward picks from) holds,
    except those listed as UNREACHABLE with the planner condition that excludes them (and none of those is reached);
  * every pair route of coclr_conv3d_fwd_multi (PAIRS);
  * every dispatch edge, per kernel family, by a NAMED row (HOLDERS): deleting one of those rows fails here;
  * the conditions the exact comparison of tests/test_gpu_fwd_exact.py rests on, per row;

and that the query refuses what the launch refuses.  tests/test_gpu_fwd_exact.py runs the same rows against
float64.
"""
import contextlib
import ctypes as C
import os

import pytest

import _fwd_cases as W
from coclr_amd import _lib, ops

K_STEM_GRID, K_WINO_GRID = 512, 256      # kStemGrid, kWinoGrid of conv_igemm.hip


@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def plan_of(c, **kw):
    with environment(c.env):
        return W.plan(c, **kw)


PLANS = [(c, W.launch_geom(c), plan_of(c)) for c in W.CASES]
PLAN = {c.name: pl for c, g, pl in PLANS}

LARGE = {"stem_grid", "hw_grid", "hw8_grid", "pw0_128x128", "pw1_64x128", "s10_128x128", "s11_64x128",
         "t20_128x128", "t21_64x128"}


def test_rows_are_small():
    """At most 32768 output positions; only the rows whose edge is a work-item count (see the table's docstring)
    come near it, every other row stays below 4096."""
    for c, g, pl in PLANS:
        n = W.positions(c)
        assert n <= 32768, c.name
        assert n <= 4096 or W.base_name(c) in LARGE, (c.name, n)
        assert max(c.Cin, c.Cout) <= 72 or c.Cout in (130, 380), c.name


def test_plan_agrees_with_the_other_queries():
    for c, g, pl in PLANS:
        assert g.ntiles() == pl["ntiles"], c.name
        assert g.bwd_sums_ok() == pl["bwd_sums_ok"], c.name
        assert pl["lattice"] == (g.lattice is not None), c.name
        assert pl["lTW"] + pl["lTH"] + pl["lTT"] + pl["lTN"] == {64: 6, 128: 7}[pl["BN"]], c.name
        assert pl["mtiles"] == -(-g.Cout // (64 if pl["family"] in ("wino_hw", "wino_hw8", "stem") else pl["BM"]))
        assert pl["lds"] <= 160 * 1024 and pl["threads"] == (512 if pl["family"] == "wino_hw8" else 256)
        if pl["family"] in ("wino_hw", "wino_hw8"):
            assert pl["grid"] == min(K_WINO_GRID, pl["mtiles"] * pl["ntiles"]), c.name
        else:
            assert pl["grid"] == pl["mtiles"] * pl["ntiles"], c.name
        if pl["family"] == "stem":
            assert pl["ntiles"] == min(K_STEM_GRID, pl["nboxes"]), c.name
        else:
            assert pl["ntiles"] == pl["nboxes"], c.name
        assert pl["nchunks"] == -(-g.Cin // pl["CC"]), c.name
    lib = _lib.load()
    d = _lib.ConvDesc.from_buffer_copy(PLANS[0][1].desc)
    out = (C.c_int32 * 40)()
    assert lib.coclr_conv3d_fwd_plan(None, 3, out) == 1
    assert lib.coclr_conv3d_fwd_plan(C.byref(d), 3, None) == 1
    d.kt = 2
    assert lib.coclr_conv3d_fwd_plan(C.byref(d), 3, out) == 1


def _reached():
    reached = {}
    for c, g, pl in PLANS:
        plans = [pl]
        if pl["variant"] == 41:
            plans.append(plan_of(c, in_affine=True))
        for p in plans:
            names = reached.setdefault(W.instantiation(p), [])
            if c.name not in names:
                names.append(c.name)
    return reached


def test_table_reaches_every_instantiation():
    reached = _reached()
    print("\ninstantiation <variant, family, form, KT KH KW CC BM BN PCH OCC, XV4 XG X16 INAFF lattice> -> rows")
    for inst in W.INSTANTIATIONS:
        print("  %s %s" % ("%-2d %-8s %d <%d,%d,%d,%2d,%3d,%3d,%2d,%d> %s" % (
            inst[:11] + ("".join(f for f, v in zip(("XV4 ", "XG ", "X16 ", "INAFF ", "lattice"), inst[11:]) if v)
                         or "-",)), ", ".join(reached.get(inst, [])) or "-"))
    print("UNREACHABLE")
    for inst, why in W.UNREACHABLE.items():
        print("  %-24s %s" % (inst, why))
    assert len(set(W.INSTANTIATIONS)) == len(W.INSTANTIATIONS)
    assert set(reached) <= set(W.INSTANTIATIONS), set(reached) - set(W.INSTANTIATIONS)
    assert set(W.UNREACHABLE) <= set(W.INSTANTIATIONS)
    for inst in W.INSTANTIATIONS:
        if inst in W.UNREACHABLE:
            assert inst not in reached, "%s is listed as unreachable but %s reach it" % (inst, reached[inst])
        else:
            assert reached.get(inst), "no row of the table reaches %s" % (inst,)


def test_every_twin_reaches_the_4_byte_kernel_of_its_base_row():
    for name in W.TWINS:
        a, b = PLAN[name], PLAN[name + "_4b"]
        assert a["XV4"] or a["XG"] or a["X16"], name
        assert not (b["XV4"] or b["XG"] or b["X16"]), name
        assert a["variant"] == b["variant"] and W.instantiation(a) != W.instantiation(b), name


# ---- pair routes ------------------------------------------------------------------------------------------------

def route(names):
    """What coclr_conv3d_fwd_multi does with consecutive calls, MODELLED from the slot plans of the rows: the
    library reports per call whether it fills its slot (out[32]) and which kernel it is, and this function
    restates the pairing rule of coclr_conv3d_fwd_multi on top (both slots filled and the same kernel: its pair
    kernel; the 64x128 / 64x64 XG (1,3,3) kernels: the mixed kernel; else two launches).  It is a model of that
    rule, not the library's own answer; tests/test_gpu_fwd_exact.py::test_pairs holds the results of each route
    to the single launches' bit for bit but cannot tell which route ran.  Kernels are compared WITHOUT the
    planner variant: 12 and 13 under XG are one kernel."""
    out = []
    for i in range(0, len(names), 2):
        if i + 1 >= len(names):
            out.append("odd")
            continue
        a, b = (plan_of(W.BY_NAME[n], slot=True) for n in names[i:i + 2])
        if a["slot_filled"] and b["slot_filled"]:
            if W.instantiation(a)[1:] == W.instantiation(b)[1:]:
                out.append("pair" if a["lds"] == b["lds"] else "pair-lds")
                continue
            wide, narrow = W._i(11, "igemm", 0, W.K133, 8, 64, 128, 3, xg=True), \
                W._i(12, "igemm", 0, W.K133, 8, 64, 64, 3, xg=True)
            # variant 13 under XG is the same kernel as variant 12 under XG
            ka, kb = (W.instantiation(p)[1:] for p in (a, b))
            if {ka, kb} == {wide[1:], narrow[1:]}:
                out.append("mixed %dx%d" % (a["BN"], b["BN"]))
                continue
        out.append("singles")
    return out


def test_pair_routes():
    seen = set()
    for names, want in W.PAIRS:
        got = route(list(names))
        print(names, got)
        if want == "odd":
            assert got == ["pair", "odd"], names
        elif want == "mixed":
            assert len(got) == 1 and got[0].startswith("mixed"), (names, got)
        elif want == "pair":
            assert got in (["pair"], ["pair-lds"]), (names, got)
        else:
            assert got == [want], (names, got)
        seen.update(got)
        seen.add(PLAN[names[0]]["family"] + ":" + got[0])
    assert {"mixed 128x64", "mixed 64x128", "pair-lds", "singles", "odd"} <= seen, seen
    # same-kernel pairs of every family that has a pair kernel
    assert {"igemm", "wino_t", "wino_tf"} <= {k.split(":")[0] for k in seen if ":pair" in k}, seen
    kinds = {(PLAN[n[0]]["KH"], PLAN[n[0]]["XV4"]) for n, w in W.PAIRS if w.startswith("pair")}
    assert (3, False) in kinds and (1, True) in kinds          # the (1,3,3) family and 16-byte pointwise
    # what never fills a slot
    for c, g, pl in PLANS:
        slot = plan_of(c, slot=True)
        assert slot["slot_filled"] == pl["pairable"], c.name
        if pl["family"] in ("wino_hw", "wino_hw8", "stem") or pl["lattice"] and pl["family"] == "wino_tf" or \
                pl["form"] in (5, 9):
            assert not pl["pairable"], c.name


# ---- dispatch edges ---------------------------------------------------------------------------------------------

def family(pl):
    if pl["family"] == "igemm":
        return {1: "pointwise", 3: "spatial", 7: "stem30"}[pl["KH"]] if pl["KT"] == 1 else "temporal"
    if pl["family"] == "wino_tf":
        return {6: "f43", 5: "f24", 9: "poly7"}[pl["form"]]
    return {"wino_t": "f23"}.get(pl["family"], pl["family"])


FAMILIES = ("pointwise", "spatial", "temporal", "stem30", "stem", "f23", "f43", "f24", "poly7", "wino_hw",
            "wino_hw8")


def planned(c, g, pl):
    """(Wo, Ho, To) as the planner boxes them (conv_normalise, then the Winograd planners' grouping)."""
    To, Ho, Wo = g.odim
    lat = g.lattice is not None
    free = [g.k[i] == 1 and g.s[i] == 1 and g.p[i] == 0 and g.d[i] == 1 and g.idim[i] == g.odim[i] and
            (not lat or (g.lattice[0][i] == 1 and g.lattice[1][i] == 0)) for i in range(3)]
    if free[1] and free[2]:
        Wo, Ho = Ho * Wo, 1
        if free[0]:
            Wo, To = Wo * To, 1
    f = family(pl)
    if f in ("f23", "f24", "poly7"):
        To = (To + 1) // 2
    if f == "f43":
        To = (To + 3) // 4
    if f in ("wino_hw", "wino_hw8"):
        Wo, Ho = Wo // 2, Ho // 2
    return Wo, Ho, To


def overhang(axis):
    return lambda c, g, pl: planned(c, g, pl)[axis] % (1 << pl[("lTW", "lTH", "lTT")[axis]]) != 0


def bm(pl):
    return 64 if pl["family"] in ("wino_hw", "wino_hw8", "stem") else pl["BM"]


EDGES = {
    "Cout % BM != 0": lambda c, g, pl: g.Cout % bm(pl) != 0,
    "Cout < 32": lambda c, g, pl: g.Cout < 32,
    "Cin % CC != 0": lambda c, g, pl: g.Cin % pl["CC"] != 0,
    "Cin <= CC: one LDS stage": lambda c, g, pl: pl["nchunks"] == 1,
    "phantom samples": lambda c, g, pl: g.N % (1 << pl["lTN"]) != 0,
    "overhang W": overhang(0),
    "overhang H": overhang(1),
    "overhang T": overhang(2),
    "frames % 4 == 1": lambda c, g, pl: g.odim[0] % 4 == 1,
    "frames % 4 == 2": lambda c, g, pl: g.odim[0] % 4 == 2,
    "frames % 4 == 3": lambda c, g, pl: g.odim[0] % 4 == 3,
    "odd frames": lambda c, g, pl: g.odim[0] % 2 == 1,
    "odd output pairs": lambda c, g, pl: ((g.odim[0] + 1) // 2) % 2 == 1,
    "work beyond the persistent grid": lambda c, g, pl: (pl["nboxes"] if pl["family"] == "stem" else
                                                         pl["mtiles"] * pl["ntiles"]) > pl["grid"] // (
        pl["mtiles"] if pl["family"] == "stem" else 1),
    "dilated input": lambda c, g, pl: max(g.d) > 1,
    "negative padding, explicit odim": lambda c, g, pl: min(g.p) < 0 and c.odim is not None,
    "two-wave kernel refused on Cin % 8": lambda c, g, pl: pl["family"] == "wino_hw" and pl["X16"] and
    g.Cin % 8 != 0 and not c.env,
    "destination lattice": lambda c, g, pl: pl["lattice"],
}

# (edge, family) -> the row that holds it
HOLDERS = {
    ('Cout % BM != 0', 'pointwise'): 'pw0_128x128',
    ('Cout < 32', 'pointwise'): 'pw2_64x64',
    ('Cin % CC != 0', 'pointwise'): 'pw0_128x128',
    ('Cin <= CC: one LDS stage', 'pointwise'): 'pw0_128x128',
    ('phantom samples', 'pointwise'): 'pw2_64x64',
    ('overhang W', 'pointwise'): 'pw2_cin8',
    ('Cout % BM != 0', 'spatial'): 's10_128x128',
    ('Cout < 32', 'spatial'): 's12_xg',
    ('Cin % CC != 0', 'spatial'): 's11_64x128',
    ('Cin <= CC: one LDS stage', 'spatial'): 's12_cin8',
    ('phantom samples', 'spatial'): 's12_xg',
    ('overhang W', 'spatial'): 's12_odd',
    ('overhang H', 'spatial'): 's12_odd',
    ('overhang T', 'spatial'): 's12_t3',
    ('Cout % BM != 0', 'temporal'): 't20_128x128',
    ('Cout < 32', 'temporal'): 't22_xv4',
    ('Cin % CC != 0', 'temporal'): 't21_64x128',
    ('Cin <= CC: one LDS stage', 'temporal'): 't22_cin8',
    ('phantom samples', 'temporal'): 't20_128x128',
    ('overhang W', 'temporal'): 't22_odd',
    ('overhang T', 'temporal'): 't22_xv4',
    ('Cout % BM != 0', 'stem30'): 'stem30_cin4',
    ('Cout < 32', 'stem30'): 'stem30_cin4',
    ('Cin <= CC: one LDS stage', 'stem'): 'stem',
    ('Cin % CC != 0', 'stem30'): 'stem30_dgrad',
    ('Cin <= CC: one LDS stage', 'stem30'): 'stem30_cin4',
    ('phantom samples', 'stem30'): 'stem30_cin4',
    ('overhang W', 'stem30'): 'stem30_cin4',
    ('overhang H', 'stem30'): 'stem30_small',
    ('overhang T', 'stem30'): 'stem30_small',
    ('Cout % BM != 0', 'stem'): 'stem',
    ('Cout < 32', 'stem'): 'stem',
    ('phantom samples', 'stem'): 'stem',
    ('overhang W', 'stem'): 'stem',
    ('overhang H', 'stem'): 'stem_cout72',
    ('overhang T', 'stem'): 'stem_small',
    ('Cout % BM != 0', 'f23'): 'w50_odd_frames',
    ('Cout < 32', 'f23'): 'w50_odd_frames',
    ('Cin % CC != 0', 'f23'): 'w50_odd_frames',
    ('Cin <= CC: one LDS stage', 'f23'): 'w50_odd_plane',
    ('phantom samples', 'f23'): 'w50_odd_frames',
    ('overhang W', 'f23'): 'w50_odd_plane',
    ('overhang T', 'f23'): 'w50_odd_frames',
    ('Cout % BM != 0', 'f43'): 'w51_t5',
    ('Cout < 32', 'f43'): 'w51_t5',
    ('Cin % CC != 0', 'f43'): 'w51_t5',
    ('phantom samples', 'f43'): 'w51_t5',
    ('overhang W', 'f43'): 'w51_t7_odd_plane',
    ('overhang T', 'f43'): 'w51_dgrad',
    ('Cout % BM != 0', 'f24'): 'w52_dense_odd',
    ('Cout < 32', 'f24'): 'w52_dense_odd',
    ('Cin % CC != 0', 'f24'): 'w52_dense_odd',
    ('phantom samples', 'f24'): 'w52_dense_odd',
    ('overhang W', 'f24'): 'w52_dense_odd_plane',
    ('overhang T', 'f24'): 'w52_dense_odd',
    ('Cout % BM != 0', 'poly7'): 'w41_t16',
    ('Cout < 32', 'poly7'): 'w41_t16',
    ('Cin % CC != 0', 'poly7'): 'w41_t16',
    ('phantom samples', 'poly7'): 'w41_t16',
    ('overhang W', 'poly7'): 'w41_odd_plane',
    ('overhang T', 'poly7'): 'w41_t20_odd_pairs',
    ('Cout % BM != 0', 'wino_hw'): 'hw_x16_cin20',
    ('Cout < 32', 'wino_hw'): 'hw_x16_cin20',
    ('Cin % CC != 0', 'wino_hw'): 'hw_x16_cin20',
    ('phantom samples', 'wino_hw'): 'hw_x16_cin20',
    ('overhang W', 'wino_hw'): 'hw_pch6_mis',
    ('overhang H', 'wino_hw'): 'hw_x16_w8off',
    ('overhang T', 'wino_hw'): 'hw_pch10',
    ('Cout % BM != 0', 'wino_hw8'): 'hw8',
    ('Cout < 32', 'wino_hw8'): 'hw8_dgrad',
    ('phantom samples', 'wino_hw8'): 'hw8',
    ('overhang W', 'wino_hw8'): 'hw8_dgrad',
    ('overhang H', 'wino_hw8'): 'hw8',
    ('overhang T', 'wino_hw8'): 'hw8_dgrad',
    ('frames % 4 == 1', 'f43'): 'w51_t5',
    ('frames % 4 == 2', 'f43'): 'w51_t6',
    ('frames % 4 == 3', 'f43'): 'w51_t7',
    ('odd frames', 'f23'): 'w50_odd_frames',
    ('odd frames', 'f24'): 'w52_dense_odd',
    ('odd output pairs', 'poly7'): 'w41_t20_odd_pairs',
    ('work beyond the persistent grid', 'stem'): 'stem_grid',
    ('work beyond the persistent grid', 'wino_hw'): 'hw_grid',
    ('work beyond the persistent grid', 'wino_hw8'): 'hw8_grid',
    ('dilated input', 'pointwise'): 'pw3_dilated',
    ('dilated input', 'spatial'): 's13_dilated',
    ('dilated input', 'temporal'): 't22_dgrad_st2',
    ('negative padding, explicit odim', 'stem'): 'stem_slice_kt3',
    ('two-wave kernel refused on Cin % 8', 'wino_hw'): 'hw_x16_cin20',
    ('destination lattice', 'temporal'): 't22_phase0',
    ('destination lattice', 'f43'): 'w51_phase0_t32',
    ('destination lattice', 'f24'): 'w52_phase1_t32',
}

# (edge, family) pairs no row can hold, with the reason
NO_SUCH_EDGE = {
    # a policy of ConvGeom, not of the launcher: through the C ABI alone these kernels do run with one stage, and
    # that path stays untested here (every caller in the tree goes through ConvGeom)
    ("Cin <= CC: one LDS stage", "f43"): "ConvGeom refuses Winograd below 16 input channels (winograd_ok); CC = 8",
    ("Cin <= CC: one LDS stage", "f24"): "as f43",
    ("Cin <= CC: one LDS stage", "poly7"): "as f43",
    ("Cin <= CC: one LDS stage", "wino_hw"): "as f43",
    ("Cin <= CC: one LDS stage", "wino_hw8"): "as f43",
    ("Cin % CC != 0", "stem"): "Cin = CC = 3",
    ("Cin % CC != 0", "wino_hw8"): "the two-wave kernel refuses Cin % 8 (held as its own edge)",
}

PER_FAMILY = ("Cout % BM != 0", "Cout < 32", "Cin % CC != 0", "Cin <= CC: one LDS stage", "phantom samples",
              "overhang W", "overhang H", "overhang T")
SPECIFIC = {
    "frames % 4 == 1": ("f43",), "frames % 4 == 2": ("f43",), "frames % 4 == 3": ("f43",),
    "odd frames": ("f23", "f24"), "odd output pairs": ("poly7",),
    "work beyond the persistent grid": ("stem", "wino_hw", "wino_hw8"),
    "dilated input": ("pointwise", "spatial", "temporal"),
    "negative padding, explicit odim": ("stem",),
    "two-wave kernel refused on Cin % 8": ("wino_hw",),
    "destination lattice": ("temporal", "f43", "f24"),
}


def hits():
    table = {}
    for c, g, pl in PLANS:
        for edge, pred in EDGES.items():
            if pred(c, g, pl):
                table.setdefault((edge, family(pl)), []).append(c.name)
    return table


def required():
    """Axes a family's planner never boxes cannot overhang: the 1-wide axes of each stencil class."""
    req = []
    flat = {"pointwise": ("overhang H", "overhang T"), "temporal": ("overhang H",), "f23": ("overhang H",),
            "f43": ("overhang H",), "f24": ("overhang H",), "poly7": ("overhang H",)}
    for f in FAMILIES:
        for e in PER_FAMILY:
            if e in flat.get(f, ()) or (e, f) in NO_SUCH_EDGE:
                continue
            req.append((e, f))
    for e, fams in SPECIFIC.items():
        req += [(e, f) for f in fams]
    return req


def test_every_edge_is_held_by_a_named_row():
    table = hits()
    print()
    for key in required():
        print("  %-40s %-10s %s" % (key[0], key[1], ", ".join(table.get(key, [])) or "-"))
    for key in required():
        assert key in HOLDERS, "no holder named for %s in %s (rows that hit it: %s)" % (key + (table.get(key),))
        name = HOLDERS[key]
        assert name in W.BY_NAME, "%s, the holder of %s, is not in the table" % (name, key)
        assert name in table.get(key, []), "%s does not hit %s in %s" % ((name,) + key)
    for key in NO_SUCH_EDGE:
        assert not table.get(key), (key, table.get(key))


def test_stem_partial_carries_several_boxes():
    pl = PLAN["stem_grid"]
    assert pl["nboxes"] > K_STEM_GRID == pl["ntiles"]
    for n in ("hw_grid", "hw8_grid"):
        assert PLAN[n]["mtiles"] * PLAN[n]["ntiles"] > K_WINO_GRID == PLAN[n]["grid"], n
    assert PLAN["hw8_grid"]["family"] == "wino_hw8" and PLAN["hw_grid"]["family"] == "wino_hw"
    assert PLAN["hw_grid"]["X16"]


# ---- refusals ---------------------------------------------------------------------------------------------------

def refused(c, **kw):
    try:
        plan_of(c, **kw)
    except _lib.HipLibraryError:
        return True
    return False


def test_query_refuses_what_the_launch_refuses():
    for c, g, pl in PLANS:
        v = pl["variant"]
        assert refused(c, n_index=True) == (v in (41, 50, 51, 52, 60)), c.name        # every Winograd form
        assert refused(c, in_affine=True) == (v != 41), c.name
        assert refused(c, in_affine=True, n_index=True), c.name
        assert refused(c, bwd_sums=True) == (v in (60, 31, 51, 52, 41)) == (not pl["bwd_sums_ok"]), c.name
        assert refused(c, bwd_sums=True, n_index=True), c.name
        if v == 60:
            assert refused(c, y_aligned=False), c.name
            assert refused(c, y_nstride=g.Cout * g.odim[0] * g.odim[1] * g.odim[2] + 1), c.name
        else:
            assert not refused(c, y_aligned=False), c.name
    # a byte offset past the descriptors' 2 GiB range
    c = W.BY_NAME["pw2_64x64"]
    assert refused(c, x_nstride=2 ** 29) and not refused(c, x_nstride=2 ** 27)
    assert refused(c, n_index=True, x_nstride=2 ** 25, Nx=16) and not refused(c, n_index=True, x_nstride=2 ** 25, Nx=15)


# ---- what the exact comparison rests on -------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c.name for c in W.CASES if W.base_name(c) == c.name])
def test_exactness_conditions(name):
    """Every product sum of the row stays below 2^24 units of its granule, in the accumulators (Cin * taps *
    alphabet maxima, times the transform gains bounded in tests/test_gpu_fwd_exact.py) and in the statistics
    (per channel sum |y| / G and sum y^2 / G^2 of the float64 reference): every partial in any order is exact."""
    c = W.BY_NAME[name]
    g = W.launch_geom(c)
    G = W.granule(c)
    taps = g.k[0] * g.k[1] * g.k[2]
    # 2^9: the largest product of input- and output-transform gains of any form (F(4,3): 10 * 19 < 2^8, times the
    # operand gain 7/24 * G; F(2x2,3x3): 4 * 4 * 4)
    assert g.Cin * taps * c.xa * c.wa * 2 ** 9 < 2 ** 24, name
    x, w, ref = W.problem(name)
    assert float(x.abs().max()) <= c.xa and float((w / G).abs().max()) <= c.wa
    assert bool((w / G == (w / G).round()).all()) and bool((ref == ref.round()).all())
    s1 = float((ref.abs() / G).sum((0, 2, 3, 4)).max())
    s2 = float(((ref / G) ** 2).sum((0, 2, 3, 4)).max())
    print("%s: max over channels of sum|y|/G = %d, of sum y^2/G^2 = %d" % (name, s1, s2))
    assert s1 < 2 ** 24 and s2 < 2 ** 24, name
    # an accumulate pass on a prior of G * [-8, 8]: sum (y + prior)^2 / G^2 <= s2 + 16 s1 + 64 positions; the
    # second pass of a phase row doubles y
    assert s2 + 16 * s1 + 64 * W.positions(c) < 2 ** 24, name
    assert W.phase(c) is None or 4 * s2 < 2 ** 24, name
    # backward sums (the rows whose kernel forms them): sum g in units of G, sum g * xhat in units of G / 2
    if PLAN[name]["bwd_sums_ok"]:
        for relu in (False, True):
            by, scale, shift, mean, invstd, gz, xhat = W.bwd_operands(name, relu)
            assert bool((2 * xhat == (2 * xhat).round()).all()) and float(xhat.abs().max()) <= 12
            b1 = float((gz.abs() / G).sum((0, 2, 3, 4)).max())
            b2 = float(((gz * xhat).abs() * 2 / G).sum((0, 2, 3, 4)).max())
            assert b1 < 2 ** 24 and b2 < 2 ** 24, (name, relu, b1, b2)
