"""CPU tier for the pooling dispatch: coclr_pool_plan (the plan structs the launchers of coclr_amd/csrc/pool.hip
switch on, nothing launched) says what every row of tests/_pool_cases.py reaches, and this module asserts that the
table covers

  * every kernel instantiation the launchers can select (forward: generic, separable TT x indices, tiled template x
    indices; backward: generic gather, 3x3x3 gather, the four colour-class templates and the generic form; pooled
    BatchNorm backward: its two templates and the generic form), except those listed as UNREACHABLE with the
    excluding condition (and none of those is reached);
  * every dispatch edge in EDGES below.

The `vec` flags of the plan are not a mirror of the kernels' conditions: the launchers pass them to the kernels,
which branch on them alone (the 3x3x3 gather's `S % 4 == 0` rule lives in plan_pool_bwd).

tests/test_gpu_pool_exact.py runs the same rows against float64, so a row that is the only cover of an
instantiation or edge cannot be dropped without this module failing.  Also here: the refusals of the plan query
and of coclr_bn_act_backward_pooled for a plane that does not fit, which are host-side and need no GPU.
"""
import ctypes as C

import pytest

import _pool_cases as P
from coclr_amd import _lib, ops

PLANS = [(c, P.plan(c, True), P.plan(c, False)) for c in P.CASES]

T133 = (1, 3, 3, 1, 2, 2, 2)
T333 = (3, 3, 3, 1, 1, 1, 4)
T333S2 = (3, 3, 3, 2, 2, 2, 2)
T222 = (2, 2, 2, 2, 2, 2, 2)
TILED = (T133, T333, T333S2, T222)


def test_rows_are_small():
    for c in P.CASES:
        assert P.elems(c) <= P.MAX_ELEMS, c.name


def test_plan_is_consistent():
    """Grids, LDS sizes and the older query agree with the plan."""
    for c, pi, pn in PLANS:
        g = P.geom(c)
        assert ops.pooled_backward_fits(g) == pi["pooled"]["fits"], c.name
        for pl in (pi, pn):
            f = pl["fwd"]
            assert f["lds"] <= 64 * 1024, c.name
            if f["family"] != "generic":
                folded = c.N * c.C * (f["tfold"] if f["tfold"] > 1 else 1)
                assert f["grid"] == ((folded + f["G"] - 1) // f["G"], 1), c.name
            else:
                assert f["grid"][1] == min(c.N * c.C, 65535) and f["lds"] == 0, c.name
        assert pi["bwd"] == pn["bwd"] and pi["pooled"] == pn["pooled"], c.name
        assert pi["bwd"]["lds"] <= 64 * 1024 and pi["pooled"]["lds"] <= 64 * 1024, c.name
        assert pi["pooled"]["G"] <= 8, c.name                  # coef[8][4] of the apply kernel


def test_plan_refusals():
    lib = _lib.load()
    d = _lib.PoolDesc.from_buffer_copy(P.geom(P.CASES[0]).desc)
    out = (C.c_int32 * 32)()
    assert lib.coclr_pool_plan(None, 1, 0, 0, out) == 1
    assert lib.coclr_pool_plan(C.byref(d), 1, 0, 0, None) == 1
    d.pt = 2                                                   # padding above half the window, as the forward
    assert lib.coclr_pool_plan(C.byref(d), 1, 0, 0, out) == 1


def test_pooled_backward_refuses_a_plane_that_does_not_fit():
    """Si == 16384 fits, 16896 does not: COCLR_EINVAL (1) from the host, before anything is launched.  (A call that
    got as far as a launch here would report the missing device, not 1.)"""
    lib = _lib.load()
    assert P.plan(P.BY_NAME["t133_128"])["pooled"]["fits"]
    c = P.BY_NAME["gen_132x128"]
    assert not P.plan(c)["pooled"]["fits"]
    g = P.geom(c)
    assert not ops.pooled_backward_fits(g)
    d = _lib.PoolDesc.from_buffer_copy(g.desc)
    p = C.c_void_p(4096)
    st = P.strides(c)
    assert lib.coclr_bn_act_backward_pooled(C.byref(d), p, p, p, p, p, p, p, p, p, p, p, st["dy"], st["x"],
                                            st["dx"], 1, 1, None) == 1


def _reached():
    fwd, bwd, pooled = {}, {}, {}
    for c, pi, pn in PLANS:
        for idx, pl in ((True, pi), (False, pn)):
            f = pl["fwd"]
            key = ("generic", None) if f["family"] == "generic" else (f["family"], f["template"], idx)
            fwd.setdefault(key, []).append(c.name)
        b = pi["bwd"]
        bwd.setdefault((b["family"], b["template"]), []).append(c.name)
        if c.pooled:
            pooled.setdefault(pi["pooled"]["template"], []).append(c.name)
    return fwd, bwd, pooled


@pytest.mark.parametrize("which", ["fwd", "bwd", "pooled"])
def test_table_reaches_every_instantiation(which):
    reached = dict(zip(("fwd", "bwd", "pooled"), _reached()))[which]
    insts = dict(fwd=P.FWD_INSTANTIATIONS, bwd=P.BWD_INSTANTIATIONS, pooled=P.POOLED_INSTANTIATIONS)[which]
    print("\n%s instantiation -> rows" % which)
    for inst in insts:
        print("  %-40s %s" % (inst, ", ".join(reached.get(inst, [])) or "-"))
    assert set(reached) <= set(insts), set(reached) - set(insts)
    for inst in insts:
        if (which, inst) in P.UNREACHABLE:
            assert inst not in reached, "%s is listed as unreachable but %s reach it" % (inst, reached[inst])
        else:
            assert reached.get(inst), "no row of the table reaches %s %s" % (which, inst)


def _si(c, tfold):
    return c.idim[0] * c.idim[1] * c.idim[2] // (tfold if tfold > 1 else 1)


def _planes(c, tfold):
    return c.N * c.C * (tfold if tfold > 1 else 1)


def _straddles(c, part, extras):
    """A group of part["G"] > 1 volumes holds the last volume of one sample and the first of the next, and the
    operands named in `extras` are channel slices, so the two are not adjacent in memory."""
    per_sample = c.C * (part["tfold"] if part["tfold"] > 1 else 1)
    return part["G"] > 1 and per_sample % part["G"] != 0 and c.N > 1 and all(getattr(c, e) > 0 for e in extras)


def _partial(c, part):
    return part["G"] > 1 and _planes(c, part["tfold"]) % part["G"] != 0


def _fwd(pred, family=None, template=None):
    def f(c, pi, pn):
        return any((family is None or pl["fwd"]["family"] == family) and
                   (template is None or pl["fwd"]["template"] == template) and pred(c, pl["fwd"]) for pl in (pi, pn))
    return f


def _bwd(pred, family=None, template=None):
    def f(c, pi, pn):
        b = pi["bwd"]
        return (family is None or b["family"] == family) and (template is None or b["template"] == template) and \
            pred(c, b)
    return f


def _pooled(pred):
    def f(c, pi, pn):
        return c.pooled and pi["pooled"]["fits"] and pred(c, pi["pooled"])
    return f


def _max_class_g():
    """The largest G the colour-class backward can run with under the table's size limit, by the launcher's rule:
    G = 4096 / Si, halved while ceil(planes / G) < 1024; planes * Si <= MAX_ELEMS.  G is a power of two below
    4096 / Si, kept only if planes >= 1023 * G + 1."""
    best = 0
    for si in (1, 2, 4, 8, 16):
        g = 4096 // si
        while g > 1 and (1023 * g + 1) * si > P.MAX_ELEMS:
            g >>= 1
        best = max(best, g)
    return best


MAX_CLASS_G = _max_class_g()


def _wo(c):
    return P.odim(c)[2]


EDGES = {}

# ---- separable 3x3x3 forward
for hw in (16, 32, 64, 256):
    EDGES["sep333 H*W = %d" % hw] = _fwd(lambda c, f, hw=hw: c.idim[1] * c.idim[2] == hw, "sep333")
EDGES["sep333 8x4 plane (W != H)"] = _fwd(lambda c, f: c.idim[1:] == (4, 8), "sep333")
for ti in (1, 5, 32):
    EDGES["sep333 run-time frame count Ti = %d" % ti] = _fwd(lambda c, f, ti=ti: c.idim[0] == ti, "sep333", 0)
EDGES["sep333 4-byte staging (x_nstride % 4 != 0)"] = _fwd(lambda c, f: not f["vec"], "sep333")
EDGES["sep333 last group with gcount < PG"] = _fwd(lambda c, f: (c.N * c.C) % f["G"] != 0, "sep333")
EDGES["sep333 group straddles two samples of a channel slice"] = _fwd(
    lambda c, f: c.C % f["G"] != 0 and c.N > 1 and c.x_extra > 0 and c.y_extra > 0, "sep333")
EDGES["sep333 in-affine with ReLU"] = _fwd(lambda c, f: c.aff == "relu", "sep333")
EDGES["sep333 in-affine without ReLU"] = _fwd(lambda c, f: c.aff == "plain", "sep333")
EDGES["sep333 -inf / NaN input"] = _fwd(lambda c, f: c.special, "sep333")
# ---- its fall-throughs
EDGES["333 fall-through: Ti = 33"] = _fwd(lambda c, f: c.idim[0] == 33 and c.idim[1:] == (4, 4), "tiled", T333)
EDGES["333 fall-through: H*W = 8"] = _fwd(lambda c, f: c.idim[1] * c.idim[2] == 8, "tiled", T333)
EDGES["333 fall-through: 32x16 plane"] = _fwd(lambda c, f: c.idim[1:] == (16, 32), "tiled", T333)
EDGES["333 fall-through: W = 6"] = _fwd(lambda c, f: c.idim[2] == 6, "tiled", T333)
EDGES["Ti = 32 at 16x16: separable without indices, tiled with them"] = (
    lambda c, pi, pn: c.idim == (32, 16, 16) and pn["fwd"]["family"] == "sep333" and pn["fwd"]["lds"] == 65536 and
    pi["fwd"]["family"] == "tiled" and pi["fwd"]["template"] == T333)
# ---- tiled forward, per template
for t in TILED:
    EDGES["tiled %s G == 1" % (t,)] = _fwd(lambda c, f: f["G"] == 1, "tiled", t)
    EDGES["tiled %s G >= 2" % (t,)] = _fwd(lambda c, f: f["G"] >= 2, "tiled", t)
    EDGES["tiled %s last group with gcount < G" % (t,)] = _fwd(_partial, "tiled", t)
    EDGES["tiled %s group straddles two samples, x and y channel slices" % (t,)] = _fwd(
        lambda c, f: _straddles(c, f, ("x_extra", "y_extra")), "tiled", t)
    EDGES["tiled %s 16-byte staging" % (t,)] = _fwd(lambda c, f: f["vec"], "tiled", t)
    EDGES["tiled %s 4-byte staging (Si %% 4 != 0)" % (t,)] = _fwd(
        lambda c, f: not f["vec"] and _si(c, f["tfold"]) % 4 != 0, "tiled", t)
    EDGES["tiled %s Wo %% WPT != 0" % (t,)] = _fwd(lambda c, f, t=t: _wo(c) % t[6] != 0, "tiled", t)
    EDGES["tiled %s in-affine" % (t,)] = _fwd(lambda c, f: c.aff is not None, "tiled", t)
EDGES["tiled tfold > 1 with T not a multiple of G >= 2"] = _fwd(
    lambda c, f: f["tfold"] > 1 and f["G"] >= 2 and f["tfold"] % f["G"] != 0, "tiled", T133)
EDGES["tiled in-affine with ReLU"] = _fwd(lambda c, f: c.aff == "relu", "tiled")
EDGES["tiled in-affine without ReLU, tfold > 1 (channel = plane / tfold)"] = _fwd(
    lambda c, f: c.aff == "plain" and f["tfold"] > 1, "tiled")
EDGES["tiled -inf / NaN input"] = _fwd(lambda c, f: c.special, "tiled")
EDGES["tiled Si == 16384 (the whole 64 KiB)"] = _fwd(lambda c, f: f["lds"] == 65536, "tiled")
# ---- generic forward
EDGES["generic forward: Si > 16384 (132x128 plane)"] = _fwd(
    lambda c, f: c.idim[1:] == (132, 128) and c.k == (1, 3, 3), "generic")
EDGES["generic forward: unlisted stencil (1,1,1)/(1,2,2)"] = _fwd(
    lambda c, f: c.k == (1, 1, 1) and c.s == (1, 2, 2), "generic")
EDGES["generic forward: more than 65535 planes of a 2x2 map"] = _fwd(
    lambda c, f: c.N * c.C > 65535 and c.idim[1:] == (2, 2) and f["grid"][1] == 65535, "generic")
EDGES["generic forward: in-affine with ReLU"] = _fwd(lambda c, f: c.aff == "relu", "generic")
EDGES["generic forward: in-affine without ReLU"] = _fwd(lambda c, f: c.aff == "plain", "generic")
# ---- 3x3x3 gather backward
for s in (1, 2, 3, 6, 8, 64, 128):
    EDGES["gather333 S = %d" % s] = _bwd(lambda c, b, s=s: _si(c, 1) == s, "gather333")
EDGES["gather333 S = 2 as H*W = 1, T = 2"] = _bwd(lambda c, b: c.idim == (2, 1, 1), "gather333")
EDGES["gather333 S = 2 as H*W = 2, T = 1"] = _bwd(lambda c, b: c.idim == (1, 1, 2), "gather333")
EDGES["gather333 G > 1"] = _bwd(lambda c, b: b["G"] > 1 and c.N * c.C >= 4096, "gather333")
EDGES["gather333 last group with gcount < G"] = _bwd(_partial, "gather333")
EDGES["gather333 dy a channel slice, group straddles two samples"] = _bwd(
    lambda c, b: _straddles(c, b, ("d_extra",)), "gather333")
EDGES["gather333 16-byte staging"] = _bwd(lambda c, b: b["vec"], "gather333")
EDGES["gather333 4-byte staging because S % 4 != 0, dy_nstride % 4 == 0"] = _bwd(
    lambda c, b: not b["vec"] and _si(c, 1) % 4 != 0 and P.strides(c)["dy"] % 4 == 0 and c.C % 2 == 1, "gather333")
for s in (1, 2, 3, 6):
    # dy_nstride % 4 == 0 alone used to select the 16-byte loop, which stages only S >> 2 slots per volume
    EDGES["gather333 S = %d with dy_nstride %% 4 == 0: 4-byte staging" % s] = _bwd(
        lambda c, b, s=s: _si(c, 1) == s and P.strides(c)["dy"] % 4 == 0 and not b["vec"], "gather333")
EDGES["gather333 4-byte staging because dy_nstride % 4 != 0"] = _bwd(
    lambda c, b: not b["vec"] and _si(c, 1) % 4 == 0, "gather333")
# ---- colour-class backward
EDGES["classes G == 1"] = _bwd(lambda c, b: b["G"] == 1, "classes")
EDGES["classes G == 2"] = _bwd(lambda c, b: b["G"] == 2, "classes")
EDGES["classes G >= 8"] = _bwd(lambda c, b: b["G"] >= 8, "classes")
EDGES["classes G == 64"] = _bwd(lambda c, b: b["G"] == 64, "classes")
EDGES["classes G == 2048, the largest within the table's size limit"] = _bwd(
    lambda c, b: b["G"] == MAX_CLASS_G == 2048 and P.elems(c) <= P.MAX_ELEMS, "classes")
EDGES["classes last group with gcount < G"] = _bwd(_partial, "classes")
EDGES["classes group straddles two samples, dy and dx channel slices"] = _bwd(
    lambda c, b: _straddles(c, b, ("d_extra",)), "classes")
EDGES["classes tfold > 1 with G > 1"] = _bwd(lambda c, b: b["tfold"] > 1 and b["G"] > 1, "classes")
EDGES["classes generic form through kq above the template's: (1,3,3)/(1,2,2) on 112x112"] = _bwd(
    lambda c, b: c.k == (1, 3, 3) and c.idim[1:] == (112, 112) and b["kq"] > 1, "classes", (0, 0, 0, 0))
EDGES["classes generic form: (3,3,3)/(1,1,1) with kq = 2"] = _bwd(
    lambda c, b: c.k == (3, 3, 3) and c.s == (1, 1, 1) and b["kq"] == 2, "classes", (0, 0, 0, 0))
EDGES["classes (1,1,1,2) with kq == 2"] = _bwd(lambda c, b: b["kq"] == 2, "classes", (1, 1, 1, 2))
EDGES["classes (1,1,1,2) refused at kq = 3+"] = _bwd(
    lambda c, b: c.k == (1, 1, 1) and b["kq"] > 2, "classes", (0, 0, 0, 0))
EDGES["classes 16-byte stores of dx"] = _bwd(lambda c, b: b["vec"], "classes")
EDGES["classes 4-byte stores: Si % 4 != 0"] = _bwd(
    lambda c, b: not b["vec"] and _si(c, b["tfold"]) % 4 != 0, "classes")
EDGES["classes 4-byte stores: dx_nstride % 4 != 0"] = _bwd(
    lambda c, b: not b["vec"] and _si(c, b["tfold"]) % 4 == 0, "classes")
# ---- generic gather backward
EDGES["generic gather backward: Si > 16384"] = _bwd(lambda c, b: _si(c, 1) > 16384, "generic")
# ---- pooled BatchNorm backward
for g in (1, 2, 4, 8):
    EDGES["pooled G == %d" % g] = _pooled(lambda c, q, g=g: q["G"] == g)
EDGES["pooled group crosses a channel boundary (T = 3, G = 8)"] = _pooled(
    lambda c, q: q["G"] == 8 and q["tfold"] == 3)
EDGES["pooled group crosses a sample boundary"] = _pooled(
    lambda c, q: q["G"] > 1 and (c.C * max(q["tfold"], 1)) % q["G"] != 0 and c.N > 1)
EDGES["pooled last group with gcount < G"] = _pooled(_partial)
EDGES["pooled Si == 16384 fits"] = _pooled(lambda c, q: _si(c, q["tfold"]) == 16384)
EDGES["pooled generic form of (3,3,3)-class pools"] = _pooled(
    lambda c, q: c.k == (3, 3, 3) and c.s == (1, 1, 1) and q["template"] == (0, 0, 0, 0))
EDGES["pooled (2,2,2,1) through (3,3,3)/(2,2,2)"] = _pooled(
    lambda c, q: c.k == (3, 3, 3) and c.s == (2, 2, 2) and q["template"] == (2, 2, 2, 1))
EDGES["pooled generic form of a one-class pool, (2,2,2)/(2,2,2), with G > 1"] = _pooled(
    lambda c, q: c.k == (2, 2, 2) and q["template"] == (0, 0, 0, 0) and q["G"] > 1)
EDGES["pooled generic form through kq above the template's"] = _pooled(
    lambda c, q: c.k == (1, 3, 3) and q["kq"] > 1 and q["template"] == (0, 0, 0, 0))
EDGES["pooled 16-byte apply pass"] = _pooled(lambda c, q: q["vec"])
EDGES["pooled 4-byte apply pass"] = _pooled(lambda c, q: not q["vec"])
EDGES["pooled 4-byte apply pass: Si % 4 == 0, only y's stride is odd"] = _pooled(
    lambda c, q: not q["vec"] and _si(c, q["tfold"]) % 4 == 0 and P.strides(c)["x"] % 4 != 0 and
    P.strides(c)["dx"] % 4 == 0)
EDGES["pooled 4-byte apply pass: Si % 4 == 0, only dy's stride is odd"] = _pooled(
    lambda c, q: not q["vec"] and _si(c, q["tfold"]) % 4 == 0 and P.strides(c)["x"] % 4 == 0 and
    P.strides(c)["dx"] % 4 != 0)
EDGES["pooled without ReLU in the pool's in-affine"] = _pooled(lambda c, q: c.aff == "plain")
EDGES["pooled with ReLU in the pool's in-affine"] = _pooled(lambda c, q: c.aff == "relu")


@pytest.mark.parametrize("edge", list(EDGES))
def test_table_hits_edge(edge):
    hit = [c.name for c, pi, pn in PLANS if EDGES[edge](c, pi, pn)]
    print("\n%s: %s" % (edge, hit))
    assert hit, "no row hits: %s" % edge


def test_pooled_rows_carry_the_pools_affine():
    """The pooled backward is the backward of a unit the pool read through its affine."""
    for c in P.CASES:
        if c.pooled:
            assert c.aff is not None and not c.special, c.name
            assert P.plan(c)["pooled"]["fits"], c.name


def test_unreachable_edges_have_reasons():
    for edge, why in P.UNREACHABLE_EDGES.items():
        assert edge not in EDGES and why
    # the excluding conditions, from the table's own limit
    assert 65536 * 16385 > P.MAX_ELEMS
    assert 1023 * 4096 + 1 > P.MAX_ELEMS >= 1023 * 2048 + 1 and MAX_CLASS_G == 2048
