"""CPU tier for the BatchNorm dispatch: coclr_bn_plan (the route struct the launchers of coclr_amd/csrc/bn.hip switch
on, nothing launched) says what every row of tests/_bn_cases.py reaches, and this module asserts that the table
covers every route x vector-width instantiation and every dispatch edge in EDGES below.
tests/test_gpu_bn_exact.py runs the same rows against float64, so a row that is the only cover of something cannot
be dropped without this module failing.

Instantiations: forward fused <VEC>, forward apply <VEC> (+ the non-temporal one), backward fused <VEC>, backward
reduce / apply <VEC>, and the multi kernels <VEC>.  The TEMPORAL vector instantiations of the streaming passes are
reachable only with COCLR_BN_NT_MB < 0, read once per process: tests/test_gpu_bn_exact.py covers them in a child
process, and test_non_temporal_switch below asserts what the switch does to the plan.
"""
import ctypes as C
import os
import subprocess
import sys

import pytest

import _bn_cases as B
from coclr_amd import _lib, ops

PLANS = [(c, B.plan(c)) for c in B.CASES]


def test_rows_are_small():
    for c in B.CASES:
        assert B.elems(c) <= B.MAX_ELEMS, c.name


def test_plan_is_consistent():
    for c, pl in PLANS:
        f, b = pl["fwd"], pl["bwd"]
        small = c.N * B.S(c) <= ops.SMALL_CHANNEL
        assert f["one_wg"] == small, c.name
        assert b["one_wg"] == (small and not c.z and not c.dres), c.name
        for r in (f, b):
            assert (r["grid"] == (0, 0)) == r["one_wg"], c.name
            if not r["one_wg"]:
                assert r["grid"][1] % c.C == 0 and r["grid"][0] >= 1, c.name
                assert r["nt"] == r["vec"], c.name                  # COCLR_BN_NT_MB defaults to 0: every vector pass
        assert (b["groups"] == 0) == b["one_wg"], c.name
        assert b["groups"] <= c.N, c.name                            # the workspace holds 2 * C * N doubles
        st = B.strides(c)
        s4 = B.S(c) % 4 == 0
        assert f["vec"] == (s4 and st["y"] % 4 == 0 and st["z"] % 4 == 0), c.name
        assert b["vec"] == (s4 and all(st[k] % 4 == 0 for k in ("dz", "y", "dy")) and
                            (not c.z or st["z"] % 4 == 0) and (not c.dres or st["dres"] % 4 == 0)), c.name
    out = (C.c_int32 * 16)()
    lib = _lib.load()
    assert lib.coclr_bn_plan(0, 1, 4, 4, 4, 4, 4, 4, 0, 0, 0, out) == 1
    assert lib.coclr_bn_plan(1, 1, 4, 4, 4, 4, 4, 4, 0, 0, 0, None) == 1
    assert lib.coclr_bn_plan(1, 1, 4, 4, 4, 4, 4, 4, 1, 0, 1, out) == 1      # partials with z: no such form


def test_table_reaches_every_instantiation():
    want = {(d, one, vec) for d in ("fwd", "bwd") for one in (True, False) for vec in (True, False)}
    got = {}
    for c, pl in PLANS:
        for d in ("fwd", "bwd"):
            got.setdefault((d, pl[d]["one_wg"], pl[d]["vec"]), []).append(c.name)
    print()
    for k in sorted(want):
        print("  %-5s one_wg=%-5s vec=%-5s %s" % (k + (", ".join(got.get(k, [])) or "-",)))
    assert want == set(got)
    # from-partials apply pass, both widths
    assert {B.plan(B.BY_NAME[r], partials=True)["bwd"]["vec"] for r, _ in B.PARTIALS.values()} == {True, False}
    for r, _ in B.PARTIALS.values():
        b = B.plan(B.BY_NAME[r], partials=True)["bwd"]
        assert b["partials"] and not b["one_wg"] and b["groups"] == 0, r
    # the multi kernels <VEC>: a run of >= 2 units of each width, forward and backward
    for direction in ("fwd", "bwd"):
        widths = set()
        for names in B.MULTI.values():
            for run in B.runs(names, [None] * len(names) if direction == "bwd" else None):
                if len(run) >= 2:
                    widths.add(B.plan(B.BY_NAME[run[0]])[direction]["vec"])
        assert widths == {True, False}, direction


def _only_odd(op):
    def pred(c, pl):
        return B.S(c) % 4 == 0 and c.pad == (op,)
    return pred


EDGES = {
    "N*S == 32768: one workgroup per channel": lambda c, pl: c.N * B.S(c) == 32768 and pl["fwd"]["one_wg"] and
    pl["bwd"]["one_wg"],
    "N*S == 32772: streaming": lambda c, pl: c.N * B.S(c) == 32772 and not pl["fwd"]["one_wg"] and
    not pl["bwd"]["one_wg"],
    "S % 4 != 0, one workgroup": lambda c, pl: B.S(c) % 4 != 0 and pl["bwd"]["one_wg"],
    "S % 4 != 0, streaming": lambda c, pl: B.S(c) % 4 != 0 and not pl["bwd"]["one_wg"],
    "z given: streaming even when small": lambda c, pl: c.z and pl["fwd"]["one_wg"] and not pl["bwd"]["one_wg"],
    "dres given: streaming even when small": lambda c, pl: c.dres and not c.z and pl["fwd"]["one_wg"] and
    not pl["bwd"]["one_wg"],
    "z and dres, every operand a channel slice": lambda c, pl: c.z and c.dres and set(c.extra) == set(B.OPERANDS),
    "reduce groups: S = 64, N = 70 (64 samples per group and a remainder)":
        lambda c, pl: B.S(c) == 64 and c.N == 70 and pl["bwd"]["groups"] == 2,
    "reduce groups: S >= 4096, one per sample": lambda c, pl: B.S(c) >= 4096 and pl["bwd"]["groups"] == c.N > 1,
    "plane grid with gx > 1 and S/4 not a multiple of the unrolled stride":
        lambda c, pl: pl["bwd"]["grid"][0] > 1 and (B.S(c) // 4) % (2 * 256 * pl["bwd"]["grid"][0]) != 0 and
        (B.S(c) // 4) % (4 * 256 * pl["fwd"]["grid"][0]) != 0 and pl["bwd"]["vec"],
    "plane grid with several samples per block": lambda c, pl: not pl["bwd"]["one_wg"] and
    pl["bwd"]["grid"][1] < c.N * c.C,
    "plane grid with one block row per sample": lambda c, pl: not pl["bwd"]["one_wg"] and
    pl["bwd"]["grid"][1] == c.N * c.C,
    "one workgroup with N*S/4 >= 4096 and not a multiple of 1024":
        lambda c, pl: pl["bwd"]["one_wg"] and pl["bwd"]["vec"] and c.N * B.S(c) // 4 >= 4096 and
        (c.N * B.S(c) // 4) % 1024 != 0,
    "one workgroup with N*S/4 < 256 (idle threads)": lambda c, pl: pl["bwd"]["one_wg"] and pl["bwd"]["vec"] and
    c.N * B.S(c) // 4 < 256,
}
for _op in ("y", "z"):
    EDGES["forward, one workgroup: only %s's stride is odd" % _op] = (
        lambda c, pl, p=_only_odd(_op): p(c, pl) and pl["fwd"]["one_wg"] and not pl["fwd"]["vec"])
for _op in ("dz", "y", "dy"):
    EDGES["backward, one workgroup: only %s's stride is odd" % _op] = (
        lambda c, pl, p=_only_odd(_op): p(c, pl) and pl["bwd"]["one_wg"] and not pl["bwd"]["vec"])
for _op in ("dz", "y", "dy", "z", "dres"):
    EDGES["backward, streaming: only %s's stride is odd" % _op] = (
        lambda c, pl, p=_only_odd(_op): p(c, pl) and not pl["bwd"]["one_wg"] and not pl["bwd"]["vec"])


@pytest.mark.parametrize("edge", list(EDGES))
def test_table_hits_edge(edge):
    hit = [c.name for c, pl in PLANS if EDGES[edge](c, pl)]
    print("\n%s: %s" % (edge, hit))
    assert hit, "no row hits: %s" % edge


def test_an_odd_z_only_matters_where_z_is_read():
    pl = B.plan(B.BY_NAME["one_odd_z"])
    assert not pl["fwd"]["vec"] and pl["bwd"]["vec"]


def test_multi_calls_cut_into_the_intended_launches():
    r = B.runs(B.MULTI["five_small"])
    assert [len(x) for x in r] == [4, 1]
    r = B.runs(B.MULTI["vector_width_splits_a_run"])
    assert [len(x) for x in r] == [2, 2, 1]
    r = B.runs(B.MULTI["large_unit_inside"])
    assert [len(x) for x in r] == [2, 1, 2] and r[1] == ("edge_32772",)
    names = [n for n, _ in B.MULTI_PARTIALS["part_inside"]]
    parts = [p for _, p in B.MULTI_PARTIALS["part_inside"]]
    assert [len(x) for x in B.runs(names, parts)] == [2, 1, 2]


def test_multi_cut_follows_the_switch_and_refuses_bad_arguments(monkeypatch):
    """COCLR_PAIR=0 (read at every call) keeps every unit alone; the query refuses what the launchers refuse."""
    names = B.MULTI["five_small"]
    monkeypatch.setenv("COCLR_PAIR", "0")
    assert [len(x) for x in B.runs(names)] == [1] * 5
    assert [len(x) for x in B.runs(names, [None] * 5)] == [1] * 5
    monkeypatch.delenv("COCLR_PAIR")
    assert [len(x) for x in B.runs(names, [None] * 5)] == [4, 1]
    lib = _lib.load()
    out = (C.c_int32 * 3)()
    farr, barr = (_lib.BnFwdCall * 2)(), (_lib.BnBwdCall * 2)()
    assert lib.coclr_bn_multi_plan(None, None, 2, out) == 1
    assert lib.coclr_bn_multi_plan(farr, barr, 2, out) == 1
    assert lib.coclr_bn_multi_plan(farr, None, 0, out) == 1
    assert lib.coclr_bn_multi_plan(farr, None, 2, None) == 1
    assert lib.coclr_bn_multi_plan(farr, None, 2, out) == 1            # N = 0, null operands
    assert lib.coclr_bn_multi_plan(None, barr, 2, out) == 1


def test_partials_cover_one_and_two_arrays_and_a_ragged_tile_count():
    counts = [t for _, t in B.PARTIALS.values()]
    assert {len(t) for t in counts} == {1, 2}
    assert any(n % 256 != 0 and n > 256 for t in counts for n in t) and any(n < 256 for t in counts for n in t)
    assert set(B.FINALIZE_NTILES) == {1, 3, 300}


def test_multi_argument_refusals():
    lib = _lib.load()
    assert lib.coclr_bn_finalize_apply_multi(None, 1, None) == 1
    assert lib.coclr_bn_act_backward_multi(None, 1, None) == 1
    arr = (_lib.BnBwdCall * 1)()
    assert lib.coclr_bn_act_backward_multi(arr, 0, None) == 1
    assert lib.coclr_bn_act_backward_multi(arr, 1, None) == 1          # N = 0, null operands
    farr = (_lib.BnFwdCall * 1)()
    assert lib.coclr_bn_finalize_apply_multi(farr, 1, None) == 1


def test_non_temporal_switch():
    """COCLR_BN_NT_MB is read once per process: a fresh interpreter with -1 plans every pass temporal, one with a
    threshold plans by size."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import _bn_cases as B; "
            "print([(B.plan(B.BY_NAME[n])['fwd']['nt'], B.plan(B.BY_NAME[n])['bwd']['nt']) "
            "for n in ('large_stream', 'grid_gx2', 'str_scalar_s15')])" %
            (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

    def run(value):
        env = dict(os.environ, COCLR_BN_NT_MB=value)
        return subprocess.check_output([sys.executable, "-c", code], env=env).decode().strip()

    assert run("-1") == "[(False, False), (False, False), (False, False)]"
    assert run("0") == "[(True, True), (True, True), (False, False)]"
    assert run("1") == "[(False, False), (False, False), (False, False)]"      # all below 1 MB
