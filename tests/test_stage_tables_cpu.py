"""The host side of the staging and of the JPEG path against its recorded results (tests/golden/stage_tables.pt, written
by tools/make_stage_tables_golden.py from the code as it stood BEFORE the one-size and the ragged functions were given
one body each): descriptor rows, axis tables, program tables, concatenated packs, checked geometry and decode stages of
the batches the CPU and the GPU tier share, element by element -- same structure, same dtypes, same scalars, same bytes.
Then the refusals of the six ctypes wrappers that take a descriptor, on CPU tensors, before the library is asked for."""
import os
import sys

import pytest
import torch

import _jpeg_cases as J
from coclr_amd import _lib, jpeg, ops

sys.path.insert(0, os.path.join(J.ROOT, "tools"))
import make_stage_tables_golden as G        # noqa: E402

GOLDEN = torch.load(G.OUT)
_NOW = {}


def now():
    if not _NOW:
        _NOW.update(G.entries())
    return _NOW


def same(got, want, where):
    """`got` (frozen by the tool, as `want` was) equals `want` in structure, type and value."""
    assert type(got) is type(want), where
    if torch.is_tensor(want):
        assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), where
    elif isinstance(want, list):
        assert len(got) == len(want), where
        for k, (g, w) in enumerate(zip(got, want)):
            same(g, w, "%s[%d]" % (where, k))
    else:                                               # a scalar, a refusal's name, or a large tensor's digest
        assert got == want, where


def test_every_recorded_entry_is_recomputed():
    assert sorted(now()) == sorted(GOLDEN) and len(GOLDEN) >= 30
    for prefix in ("train_tables", "train_tables_ragged", "classifier_tables/", "classifier_tables_ragged/",
                   "program_tables/", "augment_tables/", "cat/", "cat_ragged/", "check_meta/", "check_meta_ragged/",
                   "ragged_plan/"):
        assert any(name.startswith(prefix) for name in GOLDEN), prefix
    # the one-size functions refuse the mixed list, and are recorded as refusing it
    assert GOLDEN["cat/mixed"] == "raises Unsupported" and GOLDEN["check_meta/mixed"] == "raises ValueError"
    assert not isinstance(GOLDEN["cat/one_size"], str) and not isinstance(GOLDEN["check_meta/one_size"], str)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_host_result_is_the_recorded_one(name):
    same(now()[name], GOLDEN[name], name)


def test_freeze_keeps_what_the_comparison_needs():
    """The tool's digest of a large tensor covers shape, dtype and every byte; small tensors and scalars are kept."""
    t = torch.arange(G.KEEP + 1, dtype=torch.int32)
    d = G.freeze(t)
    assert d["shape"] == (G.KEEP + 1,) and d["dtype"] == "torch.int32"
    changed = t.clone()
    changed[-1] += 1
    assert G.freeze(changed) != d and G.freeze(t.to(torch.int64)) != d and G.freeze(t.view(1, -1)) != d
    small = G.freeze((torch.arange(3), True, 1))
    assert torch.equal(small[0], torch.arange(3)) and small[1] is True and small[2] == 1
    with pytest.raises(AssertionError):
        same([1], [True], "bool against int")


# ---- the wrappers' refusals ------------------------------------------------------------------------------------------

T, SIZE, S = 2, 8, 6
i32 = torch.int32
REACHED = (AssertionError, _lib.HipLibraryError)        # the library asked for, or a host tensor's pointer: past every check


class OnDevice:
    """A host tensor that says it is on the device, as far as the wrappers' checks ask: this tier has no GPU."""
    is_cuda = True

    def __init__(self, t):
        self.t = t

    def __getattr__(self, name):
        return getattr(self.t, name)


def _resize_args(fields, ragged):
    """Well-formed CPU arguments of a resize wrapper for 3 clips; `fields` words per descriptor."""
    src = torch.zeros(4096, dtype=torch.uint8) if ragged else torch.zeros(3 * T, 5, 7, 3, dtype=torch.uint8)
    desc = torch.zeros(3, fields, dtype=i32)
    return {"src": src, "desc": desc, "desc_host": desc.clone(), "xtab": torch.zeros(64, dtype=i32),
            "ytab": torch.zeros(64, dtype=i32)}


def _boxes(fn, fields, ragged, **bad):
    a = dict(_resize_args(fields, ragged), out=torch.zeros(3 * T, S, S, 3, dtype=torch.uint8))
    a.update(bad)
    fn(a["src"], a["desc"], a["desc_host"], a["xtab"], a["ytab"], T, S, a["out"])


def _resize2(fn, fields, ragged, **bad):
    a = dict(_resize_args(fields, ragged), tab2=torch.zeros(3, 8, dtype=i32), mean=None, std=None,
             out=torch.zeros(3 * T, S, S, 3, dtype=torch.uint8))
    a.update(bad)
    fn(a["src"], a["desc"], a["desc_host"], a["xtab"], a["ytab"], a["tab2"], T, SIZE, S, a["out"], a["mean"], a["std"])


def _resize_cases():
    rows = []
    for call, name, fields, other, ragged in ((_boxes, "resize_boxes_u8", 10, 14, False),
                                              (_boxes, "resize_boxes_ragged_u8", 14, 10, True),
                                              (_resize2, "resize2_boxes", 14, 18, False),
                                              (_resize2, "resize2_boxes_ragged", 18, 14, True)):
        wide = torch.zeros(3, other, dtype=i32)
        strided = torch.zeros(3, 2 * fields, dtype=i32)[:, ::2]
        bad = [("width", {"desc": wide, "desc_host": wide.clone()}),
               ("strided", {"desc": strided}), ("strided_host", {"desc_host": strided}),
               ("host_dtype", {"desc_host": torch.zeros(3, fields, dtype=torch.int64)}),
               ("host_device", {"desc_host": OnDevice(torch.zeros(3, fields, dtype=i32))}),
               ("out_u8", {"out": torch.zeros(3 * T, S, S + 1, 3, dtype=torch.uint8)})]
        if call is _resize2:
            f32 = torch.zeros(3, 3, T, S, S)
            bad += [("out_f32", {"out": torch.zeros(3, 3, T, S, S + 1), "mean": (0.5,) * 3, "std": (0.5,) * 3}),
                    ("no_mean", {"out": f32, "std": (0.5,) * 3}), ("no_std", {"out": f32, "mean": (0.5,) * 3})]
        rows += [pytest.param(call, name, fields, ragged, kw, id="%s-%s" % (name, why)) for why, kw in bad]
    return rows


@pytest.fixture
def no_library(monkeypatch):
    def touched():
        raise AssertionError("the wrapper asked for the library before it refused")
    monkeypatch.setattr(ops, "_L", touched)


@pytest.mark.parametrize("call,name,fields,ragged,bad", _resize_cases())
def test_resize_wrapper_refuses_before_the_library(call, name, fields, ragged, bad, no_library):
    with pytest.raises(ValueError):
        call(getattr(ops, name), fields, ragged, **bad)
    # and the arguments the case was derived from get past every check, to the library itself
    with pytest.raises(REACHED):
        call(getattr(ops, name), fields, ragged, **({"out": torch.zeros(3, 3, T, S, S), "mean": (0.5,) * 3,
                                                    "std": (0.5,) * 3} if "mean" in bad or "std" in bad else {}))


def _decode(ragged, why=None):
    packs = [jpeg.pack([J.raw(J.case(n))]) for n in G.MIXED[:1] * 2]
    data, meta = jpeg.cat(packs)
    host = meta[:, 8:].contiguous()
    a = {"data": data, "meta": host.clone(), "meta_host": host, "status": torch.zeros(2, dtype=i32), "chunk_bytes": 0}
    a.update({None: {}, "chunk_bytes": {"chunk_bytes": 7}, "status": {"status": torch.zeros(3, dtype=i32)},
              "strided": {"meta": torch.zeros(2, 2 * host.shape[1], dtype=i32)[:, ::2]},
              "host_dtype": {"meta_host": host.to(torch.int64)}, "host_device": {"meta_host": OnDevice(host)}}[why])
    if ragged:
        geo = jpeg.check_meta_ragged(data, meta)
        _, total, stages, blocks = jpeg.ragged_plan(geo, 256 << 20)
        _, _, geom, prefix = stages[0]
        ops.jpeg_decode_ragged(a["data"], a["meta"], a["meta_host"], geom.clone(), geom, prefix.clone(), prefix,
                               torch.zeros(blocks * 64, dtype=torch.int16), torch.zeros(blocks * 64, dtype=torch.uint8),
                               torch.zeros((total + 15) & ~15, dtype=torch.uint8), a["status"],
                               chunk_bytes=a["chunk_bytes"])
    else:
        H, W, ncomp, hs, vs = jpeg.check_meta(data, meta)
        cb, pb = ops.jpeg_workspace(H, W, ncomp, hs, vs)
        ops.jpeg_decode(a["data"], a["meta"], a["meta_host"], H, W, ncomp, hs, vs,
                        torch.zeros(2 * cb // 2, dtype=torch.int16), torch.zeros(2 * pb, dtype=torch.uint8),
                        torch.zeros(2, H, W, 3, dtype=torch.uint8), a["status"], chunk_bytes=a["chunk_bytes"])


@pytest.mark.parametrize("why", ["chunk_bytes", "status", "strided", "host_dtype", "host_device"])
@pytest.mark.parametrize("ragged", [False, True], ids=["jpeg_decode", "jpeg_decode_ragged"])
def test_decode_wrapper_refuses_before_the_library(ragged, why, no_library):
    with pytest.raises(ValueError):
        _decode(ragged, why)
    with pytest.raises(REACHED):
        _decode(ragged)
