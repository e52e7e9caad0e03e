"""CPU tier of the classifier-clip staging (coclr_amd/staging.py: ClassifierTransform, pack_cls_plan,
classifier_tables, stage_classifier_clips; csrc/staging.hip: coclr_resize2_boxes): the numpy restatement of
tests/cls_harness.py against PIL itself where PIL is installed and against the committed fixture of the reference's
own classifier transform (tests/golden/cls_transform.pt); the draws of ClassifierTransform against the reference's
use of the generator; the host logic on the doubles; every refusal.  Zero tolerance throughout."""
import ctypes as C
import math
import random

import numpy as np
import pytest
import torch

import cls_harness as CL
import crops_harness as CH
import jitter_harness as JH
import train_harness as TH
from coclr_amd import _lib, staging


@pytest.fixture(scope="module")
def gold():
    return CL.golden()


@pytest.fixture(scope="module")
def plans(gold):
    return CL.fixture_plans(gold)


class CountedRandom:
    """Counts the calls `draw` makes, as the fixture's tool counted the reference's module-level calls."""

    def __init__(self, inner, count):
        for name in ("random", "uniform", "shuffle", "randint"):
            setattr(self, name, self._counted(getattr(inner, name), name, count))

    @staticmethod
    def _counted(fn, name, count):
        def call(*a, **kw):
            count[name] += 1
            return fn(*a, **kw)
        return call


# ---- the restatement against PIL itself --------------------------------------------------------------------------

def test_restatement_against_pil():
    Image = pytest.importorskip("PIL.Image")
    fr = CL.frames(2, 40, 52, 1)
    pil = [Image.fromarray(f) for f in fr]

    def arr(imgs):
        return np.stack([np.asarray(i) for i in imgs])
    # crop -> resize -> a second resize, up- and down-sampling, a side equal to size, one-pixel boxes
    for x0, y0, w, h in ((0, 0, 52, 40), (9, 3, 35, 36), (3, 8, 24, 25), (5, 2, 30, 24), (51, 0, 1, 40), (0, 39, 52, 1)):
        first = [i.crop((x0, y0, x0 + w, y0 + h)).resize((24, 24), Image.BICUBIC) for i in pil]
        assert np.array_equal(CL.geometry(fr, (x0, y0, w, h), (24, 24), (0, 0), 24), arr(first)), (x0, y0, w, h)
        for S in (16, 7, 30):
            second = [i.resize((S, S), Image.BICUBIC) for i in first]
            assert np.array_equal(CL.resized_u8(fr, (x0, y0, w, h), (24, 24), (0, 0), 24, S), arr(second)), (w, h, S)
        # the identity case: Scale(24) of a 24 x 24 image returns it, and PIL's resize to the same size copies it
        assert np.array_equal(CL.resized_u8(fr, (x0, y0, w, h), (24, 24), (0, 0), 24, 24), arr(first))
        assert np.array_equal(arr([i.resize((24, 24), Image.BICUBIC) for i in first]), arr(first))
        assert np.array_equal(CH.resize_u8(arr(first), 24), arr(first))         # and so do the identity tables
    # the fallback: the whole frame resized, then the centre window
    for H, W, want in ((8, 96, ((288, 24), (132, 0))), (24, 192, ((192, 24), (84, 0))), (40, 52, ((31, 24), (4, 0))),
                       (52, 40, ((24, 31), (0, 4))), (30, 30, ((24, 24), (0, 0)))):
        fr = CL.frames(2, H, W, H + W)
        (ow, oh), (cx, cy) = want
        whole = [Image.fromarray(f) for f in fr]
        if (ow, oh) != (W, H):
            whole = [i.resize((ow, oh), Image.BICUBIC) for i in whole]
        kept = arr([i.crop((cx, cy, cx + 24, cy + 24)) for i in whole])
        assert staging.fallback_geometry(W, H, 24) == want
        assert np.array_equal(CL.geometry(fr, (0, 0, W, H), (ow, oh), (cx, cy), 24), kept), (H, W)
    # round-half-to-even of the window's corner, as Python 3 rounds in the reference
    assert staging.fallback_geometry(29, 24, 24) == ((29, 24), (2, 0)) and staging.fallback_geometry(27, 24, 24)[1] == (2, 0)
    assert staging.fallback_geometry(320, 240, 224) == ((298, 224), (37, 0))


def test_window_tables_are_the_whole_tables_restricted():
    for n_in, n_out, c0, size in ((96, 288, 132, 24), (8, 24, 0, 24), (52, 24, 0, 24), (320, 298, 37, 224), (17, 30, 3, 22)):
        lo, K = staging.resample_tables(n_in, n_out)
        t = staging._window_table(n_in, n_out, c0, size)
        wl, wk = CL.window_layout(n_in, n_out, c0, size)
        assert torch.equal(torch.from_numpy(t[0]), wl) and torch.equal(torch.from_numpy(t[1:]), wk)
        assert np.array_equal(t[0, :size], lo[c0:c0 + size]) and np.array_equal(t[1:, :size], K[c0:c0 + size].T)
        assert not t[:, size:].any()
    # size -> size: one tap of 2^22 on the sample itself, PIL's identity
    t = staging._window_table(24, 24, 0, 24)
    x = np.arange(24)
    assert all(int(t[1 + i, j]) == (4194304 if t[0, j] + i == j else 0) for j in x for i in range(t.shape[0] - 1))


# ---- the fixture: the reference's own chain --------------------------------------------------------------------

def test_fixture_has_every_case(gold, plans):
    covers = {c for run in gold["runs"] for c in run["covers"]}
    assert covers >= {"box on the first attempt", "box after a miss", "swapped box", "jitter applied", "jitter skipped",
                      "fallback with a resample", "fallback without a resample", "img_dim == size", "validation"}
    assert (gold["size"], gold["img_dim"], gold["seq_len"]) == (24, 16, 3)
    geo = {(run["set"], plan["form"], plan["resample"], plan["window"]) for run, plan, _ in plans}
    assert ("wide8", "fallback", (288, 24), (132, 0)) in geo and ("wide24", "fallback", (192, 24), (84, 0)) in geo
    assert any(g[1] == "box" for g in geo)
    for run, plan, _ in plans:
        S = run["img_dim"]
        assert tuple(run["out"].shape) == (3, S, S, 3) and run["frames"].shape[0] == 3
        assert bool(plan["program"]) == ("jitter applied" in run["covers"])


def test_draws_reproduce_the_fixture(gold, plans):
    """ClassifierTransform.draw under the run's seed yields a plan whose restated chain equals the reference's bytes,
    makes the reference's calls of the generator, and leaves it where the reference left it."""
    for run, plan, after in plans:
        got = CL.chain_u8(run["frames"], plan, gold["size"], run["img_dim"])
        assert np.array_equal(got, run["out"].numpy()), (run["seed"], run["set"])
        assert after == run["next"], (run["seed"], run["set"])
        count = {k: 0 for k in run["draws"]}
        random.seed(run["seed"])
        ct = staging.ClassifierTransform(run["img_dim"], 3, size=gold["size"], mode=run["mode"])
        H, W = run["frames"].shape[1:3]
        again = ct.draw(W, H, rng=CountedRandom(random, count))
        assert count == run["draws"] and again == plan, (run["seed"], run["set"])
        if run["mode"] == "val":
            assert count["shuffle"] == 0 and plan["program"] == []
        # an own generator instead of the module: the same plan
        assert ct.draw(W, H, rng=random.Random(run["seed"])) == plan


def test_tenth_attempt_and_generator_state():
    """Frames of 14 rows x 60 columns under seed 43: nine draws do not fit, the tenth does.  The reference's loop,
    written out, must leave its generator where `draw` leaves its own."""
    W, H, seed = 60, 14, 43
    ref = random.Random(seed)
    ref.random()
    box = None
    for attempt in range(10):
        target_area = ref.uniform(0.2, 1) * (W * H)
        aspect_ratio = ref.uniform(3. / 4, 4. / 3)
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if ref.random() < 0.5:
            w, h = h, w
        if w <= W and h <= H:
            x1 = ref.randint(0, W - w)
            y1 = ref.randint(0, H - h)
            box = (x1, y1, w, h)
            break
    assert attempt == 9 and box is not None
    for mode in ("train", "val"):
        own, count = random.Random(seed), {k: 0 for k in ("random", "uniform", "shuffle", "randint")}
        plan = staging.ClassifierTransform(16, 3, size=24, mode=mode).draw(W, H, rng=CountedRandom(own, count))
        assert plan["form"] == "box" and plan["region"] == box and plan["resample"] == (24, 24) and plan["window"] == (0, 0)
        assert count["randint"] == 2 and count["uniform"] - 4 * count["shuffle"] == 20
        ref2 = random.Random(seed)
        ref2.setstate(ref.getstate())
        if mode == "train":                                   # ColorJitter(p=0.3)'s own draws follow
            jit = staging.ColorJitter(0.4, 0.4, 0.4, 0.1, p=0.3).draw(ref2, 1)[0]
            assert jit == plan["program"] and count["random"] == 12
        else:
            assert plan["program"] == [] and count["random"] == 11 and count["shuffle"] == 0
        assert own.random() == ref2.random()
    # ten misses: nothing further is drawn for the geometry
    own, count = random.Random(0), {k: 0 for k in ("random", "uniform", "shuffle", "randint")}
    plan = staging.ClassifierTransform(16, 3, size=24, mode="val").draw(96, 8, rng=CountedRandom(own, count))
    assert plan == {"form": "fallback", "region": (0, 0, 96, 8), "resample": (288, 24), "window": (132, 0), "program": []}
    assert count == {"random": 11, "uniform": 20, "shuffle": 0, "randint": 0}


def test_construction_and_batch_flip():
    for kw in (dict(mode="test"), dict(size=225), dict(jitter=(-1, 0, 0, 0)), dict(size=0)):
        with pytest.raises(ValueError):
            staging.ClassifierTransform(16, 3, **kw)
    for img_dim in (0, 225):
        with pytest.raises(ValueError):
            staging.ClassifierTransform(img_dim, 3)
    with pytest.raises(ValueError, match="ClassifierTransform"):           # the pretraining class still refuses this mode
        staging.TrainTransform(16, 3, consistent=True)
    ct = staging.ClassifierTransform(128, 32)
    plan = ct.draw(320, 240, rng=random.Random(0))
    x0, y0, w, h = plan["region"]
    assert plan["form"] == "box" and 0 <= x0 and 0 <= y0 and x0 + w <= 320 and y0 + h <= 240 and w * h >= 0.19 * 320 * 240
    a, b = random.Random(4), random.Random(4)
    assert [staging.draw_batch_flip(a) for _ in range(20)] == [b.random() < 0.5 for _ in range(20)]
    assert a.random() == b.random()


def test_pack_round_trip_and_collate(plans):
    each = [p for _, p, _ in plans]
    packed = [staging.pack_cls_plan(p) for p in each]
    assert all(q.shape == (25,) and q.dtype == torch.float64 for q in packed)
    for p, q in zip(each, packed):
        assert staging.unpack_cls_plan(q) == p
    collated = torch.utils.data.default_collate([(run["frames"][:, :8, :8], q) for (run, _, _), q in zip(plans, packed)])
    assert collated[1].shape == (len(each), 25) and collated[1].dtype == torch.float64
    assert [staging.unpack_cls_plan(q) for q in collated[1]] == each
    with pytest.raises(ValueError):
        staging.unpack_cls_plan(torch.zeros(24, dtype=torch.float64))
    with pytest.raises(ValueError):
        staging.pack_cls_plan(dict(each[0], form="rotate"))
    with pytest.raises(ValueError):
        staging.pack_cls_plan(dict(each[0], program=[(1, 1.0)] * 9))
    bad = packed[0].clone()
    bad[3] = 1.5
    with pytest.raises(ValueError):
        staging.unpack_cls_plan(bad)


# ---- the host logic on the doubles -------------------------------------------------------------------------------

def _levels(u8, gold, T):
    return JH.levels_expected(u8, gold["levels"], T)


def test_stage_classifier_clips_on_the_doubles(monkeypatch, gold, plans):
    CL.install(monkeypatch)
    monkeypatch.delenv("COCLR_CLS_FUSED", raising=False)
    size, T = gold["size"], gold["seq_len"]
    for run, plan, _ in plans:
        del CL.CALLS[:], TH.CALLS[:]
        S = run["img_dim"]
        out = staging.stage_classifier_clips(run["frames"], plan, S, size=size, device="cpu")
        assert out.shape == (1, 3, T, S, S) and out.dtype == torch.float32
        assert torch.equal(out, _levels(run["out"].numpy(), gold, T)), (run["seed"], run["set"])
        if plan["program"]:                                    # two launches: bytes, then the program per clip
            assert CL.CALLS == [("resize2", 1, T, "u8")] and [c[:3] for c in TH.CALLS] == [("augment", T, T)]
            assert [(int(k), v) for k, v in TH.CALLS[0][3][0] if k] == [(k, float(np.float32(v))) for k, v in plan["program"]]
        else:                                                  # validation, or a jitter draw that said no: one launch
            assert CL.CALLS == [("resize2", 1, T, "f32")] and not TH.CALLS
        # the batch flip: kind 7 behind every clip's program, and always two launches
        del CL.CALLS[:], TH.CALLS[:]
        flipped = staging.stage_classifier_clips(run["frames"], plan, S, flip=True, size=size, device="cpu")
        assert CL.CALLS == [("resize2", 1, T, "u8")] and [c[:3] for c in TH.CALLS] == [("augment", T, T)]
        prog = [(int(k), v) for k, v in TH.CALLS[0][3][0]]
        assert prog[len(plan["program"])][0] == 7 and [k for k, _ in prog[:len(plan["program"])]] == [k for k, _ in plan["program"]]
        assert torch.equal(flipped, out.flip(-1))
    # a batch of the runs that share frames and img_dim, every sample with its own plan; packed plans through the
    # default collate give the same
    picked = [(run, plan) for run, plan, _ in plans if run["set"] == "main" and run["img_dim"] == 16]
    assert len(picked) >= 3 and any(p["program"] for _, p in picked) and any(not p["program"] for _, p in picked)
    frames = torch.stack([run["frames"].flip(0) if i % 2 else run["frames"] for i, (run, _) in enumerate(picked)])
    each = [p for _, p in picked]
    del CL.CALLS[:], TH.CALLS[:]
    batch = staging.stage_classifier_clips(frames, each, 16, size=size, device="cpu")
    assert CL.CALLS == [("resize2", len(each), T, "u8")] and [c[:3] for c in TH.CALLS] == [("augment", len(each) * T, T)]
    assert torch.equal(batch, CL.chain_reference(frames.numpy(), each, size, 16))
    collated = torch.utils.data.default_collate([(f, staging.pack_cls_plan(p)) for f, p in zip(frames, each)])
    assert torch.equal(staging.stage_classifier_clips(collated[0], collated[1], 16, size=size, device="cpu"), batch)
    out = torch.empty_like(batch)
    assert staging.stage_classifier_clips(frames, each, 16, size=size, out=out, device="cpu") is out and torch.equal(out, batch)
    # tables computed ahead: the plans are not read
    tables = staging.classifier_tables(each, len(each), T, 52, 40, 16, size=size, flip=True)
    assert tuple(tables[0].shape) == (len(each), 14) and tables[6] is False
    ahead = staging.stage_classifier_clips(frames, None, 16, size=size, device="cpu", tables=tables)
    assert torch.equal(ahead, CL.chain_reference(frames.numpy(), each, size, 16, flip=True))
    # validation plans only: one launch for the whole batch
    val = [dict(p, program=[]) for p in each]
    del CL.CALLS[:], TH.CALLS[:]
    got = staging.stage_classifier_clips(frames, val, 16, size=size, device="cpu")
    assert CL.CALLS == [("resize2", len(each), T, "f32")] and not TH.CALLS
    assert torch.equal(got, CL.chain_reference(frames.numpy(), val, size, 16))


def test_chained_switch_on_the_doubles(monkeypatch, gold, plans):
    """COCLR_CLS_FUSED=0: the same tensors from two coclr_resize_boxes_u8 launches and coclr_augment_clips; the
    fallback form is refused."""
    CL.install(monkeypatch)
    size, T = gold["size"], gold["seq_len"]
    assert staging.cls_fused()
    monkeypatch.setenv("COCLR_CLS_FUSED", "0")
    assert not staging.cls_fused()
    for run, plan, _ in plans:
        del CL.CALLS[:], TH.CALLS[:]
        S = run["img_dim"]
        if plan["form"] == "fallback":
            with pytest.raises(ValueError, match="fallback"):
                staging.stage_classifier_clips(run["frames"], plan, S, size=size, device="cpu")
            assert not CL.CALLS and not TH.CALLS
            continue
        out = staging.stage_classifier_clips(run["frames"], plan, S, size=size, device="cpu")
        assert not CL.CALLS and [c[0] for c in TH.CALLS] == ["boxes", "boxes", "augment"]
        assert torch.equal(out[0], _levels(run["out"].numpy(), gold, T)[0]), (run["seed"], run["set"])


def test_stage_classifier_clips_refusals(monkeypatch, gold, plans):
    CL.install(monkeypatch)
    monkeypatch.delenv("COCLR_CLS_FUSED", raising=False)
    run, plan, _ = [x for x in plans if x[0]["set"] == "main"][0]
    fr = run["frames"]                                                                     # 40 rows x 52 columns

    def changed(**kw):
        return dict(plan, **kw)
    bad = [changed(region=(40, 0, 16, 16)), changed(region=(0, 30, 20, 11)), changed(region=(0, 0, 0, 5)),
           changed(region=(-1, 0, 5, 5)), changed(region=(0, 0, 5.5, 5)),                  # a box outside the frame
           changed(form="fallback", region=(0, 0, 52, 40), resample=(31, 24), window=(8, 0)),    # a window outside (ow, oh)
           changed(form="fallback", region=(0, 0, 52, 40), resample=(31, 24), window=(0, 1)),
           changed(form="fallback", region=(0, 0, 52, 40), resample=(31, 24), window=(-1, 0)),
           changed(form="fallback", region=(0, 0, 52, 40), resample=(23, 24), window=(0, 0)),
           changed(resample=(31, 24)), changed(window=(1, 0)),                             # a box keeps all of (size, size)
           changed(form="rotate"),
           changed(program=[(8, 1.0)]), changed(program=[(6, 0.25)]), changed(program=[(7, 0)]),   # what program_tables refuses
           changed(program=[(4, 1.5)]), changed(program=[(1, float("nan"))]), changed(program=[(1, 1.0)] * 9)]
    for b in bad:
        with pytest.raises(ValueError):
            staging.stage_classifier_clips(fr, b, 16, size=24, device="cpu")
    # a side that needs more taps than the kernel takes: 40 rows to 1 is 161 taps
    tall = torch.zeros(3, 4000, 30, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="taps"):
        staging.stage_classifier_clips(tall, dict(plan, region=(0, 0, 30, 4000)), 16, size=24, device="cpu")
    with pytest.raises(ValueError, match="taps"):
        staging.stage_classifier_clips(fr, dict(plan, resample=(224, 224)), 1, size=224, device="cpu")   # 224 -> 1: stage 2
    for kw in (dict(img_dim=225), dict(img_dim=16, size=225), dict(img_dim=0), dict(img_dim=16, size=0)):
        with pytest.raises(ValueError):
            staging.stage_classifier_clips(fr, plan, device="cpu", **dict(dict(size=24), **kw))
    with pytest.raises(ValueError):
        staging.stage_classifier_clips(fr, [plan, plan], 16, size=24, device="cpu")           # two plans, one sample
    with pytest.raises(ValueError):
        staging.stage_classifier_clips(fr.float(), plan, 16, size=24, device="cpu")
    with pytest.raises(ValueError):
        staging.stage_classifier_clips(fr[..., :2], plan, 16, size=24, device="cpu")
    with pytest.raises(ValueError):
        staging.stage_classifier_clips(fr, plan, 16, size=24, out=torch.empty(1, 3, 3, 16, 15), device="cpu")
    with pytest.raises(ValueError):                                                         # tables of another batch
        staging.stage_classifier_clips(fr, None, 16, size=24, device="cpu",
                                       tables=staging.classifier_tables([plan, plan], 2, 3, 52, 40, 16, size=24))
    assert not CL.CALLS and not TH.CALLS                                                    # refused before any call


def test_entry_point_refusals():
    """coclr_resize2_boxes validates on the host before anything is launched: no GPU is needed to be refused.  The
    addition is additive: the ABI number stays."""
    assert _lib.ABI_VERSION == 26 and "coclr_resize2_boxes" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert lib.coclr_abi_version() == 26
    p = C.c_void_p(4096)
    P, Sp = 24, 16
    #           first T  x0 y0 w   h   ow  oh  cx   cy xoff yoff xt yt
    hd = [0, 3, 5, 4, 30, 28, 24, 24, 0, 0, 0, 0, 9, 9,
          3, 3, 0, 0, 52, 40, 288, 24, 132, 0, 240, 240, 5, 11]
    args = dict(frames=p, F=6, H=40, W=52, desc=p, hd=hd, n_clips=2, T=3, size=24, S=16, xtab=p, xlen=240 + P * 6,
                ytab=p, ylen=240 + P * 12, tab2=p, len2=Sp * 8, taps2=7, mean=[0.5, 0.5, 0.5], std=[0.2, 0.2, 0.2],
                out8=None, out=p)

    def call(**kw):
        a = dict(args, **kw)
        d = None if a["hd"] is None else (C.c_int32 * len(a["hd"]))(*a["hd"])
        mean = None if a["mean"] is None else (C.c_float * 3)(*a["mean"])
        std = None if a["std"] is None else (C.c_float * 3)(*a["std"])
        return lib.coclr_resize2_boxes(a["frames"], a["F"], a["H"], a["W"], a["desc"], d, a["n_clips"], a["T"], a["size"],
                                       a["S"], a["xtab"], a["xlen"], a["ytab"], a["ylen"], a["tab2"], a["len2"], a["taps2"],
                                       mean, std, a["out8"], a["out"], None)

    def desc(k, field, value):
        d = list(hd)
        d[k * 14 + field] = value
        return d
    for name in ("frames", "desc", "hd", "xtab", "ytab", "tab2", "out", "mean", "std"):     # null pointers
        assert call(**{name: None}) == 1, name
    assert call(out8=p) == 1                                                                 # both outputs
    assert call(out8=None, out=None) == 1
    for name in ("F", "H", "W", "n_clips", "T", "size", "S"):                                # zero or negative sizes
        assert call(**{name: 0}) == 1 and call(**{name: -2}) == 1, name
    assert call(S=225) == 1 and call(size=225) == 1 and call(size=225, S=225) == 1           # S or size over 224
    assert call(xtab=C.c_void_p(4100)) == 1 and call(ytab=C.c_void_p(4104)) == 1 and call(tab2=C.c_void_p(4108)) == 1
    assert call(std=[0.2, 0.0, 0.2]) == 1
    # a region outside its frame
    assert call(hd=desc(0, 2, 23)) == 1 and call(hd=desc(0, 3, 13)) == 1 and call(hd=desc(1, 4, 53)) == 1
    assert call(hd=desc(0, 2, -1)) == 1 and call(hd=desc(0, 4, 0)) == 1 and call(hd=desc(1, 5, 41)) == 1
    # a window outside its resample
    assert call(hd=desc(1, 8, 265)) == 1 and call(hd=desc(1, 9, 1)) == 1 and call(hd=desc(1, 8, -1)) == 1
    assert call(hd=desc(0, 6, 23)) == 1 and call(hd=desc(0, 7, 0)) == 1 and call(hd=desc(0, 9, -3)) == 1
    # tap counts over the limit
    assert call(hd=desc(0, 12, 0)) == 1 and call(hd=desc(0, 12, 65)) == 1 and call(hd=desc(1, 13, 0)) == 1
    assert call(hd=desc(1, 13, 65)) == 1 and call(taps2=0) == 1 and call(taps2=65, len2=Sp * 66) == 1
    # frames
    assert call(hd=desc(0, 0, 4)) == 1 and call(hd=desc(0, 0, -1)) == 1 and call(hd=desc(0, 1, 2)) == 1
    # a table offset past the buffer, or not a multiple of 4
    assert call(hd=desc(1, 10, 241)) == 1 and call(hd=desc(1, 10, 244)) == 1 and call(hd=desc(1, 11, -4)) == 1
    assert call(hd=desc(1, 11, 244)) == 1
    assert call(xlen=240 + P * 6 - 1) == 1 and call(ylen=47) == 1 and call(len2=Sp * 8 - 1) == 1
    assert call(n_clips=2, T=40000, hd=desc(0, 1, 40000)) == 1
    with pytest.raises(_lib.HipLibraryError):                        # and the binding has no CPU path
        staging.stage_classifier_clips(torch.zeros(2, 30, 30, 3, dtype=torch.uint8),
                                       {"form": "box", "region": (0, 0, 30, 30), "resample": (24, 24), "window": (0, 0),
                                        "program": []}, 16, size=24, device="cpu")
