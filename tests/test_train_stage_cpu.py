"""CPU tier of the training-clip staging (coclr_amd/staging.py: TrainTransform, blur_box_radius, augment_tables,
stage_train_clips; csrc/staging.hip: coclr_augment_clips, coclr_resize_boxes_u8): the numpy restatement of
tests/train_harness.py against PIL's own GaussianBlur where PIL is installed and against the committed fixture of
the reference's own training transform (tests/golden/train_transform.pt); the draws of TrainTransform against the
reference's use of both generators; the host logic on the doubles; every refusal.  Zero tolerance throughout."""
import ctypes as C
import math
import random

import numpy as np
import pytest
import torch

import crops_harness as CH
import jitter_harness as JH
import train_harness as TH
from coclr_amd import _lib, staging


@pytest.fixture(scope="module")
def gold():
    return TH.golden()


@pytest.fixture(scope="module")
def plans(gold):
    return TH.fixture_plans(gold)


# ---- the blur against PIL itself ---------------------------------------------------------------------------------

ROOT2 = math.sqrt(2.0)          # where the box radius' integer part l steps from 0 to 1 -- in PIL's floats
BELOW, ABOVE = float(np.float32(ROOT2)), float(np.nextafter(np.float32(ROOT2), np.float32(2)))      # fp32 neighbours
SIGMAS = [0.0, 0.05, 0.1, 0.3, 0.5, 0.75, 1.0, 1.2, 1.4, 1.41, 1.414, 1.4142, BELOW, float(np.nextafter(ROOT2, 0)), ROOT2, ABOVE,
          1.42, 1.6, 1.8, 2.0, 3.0, 5.5, 9.0, 12.0]


def _blur_inputs(H, W):
    rng = np.random.RandomState(H * 1000 + W)
    out = [rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8),
           (rng.randint(0, 2, size=(H, W, 3)) * 255).astype(np.uint8)]
    for y, x in ((0, 0), (H // 2, W // 2), (H - 1, W - 1)):
        f = np.zeros((H, W, 3), dtype=np.uint8)
        f[y, x] = (255, 200, 255)
        out.append(f)
    return out


@pytest.mark.parametrize("H,W", [(128, 128), (17, 33), (7, 5), (9, 1), (3, 3)])
def test_blur_restatement_against_pil(H, W):
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageFilter
    for f in _blur_inputs(H, W):
        for sigma in SIGMAS:
            want = np.asarray(Image.fromarray(f).filter(ImageFilter.GaussianBlur(radius=sigma)))
            got = TH.blur_u8(f, TH.box_radius(sigma))
            assert int((want != got).sum()) == 0, (sigma, H, W)
            assert np.array_equal(TH.blur_u8(f, staging.blur_box_radius(sigma)), got)
    assert any(int(TH.box_radius(s)) >= 2 for s in SIGMAS) and int(TH.box_radius(12.0)) + 1 > 9       # lines shorter than r + 1


def test_blur_box_radius():
    # the formula's value is 0.25 at sigma 1 and 1.375 at sigma 2; PIL's C evaluates it in floats, which lands one
    # fp32 unit (2^-25) off the former and on the latter -- and the bytes below follow PIL, not the formula
    assert abs(staging.blur_box_radius(1) - 0.25) <= 2.0 ** -25 and staging.blur_box_radius(2) == 1.375
    assert staging.blur_box_radius(0) == 0.0
    # in PIL's floats sigma^2 / 3 of the fp32 value just below sqrt(2) already rounds to 2/3: l steps there
    assert BELOW < ROOT2 < ABOVE and [int(staging.blur_box_radius(s)) for s in (1.414, 1.4142, BELOW, ROOT2, ABOVE)] == \
        [0, 0, 1, 1, 1]
    for sigma in SIGMAS + np.random.RandomState(0).uniform(0.1, 2, 200).tolist():
        r = staging.blur_box_radius(sigma)
        assert isinstance(r, float) and np.float32(r) == TH.box_radius(sigma) and r == float(np.float32(r))
    assert abs(staging.blur_box_radius(0.1) - 0.00167) < 1e-5          # the reference's range: 0.00167 .. 1.375
    r, ww, fw = TH.box_weights(0.0)
    assert (r, ww, fw) == (0, 1 << 24, 0)                              # the identity
    f = TH.frames(1, 9, 11, 3)[0]
    assert np.array_equal(TH.blur_u8(f, 0.0), f)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            staging.blur_box_radius(bad)


def test_flip_commutes_with_every_op():
    """Why the kernel may apply an odd number of flips at the final store alone."""
    f = TH.frames(1, 10, 13, 5)[0]
    ops_ = [(1, 1.3), (2, 0.7), (3, 1.4), (4, 23), (5, 1), (TH.BLUR, 0.25), (TH.BLUR, 1.375), (TH.BLUR, 3.7)]
    for op in ops_:
        assert np.array_equal(TH.apply_program(f, [op, (TH.FLIP, 0)]), TH.apply_program(f, [(TH.FLIP, 0), op])), op
    assert np.array_equal(TH.apply_program(f, [(TH.FLIP, 0), (TH.FLIP, 0)]), f)


# ---- the fixture: the reference's own chain --------------------------------------------------------------------

class CountedRandom:
    """Counts the calls `draw` makes, as the fixture's tool counted the reference's module-level calls."""

    def __init__(self, inner, names, count):
        for name in names:
            setattr(self, name, self._counted(getattr(inner, name), name, count))

    @staticmethod
    def _counted(fn, name, count):
        def call(*a, **kw):
            count[name] += 1
            return fn(*a, **kw)
        return call


def test_fixture_has_every_case(gold, plans):
    covers = {c for run in gold["runs"] for c in run["covers"]}
    assert covers >= {"two clips", "one clip", "one clip, half 0", "one clip, half 1", "base on clip 0",
                      "null on clip 0", "base on clip 1", "null on clip 1", "jitter applied", "jitter skipped", "gray",
                      "gray, channels differ", "blur r = 0", "blur r = 1", "flip", "box does not fit"}
    assert gold["img_dim"] == 16 and gold["seq_len"] == 3
    for run in gold["runs"]:
        assert tuple(run["frames"].shape) == (6, 40, 52, 3) and tuple(run["out"].shape) == (6, 16, 16, 3)
    # and the plans say the same
    kinds = [[k for k, _ in p] for _, plan, _ in plans for c in range(2) for p in plan["programs"][c]]
    assert any(6 in k for k in kinds) and any(7 in k for k in kinds) and any(5 in k for k in kinds)
    radii = {int(v) for _, plan, _ in plans for c in range(2) for k, v in plan["programs"][c][0] if k == 6}
    assert radii == {0, 1}
    assert any(plan["box"][c] == (0, 0, 52, 40) for _, plan, _ in plans for c in range(2))
    assert {plan["half"] for _, plan, _ in plans} == {(0, 1), (0, 0), (1, 1)}


def test_draws_reproduce_the_fixture(gold, plans):
    """TrainTransform.draw under the run's seeds yields a plan whose restated chain equals the reference's bytes,
    makes the reference's calls of both generators, and leaves both where the reference left them."""
    tt = staging.TrainTransform(gold["img_dim"], gold["seq_len"])
    for run, plan, after in plans:
        got = TH.chain_u8(run["frames"], plan, gold["img_dim"])
        assert np.array_equal(got, run["out"].numpy()), run["seed"]
        assert after == (run["next"], run["np_next"]), run["seed"]
        count = {k: 0 for k in run["draws"]}
        random.seed(run["seed"])
        np.random.seed(run["seed"])
        again = tt.draw(52, 40, rng=CountedRandom(random, ("random", "uniform", "shuffle", "randint", "choices"), count),
                        np_rng=CountedRandom(np.random, ("choice",), count))
        assert count == run["draws"] and again == plan, run["seed"]
        assert any(not np.array_equal(got[i], got[0]) for i in range(1, 6))
    # an own generator instead of the module: the same plan
    r, n = random.Random(5), np.random.RandomState(5)
    assert tt.draw(52, 40, rng=r, np_rng=n) == [p for run, p, _ in plans if run["seed"] == 5][0]


def test_train_transform_construction():
    for kw in (dict(consistent=True), dict(p=0.5), dict(blur_sigma=(0.1, 40.0)), dict(jitter=(-1, 0, 0, 0))):
        with pytest.raises(ValueError):
            staging.TrainTransform(16, 3, **kw)
    with pytest.raises(ValueError):
        staging.TrainTransform(0, 3)
    tt = staging.TrainTransform(128, 32)
    plan = tt.draw(320, 240, rng=random.Random(0), np_rng=np.random.RandomState(0))
    assert all(len(plan["programs"][c]) == 32 for c in range(2))
    for c in range(2):
        x0, y0, w, h = plan["box"][c]
        assert 0 <= x0 and 0 <= y0 and x0 + w <= 320 and y0 + h <= 240 and w * h >= 0.19 * 320 * 240


# ---- the host logic on the doubles -------------------------------------------------------------------------------

def test_stage_train_clips_on_the_doubles(monkeypatch, gold, plans):
    TH.install(monkeypatch)
    S, T = gold["img_dim"], gold["seq_len"]
    for run, plan, _ in plans:
        del TH.CALLS[:], JH.CALLS[:], CH.CALLS[:]
        out = staging.stage_train_clips(run["frames"], plan, S, device="cpu")
        assert [c[0] for c in TH.CALLS] == ["boxes", "augment"] and not JH.CALLS and not CH.CALLS
        assert TH.CALLS[0][1:] == (2, T)
        per_frame = any(p != progs[0] for progs in plan["programs"] for p in progs)     # a gray clip: a channel per frame
        assert TH.CALLS[1][1:3] == (2 * T, 1 if per_frame else T)
        assert out.shape == (1, 2, 3, T, S, S) and out.dtype == torch.float32
        assert torch.equal(out[0], TH.levels_expected(run["out"].numpy(), gold["levels"], T)), run["seed"]
    # a batch: every sample with its own plan; packed plans through the default collate give the same
    frames = torch.stack([run["frames"].flip(0) if i % 2 else run["frames"] for i, (run, _, _) in enumerate(plans)])
    each = [p for _, p, _ in plans]
    del TH.CALLS[:]
    batch = staging.stage_train_clips(frames, each, S, device="cpu")
    assert [c[0] for c in TH.CALLS] == ["boxes", "augment"] and TH.CALLS[0][1:] == (2 * len(each), T)
    assert torch.equal(batch, TH.chain_reference(frames.numpy(), each, S))
    packed = [staging.pack_plan(p, T) for p in each]
    assert all(p.shape == (2, 5 + 16 * T) and p.dtype == torch.float64 for p in packed)
    for p, q in zip(each, packed):
        back = staging.unpack_plan(q)
        assert back["half"] == tuple(p["half"]) and back["box"] == tuple(p["box"])
        assert [list(x) for x in back["programs"]] == [list(x) for x in p["programs"]]
    collated = torch.utils.data.default_collate([(f, q) for f, q in zip(frames, packed)])
    assert collated[1].shape == (len(each), 2, 5 + 16 * T)
    assert torch.equal(staging.stage_train_clips(collated[0], collated[1], S, device="cpu"), batch)
    out = torch.empty_like(batch)
    assert staging.stage_train_clips(frames, each, S, out=out, device="cpu") is out and torch.equal(out, batch)


def test_stage_train_clips_refusals(monkeypatch, gold, plans):
    TH.install(monkeypatch)
    run, plan, _ = plans[0]
    fr = run["frames"]

    def changed(**kw):
        return dict(plan, **kw)
    box = plan["box"]
    bad = [changed(half=(0, 2)), changed(box=(box[0], (40, 0, 16, 16))), changed(box=((0, 30, 20, 11), box[1])),
           changed(box=(box[0], (0, 0, 0, 5))), changed(box=((-1, 0, 5, 5), box[1])),
           changed(programs=(plan["programs"][0], plan["programs"][1][:2])),
           changed(programs=([[(8, 1.0)]] * 3, plan["programs"][1])),
           changed(programs=([[(6, 16.5)]] * 3, plan["programs"][1])),
           changed(programs=([[(6, -0.5)]] * 3, plan["programs"][1])),
           changed(programs=([[(6, float("nan"))]] * 3, plan["programs"][1])),
           changed(programs=([[(1, 1.0)] * 9] * 3, plan["programs"][1]))]
    for b in bad:
        with pytest.raises(ValueError):
            staging.stage_train_clips(fr, b, 16, device="cpu")
    with pytest.raises(ValueError):
        staging.stage_train_clips(fr, [plan, plan], 16, device="cpu")                 # two plans, one sample
    with pytest.raises(ValueError):
        staging.stage_train_clips(fr[:5], plan, 16, device="cpu")                     # an odd number of frames
    with pytest.raises(ValueError):
        staging.stage_train_clips(fr.float(), plan, 16, device="cpu")
    with pytest.raises(ValueError):
        staging.stage_train_clips(fr, plan, 225, device="cpu")
    with pytest.raises(ValueError):
        staging.stage_train_clips(fr, plan, 16, out=torch.empty(1, 2, 3, 3, 16, 15), device="cpu")
    assert not TH.CALLS                                                               # refused before any call
    # augment_tables admits 6 and 7 and nothing further; program_tables stays as it was
    k, p = staging.augment_tables([[(6, 1.375), (7, 0)], [(2, 0.5)]])
    assert k.tolist() == [[6, 7], [2, 0]] and p.tolist() == [[1.375, 0.0], [0.5, 0.0]]
    for prog in ([(6, 0.25)], [(7, 0)]):
        with pytest.raises(ValueError):
            staging.program_tables([prog])
        with pytest.raises(ValueError):
            staging.color_jitter(fr, [prog], 6, 3, device="cpu")
    for prog in ([(8, 0)], [(-1, 0)], [(6, 16.5)], [(6, -0.5)], [(6, float("nan"))], [(4, 1.5)], [(True, 1.0)]):
        with pytest.raises(ValueError):
            staging.augment_tables([prog])
    out = staging.augment(fr, [[(6, 0.25), (7, 0)]], 6, 3, device="cpu")
    assert torch.equal(out, TH.reference(fr, [[(6, 0.25), (7, 0)]], 6, 3)) and TH.CALLS[-1][0] == "augment"


def test_entry_point_refusals():
    """coclr_augment_clips and coclr_resize_boxes_u8 validate on the host before anything is launched: no GPU is
    needed to be refused.  The additions are additive: the ABI number and the old entry points' limits stay."""
    assert _lib.ABI_VERSION == 26
    for name in ("coclr_augment_clips", "coclr_resize_boxes_u8"):
        assert name in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert lib.coclr_abi_version() == 26
    p = C.c_void_p(4096)
    ok = dict(frames=p, N=6, H=20, W=24, T=3, kinds=p, params=p, hk=[1, 6, 7, 5], hp=[1.2, 1.375, 0, 2], G=2, P=2,
              gs=3, mean=[0.5, 0.5, 0.5], std=[0.2, 0.2, 0.2], out=p)

    def call(fn=lib.coclr_augment_clips, **kw):
        a = dict(ok, **kw)
        hk = None if a["hk"] is None else (C.c_int32 * len(a["hk"]))(*a["hk"])
        hp = None if a["hp"] is None else (C.c_float * len(a["hp"]))(*a["hp"])
        mean = None if a["mean"] is None else (C.c_float * 3)(*a["mean"])
        std = None if a["std"] is None else (C.c_float * 3)(*a["std"])
        return fn(a["frames"], a["N"], a["H"], a["W"], a["T"], a["kinds"], a["params"], hk, hp, a["G"], a["P"],
                  a["gs"], mean, std, a["out"], None)
    for name in ("frames", "kinds", "params", "hk", "hp", "mean", "std", "out"):
        assert call(**{name: None}) == 1, name
    for name in ("N", "H", "W", "T", "G", "P", "gs"):
        assert call(**{name: 0}) == 1 and call(**{name: -2}) == 1, name
    assert call(hk=[1, 6, 7, 8]) == 1 and call(hk=[1, 6, 7, -1]) == 1                       # unknown kinds
    assert call(hp=[1.2, -0.5, 0, 2]) == 1 and call(hp=[1.2, 16.5, 0, 2]) == 1 and call(hp=[1.2, float("nan"), 0, 2]) == 1
    assert call(hp=[1.2, float("inf"), 0, 2]) == 1
    assert call(P=9, hk=[0] * 18, hp=[0] * 18) == 1
    assert call(H=225, W=224) == 1 and call(H=224, W=225) == 1 and call(H=1, W=50177) == 1
    assert call(T=4) == 1 and call(gs=2) == 1 and call(std=[0.2, 0.2, 0.0]) == 1
    assert call(hp=[1.2, 1.375, 0, 3]) == 1 and call(hk=[4, 6, 7, 5], hp=[17.5, 1.375, 0, 2]) == 1     # the old rules hold
    # the old entry point: kinds 6 and 7 stay refused
    old = lib.coclr_color_jitter_clips
    assert call(old, hk=[1, 6, 0, 5]) == 1 and call(old, hk=[1, 7, 0, 5]) == 1 and call(old, hk=[1, 2, 0, 6]) == 1

    Sp = 16
    args = dict(frames=p, F=12, H=40, W=52, desc=p, hd=[0, 3, 5, 4, 30, 28, 0, 0, 9, 9, 6, 3, 0, 0, 52, 40, 160, 160, 15, 13],
                n_clips=2, T=3, S=16, xtab=p, xlen=160 + Sp * 16, ytab=p, ylen=160 + Sp * 14, out=p)

    def boxes(**kw):
        a = dict(args, **kw)
        hd = None if a["hd"] is None else (C.c_int32 * len(a["hd"]))(*a["hd"])
        return lib.coclr_resize_boxes_u8(a["frames"], a["F"], a["H"], a["W"], a["desc"], hd, a["n_clips"], a["T"], a["S"],
                                         a["xtab"], a["xlen"], a["ytab"], a["ylen"], a["out"], None)

    def desc(k, field, value):
        hd = list(args["hd"])
        hd[k * 10 + field] = value
        return hd
    for name in ("frames", "desc", "hd", "xtab", "ytab", "out"):
        assert boxes(**{name: None}) == 1, name
    for name in ("F", "H", "W", "n_clips", "T", "S"):
        assert boxes(**{name: 0}) == 1, name
    assert boxes(S=513) == 1 and boxes(xtab=C.c_void_p(4100)) == 1
    assert boxes(hd=desc(0, 2, 23)) == 1 and boxes(hd=desc(0, 3, 13)) == 1 and boxes(hd=desc(1, 4, 53)) == 1     # box leaves
    assert boxes(hd=desc(0, 2, -1)) == 1 and boxes(hd=desc(0, 4, 0)) == 1 and boxes(hd=desc(1, 5, 41)) == 1
    assert boxes(hd=desc(0, 8, 0)) == 1 and boxes(hd=desc(0, 8, 65)) == 1 and boxes(hd=desc(1, 9, 0)) == 1       # taps
    assert boxes(hd=desc(1, 9, 65)) == 1
    assert boxes(hd=desc(0, 0, 10)) == 1 and boxes(hd=desc(0, 0, -1)) == 1 and boxes(hd=desc(0, 1, 2)) == 1      # frames
    assert boxes(hd=desc(1, 6, 161)) == 1 and boxes(hd=desc(1, 6, 164)) == 1 and boxes(hd=desc(1, 7, -4)) == 1   # tables
    assert boxes(xlen=160 + Sp * 16 - 1) == 1 and boxes(ylen=31) == 1
    assert boxes(n_clips=2, T=40000, hd=desc(0, 1, 40000)) == 1
    with pytest.raises(_lib.HipLibraryError):                        # and the bindings have no CPU path
        staging.augment(torch.zeros(2, 4, 4, 3, dtype=torch.uint8), [[]], 2, 1, device="cpu")
