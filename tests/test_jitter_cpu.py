"""CPU tier of the colour jitter (coclr_amd/staging.py: ColorJitter, color_jitter, stage_crops(jitter=);
coclr_amd/eval/video.py: add_frames(jitter=); csrc/staging.hip: coclr_color_jitter_clips, coclr_resize_crops_u8):
the numpy restatement of tests/jitter_harness.py against the committed fixture of the reference's own classes
(tests/golden/color_jitter.pt) and, where PIL is installed, against PIL itself over EVERY input; the draws of
ColorJitter against the reference's use of the generator; every refusal; and the host logic on the doubles."""
import ctypes as C
import itertools
import random

import numpy as np
import pytest
import torch

import crops_harness as CH
import jitter_harness as JH
from coclr_amd import _lib, staging
from coclr_amd.eval.video import VideoEvaluator


@pytest.fixture(scope="module")
def gold():
    return JH.golden()


@pytest.fixture(scope="module")
def cases(gold):
    return JH.fixture_cases(gold)


def test_fixture_has_every_case(gold, cases):
    assert [len(gold[k]) for k in "ABCDE"] == [4, 4, 1, 2, 3] and len(cases) == 14
    assert tuple(gold["frames"].shape) == (6, 20, 24, 3) and bool((gold["frames"][5] % 255 == 0).all())


def test_restatement_and_draws_reproduce_the_fixture(gold, cases):
    """ColorJitter.draw under random.seed(k) yields programs whose application equals the reference's bytes, and
    leaves the generator where the reference left it."""
    for name, frames, progs, gs, want, nxt in cases:
        got = JH.jitter_u8(frames, progs, gs)
        assert np.array_equal(got, want), name
        if nxt is not None:
            assert nxt[0] == nxt[1], name
    by = {c[0]: c for c in cases}
    assert by["C%d" % gold["C"][0]["seed"]][2] == [[]]                  # the p = 0.3 miss: nothing drawn, nothing done
    assert gold["C"][0]["draws"] == {"random": 1, "uniform": 0, "shuffle": 0}
    for run in gold["A"]:
        assert run["draws"] == {"random": 1, "uniform": 4, "shuffle": 1}
        assert sorted(k for k, _ in by["A%d" % run["seed"]][2][0]) == [1, 2, 3, 4]
    for run in gold["B"]:
        progs = by["B%d" % run["seed"]][2]
        assert run["draws"] == {"random": 1, "uniform": 8, "shuffle": 2} and len(progs) == 2 and progs[0] != progs[1]
    assert len({tuple(k for k, _ in by["A%d" % s][2][0]) for s in (0, 1, 2, 3)}) > 1      # the shuffle shows
    assert any(not np.array_equal(c[4], c[1]) for c in cases if c[0][0] in "ABDE")


def test_fixture_levels_are_totensor_normalize(gold):
    x = np.arange(256, dtype=np.uint8).reshape(1, 1, 256, 1).repeat(3, -1)
    assert torch.equal(CH.normalise(x)[0, 0].t().contiguous(), gold["levels"])
    want = JH.levels_expected(gold["frames"].numpy(), gold["levels"], 3)
    assert torch.equal(JH.reference(gold["frames"], [[]], 6, 3), want)


# ---- against PIL itself, exhaustively ---------------------------------------------------------------------------

def _slab(lo):
    r = np.arange(256, dtype=np.uint8)
    return np.ascontiguousarray(np.stack(np.meshgrid(r[lo:lo + 64], r, r, indexing="ij"), -1).reshape(64 * 256, 256, 3))


@pytest.mark.parametrize("lo", [0, 64, 128, 192])
@pytest.mark.parametrize("what", ["L", "rgb_to_hsv", "hsv_to_rgb"])
def test_cube_against_pil(what, lo):
    Image = pytest.importorskip("PIL.Image")
    cube = _slab(lo)
    if what == "L":
        want, got = np.asarray(Image.fromarray(cube, "RGB").convert("L")), JH.lum(cube)
    elif what == "rgb_to_hsv":
        want, got = np.asarray(Image.fromarray(cube, "RGB").convert("HSV")), JH.rgb_to_hsv(cube)
    else:
        want, got = np.asarray(Image.fromarray(cube, "HSV").convert("RGB")), JH.hsv_to_rgb(cube)
    assert int((want != got).sum()) == 0


def test_blend_against_pil():
    Image = pytest.importorskip("PIL.Image")
    d, i = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    im1, im2 = Image.fromarray(d, "L"), Image.fromarray(i, "L")
    alphas = [0, 1, 0.6, 0.8, 1.2, 1.4, 2.0] + list(np.random.RandomState(1).uniform(0, 2.2, 5))
    for a in alphas:
        assert int((np.asarray(Image.blend(im1, im2, float(a))) != JH.blend(d, i, a)).sum()) == 0, a


def test_ops_against_image_enhance():
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance
    fr = JH.golden()["frames"].numpy()
    for f in (fr[0], fr[5]):
        img = Image.fromarray(f)
        for a in (0.0, 0.5, 0.77, 1.0, 1.4, 2.0):
            for kind, E in ((JH.BRIGHTNESS, ImageEnhance.Brightness), (JH.CONTRAST, ImageEnhance.Contrast),
                            (JH.SATURATION, ImageEnhance.Color)):
                assert np.array_equal(np.asarray(E(img).enhance(a)), JH.apply_op(f, kind, a)), (kind, a)


def test_contrast_mean_is_the_integer_form():
    """int(sum / count + 0.5) in doubles equals (2*sum + count) // (2*count), which the kernel computes."""
    rng = np.random.RandomState(2)
    for count in (1, 2, 3, 256, 396, 16384, 50175, 50176):
        sums = np.unique(np.concatenate([rng.randint(0, 255 * count + 1, 2000), [0, 255 * count],
                                         (np.arange(256) * count + count // 2).clip(0, 255 * count),
                                         (np.arange(256) * count + count // 2 - 1).clip(0, 255 * count),
                                         (np.arange(256) * count + (count + 1) // 2).clip(0, 255 * count)]))
        for s in sums.tolist():
            assert int(float(s) / float(count) + 0.5) == (2 * s + count) // (2 * count), (s, count)
    for k, nudge, want in ((100, False, 101), (100, True, 100), (0, False, 1), (254, True, 254)):
        f = JH.half_mean_frame(18, 22, k, nudge)[0]
        assert JH.contrast_mean(f) == want


def test_hue_shift_byte():
    assert staging.hue_shift_byte(0.0) == 0 and staging.hue_shift_byte(0.1) == 25 and staging.hue_shift_byte(0.5) == 127
    assert staging.hue_shift_byte(-0.05) == 244 and staging.hue_shift_byte(-0.5) == 129       # -12.75 -> -12, -127.5 -> -127
    assert staging.hue_shift_byte(-0.001) == 0 and staging.hue_shift_byte(0.003) == 0         # truncation toward zero
    assert staging.hue_shift_byte(-1 / 255) == 255
    for f in np.random.RandomState(3).uniform(-0.5, 0.5, 200).tolist():
        assert staging.hue_shift_byte(f) == int(np.float64(f * 255).astype(np.int64)) % 256


def test_order_case_tells_the_orders_apart():
    frames, progs = JH.order_case()
    assert len(progs) == 24 and len({tuple(k for k, _ in p) for p in progs}) == 24
    res = JH.jitter_u8(frames, progs, 1)
    assert len({r.tobytes() for r in res}) >= 20


# ---- the host API ------------------------------------------------------------------------------------------------

def test_color_jitter_ranges():
    j = staging.ColorJitter(0.2, (0.5, 1.5), 0, (-0.1, 0.3), p=0.3)
    assert j.brightness == [0.8, 1.2] and j.contrast == (0.5, 1.5) and j.saturation is None and j.hue == (-0.1, 0.3)
    assert staging.ColorJitter(1.5).brightness == [0, 2.5]                     # clipped at zero
    assert staging.ColorJitter(saturation=(1, 1)).saturation is None and staging.ColorJitter(hue=(0, 0)).hue is None
    assert staging.ColorJitter(hue=0.5).hue == [-0.5, 0.5]
    for kw in (dict(brightness=-0.1), dict(hue=-0.1), dict(hue=(-0.6, 0.1)), dict(hue=(0.2, 0.1)),
               dict(contrast=(-0.5, 1)), dict(saturation=(2, 1))):
        with pytest.raises(ValueError):
            staging.ColorJitter(**kw)
    for kw in (dict(brightness="a"), dict(contrast=(1, 2, 3)), dict(hue=None)):
        with pytest.raises(TypeError):
            staging.ColorJitter(**kw)
    # only the enabled ops are drawn, in the reference's order of uniform() calls
    class Rec(random.Random):
        log = []

        def uniform(self, a, b):
            self.log.append((a, b))
            return super().uniform(a, b)
    r = Rec(4)
    progs = j.draw(r, 3) if r.random() * 0 == 0 else None
    r2 = Rec(4)
    r2.random()
    hit = r2.random() < 0.3
    assert (progs == [[]] * 3) == (not hit)
    j1 = staging.ColorJitter(0.2, (0.5, 1.5), 0, (-0.1, 0.3))
    del Rec.log[:]
    progs = j1.draw(Rec(5), 2)
    assert Rec.log == [(0.8, 1.2), (0.5, 1.5), (-0.1, 0.3)] * 2
    assert [sorted(k for k, _ in p) for p in progs] == [[1, 2, 4]] * 2
    assert staging.ColorJitter().draw(random.Random(0), 2) == [[], []]


def test_color_jitter_host_logic_and_refusals(monkeypatch):
    JH.install(monkeypatch)
    fr = torch.from_numpy(np.random.RandomState(0).randint(0, 256, size=(6, 9, 10, 3)).astype(np.uint8))
    progs = [[(1, 1.2), (2, 0.5)], [(4, 17)], []]
    out = staging.color_jitter(fr, progs, 2, 3, device="cpu")
    assert out.shape == (2, 3, 3, 9, 10) and torch.equal(out, JH.reference(fr, progs, 2, 3))
    kind, N, gs, seen = JH.CALLS[-1]
    assert (kind, N, gs) == ("jitter", 6, 2) and len(seen) == 3 and len(seen[0]) == 2      # padded to the longest
    assert seen[1] == [(4, 17.0), (0, 0.0)] and seen[2] == [(0, 0.0)] * 2
    n = len(JH.CALLS)
    with pytest.raises(ValueError):
        staging.color_jitter(fr, [[(1, 1.0)] * 9], 6, 3, device="cpu")             # a program longer than 8
    with pytest.raises(ValueError):
        staging.color_jitter(fr, progs, 2, 4, device="cpu")                        # N % T
    with pytest.raises(ValueError):
        staging.color_jitter(fr, progs[:2], 2, 3, device="cpu")                    # too few programs
    with pytest.raises(ValueError):
        staging.color_jitter(fr, [], 6, 3, device="cpu")
    with pytest.raises(ValueError):
        staging.color_jitter(fr, progs, 0, 3, device="cpu")
    with pytest.raises(ValueError):
        staging.color_jitter(torch.zeros(1, 225, 224, 3, dtype=torch.uint8), [[]], 1, 1, device="cpu")
    with pytest.raises(ValueError):
        staging.color_jitter(fr.float(), progs, 2, 3, device="cpu")                # dtype
    with pytest.raises(ValueError):
        staging.color_jitter(fr[..., :2], progs, 2, 3, device="cpu")               # shape
    with pytest.raises(ValueError):
        staging.color_jitter(fr[0], progs, 2, 3, device="cpu")
    for bad in ([(6, 1.0)], [(-1, 1.0)], [(4, 256)], [(4, 1.5)], [(4, -1)], [(5, 3)], [(5, 0.5)], [(1, float("nan"))],
                [(3, float("inf"))]):
        with pytest.raises(ValueError):
            staging.color_jitter(fr, [bad], 6, 3, device="cpu")
    assert len(JH.CALLS) == n                                                      # refused before any call
    assert staging.color_jitter(torch.zeros(1, 224, 224, 3, dtype=torch.uint8), [[]], 1, 1, device="cpu").shape == \
        (1, 3, 1, 224, 224)


def test_entry_point_refusals():
    """coclr_color_jitter_clips and coclr_resize_crops_u8 validate on the host before anything is launched: no GPU
    is needed to be refused.  The ABI number moves only with the library (coclr_pool_plan, coclr_bn_plan: 25; the staging plan queries: 26)."""
    assert _lib.ABI_VERSION == 26
    for name in ("coclr_color_jitter_clips", "coclr_resize_crops_u8"):
        assert name in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    p = C.c_void_p(4096)
    ok = dict(frames=p, N=6, H=20, W=24, T=3, kinds=p, params=p, hk=[1, 2, 4, 5], hp=[1.2, 0.5, 17, 2], G=2, P=2,
              gs=3, mean=[0.5, 0.5, 0.5], std=[0.2, 0.2, 0.2], out=p)

    def call(**kw):
        a = dict(ok, **kw)
        hk = None if a["hk"] is None else (C.c_int32 * len(a["hk"]))(*a["hk"])
        hp = None if a["hp"] is None else (C.c_float * len(a["hp"]))(*a["hp"])
        mean = None if a["mean"] is None else (C.c_float * 3)(*a["mean"])
        std = None if a["std"] is None else (C.c_float * 3)(*a["std"])
        return lib.coclr_color_jitter_clips(a["frames"], a["N"], a["H"], a["W"], a["T"], a["kinds"], a["params"], hk, hp,
                                            a["G"], a["P"], a["gs"], mean, std, a["out"], None)
    for name in ("frames", "kinds", "params", "hk", "hp", "mean", "std", "out"):
        assert call(**{name: None}) == 1, name
    for name in ("N", "H", "W", "T", "G", "P", "gs"):
        assert call(**{name: 0}) == 1 and call(**{name: -2}) == 1, name
    assert call(T=4) == 1                                            # N % T
    assert call(gs=2) == 1 and call(G=1, hk=[1, 2], hp=[1.2, 0.5]) == 1       # G * group_size < N
    assert call(P=9, hk=[0] * 18, hp=[0] * 18) == 1
    assert call(std=[0.2, 0.2, 0.0]) == 1
    assert call(hk=[1, 2, 4, 6]) == 1 and call(hk=[1, 2, 4, -1]) == 1        # unknown kinds
    assert call(hp=[1.2, 0.5, 17, 3]) == 1 and call(hp=[1.2, 0.5, 17, -1]) == 1 and call(hp=[1.2, 0.5, 17, 0.5]) == 1
    assert call(hp=[1.2, 0.5, 256, 2]) == 1 and call(hp=[1.2, 0.5, 17.5, 2]) == 1 and call(hp=[1.2, 0.5, -1, 2]) == 1
    assert call(hp=[float("nan"), 0.5, 17, 2]) == 1 and call(hp=[1.2, float("inf"), 17, 2]) == 1
    assert call(H=225, W=224) == 1 and call(H=224, W=225) == 1 and call(H=1, W=50177) == 1
    # the uint8 sibling of coclr_stage_crops: the same refusals
    args = dict(frames=p, F=6, H=40, W=52, slot_frame=p, n_clips=3, T=4, crops=[0, 0, 0, 24, 12, 1], cw=28, ch=28, S=16,
                xmin=p, xk=p, xtaps=9, ymin=p, yk=p, ytaps=9, out=p)

    def resize(**kw):
        a = dict(args, **kw)
        crops = None if a["crops"] is None else (C.c_int32 * len(a["crops"]))(*a["crops"])
        return lib.coclr_resize_crops_u8(a["frames"], a["F"], a["H"], a["W"], a["slot_frame"], a["n_clips"], a["T"], crops,
                                         a.get("n_crops", 0 if a["crops"] is None else len(a["crops"]) // 3), a["cw"],
                                         a["ch"], a["S"], a["xmin"], a["xk"], a["xtaps"], a["ymin"], a["yk"], a["ytaps"],
                                         a["out"], None)
    for name in ("frames", "slot_frame", "xmin", "xk", "ymin", "yk", "out"):
        assert resize(**{name: None}) == 1, name
    assert resize(crops=None, n_crops=2) == 1 and resize(crops=[25, 0, 0]) == 1 and resize(crops=[0, 0, 2]) == 1
    assert resize(S=513) == 1 and resize(xtaps=65) == 1 and resize(n_clips=16384, T=4) == 1 and resize(F=0) == 1
    with pytest.raises(_lib.HipLibraryError):                        # and the bindings have no CPU path
        staging.color_jitter(torch.zeros(2, 4, 4, 3, dtype=torch.uint8), [[]], 2, 1, device="cpu")


def _video(F=7, H=24, W=30, seed=0):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, size=(F, H, W, 3)).astype(np.uint8))


def test_stage_crops_with_jitter_on_the_doubles(monkeypatch):
    JH.install(monkeypatch)
    frames, idx = _video(), staging.test_frame_index(7, 4)
    boxes = [(0, 0), (14, 8), (7, 4)]
    flips = [0, 1, 1]
    progs = [[(1, 1.3), (4, 200)], [], [(2, 0.6), (3, 1.5), (5, 1)]]
    out = staging.stage_crops(frames, idx, boxes, flips, 16, 8, device="cpu", jitter=progs)
    assert [c[0] for c in JH.CALLS] == ["resize", "jitter"] and not CH.CALLS        # two calls, not the fp32 one
    n = idx.shape[0]
    assert out.shape == (3, n, 3, 4, 8, 8) and JH.CALLS[1][1:3] == (3 * n * 4, n * 4)
    u8 = CH.crop_resized_u8(frames.numpy(), [(x, y, f) for (x, y), f in zip(boxes, flips)], 16, 16, 8)
    sel = idx.reshape(-1)
    for k in range(3):
        assert torch.equal(out[k], JH.reference(u8[k][sel], [progs[k]], n * 4, 4)), k
    plain = staging.stage_crops(frames, idx, boxes, flips, 16, 8, device="cpu")
    assert torch.equal(out[1], plain[1]) and not torch.equal(out[0], plain[0])      # the empty program is no jitter
    assert len(CH.CALLS) == 1
    for bad in (progs[:2], progs + [[]], [[(7, 1.0)], [], []], [[(1, 1.0)] * 9, [], []]):
        calls = len(JH.CALLS)
        with pytest.raises(ValueError):
            staging.stage_crops(frames, idx, boxes, flips, 16, 8, device="cpu", jitter=bad)
        assert len(JH.CALLS) == calls
    # more than 16 crops: the resize is cut into launches, the jitter stays one
    del JH.CALLS[:]
    many = staging.stage_crops(frames, idx, [(i % 14, 0) for i in range(17)], [0] * 17, 16, 8, device="cpu",
                               jitter=[[(1, 0.5 + 0.05 * i)] for i in range(17)])
    assert [c[:2] for c in JH.CALLS] == [("resize", 16), ("resize", 1), ("jitter", 17 * n * 4)]
    assert many.shape[0] == 17 and not torch.equal(many[0], many[14])


def test_add_frames_with_jitter_on_the_doubles(monkeypatch):
    JH.install(monkeypatch)
    W, H, size, S, T = 30, 24, 16, 8, 4
    frames, idx = _video(13, H, W, 3), staging.test_frame_index(13, T)
    n = idx.shape[0]
    per_crop = n * 3 * T * S * S * 4
    jit = staging.ColorJitter(0.2, 0.2, 0.2, 0.1, p=0.6)
    ref = random.Random(5)
    drawn = [jit.draw(ref, 1)[0] for _ in range(10)]
    ref_after = ref.random()
    assert any(drawn) and not all(drawn)                                  # hits and misses of p among the ten
    seen = []
    inner = VideoEvaluator.add
    monkeypatch.setattr(VideoEvaluator, "add", lambda self, clips, label=None, video=None: (
        seen.append(clips.clone()), inner(self, clips, label=label, video=video))[1])
    results = []
    for budget in (3 * per_crop + 5, 10 * per_crop, per_crop):
        del seen[:], JH.CALLS[:]
        ev = VideoEvaluator(CH.ToyClassifier().eval(), batch_clips=8)
        rng = random.Random(5)
        ev.add_frames(frames, idx, label=1, crops="ten", crop_size=size, out_size=S, max_stage_bytes=budget,
                      jitter=jit, rng=rng)
        after = rng.random()
        progs = [[g for g in p if g[0] != 0] for c in JH.CALLS if c[0] == "jitter" for p in c[3]]     # less padding
        results.append(([s.clone() for s in seen], progs, after, ev.finish().probs))
    chunks = [c[1] for c in JH.CALLS if c[0] == "resize"]
    assert chunks == [1] * 10                                              # the last budget: one crop at a time
    first = results[0]
    assert len(first[0]) == 10
    for other in results[1:]:
        assert all(torch.equal(a, b) for a, b in zip(first[0], other[0])) and other[1] == first[1]
        assert other[2] == first[2] and torch.equal(other[3], first[3])
    # the draws come in crop order: crop k runs the k-th program drawn from Random(5)
    assert len(first[1]) == 10 and first[2] == ref_after
    for k, got in enumerate(first[1]):
        assert [(kk, float(np.float32(v))) for kk, v in drawn[k]] == got, k
    # and equal staging the same crops by hand
    boxes = staging.five_crop_boxes(W, H, size) * 2
    flips = [0] * 5 + [1] * 5
    by_hand = staging.stage_crops(frames, idx, boxes, flips, size, S, device="cpu", jitter=drawn)
    assert all(torch.equal(a, b) for a, b in zip(first[0], by_hand))
    # jitter=None: exactly the calls of today -- the fp32 launch alone, no draw
    del JH.CALLS[:], CH.CALLS[:]
    rng = random.Random(5)
    ev = VideoEvaluator(CH.ToyClassifier().eval(), batch_clips=8)
    ev.add_frames(frames, idx, label=1, crops="ten", crop_size=size, out_size=S, max_stage_bytes=3 * per_crop + 5, rng=rng)
    assert not JH.CALLS and [c[0] for c in CH.CALLS] == [3, 3, 3, 1] and rng.random() == random.Random(5).random()
    with pytest.raises(AttributeError):
        ev.add_frames(frames, idx, crops="center", crop_size=size, out_size=S, jitter=[[(1, 1.0)]])     # not a ColorJitter
