"""CPU tier of the many-videos test staging (csrc/staging.hip: coclr_stage_crops_ragged; staging.stage_crops_ragged,
crops_tables_ragged; VideoEvaluator.add_videos): the additive ABI, every refusal of the entry point before any launch,
the host tables against expectations written out by hand, the Python refusals, and add_videos against a per-video
add_frames loop with numpy doubles for the two ops.  Nothing here needs a GPU, and the pointers that stand for device
memory are never dereferenced: only refused calls are made (one call that passes every check is made where no GPU is
visible, so that nothing can be launched)."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch

import crops_harness as CH
from coclr_amd import _lib, ops, staging
from coclr_amd.eval.video import CROP_MODES, VideoEvaluator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000                                                # a non-null, 16-byte aligned stand-in, never dereferenced
NAME = "coclr_stage_crops_ragged"


def hp(t, ty=C.c_int32):
    return C.cast(t.data_ptr(), C.POINTER(ty))


def _video(F, H, W, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, size=(F, H, W, 3)).astype(np.uint8))


# ---- ABI -----------------------------------------------------------------------------------------------------------------

def test_abi_is_additive_and_exported():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "coclr_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\bint\s+(coclr_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (coclr_[a-z0-9_]+)", out))
    assert NAME in declared and NAME in exported and NAME in _lib.EXPORTED_SYMBOLS
    assert declared == exported == set(_lib.EXPORTED_SYMBOLS)
    assert hasattr(ops, "stage_crops_ragged")
    assert lib.coclr_abi_version() == _lib.ABI_VERSION == 26
    # the signature the header states, word for word in the binding: pointers, 64-bit sizes, 32-bit counts
    i32, i64, vp, P = C.c_int32, C.c_int64, C.c_void_p, C.POINTER
    assert _lib._SIGNATURES[NAME] == [vp, i64, vp, P(i32), i32, i32, vp, P(i64), i32, i32, i32, vp, vp, i32, vp, vp,
                                      i32, P(C.c_float), P(C.c_float), vp, vp, vp]


# ---- the entry point refuses before any launch ---------------------------------------------------------------------------

def _two_videos():
    """57 x 43 (3 W H = 7353, padded to 7360) then 64 x 48 frames, W x H, two of each; one clip of T = 2 per video."""
    frames = staging.ragged_from_frames([torch.zeros(2, 43, 57, 3, dtype=torch.uint8),
                                         torch.zeros(2, 48, 64, 3, dtype=torch.uint8)], device="cpu")
    clips = [([0, 1], (17, 3), 0), ([2, 3], (24, 8), 1)]
    return frames, clips


def test_entry_point_rejects_before_any_launch():
    lib = _lib.load()
    frames, clips = _two_videos()
    desc, off = staging.crops_tables_ragged(frames, clips, 40)
    assert desc.tolist() == [[17, 3, 0, 57, 43], [24, 8, 1, 64, 48]]
    assert off.tolist() == [[0, 7360], [14720, 14720 + 9216]]
    nbytes = frames.pixels.numel()
    assert nbytes == 14720 + 2 * 9216
    third = (C.c_float * 3)(0.5, 0.5, 0.5)
    zero_std = (C.c_float * 3)(0.5, 0.0, 0.5)

    def call(d=desc, o=off, nbytes=nbytes, n=2, T=2, cw=40, ch=40, S=16, xtaps=9, ytaps=9, mean=third, std=third,
             ptrs=None):
        q = {"frames": FAKE, "desc": FAKE, "slot_off": FAKE, "xmin": FAKE, "xk": FAKE, "ymin": FAKE, "yk": FAKE,
             "out8": None, "out": FAKE}
        q.update(ptrs or {})
        return lib.coclr_stage_crops_ragged(q["frames"], nbytes, q["desc"], hp(d) if d is not None else None, n, T,
                                            q["slot_off"], hp(o, C.c_int64) if o is not None else None, cw, ch, S,
                                            q["xmin"], q["xk"], xtaps, q["ymin"], q["yk"], ytaps, mean, std, q["out8"],
                                            q["out"], None)

    def changed(t, row, col, value):
        t = t.clone()
        t[row, col] = value
        return t

    # a null or misaligned pointer
    for name in ("frames", "desc", "slot_off", "xmin", "xk", "ymin", "yk"):
        assert call(ptrs={name: None}) == 1, name
    assert call(d=None) == 1 and call(o=None) == 1
    for name, by in (("frames", 8), ("desc", 2), ("slot_off", 4), ("xmin", 8), ("xk", 4), ("ymin", 2), ("yk", 1),
                     ("out", 2)):
        assert call(ptrs={name: FAKE + by}) == 1, name
    # both outputs or neither; out without mean / std; a zero std
    assert call(ptrs={"out8": FAKE}) == 1 and call(ptrs={"out": None}) == 1
    assert call(mean=None) == 1 and call(std=None) == 1 and call(std=zero_std) == 1
    # sizes
    assert call(nbytes=0) == 1 and call(n=0) == 1 and call(T=0) == 1 and call(S=0) == 1 and call(cw=0) == 1
    assert call(ch=0) == 1 and call(n=-1) == 1 and call(T=-2) == 1
    assert call(S=513) == 1
    assert call(xtaps=0) == 1 and call(xtaps=65) == 1 and call(ytaps=0) == 1 and call(ytaps=65) == 1
    # W or H outside 1..32768
    for col in (3, 4):
        for v in (0, -1, 32769):
            assert call(d=changed(desc, 0, col, v)) == 1, (col, v)
    # a box that leaves its OWN frame: x0 = 18 fits the 64-wide frames of the batch, not this clip's 57
    assert call(d=changed(desc, 0, 0, 18)) == 1 and call(d=changed(desc, 0, 1, 4)) == 1
    assert call(d=changed(desc, 1, 0, 25)) == 1 and call(d=changed(desc, 1, 1, 9)) == 1
    assert call(d=changed(desc, 0, 0, -1)) == 1 and call(d=changed(desc, 1, 1, -1)) == 1
    assert call(cw=41) == 1 and call(ch=41) == 1              # and so does a larger crop at the same corner
    # the frame taken for a larger one than it is: the box fits then, the slot's bytes leave the buffer
    assert call(d=changed(desc, 1, 4, 49)) == 1
    # flip not 0/1
    assert call(d=changed(desc, 0, 2, 2)) == 1 and call(d=changed(desc, 1, 2, -1)) == 1
    # slot offsets: negative, not a multiple of 16, leaving the buffer
    assert call(o=changed(off, 0, 0, -16)) == 1 and call(o=changed(off, 0, 1, 7360 + 8)) == 1
    assert call(o=changed(off, 1, 1, nbytes - 9216 + 16)) == 1 and call(o=changed(off, 0, 0, nbytes)) == 1
    assert call(o=changed(off, 0, 1, 1 << 40)) == 1
    assert call(nbytes=nbytes - 1) == 1                        # the last frame's bytes leave the buffer
    # more slots than a launch has: n_clips * T > 65535 (the tables are refused before they are read past their end)
    assert call(n=32768, T=2) == 1 and call(n=65536, T=1) == 1
    # a grid over the launch limits: one clip of T slots, ch = S = 512 and 19 taps give bands of R = 1 row (21 source
    # rows of 3 * 512 bytes; two rows would need 22 > 32 KiB), 512 bands, and 512 * T * 256 threads reach 2^32 at T = 32768
    wide = torch.tensor([[0, 0, 0, 40, 512]], dtype=torch.int32)
    assert call(d=wide, o=torch.zeros(1, 32768, dtype=torch.int64), nbytes=1 << 20, n=1, T=32768, ch=512, S=512,
                ytaps=19) == 1
    if not torch.cuda.is_available():
        # one slot fewer passes every check.  Where no GPU is visible the launch that follows cannot happen and the
        # runtime's own error comes back instead of COCLR_EINVAL; with a GPU this call is not made: it would launch
        rc = call(d=wide, o=torch.zeros(1, 32767, dtype=torch.int64), nbytes=1 << 20, n=1, T=32767, ch=512, S=512,
                  ytaps=19)
        assert rc not in (0, 1), rc
    # an output row whose ytaps source rows exceed 64 KiB of LDS: 64 + 2 rows of 3 * 512 bytes
    big = changed(changed(desc, 0, 1, 0), 1, 1, 0)
    tall = changed(changed(big, 0, 4, 30000), 1, 4, 30000)
    huge = torch.zeros_like(off)
    assert call(d=tall, o=huge, nbytes=1 << 40, ch=30000, S=512, ytaps=64) == 1


# ---- the host tables ---------------------------------------------------------------------------------------------------

class _Tables:
    """What crops_tables_ragged reads of a RaggedFrames: the three host tables, no pixels."""

    def __init__(self, offset, height, width):
        self.offset = torch.tensor(offset, dtype=torch.int64)
        self.height = torch.tensor(height, dtype=torch.int32)
        self.width = torch.tensor(width, dtype=torch.int32)


def test_crops_tables_by_hand():
    # video A: three 57 x 43 frames at 0, 7360, 14720; video B: two 64 x 48 frames far beyond 2^31
    far = (1 << 31) + 4096
    frames = _Tables([0, 7360, 14720, far, far + 9216], [43, 43, 43, 48, 48], [57, 57, 57, 64, 64])
    # A is shorter than a clip of four: left-padded with frame 0 (test_frame_index(3, 4)); B at ds = 1 of T = 4 repeats
    a = staging.test_frame_index(3, 4)[0]
    assert a.tolist() == [0, 0, 1, 2]
    clips = [(a, (17, 3), 0), (a, (0, 0), 1), (np.array([3, 4, 4, 3]), (24, 8), 0), (torch.tensor([4, 4, 4, 4]), (0, 8), 1)]
    desc, off = staging.crops_tables_ragged(frames, clips, 40)
    assert desc.dtype == torch.int32 and off.dtype == torch.int64 and desc.is_contiguous() and off.is_contiguous()
    assert desc.tolist() == [[17, 3, 0, 57, 43], [0, 0, 1, 57, 43], [24, 8, 0, 64, 48], [0, 8, 1, 64, 48]]
    assert off.tolist() == [[0, 0, 7360, 14720], [0, 0, 7360, 14720], [far, far + 9216, far + 9216, far],
                            [far + 9216] * 4]
    assert int(off.max()) >= 1 << 31
    # rectangular crops: (width, height)
    desc, _ = staging.crops_tables_ragged(frames, [(a, (1, 33), 1)], (56, 10))
    assert desc.tolist() == [[1, 33, 1, 57, 43]]


def test_clip_order_is_video_crop_clip(monkeypatch):
    """What add_videos hands to the op: video, then crop in CROP_MODES order, then clip."""
    seen = _install(monkeypatch)
    vids = [_video(9, 24, 30, 1), _video(3, 30, 24, 2)]
    frames = staging.ragged_from_frames(vids, device="cpu")
    index = [staging.test_frame_index(9, 4), staging.test_frame_index(3, 4)]
    assert [i.shape[0] for i in index] == [6, 1]
    ev = VideoEvaluator(_TableModel().eval(), batch_clips=200)
    assert ev.add_videos(frames, [(0, 9, index[0], 4), (9, 3, index[1], 6)], crops="ten", crop_size=16, out_size=8) \
        == [0, 1]
    (desc, off), = seen
    want_desc, want_off = [], []
    for first, (W, H), idx in ((0, (30, 24), index[0]), (9, (24, 30), index[1])):
        where, flips = CROP_MODES["ten"]
        for fl in flips:
            for x0, y0 in staging.five_crop_boxes(W, H, 16, where):
                for row in idx:
                    want_desc.append([x0, y0, fl, W, H])
                    want_off.append([int(frames.offset[first + f]) for f in row])
    assert desc.tolist() == want_desc and off.tolist() == want_off and len(want_desc) == 70


def test_python_refusals(monkeypatch):
    seen = _install(monkeypatch)
    frames = staging.ragged_from_frames([_video(3, 43, 57, 1), _video(3, 48, 64, 2)], device="cpu")
    ok = [([0, 1], (17, 3), 0), ([3, 4], (24, 8), 1)]
    assert staging.stage_crops_ragged(frames, ok, 40, 16).shape == (2, 3, 2, 16, 16) and len(seen) == 1
    with pytest.raises(ValueError):                           # fits the batch's 64 x 48 frames, not its own 57 x 43
        staging.stage_crops_ragged(frames, [([0, 1], (18, 3), 0)], 40, 16)
    with pytest.raises(ValueError):
        staging.stage_crops_ragged(frames, [([0, 1], (17, 4), 0)], 40, 16)
    with pytest.raises(ValueError):                           # mixed sizes inside one clip
        staging.stage_crops_ragged(frames, [([2, 3], (0, 0), 0)], 40, 16)
    for bad in ([0, 6], [-1, 0]):
        with pytest.raises(IndexError):                       # an id outside `frames`
            staging.stage_crops_ragged(frames, [(bad, (0, 0), 0)], 40, 16)
    with pytest.raises(ValueError):
        staging.stage_crops_ragged(frames, [([0, 1], (0, 0), 2)], 40, 16)           # flip
    with pytest.raises(ValueError):
        staging.stage_crops_ragged(frames, [([0, 1], (0, 0), 0), ([0, 1, 2], (0, 0), 0)], 40, 16)   # two lengths
    with pytest.raises(ValueError):
        staging.stage_crops_ragged(frames, [], 40, 16)
    with pytest.raises(ValueError):
        staging.stage_crops_ragged(frames.pixels, ok, 40, 16)
    with pytest.raises(ValueError):
        staging.stage_crops_ragged(frames, ok, 40, 16, out=torch.empty(2, 3, 2, 16, 17))
    with pytest.raises(ValueError):
        staging.stage_crops_ragged(frames, ok, 40, 16, jitter=[[]])                  # one program per clip
    ev = VideoEvaluator(_TableModel().eval(), batch_clips=8)
    idx = [[0, 1], [1, 2]]
    with pytest.raises(ValueError):                           # a video whose frames differ in size
        ev.add_videos(frames, [(2, 3, idx, 0)], crop_size=40, out_size=16)
    with pytest.raises(IndexError):
        ev.add_videos(frames, [(4, 3, idx, 0)], crop_size=40, out_size=16)
    with pytest.raises(IndexError):
        ev.add_videos(frames, [(0, 3, [[0, 3]], 0)], crop_size=40, out_size=16)
    with pytest.raises(ValueError):
        ev.add_videos(frames, [(0, 3, idx, 0)], crop_size=44, out_size=16)            # FiveCrop: bigger than the frame
    with pytest.raises(ValueError):
        ev.add_videos(frames, [(0, 3, idx, 0)], crops="three", crop_size=40, out_size=16)
    with pytest.raises(ValueError):
        ev.add_videos(frames, [(0, 3, idx, 0), (3, 3, [[0, 1, 2]], 1)], crop_size=40, out_size=16)   # two clip lengths
    with pytest.raises(ValueError):                           # more slots in one clip than a launch has
        ev.add_videos(frames, [(0, 3, np.zeros((1, 65536), dtype=np.int64), 0)], crop_size=40, out_size=16)
    assert len(ev) == 0 and len(seen) == 1                    # refused before anything changed or was staged
    # a bad LATER video: nothing of the earlier ones is registered or staged, and the caller's rng has not moved
    rng = random.Random(3)
    state = rng.getstate()
    jitter = staging.ColorJitter(0.2, 0.2, 0.2, 0.1, p=0.7)
    for bad, err in (((3, 3, [[0, 3]], 1), IndexError), ((4, 3, idx, 1), IndexError), ((2, 3, idx, 1), ValueError)):
        with pytest.raises(err):
            ev.add_videos(frames, [(0, 3, idx, 0), bad], crop_size=40, out_size=16, jitter=jitter, rng=rng)
    assert len(ev) == 0 and len(seen) == 1 and rng.getstate() == state


class _FakeStore:
    """What add_stored uses of a jpeg.Store, over decoded frames held on the host: len, the frame sizes, decode."""

    def __init__(self, vids):
        self.frames = [f for v in vids for f in v]
        self._geo = torch.tensor([[f.shape[0], f.shape[1], 3, 1, 1] for f in self.frames], dtype=torch.int64)
        self.calls = []

    def __len__(self):
        return len(self.frames)

    def frame_size(self, id):
        return int(self._geo[id, 1]), int(self._geo[id, 0])

    def decode(self, ids):
        self.calls.append(torch.as_tensor(ids).tolist())
        return staging.ragged_from_frames([self.frames[i] for i in self.calls[-1]], device="cpu")


def test_add_stored_groups_validates_first_and_equals_the_loop(monkeypatch):
    seen = _install(monkeypatch)
    T, size, S = 4, 16, 8
    shapes = [(7, 24, 30), (3, 30, 24), (13, 24, 30), (9, 20, 33)]
    vids = [_video(F, H, W, 20 + k) for k, (F, H, W) in enumerate(shapes)]
    index = [staging.test_frame_index(v.shape[0], T) for v in vids]
    index[3] = index[3][2:3]                                                 # one clip: frames 2..5 of the last video
    first = np.cumsum([0] + [s[0] for s in shapes])
    store = _FakeStore(vids)
    videos = [(int(first[k]), shapes[k][0], index[k], k) for k in range(4)]
    model = _TableModel().eval()
    ev = VideoEvaluator(model, batch_clips=8)
    rng = random.Random(3)
    state = rng.getstate()
    jitter = staging.ColorJitter(0.2, 0.2, 0.2, 0.1, p=0.7)
    for bad, err in (((int(first[3]), 9, [[0, 9, 1, 2]], 3), IndexError),      # an id outside the video
                     ((int(first[3]) + 1, 9, index[3], 3), IndexError),         # the video leaves the store
                     ((int(first[1]) + 1, 4, [[0, 1, 2, 3]], 3), ValueError),   # frames of two sizes
                     ((int(first[3]), 9, index[3][:, :3], 3), ValueError)):     # another clip length
        with pytest.raises(err):
            ev.add_stored(store, videos[:3] + [bad], crops="five", crop_size=size, out_size=S, jitter=jitter, rng=rng,
                          max_stage_bytes=20000)
    with pytest.raises(ValueError):
        ev.add_stored(store, [], crop_size=size, out_size=S)
    assert len(ev) == 0 and not store.calls and not seen and rng.getstate() == state
    # groups by decoded bytes: 7 * 2160 fits 20000, + 3 * 2160 does not, 13 * 2160 alone exceeds it, 4 * 1984 follows
    assert ev.add_stored(store, videos, crops="five", crop_size=size, out_size=S, max_stage_bytes=20000) == [0, 1, 2, 3]
    assert store.calls == [list(range(0, 7)), list(range(7, 10)), list(range(10, 23)), list(range(25, 29))]
    got = ev.finish()
    loop = VideoEvaluator(model, batch_clips=8)
    for v, idx, k in zip(vids, index, range(4)):
        loop.add_frames(v, idx, label=k, crops="five", crop_size=size, out_size=S)
    want = loop.finish()
    assert ev.passes == loop.passes == -(-5 * (4 + 1 + 10 + 1) // 8)
    assert torch.equal(got.probs, want.probs) and torch.equal(got.features, want.features)
    assert torch.equal(got.labels, want.labels) and torch.equal(got.top1, want.top1) and torch.equal(got.top5, want.top5)


# ---- add_videos against the per-video loop, on doubles of the two ops ----------------------------------------------------

def stage_crops_ragged_double(seen):
    """Double of ops.stage_crops_ragged on the integer restatement of tests/crops_harness.py, clip by clip."""

    def op(pixels, desc, desc_host, slot_off, slot_off_host, cw, ch, S, xmin, xk, ymin, yk, out, mean=None, std=None):
        for got, want in zip((xmin, xk), CH.kernel_layout(cw, S)):
            assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)
        for got, want in zip((ymin, yk), CH.kernel_layout(ch, S)):
            assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)
        assert pixels.dtype == torch.uint8 and pixels.dim() == 1
        assert desc.dtype == torch.int32 and slot_off.dtype == torch.int64
        assert torch.equal(desc.cpu(), desc_host) and torch.equal(slot_off.cpu(), slot_off_host)
        n, T = slot_off_host.shape
        assert n * T <= 65535 and tuple(out.shape) == (n, 3, T, S, S) and out.dtype == torch.float32
        seen.append((desc_host.clone(), slot_off_host.clone()))
        for k in range(n):
            x0, y0, flip, W, H = desc_host[k].tolist()
            fr = np.stack([pixels[o:o + 3 * W * H].view(H, W, 3).cpu().numpy() for o in slot_off_host[k].tolist()])
            u8, = CH.crop_resized_u8(fr, [(x0, y0, flip)], cw, ch, S)                  # (T, S, S, 3)
            out[k].copy_(CH.normalise(u8, mean, std).permute(3, 0, 1, 2))

    return op


def _install(monkeypatch):
    CH.install(monkeypatch)
    seen = []
    monkeypatch.setattr(ops, "stage_crops_ragged", stage_crops_ragged_double(seen))
    return seen


class _TableModel(torch.nn.Module):
    """Stands in for the classifier: a clip -> the row of fixed tables that its first red byte names."""

    def __init__(self, num_class=11, width=6, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.logits = torch.nn.Parameter(torch.randn(256, num_class, generator=g) * 3, requires_grad=False)
        self.feats = torch.nn.Parameter(torch.randn(256, width, generator=g), requires_grad=False)
        self.rows = []

    def forward(self, block):
        x = block[:, 0, 0, 0, 0].double() * staging.IMAGENET_STD[0] + staging.IMAGENET_MEAN[0]
        idx = (x * 255).round().long().clamp(0, 255)
        self.rows.append(idx.tolist())
        return self.logits[idx], self.feats[idx]


@pytest.mark.parametrize("mode", ["center", "ten"])
def test_add_videos_equals_the_add_frames_loop(monkeypatch, mode):
    seen = _install(monkeypatch)
    T, size, S = 4, 16, 8
    shapes = [(7, 24, 30), (3, 30, 24), (13, 24, 30), (9, 20, 33)]           # F, H, W: three sizes, one shorter than T
    vids = [_video(F, H, W, 10 + k) for k, (F, H, W) in enumerate(shapes)]
    index = [staging.test_frame_index(v.shape[0], T) for v in vids]
    assert [i.shape[0] for i in index] == [4, 1, 10, 6]
    labels = [3, 0, 7, 9]
    n_crops = len(CROP_MODES[mode][0]) * len(CROP_MODES[mode][1])
    want_model, got_model = _TableModel().eval(), _TableModel().eval()
    loop = VideoEvaluator(want_model, batch_clips=8)
    for v, idx, l in zip(vids, index, labels):
        loop.add_frames(v, idx, label=l, crops=mode, crop_size=size, out_size=S)
    want = loop.finish()
    frames = staging.ragged_from_frames(vids, device="cpu")
    first = np.cumsum([0] + [s[0] for s in shapes])
    ev = VideoEvaluator(got_model, batch_clips=8)
    # two calls, the second beginning inside a batch: 21 * n_crops clips in batches of 8
    ids = ev.add_videos(frames, [(int(first[k]), shapes[k][0], index[k], labels[k]) for k in (0, 1)], crops=mode,
                        crop_size=size, out_size=S)
    ids += ev.add_videos(frames, [(int(first[k]), shapes[k][0], index[k], labels[k]) for k in (2, 3)], crops=mode,
                         crop_size=size, out_size=S)
    assert ids == [0, 1, 2, 3] and len(ev) == 4
    got = ev.finish()
    assert ev.passes == loop.passes == -(-21 * n_crops // 8)
    # one launch per stretch of rows up to the next model pass, none larger than the batch, and no copy: video 2's
    # ten clips per crop straddle a flush, so does the boundary between the two calls
    assert all(d.shape[0] <= 8 for d, _ in seen) and sum(d.shape[0] for d, _ in seen) == 21 * n_crops
    assert len(seen) <= ev.passes + 1
    assert got_model.rows[:-1] == want_model.rows[:-1]         # the same clips in the same rows of every full batch
    tail = 21 * n_crops % 8 or 8
    assert got_model.rows[-1][:tail] == want_model.rows[-1][:tail]
    assert torch.equal(got.probs, want.probs) and torch.equal(got.features, want.features)
    assert torch.equal(got.labels, want.labels) and got.labels.tolist() == labels
    assert torch.equal(got.top1, want.top1) and torch.equal(got.top5, want.top5)
    assert len({r for rows in got_model.rows for r in rows}) > 10          # the table model tells clips apart
