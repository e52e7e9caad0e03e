"""Input staging of the training loops on MI355X.

Reference (main_nce.py:207-209,299-302,310; main_coclr.py:221-223,366-368):

    transform_train_cuda = Compose([T.Normalize(mean, std, channel=1)])
    def tr(x):  return transforms_cuda(x).view(B,3,num_seq,seq_len,H,W).transpose(1,2).contiguous()
    input_seq = tr(input_seq.cuda(non_blocking=True))

i.e. fp32 frames over PCIe (403 MB/step at B=32), a normalise pass, a transposing copy, and two
more `.contiguous()` copies inside the model (model/pretrain.py:149-150).  `tr()` below does the
normalisation and the re-layout in ONE kernel (csrc/staging.hip) and also accepts the loader's
frames as uint8 (what they are before ToTensor: 4x less PCIe traffic), bit-identical to
`ToTensor` + `Normalize` on the same bytes.  The model already consumes `block[:, i]` as strided
views, so nothing else is copied.

The test protocol's input (eval/main_classifier.py:453-469) is staged here too: `stage_crops` turns ONE
video's raw uint8 frames into every crop x flip x clip the five/ten-crop test feeds the classifier, in one
launch, bit-identical to the reference's PIL chain (flip -> FiveCrop -> Scale(BICUBIC) -> ToTensor) plus
Normalize; `resample_tables`, `five_crop_boxes` and `test_frame_index` are the host-side restatements it needs.
The chain's ColorJitter (utils/augmentation.py:219-320) is `ColorJitter` below: it draws from the generator as
the reference does and hands the kernel one small program per group of frames (`color_jitter`,
`stage_crops(jitter=...)`), bit-identical to torchvision 0.5's functional ops on PIL images.
The training transform (main_nce.py:366-392) is `TrainTransform` + `stage_train_clips` at the end of this file: the
reference's draws on the host, then every clip's RandomSizedCrop box and its ColorJitter / RandomGray / GaussianBlur
/ RandomHorizontalFlip program in two launches, bit-identical to the reference's classes.
The classifier's transform (eval/main_classifier.py:729-744) is `ClassifierTransform` + `stage_classifier_clips`: the
draws of RandomSizedCrop(consistent=True) with its ten attempts and its Scale + CenterCrop fallback, then both bicubic
resizes (to 224, then to img_dim) in ONE launch, the clip's ColorJitter and the loop's batch flip in a second.
CoCLR's two-stream samples (main_coclr.py:447-473; dataset/lmdb_dataset.py:498-509), 4 T frames of RGB and flow under
the chain at seq_len = 2 T, are `stage_two_stream_clips` and its ragged and cropped forms: the same kernels on another
decomposition of a sample into clips, landing in the tensors CoCLR.forward reads (`TwoStreamClips`).
"""
import math
import numbers
import os
import random

import numpy as np
import torch

from . import ops

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def tr(x, num_seq, seq_len, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None):
    """x: (B, 3, num_seq*seq_len, H, W) on the device, fp32 in [0,1] (the loader's ToTensor output)
    or uint8 (raw frames) -> (B, num_seq, 3, seq_len, H, W) fp32, normalised per channel."""
    if x.dim() != 5 or x.shape[2] != num_seq * seq_len:
        raise ValueError("coclr_amd: expected frames of shape (B, C, %d, H, W), got %s"
                         % (num_seq * seq_len, tuple(x.shape)))
    if x.dtype not in (torch.uint8, torch.float32):
        raise TypeError("coclr_amd: frames must be uint8 or float32, got %s" % x.dtype)
    x = x.contiguous()
    B, C, _, H, W = x.shape
    if out is None:
        out = torch.empty(B, num_seq, C, seq_len, H, W, dtype=torch.float32, device=x.device)
    ops.stage_clips(x, out, num_seq, mean, std)
    return out


class ClipStager:
    """Host side of the uint8 path: two pinned buffers and a copy stream, so the H2D transfer of
    batch i+1 (101 MB at B=32 instead of 403 MB) overlaps the compute of batch i.

        stager = ClipStager(num_seq=2, seq_len=32)
        for frames_u8, ... in loader:                 # (B, 3, 64, 128, 128) uint8, host
            block = stager(frames_u8)                 # (B, 2, 3, 32, 128, 128) fp32, device
    """

    def __init__(self, num_seq, seq_len, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
        self.num_seq, self.seq_len, self.mean, self.std = num_seq, seq_len, mean, std
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None \
            else torch.device(device)
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.pinned = [None, None]
        self.staged = [None, None]
        self.done = [None, None]
        self.read_done = [None, None]      # main-stream event: the kernel that last READ staged[f]
        self.flip = 0

    def __call__(self, frames):
        f = self.flip
        self.flip = 1 - f
        if frames.is_cuda:
            return tr(frames, self.num_seq, self.seq_len, self.mean, self.std)
        if self.done[f] is not None:
            self.done[f].synchronize()         # the transfer that last used this pinned buffer
        if not frames.is_pinned():
            if self.pinned[f] is None or self.pinned[f].shape != frames.shape or \
                    self.pinned[f].dtype != frames.dtype:
                self.pinned[f] = torch.empty(frames.shape, dtype=frames.dtype).pin_memory()
            self.pinned[f].copy_(frames)
            frames = self.pinned[f]
        main = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self.copy_stream):
            if self.staged[f] is None or self.staged[f].shape != frames.shape or \
                    self.staged[f].dtype != frames.dtype:
                self.staged[f] = torch.empty(frames.shape, dtype=frames.dtype, device=self.device)
            elif self.read_done[f] is not None:
                # only the kernel that last read THIS buffer (two calls ago), not everything the
                # main stream has queued since: the transfer of batch i+1 runs under step i
                self.copy_stream.wait_event(self.read_done[f])
            self.staged[f].copy_(frames, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self.done[f] = ev
        main.wait_stream(self.copy_stream)
        out = tr(self.staged[f], self.num_seq, self.seq_len, self.mean, self.std)
        ev = torch.cuda.Event()
        ev.record(main)
        self.read_done[f] = ev
        return out


# ---- five/ten-crop test clips from raw frames ---------------------------------------------------------------

def _cubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def resample_tables(n_in, n_out):
    """PIL's BICUBIC coefficients for one axis of `Image.resize` on 8-bit pixels, n_in samples -> n_out:
    (xmin int32 (n_out,), K int32 (n_out, taps)) with result[xx] = clip8((2^21 + sum_i K[xx, i] *
    src[xmin[xx] + i]) >> 22).  Computed in Python floats (IEEE doubles) in PIL's order of operations; rows
    with fewer than `taps` = 2*ceil(support) + 1 samples are padded with zero taps."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError("coclr_amd: resample_tables needs n_in, n_out >= 1")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    taps = int(math.ceil(support)) * 2 + 1
    xmin = np.zeros(n_out, dtype=np.int32)
    K = np.zeros((n_out, taps), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        w = [_cubic((i + lo - center + 0.5) * ss) for i in range(hi - lo)]
        ww = 0.0
        for v in w:
            ww += v
        xmin[xx] = lo
        for i, v in enumerate(w):
            k = v / ww if ww != 0.0 else v
            K[xx, i] = int(k * 4194304.0 + 0.5) if k >= 0 else int(k * 4194304.0 - 0.5)
    return xmin, K


def five_crop_boxes(W, H, size, where=(5, 1, 2, 3, 4)):
    """Top-left corners [(x0, y0)] of FiveCrop(size, where=k) on a W x H frame for every k of `where`
    (utils/augmentation.py:61-88: 1 = top left, 2 = top right, 3 = bottom left, 4 = bottom right, 5 = centre,
    with Python's round-half-to-even for the centre).  Square crops only."""
    W, H, size = int(W), int(H), int(size)
    if size < 1 or size > H or size > W:
        raise ValueError("coclr_amd: requested crop size %d is bigger than input size %s" % (size, (H, W)))
    at = {1: (0, 0), 2: (W - size, 0), 3: (0, H - size), 4: (W - size, H - size),
          5: (int(round((W - size) / 2.)), int(round((H - size) / 2.)))}
    out = []
    for k in where:
        if k not in at:
            raise ValueError("coclr_amd: FiveCrop has no position %r" % (k,))
        out.append(at[k])
    return out


def test_frame_index(total, num_frames, ds=1):
    """Frame indices of the test-mode clips of a video of `total` frames (dataset/lmdb_dataset.py:111-122):
    int64 (n_clips, num_frames).  Clips of num_frames*ds frames start every num_frames*ds//2 - 1 frames; a
    video no longer than one clip gives ONE clip, right-aligned and left-padded with frame 0."""
    total, num_frames, ds = int(total), int(num_frames), int(ds)
    if total < 1 or num_frames < 1 or ds < 1:
        raise ValueError("coclr_amd: test_frame_index needs total, num_frames, ds >= 1")
    step = num_frames * ds // 2 - 1
    if step < 1:
        raise ValueError("coclr_amd: clips of %d frames at stride %d give a window step of %d" %
                         (num_frames, ds, step))
    seq = np.arange(num_frames, dtype=np.int64) * ds
    if total - num_frames * ds <= 0:
        idx = np.zeros_like(seq)
        keep = seq[seq < total]
        idx[len(idx) - len(keep):] = keep
        return idx[None, :]
    start = np.arange(0, total - num_frames * ds + 1, step, dtype=np.int64)
    return seq[None, :] + start[:, None]


test_frame_index.__test__ = False        # (a product function whose name pytest would collect)

_TABLES = {}        # (cw, ch, S, device) -> (xmin, xk, ymin, yk) on the device, in the kernel's layout


def _device_tables(cw, ch, S, device):
    key = (cw, ch, S, str(device))
    if key not in _TABLES:
        Sp = (S + 3) & ~3
        tabs = []
        for n_in in (cw, ch):
            lo, K = resample_tables(n_in, S)
            lo_p = np.zeros(Sp, dtype=np.int32)
            lo_p[:S] = lo
            K_p = np.zeros((K.shape[1], Sp), dtype=np.int32)       # tap-major: one 16-byte load per tap
            K_p[:, :S] = K.T
            tabs += [torch.from_numpy(lo_p).to(device), torch.from_numpy(K_p).to(device)]
        _TABLES[key] = tuple(tabs)
    return _TABLES[key]


def _crop_wh(crop_size):
    cw, ch = (crop_size, crop_size) if isinstance(crop_size, int) else crop_size
    return int(cw), int(ch)


def check_frame_index(frame_index, F):
    """`frame_index` (n_clips, T) of anything array-like -> int32 host tensor, refused here, on the host, when
    an index is outside [0, F): the kernel reads the indices on the device."""
    idx = torch.as_tensor(np.asarray(frame_index.cpu() if torch.is_tensor(frame_index) else frame_index))
    if idx.dim() != 2 or idx.numel() == 0 or idx.is_floating_point():
        raise ValueError("coclr_amd: frame_index must be integers of shape (n_clips, T), got %s %s" %
                         (idx.dtype, tuple(idx.shape)))
    lo, hi = int(idx.min()), int(idx.max())
    if lo < 0 or hi >= F:
        raise IndexError("coclr_amd: frame_index spans %d..%d but the video has %d frames" % (lo, hi, F))
    return idx.to(torch.int32).contiguous()


def check_crops(boxes, flips, cw, ch, W, H):
    boxes, flips = list(boxes), list(flips)
    if not boxes or len(boxes) != len(flips):
        raise ValueError("coclr_amd: need one flip per crop box, got %d boxes and %d flips" %
                         (len(boxes), len(flips)))
    crops = []
    for (x0, y0), fl in zip(boxes, flips):
        x0, y0, fl = int(x0), int(y0), int(fl)
        if x0 < 0 or y0 < 0 or x0 + cw > W or y0 + ch > H or fl not in (0, 1):
            raise ValueError("coclr_amd: crop (%d, %d, flip %d) of %dx%d leaves the %dx%d frame" %
                             (x0, y0, fl, cw, ch, W, H))
        crops.append((x0, y0, fl))
    return crops


# ---- ColorJitter (utils/augmentation.py:219-320) ------------------------------------------------------------

# op kinds of a program, as csrc/staging.hip takes them: [(kind, parameter)] in order of application
JITTER_NOP, JITTER_BRIGHTNESS, JITTER_CONTRAST, JITTER_SATURATION, JITTER_HUE, JITTER_GRAY = range(6)
AUGMENT_BLUR, AUGMENT_FLIP = 6, 7       # the two kinds coclr_augment_clips adds to the six of the jitter
BLUR_MAX_RADIUS = 16.0                  # the kernel's design limit; the reference's sigma in [0.1, 2] needs 1.375
JITTER_MAX_OPS = 8
JITTER_MAX_PIXELS = 224 * 224        # one workgroup holds the frame in LDS


def hue_shift_byte(hue_factor):
    """What torchvision 0.5's adjust_hue adds to the uint8 H channel, `np.uint8(hue_factor * 255)`: truncated
    toward zero, modulo 256 (a negative factor wraps round)."""
    return int(hue_factor * 255) % 256


class ColorJitter:
    """The reference's ColorJitter as a source of programs: same argument checks, same ranges, and `draw`
    consumes the generator exactly as its `__call__` + `get_params` do, so with the same seed in front it yields
    what the reference applies.  `consistent=True` is draw(rng, 1) for the whole item, `seq_len=k` is
    draw(rng, n_frames / k) with group_size k, per-frame jitter is draw(rng, n_frames) with group_size 1."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0, p=1.0):
        self.brightness = self._check_input(brightness, 'brightness')
        self.contrast = self._check_input(contrast, 'contrast')
        self.saturation = self._check_input(saturation, 'saturation')
        self.hue = self._check_input(hue, 'hue', center=0, bound=(-0.5, 0.5), clip_first_on_zero=False)
        self.p = p

    @staticmethod
    def _check_input(value, name, center=1, bound=(0, float('inf')), clip_first_on_zero=True):
        if isinstance(value, numbers.Number):
            if value < 0:
                raise ValueError("coclr_amd: if %s is a single number, it must be non negative" % name)
            value = [center - value, center + value]
            if clip_first_on_zero:
                value[0] = max(value[0], 0)
        elif isinstance(value, (tuple, list)) and len(value) == 2:
            if not bound[0] <= value[0] <= value[1] <= bound[1]:
                raise ValueError("coclr_amd: %s values should be between %s" % (name, (bound,)))
        else:
            raise TypeError("coclr_amd: %s should be a single number or a list/tuple of length 2" % name)
        if value[0] == value[1] == center:          # nothing to draw: the op is dropped
            value = None
        return value

    def draw(self, rng=random, n_groups=1):
        """`n_groups` programs.  One `rng.random() < p` for the call; then per group a `rng.uniform` for
        brightness, contrast, saturation and hue in that order (those enabled) and one `rng.shuffle`."""
        if not rng.random() < self.p:
            return [[] for _ in range(n_groups)]
        programs = []
        for _ in range(n_groups):
            ops_ = []
            if self.brightness is not None:
                ops_.append((JITTER_BRIGHTNESS, rng.uniform(self.brightness[0], self.brightness[1])))
            if self.contrast is not None:
                ops_.append((JITTER_CONTRAST, rng.uniform(self.contrast[0], self.contrast[1])))
            if self.saturation is not None:
                ops_.append((JITTER_SATURATION, rng.uniform(self.saturation[0], self.saturation[1])))
            if self.hue is not None:
                ops_.append((JITTER_HUE, hue_shift_byte(rng.uniform(self.hue[0], self.hue[1]))))
            rng.shuffle(ops_)
            programs.append(ops_)
        return programs


def _check_op(kind, value, n_kinds, word):
    """One op of a program -> (kind, parameter as the kernel takes it): kinds 0..5 of the jitter, and with n_kinds = 8
    the blur and the flip of the training transform."""
    if isinstance(kind, bool) or kind not in range(n_kinds) or int(kind) != kind:
        raise ValueError("coclr_amd: no %s op kind %r" % (word, kind))
    kind, value = int(kind), float(value)
    if kind == AUGMENT_FLIP:
        return kind, 0.0
    if kind == AUGMENT_BLUR:
        if not 0.0 <= value <= BLUR_MAX_RADIUS:
            raise ValueError("coclr_amd: a blur box radius lies in [0, %g] (blur_box_radius), got %r" %
                             (BLUR_MAX_RADIUS, value))
    elif kind == JITTER_HUE and not (0 <= value <= 255 and value == int(value)):
        raise ValueError("coclr_amd: a hue shift is a byte (hue_shift_byte), got %r" % (value,))
    elif kind == JITTER_GRAY and value not in (0.0, 1.0, 2.0):
        raise ValueError("coclr_amd: gray takes channel 0, 1 or 2, got %r" % (value,))
    elif not math.isfinite(value):
        raise ValueError("coclr_amd: jitter factor %r is not finite" % (value,))
    return kind, value


def _program_tables(programs, n_kinds, word):
    """The body of program_tables and augment_tables.  A batch names few distinct programs (one per clip, or per frame
    of a gray clip), so each is checked once."""
    programs = [list(prog) for prog in programs]
    if not programs:
        raise ValueError("coclr_amd: need at least one %s program" % word)
    P = max(1, max(len(prog) for prog in programs))
    if P > JITTER_MAX_OPS:
        raise ValueError("coclr_amd: one %s program has %d ops, the kernel takes %d" % (word, P, JITTER_MAX_OPS))
    rows, kinds, params = {}, [], []
    for prog in programs:
        key = tuple(tuple(op) for op in prog)
        if key not in rows:
            checked = [_check_op(kind, value, n_kinds, word) for kind, value in prog] + [(0, 0.0)] * (P - len(prog))
            rows[key] = ([k for k, _ in checked], [v for _, v in checked])
        kinds.append(rows[key][0])
        params.append(rows[key][1])
    return torch.from_numpy(np.array(kinds, dtype=np.int32)), torch.from_numpy(np.array(params, dtype=np.float32))


def program_tables(programs):
    """[[(kind, parameter)]] -> host tables (kinds int32 (G, P), params fp32 (G, P)), P = the longest program
    (at least 1), shorter ones padded with no-ops.  Refuses what the kernel does not know."""
    return _program_tables(programs, 6, "jitter")


def _upload(frames_u8, device):
    """`frames_u8` contiguous on `device`, which defaults to the frames' own device, or the current GPU; a batch
    (B, n, H, W, 3) as its B * n frames."""
    if device is None:
        device = frames_u8.device if frames_u8.is_cuda else torch.device("cuda", torch.cuda.current_device())
    frames = frames_u8.contiguous().to(device)
    return frames.flatten(0, 1) if frames.dim() == 5 else frames


def _check_out(out, shape, fp32=False):
    if out is not None and (tuple(out.shape) != shape or not out.is_contiguous() or
                            (fp32 and out.dtype != torch.float32)):
        raise ValueError("coclr_amd: out must be contiguous %s%s, got %s" %
                         ("fp32 " if fp32 else "", shape, tuple(out.shape)))


def _run_programs(launch, tables, what, frames_u8, programs, group_size, T, mean, std, out, device):
    """The body of color_jitter and augment: `tables` makes the host tables of `programs`, `launch` runs them."""
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or frames_u8.dtype != torch.uint8:
        raise ValueError("coclr_amd: frames must be uint8 (N, H, W, 3), got %s %s" %
                         (frames_u8.dtype, tuple(frames_u8.shape)))
    N, H, W = frames_u8.shape[:3]
    group_size, T = int(group_size), int(T)
    if N < 1 or T < 1 or N % T != 0:
        raise ValueError("coclr_amd: %d frames do not make clips of %d" % (N, T))
    if H * W > JITTER_MAX_PIXELS or H * W < 1:
        raise ValueError("coclr_amd: %s takes frames of up to 224 x 224 pixels, got %d x %d" % (what, H, W))
    kinds, params = tables(programs)
    if group_size < 1 or kinds.shape[0] * group_size < N:
        raise ValueError("coclr_amd: %d programs for groups of %d frames do not cover %d frames" %
                         (kinds.shape[0], group_size, N))
    frames = _upload(frames_u8, device)
    if out is None:
        out = torch.empty(N // T, 3, T, H, W, dtype=torch.float32, device=frames.device)
    launch(frames, kinds.to(frames.device), params.to(frames.device), group_size, T, mean, std, out,
           host_tables=(kinds, params))
    return out


def color_jitter(frames_u8, programs, group_size, T, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None, device=None):
    """ColorJitter / RandomGray -> ToTensor -> Normalize of `frames_u8` (N, H, W, 3) uint8 (host or device) in ONE
    launch: (N/T, 3, T, H, W) fp32 on the device, frame n at clip n // T, position n % T, after running program
    n // group_size of `programs` ([[(kind, parameter)]], e.g. ColorJitter.draw).  Bit-identical to the
    reference's PIL ops; an empty program is ToTensor + Normalize alone.  Frames up to 224 x 224."""
    return _run_programs(ops.color_jitter_clips, program_tables, "color_jitter", frames_u8, programs, group_size, T,
                         mean, std, out, device)


def stage_crops_on_device(frames, slot_frame, crops, cw, ch, S, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None,
                          jitter=None):
    """The launch alone: `frames` (F, H, W, 3) uint8 and `slot_frame` (n_clips, T) int32 already on the device
    and checked (check_frame_index, check_crops).  Up to 16 crops per launch; more are cut into launches.
    `jitter`: one program per crop; the crops are then resized to bytes and jittered in one further launch."""
    n_clips, T = slot_frame.shape
    if out is None:
        out = torch.empty(len(crops), n_clips, 3, T, S, S, dtype=torch.float32, device=frames.device)
    xmin, xk, ymin, yk = _device_tables(cw, ch, S, frames.device)
    if jitter is not None:
        jitter = list(jitter)
        if len(jitter) != len(crops):
            raise ValueError("coclr_amd: need one jitter program per crop, got %d programs and %d crops" %
                             (len(jitter), len(crops)))
        _check_out(out, (len(crops), n_clips, 3, T, S, S))
        if S * S > JITTER_MAX_PIXELS:
            raise ValueError("coclr_amd: color_jitter takes frames of up to 224 x 224 pixels, got %d x %d" % (S, S))
        program_tables(jitter)                            # refuse a bad program before anything is launched
        u8 = torch.empty(len(crops), n_clips * T, S, S, 3, dtype=torch.uint8, device=frames.device)
        for k in range(0, len(crops), 16):
            ops.resize_crops_u8(frames, slot_frame, crops[k:k + 16], cw, ch, S, xmin, xk, ymin, yk, u8[k:k + 16])
        color_jitter(u8.view(-1, S, S, 3), jitter, n_clips * T, T, mean, std,
                     out=out.view(len(crops) * n_clips, 3, T, S, S), device=frames.device)
        return out
    for k in range(0, len(crops), 16):
        ops.stage_crops(frames, slot_frame, crops[k:k + 16], cw, ch, S, xmin, xk, ymin, yk, mean, std,
                        out[k:k + 16])
    return out


def stage_crops(frames_u8, frame_index, boxes, flips, crop_size, out_size, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                out=None, device=None, jitter=None):
    """One video's decoded frames -> every crop x clip of the test protocol, (n_crops, n_clips, 3, T, S, S)
    fp32 on the device: per crop `flip the frame -> crop the box at boxes[k] -> Image.resize((S, S), BICUBIC)
    -> ColorJitter -> ToTensor -> Normalize`, bit-identical to that chain.  `jitter=None` (one launch) leaves
    the ColorJitter out; otherwise it is one program per crop (ColorJitter.draw(rng)[0] for each crop in turn:
    the reference jitters all frames of a crop alike) and the call is two launches, resize then jitter.
    frames_u8: (F, H, W, 3) uint8 on the host (uploaded once) or the device.  frame_index: (n_clips, T) frame
    of every clip position, checked on the host.  boxes: [(x0, y0)] in the FLIPPED frame where flips[k] is 1.
    crop_size: int or (width, height).  `device` defaults to the frames' device, or the current GPU."""
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or frames_u8.dtype != torch.uint8:
        raise ValueError("coclr_amd: frames must be uint8 (F, H, W, 3), got %s %s" %
                         (frames_u8.dtype, tuple(frames_u8.shape)))
    F, H, W = frames_u8.shape[:3]
    cw, ch = _crop_wh(crop_size)
    crops = check_crops(boxes, flips, cw, ch, W, H)
    idx = check_frame_index(frame_index, F)
    frames = _upload(frames_u8, device)
    return stage_crops_on_device(frames, idx.to(frames.device), crops, cw, ch, int(out_size), mean, std, out, jitter)


# ---- the training transform (main_nce.py:366-392; utils/augmentation.py:90-216,357-444) -----------------------------

PLAN_HEAD = 5                           # packed plan, per clip: half, x0, y0, w, h, then T x 8 kinds, T x 8 parameters


def blur_box_radius(sigma):
    """ImageFilter.GaussianBlur(radius=sigma) as PIL runs it: three box blurs of this (fractional) radius per
    direction -- the number the kernel takes (kind 6).  PIL's C evaluates the formula in `float` variables (sigma
    itself arrives as one) with the square root and the floor in double, and the last bit matters: the same
    formula in doubles gives another fp32 radius for four sigmas in ten and other bytes for about one in 250
    (1.4 is one).  So every float operation below is a numpy float32 operation of its own."""
    sigma = float(sigma)
    if not sigma >= 0.0 or not math.isfinite(sigma):
        raise ValueError("coclr_amd: a blur sigma is a finite number >= 0, got %r" % (sigma,))
    f = np.float32
    r = f(sigma)
    s2 = r * r / f(3)
    L = f(math.sqrt(12.0 * float(s2) + 1.0))
    l = f(math.floor((float(L) - 1.0) / 2.0))
    a = (f(2) * l + f(1)) * (l * (l + f(1)) - f(3) * s2)
    a = a / (f(6) * (s2 - (l + f(1)) * (l + f(1))))
    out = l + a
    assert out.dtype == np.float32
    return float(out)


def augment_tables(programs):
    """program_tables for coclr_augment_clips: kinds 0..5 as there, plus (6, r_f) -- blur, r_f from blur_box_radius,
    0 <= r_f <= 16 -- and (7, anything) -- horizontal flip."""
    return _program_tables(programs, 8, "augment")


def augment(frames_u8, programs, group_size, T, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None, device=None):
    """color_jitter with the blur and the flip admitted (augment_tables): `frames_u8` (N, H, W, 3) uint8 ->
    (N/T, 3, T, H, W) fp32 on the device in one launch, frame n running program n // group_size."""
    return _run_programs(ops.augment_clips, augment_tables, "augment", frames_u8, programs, group_size, T, mean, std,
                         out, device)


class TrainTransform:
    """The reference's training transform (main_nce.py:366-390) as a source of PLANS: `draw` consumes `random` and
    `np.random` exactly as `transform(seq)` does on 2 * seq_len frames and says what it would do; stage_train_clips
    does it on the GPU.  main_coclr.py:447-473 is the same chain at `seq_len = args.seq_len * 2` on 4 T frames, RGB and
    flow: TrainTransform(img_dim, 2 * T) draws its plans and stage_two_stream_clips stages them (the two-stream
    section below; tests/golden/two_stream_transform.pt).  A plan is a dict
        half      (a, b): which half of the 2T frames clip 0 / clip 1 reads (0 or 1)
        box       ((x0, y0, w, h), (x0, y0, w, h)): RandomSizedCrop's box per clip (the whole frame when its draw
                  does not fit)
        programs  per clip T programs [(kind, parameter)], one per frame: ColorJitter's ops in their shuffled
                  order, gray (the channel differs from frame to frame), blur (6, box radius), flip (7, 0)."""

    def __init__(self, img_dim, seq_len, bottom_area=0.2, jitter=(0.4, 0.4, 0.4, 0.1), p_jitter=0.8, p_gray=0.2,
                 blur_sigma=(0.1, 2.0), p_blur=0.5, p_flip=0.5, p_base=0.3, weights=(0.5, 0.5), consistent=False, p=1.0):
        if consistent:
            raise ValueError("coclr_amd: RandomSizedCrop(consistent=True) retries and falls back to another resample; "
                             "the training scripts never use it (the classifier script does: ClassifierTransform)")
        if p != 1.0:
            raise ValueError("coclr_amd: RandomSizedCrop(p != 1.0) centre-crops without a resize; the training "
                             "scripts never use it")
        self.img_dim, self.seq_len = int(img_dim), int(seq_len)
        if self.img_dim < 1 or self.seq_len < 1:
            raise ValueError("coclr_amd: img_dim and seq_len must be >= 1")
        self.bottom_area = bottom_area
        self.jitter = ColorJitter(*jitter, p=1.0)
        self.p_jitter, self.p_gray, self.p_blur, self.p_flip, self.p_base = p_jitter, p_gray, p_blur, p_flip, p_base
        self.blur_sigma = tuple(blur_sigma)
        blur_box_radius(self.blur_sigma[0]), blur_box_radius(self.blur_sigma[1])
        if blur_box_radius(max(self.blur_sigma)) > BLUR_MAX_RADIUS:
            raise ValueError("coclr_amd: blur sigma %r needs a box radius over %g" % (blur_sigma, BLUR_MAX_RADIUS))
        self.weights = list(weights)

    def _crop(self, W, H, rng):
        rng.random()                                            # `random.random() < p`, p = 1.0
        target_area = rng.uniform(self.bottom_area, 1) * (W * H)
        aspect_ratio = rng.uniform(3. / 4, 4. / 3)
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if rng.random() < 0.5:
            w, h = h, w
        if w <= W and h <= H:
            if w < 1 or h < 1:
                raise ValueError("coclr_amd: RandomSizedCrop drew an empty %d x %d box" % (w, h))
            x1 = rng.randint(0, W - w)
            y1 = rng.randint(0, H - h)
            return (x1, y1, w, h)
        return (0, 0, W, H)                                     # no retry in this mode: the frame as it is

    def _flip(self, rng):
        return [(AUGMENT_FLIP, 0.0)] if rng.random() < self.p_flip else []

    def _null(self, W, H, rng, np_rng):
        box = self._crop(W, H, rng)
        return box, [self._flip(rng)] * self.seq_len

    def _base(self, W, H, rng, np_rng):
        box = self._crop(W, H, rng)
        prog = []
        if not self.p_jitter < rng.random():                    # transforms.RandomApply
            prog += self.jitter.draw(rng, 1)[0]
        gray = None
        if rng.random() < self.p_gray:
            gray = [int(np_rng.choice(3)) for _ in range(self.seq_len)]
        tail = []
        if not self.p_blur < rng.random():
            tail.append((AUGMENT_BLUR, blur_box_radius(rng.uniform(self.blur_sigma[0], self.blur_sigma[1]))))
        tail += self._flip(rng)
        if gray is None:
            return box, [prog + tail] * self.seq_len
        return box, [prog + [(JITTER_GRAY, ch)] + tail for ch in gray]

    def draw(self, W, H, rng=random, np_rng=np.random):
        """The plan of one sample of 2 * seq_len frames of W x H."""
        W, H = int(W), int(H)
        if W < 1 or H < 1:
            raise ValueError("coclr_amd: frames of %d x %d" % (W, H))
        if rng.choices(range(2), weights=self.weights)[0] == 0:             # TwoClipTransform
            tr1 = self._base if rng.random() < self.p_base else self._null
            tr2 = self._base if rng.random() < self.p_base else self._null
            half = (0, 1)
        else:                                                               # OneClipTransform
            tr1, tr2 = (self._base, self._null) if rng.random() < 0.5 else (self._null, self._base)
            half = (0, 0) if rng.random() < 0.5 else (1, 1)
        box1, progs1 = tr1(W, H, rng, np_rng)
        box2, progs2 = tr2(W, H, rng, np_rng)
        return {"half": half, "box": (box1, box2), "programs": ([list(p) for p in progs1], [list(p) for p in progs2])}


def pack_plan(plan, T):
    """A plan as ONE tensor of fixed shape, float64 (2, 5 + 16 T): per clip half, x0, y0, w, h, then T x 8 op kinds
    and T x 8 parameters (doubles hold both exactly).  What a dataset returns beside its frames: the default
    collate stacks it, and stage_train_clips takes the stacked (B, 2, 5 + 16 T) tensor as `plans`."""
    T = int(T)
    t = torch.zeros(2, PLAN_HEAD + 2 * T * JITTER_MAX_OPS, dtype=torch.float64)
    for c in range(2):
        progs = plan["programs"][c]
        if len(progs) != T:
            raise ValueError("coclr_amd: a plan has one program per frame, got %d for T = %d" % (len(progs), T))
        t[c, 0] = plan["half"][c]
        t[c, 1:PLAN_HEAD] = torch.tensor([float(v) for v in plan["box"][c]], dtype=torch.float64)
        kinds, params = t[c, PLAN_HEAD:].view(2, T, JITTER_MAX_OPS)
        for f, prog in enumerate(progs):
            if len(prog) > JITTER_MAX_OPS:
                raise ValueError("coclr_amd: a program has %d ops, the kernel takes %d" % (len(prog), JITTER_MAX_OPS))
            for j, (kind, value) in enumerate(prog):
                kinds[f, j], params[f, j] = kind, value
    return t


def unpack_plan(packed):
    """The plan pack_plan packed (no-ops dropped)."""
    if packed.dim() != 2 or packed.shape[0] != 2 or (packed.shape[1] - PLAN_HEAD) % (2 * JITTER_MAX_OPS) != 0 or \
            packed.shape[1] <= PLAN_HEAD:
        raise ValueError("coclr_amd: a packed plan is (2, 5 + 16 T), got %s" % (tuple(packed.shape),))
    T = (packed.shape[1] - PLAN_HEAD) // (2 * JITTER_MAX_OPS)
    packed = packed.detach().cpu().to(torch.float64)
    half, box, programs = [], [], []
    for c in range(2):
        head = packed[c, :PLAN_HEAD].tolist()
        if any(v != int(v) for v in head):
            raise ValueError("coclr_amd: a packed plan's half and box are integers, got %r" % (head,))
        half.append(int(head[0]))
        box.append(tuple(int(v) for v in head[1:]))
        rows = packed[c, PLAN_HEAD:].view(2, T, JITTER_MAX_OPS)
        same = bool((rows == rows[:, :1]).all())               # one program for the clip: read it once
        kinds, params = (rows[:, :1] if same else rows).tolist()
        progs = [[(int(k) if k == int(k) else k, v) for k, v in zip(kk, vv) if k != 0] for kk, vv in zip(kinds, params)]
        programs.append([list(progs[0]) for _ in range(T)] if same else progs)
    return {"half": tuple(half), "box": tuple(box), "programs": tuple(programs)}


_BOX_TABLES = {}        # (n_in, S) -> int32 (1 + taps, Sp): min then k, in the kernel's layout


def _box_table(n_in, S):
    key = (n_in, S)
    if key not in _BOX_TABLES:
        Sp = (S + 3) & ~3
        lo, K = resample_tables(n_in, S)
        if K.shape[1] > 64:
            raise ValueError("coclr_amd: a box side of %d to %d needs %d taps, the kernel takes 64" %
                             (n_in, S, K.shape[1]))
        t = np.zeros((1 + K.shape[1], Sp), dtype=np.int32)
        t[0, :S] = lo
        t[1:, :S] = K.T
        _BOX_TABLES[key] = t
    return _BOX_TABLES[key]


def _plan_list(plans, unpack, packed_dim):
    """`plans` as a list of plan dicts: a list of them already, or packed tensors stacked (one alone has `packed_dim`
    dimensions)."""
    if torch.is_tensor(plans):
        return [unpack(p) for p in (plans[None] if plans.dim() == packed_dim else plans)]
    return list(plans)


def _axis_tables(keys, make):
    """Every distinct table of the batch once, one after the other, per axis.  keys: per clip (x key, y key);
    make(key): the key's int32 (1 + taps, P) table.  Returns (xtab, ytab, per clip [x offset, y offset, x taps, y taps]:
    the four table words of its descriptor)."""
    bufs, at, fill, words = ([], []), ({}, {}), [0, 0], []
    for pair in keys:
        offs = []
        for axis, key in enumerate(pair):
            if key not in at[axis]:
                t = make(key)
                at[axis][key] = (fill[axis], t.shape[0] - 1)
                bufs[axis].append(t.reshape(-1))
                fill[axis] += t.size
            offs.append(at[axis][key])
        words.append([offs[0][0], offs[1][0], offs[0][1], offs[1][1]])
    return torch.from_numpy(np.concatenate(bufs[0])), torch.from_numpy(np.concatenate(bufs[1])), words


def check_train_plans(plans, B, T, W, H, slots=None):
    """`plans` (a list of B plans, or the stacked packed tensor) -> (descriptor rows without table fields, per-frame
    programs of all B * 2 clips), refused here, on the host, when a plan is not one the kernels take.
    `slots`: two_stream_slots(reverse) for two-stream samples of 4 T frames.  A plan clip then has 2 T programs and
    becomes one clip of T frames per slot (clip c, stream s) that names it: quarter 2 half[c] + s of the sample's
    frames, box[c], programs s T .. s T + T - 1.  The rows are slot-major -- len(slots) * B clips -- as the outputs are."""
    plans = _plan_list(plans, unpack_plan, 2)
    if len(plans) != B:
        raise ValueError("coclr_amd: %d plans for %d samples" % (len(plans), B))
    per_clip = T if slots is None else 2 * T
    checked = []
    for plan in plans:
        if len(plan["half"]) != 2 or len(plan["box"]) != 2 or len(plan["programs"]) != 2:
            raise ValueError("coclr_amd: a plan names two clips")
        checked.append([])
        for c in range(2):
            half = plan["half"][c]
            x0, y0, w, h = plan["box"][c]
            if half not in (0, 1) or isinstance(half, bool):
                raise ValueError("coclr_amd: a clip reads half 0 or 1 of the frames, got %r" % (half,))
            if any(int(v) != v for v in (x0, y0, w, h)) or x0 < 0 or y0 < 0 or w < 1 or h < 1 or x0 + w > W or y0 + h > H:
                raise ValueError("coclr_amd: box (%r, %r, %r, %r) leaves the %d x %d frame" % (x0, y0, w, h, W, H))
            progs = [list(p) for p in plan["programs"][c]]
            if len(progs) != per_clip:
                raise ValueError("coclr_amd: a plan has one program per frame%s, got %d for T = %d" %
                                 ("" if slots is None else " of both streams, 2 T", len(progs), T))
            checked[-1].append((int(half), (int(x0), int(y0), int(w), int(h)), progs))
    rows, programs = [], []
    if slots is None:
        for b, clips in enumerate(checked):
            for half, box, progs in clips:
                rows.append((b * 2 * T + half * T, T) + box)
                programs.append(progs)
    else:
        for c, s in slots:
            for b, clips in enumerate(checked):
                half, box, progs = clips[c]
                rows.append((b * 4 * T + (2 * half + s) * T, T) + box)
                programs.append(progs[s * T:(s + 1) * T])
    distinct = {tuple(tuple(op) for op in p) for clips in checked for _, _, progs in clips for p in progs}
    augment_tables([list(p) for p in distinct])                    # refuses a bad op
    return rows, programs


def _train_tables(rows, programs, rag, T, S):
    """The body of train_tables and train_tables_ragged: `rows` and `programs` of check_train_plans, `rag` the words
    that follow each clip's ten (none when the batch has one frame size)."""
    xtab, ytab, words = _axis_tables([(row[4], row[5]) for row in rows], lambda n_in: _box_table(n_in, S))
    desc = torch.tensor([list(row) + w + r for row, w, r in zip(rows, words, rag)], dtype=torch.int32)
    # one program per clip where its frames agree, else (a gray clip: the channel is per frame) one per frame
    per_clip = all(all(p == progs[0] for p in progs) for progs in programs)
    flat = [progs[0] for progs in programs] if per_clip else [p for progs in programs for p in progs]
    kinds, params = augment_tables(flat)
    return desc, xtab, ytab, kinds, params, T if per_clip else 1


def train_tables(plans, B, T, W, H, S, slots=None):
    """The host side of stage_train_clips for B samples of 2 T frames of W x H staged to S x S: checks the plans and
    returns (desc int32 (2B, 10), xtab, ytab int32, kinds int32 (G, P), params fp32 (G, P), group_size) as the
    two entry points take them, all on the host.  May be computed ahead (stage_train_clips(tables=)).
    `slots`: as check_train_plans takes it, for samples of 4 T frames; desc is then (len(slots) B, 10)."""
    rows, programs = check_train_plans(plans, B, T, W, H, slots)
    return _train_tables(rows, programs, [[]] * len(rows), T, S)


def _stage_train(resize, frames, device, tables, lead, T, S, mean, std, out):
    """The tail of every stage_train_clips_* and stage_two_stream_clips_*: `out` checked, the frames uploaded, the
    two launches.  `frames`: (B, n, H, W, 3), or the flat bytes of a RaggedFrames; `resize`: the form of
    ops.resize_boxes_u8 that takes them; `lead`: the leading dimensions of the result, lead + (3, T, S, S), whose
    product is the number of clips in `tables` -- clip k of the descriptors is clip k of the result."""
    desc, xtab, ytab, kinds, params, group_size = tables
    shape, n_clips = tuple(lead) + (3, T, S, S), desc.shape[0]
    assert math.prod(lead) == n_clips
    _check_out(out, shape)
    frames = _upload(frames, device)
    device = frames.device
    u8 = torch.empty(n_clips * T, S, S, 3, dtype=torch.uint8, device=device)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=device)
    resize(frames, desc.to(device), desc, xtab.to(device), ytab.to(device), T, S, u8)
    ops.augment_clips(u8, kinds.to(device), params.to(device), group_size, T, mean, std,
                      out.view(n_clips, 3, T, S, S), host_tables=(kinds, params))
    return out


def _result_lead(slots, B):
    """The leading dimensions of a staged batch: (B, 2), or two streams' (2, 2, B) / (3, B) (TwoStreamClips)."""
    return (B, 2) if slots is None else (2, 2, B) if len(slots) == 4 else (len(slots), B)


def _train_clips(who, slots, frames_u8, plans, out_size, mean, std, out, device, tables=None):
    """The body of stage_train_clips (slots None: a sample is 2 T frames) and stage_two_stream_clips (slots of
    two_stream_slots: 4 T frames)."""
    parts = 2 if slots is None else 4
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() not in (4, 5) or frames_u8.shape[-1] != 3:
        raise ValueError("coclr_amd: frames must be uint8 (B, %dT, H, W, 3) or (%dT, H, W, 3), got %s %s" %
                         (parts, parts, frames_u8.dtype, tuple(frames_u8.shape)))
    if frames_u8.dim() == 4:
        frames_u8 = frames_u8[None]
        if isinstance(plans, dict):
            plans = [plans]
    B, n, H, W = frames_u8.shape[:4]
    if B < 1 or n < parts or n % parts != 0 or H < 1 or W < 1:
        raise ValueError("coclr_amd: a sample is %d T frames, got %s" % (parts, tuple(frames_u8.shape)))
    T, S = n // parts, int(out_size)
    if S < 1 or S * S > JITTER_MAX_PIXELS:
        raise ValueError("coclr_amd: %s takes an output size of 1..224, got %d" % (who, S))
    if tables is None:
        tables = train_tables(plans, B, T, W, H, S, slots)
    lead = _result_lead(slots, B)
    if tuple(tables[0].shape) != (math.prod(lead), 10):
        raise ValueError("coclr_amd: tables for %d clips, frames for %d" % (tables[0].shape[0], math.prod(lead)))
    return _stage_train(ops.resize_boxes_u8, frames_u8, device, tables, lead, T, S, mean, std, out)


def stage_train_clips(frames_u8, plans, out_size, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None, device=None,
                      tables=None):
    """Raw frames + the reference's draws -> the model's input, in TWO launches (coclr_resize_boxes_u8, then
    coclr_augment_clips): per clip `crop the box -> Image.resize((S, S), BICUBIC) -> ColorJitter -> RandomGray ->
    GaussianBlur -> RandomHorizontalFlip -> ToTensor -> Normalize`, bit-identical to the reference's classes.
    frames_u8: (B, 2T, H, W, 3) or (2T, H, W, 3) uint8, on the host (uploaded once, as bytes) or the device.
    plans: B plans of TrainTransform.draw, or their pack_plan tensors stacked (B, 2, 5 + 16 T).
    Returns (B, 2, 3, T, S, S) fp32 on the device: what `model(...)` takes after the script's `tr()`.
    A bad plan is refused here before anything is launched.  S up to 224 (the augment kernel's frame limit).
    `tables`: train_tables(plans, ...) computed ahead; `plans` is then not read."""
    return _train_clips("stage_train_clips", None, frames_u8, plans, out_size, mean, std, out, device, tables)


# ---- the classifier's transform (eval/main_classifier.py:729-744,216-220; utils/augmentation.py:21-58,90-146) --------

CLS_MAX_SIDE = 224                      # size and img_dim: what coclr_resize2_boxes and coclr_augment_clips take
CLS_MAX_TAPS = 64
CLS_PLAN_LEN = 9 + 2 * JITTER_MAX_OPS   # packed plan: form, region (4), resample (2), window (2), 8 kinds, 8 parameters
CLS_FORMS = ("box", "fallback")


def cls_fused():
    """COCLR_CLS_FUSED (default 1, read per call; PROVISIONAL: tools/cls_stage_step.py has measured one geometry,
    DESIGN.md 4.5e): stage_classifier_clips resamples twice in ONE launch (coclr_resize2_boxes); with 0 it chains two
    coclr_resize_boxes_u8 launches through a byte buffer, which cannot express the fallback form."""
    return os.environ.get("COCLR_CLS_FUSED", "1") != "0"


def draw_batch_flip(rng=random):
    """The ONE draw of T.RandomHorizontalFlip() the fine-tuning loop makes per batch, in the main process
    (utils/transforms.py:286-293): `flip=` of stage_classifier_clips."""
    return rng.random() < 0.5


def fallback_geometry(W, H, size):
    """RandomSizedCrop's fallback, Scale(size) then CenterCrop(size) (utils/augmentation.py:21-58,140-143), on a W x H
    frame: ((ow, oh), (cx, cy)) -- what the whole frame is resampled to (itself when its shorter side already is
    `size`) and where the size x size window starts, with Python's round-half-to-even."""
    W, H, size = int(W), int(H), int(size)
    if (W <= H and W == size) or (H <= W and H == size):
        ow, oh = W, H
    elif W < H:
        ow, oh = size, int(size * H / W)
    else:
        ow, oh = int(size * W / H), size
    return (ow, oh), (int(round((ow - size) / 2.)), int(round((oh - size) / 2.)))


class ClassifierTransform:
    """The transform of the fine-tuning / linear-probe loop (eval/main_classifier.py:729-744) as a source of PLANS:
    RandomSizedCrop(size, consistent=True, bottom_area) -> Scale(img_dim) -> ColorJitter(*jitter, p=p_jitter,
    consistent=True) (mode "train" only; "val" crops at random too, as the reference does).  `draw` consumes the
    generator exactly as `transform(seq)` does; stage_classifier_clips does the work on the GPU.  A plan is a dict
        form      "box" (an attempt fitted) or "fallback" (ten did not: Scale(size) + CenterCrop(size))
        region    (x0, y0, w, h) of the frame that is resampled: the drawn box, or the whole frame
        resample  (ow, oh) the region is resampled to: (size, size), or Scale's size of the whole frame
        window    (cx, cy) where the size x size window of that starts: (0, 0), or CenterCrop's corner
        program   ColorJitter's ops [(kind, parameter)] in their shuffled order, one program for the whole clip."""

    def __init__(self, img_dim, seq_len, size=224, bottom_area=0.2, jitter=(0.4, 0.4, 0.4, 0.1), p_jitter=0.3,
                 mode="train"):
        self.img_dim, self.seq_len, self.size = int(img_dim), int(seq_len), int(size)
        if self.img_dim < 1 or self.seq_len < 1 or self.size < 1:
            raise ValueError("coclr_amd: img_dim, seq_len and size must be >= 1")
        if self.img_dim > CLS_MAX_SIDE or self.size > CLS_MAX_SIDE:
            raise ValueError("coclr_amd: the classifier staging takes img_dim and size up to %d, got %d and %d" %
                             (CLS_MAX_SIDE, self.img_dim, self.size))
        if mode not in ("train", "val"):
            raise ValueError("coclr_amd: mode is 'train' or 'val', got %r" % (mode,))
        self.mode, self.bottom_area = mode, bottom_area
        self.jitter = ColorJitter(*jitter, p=p_jitter)

    def draw(self, W, H, rng=random):
        """The plan of one sample of seq_len frames of W x H."""
        W, H = int(W), int(H)
        if W < 1 or H < 1:
            raise ValueError("coclr_amd: frames of %d x %d" % (W, H))
        rng.random()                                            # `random.random() < p`, p = 1.0
        plan = None
        for _ in range(10):
            target_area = rng.uniform(self.bottom_area, 1) * (W * H)
            aspect_ratio = rng.uniform(3. / 4, 4. / 3)
            w = int(round(math.sqrt(target_area * aspect_ratio)))
            h = int(round(math.sqrt(target_area / aspect_ratio)))
            if rng.random() < 0.5:
                w, h = h, w
            if w <= W and h <= H:
                if w < 1 or h < 1:
                    raise ValueError("coclr_amd: RandomSizedCrop drew an empty %d x %d box" % (w, h))
                x1 = rng.randint(0, W - w)
                y1 = rng.randint(0, H - h)
                plan = {"form": "box", "region": (x1, y1, w, h), "resample": (self.size, self.size), "window": (0, 0)}
                break
        if plan is None:                                        # the fallback draws nothing
            resample, window = fallback_geometry(W, H, self.size)
            plan = {"form": "fallback", "region": (0, 0, W, H), "resample": resample, "window": window}
        plan["program"] = self.jitter.draw(rng, 1)[0] if self.mode == "train" else []
        return plan


def pack_cls_plan(plan):
    """A plan of ClassifierTransform.draw as ONE tensor of fixed shape, float64 (25,): form (0 box, 1 fallback), region,
    resample, window, then 8 op kinds and 8 parameters (doubles hold all of them exactly).  What a dataset returns
    beside its frames: the default collate stacks it, and stage_classifier_clips takes the stacked (B, 25) tensor."""
    if plan["form"] not in CLS_FORMS:
        raise ValueError("coclr_amd: a plan's form is one of %r, got %r" % (CLS_FORMS, plan["form"]))
    prog = list(plan["program"])
    if len(prog) > JITTER_MAX_OPS:
        raise ValueError("coclr_amd: a program has %d ops, the kernel takes %d" % (len(prog), JITTER_MAX_OPS))
    head = [CLS_FORMS.index(plan["form"])] + list(plan["region"]) + list(plan["resample"]) + list(plan["window"])
    if len(head) != 9:
        raise ValueError("coclr_amd: a plan has a region of 4, a resample of 2 and a window of 2 numbers")
    t = torch.zeros(CLS_PLAN_LEN, dtype=torch.float64)
    t[:9] = torch.tensor([float(v) for v in head], dtype=torch.float64)
    for j, (kind, value) in enumerate(prog):
        t[9 + j], t[9 + JITTER_MAX_OPS + j] = kind, value
    return t


def unpack_cls_plan(packed):
    """The plan pack_cls_plan packed (no-ops dropped)."""
    if packed.dim() != 1 or packed.shape[0] != CLS_PLAN_LEN:
        raise ValueError("coclr_amd: a packed classifier plan is (%d,), got %s" % (CLS_PLAN_LEN, tuple(packed.shape)))
    v = packed.detach().cpu().to(torch.float64).tolist()
    if any(x != int(x) for x in v[:9]) or int(v[0]) not in (0, 1):
        raise ValueError("coclr_amd: a packed plan's form and geometry are integers, got %r" % (v[:9],))
    head = [int(x) for x in v[:9]]
    kinds, params = v[9:9 + JITTER_MAX_OPS], v[9 + JITTER_MAX_OPS:]
    return {"form": CLS_FORMS[head[0]], "region": tuple(head[1:5]), "resample": tuple(head[5:7]),
            "window": tuple(head[7:9]),
            "program": [(int(k) if k == int(k) else k, p) for k, p in zip(kinds, params) if k != 0]}


def check_cls_plans(plans, B, W, H, size):
    """`plans` (a list of B plans, or the stacked packed tensor) -> (per clip (x0, y0, w, h, ow, oh, cx, cy), per clip
    program), refused here, on the host, when a plan is not one the kernel takes."""
    plans = _plan_list(plans, unpack_cls_plan, 1)
    if len(plans) != B:
        raise ValueError("coclr_amd: %d plans for %d samples" % (len(plans), B))
    rows, programs = [], []
    for plan in plans:
        if plan["form"] not in CLS_FORMS:
            raise ValueError("coclr_amd: a plan's form is one of %r, got %r" % (CLS_FORMS, plan["form"]))
        geo = tuple(plan["region"]) + tuple(plan["resample"]) + tuple(plan["window"])
        if len(geo) != 8 or any(isinstance(v, bool) or int(v) != v for v in geo):
            raise ValueError("coclr_amd: a plan's region, resample and window are 4 + 2 + 2 integers, got %r" % (geo,))
        x0, y0, w, h, ow, oh, cx, cy = (int(v) for v in geo)
        if x0 < 0 or y0 < 0 or w < 1 or h < 1 or x0 + w > W or y0 + h > H:
            raise ValueError("coclr_amd: region (%d, %d, %d, %d) leaves the %d x %d frame" % (x0, y0, w, h, W, H))
        if cx < 0 or cy < 0 or cx + size > ow or cy + size > oh:
            raise ValueError("coclr_amd: a %d x %d window at (%d, %d) leaves the %d x %d resample" %
                             (size, size, cx, cy, ow, oh))
        if plan["form"] == "box" and (ow, oh, cx, cy) != (size, size, 0, 0):
            raise ValueError("coclr_amd: a box plan resamples to (%d, %d) and keeps all of it, got %r" %
                             (size, size, (ow, oh, cx, cy)))
        rows.append((x0, y0, w, h, ow, oh, cx, cy))
        programs.append([tuple(op) for op in plan["program"]])
    program_tables([list(p) for p in {tuple(p) for p in programs}])            # refuses a bad op
    return rows, programs


_WIN_TABLES = {}        # (n_in, n_out, c0, size) -> int32 (1 + taps, P): min then k of columns c0 .. c0 + size - 1


def _window_table(n_in, n_out, c0, size):
    key = (n_in, n_out, c0, size)
    if key not in _WIN_TABLES:
        P = (size + 3) & ~3
        lo, K = resample_tables(n_in, n_out)
        if K.shape[1] > CLS_MAX_TAPS:
            raise ValueError("coclr_amd: a side of %d to %d needs %d taps, the kernel takes %d" %
                             (n_in, n_out, K.shape[1], CLS_MAX_TAPS))
        t = np.zeros((1 + K.shape[1], P), dtype=np.int32)
        t[0, :size] = lo[c0:c0 + size]
        t[1:, :size] = K[c0:c0 + size].T
        _WIN_TABLES[key] = t
    return _WIN_TABLES[key]


def _cls_sides(img_dim, size, who):
    S, size = int(img_dim), int(size)
    if S < 1 or size < 1 or S > CLS_MAX_SIDE or size > CLS_MAX_SIDE:
        raise ValueError("coclr_amd: %s takes img_dim and size of 1..%d, got %d and %d" % (who, CLS_MAX_SIDE, S, size))
    return S, size


def _classifier_tables(rows, programs, first, rag, T, S, size, flip):
    """The body of classifier_tables and classifier_tables_ragged: `rows` and `programs` of check_cls_plans, `first`
    each clip's first frame, `rag` the words that follow its fourteen (none when the batch has one frame size)."""
    tab2 = _window_table(size, S, 0, S)                  # size -> S whole: PIL's identity when they are equal
    xtab, ytab, words = _axis_tables([((w, ow, cx), (h, oh, cy)) for _, _, w, h, ow, oh, cx, cy in rows],
                                     lambda key: _window_table(key[0], key[1], key[2], size))
    desc = torch.tensor([[f, T] + list(row) + w + r for f, row, w, r in zip(first, rows, words, rag)], dtype=torch.int32)
    tail = [(AUGMENT_FLIP, 0.0)] if flip else []
    kinds, params = augment_tables([list(p) + tail for p in programs])
    direct = not flip and not any(programs)
    return desc, xtab, ytab, torch.from_numpy(tab2), kinds, params, direct


def classifier_tables(plans, B, T, W, H, img_dim, size=224, flip=False):
    """The host side of stage_classifier_clips for B samples of T frames of W x H: checks the plans and returns
    (desc int32 (B, 14), xtab, ytab int32, tab2 int32 (1 + taps, Sp), kinds int32 (B, P), params fp32 (B, P), direct)
    as the entry points take them, all on the host; `direct` says that no clip has a program and `flip` is off, so
    that one launch writes fp32.  May be computed ahead (stage_classifier_clips(tables=))."""
    B, T = int(B), int(T)
    S, size = _cls_sides(img_dim, size, "the classifier staging")
    rows, programs = check_cls_plans(plans, B, W, H, size)
    return _classifier_tables(rows, programs, [b * T for b in range(B)], [[]] * B, T, S, size, flip)


def _stage_classifier(ragged, frames, device, tables, B, T, S, size, mean, std, out):
    """The tail of stage_classifier_clips and stage_classifier_clips_ragged: `out` and the chained form checked, the
    frames uploaded, the launches.  `frames`: (B, T, H, W, 3), or with `ragged` the flat bytes of a RaggedFrames."""
    desc, xtab, ytab, tab2, kinds, params, direct = tables
    _check_out(out, (B, 3, T, S, S), fp32=True)
    fused = cls_fused()
    if not fused and bool((desc[:, 6:10] != torch.tensor([size, size, 0, 0], dtype=torch.int32)).any()):
        raise ValueError("coclr_amd: COCLR_CLS_FUSED=0 chains two box resizes and cannot express the fallback form "
                         "(a window of a whole-frame resample)")
    resize2, boxes = (ops.resize2_boxes_ragged, ops.resize_boxes_ragged_u8) if ragged else \
        (ops.resize2_boxes, ops.resize_boxes_u8)
    frames = _upload(frames, device)
    device = frames.device
    if out is None:
        out = torch.empty(B, 3, T, S, S, dtype=torch.float32, device=device)
    if fused and direct:
        resize2(frames, desc.to(device), desc, xtab.to(device), ytab.to(device), tab2.to(device), T, size, S, out, mean,
                std)
        return out
    u8 = torch.empty(B * T, S, S, 3, dtype=torch.uint8, device=device)
    if fused:
        resize2(frames, desc.to(device), desc, xtab.to(device), ytab.to(device), tab2.to(device), T, size, S, u8)
    else:
        # the same bytes from the entry points of the training staging: box -> size per clip (the table words and what
        # follows them kept), then the whole of that, which has one size, -> S
        d1 = desc[:, list(range(6)) + list(range(10, desc.shape[1]))].contiguous()
        taps2 = tab2.shape[0] - 1
        d2 = torch.tensor([[b * T, T, 0, 0, size, size, 0, 0, taps2, taps2] for b in range(B)], dtype=torch.int32)
        mid = torch.empty(B * T, size, size, 3, dtype=torch.uint8, device=device)
        flat2 = tab2.reshape(-1).to(device)
        boxes(frames, d1.to(device), d1, xtab.to(device), ytab.to(device), T, size, mid)
        ops.resize_boxes_u8(mid, d2.to(device), d2, flat2, flat2, T, S, u8)
    ops.augment_clips(u8, kinds.to(device), params.to(device), T, T, mean, std, out, host_tables=(kinds, params))
    return out


def stage_classifier_clips(frames_u8, plans, img_dim, flip=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None,
                           device=None, tables=None, size=224):
    """Raw frames + the reference's draws -> the classifier's input: per clip `resample the plan's region -> keep the
    size x size window (RandomSizedCrop(size, consistent=True), box or fallback) -> Image.resize to img_dim (Scale) ->
    ColorJitter -> ToTensor -> RandomHorizontalFlip -> Normalize`, bit-identical to the reference's classes.
    frames_u8: (B, T, H, W, 3) or (T, H, W, 3) uint8, on the host (uploaded once, as bytes) or the device.
    plans: B plans of ClassifierTransform.draw, or their pack_cls_plan tensors stacked (B, 25).
    flip: draw_batch_flip(), the loop's one draw per batch; kind 7 is appended to every clip's program.
    Returns (B, 3, T, S, S) fp32 on the device: what `model(input_seq)` takes after the script's `tr()`.
    TWO launches (coclr_resize2_boxes to bytes, then coclr_augment_clips with one program per clip), or ONE
    (coclr_resize2_boxes writing fp32) when no clip has a program and `flip` is off -- validation, or a training batch
    whose jitter draws all said no.  COCLR_CLS_FUSED=0 chains two coclr_resize_boxes_u8 launches instead of
    coclr_resize2_boxes (box plans only).  A bad plan is refused here before anything is launched.
    `tables`: classifier_tables(plans, ..., flip=flip) computed ahead; `plans` and `flip` are then not read."""
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() not in (4, 5) or frames_u8.shape[-1] != 3:
        raise ValueError("coclr_amd: frames must be uint8 (B, T, H, W, 3) or (T, H, W, 3), got %s %s" %
                         (frames_u8.dtype, tuple(frames_u8.shape)))
    if frames_u8.dim() == 4:
        frames_u8 = frames_u8[None]
        if isinstance(plans, dict):
            plans = [plans]
    B, T, H, W = frames_u8.shape[:4]
    if B < 1 or T < 1 or H < 1 or W < 1:
        raise ValueError("coclr_amd: a sample is T frames, got %s" % (tuple(frames_u8.shape),))
    S, size = _cls_sides(img_dim, size, "stage_classifier_clips")
    if tables is None:
        tables = classifier_tables(plans, B, T, W, H, S, size, flip)
    desc, tab2, kinds = tables[0], tables[3], tables[4]
    if tuple(desc.shape) != (B, 14) or tuple(kinds.shape[:1]) != (B,) or tab2.shape[1] != (S + 3) & ~3:
        raise ValueError("coclr_amd: tables for %d clips to %d, frames for %d to %d" %
                         (desc.shape[0], tab2.shape[1], B, S))
    return _stage_classifier(False, frames_u8, device, tables, B, T, S, size, mean, std, out)


# ---- batches whose videos differ in frame size (kinetics400-256: a 256-pixel short side, the video's own aspect) -------

RAGGED_ALIGN = 16        # every frame starts on a multiple of this in RaggedFrames.pixels


class RaggedFrames:
    """Frames of differing sizes in ONE flat uint8 device buffer, in batch order: what jpeg.decode_ragged returns and
    the *_ragged staging functions take.
      pixels  flat uint8 on the device
      offset  int64 (F,), host: frame i is pixels[offset[i] : offset[i] + 3 * H[i] * W[i]] viewed as (H, W, 3);
              64-bit (a batch may exceed 2 GiB), increasing, and a multiple of 16 so that the kernels' 16-byte
              accesses keep their aligned forms
      height, width  int32 (F,), host"""

    def __init__(self, pixels, offset, height, width):
        if not torch.is_tensor(pixels) or pixels.dtype != torch.uint8 or pixels.dim() != 1 or not pixels.is_contiguous():
            raise ValueError("coclr_amd: RaggedFrames.pixels is a flat contiguous uint8 tensor")
        offset = torch.as_tensor(offset, dtype=torch.int64).cpu().contiguous()
        height = torch.as_tensor(height, dtype=torch.int32).cpu().contiguous()
        width = torch.as_tensor(width, dtype=torch.int32).cpu().contiguous()
        F = offset.numel()
        if F < 1 or offset.dim() != 1 or tuple(height.shape) != (F,) or tuple(width.shape) != (F,):
            raise ValueError("coclr_amd: RaggedFrames takes offset, height and width of one length F >= 1")
        if bool((height < 1).any()) or bool((width < 1).any()):
            raise ValueError("coclr_amd: RaggedFrames holds frames of at least 1 x 1")
        end = offset + 3 * height.to(torch.int64) * width.to(torch.int64)
        if int(offset[0]) < 0 or bool((offset % RAGGED_ALIGN != 0).any()) or bool((offset[1:] < end[:-1]).any()) or \
                int(end[-1]) > pixels.numel():
            raise ValueError("coclr_amd: RaggedFrames offsets are multiples of %d, increasing, and the frames neither "
                             "overlap nor leave the %d bytes of pixels" % (RAGGED_ALIGN, pixels.numel()))
        self.pixels, self.offset, self.height, self.width = pixels, offset, height, width

    def __len__(self):
        return self.offset.numel()

    def frame(self, i):
        """Frame i as a (H, W, 3) view of `pixels`."""
        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError("coclr_amd: frame %d of %d" % (i, len(self)))
        o, H, W = int(self.offset[i]), int(self.height[i]), int(self.width[i])
        return self.pixels[o:o + 3 * H * W].view(H, W, 3)


def ragged_from_frames(frames, device=None):
    """uint8 tensors (n_i, H_i, W_i, 3) (or (H_i, W_i, 3)), on the host or the device, in batch order -> RaggedFrames
    with ONE upload: for callers who decode elsewhere."""
    frames = list(frames)
    if not frames:
        raise ValueError("coclr_amd: ragged_from_frames needs at least one tensor")
    offset, height, width, parts, at = [], [], [], [], 0
    for t in frames:
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() not in (3, 4) or t.shape[-1] != 3 or t.numel() == 0:
            raise ValueError("coclr_amd: ragged_from_frames takes uint8 (n, H, W, 3) tensors")
        t = t[None] if t.dim() == 3 else t
        n, H, W = t.shape[:3]
        for k in range(n):
            pad = -at % RAGGED_ALIGN
            if pad:
                parts.append(torch.zeros(pad, dtype=torch.uint8, device=t.device))
                at += pad
            offset.append(at)
            height.append(H)
            width.append(W)
            parts.append(t[k].contiguous().view(-1))
            at += 3 * H * W
    if device is None:
        on = [t.device for t in frames if t.is_cuda]
        device = on[0] if on else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if all(p.device == device for p in parts):
        pixels = torch.cat(parts)
    else:
        pixels = torch.cat([p.cpu() for p in parts]).to(device)
    return RaggedFrames(pixels, offset, height, width)


def _ragged_samples(frames, B, n, first):
    """Per sample its first frame, checked: frames first[b] .. first[b] + n - 1 exist, share one size and follow each
    other at 3 H W bytes rounded up to 16, which is how the kernels step through a clip and how decode_ragged and
    ragged_from_frames lay frames out.  Returns [(byte offset, W, H)] per sample."""
    if not isinstance(frames, RaggedFrames):
        raise ValueError("coclr_amd: the ragged staging takes a RaggedFrames (jpeg.decode_ragged, ragged_from_frames)")
    F = len(frames)
    first = [b * n for b in range(B)] if first is None else [int(v) for v in torch.as_tensor(first).reshape(-1).tolist()]
    if len(first) != B:
        raise ValueError("coclr_amd: %d first frames for %d samples" % (len(first), B))
    off, Hs, Ws = frames.offset.tolist(), frames.height.tolist(), frames.width.tolist()
    out = []
    for b, f0 in enumerate(first):
        if f0 < 0 or f0 + n > F:
            raise ValueError("coclr_amd: sample %d reads frames %d..%d of %d" % (b, f0, f0 + n - 1, F))
        H, W = Hs[f0], Ws[f0]
        if any(Hs[f] != H or Ws[f] != W for f in range(f0, f0 + n)):
            raise ValueError("coclr_amd: the frames of sample %d differ in size; one sample is one video" % b)
        stride = (3 * H * W + RAGGED_ALIGN - 1) & ~(RAGGED_ALIGN - 1)
        if any(off[f0 + k] != off[f0] + k * stride for k in range(n)):
            raise ValueError("coclr_amd: the frames of sample %d do not follow each other at %d bytes" % (b, stride))
        out.append((off[f0], W, H))
    return out


def _rag_words(offset, W, H):
    """The four trailing words of a ragged descriptor: the 64-bit byte offset as two int32 (low first), W, H."""
    lo = offset & 0xffffffff
    return [lo - (1 << 32) if lo >= 1 << 31 else lo, offset >> 32, W, H]


def _slot_major(per_sample, slots):
    """Per sample its clips, in check_train_plans' order for one plan -> the clips of the batch in the order of the
    result: sample by sample, or (two streams) slot by slot."""
    return [clip for group in (per_sample if slots is None else zip(*per_sample)) for clip in group]


def train_tables_ragged(plans, samples, T, S, slots=None):
    """train_tables for samples of differing frame sizes: `samples` [(byte offset of the sample's first frame, W, H)];
    every plan is checked against its own sample's (W, H).  Returns (desc int32 (2B, 14), xtab, ytab, kinds, params,
    group_size) as coclr_resize_boxes_ragged_u8 and coclr_augment_clips take them, all on the host.
    `slots`: as check_train_plans takes it; a sample's offset is then FOUR, one per quarter of its 4 T frames (None: not
    decoded, refused when a slot reads it), and desc is (len(slots) B, 14), slot-major."""
    plans = _plan_list(plans, unpack_plan, 2)
    if len(plans) != len(samples):
        raise ValueError("coclr_amd: %d plans for %d samples" % (len(plans), len(samples)))
    per_sample = []
    for b, (plan, (offset, W, H)) in enumerate(zip(plans, samples)):
        r, p = check_train_plans([plan], 1, T, W, H, slots)
        stride = (3 * H * W + RAGGED_ALIGN - 1) & ~(RAGGED_ALIGN - 1)
        clips = []
        for row, progs in zip(r, p):                             # row[0]: the clip's first frame within its sample
            at = offset + row[0] * stride if slots is None else offset[row[0] // T]
            if at is None:
                raise ValueError("coclr_amd: a staged clip of sample %d reads quarter %d of its frames, which is marked "
                                 "as not decoded" % (b, row[0] // T))
            clips.append(((0,) + row[1:], _rag_words(at, W, H), progs))
        per_sample.append(clips)
    rows, rag, programs = zip(*_slot_major(per_sample, slots))
    return _train_tables(rows, programs, rag, T, S)


def _train_head(who, slots, plans, out_size):
    """The head of the ragged and the cropped forms, where T comes from the plans: (plans as a list, B, T, S)."""
    plans = _plan_list([plans] if isinstance(plans, dict) else plans, unpack_plan, 2)
    B, S = len(plans), int(out_size)
    if B < 1:
        raise ValueError("coclr_amd: %s needs at least one plan" % who)
    n = len(plans[0]["programs"][0])
    if n < 1 or (slots is not None and n % 2 != 0):
        raise ValueError("coclr_amd: a plan has one program per frame%s, got %d" %
                         ("" if slots is None else " of both streams, 2 T (TrainTransform(img_dim, 2 * T))", n))
    if S < 1 or S * S > JITTER_MAX_PIXELS:
        raise ValueError("coclr_amd: %s takes an output size of 1..224, got %d" % (who, S))
    return plans, B, n if slots is None else n // 2, S


def _ragged_quarters(frames, B, T, first):
    """_ragged_samples for two-stream samples, whose four quarters of T frames need not follow each other: `first`
    (B, 4), the first frame of each quarter (default 4 T b + T q), -1 where a quarter was not decoded.  Each quarter is
    checked as _ragged_samples checks a sample, and the quarters of a sample must share one size.  Returns per sample
    ((byte offset per quarter, None for a missing one), W, H)."""
    if first is None:
        first = [[4 * T * b + T * q for q in range(4)] for b in range(B)]
    else:
        first = torch.as_tensor(first)
        if first.is_floating_point() or first.is_complex() or first.dtype == torch.bool or tuple(first.shape) != (B, 4):
            raise ValueError("coclr_amd: first must be integers of shape (%d, 4), the first frame of each quarter, got %s "
                             "%s" % (B, first.dtype, tuple(first.shape)))
        first = first.tolist()
    there = [(b, q) for b in range(B) for q in range(4) if first[b][q] != -1]
    got = dict(zip(there, _ragged_samples(frames, len(there), T, [first[b][q] for b, q in there]))) if there else {}
    out = []
    for b in range(B):
        sizes = {got[b, q][1:] for q in range(4) if (b, q) in got}
        if len(sizes) != 1:
            raise ValueError("coclr_amd: the quarters of sample %d hold frames of %d sizes; the RGB and the flow frames "
                             "of one sample share one size" % (b, len(sizes)))
        (W, H), = sizes
        out.append(([got[b, q][0] if (b, q) in got else None for q in range(4)], W, H))
    return out


def _train_clips_ragged(who, slots, frames, plans, out_size, first, mean, std, out):
    """The body of stage_train_clips_ragged (slots None) and stage_two_stream_clips_ragged."""
    plans, B, T, S = _train_head(who, slots, plans, out_size)
    samples = _ragged_samples(frames, B, 2 * T, first) if slots is None else _ragged_quarters(frames, B, T, first)
    tables = train_tables_ragged(plans, samples, T, S, slots)
    return _stage_train(ops.resize_boxes_ragged_u8, frames.pixels, frames.pixels.device, tables, _result_lead(slots, B),
                        T, S, mean, std, out)


def stage_train_clips_ragged(frames, plans, out_size, first=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None):
    """stage_train_clips for a batch whose samples differ in frame size, still TWO launches
    (coclr_resize_boxes_ragged_u8, then coclr_augment_clips on the S x S bytes, unchanged).
    frames: RaggedFrames.  Sample b is frames first[b] .. first[b] + 2T - 1 (default first[b] = 2 T b), which share
    one size; T comes from the plans.  plans: B plans of TrainTransform.draw(W_b, H_b), or their pack_plan tensors
    stacked.  Returns (B, 2, 3, T, S, S) fp32 on the device, each sample bit-identical to stage_train_clips on it."""
    return _train_clips_ragged("stage_train_clips_ragged", None, frames, plans, out_size, first, mean, std, out)


def classifier_tables_ragged(plans, samples, T, img_dim, size=224, flip=False):
    """classifier_tables for samples of differing frame sizes: `samples` [(byte offset, W, H)]; every plan is checked
    against its own sample's (W, H).  Returns (desc int32 (B, 18), xtab, ytab, tab2, kinds, params, direct)."""
    B, T = len(samples), int(T)
    S, size = _cls_sides(img_dim, size, "the classifier staging")
    plans = _plan_list(plans, unpack_cls_plan, 1)
    if len(plans) != B:
        raise ValueError("coclr_amd: %d plans for %d samples" % (len(plans), B))
    rows, programs = [], []
    for plan, (_, W, H) in zip(plans, samples):
        r, p = check_cls_plans([plan], 1, W, H, size)
        rows.extend(r)
        programs.extend(p)
    return _classifier_tables(rows, programs, [0] * B, [_rag_words(*sample) for sample in samples], T, S, size, flip)


def stage_classifier_clips_ragged(frames, plans, img_dim, flip=False, first=None, T=None, mean=IMAGENET_MEAN,
                                  std=IMAGENET_STD, out=None, size=224):
    """stage_classifier_clips for a batch whose samples differ in frame size: ONE launch fused
    (coclr_resize2_boxes_ragged) plus coclr_augment_clips when a clip has a program or `flip` is on, or two chained
    coclr_resize_boxes_ragged_u8 / coclr_resize_boxes_u8 launches with COCLR_CLS_FUSED=0 (box plans only).
    frames: RaggedFrames.  Sample b is frames first[b] .. first[b] + T - 1 (default first[b] = T b, T = frames / B),
    which share one size.  plans: B plans of ClassifierTransform.draw(W_b, H_b), or their packed tensors stacked.
    Returns (B, 3, T, S, S) fp32 on the device, each sample bit-identical to stage_classifier_clips on it."""
    plans = _plan_list([plans] if isinstance(plans, dict) else plans, unpack_cls_plan, 1)
    B, S, size = len(plans), int(img_dim), int(size)
    if B < 1:
        raise ValueError("coclr_amd: stage_classifier_clips_ragged needs at least one plan")
    if T is None:
        if not isinstance(frames, RaggedFrames) or first is not None or len(frames) % B != 0:
            raise ValueError("coclr_amd: give T, the frames per sample, when `first` is given or frames / B is not whole")
        T = len(frames) // B
    T = int(T)
    if T < 1:
        raise ValueError("coclr_amd: a sample is T >= 1 frames")
    samples = _ragged_samples(frames, B, T, first)
    tables = classifier_tables_ragged(plans, samples, T, S, size, flip)
    return _stage_classifier(True, frames.pixels, frames.pixels.device, tables, B, T, S, size, mean, std, out)


# ---- training clips whose frames were decoded as their crop boxes alone (jpeg.Store.decode(ids, boxes)) ---------------

def clip_frames(ids, plans, T):
    """What a batch's clips read, for jpeg.Store.decode(sel, boxes): ids (B, 2T) store ids, sample b's 2 T frames;
    plans: B plans of TrainTransform.draw, or their pack_plan tensors stacked.  Returns (sel int64 (2 B T,), boxes
    int64 (2 B T, 4)): for clip c of sample b the T ids of half[c] of the sample's frames, each with box[c] -- the
    layout stage_train_clips_cropped takes.  A half that no clip reads (OneClipTransform) is not selected, so it is
    not decoded; a half both clips read is selected twice, once per box."""
    ids, clips = _selection_args(ids, plans, T)
    T = int(T)
    sel, boxes = [], []
    for b, pair in enumerate(clips):
        for half, box in pair:
            sel.append(ids[b, half * T:(half + 1) * T])
            boxes.extend([box] * T)
    return torch.cat(sel), torch.tensor(boxes, dtype=torch.int64)


def _check_ids(ids, T):
    """`ids` as int64 (B, 2T) on the host, refused when it is not that."""
    T = int(T)
    ids = torch.as_tensor(ids)
    if ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool or ids.dim() != 2 or T < 1 or \
            ids.shape[1] != 2 * T or ids.shape[0] < 1:
        raise ValueError("coclr_amd: ids must be integers of shape (B, 2 T), got %s %s for T = %d" %
                         (ids.dtype, tuple(ids.shape), T))
    return ids.to("cpu", torch.int64)


def _selection_args(ids, plans, T):
    """The checks of clip_frames and two_stream_frames: (ids int64 (B, 2T) on the host, per plan its two clips'
    (half, box as a list of ints))."""
    ids = _check_ids(ids, T)
    plans = _plan_list([plans] if isinstance(plans, dict) else plans, unpack_plan, 2)
    if len(plans) != ids.shape[0]:
        raise ValueError("coclr_amd: %d plans for %d samples" % (len(plans), ids.shape[0]))
    clips = []
    for plan in plans:
        if len(plan["half"]) != 2 or len(plan["box"]) != 2:
            raise ValueError("coclr_amd: a plan names two clips")
        clips.append([])
        for c in range(2):
            half, box = plan["half"][c], plan["box"][c]
            if half not in (0, 1) or isinstance(half, bool):
                raise ValueError("coclr_amd: a clip reads half 0 or 1 of the frames, got %r" % (half,))
            if len(box) != 4 or any(int(v) != v for v in box):
                raise ValueError("coclr_amd: a box is four integers, got %r" % (box,))
            clips[-1].append((int(half), [int(v) for v in box]))
    return ids, clips


def train_tables_cropped(plans, clips, T, S, slots=None):
    """train_tables_ragged for clips whose frames ARE their boxes: `clips` [(byte offset of the clip's first frame, w,
    h)], two per plan; clip c of a plan must have its box[c]'s size.  The descriptors read the whole of every frame,
    (0, T, 0, 0, w, h), so the axis tables, the programs and the group size are train_tables_ragged's for the same
    plans.  Returns (desc int32 (2B, 14), xtab, ytab, kinds, params, group_size), all on the host.
    `slots`: as check_train_plans takes it; `clips` are then len(slots) per plan, slot-major, as two_stream_frames
    selects them, and so is desc."""
    plans = _plan_list(plans, unpack_plan, 2)
    B, per = len(plans), 2 if slots is None else len(slots)
    if per * B != len(clips):
        raise ValueError("coclr_amd: %d plans for %d clips" % (B, len(clips)))
    per_sample = []
    for b, plan in enumerate(plans):
        W = max(int(box[0] + box[2]) for box in plan["box"])              # the frame is gone: each box against itself
        H = max(int(box[1] + box[3]) for box in plan["box"])
        r, p = check_train_plans([plan], 1, T, W, H, slots)
        staged = []
        for c, (row, progs) in enumerate(zip(r, p)):
            offset, w, h = clips[2 * b + c if slots is None else c * B + b]
            if (w, h) != (row[4], row[5]):
                raise ValueError("coclr_amd: clip %d of sample %d holds %d x %d frames and its box is %d x %d" %
                                 (c, b, w, h, row[4], row[5]))
            staged.append(((0, T, 0, 0, w, h), _rag_words(offset, w, h), progs))
        per_sample.append(staged)
    rows, rag, programs = zip(*_slot_major(per_sample, slots))
    return _train_tables(rows, programs, rag, T, S)


def stage_train_clips_cropped(frames, plans, out_size, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None):
    """stage_train_clips_ragged for frames decoded as their crop boxes alone, the same TWO launches
    (coclr_resize_boxes_ragged_u8 reading every frame whole, then coclr_augment_clips):
        frames = store.decode(*clip_frames(ids, plans, T))
    frames: RaggedFrames of 2 B T frames; clip (b, c) is frames (2 b + c) T .. + T - 1, all of the size of box[c] of
    plan b, following each other at 3 w h bytes rounded up to 16 (checked here, on the host).  plans: the B plans
    clip_frames was given.  Returns (B, 2, 3, T, S, S) fp32 on the device, bit for bit stage_train_clips_ragged's
    result on the whole frames."""
    return _train_clips_cropped("stage_train_clips_cropped", None, frames, plans, out_size, mean, std, out)


def _train_clips_cropped(who, slots, frames, plans, out_size, mean, std, out):
    """The body of stage_train_clips_cropped (slots None) and stage_two_stream_clips_cropped."""
    plans, B, T, S = _train_head(who, slots, plans, out_size)
    n_clips = math.prod(_result_lead(slots, B))
    if isinstance(frames, RaggedFrames) and len(frames) != n_clips * T:
        raise ValueError("coclr_amd: %d frames for %d clips of %d" % (len(frames), n_clips, T))
    clips = _ragged_samples(frames, n_clips, T, None)                        # a clip's frames: one size, one stride
    tables = train_tables_cropped(plans, [(o, W, H) for o, W, H in clips], T, S, slots)
    return _stage_train(ops.resize_boxes_ragged_u8, frames.pixels, frames.pixels.device, tables, _result_lead(slots, B),
                        T, S, mean, std, out)


# ---- CoCLR's two-stream batches: RGB + flow (main_coclr.py:365-376,447-473; dataset/lmdb_dataset.py:498-509) ---------
#
# A sample is 4 T frames in the dataset's order, four QUARTERS: rgb(clip 1), flow(clip 1), rgb(clip 2), flow(clip 2).
# The reference transforms them with the chain of main_nce.py at seq_len = 2 T, so the plans are
# TrainTransform(img_dim, 2 * T).draw(W, H) and pack_plan(plan, 2 * T) unchanged: a plan clip has 2 T programs, program
# j < T for RGB frame j and program j >= T for flow frame j - T (one box, one jitter draw, one blur sigma and one flip
# for both streams; a gray clip's channel is drawn per frame across all 2 T), and half[c] selects quarters 2 half[c]
# (RGB) and 2 half[c] + 1 (flow).  Nothing new runs on the GPU: every (output tensor, sample) pair is ONE clip of T
# frames for the kernels stage_train_clips launches -- a first frame, a box and T programs -- and the result lands
# where the model reads it.

_TWO_STREAM_SLOTS = ((None, ((0, 0), (0, 1), (1, 0), (1, 1))),         # x1, f1, x2, f2
                     (False, ((0, 0), (1, 0), (1, 1))),                # x1, x2, f2: what CoCLR.forward reads
                     (True, ((1, 0), (1, 1), (0, 1))))                 # x2, f2, f1: what it reads with reverse=True


def two_stream_slots(reverse):
    """The tensors a two-stream batch is staged into, in the order they lie in TwoStreamClips.out, as (clip, stream)
    pairs, stream 0 RGB and 1 flow.  `reverse`: None for all four, or CoCLR's `reverse` (a bool) for the three its
    forward reads."""
    for key, slots in _TWO_STREAM_SLOTS:
        if reverse is key:
            return slots
    raise ValueError("coclr_amd: reverse is None (stage all four clips), False or True (the three clips CoCLR reads "
                     "with that `reverse`), got %r" % (reverse,))


class TwoStreamClips:
    """A staged two-stream batch.
      x1, f1, x2, f2  fp32 (B, 3, T, S, S), each contiguous: RGB and flow of clip 1 and of clip 2; None where the clip
                      was not staged
      out             the ONE allocation behind them:
                        reverse=None   (2, 2, B, 3, T, S, S), [clip][stream]
                        reverse=False  (3, B, 3, T, S, S), [x1, x2, f2]
                        reverse=True   (3, B, 3, T, S, S), [x2, f2, f1]
      blocks()        (block1, block2), (B, 2, 3, T, S, S) views of `out` for `model(block1, block2, vname)`: block[:, 0]
                      and block[:, 1], which is all CoCLR.forward takes of a block, ARE the staged tensors -- no copy.
    ALIASING in the three-clip forms: two neighbouring slots of `out` make a block, so the stream of block1 that
    CoCLR.forward never reads is not staged but aliases a tensor of block2 -- block1[:, 1] is x2 (not f1) with
    reverse=False, block1[:, 0] is f2 (not x1) with reverse=True.  Such blocks are right for a CoCLR of that `reverse`
    and wrong for any other reader of block1, which is why reverse=None, all four clips, is the default."""

    def __init__(self, out, reverse=None):
        slots = two_stream_slots(reverse)
        if out.dim() != (7 if reverse is None else 6) or tuple(out.shape[:-4]) != _result_lead(slots, out.shape[-5]) or \
                out.shape[-4] != 3 or not out.is_contiguous():
            raise ValueError("coclr_amd: a two-stream result with reverse=%r is contiguous %s, got %s" %
                             (reverse, "(2, 2, B, 3, T, S, S)" if reverse is None else "(3, B, 3, T, S, S)",
                              tuple(out.shape)))
        self.out, self.reverse = out, reverse
        self.x1 = self.f1 = self.x2 = self.f2 = None
        flat = out.view((len(slots),) + tuple(out.shape[-5:]))
        for k, (c, s) in enumerate(slots):
            setattr(self, "xf"[s] + "12"[c], flat[k])

    def blocks(self):
        if self.reverse is None:
            return self.out[0].transpose(0, 1), self.out[1].transpose(0, 1)
        first, second = self.out[0:2].transpose(0, 1), self.out[1:3].transpose(0, 1)
        return (second, first) if self.reverse else (first, second)


def stage_two_stream_clips(frames_u8, plans, out_size, reverse=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None,
                           device=None):
    """stage_train_clips for CoCLR's two-stream samples, the same TWO launches, bit-identical to the reference's
    transform of main_coclr.py on the 4 T frames.
    frames_u8: (B, 4T, H, W, 3) or (4T, H, W, 3) uint8 in the dataset's order -- rgb(clip 1), flow(clip 1), rgb(clip 2),
    flow(clip 2) -- on the host (uploaded once, as bytes) or the device.
    plans: B plans of TrainTransform(img_dim, 2 * T).draw, or their pack_plan(plan, 2 * T) tensors stacked.
    reverse: None stages all four clips; False / True stage only the three that CoCLR(reverse=...).forward reads
    (TwoStreamClips, which see for the aliasing this implies).  out: TwoStreamClips.out to fill.
    Returns a TwoStreamClips; `model(*clips.blocks(), vname)`.  Refusals come before anything is launched."""
    slots = two_stream_slots(reverse)
    return TwoStreamClips(_train_clips("stage_two_stream_clips", slots, frames_u8, plans, out_size, mean, std, out,
                                       device), reverse)


def stage_two_stream_clips_ragged(frames, plans, out_size, first=None, reverse=None, mean=IMAGENET_MEAN,
                                  std=IMAGENET_STD, out=None):
    """stage_two_stream_clips for a batch whose samples differ in frame size (stage_train_clips_ragged's launches).
    frames: RaggedFrames.  first: integer (B, 4), the first frame of each quarter of each sample (default
    4 T b + T q: every sample's 4 T frames in the dataset's order, one sample after the other); -1 marks a quarter that
    was not decoded, refused if a staged clip reads it (two_stream_frames(boxes=False) makes `first` for a selection
    without the quarters nothing reads).  A quarter's T frames share one size and follow each other at 3 H W bytes
    rounded up to 16; the quarters of one sample share one size -- RGB and flow frames of different sizes are refused
    (two_stream_frames).  T comes from the plans.  Returns a TwoStreamClips, each sample bit-identical to
    stage_two_stream_clips on it."""
    slots = two_stream_slots(reverse)
    return TwoStreamClips(_train_clips_ragged("stage_two_stream_clips_ragged", slots, frames, plans, out_size, first,
                                              mean, std, out), reverse)


def stage_two_stream_clips_cropped(frames, plans, out_size, reverse=None, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                                   out=None):
    """stage_two_stream_clips_ragged for frames decoded as their crop boxes alone (stage_train_clips_cropped's launches):
        frames = store.decode(*two_stream_frames(ids_rgb, ids_flow, plans, T, reverse))
    frames: RaggedFrames of len(two_stream_slots(reverse)) B T frames in two_stream_frames' order -- slot, then sample,
    then T frames, all of the size of the clip's box.  plans, reverse: what two_stream_frames was given.  Returns a
    TwoStreamClips, bit for bit stage_two_stream_clips_ragged's on the whole frames."""
    slots = two_stream_slots(reverse)
    return TwoStreamClips(_train_clips_cropped("stage_two_stream_clips_cropped", slots, frames, plans, out_size, mean,
                                               std, out), reverse)


def two_stream_frames(ids_rgb, ids_flow, plans, T, reverse=None, boxes=True, frame_size=None):
    """What a two-stream batch's staged clips read from ONE jpeg.Store or ShardedStore that holds the RGB and the flow
    videos under different ids: the two-stream clip_frames.
    ids_rgb, ids_flow: integer (B, 2T), the store ids of sample b's two clips of T frames (the SAME frame indices
    of the RGB and of the flow video: dataset/lmdb_dataset.py:498-500).  plans, reverse: as the staging takes them.
      boxes=True   -> (sel int64 (n B T,), boxes int64 (n B T, 4)) for store.decode(sel, boxes) and
                      stage_two_stream_clips_cropped, n = len(two_stream_slots(reverse)): slot by slot, sample by sample,
                      the T ids of the quarter the clip reads, each with the clip's box.
      boxes=False  -> (sel int64, first int64 (B, 4)) for a full-frame store.decode(sel) and
                      stage_two_stream_clips_ragged(first=first): sample by sample the quarters some staged clip reads,
                      each once; first[b, q] is quarter q's place in `sel`, or -1.
    A quarter no staged clip reads is absent from `sel` either way: the clip CoCLR.forward does not read (reverse False
    or True) and the half OneClipTransform abandons.
    The RGB and the flow frames of a sample must have ONE size.  The reference would crop a flow frame with the box
    drawn for the RGB frame's size and let PIL pad with black what the box leaves; UCF101, HMDB51 and kinetics400-256
    never do this (flow is computed on the RGB frames), so it is refused with ValueError instead: here when
    `frame_size` is given (store.frame_size: the first RGB and the first flow frame of every sample are compared; a
    video's frames share one size), and in any case by stage_two_stream_clips_ragged, which sees every frame.  The
    cropped route without `frame_size` refuses only a box that leaves the flow frame (store.decode)."""
    slots = two_stream_slots(reverse)
    T = int(T)
    rgb, clips = _selection_args(ids_rgb, plans, T)
    flow = _check_ids(ids_flow, T)
    if flow.shape != rgb.shape:
        raise ValueError("coclr_amd: ids_rgb is %s and ids_flow %s" % (tuple(rgb.shape), tuple(flow.shape)))
    ids, B = (rgb, flow), rgb.shape[0]
    if frame_size is not None:
        for b in range(B):
            a, f = tuple(frame_size(int(rgb[b, 0]))), tuple(frame_size(int(flow[b, 0])))
            if a != f:
                raise ValueError("coclr_amd: sample %d has RGB frames of %d x %d and flow frames of %d x %d; the two "
                                 "streams of a sample share one size" % ((b,) + a + f))
    if boxes:
        sel, rows = [], []
        for c, s in slots:
            for b in range(B):
                half, box = clips[b][c]
                sel.append(ids[s][b, half * T:(half + 1) * T])
                rows.extend([box] * T)
        return torch.cat(sel), torch.tensor(rows, dtype=torch.int64)
    sel, first = [], torch.full((B, 4), -1, dtype=torch.int64)
    for b in range(B):
        for q in sorted({2 * clips[b][c][0] + s for c, s in slots}):
            first[b, q] = T * len(sel)
            sel.append(ids[q % 2][b, (q // 2) * T:(q // 2 + 1) * T])
    return torch.cat(sel), first


# ---- test clips of many videos in one launch (eval/main_classifier.py:425-521,548-684) ---------------------------------

CROPS_MAX_SLOTS = 65535                 # (clip, t) slots per coclr_stage_crops_ragged launch: the grid's y limit


def crops_tables_ragged(frames, clips, crop_size):
    """The host tables of coclr_stage_crops_ragged.  frames: a RaggedFrames, or anything with its three host tables
    `offset`, `height`, `width` (the pixels are not touched).  clips: [(frame ids (T,) into `frames`, (x0, y0), flip)],
    one per output clip, in output order; the box is the crop_size box at (x0, y0) of the FLIPPED frame, as stage_crops
    takes it.  Every clip is checked against its OWN frames, which must share one size.  Returns (desc int32 (n, 5) =
    {x0, y0, flip, W, H}, slot_off int64 (n, T): the byte offset of every slot's frame)."""
    cw, ch = _crop_wh(crop_size)
    clips = list(clips)
    if not clips:
        raise ValueError("coclr_amd: crops_tables_ragged needs at least one clip")
    off = np.asarray(torch.as_tensor(frames.offset).cpu(), dtype=np.int64)
    Hs = np.asarray(torch.as_tensor(frames.height).cpu(), dtype=np.int64)
    Ws = np.asarray(torch.as_tensor(frames.width).cpu(), dtype=np.int64)
    F = off.shape[0]
    rows = []
    for ids, _, _ in clips:
        ids = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids)
        if ids.ndim != 1 or ids.size == 0 or ids.dtype.kind not in "iu":
            raise ValueError("coclr_amd: a clip's frame ids must be integers of shape (T,), got %s %s" %
                             (ids.dtype, ids.shape))
        rows.append(ids.astype(np.int64))
    T = rows[0].size
    if any(r.size != T for r in rows):
        raise ValueError("coclr_amd: the clips of one call share one length T")
    ids = np.stack(rows)
    lo, hi = int(ids.min()), int(ids.max())
    if lo < 0 or hi >= F:
        raise IndexError("coclr_amd: frame ids span %d..%d but there are %d frames" % (lo, hi, F))
    W, H = Ws[ids], Hs[ids]
    mixed = np.nonzero((W != W[:, :1]).any(1) | (H != H[:, :1]).any(1))[0]
    if mixed.size:
        raise ValueError("coclr_amd: the frames of clip %d differ in size; one clip is one video" % int(mixed[0]))
    desc = np.zeros((len(clips), 5), dtype=np.int32)
    for k, (_, box, flip) in enumerate(clips):
        (x0, y0, fl), = check_crops([box], [flip], cw, ch, int(W[k, 0]), int(H[k, 0]))
        desc[k] = (x0, y0, fl, W[k, 0], H[k, 0])
    return torch.from_numpy(desc), torch.from_numpy(np.ascontiguousarray(off[ids]))


def stage_crops_ragged(frames, clips, crop_size, out_size, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None, jitter=None):
    """stage_crops for the clips of MANY videos, of differing frame sizes, in ONE launch (coclr_stage_crops_ragged):
    frames: RaggedFrames (jpeg.Store.decode, jpeg.decode_ragged, ragged_from_frames).  clips: [(frame ids (T,) into
    `frames`, (x0, y0), flip)], one per output clip: flip the frame -> crop the crop_size box at (x0, y0) of the FLIPPED
    frame -> Image.resize((S, S), BICUBIC) -> ColorJitter -> ToTensor -> Normalize.  The frames of a clip share one size;
    ids may repeat (a strided or left-padded test clip) and clips may share frames.  Returns (n, 3, T, S, S) fp32 on the
    device, every clip bit-identical to stage_crops on its video alone.  `out`: any contiguous 16-byte-aligned fp32
    destination of that shape, e.g. free rows of a model's input batch.  `jitter`: one program per clip
    (ColorJitter.draw); the call is then two launches, resize to bytes and coclr_color_jitter_clips.  More than 65535
    slots are cut into launches."""
    if not isinstance(frames, RaggedFrames):
        raise ValueError("coclr_amd: the ragged staging takes a RaggedFrames (jpeg.Store.decode, ragged_from_frames)")
    cw, ch = _crop_wh(crop_size)
    S = int(out_size)
    desc, slot_off = crops_tables_ragged(frames, clips, (cw, ch))
    n, T = slot_off.shape
    device = frames.pixels.device
    _check_out(out, (n, 3, T, S, S), fp32=True)
    if out is not None and (out.device != device or out.data_ptr() % 16):
        raise ValueError("coclr_amd: out must be 16-byte aligned and on the frames' device %s" % device)
    if jitter is not None:
        jitter = list(jitter)
        if len(jitter) != n:
            raise ValueError("coclr_amd: need one jitter program per clip, got %d programs and %d clips" %
                             (len(jitter), n))
        if S * S > JITTER_MAX_PIXELS:
            raise ValueError("coclr_amd: color_jitter takes frames of up to 224 x 224 pixels, got %d x %d" % (S, S))
        program_tables(jitter)                            # refuse a bad program before anything is launched
    if out is None:
        out = torch.empty(n, 3, T, S, S, dtype=torch.float32, device=device)
    return launch_crops_ragged(frames.pixels, desc, slot_off, desc.to(device), slot_off.to(device), cw, ch, S, mean, std,
                               out, jitter)


def launch_crops_ragged(pixels, desc, slot_off, desc_dev, off_dev, cw, ch, S, mean, std, out, jitter=None):
    """The launches alone: the tables of crops_tables_ragged on the host and on the device, already checked, for any
    run of their rows; `out` (n, 3, T, S, S) fp32 on the device; `jitter` one checked program per clip."""
    n, T = slot_off.shape
    if T > CROPS_MAX_SLOTS:
        raise ValueError("coclr_amd: a clip of %d frames exceeds the %d slots of a launch" % (T, CROPS_MAX_SLOTS))
    device = pixels.device
    xmin, xk, ymin, yk = _device_tables(cw, ch, S, device)
    per = CROPS_MAX_SLOTS // T
    u8 = None if jitter is None else torch.empty(min(n, per) * T, S, S, 3, dtype=torch.uint8, device=device)
    for k in range(0, n, per):
        e = min(k + per, n)
        if jitter is None:
            ops.stage_crops_ragged(pixels, desc_dev[k:e], desc[k:e], off_dev[k:e], slot_off[k:e], cw, ch, S, xmin, xk,
                                   ymin, yk, out[k:e], mean, std)
        else:
            ops.stage_crops_ragged(pixels, desc_dev[k:e], desc[k:e], off_dev[k:e], slot_off[k:e], cw, ch, S, xmin, xk,
                                   ymin, yk, u8[:(e - k) * T])
            color_jitter(u8[:(e - k) * T], jitter[k:e], T, T, mean, std, out=out[k:e], device=device)
    return out
