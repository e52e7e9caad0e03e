"""Video-level evaluation on MI355X: the 5/10-crop test and the feature extraction of
eval/main_classifier.py:425-521,548-684.

The reference runs the model once per video (`batch_size=1`, a different number of clips every time: a new
input shape per video), then `F.softmax(logit).mean(0)` per crop (:488), `torch.stack(...).mean(0)` over the
crops plus the accuracy with two `.item()` reads per video (:533-537), and `feature.mean(0)` for retrieval
(:637,673).  Here the clips of all videos are packed into ONE static (batch_clips, 3, T, H, W) buffer: the
backbone sees a single shape (one inference launch plan, engine.PLAN_INFER, and full-width kernels whatever
the videos' lengths), and after every batch two segmented-accumulate kernels add each video's share of the
batch -- weight 1/n per crop of n clips -- to its row of the probability and feature tables
(ops.segment_softmax_accum / ops.segment_accum).  A video that spans two batches contributes two segments.
Nothing is read back and nothing synchronises before `finish()`, whose results are device tensors (clips handed
over as HOST tensors are copied before `add()` returns, so the caller may reuse its staging buffer).
"""
import collections
import random

import torch

from .. import loss as _loss
from .. import ops
from .. import staging

# the reference's aug_list / flip_list (eval/main_classifier.py:431-442), in its order: flips outermost
CROP_MODES = {"center": ((5,), (0,)), "five": ((5, 1, 2, 3, 4), (0,)), "ten": ((5, 1, 2, 3, 4), (0, 1))}

VideoScores = collections.namedtuple("VideoScores", "probs features labels top1 top5")


class VideoEvaluator:
    """`model(clips) -> (logit (B, num_class), feature (B, C))` in eval mode, e.g. LinearClassifier (bare or
    in DataParallel(device_ids=[0])).  `device` defaults to the device of the model's parameters."""

    def __init__(self, model, batch_clips=32, device=None):
        batch_clips = int(batch_clips)
        if batch_clips < 1:
            raise ValueError("coclr_amd: batch_clips must be >= 1")
        if device is None:
            device = next(model.parameters()).device
        self.model, self.batch_clips, self.device = model, batch_clips, torch.device(device)
        self.passes = 0              # model passes so far
        self._buf = None             # the static clip batch
        self._fill = 0               # rows of it in use
        self._segs, self._weights = [], []      # segments of the batch being filled
        self._labels, self._crops = [], []      # per video
        self._probs = self._feats = None        # (capacity, num_class) / (capacity, C) running sums

    def __len__(self):
        return len(self._crops)

    def add(self, clips, label=None, video=None):
        """One crop of a video: `clips` (n, 3, T, H, W), n >= 1 (any n: a crop longer than the batch is cut).
        `video=None` starts a new video and returns its index; `video=i` adds a further crop to video i."""
        if clips.dim() != 5 or clips.shape[0] < 1 or clips.dtype != torch.float32:
            raise ValueError("coclr_amd: clips must be fp32 (n, 3, T, H, W) with n >= 1, got %s %s" %
                             (clips.dtype, tuple(clips.shape)))
        if self._buf is not None and tuple(clips.shape[1:]) != tuple(self._buf.shape[1:]):
            raise ValueError("coclr_amd: clip size %s differs from the evaluator's %s" %
                             (tuple(clips.shape[1:]), tuple(self._buf.shape[1:])))
        if label is not None:
            label = int(label)
        if video is None:
            video = len(self._crops)
            self._labels.append(label)
            self._crops.append(0)
        else:
            video = int(video)
            if not 0 <= video < len(self._crops):
                raise IndexError("coclr_amd: no video %d (have %d)" % (video, len(self._crops)))
            if label is not None and self._labels[video] is not None and label != self._labels[video]:
                raise ValueError("coclr_amd: video %d has label %d, got %d" % (video, self._labels[video], label))
            if self._labels[video] is None:
                self._labels[video] = label
        if self._buf is None:
            self._buf = torch.zeros((self.batch_clips,) + tuple(clips.shape[1:]), dtype=torch.float32,
                                    device=self.device)
        self._crops[video] += 1
        n, done = clips.shape[0], 0
        while done < n:
            k = min(n - done, self.batch_clips - self._fill)
            # (a host source is copied before add() returns: the caller may reuse its staging buffer at once)
            self._buf[self._fill:self._fill + k].copy_(clips[done:done + k], non_blocking=clips.is_cuda)
            self._segs.append((self._fill, k, video))
            self._weights.append(1.0 / n)
            self._fill += k
            done += k
            if self._fill == self.batch_clips:
                self._flush()
        return video

    def add_frames(self, frames_u8, frame_index, label=None, crops="ten", crop_size=224, out_size=128,
                   max_stage_bytes=256 << 20, jitter=None, rng=random):
        """One video from its decoded frames: `frames_u8` (F, H, W, 3) uint8, host or device, uploaded ONCE;
        `frame_index` (n_clips, T) the frame of every clip position (staging.test_frame_index).  `crops`:
        "center", "five" or "ten" -- the reference's --center_crop / --five_crop / --ten_crop, centre first and
        the flipped five last.  Every crop is staged on the GPU (staging.stage_crops: flip, FiveCrop(crop_size),
        Scale(out_size) in PIL's bicubic, ColorJitter, ToTensor, Normalize) and handed to add() as a further crop
        of one video, whose index is returned.  Whole crops are staged in chunks of at most `max_stage_bytes`.
        `jitter`: a staging.ColorJitter, e.g. the reference's ColorJitter(0.2, 0.2, 0.2, 0.1, p=0.3); it is drawn
        from `rng` once per crop, in staging order, before anything is staged (the chunking does not show in the
        draws).  None leaves the jitter out."""
        if crops not in CROP_MODES:
            raise ValueError("coclr_amd: crops must be one of %s, got %r" % (sorted(CROP_MODES), crops))
        if frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or frames_u8.dtype != torch.uint8:
            raise ValueError("coclr_amd: frames must be uint8 (F, H, W, 3), got %s %s" %
                             (frames_u8.dtype, tuple(frames_u8.shape)))
        where, flip_list = CROP_MODES[crops]
        F, H, W = frames_u8.shape[:3]
        crop_size, S = int(crop_size), int(out_size)
        boxes = staging.five_crop_boxes(W, H, crop_size, where)
        todo = staging.check_crops(boxes * len(flip_list), [f for f in flip_list for _ in boxes],
                                   crop_size, crop_size, W, H)
        idx = staging.check_frame_index(frame_index, F)
        n, T = idx.shape
        per_crop = n * 3 * T * S * S * 4
        if per_crop > max_stage_bytes:
            raise ValueError("coclr_amd: one crop of this video is %d bytes, max_stage_bytes is %d" %
                             (per_crop, max_stage_bytes))
        if self._buf is not None and (3, T, S, S) != tuple(self._buf.shape[1:]):
            raise ValueError("coclr_amd: clip size %s differs from the evaluator's %s" %
                             ((3, T, S, S), tuple(self._buf.shape[1:])))
        frames = frames_u8.contiguous().to(self.device)
        idx = idx.to(self.device)
        chunk = min(len(todo), 16, max_stage_bytes // per_crop)
        buf = torch.empty(chunk, n, 3, T, S, S, dtype=torch.float32, device=self.device)
        programs = None if jitter is None else [jitter.draw(rng, 1)[0] for _ in todo]
        video = None
        for k in range(0, len(todo), chunk):
            part = todo[k:k + chunk]
            if programs is None:
                staged = staging.stage_crops_on_device(frames, idx, part, crop_size, crop_size, S,
                                                       out=buf[:len(part)])
            else:
                staged = staging.stage_crops_on_device(frames, idx, part, crop_size, crop_size, S,
                                                       out=buf[:len(part)], jitter=programs[k:k + chunk])
            for clips in staged:
                # (add() copies the crop into the batch on this stream before the next chunk overwrites `buf`)
                video = self.add(clips, label=label if video is None else None, video=video)
        return video

    def _flush(self):
        """Run the batch (rows past `_fill` are padding: they belong to no segment) and accumulate."""
        if getattr(self.model, "training", False):
            raise RuntimeError("coclr_amd: VideoEvaluator needs the model in eval() mode")
        with torch.no_grad():
            logit, feat = self.model(self._buf)
        self.passes += 1
        logit, feat = logit.contiguous(), feat.contiguous()
        need = len(self._crops)
        if self._probs is None or self._probs.shape[0] < need:
            cap = max(64, 2 * need)
            probs = torch.zeros(cap, logit.shape[1], dtype=torch.float32, device=self.device)
            feats = torch.zeros(cap, feat.shape[1], dtype=torch.float32, device=self.device)
            if self._probs is not None:
                probs[:self._probs.shape[0]].copy_(self._probs)
                feats[:self._feats.shape[0]].copy_(self._feats)
            self._probs, self._feats = probs, feats
        ops.segment_softmax_accum(logit, self._segs, self._weights, self._probs)
        ops.segment_accum(feat, self._segs, self._weights, self._feats)
        self._segs, self._weights, self._fill = [], [], 0

    def finish(self):
        """Run the tail batch and return VideoScores(probs (V, num_class), features (V, C), labels (V,) int64
        or None, top1, top5): the means over each video's crops of the per-crop mean softmax / mean feature,
        and the top-k accuracies of `probs` as device scalars (None without labels).  The evaluator is empty
        afterwards."""
        V = len(self._crops)
        if V == 0:
            raise ValueError("coclr_amd: no video was added")
        if self._fill:
            self._flush()
        gain = torch.tensor([[1.0 / c for c in self._crops]], dtype=torch.float32).to(self.device)
        outs = []
        for table in (self._probs, self._feats):
            src = table[:V]
            out = torch.empty_like(src)
            ops.plane_scale(src.view(1, V, src.shape[1], 1, 1), gain, None, out.view(1, V, src.shape[1], 1, 1))
            outs.append(out)
        probs, feats = outs
        labels = top1 = top5 = None
        if all(l is not None for l in self._labels):
            labels = torch.tensor(self._labels, dtype=torch.long).to(self.device)
            top1, top5 = _loss.calc_topk_accuracy(probs, labels, (1, 5))
        self._labels, self._crops = [], []
        self._probs = self._feats = None
        return VideoScores(probs, feats, labels, top1, top5)


def extract_features(model, videos, batch_clips=32, device=None):
    """Per-video mean features for retrieval (eval/main_classifier.py:624-640,660-676): `videos` yields
    `clips` or `(clips, label)`; returns (features (V, C), labels or None), ready for
    coclr_amd.eval.retrieval.nn_retrieval."""
    ev = VideoEvaluator(model, batch_clips=batch_clips, device=device)
    for item in videos:
        clips, label = item if isinstance(item, (tuple, list)) else (item, None)
        ev.add(clips, label)
    res = ev.finish()
    return res.features, res.labels
