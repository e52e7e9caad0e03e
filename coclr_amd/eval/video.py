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
`add()` takes staged clips, `add_frames` one video's decoded frames, `add_videos` / `add_stored` many videos of any
mix of frame sizes from a staging.RaggedFrames / a jpeg.Store, staged straight into the batch once per model pass.
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

    def add_videos(self, frames, videos, crops="ten", crop_size=224, out_size=128, jitter=None, rng=random):
        """MANY videos, of differing frame sizes, from their decoded frames in one staging.RaggedFrames (jpeg.Store.decode,
        jpeg.decode_ragged, staging.ragged_from_frames): `videos` [(first, count, frame_index, label)] -- the video's
        frame 0 is frame `first` of `frames`, it has `count` frames there, all of one size, and `frame_index`
        (n_clips, T) names the frame of every clip position RELATIVE to the video (staging.test_frame_index, or one row
        of a train-mode sampler).  The clips go video by video, crop by crop in the order of `crops`, clip by clip,
        STRAIGHT into the free rows of the batch: one coclr_stage_crops_ragged launch (two with `jitter`) per stretch
        of rows up to the next model pass, whatever number of videos it holds.  Segments, weights and results are those
        of add_frames called per video; `jitter` is drawn from `rng` once per crop, video by video, in staging order,
        before anything is staged.  Returns the videos' indices."""
        if not isinstance(frames, staging.RaggedFrames):
            raise ValueError("coclr_amd: add_videos takes a staging.RaggedFrames; add_frames takes one video's tensor")
        if frames.pixels.device != self.device:
            raise ValueError("coclr_amd: the frames are on %s, the evaluator on %s" % (frames.pixels.device, self.device))
        crop_size, S = int(crop_size), int(out_size)
        Hs, Ws = frames.height.tolist(), frames.width.tolist()

        def size_of(first, count, idx):
            if first + count > len(frames):
                raise IndexError("coclr_amd: a video of frames %d..%d, but there are %d frames" %
                                 (first, first + count - 1, len(frames)))
            H, W = Hs[first], Ws[first]
            if any(Hs[f] != H or Ws[f] != W for f in range(first, first + count)):
                raise ValueError("coclr_amd: the frames %d..%d of one video differ in size" % (first, first + count - 1))
            return W, H

        # first everything that can be refused, for every video; only then the draws and the evaluator's state
        checked, T = self._check_videos(videos, size_of, crops, crop_size, S, jitter)
        clips, programs, runs = [], [], []                # runs: (label, [clips of every crop])
        for first, idx, todo, label in checked:
            drawn = None if jitter is None else [jitter.draw(rng, 1)[0] for _ in todo]
            for k, (x0, y0, fl) in enumerate(todo):
                clips.extend((row, (x0, y0), fl) for row in idx + first)
                if drawn is not None:
                    programs.extend([drawn[k]] * idx.shape[0])
            runs.append((label, [idx.shape[0]] * len(todo)))
        desc, slot_off = staging.crops_tables_ragged(frames, clips, crop_size)
        if jitter is not None:
            staging.program_tables(programs)              # refuse a bad program before anything is launched
        desc_dev, off_dev = desc.to(self.device), slot_off.to(self.device)
        if self._buf is None:
            self._buf = torch.zeros(self.batch_clips, 3, T, S, S, dtype=torch.float32, device=self.device)
        # the crops still to be registered, as add() registers them: (video, clips of the crop, clips still to go)
        out, pending = [], collections.deque()
        for label, per_crop in runs:
            out.append(len(self._crops))
            self._labels.append(label)
            self._crops.append(len(per_crop))
            pending.extend([out[-1], n, n] for n in per_crop)
        at, total = 0, desc.shape[0]
        while at < total:
            k = min(total - at, self.batch_clips - self._fill)
            staging.launch_crops_ragged(frames.pixels, desc[at:at + k], slot_off[at:at + k], desc_dev[at:at + k],
                                        off_dev[at:at + k], crop_size, crop_size, S, staging.IMAGENET_MEAN,
                                        staging.IMAGENET_STD, self._buf[self._fill:self._fill + k],
                                        None if jitter is None else programs[at:at + k])
            left = k
            while left:
                crop = pending[0]
                m = min(left, crop[2])
                self._segs.append((self._fill, m, crop[0]))
                self._weights.append(1.0 / crop[1])
                self._fill += m
                left -= m
                crop[2] -= m
                if not crop[2]:
                    pending.popleft()
            at += k
            if self._fill == self.batch_clips:
                self._flush()
        return out

    def add_stored(self, store, videos, crops="ten", crop_size=224, out_size=128, jitter=None, rng=random,
                   max_stage_bytes=256 << 20):
        """add_videos from a jpeg.Store: `videos` [(first, count, frame_index, label)] with `first` the STORE id of the
        video's frame 0.  As many videos share one `store.decode` call as `max_stage_bytes` of decoded pixels allows
        (one at least), and only the distinct frames their `frame_index` rows name are decoded: a video with one clip
        of T frames decodes T frames, not the whole video.  Returns the videos' indices."""
        max_stage_bytes, crop_size, S = int(max_stage_bytes), int(crop_size), int(out_size)

        def size_of(first, count, idx):
            if first + count > len(store):
                raise IndexError("coclr_amd: a video of frames %d..%d, but the store holds %d" %
                                 (first, first + count - 1, len(store)))
            hw = store._geo[torch.from_numpy(idx).reshape(-1) + first, :2]      # H, W of the frames the clips read
            if bool((hw != hw[0]).any()):
                raise ValueError("coclr_amd: the frames %d..%d of one video differ in size" % (first, first + count - 1))
            return int(hw[0, 1]), int(hw[0, 0])

        # every video is checked before the first decode: a refused call leaves the evaluator and `rng` as they were
        checked, _ = self._check_videos(videos, size_of, crops, crop_size, S, jitter)
        out, group, ids, held, nbytes = [], [], [], 0, 0

        def run():
            frames = store.decode(torch.cat(ids))
            out.extend(self.add_videos(frames, group, crops, crop_size, S, jitter, rng))

        for first, idx, _, label in checked:
            distinct, local = torch.unique(torch.from_numpy(idx), return_inverse=True)      # sorted: the frames keep their order
            W, H = store.frame_size(first + int(distinct[0]))
            need = distinct.numel() * ((3 * W * H + staging.RAGGED_ALIGN - 1) & ~(staging.RAGGED_ALIGN - 1))
            if group and nbytes + need > max_stage_bytes:
                run()
                group, ids, held, nbytes = [], [], 0, 0
            group.append((held, distinct.numel(), local, label))
            ids.append(first + distinct)
            held += distinct.numel()
            nbytes += need
        run()
        return out

    def _check_videos(self, videos, size_of, crops, crop_size, S, jitter):
        """What add_videos and add_stored refuse, for ALL `videos` [(first, count, frame_index, label)] and before
        anything is drawn, decoded, staged or registered.  `size_of(first, count, idx)` -> (W, H) of the video's frames,
        refusing frames that do not exist or differ in size.  Returns ([(first, idx int64 (n_clips, T) relative to the
        video, crops [(x0, y0, flip)], label)], T)."""
        if crops not in CROP_MODES:
            raise ValueError("coclr_amd: crops must be one of %s, got %r" % (sorted(CROP_MODES), crops))
        videos = list(videos)
        if not videos:
            raise ValueError("coclr_amd: at least one video is needed")
        if jitter is not None and S * S > staging.JITTER_MAX_PIXELS:
            raise ValueError("coclr_amd: color_jitter takes frames of up to 224 x 224 pixels, got %d x %d" % (S, S))
        where, flip_list = CROP_MODES[crops]
        out, T = [], None
        for first, count, frame_index, label in videos:
            first, count = int(first), int(count)
            if count < 1 or first < 0:
                raise IndexError("coclr_amd: a video of %d frames from frame %d" % (count, first))
            idx = staging.check_frame_index(frame_index, count).numpy().astype("int64")
            W, H = size_of(first, count, idx)
            boxes = staging.five_crop_boxes(W, H, crop_size, where)
            todo = staging.check_crops(boxes * len(flip_list), [f for f in flip_list for _ in boxes],
                                       crop_size, crop_size, W, H)
            T = idx.shape[1] if T is None else T
            want = (3, T, S, S) if self._buf is None else tuple(self._buf.shape[1:])
            if (3, idx.shape[1], S, S) != want:
                raise ValueError("coclr_amd: clip size %s differs from the evaluator's %s" % ((3, idx.shape[1], S, S), want))
            if T > staging.CROPS_MAX_SLOTS:
                raise ValueError("coclr_amd: a clip of %d frames exceeds the %d slots of a launch" %
                                 (T, staging.CROPS_MAX_SLOTS))
            out.append((first, idx, todo, None if label is None else int(label)))
        return out, T

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
