"""What the CPU and the GPU tier of the two-stream staging share (coclr_amd/staging.py: stage_two_stream_clips and its
ragged and cropped forms, two_stream_frames, TwoStreamClips): the fixture of the reference's own two-stream transform
(tests/golden/two_stream_transform.pt, tools/make_two_stream_golden.py), its plans, the expected tensors through the
fixture's byte table, a restatement of the decomposition on tests/train_harness.py's chain for samples the fixture
does not hold, and a list of frames addressed by id that stands in for a JPEG store where none is needed.  Nothing here
shares code with coclr_amd/staging.py."""
import os
import random

import numpy as np
import torch

import jitter_harness as JH
import train_harness as TH

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "two_stream_transform.pt")
NAMES = ("x1", "f1", "x2", "f2")                                    # the fixture's order, and (clip, stream) row-major
SLOTS = {None: ("x1", "f1", "x2", "f2"), False: ("x1", "x2", "f2"), True: ("x2", "f2", "f1")}       # the issue's orders
COVERS = {"two clips", "one clip", "one clip, half 0", "one clip, half 1", "base on clip 0", "null on clip 0",
          "base on clip 1", "null on clip 1", "jitter applied", "jitter skipped", "gray",
          "gray, rgb and flow channels differ", "blur r = 0", "blur r = 1", "flip", "box does not fit"}


def golden():
    return torch.load(GOLDEN)


def fixture_plans(gold):
    """Per recorded run (run, plan, (random.random(), np.random.random()) right after the draw): the plan
    staging.TrainTransform(img_dim, 2 * T).draw yields with both generators seeded as the run was."""
    from coclr_amd import staging
    tt = staging.TrainTransform(gold["img_dim"], 2 * gold["seq_len"])
    out = []
    for run in gold["runs"]:
        random.seed(run["seed"])
        np.random.seed(run["seed"])
        H, W = run["frames"].shape[1:3]
        plan = tt.draw(W, H)
        out.append((run, plan, (random.random(), float(np.random.random()))))
    return out


def expected(run, gold):
    """The run's four clips as the model takes them: fp32 (4, 3, T, S, S), x1, f1, x2, f2, through the byte table."""
    T, S = gold["seq_len"], gold["img_dim"]
    assert tuple(run["clips"].shape) == (4, T, S, S, 3)
    return JH.levels_expected(run["clips"].reshape(4 * T, S, S, 3).numpy(), gold["levels"], T)


def chain_expected(frames, plan, T, S):
    """One sample the fixture does not hold: frames uint8 (4T, H, W, 3) in the dataset's order and a plan of
    TrainTransform(S, 2 T) -> fp32 (4, 3, T, S, S), x1, f1, x2, f2.  The reference's transform sees the 2 T frames
    [rgb, flow] of a clip as ONE clip of the single-stream chain, which tests/train_harness.py restates."""
    u8 = TH.chain_u8(frames, plan, S)                                # (4T, S, S, 3): clip 0's 2T frames, then clip 1's
    return JH.to_clips(u8, T)


def check(clips, want, reverse, b=slice(None)):
    """A TwoStreamClips against `want` (4, B, 3, T, S, S) in NAMES' order, for samples `b`: the staged tensors equal,
    the others None."""
    for k, name in enumerate(NAMES):
        got = getattr(clips, name)
        if name in SLOTS[reverse]:
            assert got is not None and torch.equal(got[b].cpu(), want[k][b]), (name, reverse)
        else:
            assert got is None, (name, reverse)


class Frames:
    """Frames addressed by id: `add` takes a sample's (4T, H, W, 3) in the dataset's order and returns (ids_rgb (2T,),
    ids_flow (2T,)) as a dataset would hand them out; `decode(sel, boxes)` returns the selected frames (or their boxes)
    as staging.ragged_from_frames lays them out -- what jpeg.Store.decode does with real files."""

    def __init__(self, device):
        self.frames, self.device = [], device

    def add(self, sample):
        T = sample.shape[0] // 4
        at = len(self.frames)
        self.frames.extend(sample)
        q = [list(range(at + k * T, at + (k + 1) * T)) for k in range(4)]
        return q[0] + q[2], q[1] + q[3]

    def frame_size(self, i):
        H, W = self.frames[i].shape[:2]
        return W, H

    def decode(self, sel, boxes=None):
        from coclr_amd import staging
        sel = sel.tolist()
        if boxes is None:
            cut = [self.frames[i] for i in sel]
        else:
            cut = [self.frames[i][y0:y0 + h, x0:x0 + w] for i, (x0, y0, w, h) in zip(sel, boxes.tolist())]
        return staging.ragged_from_frames(cut, device=self.device)


def mixed_batch(gold):
    """The fixture's runs (40 x 52) followed by seeded samples of 8 x 96, 57 x 41 and 24 x 192 (H x W; the sizes of
    tests/ragged_harness.py: the 57 x 41 frames are no multiple of 16 bytes) whose plans come from
    TrainTransform(S, 2 T).draw: [(frames uint8 (4T, H, W, 3), plan, want fp32 (4, 3, T, S, S))]."""
    from coclr_amd import staging
    import ragged_harness as RH
    S, T = gold["img_dim"], gold["seq_len"]
    batch = [(run["frames"], plan, expected(run, gold)) for run, plan, _ in fixture_plans(gold)]
    tt = staging.TrainTransform(S, 2 * T)
    for seed, (H, W) in ((31, (8, 96)), (32, RH.EDGE), (33, (24, 192))):
        plan = tt.draw(W, H, rng=random.Random(seed), np_rng=np.random.RandomState(seed))
        frames = torch.from_numpy(TH.frames(4 * T, H, W, seed))
        batch.append((frames, plan, chain_expected(frames, plan, T, S)))
    return batch
