"""TEST DOUBLES of the segmented-accumulate kernels (coclr_amd/csrc/retrieval.hip: coclr_segment_softmax_accum,
coclr_segment_accum) in ATen on the CPU, and a small stand-in model, so that the HOST logic of
coclr_amd/eval/video.py -- batching, segment bookkeeping, crop weights -- runs in the CPU tier.  Installed only
by tests, on top of tests/fake_backend.py; the product has no CPU path and never imports this file."""
import torch

import fake_backend
from coclr_amd import _lib, ops


def _check(x, segs, weight, out):
    R, V = x.shape[0], out.shape[0]
    segs = [tuple(int(v) for v in s) for s in segs]
    if not segs or len(weight) != len(segs):
        raise ValueError("segments and weights")
    for first, rows, o in segs:
        if first < 0 or rows < 1 or first + rows > R or not 0 <= o < V:
            raise _lib.HipLibraryError("segment (%d, %d, %d) out of range" % (first, rows, o))
    return segs


def segment_softmax_accum(logits, segs, weight, out):
    for (first, rows, o), w in zip(_check(logits, segs, weight, out), weight):
        out[o] += (float(w) * torch.softmax(logits[first:first + rows].double(), dim=-1).sum(0)).float()


def segment_accum(x, segs, weight, out):
    for (first, rows, o), w in zip(_check(x, segs, weight, out), weight):
        out[o] += (float(w) * x[first:first + rows].double().sum(0)).float()


def install(monkeypatch):
    fake_backend.install(monkeypatch)
    monkeypatch.setattr(ops, "segment_softmax_accum", segment_softmax_accum)
    monkeypatch.setattr(ops, "segment_accum", segment_accum)


class ToyClassifier(torch.nn.Module):
    """(B, 3, T, H, W) -> (logit (B, num_class), feature (B, C)) with LinearClassifier's call signature."""

    def __init__(self, num_class=11, width=16, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.proj = torch.nn.Parameter(torch.randn(3 * 2, width, generator=g))
        self.fc = torch.nn.Parameter(torch.randn(width, num_class, generator=g) * 3)
        self.shapes = []

    def forward(self, block):
        self.shapes.append(tuple(block.shape))
        B = block.shape[0]
        half = block.shape[2] // 2
        pooled = torch.cat([block[:, :, :half].mean((2, 3, 4)), block[:, :, half:].mean((2, 3, 4))], 1)
        feat = torch.tanh(pooled.view(B, 6) @ self.proj)
        return feat @ self.fc, feat
