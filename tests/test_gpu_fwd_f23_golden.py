"""The temporal Winograd F(2,3) kernels (variant 50) on non-integer data, bit for bit.

tests/test_gpu_fwd_exact.py feeds small integers on purpose: exact whatever the order of summation.  So nothing
there sees a change in the ORDER of the epilogue's additions into the statistics, or in which multiply-adds the
compiler fuses -- and the project holds outputs, BatchNorm sums and backward sums to the bit.  This test replays
the launches of tests/_fwd_f23_golden.py on seeded randn data and compares the raw fp32 bits of every y and every
[2][Cout][ntiles] statistics tensor with tests/golden/fwd_f23_randn.pt (recorded by tools/make_fwd_f23_golden.py;
docs/history.md names the commit).

The rows are the w50_* rows of tests/_fwd_cases.py: odd frame counts 5 and 3 (a half-valid last pair), Cout 20 /
24 / 72 against the 64-row tile, Cin 16 / 20 / 24 against chunks of 16 (4-byte staging) and 8 (16-byte), 9
positions per frame for the 4-byte form, the data gradient, and the pair kernel."""
import functools
import os

import pytest
import torch

import _fwd_f23_golden as G

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", G.FIXTURE)
MODES = ["plain", "accum", "ep_relu", "ep_linear", "bwd0", "bwd1"]


@functools.lru_cache(maxsize=None)
def fixture():
    fix = torch.load(GOLDEN)
    assert fix["rows"] == list(G.ROWS) and fix["pair"] == list(G.PAIR)
    return fix["tensors"]


@functools.lru_cache(maxsize=None)
def replayed():
    try:
        return G.replay()
    except RuntimeError as e:
        # a launch that faulted ends the session: nothing more is started on a device in that state
        pytest.exit("GPU error in an F(2,3) launch: %s" % e, returncode=3)


def same_bits(key):
    got, want = replayed()[key], fixture()[key]
    assert got.shape == want.shape, (key, got.shape, want.shape)
    diff = got.view(torch.int32) != want.view(torch.int32)
    if bool(diff.any()):
        idx = tuple(diff.nonzero()[0].tolist())
        raise AssertionError("%s: %d of %d values differ in their bits; first at %s: got %r, recorded %r" % (
            key, int(diff.sum()), diff.numel(), idx, got[idx].item(), want[idx].item()))


def test_every_recorded_tensor_is_replayed():
    assert set(replayed()) == set(fixture())
    assert len(fixture()) == 2 * (len(G.ROWS) * len(MODES) + len(G.PAIR))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", G.ROWS)
def test_row(name, mode):
    same_bits("%s/%s/y" % (name, mode))
    same_bits("%s/%s/stats" % (name, mode))


@pytest.mark.parametrize("name", G.PAIR)
def test_pair(name):
    same_bits("pair/%s/y" % name)
    same_bits("pair/%s/stats" % name)
    # each problem of the pair keeps the plan it has alone
    for part in ("y", "stats"):
        a, b = replayed()["pair/%s/%s" % (name, part)], replayed()["%s/plain/%s" % (name, part)]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, part)
