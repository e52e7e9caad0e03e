"""Writes tests/golden/fwd_f23_randn.pt: the raw fp32 outputs and statistics of the temporal Winograd F(2,3)
kernels (variant 50 of coclr_conv3d_fwd_plan) on seeded randn data, for tests/test_gpu_fwd_f23_golden.py.

    COCLR_LIB_PATH=<libcoclr_hip.so of the commit to pin> python tools/make_fwd_f23_golden.py [--out FILE]

Run it on the MI355X with the library of the commit whose arithmetic is to be held still (docs/history.md names the
commit the committed fixture was recorded from).  The launches are those of tests/_fwd_f23_golden.py, which the test
replays; two recordings in one process must agree bit for bit before anything is written."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _fwd_f23_golden as G      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", G.FIXTURE))
    args = ap.parse_args()
    from coclr_amd import _lib
    rec, again = G.replay(), G.replay()
    assert rec.keys() == again.keys()
    for k in rec:
        assert torch.equal(rec[k].view(torch.int32), again[k].view(torch.int32)), "%s: two runs differ" % k
        assert bool(rec[k].isfinite().all()), k
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    torch.save({"torch": str(torch.__version__), "rows": list(G.ROWS), "pair": list(G.PAIR), "tensors": rec}, args.out)
    size = os.path.getsize(args.out)
    print("wrote %s (%d bytes, %d tensors) with %s" % (args.out, size, len(rec), _lib.LIB_PATH))
    assert size <= 1 << 20


if __name__ == "__main__":
    main()
