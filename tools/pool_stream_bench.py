"""The pooling launches of one bench.py step (S3D InfoNCE, B = 32, 3x32x128x128) on their own, for a rocprofv3
kernel trace or a counter pass:

    rocprofv3 --kernel-trace -f csv -d DIR -o trace -- python tools/pool_stream_bench.py --reps 5 --plan DIR/plan.json
    python tools/pool_stream_table.py DIR/plan.json <kernel_trace.csv | counter_collection.csv> ...

Every launch of a pooling kernel that this script makes is appended to the plan file in launch order (label, kernels
per call, algorithmic bytes = x or dy, the indices where they exist, and the output, each once), so the table script
can tell the dispatches of one geometry from the next without guessing from the kernel's name.  The backward of a
layer uses the arg-max indices its forward just wrote.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coclr_amd import _lib, ops  # noqa: E402

K333, K133, K222 = (3, 3, 3), (1, 3, 3), (2, 2, 2)
S1, S122, S222 = (1, 1, 1), (1, 2, 2), (2, 2, 2)
P1, P011, P0 = (1, 1, 1), (0, 1, 1), (0, 0, 0)

# (name, C, input extent, window, stride, padding, lazy BatchNorm + ReLU on read, pooled BatchNorm backward)
LAYERS = [
    ("MaxPool_2a", 64, (16, 64, 64), K133, S122, P011, True, True),
    ("MaxPool_3a", 192, (16, 32, 32), K133, S122, P011, True, True),
    ("Mixed_3b.pool", 192, (16, 16, 16), K333, S1, P1, False, False),
    ("Mixed_3c.pool", 256, (16, 16, 16), K333, S1, P1, False, False),
    ("MaxPool_4a", 480, (16, 16, 16), K333, S222, P1, False, False),
    ("Mixed_4b.pool", 480, (8, 8, 8), K333, S1, P1, False, False),
    ("Mixed_4c.pool", 512, (8, 8, 8), K333, S1, P1, False, False),
    ("Mixed_4d.pool", 512, (8, 8, 8), K333, S1, P1, False, False),
    ("Mixed_4e.pool", 512, (8, 8, 8), K333, S1, P1, False, False),
    ("Mixed_4f.pool", 528, (8, 8, 8), K333, S1, P1, False, False),
    ("MaxPool_5a", 832, (8, 8, 8), K222, S222, P0, False, False),
    ("Mixed_5b.pool", 832, (4, 4, 4), K333, S1, P1, False, False),
    ("Mixed_5c.pool", 832, (4, 4, 4), K333, S1, P1, False, False),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plan", required=True, help="JSON file that receives the launch order")
    ap.add_argument("--only", default=None, help="comma-separated layer names")
    args = ap.parse_args()
    _lib.load()
    dev = torch.device("cuda")
    N = args.batch
    plan = []

    def launch(label, kernels, nbytes, fn, reps):
        for _ in range(reps):
            fn()
        plan.append(dict(label=label, kernels=kernels, reps=reps, bytes=int(nbytes)))

    gen = torch.Generator(device=dev).manual_seed(7)
    only = set(args.only.split(",")) if args.only else None
    for name, Cc, idim, k, s, p, lazy, pooled in LAYERS:
        if only and name not in only:
            continue
        g = ops.PoolGeom(N, Cc, idim, k, s, p)
        x = torch.randn((N, Cc) + tuple(idim), device=dev, generator=gen)
        y = torch.empty((N, Cc) + tuple(g.odim), device=dev)
        idx = torch.empty((N, Cc) + tuple(g.odim), device=dev, dtype=torch.int32)
        aff = {}
        if lazy:
            scale = torch.rand(Cc, device=dev, generator=gen) + 0.5
            shift = torch.randn(Cc, device=dev, generator=gen) * 0.2
            aff = dict(in_scale=scale, in_shift=shift, in_relu=True)
        nx, ny = x.numel() * 4, y.numel() * 4
        launch(name + " fwd idx", 1, nx + 2 * ny, lambda: ops.maxpool_fwd(g, x, y, idx, **aff), args.reps)
        launch(name + " fwd noidx", 1, nx + ny, lambda: ops.maxpool_fwd(g, x, y, None, **aff), args.reps)
        dy = torch.randn(y.shape, device=dev, generator=gen)
        dx = torch.zeros_like(x)
        if pooled:
            mean = torch.randn(Cc, device=dev, generator=gen) * 0.3
            invstd = torch.rand(Cc, device=dev, generator=gen) + 0.5
            sums = torch.zeros(ops.bn_backward_workspace(N, Cc), device=dev, dtype=torch.float64)
            dgb = torch.zeros(2, Cc, device=dev)
            # reduce: dy, indices and the gathered y; apply: dy, indices, y in, dy_bn out
            launch(name + " pooled bn bwd (reduce, apply)", 2, 2 * ny + nx + 2 * ny + 2 * nx,
                   lambda: ops.bn_act_backward_pooled(g, dy, idx, x, scale, shift, mean, invstd, sums, dx, dgb[0],
                                                      dgb[1], True, True), args.reps)
        else:
            launch(name + " bwd", 1, 2 * ny + nx, lambda: ops.maxpool_bwd(g, dy, idx, dx, accumulate=False),
                   args.reps)
        torch.cuda.synchronize()
        del x, y, idx, dy, dx
    torch.cuda.synchronize()
    json.dump(plan, open(args.plan, "w"), indent=1)
    print("pool_stream_bench: %d launch groups" % len(plan))


if __name__ == "__main__":
    main()
