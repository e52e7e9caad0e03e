"""Times coclr_amd.eval.linear_probe.fit on features of UCF101's size against the loop a caller could write before it.

    python tools/time_linear_probe.py [--epochs 20] [--rounds 3] [--out profiles/linear_probe.json]

9537 training and 3783 test rows of width 1024 in 101 classes (split 1 with an S3D backbone), seeded, on the device;
batch 1024, eval_freq 5, the script's defaults otherwise.  Two legs, alternating, each between device events after a
warm-up run of the same shapes:

  fit       linear_probe.fit: index batches gathered by ops.gather_rows, the single-launch SGD, loss and top-1 kept on
            the device and read once per epoch
  baseline  the same index batches and the same head (FeatureBatchNorm1d off, FeatureLinear), the same
            coclr_amd.loss.cross_entropy / calc_topk_accuracy, but rows taken by ATen indexing, torch's own SGD, and the
            script's two `.item()` per iteration: what existed before this module, arranged as the script arranges it

The baseline does NOT iterate the script's per-sample Dataset (9537 `__getitem__` calls and a collate per epoch on the
host): that is the reference's loader, not something this project had a faster form of.  Both legs end with the same
validation pass; the final losses are printed so that a reader sees they computed the same thing."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from coclr_amd import loss as L                      # noqa: E402
from coclr_amd import optim as O                     # noqa: E402
from coclr_amd.eval import linear_probe as LP        # noqa: E402

NTR, NTE, DIM, NCLS, BATCH, EVAL_FREQ, SCHEDULE = 9537, 3783, 1024, 101, 1024, 5, (60, 80)


def features():
    g = torch.Generator().manual_seed(0)
    centres = torch.randn(NCLS, DIM, generator=g)
    trl = torch.randint(0, NCLS, (NTR,), generator=g)
    tel = torch.randint(0, NCLS, (NTE,), generator=g)
    trl[:NCLS] = torch.arange(NCLS)
    return ((centres[trl] + 4 * torch.randn(NTR, DIM, generator=g)).cuda(), trl.cuda(),
            (centres[tel] + 4 * torch.randn(NTE, DIM, generator=g)).cuda(), tel.cuda())


def baseline(trf, trl, tef, tel, epochs):
    model = LP.LinearProbe(DIM, NCLS, False).cuda()
    opt = O._TorchSGD(model.parameters(), lr=1.0, weight_decay=1e-3, momentum=0.9)
    out = {}
    for phase, epoch, batches in LP.draws(NTR, NTE, BATCH, epochs, EVAL_FREQ):
        train = phase == "train"
        if train:
            for group in opt.param_groups:
                group["lr"] = LP.learning_rate(1.0, epoch, SCHEDULE)
        feature, label = (trf, trl) if train else (tef, tel)
        model.train(train)
        loss_sum = acc_sum = 0.0
        count = 0
        for idx in batches:
            idx = idx.cuda(non_blocking=True)
            x, y = feature[idx], label[idx]
            with torch.set_grad_enabled(train):
                logit = model(x)
                loss = L.cross_entropy(logit, y)
                top1, = L.calc_topk_accuracy(logit, y, (1,))
            loss_sum += loss.item() * idx.shape[0]
            acc_sum += top1.item() * idx.shape[0]
            count += idx.shape[0]
            if train:
                opt.zero_grad()
                loss.backward()
                opt.step()
        out[phase] = (loss_sum / count, acc_sum / count)
    return out["final"]


def fit(trf, trl, tef, tel, epochs):
    res = LP.fit(trf, trl, tef, tel, batch_size=BATCH, epochs=epochs, eval_freq=EVAL_FREQ, schedule=SCHEDULE)
    return res.history[-1]["val_loss"], res.history[-1]["val_acc"]


def timed(fn, data, epochs):
    torch.manual_seed(0)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    result = fn(*data, epochs)
    end.record()
    end.synchronize()
    return start.elapsed_time(end), result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_linear_probe.py measures on the GPU; none found")
    data = features()
    legs = {"fit": fit, "baseline": baseline}
    for fn in legs.values():                       # every shape of the timed window, once
        timed(fn, data, 1)
    ms = {k: [] for k in legs}
    final = {}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            t, final[k] = timed(fn, data, args.epochs)
            ms[k].append(t)
    iters = args.epochs * -(-NTR // BATCH)
    rec = {"epochs": args.epochs, "train_iterations": iters, "ms": ms, "final": final,
           "median_ms": {k: sorted(v)[len(v) // 2] for k, v in ms.items()}}
    for k in legs:
        print("%-8s median %.1f ms for %d epochs (%.3f ms per training iteration, validation included), rounds %s, "
              "final loss %.6f acc %.4f" % (k, rec["median_ms"][k], args.epochs, rec["median_ms"][k] / iters,
                                            ["%.1f" % t for t in ms[k]], final[k][0], final[k][1]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            json.dump(rec, fp, indent=1)


if __name__ == "__main__":
    main()
