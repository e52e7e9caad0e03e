"""Linear probe on cached features, trained on MI355X (eval/feature_linear_probe.py).

The reference trains BatchNorm1d + Linear on the features `main_classifier.py --retrieval` cached, with SGD
(momentum 0.9, a stepwise schedule), evaluates every `eval_freq` epochs and writes the test probabilities as JSON
for merge_2stream_prob.py.  Here the features stay on the device for the whole run and an iteration is:
`ops.gather_rows` of the index batch, the probe's forward (`FeatureBatchNorm1d`, `FeatureLinear`: the head of
`LinearClassifier`), `coclr_amd.loss.cross_entropy` + `calc_topk_accuracy` (one launch yields both), the
backward and the single-launch `coclr_amd.optim.SGD` step.  Nothing is read back inside an epoch: the loss and
top-1 scalars of every iteration go into a device vector that is read once per epoch and folded in float64 with
AverageMeter's weights, the batch sizes.

Two behaviours of the script are kept, because its numbers depend on them:

  * Draws.  The index batches come from `torch.utils.data.DataLoader` over an index tensor -- `shuffle=True,
    drop_last=False` for training, `shuffle=False` for every validation pass -- so every `iter()` draws from the
    global generator what the reference's loaders draw, at the same points of the run (`draws`).  Under the same
    `torch.manual_seed`, with `LinearProbe` constructed as the reference constructs `LP`, the run sees the
    reference's batches and leaves the generator where the reference leaves it.

  * "Best model".  `best_model = model.state_dict()` (:143) holds VIEWS of the live tensors, not copies, so the
    `load_state_dict(best_model)` before the final pass (:148) changes nothing: the probabilities the script saves
    come from the LAST epoch's weights, while `best_acc` / `best_epoch` are the maximum (found with `>=`, so the
    latest of equal epochs).  `fit` reproduces that by default; `snapshot_best=True` keeps a real copy of the best
    epoch's state and saves its probabilities -- a documented deviation.

    python -m coclr_amd.eval.linear_probe --test CKPT --dataset ucf101 --dirname feature [--final_bn] ...
"""
import argparse
import collections
import copy
import os
import sys

import numpy as np
import torch
import torch.nn as nn
from torch.utils import data

from .. import loss as L
from .. import ops
from .. import optim as O
from ..model.classifier import FeatureBatchNorm1d, FeatureLinear
from . import fusion

LPResult = collections.namedtuple("LPResult", "best_acc best_epoch state_dict probs history")


class LinearProbe(nn.Module):
    """The reference's `LP` (:43-60) on the HIP head: same attribute names (`bn`, `fc`), so its state dict loads
    with strict=True, and the same construction -- nn.Linear's own initialisation first, then normal_(0, 0.01) and
    a zeroed bias -- so the global generator is left where the reference leaves it."""

    def __init__(self, dim, num_class=10, final_bn=False):
        super(LinearProbe, self).__init__()
        self.use_bn = final_bn
        if self.use_bn:
            self.bn = FeatureBatchNorm1d(dim)
            self.bn.weight.data.fill_(1)
            self.bn.bias.data.zero_()

        self.fc = FeatureLinear(dim, num_class, bias=True)
        self.fc.weight.data.normal_(mean=0.0, std=0.01)
        self.fc.bias.data.zero_()

    def forward(self, x):
        if self.use_bn:
            x = self.bn(x)
        return self.fc(x)


def draws(n_train, n_test, batch_size, epochs, eval_freq):
    """The index batches of a run, in order, drawn as the reference's two loaders draw them (:124-128, :134-149).
    Yields (phase, epoch, batches): phase 'train' for every epoch, 'val' after the epochs with
    `epoch % eval_freq == 0`, and one 'final' pass (epoch None) at the end; `batches` iterates over int64 host
    index tensors.  Each loader's `iter()` -- which is what consumes the global generator -- runs when its pass is
    asked for, so a consumer that finishes a pass before asking for the next one interleaves exactly as the
    script does.  Host-only."""
    train_loader = data.DataLoader(torch.arange(n_train), batch_size=batch_size, shuffle=True, drop_last=False,
                                   num_workers=0)
    test_loader = data.DataLoader(torch.arange(n_test), batch_size=batch_size, shuffle=False, drop_last=False,
                                  num_workers=0)
    for epoch in range(epochs):
        yield "train", epoch, iter(train_loader)
        if epoch % eval_freq == 0:
            yield "val", epoch, iter(test_loader)
    yield "final", None, iter(test_loader)


def learning_rate(lr, epoch, schedule):
    """adjust_learning_rate (:218-225): the stepwise schedule, multiplied up as the script multiplies it."""
    for milestone in schedule:
        lr *= 0.1 if epoch >= milestone else 1.
    return lr


def fold_meters(stats, sizes):
    """What the script's two AverageMeters hold after a pass.  stats: (n, 2) fp32 [loss, top-1 fraction] per
    iteration as the loss kernel leaves them; sizes: the batch sizes.  Folded in float64 as AverageMeter does
    (sum += val * n; avg = sum / count).  The reference's calc_topk_accuracy forms a fraction as
    fp32(hits) * fp32(1 / B) (utils/utils.py:67-68); the kernel's is hits / B rounded once, which names the same
    count, so the fraction is re-formed the reference's way and the averages are the script's to the last bit."""
    stats = np.asarray(stats, dtype=np.float32).reshape(-1, 2)
    loss_sum = acc_sum = 0.0
    count = 0
    for (loss, frac), n in zip(stats, sizes):
        hits = np.float32(round(float(frac) * n))
        loss_sum += float(loss) * n
        acc_sum += float(hits * np.float32(1 / n)) * n
        count += n
    return loss_sum / count, acc_sum / count


def _normalize(x):
    """F.normalize(x) (:105-108)."""
    x = x.contiguous()
    out = torch.empty_like(x)
    ops.l2norm_fwd(x, out, torch.empty(x.shape[0], dtype=torch.float32, device=x.device))
    return out


def fit(train_feature, train_label, test_feature, test_label, *, batch_size=1024, lr=1.0, wd=1e-3, epochs=100,
        eval_freq=5, schedule=(60, 80), normalize=False, final_bn=False, snapshot_best=False, log=None):
    """feature_linear_probe.py's main() (:105-149) from device tensors: fp32 (n, dim) features, int64 labels.
    Construct-and-train under the caller's `torch.manual_seed` (the script seeds 0).

    Returns LPResult(best_acc, best_epoch, state_dict, probs, history): `probs` is the fp32 (n_test, num_class)
    softmax of the final validation pass on the device, `history` one dict per epoch (lr, train_loss, train_acc and,
    where the epoch was evaluated, val_loss, val_acc) plus the final pass.

    By default -- as in the script, whose "best model" is a set of views of the live tensors -- `probs` and
    `state_dict` are those of the LAST epoch's weights, while best_acc / best_epoch are the maximum over the
    evaluated epochs (ties go to the later epoch).  snapshot_best=True deviates: the state of the best epoch is
    copied when it is found, loaded before the final pass, and returned.

    `log` (a callable taking one string) receives the lines the script prints."""
    if train_feature.dtype != torch.float32 or test_feature.dtype != torch.float32 or not train_feature.is_cuda:
        raise ValueError("coclr_amd: the linear probe trains on fp32 device features")
    say = log if log is not None else (lambda line: None)
    dev = train_feature.device
    train_label = train_label.to(device=dev, dtype=torch.long).contiguous()
    test_label = test_label.to(device=dev, dtype=torch.long).contiguous()
    if normalize:
        say('Using normalized feature')
        train_feature, test_feature = _normalize(train_feature), _normalize(test_feature)
    train_feature, test_feature = train_feature.contiguous(), test_feature.contiguous()
    dim = train_feature.size(-1)
    num_class = int(train_label.max().item()) + 1
    if num_class > ops.SEGMENT_MAX_C:
        raise ValueError("coclr_amd: the probe's softmax takes up to %d classes" % ops.SEGMENT_MAX_C)
    if final_bn:
        say('Use final BN layer in network')

    model = LinearProbe(dim, num_class, final_bn)
    model.cuda(dev)
    optimizer = O.SGD(model.parameters(), lr=lr, weight_decay=wd, momentum=0.9)
    n_train, n_test = train_feature.shape[0], test_feature.shape[0]
    per_epoch = -(-n_train // batch_size) + -(-n_test // batch_size)
    stats = torch.empty(per_epoch, 2, dtype=torch.float32, device=dev)      # [loss, top-1] of every iteration

    def run_pass(batches, feature, label, row, train, probs=None):
        """One loader pass; writes stats[row:], returns the batch sizes.  Nothing is read back."""
        model.train(train)
        sizes = []
        for idx in batches:
            B = idx.shape[0]
            idx_d = idx.to(dev, non_blocking=True)
            x = fusion.take_rows(feature, idx_d)
            y = fusion.take_rows(label, idx_d)
            with torch.set_grad_enabled(train):
                logit = model(x)
                loss = L.cross_entropy(logit, y)
                top1, = L.calc_topk_accuracy(logit, y, (1,))
            at = row + len(sizes)
            stats[at, 0].copy_(loss.detach())
            stats[at, 1].copy_(top1)
            if train:
                optimizer.zero_grad()
                loss.backward()
                optimizer.step()
            if probs is not None:
                # F.softmax(logit) (:199): one-row segments, row r of the batch into row idx[r] of `probs`
                first = int(idx[0])
                ops.segment_softmax_accum(logit.detach(), [(r, 1, first + r) for r in range(B)], [1.0] * B, probs)
            sizes.append(B)
        return sizes

    best_acc, best_epoch, best_state = 0.0, 0, None
    history = []
    pending = None          # the epoch whose statistics are still on the device
    probs = None

    def finish(entry):
        """Read the epoch's statistics (one copy) and do what the script does with them."""
        nonlocal best_acc, best_epoch, best_state
        host = stats[:len(entry["train_sizes"]) + len(entry.get("val_sizes", ()))].cpu().numpy()
        nt = len(entry["train_sizes"])
        epoch = entry["epoch"]
        entry["train_loss"], entry["train_acc"] = fold_meters(host[:nt], entry.pop("train_sizes"))
        say('train: Epoch[{}] loss {:.4f} acc {:.4f}'.format(epoch, entry["train_loss"], entry["train_acc"]))
        if "val_sizes" in entry:
            entry["val_loss"], entry["val_acc"] = fold_meters(host[nt:], entry.pop("val_sizes"))
            say('eval[{}] loss {:.4f} acc {:.4f}'.format(epoch, entry["val_loss"], entry["val_acc"]))
            if entry["val_acc"] >= best_acc:                                   # :139-144
                best_acc, best_epoch = entry["val_acc"], epoch
                if snapshot_best:
                    best_state = copy.deepcopy(model.state_dict())
                say('Best acc: %.4f' % entry["val_acc"])
        history.append(entry)

    for phase, epoch, batches in draws(n_train, n_test, batch_size, epochs, eval_freq):
        if phase == "train":
            if pending is not None:
                finish(pending)
            cur_lr = learning_rate(lr, epoch, schedule)
            for group in optimizer.param_groups:
                group['lr'] = cur_lr
            pending = {"epoch": epoch, "lr": cur_lr}
            pending["train_sizes"] = run_pass(batches, train_feature, train_label, 0, True)
        elif phase == "val":
            pending["val_sizes"] = run_pass(batches, test_feature, test_label, len(pending["train_sizes"]), False)
        else:
            if pending is not None:
                finish(pending)
            say('Final best acc: %.4f' % best_acc)
            say('Save probability ... ')
            if best_state is not None:
                model.load_state_dict(best_state)
            probs = torch.zeros(n_test, num_class, dtype=torch.float32, device=dev)
            sizes = run_pass(batches, test_feature, test_label, 0, False, probs)
            final_loss, final_acc = fold_meters(stats[:len(sizes)].cpu().numpy(), sizes)
            say('eval[{}] loss {:.4f} acc {:.4f}'.format(best_epoch, final_loss, final_acc))
            history.append({"epoch": best_epoch, "final": True, "val_loss": final_loss, "val_acc": final_acc})
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return LPResult(best_acc, best_epoch, state, probs, history)


# ---- command line ------------------------------------------------------------------------------------------------

def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--test', default='', type=str)
    parser.add_argument('--dataset', default='ucf101', type=str)
    parser.add_argument('--dirname', default='feature', type=str)

    parser.add_argument('--batch_size', default=1024, type=int)
    parser.add_argument('--lr', default=1.0, type=float)
    parser.add_argument('--wd', default=1e-3, type=float)
    parser.add_argument('--epochs', default=100, type=int)
    parser.add_argument('--eval_freq', default=5, type=int)
    parser.add_argument('--verbose', default=0, type=int)
    parser.add_argument('--schedule', default=[60, 80], nargs='*',
                        type=int, help='learning rate schedule (when to drop lr by 10x)')
    parser.add_argument('--normalize', action='store_true', help='normalize feature')
    parser.add_argument('--final_bn', action='store_true', help='final bn')
    parser.add_argument('--snapshot_best', action='store_true',
                        help='save the probabilities of the best epoch, not (as the reference does) of the last')
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    torch.manual_seed(0)
    directory = os.path.join(os.path.dirname(args.test), args.dirname)
    if not os.path.exists(os.path.join(directory, '%s_train_feature.pth.tar' % args.dataset)):
        print('feature path does not exist')
        sys.exit(0)
    f = fusion.load_features(directory, args.dataset)
    res = fit(f["train_feature"].float().cuda(), f["train_label"].cuda(), f["test_feature"].float().cuda(),
              f["test_label"].cuda(), batch_size=args.batch_size, lr=args.lr, wd=args.wd, epochs=args.epochs,
              eval_freq=args.eval_freq, schedule=tuple(args.schedule), normalize=args.normalize,
              final_bn=args.final_bn, snapshot_best=args.snapshot_best, log=print)
    path = os.path.join(directory, '%s-lp-%s-prob.json' % (os.path.basename(args.test), args.dataset))
    fusion.save_probs(path, f["test_vname"], res.probs, form="nested")
    print('prob saved to %s' % path)


if __name__ == '__main__':
    main()
