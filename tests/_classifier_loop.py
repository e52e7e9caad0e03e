"""The call sequence of the reference's eval/main_classifier.py, restated (test infrastructure).

`run_classifier` makes, in the same order, the calls `main()` + `train_one_epoch` + `validate` of
eval/main_classifier.py:80-305,308-422 make on the model, the optimiser, DataParallel, the criterion,
the accuracy helper and the meters' `.item()` reads: the `train_what` switch (:102-146), the
optimiser (:155-160), `adjust_learning_rate` (:721-726), `model.eval()` + `final_bn.train()` for the
linear probe (:319-324), the `tr()` closure with RandomHorizontalFlip + Normalize (:257-261,328-331),
a validation pass per epoch.  The data loaders are the script's (RandomSampler / shuffle, drop_last), drawn
from the global RNG at the same points.  The GPU box has no /root/reference, so the script itself cannot
be imported there; tests/test_dropin_classifier.py proves (in the build container, on the CPU double)
that this restatement and the unmodified script produce IDENTICAL logits, targets and losses.
The module is called directly or through DataParallel(device_ids=[0]): never replicated.
"""
import random

import numpy as np
import torch
import torch.nn as nn

NORM = ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])


def _tr(x, flip, num_seq, seq_len, img_dim):
    # transforms.Compose([T.RandomHorizontalFlip(), T.Normalize(mean, std, channel=1)]) (utils/transforms.py)
    if flip and random.random() < 0.5:
        x = x.flip(dims=(-1,))
    shape = [1] * x.dim()
    shape[1] = -1
    mean = torch.as_tensor(NORM[0]).to(x.device).reshape(shape)
    std = torch.as_tensor(NORM[1]).to(x.device).reshape(shape)
    x = (x - mean) / std
    B = x.size(0)
    return x.view(B, 3, num_seq, seq_len, img_dim, img_dim).transpose(1, 2).contiguous()


def load_pretrained(model_without_dp, path):
    """--pretrain (:222-237): encoder_q.0.* of a pretraining checkpoint becomes backbone.*; a strict
    load, else utils.neq_load_customized (update the model's own state dict and load it back)."""
    state_dict = torch.load(path, map_location='cpu', weights_only=False)['state_dict']
    state_dict = {k.replace('encoder_q.0.', 'backbone.'): v for k, v in state_dict.items()}
    try:
        model_without_dp.load_state_dict(state_dict)
    except RuntimeError:
        model_dict = model_without_dp.state_dict()
        model_dict.update({k: v for k, v in state_dict.items() if k in model_dict})
        model_without_dp.load_state_dict(model_dict)


def build_classifier(product, *, train_what, optim, net='s3d', num_class=101, lr=1e-3, wd=1e-3, dropout=0.9,
                     gpu=None, data_parallel=True):
    """main() up to the DataParallel wrap (:87-164): (model_without_dp, model, optimizer, criterion)."""
    device = torch.device('cuda') if gpu is not None else torch.device('cpu')
    final_bn = final_norm = train_what == 'last'
    use_dropout = train_what != 'last'
    model = product.LinearClassifier(network=net, num_class=num_class, dropout=dropout,
                                     use_dropout=use_dropout, use_final_bn=final_bn, use_l2_norm=final_norm)
    model.to(device)
    params = []
    if train_what == 'last':
        for name, param in model.named_parameters():
            if 'backbone' in name:
                param.requires_grad = False
            else:
                params.append({'params': param})
    elif train_what == 'ft':
        for name, param in model.named_parameters():
            if 'backbone' in name:
                params.append({'params': param, 'lr': lr / 10})
            else:
                params.append({'params': param})
    else:
        params = [{'params': param} for _, param in model.named_parameters()]
    if optim == 'adam':
        optimizer = torch.optim.Adam(params, lr=lr, weight_decay=wd)
    elif optim == 'sgd':
        optimizer = torch.optim.SGD(params, lr=lr, weight_decay=wd, momentum=0.9)
    else:
        raise NotImplementedError(optim)
    model_without_dp = model
    if data_parallel:
        model = torch.nn.DataParallel(model, device_ids=[0] if gpu is not None else None)
    return model_without_dp, model, optimizer, nn.CrossEntropyLoss()


def begin_epoch(model, model_without_dp, train_what):
    """train_one_epoch's mode switch (:319-324)."""
    if train_what == 'last':
        model.eval()
    else:
        model.train()
    if train_what == 'last':
        model_without_dp.final_bn.train()


def train_step(model, optimizer, criterion, input_seq, target, device, seq_len, img_dim, calc_topk_accuracy,
               rec=None):
    """One iteration of train_one_epoch (:333-351) on a loader batch."""
    input_seq = _tr(input_seq.to(device, non_blocking=True), True, 1, seq_len, img_dim)
    target = target.to(device, non_blocking=True)
    input_seq = input_seq.squeeze(1)
    logit, _ = model(input_seq)
    loss = criterion(logit, target)
    top1, top5 = calc_topk_accuracy(logit, target, (1, 5))
    if rec is not None:
        rec["outputs"].append(logit.detach().cpu().clone())
        rec["targets"].append(target.detach().cpu().clone())
    lv = loss.item()
    if rec is not None:
        rec["losses"].append(lv)
    top1.item(), top5.item()
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return lv


def run_classifier(product, train_set, val_set, *, train_what, optim, net='s3d', num_class=101,
                   batch_size=4, seq_len=8, img_dim=64, lr=1e-3, wd=1e-3, dropout=0.9, schedule=(60, 80),
                   pretrain=None, gpu=None, data_parallel=True, calc_topk_accuracy=None,
                   on_optimizer=None, validate=True, epochs=1):
    """main_classifier.py --train_what {ft,last} --optim {sgd,adam} --epochs `epochs`: per epoch the
    lr schedule, one training pass and one validation pass.
    `on_optimizer(optimizer, model)` (optional) is called once the optimiser exists."""
    device = torch.device('cuda') if gpu is not None else torch.device('cpu')
    torch.manual_seed(0)
    np.random.seed(0)
    random.seed(0)
    model_without_dp, call, optimizer, ce_loss = build_classifier(
        product, train_what=train_what, optim=optim, net=net, num_class=num_class, lr=lr, wd=wd,
        dropout=dropout, gpu=gpu, data_parallel=data_parallel)
    pin = gpu is not None
    train_loader = torch.utils.data.DataLoader(train_set, batch_size=batch_size, shuffle=False, num_workers=0,
                                               pin_memory=pin, sampler=torch.utils.data.RandomSampler(train_set),
                                               drop_last=True)
    val_loader = torch.utils.data.DataLoader(val_set, batch_size=batch_size, shuffle=True, num_workers=0,
                                             pin_memory=pin, sampler=None, drop_last=True)
    if pretrain is not None:
        load_pretrained(model_without_dp, pretrain)
    if on_optimizer is not None:
        on_optimizer(optimizer, model_without_dp)
    rec = {"outputs": [], "targets": [], "losses": [], "val_outputs": [], "val_losses": []}
    for epoch in range(epochs):
        np.random.seed(epoch)
        random.seed(epoch)
        ratio = 0.1 if epoch in schedule else 1.
        for param_group in optimizer.param_groups:
            param_group['lr'] = param_group['lr'] * ratio
        begin_epoch(call, model_without_dp, train_what)
        for input_seq, target in train_loader:
            train_step(call, optimizer, ce_loss, input_seq, target, device, seq_len, img_dim, calc_topk_accuracy,
                       rec)
        if validate:
            call.eval()
            with torch.no_grad():
                for input_seq, target in val_loader:
                    input_seq = _tr(input_seq.to(device, non_blocking=True), False, 1, seq_len, img_dim)
                    target = target.to(device, non_blocking=True)
                    input_seq = input_seq.squeeze(1)
                    logit, _ = call(input_seq)
                    loss = ce_loss(logit, target)
                    top1, top5 = calc_topk_accuracy(logit, target, (1, 5))
                    rec["val_outputs"].append(logit.detach().cpu().clone())
                    rec["val_losses"].append(loss.item())
                    top1.item(), top5.item()
    rec["model"] = model_without_dp
    rec["optimizer"] = optimizer
    return rec
