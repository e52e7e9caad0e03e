"""The classifier's fine-tuning loop (eval/main_classifier.py, restated by tests/_classifier_loop.py) on the
HIP kernels: S3D LinearClassifier(num_class=101), clips 3x32x128x128, B = 8, four epochs of two steps
with a validation pass after each, so the later steps run from the optimisers' launch plans.  At every
step the update the native optimiser applied equals torch's own optimiser (saved before install())
stepping shadow copies of the same parameters from the same gradients, its state evolving on its own
(1e-6 relative, the optimiser tests' bar), with exactly one optimiser launch per step."""
import pytest
import torch

from _cases import check_close

pytestmark = pytest.mark.gpu


class _Clips(torch.utils.data.Dataset):
    def __init__(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        self.frames = torch.rand(n, 3, 32, 128, 128, generator=g)
        self.label = torch.randint(0, 101, (n,), generator=g)

    def __len__(self):
        return self.label.shape[0]

    def __getitem__(self, i):
        return self.frames[i], self.label[i]


@pytest.mark.parametrize("train_what,optim", [("ft", "sgd"), ("ft", "adam"), ("last", "sgd")])
def test_finetune_steps_match_torch_optimizer(monkeypatch, train_what, optim):
    import model.classifier as product
    import _classifier_loop
    from coclr_amd import ops
    from coclr_amd import optim as O
    from oracle import coclr_oracle as orc
    launches = [0]
    name = "sgd_step" if optim == "sgd" else "adam_step"
    inner_launch = getattr(ops, name)

    def counted(*a, **k):
        launches[0] += 1
        return inner_launch(*a, **k)
    monkeypatch.setattr(ops, name, counted)
    seen = {"steps": 0}

    def on_optimizer(opt, model):
        assert isinstance(opt, O.SGD if optim == "sgd" else O.Adam)
        params = [p for g in opt.param_groups for p in g["params"]]
        shadows = [p.detach().clone() for p in params]
        groups = []
        for g, s in zip(opt.param_groups, shadows):
            h = {k: v for k, v in g.items() if k != "params"}
            h["params"] = [s]
            groups.append(h)
        ref = (O._TorchSGD if optim == "sgd" else O._TorchAdam)(groups)
        native_step = opt.step

        def step(closure=None):
            for p, s, g, rg in zip(params, shadows, opt.param_groups, ref.param_groups):
                s.copy_(p.detach())
                s.grad = None if p.grad is None else p.grad.detach().clone()
                rg["lr"] = g["lr"]
            before = launches[0]
            native_step()
            assert launches[0] - before == 1, "one optimiser launch per step"
            ref.step()
            for i, (p, s) in enumerate(zip(params, shadows)):
                if p.grad is not None:
                    check_close(p, s, 1e-6, "step %d parameter %d" % (seen["steps"], i))
            seen["steps"] += 1
        opt.step = step
        seen["opt"] = opt

    rec = _classifier_loop.run_classifier(product, _Clips(16, 41), _Clips(8, 42), train_what=train_what,
                                          optim=optim, batch_size=8, seq_len=32, img_dim=128, gpu=0,
                                          calc_topk_accuracy=orc.calc_topk_accuracy, on_optimizer=on_optimizer,
                                          epochs=4)
    torch.cuda.synchronize()
    assert seen["steps"] == 8 and len(rec["losses"]) == 8 and len(rec["val_losses"]) == 4
    assert all(torch.isfinite(torch.tensor(rec["losses"] + rec["val_losses"])))
    assert seen["opt"]._plan is not None
