"""TEST INFRASTRUCTURE: run the reference's eval/main_classifier.py UNMODIFIED (imported from
/root/reference as it lies there) through its real `main(args)`, on this repository's shadow packages or
on the reference's own `model/`, `backbone/`.  Built on tests/dropin_harness.py (stand-in modules,
sys.path / sys.modules arrangement, the lenient Tensor.view).

What this helper adds, none of it part of the path under test:
  * the data: `get_data` / `get_transform` of the script are replaced by a synthetic labelled dataset
    (the real ones open LMDB files); the script's own `get_dataloader` and everything downstream runs;
  * no GPU in the build container: `.to(<cuda device>)` is the identity for tensors and modules, and
    CUDA_VISIBLE_DEVICES is set (main() reads it when --gpu is not given);
  * a temporary working directory for `set_path`; the script's closing `sys.exit(0)` is caught.

Observation points: the logits / targets the script hands to `calc_topk_accuracy` (train and
validation), the train losses its AverageMeter receives, the optimiser it built, the checkpoint file.
"""
import importlib.util
import os
import sys

import torch

import dropin_harness as H

SCRIPT = os.path.join(H.REF, "eval", "main_classifier.py")


def reference_available():
    return os.path.isfile(SCRIPT)


class LabelledClips(torch.utils.data.Dataset):
    """What the LMDB datasets hand to the classifier loop with return_label=True
    (dataset/lmdb_dataset.py): frames (C, seq_len, H, W) in [0,1) and a class index."""

    def __init__(self, n, seq_len, img_dim, num_class, seed):
        g = torch.Generator().manual_seed(seed)
        self.frames = torch.rand(n, 3, seq_len, img_dim, img_dim, generator=g)
        self.label = torch.randint(0, num_class, (n,), generator=g)

    def __len__(self):
        return self.label.shape[0]

    def __getitem__(self, i):
        return self.frames[i], self.label[i]


def _is_cuda(dev):
    return (isinstance(dev, torch.device) and dev.type == "cuda") or \
        (isinstance(dev, str) and dev.startswith("cuda"))


def run_classifier_script(argv, train_set, val_set, use_reference_model, workdir):
    """main(parse_args()) of the unmodified eval/main_classifier.py.  Returns the observation record
    {"outputs", "targets", "losses", "val_outputs", "optimizer", "torch_optim", "checkpoint"}."""
    rec = {"outputs": [], "targets": [], "losses": [], "val_outputs": [], "val_targets": []}
    phase = ["train"]
    cwd = os.getcwd()
    saved_argv = list(sys.argv)
    saved_env = os.environ.get("CUDA_VISIBLE_DEVICES")
    saved_bench = torch.backends.cudnn.benchmark
    tensor_to, module_to = torch.Tensor.to, torch.nn.Module.to

    def to_tensor(self, *a, **k):
        if _is_cuda(a[0] if a else k.get("device")):
            return self
        return tensor_to(self, *a, **k)

    def to_module(self, *a, **k):
        if _is_cuda(a[0] if a else k.get("device")):
            return self
        return module_to(self, *a, **k)
    with H.script_environment(use_reference_model, cpu=True):
        spec = importlib.util.spec_from_file_location("_ref_script_main_classifier", SCRIPT)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        want = H.REF if use_reference_model else H.REPO
        assert sys.modules["model.classifier"].__file__.startswith(want)
        assert sys.modules["utils.utils"].__file__.startswith(H.REF)
        mod.get_transform = lambda mode, args: None
        mod.get_data = lambda transform, mode, args: train_set if mode == "train" else val_set
        inner_acc = mod.calc_topk_accuracy

        def observed_acc(output, target, topk=(1,)):
            key = "outputs" if phase[0] == "train" else "val_outputs"
            rec[key].append(output.detach().cpu().clone())
            rec["targets" if phase[0] == "train" else "val_targets"].append(target.detach().cpu().clone())
            return inner_acc(output, target, topk)
        mod.calc_topk_accuracy = observed_acc
        meter = mod.AverageMeter

        class ObservedMeter(meter):
            def update(self, val, n=1, **kw):
                if self.name == "Loss":
                    rec["losses"].append(float(val))
                return meter.update(self, val, n, **kw)
        mod.AverageMeter = ObservedMeter
        inner_train, inner_val = mod.train_one_epoch, mod.validate

        def train_one_epoch(data_loader, model, criterion, optimizer, *a, **k):
            rec["optimizer"] = optimizer
            rec["torch_optim"] = (torch.optim.SGD, torch.optim.Adam)
            phase[0] = "train"
            return inner_train(data_loader, model, criterion, optimizer, *a, **k)

        def validate(*a, **k):
            phase[0] = "val"
            return inner_val(*a, **k)
        mod.train_one_epoch, mod.validate = train_one_epoch, validate
        os.makedirs(workdir, exist_ok=True)
        os.chdir(workdir)
        os.environ["CUDA_VISIBLE_DEVICES"] = "0"
        torch.Tensor.to, torch.nn.Module.to = to_tensor, to_module
        sys.argv = ["main_classifier.py"] + list(argv)
        try:
            args = mod.parse_args()
            try:
                mod.main(args)
                raise AssertionError("main() returned without sys.exit(0)")
            except SystemExit as e:
                assert e.code == 0, "the script exited with %r" % (e.code,)
            ckpt = os.path.join(args.model_path, "epoch%d.pth.tar" % (args.epochs - 1))
            rec["checkpoint"] = torch.load(ckpt, map_location="cpu", weights_only=False)
        finally:
            torch.Tensor.to, torch.nn.Module.to = tensor_to, module_to
            torch.backends.cudnn.benchmark = saved_bench
            sys.argv = saved_argv
            os.chdir(cwd)
            if saved_env is None:
                os.environ.pop("CUDA_VISIBLE_DEVICES", None)
            else:
                os.environ["CUDA_VISIBLE_DEVICES"] = saved_env
    return rec
