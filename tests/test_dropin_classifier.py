"""The reference's eval/main_classifier.py executed UNMODIFIED (imported from /root/reference) on this
repository's shadow packages: fine-tuning (`--train_what ft`, SGD and Adam) and the end-to-end linear
probe (`--train_what last`, SGD) from a pretraining checkpoint (`--pretrain`, the README recipe).  Its
real `main(args)` is driven: LinearClassifier construction, the per-tensor param groups, `optim.SGD` /
`optim.Adam`, DataParallel, `nn.CrossEntropyLoss`, the script's data loaders, `train_one_epoch`,
`validate`, checkpoint save (tests/classifier_harness.py lists what the harness supplies).  Kernels are the
ATen double here (CPU tier); the comparison is the same script on the reference's OWN model, live, in
the same test.  Skipped where /root/reference does not exist (the GPU box)."""
import pytest
import torch

import classifier_harness as CH
import dropin_harness as H
import fake_backend
from _cases import check_close

pytestmark = pytest.mark.skipif(not CH.reference_available(), reason="needs /root/reference")

CASES = [("ft", "sgd"), ("ft", "adam"), ("last", "sgd")]


@pytest.fixture
def fake(monkeypatch):
    fake_backend.install(monkeypatch)


@pytest.fixture(autouse=True)
def _leave_a_core_free():
    """As in tests/test_dropin_scripts.py: the script runs next to its own helper threads."""
    n = torch.get_num_threads()
    torch.set_num_threads(max(1, min(n, 4)))
    yield
    torch.set_num_threads(n)


def _data():
    return (CH.LabelledClips(12, 8, 64, 101, seed=31), CH.LabelledClips(8, 8, 64, 101, seed=32))


def _argv(train_what, optim, pretrain, dropout=None):
    argv = ["--net", "s3d", "--dataset", "ucf101", "--seq_len", "8", "--img_dim", "64", "--batch_size", "4",
            "--epochs", "1", "--workers", "0", "--print_freq", "1", "--train_what", train_what,
            "--optim", optim, "--pretrain", pretrain]
    if dropout is not None:
        argv += ["--dropout", str(dropout)]
    return argv


def _pretrained(tmp_path):
    H.write_pretrained_pair(str(tmp_path), use_reference_model=False)
    return str(tmp_path / "rgb.pth.tar")


@pytest.mark.parametrize("train_what,optim", CASES)
def test_unmodified_classifier_script_on_shadow_modules(fake, tmp_path, train_what, optim):
    from coclr_amd import optim as native
    train, val = _data()
    pre = _pretrained(tmp_path)
    argv = _argv(train_what, optim, pre, dropout=0)
    mine = CH.run_classifier_script(argv, train, val, False, str(tmp_path / "product"))
    # inside the product run the script's torch.optim classes are the native subclasses
    assert issubclass(mine["torch_optim"][0], native.SGD) and issubclass(mine["torch_optim"][1], native.Adam)
    opt = mine["optimizer"]
    assert isinstance(opt, native.SGD if optim == "sgd" else native.Adam)
    assert opt._ours is True          # the product's classifier: the single-launch step's parameters
    ref = CH.run_classifier_script(argv, train, val, True, str(tmp_path / "reference"))
    # install() is process-wide: the reference model's optimiser is the subclass, on torch's path
    assert isinstance(ref["optimizer"], native.SGD if optim == "sgd" else native.Adam)
    assert ref["optimizer"]._ours is False and ref["optimizer"]._plan is None
    n = len(ref["outputs"])
    assert n == 3 and len(mine["outputs"]) == len(mine["losses"]) == n
    for i in range(n):
        assert torch.equal(mine["targets"][i], ref["targets"][i]), "targets of iteration %d" % i
        if i == 0:
            check_close(mine["outputs"][i], ref["outputs"][i], 1e-3, "logits of iteration 0")
            assert abs(mine["losses"][i] - ref["losses"][i]) <= 5e-3 * max(1.0, abs(ref["losses"][i]))
        else:
            # fine-tuning trains the backbone's BatchNorm biases from zero: their fp32 gradients (the
            # reference's ATen CPU kernels) and the double's differ by a large share of the first
            # updates (up to 1.7x relative after three steps), so the logits follow loosely (measured:
            # 0.38 of max|logit| at iteration 2 for ft/sgd, 0.15 for ft/adam, 1e-5 for last/sgd)
            check_close(mine["outputs"][i], ref["outputs"][i], 0.5, "logits of iteration %d" % i)
            assert abs(mine["losses"][i] - ref["losses"][i]) <= 1e-2 * max(1.0, abs(ref["losses"][i]))
    assert len(mine["val_outputs"]) == len(ref["val_outputs"]) == 2
    for a, b, ta, tb in zip(mine["val_outputs"], ref["val_outputs"], mine["val_targets"], ref["val_targets"]):
        assert torch.equal(ta, tb)
        check_close(a, b, 0.5, "validation logits")
    ck, rck = mine["checkpoint"], ref["checkpoint"]
    assert list(ck["state_dict"].keys()) == list(rck["state_dict"].keys())
    assert ck["epoch"] == rck["epoch"] and ck["iteration"] == rck["iteration"]
    og, rog = ck["optimizer"], rck["optimizer"]
    assert len(og["param_groups"]) == len(rog["param_groups"])
    assert [g["lr"] for g in og["param_groups"]] == [g["lr"] for g in rog["param_groups"]]
    assert sorted(og["state"]) == sorted(rog["state"])
    for k in rog["state"]:
        assert sorted(og["state"][k]) == sorted(rog["state"][k])
        if optim == "sgd":
            assert list(og["state"][k]) == ["momentum_buffer"]


@pytest.mark.parametrize("train_what,optim", CASES)
def test_restated_classifier_loop_is_the_script(fake, tmp_path, train_what, optim):
    """tests/_classifier_loop.py (what the GPU tier and tools/finetune_step.py run, the GPU box having
    no /root/reference) against the unmodified script on the same backend, at the script's default
    dropout: identical logits, targets and losses, iteration by iteration."""
    import model.classifier as product
    import _classifier_loop
    from oracle import coclr_oracle as orc
    train, val = _data()
    pre = _pretrained(tmp_path)
    rec = CH.run_classifier_script(_argv(train_what, optim, pre), train, val, False, str(tmp_path / "w"))
    with H.script_environment(False, True):        # same lenient Tensor.view as the script saw
        mine = _classifier_loop.run_classifier(product, train, val, train_what=train_what, optim=optim,
                                               pretrain=pre, calc_topk_accuracy=orc.calc_topk_accuracy)
    assert len(mine["outputs"]) == len(rec["outputs"]) == 3
    for i, (a, b) in enumerate(zip(mine["outputs"], rec["outputs"])):
        assert torch.equal(a, b), "logits of iteration %d differ" % i
        assert torch.equal(mine["targets"][i], rec["targets"][i])
        assert mine["losses"][i] == rec["losses"][i]
    assert len(mine["val_outputs"]) == len(rec["val_outputs"])
    for a, b in zip(mine["val_outputs"], rec["val_outputs"]):
        assert torch.equal(a, b)
    sd = mine["model"].state_dict()
    for k, v in rec["checkpoint"]["state_dict"].items():
        assert torch.equal(sd[k], v), k
