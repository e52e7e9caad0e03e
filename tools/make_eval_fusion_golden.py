"""Writes tests/golden/eval_fusion.pt: what the reference's OWN eval/merge_2stream_prob.py and
eval/feature_linear_probe.py make of small inputs.

    python tools/make_eval_fusion_golden.py --reference <checkout of the reference project>

Both files are imported UNMODIFIED (the script asserts that the modules it runs live under the given tree).  What
this script supplies, none of it part of what is recorded:

  * stand-ins for modules absent where this project is developed, which the files (or utils/utils.py) import at the
    top and never use here: `torchvision`, `tensorboardX` (as tests/dropin_harness.py does); `.cuda()` is the
    identity;
  * `np.int = int`: merge_prob calls np.int, which numpy 1.24 removed;
  * `get_action_idx` returns the fixture's action list: the reference's reads a path that exists only on its
    authors' machines;
  * `sys.exit()` at the end of merge_prob / merge_sim is caught.

The input files are written with coclr_amd.eval.fusion's own save_probs / save_features, so the reference reading
them is half of the interoperability the tests claim.

merge_sim: features of widths 24 and 20, 96 training and 40 test videos, 30 classes; stream 2 holds extra videos and
a different order.  `sim` is captured by wrapping torch.topk.  The seed is the first for which (a) the five accuracies
are distinct and strictly between 0 and 1, (b) wherever a test row's first label match sits at rank k, the fused
similarities at ranks k-1, k and k, k+1 differ by more than 1e-3 -- more than twice the 4e-4 a fused entry may move
-- and (c) the alignment drops at least one video.

merge_prob: 12 videos, 5 classes, file 1 in the flat form and file 2 in the mean_prob form; the three arg-maxima
differ on one video and one fused row has a tie.

Linear probe: 80 training rows of width 24 in 7 classes (batches of 32 end in one of 16), 40 test rows, 4 epochs,
schedule [2], eval_freq 2, lr 1.0, wd 1e-3, with final_bn on and off, driven through the reference's LP, D,
train_one_epoch, validate and adjust_learning_rate under torch.manual_seed(0) in the order of its main().  Recorded:
every index batch (D.__getitem__ is instrumented), the meters' averages and the printed lines, the final state dict,
the saved probabilities, torch.rand(1) drawn right after the run, the same run in float64 (from the same fp32
initialisation and the same batches), and per tensor `e_ref`, the relative L2 distance of the fp32 result from the
float64 one.  The script asserts that at every step the two largest logits of every row differ by more than 1e-4."""
import argparse
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from coclr_amd.eval import fusion      # noqa: E402

DATASET = "ucf101"
ACTIONS = ["Archery", "Biking", "Diving", "Fencing", "Kayaking"]


def install_stand_ins():
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    tbx = types.ModuleType("tensorboardX")
    tbx.SummaryWriter = object
    for name, mod in (("torchvision", tv), ("torchvision.transforms", tv.transforms), ("tensorboardX", tbx)):
        sys.modules.setdefault(name, mod)
    if not hasattr(np, "int"):
        np.int = int
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self


def load_reference(tree, name):
    tree = os.path.realpath(tree)
    if tree not in sys.path:
        sys.path.insert(1, tree)                  # `from utils.utils import ...`
    path = os.path.join(tree, "eval", name + ".py")
    spec = importlib.util.spec_from_file_location("reference_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert os.path.realpath(mod.__file__).startswith(tree + os.sep), mod.__file__
    assert os.path.realpath(sys.modules["utils.utils"].__file__).startswith(tree + os.sep)
    return mod


def run_to_exit(fn, args):
    """fn(args) until its sys.exit(); returns what it printed."""
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
        try:
            fn(args)
        except SystemExit:
            pass
    return buf.getvalue().splitlines()


def l2(got, ref):
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    return float((got - ref).norm() / (ref.norm() + 1e-300))


# ---- merge_sim -------------------------------------------------------------------------------------------------

def sim_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    ntr, nte, extra_tr, extra_te, ncls = 96, 40, 5, 3, 30
    out = {}
    for split, n, extra in (("train", ntr, extra_tr), ("test", nte, extra_te)):
        names = ["%s/v_%s_%03d" % (DATASET, split, i) for i in range(n + extra)]
        order1 = torch.randperm(n, generator=g)
        order2 = torch.randperm(n + extra, generator=g)
        out[split] = {
            "names1": [names[i] for i in order1.tolist()],
            "feature1": torch.randn(n, 24, generator=g),
            "label1": torch.randint(0, ncls, (n,), generator=g),
            "names2": [names[i] for i in order2.tolist()],
            "feature2": torch.randn(n + extra, 20, generator=g),
            # stream 2's labels are never read by the reference
            "label2": torch.randint(0, ncls, (n + extra,), generator=g),
        }
    return out


def run_merge_sim(M, inp, tmp):
    d1, d2 = os.path.join(tmp, "s1"), os.path.join(tmp, "s2")
    os.makedirs(d1, exist_ok=True)
    os.makedirs(d2, exist_ok=True)
    tr, te = inp["train"], inp["test"]
    fusion.save_features(d1, DATASET, tr["feature1"], tr["label1"], tr["names1"], te["feature1"], te["label1"],
                         te["names1"])
    fusion.save_features(d2, DATASET, tr["feature2"], tr["label2"], tr["names2"], te["feature2"], te["label2"],
                         te["names2"], flow=True)
    seen = []
    topk = torch.topk

    def observed(x, k, *a, **kw):
        r = topk(x, k, *a, **kw)
        seen.append((x.detach().clone(), k, r[1].clone()))
        return r
    torch.topk = observed
    try:
        lines = run_to_exit(M.merge_sim, argparse.Namespace(prob1=d1, prob2=d2, dataset=DATASET, mode="s"))
    finally:
        torch.topk = topk
    assert [k for _, k, _ in seen] == [1, 5, 10, 20, 50] and len(lines) == 5, lines
    sim = seen[0][0]
    assert all(torch.equal(s, sim) for s, _, _ in seen)
    return {"sim": sim, "top50": seen[-1][2], "lines": lines,
            "printed": [float(line.split("=")[1]) for line in lines]}


def sim_conditions(inp, rec):
    """The three conditions of the module docstring, from the recorded `sim` and the aligned labels."""
    tr, te = inp["train"], inp["test"]
    sim = rec["sim"]
    dropped = (len(tr["names2"]) - sim.shape[1]) + (len(te["names2"]) - sim.shape[0])
    trl = tr["label1"][np.argsort(np.array(tr["names1"]))]
    tel = te["label1"][np.argsort(np.array(te["names1"]))]
    acc = []
    for k in (1, 5, 10, 20, 50):
        idx = torch.topk(sim, k, dim=1)[1]
        acc.append(torch.any(trl[idx] == tel.unsqueeze(1), dim=1).float().mean().item())
    assert ["%.4f" % a for a in acc] == ["%.4f" % p for p in rec["printed"]], (acc, rec["printed"])
    rec["acc"] = acc
    distinct = len(set(acc)) == 5 and all(0.0 < a < 1.0 for a in acc)
    val, idx = torch.sort(sim, dim=1, descending=True, stable=True)
    match = trl[idx] == tel.unsqueeze(1)
    margin = float("inf")
    for r in range(sim.shape[0]):
        hit = match[r].nonzero()
        if hit.numel() == 0:
            continue
        k = int(hit[0])                                   # 0-based rank of the first match
        for a, b in ((k - 1, k), (k, k + 1)):
            if a >= 0 and b < sim.shape[1] and bool(match[r, a]) != bool(match[r, b]):
                margin = min(margin, float(val[r, a] - val[r, b]))
    rec["margin"] = margin
    return distinct and margin > 1e-3 and dropped >= 1


# ---- merge_prob ------------------------------------------------------------------------------------------------

def prob_inputs():
    g = torch.Generator().manual_seed(3)
    V, C_ = 12, len(ACTIONS)
    labels = torch.randint(0, C_, (V,), generator=g)
    names = ["%s/%s/v_%02d/clip" % (DATASET, ACTIONS[int(c)], i) for i, c in enumerate(labels)]
    p1 = torch.softmax(torch.randn(V, C_, generator=g) + 2.0 * torch.nn.functional.one_hot(labels, C_), 1)
    p2 = torch.softmax(torch.randn(V, C_, generator=g) + 1.0 * torch.nn.functional.one_hot(labels, C_), 1)
    # the three arg-maxima differ (0, 3, 1), and a fused tie between columns 0 and 1 (np.argmax takes 0)
    p1[4] = torch.tensor([0.4, 0.35, 0.25, 0.0, 0.0])
    p2[4] = torch.tensor([0.0, 0.35, 0.25, 0.4, 0.0])
    p1[7] = torch.tensor([0.5, 0.25, 0.25, 0.0, 0.0])
    p2[7] = torch.tensor([0.25, 0.5, 0.25, 0.0, 0.0])
    return {"names": names, "labels": labels, "actions": list(ACTIONS), "p1": p1, "p2": p2}


def run_merge_prob(M, inp, tmp):
    f1, f2 = os.path.join(tmp, "p1.json"), os.path.join(tmp, "p2.json")
    order2 = list(reversed(range(len(inp["names"]))))           # file 2 lists the videos in another order
    fusion.save_probs(f1, inp["names"], inp["p1"], form="flat")
    fusion.save_probs(f2, [inp["names"][i] for i in order2], inp["p2"][order2], form="mean_prob")
    M.get_action_idx = lambda dataset: list(inp["actions"])
    lines = run_to_exit(M.merge_prob, argparse.Namespace(prob1=f1, prob2=f2, dataset=DATASET, mode="c"))
    assert len(lines) == 1 and lines[0].startswith("merged accuracy"), lines
    am = [inp[k].double().argmax(1) for k in ("p1", "p2")] + [((inp["p1"].double() + inp["p2"].double()) / 2).argmax(1)]
    assert any(len({int(a[v]) for a in am}) == 3 for v in range(12))
    fused7 = (inp["p1"][7].double() + inp["p2"][7].double()) / 2
    assert fused7[0] == fused7[1] == fused7.max()
    inp.update(line=lines[0], file1=open(f1).read(), file2=open(f2).read())
    return inp


# ---- linear probe ----------------------------------------------------------------------------------------------

def probe_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    ntr, nte, dim, ncls = 80, 40, 24, 7
    centres = torch.randn(ncls, dim, generator=g)
    trl = torch.randint(0, ncls, (ntr,), generator=g)
    tel = torch.randint(0, ncls, (nte,), generator=g)
    trl[:ncls] = torch.arange(ncls)                              # every class occurs: num_class = 7
    return {"train_feature": centres[trl] + 1.5 * torch.randn(ntr, dim, generator=g), "train_label": trl,
            "test_feature": centres[tel] + 1.5 * torch.randn(nte, dim, generator=g), "test_label": tel,
            "test_vname": ["%s/c/v_%02d/clip" % (DATASET, i) for i in range(nte)]}


PROBE = dict(batch_size=32, lr=1.0, wd=1e-3, epochs=4, eval_freq=2, schedule=[2])


def run_probe(P, inp, final_bn, dtype, tmp):
    """The body of the reference's main() (:116-149) on its own pieces."""
    args = argparse.Namespace(test=os.path.join(tmp, "ckpt"), dirname="feature", dataset=DATASET, verbose=0,
                              normalize=False, final_bn=final_bn, **PROBE)
    os.makedirs(os.path.join(tmp, "feature"), exist_ok=True)
    passes, meters, gaps = [], [], []
    inner_get = P.D.__getitem__

    def getitem(self, index):
        passes[-1][2].append(int(index))
        return inner_get(self, index)

    class Meter(P.AverageMeter):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            meters.append(self)
    saved = (P.D.__getitem__, P.AverageMeter)
    P.D.__getitem__, P.AverageMeter = getitem, Meter
    out = {"train_loss": [], "train_acc": [], "val_loss": [], "val_acc": [], "val_epochs": []}
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            torch.manual_seed(0)
            model = P.LP(inp["train_feature"].size(-1), int(inp["train_label"].max().item()) + 1, final_bn)
            model.cuda()
            out["init_state"] = {k: v.clone() for k, v in model.state_dict().items()}
            model.to(dtype)                                      # float64 run: same initialisation, same draws
            model.register_forward_hook(lambda m, i, o: gaps.append(float(
                (lambda t: (t[:, 0] - t[:, 1]).min())(o.detach().topk(2, dim=1)[0]))))
            criterion = torch.nn.CrossEntropyLoss()
            optimizer = torch.optim.SGD(model.parameters(), lr=args.lr, weight_decay=args.wd, momentum=0.9)
            train_loader = torch.utils.data.DataLoader(
                P.D(inp["train_feature"].to(dtype), inp["train_label"]), batch_size=args.batch_size, shuffle=True,
                drop_last=False, num_workers=0)
            test_loader = torch.utils.data.DataLoader(
                P.D(inp["test_feature"].to(dtype), inp["test_label"], inp["test_vname"]),
                batch_size=args.batch_size, shuffle=False, drop_last=False, num_workers=0)
            best_acc, best_epoch, best_model = 0.0, 0, None
            for epoch in range(args.epochs):
                P.adjust_learning_rate(optimizer, epoch, args)
                passes.append(("train", epoch, []))
                P.train_one_epoch(train_loader, model, criterion, optimizer, epoch, args)
                out["train_loss"].append(meters[-2].avg)
                out["train_acc"].append(meters[-1].avg)
                if epoch % args.eval_freq == 0:
                    passes.append(("val", epoch, []))
                    val_acc = P.validate(test_loader, model, criterion, epoch, args)
                    out["val_loss"].append(meters[-2].avg)
                    out["val_acc"].append(meters[-1].avg)
                    out["val_epochs"].append(epoch)
                    if val_acc >= best_acc:
                        best_acc, best_epoch, best_model = val_acc, epoch, model.state_dict()
            model.load_state_dict(best_model)
            passes.append(("final", None, []))
            P.validate(test_loader, model, criterion, best_epoch, args, save_prob=True)
            out["final_loss"], out["final_acc"] = meters[-2].avg, meters[-1].avg
            out["rand"] = torch.rand(1)
    finally:
        P.D.__getitem__, P.AverageMeter = saved
    with open(os.path.join(tmp, "feature", "ckpt-lp-%s-prob.json" % DATASET)) as fp:
        saved_probs = json.load(fp)
    assert list(saved_probs) == inp["test_vname"]
    B = args.batch_size
    lines = [line for line in buf.getvalue().splitlines() if not line.startswith("prob saved to")]
    out.update(best_acc=best_acc, best_epoch=best_epoch, lines=lines, min_gap=min(gaps),
               state={k: v.detach().clone() for k, v in model.state_dict().items()},
               probs=torch.tensor(np.stack([np.asarray(saved_probs[v]).reshape(-1) for v in inp["test_vname"]]),
                                  dtype=dtype),
               batches=[(ph, ep, [torch.tensor(ix[i:i + B]) for i in range(0, len(ix), B)]) for ph, ep, ix in passes])
    return out


def probe_record(P, inp, final_bn, tmp):
    r32 = run_probe(P, inp, final_bn, torch.float32, tmp)
    r64 = run_probe(P, inp, final_bn, torch.float64, tmp)
    assert r32["min_gap"] > 1e-4 and r64["min_gap"] > 1e-4, (r32["min_gap"], r64["min_gap"])
    assert torch.equal(r32["rand"], r64["rand"])
    assert all(torch.equal(a, b) for (_, _, x), (_, _, y) in zip(r32["batches"], r64["batches"]) for a, b in zip(x, y))
    assert [r32[k] for k in ("train_acc", "val_acc", "final_acc")] == [r64[k] for k in ("train_acc", "val_acc", "final_acc")]
    losses = lambda r: torch.tensor(r["train_loss"] + r["val_loss"] + [r["final_loss"]], dtype=torch.float64)   # noqa: E731
    e_ref = {k: l2(v, r64["state"][k]) for k, v in r32["state"].items() if v.is_floating_point()}
    e_ref["losses"] = l2(losses(r32), losses(r64))
    e_ref["probs"] = l2(r32["probs"], r64["probs"])
    rec = dict(r32)
    rec["fp64"] = {"state": r64["state"], "probs": r64["probs"], "losses": losses(r64)}
    rec["e_ref"] = e_ref
    rec["final_bn"] = final_bn
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("COCLR_REFERENCE"), required="COCLR_REFERENCE" not in os.environ)
    args = ap.parse_args()
    install_stand_ins()
    M = load_reference(args.reference, "merge_2stream_prob")
    P = load_reference(args.reference, "feature_linear_probe")
    fix = {"torch": torch.__version__, "dataset": DATASET}
    with tempfile.TemporaryDirectory() as tmp:
        for seed in range(200):
            inp = sim_inputs(seed)
            rec = run_merge_sim(M, inp, tmp)
            if sim_conditions(inp, rec):
                fix["sim"] = {"seed": seed, "inputs": inp, **rec}
                break
        assert "sim" in fix
        fix["prob"] = run_merge_prob(M, prob_inputs(), tmp)
        fix["probe"] = {"args": dict(PROBE), "inputs": probe_inputs(11)}
        for final_bn in (False, True):
            fix["probe"]["bn" if final_bn else "plain"] = probe_record(P, fix["probe"]["inputs"], final_bn, tmp)
    out = os.path.join(ROOT, "tests", "golden", "eval_fusion.pt")
    torch.save(fix, out)
    print("wrote %s (%d bytes), merge_sim seed %d, acc %s, margin %.2e" % (
        out, os.path.getsize(out), fix["sim"]["seed"], fix["sim"]["acc"], fix["sim"]["margin"]))
    print(fix["prob"]["line"])
    for tag in ("plain", "bn"):
        r = fix["probe"][tag]
        print(tag, "best %.4f @ %d" % (r["best_acc"], r["best_epoch"]), "min logit gap %.2e" % r["min_gap"],
              {k: "%.2e" % v for k, v in r["e_ref"].items()})
        print("  ", r["lines"])
    assert os.path.getsize(out) <= 200000


if __name__ == "__main__":
    main()
