"""GPU tier of the two-stream fusion and the cached-feature linear probe: `coclr_fuse_scores` exact against the
float64 restatement (tests/_fusion_ref.py, which tests/test_eval_fusion_cpu.py holds to the reference), the fused
retrieval against the fixture and bit-equal to the sum of two one-stream retrievals, and `linear_probe.fit` against
the reference's own run recorded in tests/golden/eval_fusion.pt.

Linear probe bound (set before anything was measured): every state-dict tensor, the vector of epoch losses and the
saved probabilities lie within 8 x e_ref of the reference's FLOAT64 run in relative L2, e_ref being the distance of
the reference's own fp32 run from it (1e-7 .. 3e-7 here), with a floor of 1e-6 below which the float64 comparison
itself is noise.  Measured ratios err / e_ref on MI355X are listed in test_fit_follows_the_reference (largest: 5.2)."""
import pytest
import torch

import _fusion_ref as R
from _cases import l2_err, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fix():
    return load_golden("eval_fusion")


# ---- coclr_fuse_scores ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", R.FUSE_C)
def test_fuse_scores_exact(C):
    from coclr_amd.eval import fusion
    for V in R.FUSE_V:
        p1, p2, labels = R.fuse_case(V, C, 100 * C + V)
        fused, am, hits, acc = R.merge_prob(p1, p2, labels)
        got = fusion.fuse_probs(p1.cuda(), p2.cuda(), labels.cuda())
        assert got.fused.dtype == torch.float64 and torch.equal(got.fused.cpu(), fused), (V, C)
        assert got.argmax.dtype == torch.int32 and torch.equal(got.argmax.cpu(), am), (V, C)
        assert torch.equal(got.hits.cpu(), hits), (V, C)
        assert torch.allclose(got.acc.cpu().double(), torch.tensor(acc, dtype=torch.float64), rtol=0, atol=1e-6)


def test_fuse_probs_refuses_strided_input():
    from coclr_amd.eval import fusion
    p = torch.rand(4, 10, device="cuda")
    with pytest.raises(ValueError):
        fusion.fuse_probs(p[:, ::2], p[:, ::2], torch.zeros(4, dtype=torch.long, device="cuda"))
    with pytest.raises(ValueError):
        fusion.fuse_probs(p, p[:, :5].contiguous(), torch.zeros(4, dtype=torch.long, device="cuda"))


def test_fuse_probs_on_the_fixture(fix):
    from coclr_amd.eval import fusion
    g = fix["prob"]
    res = fusion.fuse_probs(g["p1"].cuda(), g["p2"].cuda(), g["labels"].cuda())
    assert "merged accuracy: %.6f + %.6f => %.6f" % tuple(res.acc.tolist()) == g["line"]


# ---- two-stream retrieval ------------------------------------------------------------------------------------------

def _aligned(fix):
    from coclr_amd.eval import fusion
    out = {}
    for split in ("train", "test"):
        d = fix["sim"]["inputs"][split]
        i1, i2 = fusion.align_by_name(d["names1"], d["names2"])
        out[split] = (fusion.take_rows(d["feature1"].cuda(), i1), fusion.take_rows(d["feature2"].cuda(), i2),
                      fusion.take_rows(d["label1"].cuda(), i1))
        assert torch.equal(out[split][0].cpu(), d["feature1"][i1]) and torch.equal(out[split][2].cpu(), d["label1"][i1])
        assert torch.equal(out[split][1].cpu(), d["feature2"][i2])
    return out


def test_two_stream_retrieval_on_the_fixture(fix):
    from coclr_amd.eval import fusion
    from coclr_amd.eval.retrieval import nn_retrieval
    g = fix["sim"]
    a = _aligned(fix)
    (te1, te2, tel), (tr1, tr2, trl) = a["test"], a["train"]
    acc, sim, topidx = fusion.nn_retrieval_two_stream(te1, tr1, te2, tr2, tel, trl)
    err = float((sim.cpu() - g["sim"]).abs().max())
    print("fused sim: max abs distance from the reference's %.3e" % err)
    assert err <= 4e-4
    got = torch.gather(g["sim"], 1, topidx.cpu().long())
    want = torch.gather(g["sim"], 1, g["top50"])
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-5
    assert [round(float(x), 5) for x in acc] == [round(x, 5) for x in g["acc"]]
    _, sim1, _ = nn_retrieval(te1, tel, tr1, trl)
    _, sim2, _ = nn_retrieval(te2, tel, tr2, trl)
    assert torch.equal(sim, sim1 + sim2)


@pytest.mark.parametrize("ntr,nte,ks", [(41000, 6, (1, 5, 20)), (50, 7, (1, 5, 10, 20, 50))])
def test_two_stream_retrieval_other_shapes(ntr, nte, ks):
    """41000 columns take the selection kernel's global-memory path; 50 with k = 50 selects every column."""
    from coclr_amd.eval import fusion
    from coclr_amd.eval.retrieval import nn_retrieval
    gen = torch.Generator().manual_seed(ntr)
    te1, tr1 = torch.randn(nte, 16, generator=gen).cuda(), torch.randn(ntr, 16, generator=gen).cuda()
    te2, tr2 = torch.randn(nte, 12, generator=gen).cuda(), torch.randn(ntr, 12, generator=gen).cuda()
    trl = torch.randint(0, 50, (ntr,), generator=gen)
    tel = torch.randint(0, 50, (nte,), generator=gen)
    acc, sim, topidx = fusion.nn_retrieval_two_stream(te1, tr1, te2, tr2, tel.cuda(), trl.cuda(), ks)
    _, sim1, _ = nn_retrieval(te1, tel.cuda(), tr1, trl.cuda(), ks)
    _, sim2, _ = nn_retrieval(te2, tel.cuda(), tr2, trl.cuda(), ks)
    want = (sim1 + sim2).cpu()
    assert torch.equal(sim.cpu(), want)
    assert torch.equal(topidx.cpu().long(), R.ordered_top(want, ks[-1]))
    hits = R.knn_hits(want, trl, tel, ks)
    assert [round(float(x), 5) for x in acc] == [round(float(x), 5) for x in hits.mean(0)]


# ---- linear probe --------------------------------------------------------------------------------------------------

def _fit(fix, tag, monkeypatch=None, **kw):
    from coclr_amd.eval import linear_probe
    inp, args = fix["probe"]["inputs"], dict(fix["probe"]["args"])
    args.update(kw)
    seen = []
    if monkeypatch is not None:
        inner = linear_probe.draws

        def observed(*a):
            for phase, epoch, batches in inner(*a):
                rec = (phase, epoch, [])
                seen.append(rec)

                def tee(batches=batches, rec=rec):
                    for b in batches:
                        rec[2].append(b.clone())
                        yield b
                yield phase, epoch, tee()
        monkeypatch.setattr(linear_probe, "draws", observed)
    torch.manual_seed(0)
    res = linear_probe.fit(inp["train_feature"].cuda(), inp["train_label"].cuda(), inp["test_feature"].cuda(),
                           inp["test_label"].cuda(), final_bn=fix["probe"][tag]["final_bn"], **args)
    return res, seen, torch.rand(1)


def _split(line):
    """'train: Epoch[0] loss 1.2051 acc 0.5125' -> ('train: Epoch[0]', 1.2051, 'acc 0.5125')"""
    head, rest = line.split(" loss ")
    loss, tail = rest.split(" ", 1)
    return head, float(loss), tail


def _probs_of(state, x):
    """softmax of the probe with these weights in eval mode, float64 on the host."""
    x = x.double()
    sd = {k: v.detach().cpu().double() for k, v in state.items()}
    if "bn.weight" in sd:
        x = (x - sd["bn.running_mean"]) / torch.sqrt(sd["bn.running_var"] + 1e-5) * sd["bn.weight"] + sd["bn.bias"]
    return torch.softmax(x @ sd["fc.weight"].t() + sd["fc.bias"], 1)


@pytest.mark.parametrize("tag", ["plain", "bn"])
def test_fit_follows_the_reference(fix, tag, monkeypatch):
    """Measured err / e_ref on MI355X (bound 8, floor 1e-6 on err; the figures are printed below before anything is
    asserted).  plain: fc.weight 2.77, fc.bias 2.97, losses 1.62, probs 5.22 (1.11e-6 against 2.14e-7).
    bn: bn.weight 1.27, bn.bias 1.35, bn.running_mean 0.96, bn.running_var 1.16, fc.weight 1.30, fc.bias 3.42,
    losses 1.62, probs 1.12."""
    g = fix["probe"][tag]
    res_log = []
    res, seen, rand = _fit(fix, tag, monkeypatch, log=res_log.append)
    # the draws: the reference's index batches, and the generator where the reference left it
    assert [(p, e) for p, e, _ in seen] == [(p, e) for p, e, _ in g["batches"]]
    for (p, e, mine), (_, _, ref) in zip(seen, g["batches"]):
        assert len(mine) == len(ref) and all(torch.equal(x, y) for x, y in zip(mine, ref)), (p, e)
    assert torch.equal(rand, g["rand"])
    # the script's lines: the same epochs and accuracies as printed, the losses to the printed digit
    mine = [_split(line) for line in res_log if line.startswith(("train:", "eval["))]
    ref = [_split(line) for line in g["lines"]]
    assert [(h, t) for h, _, t in mine] == [(h, t) for h, _, t in ref]
    assert all(abs(a - b) <= 1.0001e-4 for (_, a, _), (_, b, _) in zip(mine, ref))
    assert "Best acc: %.4f" % g["best_acc"] in res_log and "Final best acc: %.4f" % g["best_acc"] in res_log
    epochs = [h for h in res.history if not h.get("final")]
    final = res.history[-1]
    losses = torch.tensor([h["train_loss"] for h in epochs] + [h["val_loss"] for h in epochs if "val_loss" in h] +
                          [final["val_loss"]], dtype=torch.float64)
    errs = {k: l2_err(v, g["fp64"]["state"][k]) for k, v in res.state_dict.items() if v.is_floating_point()}
    errs["losses"] = l2_err(losses, g["fp64"]["losses"])
    errs["probs"] = l2_err(res.probs, g["fp64"]["probs"])
    for k, e in errs.items():
        print("%s %-16s err %.3e  e_ref %.3e  ratio %.2f" % (tag, k, e, g["e_ref"][k], e / g["e_ref"][k]))
    # top-1 averages: equal
    assert [h["train_acc"] for h in epochs] == g["train_acc"]
    assert [h["val_acc"] for h in epochs if "val_acc" in h] == g["val_acc"]
    assert [h["epoch"] for h in epochs if "val_acc" in h] == g["val_epochs"]
    assert final["val_acc"] == g["final_acc"]
    assert (res.best_acc, res.best_epoch) == (g["best_acc"], g["best_epoch"])
    assert sorted(errs) == sorted(g["e_ref"])
    assert int(res.state_dict.get("bn.num_batches_tracked", 0)) == int(g["state"].get("bn.num_batches_tracked", 0))
    for k, e in errs.items():
        assert e <= max(8 * g["e_ref"][k], 1e-6), "%s: %.3e vs float64, the reference's fp32 run %.3e" % (
            k, e, g["e_ref"][k])
    # default mode: the probabilities are those of the FINAL weights, as in the script
    want = _probs_of(res.state_dict, fix["probe"]["inputs"]["test_feature"])
    assert l2_err(res.probs, want) <= 1e-6
    assert res.best_epoch != fix["probe"]["args"]["epochs"] - 1          # ... which are not the best epoch's here


def test_fit_snapshot_best_keeps_the_best_epoch(fix):
    """The best epoch of the fixture is epoch 0: a one-epoch run under the same seed ends with its weights."""
    g = fix["probe"]["plain"]
    assert g["best_epoch"] == 0
    first, _, _ = _fit(fix, "plain", epochs=1)
    snap, _, _ = _fit(fix, "plain", snapshot_best=True)
    assert (snap.best_acc, snap.best_epoch) == (g["best_acc"], 0)
    for k, v in first.state_dict.items():
        assert l2_err(snap.state_dict[k], v) <= 1e-6, k
    assert l2_err(snap.probs, first.probs) <= 1e-6
    last, _, _ = _fit(fix, "plain")
    assert l2_err(snap.probs, last.probs) > 1e-3                        # the default saves other probabilities
