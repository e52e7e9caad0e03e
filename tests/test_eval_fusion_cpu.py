"""CPU tier of the two-stream fusion and the cached-feature linear probe (coclr_amd/eval/fusion.py,
coclr_amd/eval/linear_probe.py) against tests/golden/eval_fusion.pt, which tools/make_eval_fusion_golden.py recorded
from the reference's own eval/merge_2stream_prob.py and eval/feature_linear_probe.py: the numpy / torch
restatement the GPU tier compares with reproduces the reference, the host-side pieces (alignment, file formats, the
draw sequence, the meters, the argument parsers) are the reference's."""
import json

import numpy as np
import pytest
import torch

import _fusion_ref as R
from _cases import check_close, load_golden
from coclr_amd.eval import fusion, linear_probe


@pytest.fixture(scope="module")
def fix():
    return load_golden("eval_fusion")


# ---- the restatement reproduces the reference ------------------------------------------------------------------

def test_restated_merge_prob_is_the_references(fix):
    g = fix["prob"]
    fused, am, hits, acc = R.merge_prob(g["p1"], g["p2"], g["labels"])
    assert "merged accuracy: %.6f + %.6f => %.6f" % tuple(acc) == g["line"]
    assert len(set(am[4].tolist())) == 3                       # the three arg-maxima differ
    assert fused[7, 0] == fused[7, 1] == fused[7].max() and am[7, 2] == 0      # a fused tie: the first one


def test_restated_merge_sim_is_the_references(fix):
    g = fix["sim"]
    sim, top50, acc, _, _ = R.merge_sim(g["inputs"])
    assert sim.shape == g["sim"].shape == (40, 96)
    check_close(sim, g["sim"], 1e-6, "sim")
    assert torch.equal(top50, g["top50"])
    assert acc == g["acc"] and ["%.4f" % a for a in acc] == ["%.4f" % p for p in g["printed"]]
    assert torch.equal(R.ordered_top(g["sim"], 50), g["top50"])


def test_fuse_cases_hold_what_they_claim():
    """The inputs above do contain fused ties across lanes and waves' strides, and rows whose arg-maxima differ."""
    p1, p2, _ = R.fuse_case(70, 257, 1)
    fused, am, _, _ = R.merge_prob(p1, p2, torch.zeros(70, dtype=torch.long))
    gaps = set()
    for r in range(5):
        top = (fused[r] == fused[r].max()).nonzero().flatten().tolist()
        if len(top) == 2:
            gaps.add(top[1] - top[0])
            assert am[r, 2] == top[0]
    assert gaps == {1, 63, 64, 256}
    assert len(set(am[4].tolist())) == 3


# ---- align_by_name -----------------------------------------------------------------------------------------------

def test_align_by_name_on_the_fixture(fix):
    for split in ("train", "test"):
        d = fix["sim"]["inputs"][split]
        i1, i2 = fusion.align_by_name(d["names1"], d["names2"])
        r1, r2 = R.align(d["names1"], d["names2"])
        assert torch.equal(i1, r1) and torch.equal(i2, r2)
        assert len(i2) < len(d["names2"])                       # the alignment dropped videos


def test_align_by_name_cases():
    a = ["v/c", "v/a", "v/b"]
    i1, i2 = fusion.align_by_name(a, ["v/b", "v/c", "v/a"])         # equal sets, different order
    assert i1.tolist() == [1, 2, 0] and i2.tolist() == [2, 0, 1] and i1.dtype == torch.int64
    i1, i2 = fusion.align_by_name(a, ["v/z", "v/b", "v/c", "v/0", "v/a"])    # stream 2 the larger one
    assert i1.tolist() == [1, 2, 0] and i2.tolist() == [4, 1, 2]
    i1, i2 = fusion.align_by_name(["v/z", "v/b", "v/c", "v/0", "v/a"], a)    # stream 1 the larger one
    assert i1.tolist() == [4, 1, 2] and i2.tolist() == [1, 2, 0]
    assert fusion.align_by_name([["v/b"], ["v/a"]], ["v/a", "v/b"])[0].tolist() == [1, 0]   # a pickled (n, 1) list
    with pytest.raises(ValueError):
        fusion.align_by_name(a, ["v/a", "v/b", "v/d"])              # equal length, different names
    with pytest.raises(ValueError):
        fusion.align_by_name(a, ["v/a", "v/b", "v/c", "v/c"])       # duplicates
    with pytest.raises(ValueError):
        fusion.align_by_name(["v/a", "v/a", "v/b"], ["v/a", "v/b"])
    with pytest.raises(ValueError):
        fusion.align_by_name(a, ["v/a", "v/b", "v/x", "v/y"])       # the shorter list is no subset


# ---- files ---------------------------------------------------------------------------------------------------

def test_load_probs_reads_the_files_the_reference_read(fix, tmp_path):
    g = fix["prob"]
    for text, key, order in ((g["file1"], "p1", list(range(12))), (g["file2"], "p2", list(reversed(range(12))))):
        path = str(tmp_path / (key + ".json"))
        open(path, "w").write(text)
        names, probs = fusion.load_probs(path)
        assert names == [g["names"][i] for i in order]
        assert probs.dtype == torch.float32 and torch.equal(probs, g[key][order])
    assert isinstance(json.loads(g["file1"])[g["names"][0]], list)
    assert isinstance(json.loads(g["file2"])[g["names"][0]], dict)


@pytest.mark.parametrize("form", ["flat", "nested", "mean_prob"])
def test_save_probs_round_trips(fix, tmp_path, form):
    g = fix["prob"]
    path = str(tmp_path / "p.json")
    fusion.save_probs(path, g["names"], g["p1"], form=form)
    names, probs = fusion.load_probs(path)
    assert names == g["names"] and torch.equal(probs, g["p1"])
    entry = json.load(open(path))[g["names"][0]]
    if form == "mean_prob":
        assert np.array(entry["mean_prob"]).shape == (1, 5)          # main_classifier.py:535
    else:
        assert np.array(entry).shape == ((5,) if form == "flat" else (1, 5))


def test_load_probs_refuses_what_is_not_fp32(tmp_path):
    path = str(tmp_path / "p.json")
    json.dump({"a/b/c/d": [0.1, 0.9]}, open(path, "w"))
    with pytest.raises(ValueError):
        fusion.load_probs(path)


def test_feature_files_round_trip(fix, tmp_path):
    tr, te = fix["sim"]["inputs"]["train"], fix["sim"]["inputs"]["test"]
    for flow, s in ((False, "1"), (True, "2")):
        fusion.save_features(str(tmp_path), "hmdb51", tr["feature" + s], tr["label" + s], tr["names" + s],
                             te["feature" + s], te["label" + s], te["names" + s], flow=flow)
    prefix = "hmdb51-f_"
    for kind in ("train_feature.pth.tar", "test_label.pth.tar", "train_vname.pkl"):
        assert (tmp_path / (prefix + kind)).exists() and (tmp_path / ("hmdb51_" + kind)).exists()
    got = fusion.load_features(str(tmp_path), "hmdb51", flow=True)
    assert got["train_vname"] == tr["names2"] and got["test_vname"] == te["names2"]
    assert torch.equal(got["train_feature"], tr["feature2"]) and torch.equal(got["test_label"], te["label2"])


def test_labels_from_names(fix, tmp_path):
    g = fix["prob"]
    path = str(tmp_path / "ClassInd.txt")
    open(path, "w").write("".join("%d,%s\n" % (i + 1, a) for i, a in enumerate(g["actions"])))
    assert fusion.read_class_index(path) == g["actions"]
    assert torch.equal(fusion.labels_from_names(g["names"], g["actions"], "ucf101"), g["labels"])
    assert fusion.labels_from_names(["x/Biking/v.mp4"], g["actions"], "k400").tolist() == [1]


# ---- linear probe: construction, draws, meters ----------------------------------------------------------------

@pytest.mark.parametrize("tag", ["plain", "bn"])
def test_probe_construction_and_draws_follow_the_reference(fix, tag):
    g, a = fix["probe"][tag], fix["probe"]["args"]
    torch.manual_seed(0)
    model = linear_probe.LinearProbe(24, 7, final_bn=g["final_bn"])
    sd = model.state_dict()
    assert list(sd) == list(g["init_state"])
    for k, v in g["init_state"].items():
        assert torch.equal(sd[k], v), k
    model.load_state_dict(g["state"], strict=True)                  # the reference's LP state dict
    got = [(phase, epoch, [b.clone() for b in batches])
           for phase, epoch, batches in linear_probe.draws(80, 40, a["batch_size"], a["epochs"], a["eval_freq"])]
    assert [(p, e) for p, e, _ in got] == [(p, e) for p, e, _ in g["batches"]]
    for (p, e, mine), (_, _, ref) in zip(got, g["batches"]):
        assert len(mine) == len(ref) and all(torch.equal(x, y) for x, y in zip(mine, ref)), (p, e)
    assert [b.shape[0] for b in got[0][2]] == [32, 32, 16]
    assert torch.equal(torch.rand(1), g["rand"])                    # the generator is where the reference left it


def test_learning_rate_schedule():
    assert [linear_probe.learning_rate(1.0, e, [2]) for e in range(4)] == [1.0, 1.0, 0.1, 0.1]
    lr = 1.0
    lr *= 0.1
    lr *= 0.1
    assert linear_probe.learning_rate(1.0, 80, (60, 80)) == lr and linear_probe.learning_rate(1.0, 59, (60, 80)) == 1.0


def test_fold_meters_is_average_meter():
    # 36 of 40 right: hits / B rounded once (the kernel) is not fp32(hits) * fp32(1 / B) (the reference)
    k = np.float32(36.0 / 40.0)
    ref = float(np.float32(36.0) * np.float32(1 / 40))
    assert float(k) != ref
    loss, acc = linear_probe.fold_meters([[0.5, 1.0], [0.25, float(k)]], [32, 40])
    assert acc == (1.0 * 32 + ref * 40) / 72 and loss == (0.5 * 32 + 0.25 * 40) / 72


# ---- command lines ---------------------------------------------------------------------------------------------

def test_parsers_accept_the_references_flags():
    a = fusion.parse_args(["--prob1", "a.json", "--prob2", "b.json", "--dataset", "hmdb51", "--mode", "s"])
    assert (a.prob1, a.prob2, a.dataset, a.mode, a.class_index) == ("a.json", "b.json", "hmdb51", "s", "")
    d = fusion.parse_args([])
    assert (d.prob1, d.prob2, d.dataset, d.mode) == ("", "", "ucf101", "c")
    assert fusion.parse_args(["--class-index", "ClassInd.txt"]).class_index == "ClassInd.txt"
    p = linear_probe.parse_args(["--test", "m/ckpt.pth.tar", "--dataset", "hmdb51", "--dirname", "feat", "--batch_size",
                                 "64", "--lr", "0.5", "--wd", "0.01", "--epochs", "7", "--eval_freq", "2", "--verbose",
                                 "1", "--schedule", "3", "5", "--normalize", "--final_bn"])
    assert (p.test, p.dataset, p.dirname, p.batch_size, p.lr, p.wd, p.epochs, p.eval_freq, p.verbose, p.schedule,
            p.normalize, p.final_bn, p.snapshot_best) == ("m/ckpt.pth.tar", "hmdb51", "feat", 64, 0.5, 0.01, 7, 2, 1,
                                                          [3, 5], True, True, False)
    q = linear_probe.parse_args([])
    assert (q.batch_size, q.lr, q.wd, q.epochs, q.eval_freq, q.schedule, q.normalize, q.final_bn) == (
        1024, 1.0, 1e-3, 100, 5, [60, 80], False, False)


def test_fuse_scores_entry_point_rejects_on_the_host():
    """No launch: null pointers and empty shapes are answered with the invalid-value code."""
    from coclr_amd import _lib, ops
    lib = _lib.load()
    assert "coclr_fuse_scores" in _lib.EXPORTED_SYMBOLS
    a = ops.PLAN_ADDR
    assert lib.coclr_fuse_scores(None, a, a, a, a, a, 4, 5, None) == 1
    assert lib.coclr_fuse_scores(a, a, a, a, a, None, 4, 5, None) == 1
    assert lib.coclr_fuse_scores(a, a, a, a, a, a, 0, 5, None) == 1
    assert lib.coclr_fuse_scores(a, a, a, a, a, a, 4, 0, None) == 1
    with pytest.raises(ValueError):
        ops.fuse_scores(torch.zeros(2, 3), torch.zeros(2, 4), torch.zeros(2, dtype=torch.long),
                        torch.zeros(2, 3, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3))
