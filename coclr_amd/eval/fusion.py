"""Two-stream test-time fusion on MI355X (eval/merge_2stream_prob.py).

The reference fuses an RGB and a flow model after the fact, from files:

  merge_prob (:60-101)   reads two probability files, forms (prob1 + prob2) / 2 per video in float64 and counts
                         the top-1 hits of stream 1, stream 2 and the mean (np.argmax: the first maximum)
  merge_sim  (:104-198)  reads two sets of cached retrieval features, sorts both by video name, drops the videos
                         only one stream has, centres and L2-normalises each matrix, adds the two similarity
                         matrices and reports 1/5/10/20/50-NN accuracy

Here the inputs may stay where `VideoEvaluator` left them, on the device.  `fuse_probs` is ONE launch
(`coclr_fuse_scores`, csrc/retrieval.hip: float64 mean and the three arg-maxima per video, one wave each) plus the
column mean `nn_retrieval` also uses.  `nn_retrieval_two_stream` is `nn_retrieval` with a second GEMM that
accumulates into the first one's output: the GEMM's epilogue adds the finished dot product to C in one fp32 add, so
the fused matrix is bit-equal to `sim1 + sim2` of two `nn_retrieval` calls.  `align_by_name` is the host-side
bookkeeping of :118-170; the rows move on the device (`ops.gather_rows`).

File formats are the reference's, so its scripts and these read each other's files: `load_probs` / `save_probs`
(JSON: a video's entry is a flat list, the nested (1, C) list feature_linear_probe.py:199-203 writes, or
{'mean_prob': nested (1, C) list} as main_classifier.py:533-535 writes) and `load_features` / `save_features`
(`<dataset>_{train,test}_{feature,label}.pth.tar`, `<dataset>_{train,test}_vname.pkl`; stream 2 under the
`<dataset>-f` prefix, :105-137).

    python -m coclr_amd.eval.fusion --prob1 A --prob2 B --dataset ucf101 --mode c --class-index ClassInd.txt
    python -m coclr_amd.eval.fusion --prob1 DIR_A --prob2 DIR_B --dataset ucf101 --mode s

Deviations, all on the side of refusing: duplicate names raise (the reference's unstable argsort leaves their order
undefined); each pair of name lists decides for itself which side is the longer one (the reference lets the
training lists decide for the test lists too, and then fails its assert where the two disagree).
"""
import argparse
import collections
import json
import os
import pickle

import numpy as np
import torch

from .. import ops
from .retrieval import center_normalize

FusedScores = collections.namedtuple("FusedScores", "fused argmax hits acc")


def _column_mean(hits):
    """Mean over the rows of an fp32 (V, n) matrix, as nn_retrieval forms its accuracies."""
    V, n = hits.shape
    acc = torch.empty(n, dtype=torch.float32, device=hits.device)
    ops.colsum(hits, acc)
    ops.plane_scale(acc.view(1, n, 1, 1, 1), torch.full((1, n), 1.0 / V, device=hits.device), None,
                    acc.view(1, n, 1, 1, 1))
    return acc


def fuse_probs(p1, p2, labels):
    """merge_prob (:80-98) for all videos at once.  p1, p2: (V, C) fp32 contiguous device tensors; labels (V,)
    int64.  Returns FusedScores(fused (V, C) float64 = (p1 + p2) / 2 formed in double, argmax int32 (V, 3) = first
    maximum of p1, p2 and the mean, hits fp32 (V, 3) = argmax == label, acc fp32 (3,) = the three accuracies)."""
    if p1.dim() != 2 or p1.shape != p2.shape or p1.dtype != torch.float32 or p2.dtype != torch.float32:
        raise ValueError("coclr_amd: fuse_probs takes two fp32 (V, C) matrices of one shape")
    if not (p1.is_contiguous() and p2.is_contiguous()):
        raise ValueError("coclr_amd: fuse_probs takes contiguous probability matrices")
    V, C_ = p1.shape
    dev = p1.device
    labels = labels.to(device=dev, dtype=torch.long).contiguous()
    fused = torch.empty(V, C_, dtype=torch.float64, device=dev)
    argmax = torch.empty(V, 3, dtype=torch.int32, device=dev)
    hits = torch.empty(V, 3, dtype=torch.float32, device=dev)
    ops.fuse_scores(p1, p2, labels, fused, argmax, hits)
    return FusedScores(fused, argmax, hits, _column_mean(hits))


def nn_retrieval_two_stream(test1, train1, test2, train2, test_label, train_label, ks=(1, 5, 10, 20, 50)):
    """merge_sim (:178-196): every matrix centred and L2-normalised, sim = test1 . train1^T + test2 . train2^T,
    then the ordered top-max(ks) of every row and the k-NN hits.  The rows of the two streams must already be
    aligned (`align_by_name`); the feature widths may differ.  Returns (acc fp32 (len(ks),), sim fp32
    (n_test, n_train), topidx int32 (n_test, max(ks))) as `nn_retrieval` does; `sim` is bit-equal to the sum of the
    matrices two `nn_retrieval` calls return for the streams alone."""
    ks = [int(k) for k in ks]
    if ks != sorted(set(ks)) or ks[0] < 1:
        raise ValueError("coclr_amd: ks must be ascending, distinct and >= 1")
    nt, ntr = test1.shape[0], train1.shape[0]
    if test2.shape[0] != nt or train2.shape[0] != ntr:
        raise ValueError("coclr_amd: the two streams hold different numbers of videos; align them by name first")
    if test1.shape[1] != train1.shape[1] or test2.shape[1] != train2.shape[1] or ks[-1] > ntr:
        raise ValueError("coclr_amd: feature widths differ within a stream or k exceeds the training set")
    dev = test1.device
    sim = torch.empty(nt, ntr, dtype=torch.float32, device=dev)
    for accumulate, (te, tr) in enumerate(((test1, train1), (test2, train2))):
        te, tr = center_normalize(te), center_normalize(tr)
        C_ = te.shape[1]
        # sim[m][n] (+)= sum_c te[m][c] * tr[n][c]: the epilogue adds the finished product in one fp32 add (:184-187)
        ops.gemm(te, C_, 1, tr, 1, C_, sim, ntr, None, nt, ntr, C_, accumulate=bool(accumulate))
    ks_t = torch.tensor(ks, dtype=torch.int32).to(dev)
    hits = torch.empty(nt, len(ks), dtype=torch.float32, device=dev)
    topidx = torch.empty(nt, ks[-1], dtype=torch.int32, device=dev)
    ops.retrieval_hits(sim, train_label.to(device=dev, dtype=torch.long).contiguous(),
                       test_label.to(device=dev, dtype=torch.long).contiguous(), ks_t, hits, topidx)
    return _column_mean(hits), sim, topidx


# ---- alignment (host) ----------------------------------------------------------------------------------------

def _names(names):
    a = np.array(names)
    a = a.reshape(-1) if a.size == 1 else np.squeeze(a)           # :118 (a lone name squeezes to 0-d there)
    if a.ndim != 1:
        raise ValueError("coclr_amd: video names must form one list, got shape %s" % (a.shape,))
    return a


def align_by_name(names1, names2):
    """(:118-170) Returns int64 index tensors (idx1, idx2) with names1[idx1] == names2[idx2], in sorted name
    order: both lists are sorted, the longer one keeps the names the shorter one has, and the results must be
    equal.  ValueError where the reference's assert fails (the name sets differ beyond that) and on duplicates."""
    a, b = _names(names1), _names(names2)
    for n, which in ((a, 1), (b, 2)):
        if len(np.unique(n)) != len(n):
            raise ValueError("coclr_amd: stream %d lists a video name twice" % which)
    i1, i2 = np.argsort(a), np.argsort(b)
    if len(a) < len(b):
        i2 = i2[np.isin(b[i2], a)]
    elif len(a) > len(b):
        i1 = i1[np.isin(a[i1], b)]
    if len(i1) != len(i2) or not np.all(a[i1] == b[i2]):
        raise ValueError("coclr_amd: the two streams do not hold the same videos (%d and %d names; the shorter list "
                         "must be a subset of the longer one)" % (len(a), len(b)))
    return torch.from_numpy(i1.astype(np.int64)), torch.from_numpy(i2.astype(np.int64))


def take_rows(t, idx):
    """t[idx] on the device through ops.gather_rows: fp32 (n, C) rows, or an int64 (n,) vector moved as pairs of
    32-bit words."""
    idx = idx.to(device=t.device, dtype=torch.long).contiguous()
    t = t.contiguous()
    if t.dtype == torch.int64 and t.dim() == 1:
        out = torch.empty(idx.shape[0], dtype=torch.int64, device=t.device)
        ops.gather_rows(t.view(torch.float32).view(-1, 2), idx, out.view(torch.float32).view(-1, 2))
        return out
    if t.dtype != torch.float32 or t.dim() != 2:
        raise ValueError("coclr_amd: take_rows moves fp32 (n, C) rows or an int64 (n,) vector")
    out = torch.empty(idx.shape[0], t.shape[1], dtype=torch.float32, device=t.device)
    ops.gather_rows(t, idx, out)
    return out


# ---- files -----------------------------------------------------------------------------------------------------

def load_probs(path):
    """Reads a probability file of either script.  Returns (names: list in file order, probs: fp32 (V, C) host
    tensor).  The reference holds the JSON numbers in float64; they are fp32 values there, and anything that is
    not is refused here (it would not survive the way to the device)."""
    with open(path, "r") as fp:
        d = json.load(fp)
    names, rows = [], []
    for k, v in d.items():
        if isinstance(v, dict):
            v = v["mean_prob"]                                       # :81-82
        names.append(k)
        rows.append(np.asarray(v, dtype=np.float64).reshape(-1))
    if not rows or any(r.shape != rows[0].shape for r in rows):
        raise ValueError("coclr_amd: %s holds no videos or rows of different lengths" % path)
    p64 = torch.from_numpy(np.stack(rows))
    p32 = p64.float()
    if not torch.equal(p32.double(), p64):
        raise ValueError("coclr_amd: %s holds values that are not fp32 numbers" % path)
    return names, p32


def save_probs(path, names, probs, form="flat"):
    """Writes {name: row} as JSON.  form: 'flat' (a plain list), 'nested' (the (1, C) list
    feature_linear_probe.py:199-203 writes) or 'mean_prob' ({'mean_prob': (1, C) list}, main_classifier.py:535).
    The reference's merge_prob reads all three, as load_probs does."""
    if form not in ("flat", "nested", "mean_prob"):
        raise ValueError("coclr_amd: save_probs form is 'flat', 'nested' or 'mean_prob'")
    rows = probs.detach().to("cpu", torch.float32).tolist()
    if len(rows) != len(names):
        raise ValueError("coclr_amd: %d names for %d rows" % (len(names), len(rows)))
    wrap = {"flat": lambda r: r, "nested": lambda r: [r], "mean_prob": lambda r: {"mean_prob": [r]}}[form]
    with open(path, "w") as fp:
        json.dump({str(n): wrap(r) for n, r in zip(names, rows)}, fp)


def _feature_paths(directory, dataset, flow):
    prefix = os.path.join(directory, dataset + ("-f" if flow else ""))
    return {(split, kind): "%s_%s_%s" % (prefix, split, "vname.pkl" if kind == "vname" else kind + ".pth.tar")
            for split in ("train", "test") for kind in ("feature", "label", "vname")}


def load_features(directory, dataset, flow=False):
    """The cache `main_classifier.py --retrieval` leaves (:645-647, :681-683).  Returns a dict with
    {train,test}_{feature,label} as host tensors and {train,test}_vname as lists; `flow` reads stream 2's
    `<dataset>-f` files (:130-137)."""
    out = {}
    for (split, kind), path in _feature_paths(directory, dataset, flow).items():
        if kind == "vname":
            with open(path, "rb") as fp:
                out[split + "_vname"] = _names(pickle.load(fp)).tolist()
        else:
            out["%s_%s" % (split, kind)] = torch.load(path, map_location="cpu", weights_only=True)
    return out


def save_features(directory, dataset, train_feature, train_label, train_vname, test_feature, test_label, test_vname,
                  flow=False):
    """Writes what load_features reads (and the reference's merge_sim and feature_linear_probe.py)."""
    paths = _feature_paths(directory, dataset, flow)
    data = {"train": (train_feature, train_label, train_vname), "test": (test_feature, test_label, test_vname)}
    for split, (feature, label, vname) in data.items():
        torch.save(feature.detach().cpu(), paths[split, "feature"])
        torch.save(label.detach().cpu(), paths[split, "label"])
        with open(paths[split, "vname"], "wb") as fp:
            pickle.dump([str(v) for v in vname], fp)


# ---- command line ------------------------------------------------------------------------------------------------

def read_class_index(path):
    """ClassInd.txt as the reference's get_action_idx reads it (:45-57): one action per line, or `index,action`."""
    with open(path, "r") as fp:
        actions = [line.strip() for line in fp.readlines()]
    if "," in actions[0]:
        actions = [a.split(",")[-1] for a in actions]
    return actions


def labels_from_names(names, actions, dataset):
    """(:91-94) the action is the third-last path component of a video's name, the second-last for k400."""
    action_to_idx = dict(zip(actions, range(len(actions))))
    part = -2 if dataset == "k400" else -3
    return torch.tensor([action_to_idx[n.split("/")[part]] for n in names], dtype=torch.long)


def merge_prob(prob1, prob2, dataset, class_index, device="cuda"):
    """The reference's merge_prob on two files; returns the line it prints."""
    names, p1 = load_probs(prob1)
    names2, p2 = load_probs(prob2)
    at = {n: i for i, n in enumerate(names2)}
    p2 = p2[torch.tensor([at[n] for n in names], dtype=torch.long)]      # prob_dict2[k] for k of file 1 (:80-89)
    labels = labels_from_names(names, read_class_index(class_index), dataset)
    res = fuse_probs(p1.to(device), p2.contiguous().to(device), labels.to(device))
    return "merged accuracy: %.6f + %.6f => %.6f" % tuple(res.acc.tolist())


def merge_sim(dir1, dir2, dataset, device="cuda"):
    """The reference's merge_sim on two feature directories; returns the lines it prints."""
    s1, s2 = load_features(dir1, dataset), load_features(dir2, dataset, flow=True)
    rows = {}
    for split in ("train", "test"):
        i1, i2 = align_by_name(s1[split + "_vname"], s2[split + "_vname"])
        rows[split] = (take_rows(s1[split + "_feature"].float().to(device), i1),
                       take_rows(s2[split + "_feature"].float().to(device), i2),
                       take_rows(s1[split + "_label"].long().to(device), i1))       # labels are stream 1's (:122,128)
    ks = (1, 5, 10, 20, 50)
    acc, _, _ = nn_retrieval_two_stream(rows["test"][0], rows["train"][0], rows["test"][1], rows["train"][1],
                                        rows["test"][2], rows["train"][2], ks)
    return ["%dNN acc = %.4f" % (k, a) for k, a in zip(ks, acc.tolist())]


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--prob1', default='', type=str)
    parser.add_argument('--prob2', default='', type=str)
    parser.add_argument('--dataset', default='ucf101', type=str)
    parser.add_argument('--mode', default='c', type=str)
    parser.add_argument('--class-index', default='', type=str,
                        help="ClassInd.txt of the dataset (mode c); the reference hard-codes its authors' path")
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if args.mode == 'c':
        print('Merge classification probability')
        if not args.class_index:
            raise SystemExit("coclr_amd: --mode c needs --class-index PATH (the dataset's ClassInd.txt)")
        print(merge_prob(args.prob1, args.prob2, args.dataset, args.class_index))
    elif args.mode == 's':
        print('Merge similarity')
        for line in merge_sim(args.prob1, args.prob2, args.dataset):
            print(line)


if __name__ == '__main__':
    main()
