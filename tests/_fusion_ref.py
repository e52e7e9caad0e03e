"""Restatement in numpy / torch of what eval/merge_2stream_prob.py computes (merge_prob :80-98, the alignment
:118-170, merge_sim :178-196), for the tests of coclr_amd.eval.fusion.  tests/golden/eval_fusion.pt holds what the
reference itself made of the same inputs; tests/test_eval_fusion_cpu.py holds this file to it."""
import numpy as np
import torch
import torch.nn.functional as F

KS = (1, 5, 10, 20, 50)


def merge_prob(p1, p2, labels):
    """p1, p2 fp32 (V, C), labels int64 (V,).  Returns (fused float64 (V, C), argmax int32 (V, 3), hits fp32 (V, 3),
    acc: three floats).  np.argmax returns the first maximum."""
    a, b = p1.cpu().numpy().astype(np.float64), p2.cpu().numpy().astype(np.float64)
    fused = (a + b) / 2
    am = np.stack([np.argmax(a, axis=-1), np.argmax(b, axis=-1), np.argmax(fused, axis=-1)], 1)
    hits = (am == labels.cpu().numpy()[:, None])
    return (torch.from_numpy(fused), torch.from_numpy(am.astype(np.int32)), torch.from_numpy(hits.astype(np.float32)),
            [float(h) for h in hits.mean(0)])


def align(names1, names2):
    """Row indices into stream 1 and stream 2 after the sorting and dropping of :118-167; asserts as :169-170."""
    n1, n2 = np.array(names1), np.array(names2)
    s1, s2 = np.argsort(n1), np.argsort(n2)
    n1, n2 = n1[s1], n2[s2]
    if len(n1) < len(n2):
        keep = np.isin(n2, n1)
        n2, s2 = n2[keep], s2[keep]
    if len(n1) > len(n2):
        keep = np.isin(n1, n2)
        n1, s1 = n1[keep], s1[keep]
    assert n1.shape == n2.shape and np.all(n1 == n2)
    return torch.from_numpy(s1), torch.from_numpy(s2)


def preprocess(t):
    return F.normalize(t - t.mean(dim=0, keepdim=True), p=2, dim=1)


def merge_sim(inputs, ks=KS):
    """inputs: {'train': {...}, 'test': {...}} with names1/feature1/label1/names2/feature2 per split, as the
    fixture holds them.  Returns (sim, top-max(ks) indices, accuracies, aligned train labels, aligned test labels)."""
    rows = {}
    for split in ("train", "test"):
        d = inputs[split]
        i1, i2 = align(d["names1"], d["names2"])
        rows[split] = (d["feature1"][i1], d["feature2"][i2], d["label1"][i1])
    sim = preprocess(rows["test"][0]).matmul(preprocess(rows["train"][0]).t()) + \
        preprocess(rows["test"][1]).matmul(preprocess(rows["train"][1]).t())
    trl, tel = rows["train"][2], rows["test"][2]
    acc = []
    for k in ks:
        idx = torch.topk(sim, k, dim=1)[1]
        acc.append(torch.any(trl[idx] == tel.unsqueeze(1), dim=1).float().mean().item())
    return sim, torch.topk(sim, ks[-1], dim=1)[1], acc, trl, tel


def ordered_top(sim, k):
    """The k largest of every row in the order (value descending, column ascending): a stable descending sort."""
    return torch.sort(sim, dim=1, descending=True, stable=True)[1][:, :k]


def knn_hits(sim, train_label, test_label, ks):
    idx = ordered_top(sim, max(ks))
    return torch.stack([(train_label[idx[:, :k]] == test_label[:, None]).any(1).float() for k in ks], 1)


# ---- inputs of the exact fusion tests ----------------------------------------------------------------------------

FUSE_V = (1, 3, 5, 70)
FUSE_C = (1, 2, 51, 64, 65, 101, 257, 400)


def fuse_case(V, C, seed):
    """(p1, p2, labels) fp32 / int64 host tensors for one (V, C): random softmax rows, then -- where C allows --
    rows of dyadic values with a fused tie at columns (c, c+1), (c, c+63), (c, c+64), (0, C-1), and rows on which the
    three arg-maxima differ.  The special rows overwrite rows 0, 1, ... cyclically, so V = 1 sees the last one."""
    g = torch.Generator().manual_seed(seed)
    p1 = torch.softmax(3 * torch.randn(V, C, generator=g), 1)
    p2 = torch.softmax(3 * torch.randn(V, C, generator=g), 1)
    labels = torch.randint(0, C, (V,), generator=g)
    special = []
    for gap in (1, 63, 64, C - 1):
        if 0 < gap < C:
            c = 0 if gap == C - 1 else int(torch.randint(0, C - gap, (1,), generator=g))
            a = torch.full((C,), 1.0 / 1024)
            b = torch.full((C,), 1.0 / 1024)
            a[c], b[c] = 0.5, 0.25                      # fused 0.375 at c and at c + gap: the first one wins
            a[c + gap], b[c + gap] = 0.25, 0.5
            special.append((a, b, c))
    if C >= 3:
        x, y, z = torch.randperm(C, generator=g)[:3].tolist()
        a = torch.zeros(C)
        b = torch.zeros(C)
        a[x], a[y] = 0.4, 0.35                          # arg-maxima x, z and (fused 0.2, 0.35, 0.2) y
        b[z], b[y] = 0.4, 0.35
        special.append((a, b, y))
    for i, (a, b, lab) in enumerate(special):
        r = i % V
        p1[r], p2[r], labels[r] = a, b, lab
    return p1.contiguous(), p2.contiguous(), labels
