"""Video-level scores on the GPU: the two segmented-accumulate kernels (csrc/retrieval.hip) against float64
torch on the CPU, and coclr_amd.eval.video.VideoEvaluator end to end on S3D against the CPU oracle restating
eval/main_classifier.py:482-494,533 (multi-crop probabilities) and :624-640 (retrieval features).  The kernels' exact
suite is tests/test_gpu_segment_exact.py; the last tests here run the evaluator's own bookkeeping on a table model: its
tables growing past 64 videos, passes of more than 64 segments, a crop cut into several batches, batches of one clip,
and a second use after finish().

Bars: 1e-6 relative for the kernels -- elementwise fp32 formulas, the bar of the loss epilogue
(tests/test_gpu_next.py) -- and the project's standing 1e-3 for anything that went through the backbone."""
import pytest
import torch
import torch.nn.functional as F

from _cases import check_close, rel_err
from oracle import coclr_oracle as orc

pytestmark = pytest.mark.gpu

LENGTHS = [1, 5, 9, 2, 11, 8, 3, 1, 12, 12]          # 64 rows: two calls of 32, video 5 is cut by the boundary


def _segments(lengths, rows_per_call):
    """[(call, first row, rows, video)] of consecutive videos packed into calls of `rows_per_call` rows."""
    out, pos = [], 0
    for v, n in enumerate(lengths):
        left = n
        while left:
            call, first = divmod(pos, rows_per_call)
            k = min(left, rows_per_call - first)
            out.append((call, first, k, v))
            pos += k
            left -= k
    return out


@pytest.mark.parametrize("C_", [51, 101, 400, 1024])
def test_segment_kernels_match_float64(C_):
    from coclr_amd import ops
    g = torch.Generator().manual_seed(C_)
    V, R = len(LENGTHS), 32
    crops = [torch.randn(sum(LENGTHS), C_, generator=g) * 3 for _ in range(2)]
    segs = _segments(LENGTHS, R)
    assert any(n == 1 for n in LENGTHS) and len(segs) == V + 1 and max(c for c, _, _, _ in segs) == 1
    want_p = torch.zeros(V, C_, dtype=torch.float64)
    want_s = torch.zeros(V, C_, dtype=torch.float64)
    pos = 0
    for v, n in enumerate(LENGTHS):
        for x in crops:
            want_p[v] += F.softmax(x[pos:pos + n].double(), dim=-1).mean(0)       # :488, summed over crops
            want_s[v] += x[pos:pos + n].double().mean(0)                          # :637
        pos += n
    got_p = torch.zeros(V, C_, device="cuda")
    got_s = torch.zeros(V, C_, device="cuda")
    for x in crops:                                   # the second crop accumulates into the same rows
        for call in (0, 1):
            xs = x[call * R:(call + 1) * R].cuda()
            sg = [(first, k, v) for c, first, k, v in segs if c == call]
            w = [1.0 / LENGTHS[v] for _, _, v in sg]
            ops.segment_softmax_accum(xs, sg, w, got_p)
            ops.segment_accum(xs, sg, w, got_s)
    torch.cuda.synchronize()
    check_close(got_p, want_p, 1e-6, "segment softmax accumulate C=%d" % C_)
    check_close(got_s, want_s, 1e-6, "segment accumulate C=%d" % C_)
    # run-to-run identical, and two segments of ONE call may name the same output row (two crops of a video in
    # one batch): applied in order
    again = torch.zeros(V, C_, device="cuda")
    for x in crops:
        for call in (0, 1):
            sg = [(first, k, v) for c, first, k, v in segs if c == call]
            ops.segment_softmax_accum(x[call * R:(call + 1) * R].cuda(), sg, [1.0 / LENGTHS[v] for _, _, v in sg],
                                      again)
    assert torch.equal(again, got_p)
    x = crops[0][:7].cuda()
    dup = torch.zeros(2, C_, device="cuda")
    ops.segment_softmax_accum(x, [(0, 3, 0), (3, 3, 0), (6, 1, 1)], [1 / 3, 1 / 3, 1.0], dup)
    ref = torch.stack([F.softmax(crops[0][0:3].double(), -1).mean(0) + F.softmax(crops[0][3:6].double(), -1).mean(0),
                       F.softmax(crops[0][6:7].double(), -1).mean(0)])
    check_close(dup, ref, 1e-6, "two segments into one row")


def test_segment_kernels_reject_bad_segments():
    from coclr_amd import _lib, ops
    x = torch.zeros(8, 101, device="cuda")
    out = torch.full((4, 101), 7.0, device="cuda")
    for segs in ([(0, 0, 0)], [(0, 4, 0), (6, 3, 1)], [(-1, 2, 0)], [(0, 2, 4)]):
        for fn in (ops.segment_softmax_accum, ops.segment_accum):
            with pytest.raises(_lib.HipLibraryError):
                fn(x, segs, [1.0] * len(segs), out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                  # nothing was launched


class _TableModel(torch.nn.Module):
    """Stands in for the classifier: clip i (its index is written into the clip) -> row i of fixed tables."""

    def __init__(self, logits, feats):
        super().__init__()
        self.logits = torch.nn.Parameter(logits, requires_grad=False)
        self.feats = torch.nn.Parameter(feats, requires_grad=False)

    def forward(self, block):
        idx = block[:, 0, 0, 0, 0].long()
        return self.logits[idx], self.feats[idx]


def _gapped_logits(n_rows, C_, lengths, crops):
    """randn * 3 logits, from the first seed whose float64 video-level mean probabilities keep ranks 1/2 and 5/6
    more than 1e-4 apart in EVERY row (fp32 rounding cannot reorder them then)."""
    for seed in range(1000):
        g = torch.Generator().manual_seed(seed)
        logits = torch.randn(crops, n_rows, C_, generator=g) * 3
        mean, pos = [], 0
        for n in lengths:
            mean.append(F.softmax(logits[:, pos:pos + n].double(), -1).mean(1).mean(0))
            pos += n
        mean = torch.stack(mean)
        top = mean.topk(6, 1).values
        if float((top[:, 0] - top[:, 1]).min()) > 1e-4 and float((top[:, 4] - top[:, 5]).min()) > 1e-4:
            return logits, mean
    raise AssertionError("no seed keeps every row's ranks apart")


@pytest.mark.parametrize("C_", [51, 101, 400, 1024])
def test_topk_of_finish_equals_the_float64_ranking(C_):
    from coclr_amd.eval.video import VideoEvaluator
    lengths, crops = LENGTHS, 2
    n_rows = sum(lengths)
    logits, mean = _gapped_logits(n_rows, C_, lengths, crops)
    top = mean.topk(6, 1).values
    assert float((top[:, 0] - top[:, 1]).min()) > 1e-4 and float((top[:, 4] - top[:, 5]).min()) > 1e-4
    g = torch.Generator().manual_seed(1)
    # labels: a mix of rank-1, rank-3 and rank-9 classes, so neither accuracy is trivially 0 or 1
    order = mean.argsort(1, descending=True)
    labels = torch.stack([order[v, (0, 2, 8)[v % 3]] for v in range(len(lengths))])
    feats = torch.randn(crops * n_rows, 8, generator=g)
    model = _TableModel(logits.reshape(crops * n_rows, C_), feats).cuda().eval()
    ev = VideoEvaluator(model, batch_clips=32)
    for c in range(crops):
        pos = 0
        for v, n in enumerate(lengths):
            clips = torch.zeros(n, 3, 1, 1, 1)
            clips[:, 0, 0, 0, 0] = torch.arange(c * n_rows + pos, c * n_rows + pos + n, dtype=torch.float32)
            ev.add(clips.cuda(), label=int(labels[v]), video=None if c == 0 else v)
            pos += n
    res = ev.finish()
    check_close(res.probs, mean, 1e-6, "video-level mean probabilities")
    want1, want5 = orc.calc_topk_accuracy(mean, labels, (1, 5))
    assert 0 < float(want1) < float(want5) < 1
    V = len(lengths)                                  # accuracies are hit counts / V: the counts are equal
    assert round(float(res.top1) * V) == round(float(want1) * V) == 4
    assert round(float(res.top5) * V) == round(float(want5) * V) == 7
    assert abs(float(res.top1) - float(want1)) < 1e-6 and abs(float(res.top5) - float(want5)) < 1e-6
    assert res.labels.cpu().tolist() == labels.tolist()


E2E_LENGTHS = [1, 2, 3, 11, 4, 1, 5, 2, 7, 3, 1, 6]
E2E_CLIP = (3, 8, 64, 64)


def _e2e_reference(num_class=51, crops=2):
    """Everything the end-to-end test needs from the CPU: the model, the videos and the reference's loops
    (:482-494,533 and :624-640) through orc.linear_classifier_forward, per video and crop.
    final_fc is re-drawn so the oracle's logits spread (std >= 1): a softmax over near-equal logits is uniform
    whatever the model computes.  Its scale comes from the ORACLE's feature norms, and the draw is the first seed
    for which the oracle's video-level probabilities keep ranks 1/2 and 5/6 further apart, in every row, than
    twice the 1e-3 bound the product's probabilities are held to -- the ranking is then decided."""
    from coclr_amd.model.classifier import LinearClassifier
    torch.manual_seed(0)
    model = LinearClassifier(num_class=num_class, network='s3d').eval()
    g = torch.Generator().manual_seed(4)
    videos = [[torch.randn(n, *E2E_CLIP, generator=g) * (0.8 + 0.05 * v) + 0.1 * (v % 4) for _ in range(crops)]
              for v, n in enumerate(E2E_LENGTHS)]
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        feats = [[orc.linear_classifier_forward(sd, 's3d', clips, False)[1] for clips in vc] for vc in videos]
        norm = float(torch.cat([f for vf in feats for f in vf]).norm(dim=1).mean())
        for seed in range(200):
            gw = torch.Generator().manual_seed(100 + seed)
            sd["final_fc.1.weight"] = torch.randn(num_class, feats[0][0].shape[1], generator=gw) * (3.0 / norm)
            sd["final_fc.1.bias"] = torch.randn(num_class, generator=gw) * 0.1
            # (the last line of orc.linear_classifier_forward on the features it returned above)
            logits = [[F.linear(f, sd["final_fc.1.weight"], sd["final_fc.1.bias"]) for f in vf] for vf in feats]
            ref_prob = torch.stack([torch.stack([F.softmax(l.double(), dim=-1).mean(0, keepdim=True) for l in vl],
                                                0).mean(0)[0] for vl in logits])
            top = ref_prob.topk(6, 1).values
            if float(((top[:, 0] - top[:, 1]) / top[:, 0]).min()) > 2e-3 and \
                    float(((top[:, 4] - top[:, 5]) / top[:, 0]).min()) > 2e-3:
                break
        else:
            raise AssertionError("no draw of final_fc keeps the oracle's ranks apart")
        # the oracle itself on the final weights, for one video: the shortcut above is its own last line
        chk, _ = orc.linear_classifier_forward(sd, 's3d', videos[3][0], False)
        assert torch.equal(chk, logits[3][0])
        model.final_fc[1].weight.copy_(sd["final_fc.1.weight"])
        model.final_fc[1].bias.copy_(sd["final_fc.1.bias"])
    # labels: a mix of the oracle's rank-1, rank-3 and rank-9 classes, so neither accuracy is trivially 0 or 1
    order = ref_prob.argsort(1, descending=True)
    labels = [int(order[v, (0, 2, 8)[v % 3]]) for v in range(len(videos))]
    ref_feat = torch.stack([torch.stack([f.double().mean(0) for f in vf], 0).mean(0) for vf in feats])
    ref_logits = torch.cat([logits[v][c] for c in range(crops) for v in range(len(videos))])
    return model, videos, labels, ref_logits, ref_prob, ref_feat


def test_video_evaluator_end_to_end_on_s3d():
    from coclr_amd import engine
    from coclr_amd.eval.retrieval import nn_retrieval
    from coclr_amd.eval.video import VideoEvaluator
    crops = 2
    model, videos, labels, ref_logits, ref_prob, ref_feat = _e2e_reference(crops=crops)
    print("oracle logits: std over classes %.3f" % float(ref_logits.std(dim=1).mean()))
    assert float(ref_logits.std(dim=1).min()) >= 1.0
    top = ref_prob.topk(6, 1).values
    assert float(((top[:, 0] - top[:, 1]) / top[:, 0]).min()) > 2e-3
    assert float(((top[:, 4] - top[:, 5]) / top[:, 0]).min()) > 2e-3

    model = model.cuda()
    seen = []
    inner = model.forward

    def observed(block):
        out = inner(block)
        seen.append((out[0].clone(), out[1].clone()))
        return out
    model.forward = observed
    rec0 = engine.PLAN_STATS["infer_recorded"]
    ev = VideoEvaluator(model, batch_clips=8)
    for c in range(crops):
        for v, vc in enumerate(videos):
            ev.add(vc[c].cuda(), label=labels[v], video=None if c == 0 else v)
    res = ev.finish()
    torch.cuda.synchronize()
    total = crops * sum(E2E_LENGTHS)
    assert ev.passes == -(-total // 8) == len(seen)
    got_logits = torch.cat([l for l, _ in seen])[:total].cpu()          # rows in the order they were added
    e_logit = float((got_logits.double() - ref_logits.double()).abs().max() / ref_logits.abs().max())
    e_feat = float((res.features.cpu().double() - ref_feat).abs().max() / ref_feat.abs().max())
    e_prob = float(((res.probs.cpu().double() - ref_prob).abs().max(1).values / ref_prob.max(1).values).max())
    print("end to end: logits %.2e, features %.2e, probabilities (relative to each row's largest) %.2e"
          % (e_logit, e_feat, e_prob))
    assert e_logit <= 1e-3 and e_feat <= 1e-3 and e_prob <= 1e-3
    assert engine.PLAN_STATS["infer_recorded"] - rec0 == 1 and engine.inference_plan_pools(model.backbone) == 1
    assert engine.PLAN_STATS["infer_replayed"] >= ev.passes - engine._PLAN_WARMUP - 1 > 0
    # accuracies of the scores against the oracle's ranking, and the features through retrieval
    lab = torch.tensor(labels)
    want1, want5 = orc.calc_topk_accuracy(ref_prob, lab, (1, 5))
    assert 0 < float(want1) < float(want5) < 1
    V = len(videos)                                    # accuracies are hit counts / V: the counts are equal
    assert round(float(res.top1) * V) == round(float(want1) * V)
    assert round(float(res.top5) * V) == round(float(want5) * V)
    ntr = 8
    rl = torch.tensor([v % 3 for v in range(V)])       # retrieval labels: three classes over the twelve videos
    acc, _, _ = nn_retrieval(res.features[ntr:], rl[ntr:].cuda(), res.features[:ntr], rl[:ntr].cuda(), ks=(1, 5))
    want_acc, _ = orc.nn_retrieval(ref_feat[ntr:].float(), rl[ntr:], ref_feat[:ntr].float(), rl[:ntr], ks=(1, 5))
    assert [round(float(a), 5) for a in acc] == [round(a, 5) for a in want_acc]


# ---- the evaluator's tables and batching on the table model (a model pass costs nothing) ----------------------------------

def _table_run(lengths, crops, batch_clips, order="crop-major", C_=51, width=24, seed=0, ev=None):
    """`lengths[v]` clips per crop of video v through a VideoEvaluator on a _TableModel; `order`: every video's first crop,
    then every video's second ("crop-major"), or all crops of a video before the next video ("video-major").
    Returns (VideoScores, float64 probabilities, float64 features, labels, the evaluator): the references are the
    per-video loops of eval/main_classifier.py:482-494,533 and :624-640."""
    from coclr_amd.eval.video import VideoEvaluator
    g = torch.Generator().manual_seed(seed)
    n_rows = sum(lengths)
    logits = torch.randn(crops, n_rows, C_, generator=g) * 3
    feats = torch.randn(crops, n_rows, width, generator=g)
    labels = [int(v) for v in torch.randint(0, C_, (len(lengths),), generator=g)]
    want_p, want_f, pos = [], [], 0
    for n in lengths:
        want_p.append(F.softmax(logits[:, pos:pos + n].double(), -1).mean(1).mean(0))
        want_f.append(feats[:, pos:pos + n].double().mean(1).mean(0))
        pos += n
    if ev is None:
        model = _TableModel(logits.reshape(crops * n_rows, C_), feats.reshape(crops * n_rows, width)).cuda().eval()
        ev = VideoEvaluator(model, batch_clips=batch_clips)
    else:
        assert ev.model.logits.shape == (crops * n_rows, C_)
        ev.model.logits.copy_(logits.reshape(crops * n_rows, C_))
        ev.model.feats.copy_(feats.reshape(crops * n_rows, width))
    starts = [sum(lengths[:v]) for v in range(len(lengths))]

    def add(v, c):
        clips = torch.zeros(lengths[v], 3, 1, 1, 1)
        first = c * n_rows + starts[v]
        clips[:, 0, 0, 0, 0] = torch.arange(first, first + lengths[v], dtype=torch.float32)
        got = ev.add(clips.cuda(), label=labels[v], video=None if c == 0 else v)
        assert got == v
    if order == "crop-major":
        for c in range(crops):
            for v in range(len(lengths)):
                add(v, c)
    else:
        for v in range(len(lengths)):
            for c in range(crops):
                add(v, c)
    res = ev.finish()
    torch.cuda.synchronize()
    return res, torch.stack(want_p), torch.stack(want_f), labels, ev


def _held_to_the_bar(res, want_p, want_f, labels, what):
    """1e-6 of the largest reference element, probabilities and features; equal labels.  Printed besides: the worst
    video's error against its OWN largest probability (a dropped or doubled segment is wrong by the order of that)."""
    ep = (res.probs.cpu().double() - want_p).abs().max(1).values / want_p.abs().max(1).values
    print("%s: probabilities %.2e and features %.2e of the largest reference element; worst video %d, %.2e of its own "
          "largest probability" % (what, rel_err(res.probs, want_p), rel_err(res.features, want_f), int(ep.argmax()),
                                   float(ep.max())))
    check_close(res.probs, want_p, 1e-6, what + ": probabilities")
    check_close(res.features, want_f, 1e-6, what + ": features")
    assert res.labels.cpu().tolist() == labels


@pytest.mark.parametrize("order", ["crop-major", "video-major"])
def test_tables_grow_while_sums_are_live(monkeypatch, order):
    """150 videos: the tables start at 64 rows and are copied to 130 or more when the 65th video has been added, with
    the sums of the videos before it in them (video-major, a second time past 130 videos)."""
    from coclr_amd import ops
    g = torch.Generator().manual_seed(5)
    lengths = [int(n) for n in torch.randint(1, 4, (150,), generator=g)]
    assert set(lengths) == {1, 2, 3}
    caps = []
    inner = ops.segment_softmax_accum

    def watched(x, segs, w, out):
        caps.append((out.shape[0], max(o for _, _, o in segs)))
        inner(x, segs, w, out)
    monkeypatch.setattr(ops, "segment_softmax_accum", watched)
    res, want_p, want_f, labels, ev = _table_run(lengths, 2, 32, order)
    assert ev.passes == -(-2 * sum(lengths) // 32) == len(caps)
    sizes = [c for c, _ in caps]
    assert sizes[0] == 64 and sizes == sorted(sizes) and len(set(sizes)) >= 2
    grown = sorted(set(sizes))[1]
    assert grown >= 130 and sizes.index(grown) >= 2          # passes before the copy left sums in the 64-row tables
    assert all(top < cap for cap, top in caps)
    assert res.probs.shape == (150, 51) and res.features.shape == (150, 24)
    _held_to_the_bar(res, want_p, want_f, labels, "150 videos, %s" % order)
    check_close(res.probs[:64], want_p[:64], 1e-6, "the first 64 videos")


def test_more_segments_than_one_launch_takes(monkeypatch):
    from coclr_amd import ops
    seen = []
    inner = ops.segment_softmax_accum
    monkeypatch.setattr(ops, "segment_softmax_accum",
                        lambda x, segs, w, out: (seen.append(len(segs)), inner(x, segs, w, out))[1])
    res, want_p, want_f, labels, ev = _table_run([1] * 100, 2, 80)
    assert seen == [80, 80, 40] and max(seen) > 64          # 80 segments: a launch of 64 and one of 16
    _held_to_the_bar(res, want_p, want_f, labels, "80 one-clip videos per pass")
    # video-major, both crops of a video lie next to each other in one pass: the same output row twice, 40 times, in a
    # pass of more than 64 segments
    seen.clear()
    res, want_p, want_f, labels, ev = _table_run([1] * 100, 2, 80, "video-major", seed=1)
    assert seen == [80, 80, 40]
    _held_to_the_bar(res, want_p, want_f, labels, "80 one-clip crops per pass, both crops of a video adjacent")


def test_a_crop_cut_into_three_batches(monkeypatch):
    from coclr_amd import ops
    seen = []
    inner = ops.segment_accum
    monkeypatch.setattr(ops, "segment_accum",
                        lambda x, segs, w, out: (seen.append((list(segs), list(w))), inner(x, segs, w, out))[1])
    lengths = [2, 3, 20, 1, 2]
    res, want_p, want_f, labels, ev = _table_run(lengths, 2, 8)
    pieces = [n for segs, _ in seen for _, n, v in segs if v == 2]
    assert pieces[:4] == [3, 8, 8, 1] and sum(pieces) == 40          # the first crop: four pieces, two of them whole batches
    assert all(w == 1.0 / lengths[v] for segs, ws in seen for (_, _, v), w in zip(segs, ws))
    _held_to_the_bar(res, want_p, want_f, labels, "a crop of 20 clips in batches of 8")


def test_batches_of_one_clip():
    res, want_p, want_f, labels, ev = _table_run([1, 3, 2, 5], 2, 1)
    assert ev.passes == 22
    _held_to_the_bar(res, want_p, want_f, labels, "batch_clips = 1")


def test_an_evaluator_is_reusable_after_finish():
    first = [3, 1, 7, 2, 9, 1]
    second = [2, 11, 1, 4, 5]                           # another number of videos, the same number of clips
    assert sum(first) == sum(second) and len(first) != len(second)
    res1, want_p, want_f, labels, ev = _table_run(first, 2, 8, seed=2)
    _held_to_the_bar(res1, want_p, want_f, labels, "first use")
    assert len(ev) == 0
    res2, want_p, want_f, labels, ev = _table_run(second, 2, 8, seed=3, ev=ev)
    _held_to_the_bar(res2, want_p, want_f, labels, "second use")
    fresh, _, _, _, _ = _table_run(second, 2, 8, seed=3)
    assert torch.equal(res2.probs, fresh.probs) and torch.equal(res2.features, fresh.features)
    assert torch.equal(res2.labels, fresh.labels)
    assert float(res2.top1) == float(fresh.top1) and float(res2.top5) == float(fresh.top5)
    assert res2.probs.shape[0] == len(second) != res1.probs.shape[0]
