"""Inference launch plans (engine.PLAN_INFER): a gradient-free pass of a module that opted in is recorded once
and re-issued from its log.  Everything here is a bit-for-bit comparison with the interpreted pass -- the plan
re-issues the same kernels with the same operands, so there is no tolerance to choose."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CLIP = (3, 16, 64, 64)


def _backbone(network, seed=0):
    from coclr_amd import engine
    from coclr_amd.backbone.select_backbone import select_backbone
    torch.manual_seed(seed)
    net, _ = select_backbone(network)
    net = net.cuda().eval()
    _randomise_bn(net, seed + 1)
    return engine.enable_inference_plans(net)


def _randomise_bn(net, seed):
    """Running statistics and affine parameters away from (0, 1, 1, 0): the eval affine has something to fold."""
    g = torch.Generator().manual_seed(seed)
    for m in net.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)


def _inputs(n, batch=2, seed=10, clip=CLIP):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(batch, *clip, generator=g) for _ in range(n)]


def _passes(net, xs, planned, monkeypatch):
    from coclr_amd import engine
    monkeypatch.setattr(engine, "PLAN_INFER", planned)
    outs = []
    with torch.no_grad():
        for x in xs:
            outs.append(net(x.cuda() if not x.is_cuda else x).cpu())
    torch.cuda.synchronize()
    return outs


def _stats():
    from coclr_amd import engine
    s = engine.PLAN_STATS
    return s["infer_recorded"], s["infer_replayed"], len(s["disabled"])


@pytest.mark.parametrize("network", ["s3d", "s3dg", "r50"])
def test_replayed_passes_bit_identical(monkeypatch, network):
    from coclr_amd import engine
    assert engine.PLAN_INFER, "inference plans are switched off (COCLR_PLAN_INFER=0 or no private memory pools)"
    net = _backbone(network)
    xs = _inputs(engine._PLAN_WARMUP + 4)
    want = _passes(net, xs, False, monkeypatch)
    rec0, rep0, dis0 = _stats()
    got = _passes(net, xs, True, monkeypatch)
    rec1, rep1, dis1 = _stats()
    assert (rec1 - rec0, rep1 - rep0, dis1 - dis0) == (1, 3, 0), engine.PLAN_STATS
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), "pass %d differs from the interpreted pass" % i
    assert float(want[0].abs().max()) > 0


def test_moving_and_non_contiguous_input(monkeypatch):
    from coclr_amd import engine
    net = _backbone("s3d")
    n = engine._PLAN_WARMUP + 4
    xs = _inputs(n)
    # the test modes' input (eval/main_classifier.py:448): a permuted view, (3, n, T, H, W) -> (n, 3, T, H, W)
    g = torch.Generator().manual_seed(77)
    views = [torch.randn(3, 2, *CLIP[1:], generator=g).cuda().permute(1, 0, 2, 3, 4) for _ in range(2)]
    assert not views[0].is_contiguous()
    want = _passes(net, xs + views, False, monkeypatch)
    hold = [x.cuda() for x in xs]              # all alive at once: a different address on every call
    assert len({x.data_ptr() for x in hold}) == n
    rep0 = _stats()[1]
    got = _passes(net, hold + views, True, monkeypatch)
    assert _stats()[1] - rep0 == 3 + 2
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_batch_strided_and_contiguous_inputs_alternate(monkeypatch):
    """One shape, two sample strides: `block[:, 0]` of a (B, 2, 3, T, H, W) pair tensor is dense in (C, T, H, W)
    but its samples are two clips apart.  The sample stride is frozen into the logged calls, so it is part of
    the plan's key: each layout gets its own plan and neither is replayed with the other's stride."""
    from coclr_amd import engine
    net = _backbone("s3d")
    n = engine._PLAN_WARMUP + 3
    g = torch.Generator().manual_seed(55)
    pairs = [torch.randn(2, 2, *CLIP, generator=g).cuda() for _ in range(n)]
    xs = []
    for p in pairs:                                     # strided, contiguous, strided, ...
        xs += [p[:, 0], p[:, 1].contiguous()]
    assert engine._dense5(xs[0]) and not xs[0].is_contiguous() and xs[0].stride(0) == 2 * xs[1].stride(0)
    want = _passes(net, xs, False, monkeypatch)
    rec0, rep0, dis0 = _stats()
    got = _passes(net, xs, True, monkeypatch)
    rec1, rep1, dis1 = _stats()
    assert (rec1 - rec0, rep1 - rep0, dis1 - dis0) == (2, 2 * 2, 0)
    assert engine.inference_plan_pools(net) == 2
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), "pass %d (%s)" % (i, "strided" if i % 2 == 0 else "contiguous")
    # the same through ONE tensor's two halves at different addresses: the strided plan follows the pointer
    more = [pairs[0][:, 1], pairs[1][:, 1]]
    assert torch.equal(_passes(net, more, True, monkeypatch)[1], _passes(net, more, False, monkeypatch)[1])


def test_result_is_owned_by_the_caller(monkeypatch):
    from coclr_amd import engine
    net = _backbone("s3d")
    xs = _inputs(engine._PLAN_WARMUP + 4)
    monkeypatch.setattr(engine, "PLAN_INFER", True)
    with torch.no_grad():
        for x in xs[:-3]:
            net(x.cuda())                      # warm-up and recording
        held = net(xs[-3].cuda())              # a replay
        snap = held.clone()
        other = [net(x.cuda()) for x in xs[-2:]]
    torch.cuda.synchronize()
    assert torch.equal(held, snap)
    assert not torch.equal(other[0], held) and held.data_ptr() not in {o.data_ptr() for o in other}


def test_in_place_parameter_change_is_picked_up(monkeypatch):
    from coclr_amd import engine
    net = _backbone("s3d")
    xs = _inputs(engine._PLAN_WARMUP + 3)
    _passes(net, xs, True, monkeypatch)        # recorded and replayed twice
    ptrs = [p.data_ptr() for p in net.parameters()]
    torch.manual_seed(5)
    donor, _ = __import__("coclr_amd.backbone.select_backbone", fromlist=["x"]).select_backbone("s3d")
    _randomise_bn(donor, 99)
    net.load_state_dict(donor.state_dict())    # other values, the same storages
    assert ptrs == [p.data_ptr() for p in net.parameters()]
    x = _inputs(1, seed=123)
    rec0, rep0, _ = _stats()
    got = _passes(net, x, True, monkeypatch)
    rec1, rep1, _ = _stats()
    assert (rec1 - rec0, rep1 - rep0) == (0, 1)
    want = _passes(net, x, False, monkeypatch)
    assert torch.equal(got[0], want[0])
    old = _passes(_backbone("s3d"), x, False, monkeypatch)
    assert not torch.equal(old[0], want[0])    # the new values do change the result


class _Clips(torch.utils.data.Dataset):
    def __init__(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        self.frames = torch.rand(n, 3, 8, 64, 64, generator=g)
        self.label = torch.randint(0, 101, (n,), generator=g)

    def __len__(self):
        return self.label.shape[0]

    def __getitem__(self, i):
        return self.frames[i], self.label[i]


@pytest.mark.parametrize("train_what", ["last", "ft"])
def test_classifier_loop_with_train_eval_toggling(monkeypatch, train_what):
    """Two epochs of training + validation: 8 training and 8 validation batches, so the differentiated plan
    ('ft') and the inference plan (validation; every pass of 'last') both get past warm-up and recording."""
    import model.classifier as product
    import _classifier_loop
    from coclr_amd import engine
    from oracle import coclr_oracle as orc

    def run(planned):
        monkeypatch.setattr(engine, "PLAN_INFER", planned)
        before = dict(engine.PLAN_STATS, disabled=len(engine.PLAN_STATS["disabled"]))
        rec = _classifier_loop.run_classifier(product, _Clips(16, 41), _Clips(16, 42), train_what=train_what,
                                              optim="sgd", batch_size=4, seq_len=8, img_dim=64, gpu=0,
                                              calc_topk_accuracy=orc.calc_topk_accuracy, epochs=2, validate=True)
        torch.cuda.synchronize()
        after = dict(engine.PLAN_STATS, disabled=len(engine.PLAN_STATS["disabled"]))
        return rec, {k: after[k] - before[k] for k in after}

    off, d_off = run(False)
    on, d_on = run(True)
    assert d_off["infer_recorded"] == 0 and d_off["infer_replayed"] == 0
    assert d_on["infer_recorded"] == 1 and d_on["disabled"] == 0
    assert d_on["infer_replayed"] == (8 if train_what == "ft" else 16) - engine._PLAN_WARMUP - 1
    assert (d_on["recorded"], d_on["replayed"]) == (d_off["recorded"], d_off["replayed"])
    if train_what == "ft":
        assert d_on["recorded"] >= 1 and d_on["replayed"] >= 1
    assert len(on["outputs"]) == 8 and len(on["val_outputs"]) == 8
    for key in ("outputs", "val_outputs"):
        for i, (a, b) in enumerate(zip(on[key], off[key])):
            assert torch.equal(a, b), "%s[%d]" % (key, i)
    assert on["losses"] == off["losses"] and on["val_losses"] == off["val_losses"]


def test_shape_cap_and_release(monkeypatch):
    from coclr_amd import engine
    net = _backbone("s3d")
    cap = engine._INFER_MAX_SHAPES
    clips = [(3, 16, 64, 64), (3, 8, 64, 64), (3, 16, 128, 128), (3, 8, 128, 128), (3, 32, 64, 64)][:cap + 2]
    n = engine._PLAN_WARMUP + 2
    per_shape = [_inputs(n, seed=20 + i, clip=c) for i, c in enumerate(clips)]
    want = [_passes(net, xs, False, monkeypatch) for xs in per_shape]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    reserved0 = torch.cuda.memory_reserved()
    rec0, rep0, _ = _stats()
    for xs, ws in zip(per_shape, want):
        got = _passes(net, xs, True, monkeypatch)
        assert engine.inference_plan_pools(net) <= cap
        for a, b in zip(got, ws):
            assert torch.equal(a, b)
    rec1, rep1, _ = _stats()
    assert engine.inference_plan_pools(net) == cap
    assert (rec1 - rec0, rep1 - rep0) == (cap, cap)         # the shapes past the cap ran interpreted
    engine.release_inference_plans(net)
    assert engine.inference_plan_pools(net) == 0
    del got
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    one_batch = 2 * 3 * 16 * 128 * 128 * 4
    assert torch.cuda.memory_reserved() <= reserved0 + one_batch, (torch.cuda.memory_reserved(), reserved0)


def test_unmarked_module_records_nothing(monkeypatch):
    """The pretraining models did not opt in: an InfoNCE key encoder without its hipGraph (COCLR_GRAPHS=0)
    runs interpreted, and so does a bare backbone nobody marked."""
    import coclr_amd.model.pretrain as P
    from coclr_amd import engine
    from coclr_amd.backbone.select_backbone import select_backbone
    monkeypatch.setattr(engine, "PLAN_INFER", True)
    monkeypatch.setattr(P, "_GRAPHS", False)
    before = _stats()
    torch.manual_seed(0)
    model = P.InfoNCE('s3d', 128, 32, 0.999, 0.07).cuda().train()
    g = torch.Generator().manual_seed(3)
    for _ in range(engine._PLAN_WARMUP + 3):
        model(torch.randn(4, 2, 3, 16, 64, 64, generator=g).cuda())
    net, _ = select_backbone("s3d")
    net = net.cuda().eval()
    with torch.no_grad():
        for x in _inputs(engine._PLAN_WARMUP + 3):
            net(x.cuda())
    torch.cuda.synchronize()
    assert _stats() == before
    assert engine._INFER_STORE not in model.encoder_k[0].__dict__ and engine._INFER_STORE not in net.__dict__
