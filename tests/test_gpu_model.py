"""End-to-end parity on the MI355X: the product classes (model.pretrain.* on the HIP
kernel library) replay the recorded reference runs in tests/golden/ -- same seeds,
same inputs, two optimisation steps.

Step 1 (identical weights on both sides): logits, loss, labels/masks, queue columns,
queue pointer, BatchNorm running statistics and the Adam-updated parameters must agree
within BASELINE.json's 1e-3 relative tolerance; gradients are checked against a float64
evaluation with a conditioning-aware bound (see _cases.compare_step).
Step 2 starts from weights that already went through Adam (update ~ lr*sign(g): any
round-off-level gradient difference becomes a +-2e-3 weight difference, so even two
builds of the reference diverge there).  It is therefore checked against the CPU oracle
continued from the PRODUCT's post-step-1 state: logits / loss / queue / BN statistics at
1e-3 again, plus the fixture's exact fields (queue pointer, labels)."""
import os

import pytest
import torch

from _cases import (assert_checksums, build_model, case_inputs, compare_state, compare_step,
                    fp64_truth_grads, load_golden, loss_fn, recorded_truth)

pytestmark = pytest.mark.gpu


def _ensure_pg():
    import torch.distributed as dist
    if not dist.is_initialized():
        import os
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29611")
        dist.init_process_group("nccl", rank=0, world_size=1)


def _replay(name, with_pg=False):
    import model.pretrain as product
    gold = load_golden(name)
    cfg = gold["cfg"]
    kind = cfg["kind"]
    if with_pg:
        _ensure_pg()
    model = build_model(cfg, product)
    # identical initial weights as the reference from the same seed
    sd = model.state_dict()
    keys = gold["init_checksums"]["keys"]
    from _cases import checksum_table
    assert_checksums(checksum_table(sd, keys), gold["init_checksums"]["vals"])
    model = model.cuda()
    params = [{"params": p} for _, p in model.named_parameters()]
    opt = torch.optim.Adam(params, lr=1e-3, weight_decay=1e-5)
    model.train()
    if kind == "coclr":
        model.sampler.eval()
    from oracle import coclr_oracle as orc
    from _cases import check_close
    for step, rec in enumerate(gold["steps"]):
        blocks, extra = case_inputs(cfg, step)
        before = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        truth = None
        if step == 0:
            truth = recorded_truth(rec) or fp64_truth_grads(cfg, rec, before, blocks, extra)
        torch.manual_seed(cfg["perm_seed"] + step)
        if kind == "infonce":
            out, tgt = model(blocks[0].cuda())
        elif kind == "ubernce":
            out, tgt = model(blocks[0].cuda(), extra.cuda())
        else:
            out, tgt = model(blocks[0].cuda(), blocks[1].cuda(), extra.cuda())
        loss = loss_fn(kind, out, tgt)
        opt.zero_grad()
        loss.backward()
        grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
        after = model.state_dict()
        if step == 0:
            report = []
            strict = "grads64" in rec
            compare_step(rec, kind, out, tgt, loss, grads, truth=truth, report=report, strict=strict,
                         grad_factor=2.0 if strict else 4.0)
            for k, e_got, e_ref in report:
                print("%s grad %-50s err vs fp64 %.2e (reference fp32: %.2e)" % (name, k, e_got,
                                                                               e_ref))
            compare_state(rec, after, cfg["B"], cfg["K"])
        else:
            # oracle continued from the product's own pre-step state
            sd = orc.training_state(before)
            pb = [blocks[0]] if kind != "coclr" else [(blocks[0], blocks[1])]
            (o_out, o_tgt), = orc.nce_step(sd, kind, cfg["network"], pb, [extra], cfg["dim"],
                                           cfg["K"], cfg["m"], cfg["T"], rec["perm"],
                                           topk=cfg.get("topk", 5),
                                           reverse=cfg.get("reverse", False))
            check_close(out, o_out, 1e-3, "step %d logits vs oracle" % step)
            assert torch.equal(tgt.cpu(), o_tgt), "step %d target" % step
            # loss ~ 5e-3: relative loss error = absolute logit-gap error (14x the logits'
            # max-relative error), so 1e-3 on logits bounds it at ~1.4e-2
            check_close(loss, loss_fn(kind, o_out, o_tgt), 5e-3, "step %d loss" % step)
            assert int(after["queue_ptr"]) == int(sd["queue_ptr"]) == int(rec["queue_ptr"])
            for k, v in sd.items():
                if ".block" in k:
                    continue        # alias keys of the S3D stages: the oracle updates the named ones
                if k.startswith("queue") or k.endswith(("running_mean", "running_var")):
                    if v.is_floating_point():
                        check_close(after[k], v, 1e-3, "step %d %s" % (step, k))
                    else:
                        assert torch.equal(after[k].cpu(), v), k
                if k.startswith("encoder_k.") and (k.endswith("4.bias") or k.endswith("conv1.weight")):
                    check_close(after[k], v, 1e-5, "momentum-updated " + k)
        opt.step()


@pytest.mark.parametrize("name", ["infonce_s3d_small", "ubernce_s3d_small", "coclr_s3d_small",
                                  "coclr_s3d_small_reverse_cold", "infonce_s3dg_small"])
def test_small_cases_match_reference(name):
    _replay(name)


def test_conditioned_case_every_gradient_tensor():
    """De-saturated, He-initialised fixture (loss ~ 4.9 instead of ~5e-3) with float64 gradients
    recorded from the REFERENCE model itself run in double: every one of the 26 sampled tensors --
    stem to head -- is held, in the L2 norm, to 2x the reference arithmetic's own raw fp32-vs-float64
    error (see _cases.compare_step, strict; the decision-conditioned form is test_gpu_gradients.py)."""
    _replay("infonce_s3d_conditioned")


def test_r50_matches_reference():
    _replay("infonce_r50_small")


def test_config1_matches_reference():
    """BASELINE.json configs[0]: S3D InfoNCE K=2048 B=4 on 3x32x128x128 clips."""
    _replay("infonce_s3d_config1")


def test_single_rank_process_group_path():
    """Same numbers when a 1-rank RCCL process group is initialised (the way
    main_nce.py runs it on one GPU)."""
    _replay("infonce_s3d_small", with_pg=True)


def test_no_grad_forward_leaves_state_untouched():
    import model.pretrain as product
    gold = load_golden("infonce_s3d_small")
    cfg = gold["cfg"]
    model = build_model(cfg, product).cuda().train()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    blocks, _ = case_inputs(cfg, 0)
    torch.manual_seed(cfg["perm_seed"])
    with torch.no_grad():
        out, _ = model(blocks[0].cuda())
    after = model.state_dict()
    # in_train_mode is False: no momentum update, no enqueue (model/pretrain.py:157,161,188)
    for k in ("queue", "queue_ptr", "encoder_k.4.bias", "encoder_k.0.Conv_1a.conv1.weight"):
        assert torch.equal(before[k], after[k]), k
    from _cases import check_close
    check_close(out, gold["steps"][0]["logits"], 1e-3, "no-grad logits")


def test_k_not_multiple_of_batch_asserts():
    import model.pretrain as product
    torch.manual_seed(0)
    model = product.InfoNCE('s3d', 128, 30, 0.999, 0.07).cuda().train()
    x = torch.randn(4, 2, 3, 16, 64, 64).cuda()
    with pytest.raises(AssertionError):
        model(x)
    with pytest.raises(AssertionError):
        model(torch.randn(4, 3, 3, 16, 64, 64).cuda())   # N != 2


def test_select_backbone_contract():
    from backbone.select_backbone import select_backbone
    net, param = select_backbone('s3d')
    assert param == {'feature_size': 1024}
    _, param = select_backbone('r50')
    assert param == {'feature_size': 2048}
    with pytest.raises(NotImplementedError):
        select_backbone('vgg')
    x = torch.randn(2, 3, 16, 64, 64).cuda()
    y = net.cuda()(x)
    assert y.shape == (2, 1024, 2, 2, 2)


def test_graph_replay_matches_eager():
    """From its second call on, a gradient-free encoder pass is replayed from a captured hipGraph
    (model.pretrain._encode_graphed).  The same key encoder driven five times through the
    graph path and through the eager path (identical copies, identical inputs, momentum update
    as the captured prologue): keys, momentum-updated weights and BatchNorm running statistics
    must agree bit for bit -- every kernel on this path is deterministic."""
    import copy
    import model.pretrain as product
    import coclr_amd.model.pretrain as impl
    if not impl._GRAPHS:
        pytest.skip("hipGraph replay switched off by COCLR_GRAPHS=0")
    gold = load_golden("infonce_s3d_small")
    cfg = gold["cfg"]
    base = build_model(cfg, product)
    models = [copy.deepcopy(base).cuda().train() for _ in range(2)]
    keys = [[], []]
    for which, graphs in enumerate((True, False)):
        m = models[which]
        m._sync_buffers()
        product._GRAPHS = graphs
        try:
            with torch.no_grad():
                for step in range(5):
                    blocks, _ = case_inputs(cfg, step % cfg["steps"])
                    x2 = blocks[0][:, 1].cuda()
                    idx = torch.randperm(x2.shape[0], generator=torch.Generator().manual_seed(step)).cuda()
                    keys[which].append(m._encode_graphed(m.encoder_k, x2, idx,
                                                         pre=m._momentum_update_key_encoder).clone())
        finally:
            product._GRAPHS = True
    assert any("graph" in ent for key, ent in models[0].__dict__["_graphs"].items()
               if key[0] == id(models[0].encoder_k))
    for a, b in zip(*keys):
        assert torch.equal(a, b)
    sd_g, sd_e = models[0].state_dict(), models[1].state_dict()
    for k in sd_g:
        assert torch.equal(sd_g[k], sd_e[k]), k


@pytest.mark.parametrize("split", [False, True])
def test_planned_query_encoder_matches_eager(split, monkeypatch):
    """COCLR_PLAN=1 (the default): after four interpreted passes the query encoder's forward and backward are
    run once with their allocations in a private pool while every C-ABI call is logged (coclr_amd/plan.py), and
    every later pass re-issues the logs -- ordinary launches on the ordinary streams with pre-marshalled
    arguments.  Same kernels, same order, same operands: logits of every step and all parameters after ten
    Adam steps must be BIT-identical to the interpreted run -- as one autograd node and as one node per
    backbone stage.  The input is a new tensor every step (the recorded addresses of it are patched), step 7
    runs a forward that no backward follows (main_coclr.py:403 until the queue is full), and the steps after the
    recording must really have been replays."""
    import copy
    import torch.nn.functional as F
    import model.pretrain as product
    from coclr_amd import engine
    from coclr_amd.backbone import s3dg
    monkeypatch.setattr(s3dg, "_SPLIT_MODE", "1" if split else "0")
    gold = load_golden("infonce_s3d_small")
    cfg = gold["cfg"]
    base = build_model(cfg, product)
    results = []
    for planned in (False, True):
        monkeypatch.setattr(engine, "PLAN", planned)
        engine.PLAN_STATS.update(recorded=0, replayed=0, disabled=[])
        model = copy.deepcopy(base).cuda().train()
        opt = torch.optim.Adam([{"params": p} for _, p in model.named_parameters()], lr=1e-3,
                               weight_decay=1e-5)
        outs, held = [], []
        for step in range(10):
            blocks, _ = case_inputs(cfg, step % cfg["steps"])
            torch.manual_seed(cfg["perm_seed"] + step)
            x = blocks[0].cuda()
            held.append(x)                   # keeps every input alive: each step's clip has its own address
            out, tgt = model(x)
            outs.append(out.detach().clone())
            if step == 7:
                continue                     # a forward nobody differentiates
            loss = F.cross_entropy(out, tgt)
            opt.zero_grad()
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        if planned:
            mods = [model.encoder_q[0]] if not split else model.encoder_q[0]._stage_groups()
            for m in mods:
                ents = list(m.__dict__["_coclr_plan_entries"].values())
                assert any(e.fwd is not None and e.bwd is not None and not e.disabled for e in ents), \
                    "the pass was never recorded"
            n = len(mods)
            assert engine.PLAN_STATS["disabled"] == []
            assert engine.PLAN_STATS["recorded"] == n and engine.PLAN_STATS["replayed"] == 5 * n, engine.PLAN_STATS
        results.append((outs, [p.detach().clone() for p in model.parameters()],
                        {k: v.clone() for k, v in model.state_dict().items()}))
    (o_e, p_e, sd_e), (o_g, p_g, sd_g) = results
    for step, (a, b) in enumerate(zip(o_e, o_g)):
        assert torch.equal(a, b), "logits of step %d" % step
    for a, b in zip(p_e, p_g):
        assert torch.equal(a, b)
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k


@pytest.mark.parametrize("kind", ["infonce", "coclr"])
def test_fused_head_matches_module_by_module_head(kind, monkeypatch):
    """The training step runs the projection head and the logits through coclr_gemm_fused (three launches
    forward, five backward: model/pretrain.py `_QueryHeadFn`, `_head_forward`) instead of module by module
    (GlobalAvgPool3d, PointwiseConv3d, HeadReLU, PointwiseConv3d, F.normalize, logits: 8 + 21 launches).
    Same products, same split-K fold order, same row operations with every rounding pinned: logits of every
    step, every gradient of the first step and all parameters after three Adam steps are BIT-identical."""
    import copy
    import model.pretrain as product
    import coclr_amd.model.pretrain as impl
    from _cases import loss_fn
    gold = load_golden("%s_s3d_small" % kind)
    cfg = gold["cfg"]
    base = build_model(cfg, product)
    results = []
    modes = (True, False)
    if os.environ.get("COCLR_TEST_HEAD_MODES"):          # diagnosis: e.g. "0,0" runs the module path twice
        modes = tuple(v == "1" for v in os.environ["COCLR_TEST_HEAD_MODES"].split(","))
    for fused in modes:
        monkeypatch.setattr(impl, "FUSED_HEAD", fused)
        model = copy.deepcopy(base).cuda().train()
        if kind == "coclr":
            model.sampler.eval()
        opt = torch.optim.Adam([{"params": p} for _, p in model.named_parameters()], lr=1e-3,
                               weight_decay=1e-5)
        outs, grads = [], None
        for step in range(3):
            blocks, extra = case_inputs(cfg, step % cfg["steps"])
            torch.manual_seed(cfg["perm_seed"] + step)
            if kind == "infonce":
                out, tgt = model(blocks[0].cuda())
            else:
                out, tgt = model(blocks[0].cuda(), blocks[1].cuda(), extra.cuda())
            loss = loss_fn(kind, out, tgt)
            opt.zero_grad()
            loss.backward()
            if step == 0:
                grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
            opt.step()
            outs.append(out.detach().clone())
        torch.cuda.synchronize()
        results.append((outs, grads, [p.detach().clone() for p in model.parameters()]))
    (o_f, g_f, p_f), (o_m, g_m, p_m) = results
    assert set(g_f) == set(g_m) and len(g_f) >= 235
    # every rounding of the row operations is pinned in csrc/nce.hip (ep_* helpers): not "close", identical
    for k in g_f:
        assert torch.equal(g_f[k], g_m[k]), (k, float((g_f[k] - g_m[k]).abs().max()), float(g_m[k].abs().max()))
    for step, (a, b) in enumerate(zip(o_f, o_m)):
        assert torch.equal(a, b), ("logits of step %d" % step, float((a - b).abs().max()))
    for a, b in zip(p_f, p_m):
        assert torch.equal(a, b)
    exact = True
    print("fused head vs module-by-module head (%s): bit-identical = %s" % (kind, exact))
