"""Differentiated launch plans (engine.PlanFn, COCLR_PLAN=1: the default and the path bench.py times) across the
life of a training run.  After engine._PLAN_WARMUP interpreted passes the forward and the backward of a backbone
node are re-issued from recorded logs, with outputs and gradients in static buffers of a private pool: a launch
the log does not see, a stale address, a tape consumed twice or a buffer overwritten early corrupts training
without any kernel being wrong.

The oracle is the interpreted pass: every scenario runs twice from `copy.deepcopy` of one module, with
engine.PLAN False and True (tests/_train_plan_loop.py), and every comparison is `torch.equal` -- the plan
re-issues the same kernels with the same operands in the same order, so there is no tolerance to choose.
An S3D runs as ONE node here; test_gpu_model.py::test_planned_query_encoder_matches_eager keeps the split case."""
import pytest
import torch

import _train_plan_loop as L

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _one_node(monkeypatch):
    from coclr_amd.backbone import s3dg
    monkeypatch.setattr(s3dg, "_SPLIT_MODE", "0")


def _W():
    from coclr_amd import engine
    return engine._PLAN_WARMUP


def _s3d():
    return L.backbone("s3d")


@pytest.mark.parametrize("network", ["s3d", "s3dg", "r50"])
def test_replayed_steps_bit_identical(monkeypatch, network):
    W = _W()

    def scenario(tw):
        for x in tw.upload(L.clips(W + 5)):
            tw.step(x)

    oracle, plan = L.run_twins(lambda: L.backbone(network), scenario, monkeypatch)
    L.assert_not_vacuous(oracle)
    n = len(L.holders(plan.net))
    assert n >= 1
    assert plan.delta == (n, 4 * n, 0) and plan.disabled == [], (plan.delta, plan.disabled)
    assert plan.replays == [0] * (W + 1) + [n] * 4
    for m in L.holders(plan.net):
        (ent,) = m.__dict__["_coclr_plan_entries"].values()
        assert ent.fwd is not None and ent.bwd is not None and ent.run is None and not ent.disabled


def test_input_gradient_through_static_dx(monkeypatch):
    W = _W()

    def scenario(tw):
        for x in tw.upload(L.clips(W + 5)):
            tw.step(x.requires_grad_(True))

    oracle, plan = L.run_twins(_s3d, scenario, monkeypatch)
    L.assert_not_vacuous(oracle)
    assert all("dx" in rec and float(rec["dx"].abs().max()) > 0 for rec in oracle.log)
    n = len(L.holders(plan.net))
    assert plan.delta == (n, 4 * n, 0)
    assert all(e.dx is not None for e in L.entries(plan.net))


def test_input_gradient_alternating(monkeypatch):
    """requires_grad of the input is part of the entry's key: each kind gets its own plan, recorded once."""
    W = _W()

    def scenario(tw):
        for i, x in enumerate(tw.upload(L.clips(2 * (W + 3)))):
            tw.step(x.requires_grad_(i % 2 == 0))

    oracle, plan = L.run_twins(_s3d, scenario, monkeypatch)
    assert ["dx" in rec for rec in oracle.log] == [i % 2 == 0 for i in range(2 * (W + 3))]
    n = len(L.holders(plan.net))
    assert plan.delta == (2 * n, 2 * 2 * n, 0), plan.delta
    for m in L.holders(plan.net):
        store = m.__dict__["_coclr_plan_entries"]
        assert sorted(k[1] for k in store) == [False, True]
        assert all(e.fwd is not None and e.bwd is not None and not e.disabled for e in store.values())
        assert [e.dx is not None for k, e in sorted(store.items(), key=lambda kv: kv[0][1])] == [False, True]


def test_frozen_prefix_then_unfreeze(monkeypatch):
    from coclr_amd import engine
    W = _W()

    def stem(net):
        return [net.Conv_1a.conv1.weight, net.Conv_1a.bn1.weight, net.Conv_1a.bn1.bias]

    def scenario(tw):
        frozen = stem(tw.net)
        for p in frozen:
            p.requires_grad_(False)
        xs = tw.upload(L.clips(2 * (W + 3)))
        for i, x in enumerate(xs):
            if i == W + 3:
                for p in frozen:
                    p.requires_grad_(True)
            tw.step(x)
            if i == W:                           # the recording step of the first entry
                tw.marks["static"] = len(engine._STATIC_PTRS)
                tw.marks["recorded"] = L.stats()[0]

    oracle, plan = L.run_twins(_s3d, scenario, monkeypatch)
    L.assert_not_vacuous(oracle)
    idx = [i for i, p in enumerate(oracle.params) if any(p is q for q in stem(oracle.net))]
    assert len(idx) == 3
    for tw in (oracle, plan):
        for step, rec in enumerate(tw.log):
            assert [rec["g"][i] is None for i in idx] == [step < W + 3] * 3, step
    n = len(L.holders(plan.net))
    assert plan.delta[0] == 2 * n and plan.delta[2] == 0
    assert plan.marks["recorded"] + n == L.stats()[0]
    assert plan.replays == ([0] * (W + 1) + [n] * 2) * 2
    for m in L.holders(plan.net):
        assert len(m.__dict__["_coclr_plan_entries"]) == 1
    assert len(engine._STATIC_PTRS) <= plan.marks["static"]      # the dropped entry's pointers were discarded


def test_gradient_accumulation(monkeypatch):
    """Two micro-batches per update with no zeroing in between: at the second backward `.grad` still aliases the
    recorded gradient tensor that backward overwrites, so PlanFn gives it its own memory first."""
    W = _W()

    def scenario(tw):
        xs = tw.upload(L.clips(2 * (W + 4)))
        for r in range(W + 4):
            replays = 2 * r + 1 > W + 1          # both micro-batches of this round come after the recording
            tw.step(xs[2 * r], update=False)
            if tw.planned and replays:
                ents = L.entries(tw.net)
                alias = [p.grad.data_ptr() == g.data_ptr()
                         for e in ents for p, g in zip(tw.params, e.grads) if g is not None]
                assert alias and all(alias), "`.grad` does not alias the recorded gradients: nothing to clone"
            tw.step(xs[2 * r + 1], update=False)
            if tw.planned and replays:
                assert not any(p.grad.data_ptr() == g.data_ptr()
                               for e in L.entries(tw.net) for p, g in zip(tw.params, e.grads) if g is not None)
            tw.update()

    oracle, plan = L.run_twins(_s3d, scenario, monkeypatch)
    L.assert_not_vacuous(oracle)
    n = len(L.holders(plan.net))
    assert plan.delta == (n, (2 * (W + 4) - W - 1) * n, 0), plan.delta
    # the second backward of a round really added to the first one's gradients
    i = next(i for i, p in enumerate(oracle.params) if p.dim() == 5)
    assert not torch.equal(oracle.log[-1]["g"][i], oracle.log[-2]["g"][i])


@pytest.mark.parametrize("network", ["s3d", "s3dg"])
def test_gradients_stay_valid_across_the_next_forward(monkeypatch, network):
    """The launch scripts call zero_grad() in FRONT of backward, so `.grad` -- an alias of the plan's recorded
    gradient tensors -- is still held while the next forward is replayed; INTEGRATION.md promises it until the
    next backward.  Every gradient (parameters and input) is read once more after the following forward."""
    W = _W()

    def scenario(tw):
        held = None
        for x in tw.upload(L.clips(W + 4)):
            y = tw.forward(x.requires_grad_(True))
            if held is not None:
                tw.log[-1]["late"] = [g.clone() for g in held]
            rec = {"y": y.detach().clone()}
            tw.zero()
            y.backward(tw.dout(y))
            rec.update(tw.grads(x))
            tw.log.append(rec)
            held = [p.grad for p in tw.params] + [x.grad]
            for p in tw.params:
                p.data.add_(p.grad, alpha=-L.LR)

    oracle, plan = L.run_twins(lambda: L.backbone(network), scenario, monkeypatch)
    L.assert_not_vacuous(oracle)
    for rec in oracle.log[:-1]:
        assert all(torch.equal(a, b) for a, b in zip(rec["late"], rec["g"] + [rec["dx"]]))
    n = len(L.holders(plan.net))
    assert plan.delta == (n, 3 * n, 0), plan.delta


def test_forward_only_phase_across_the_recording(monkeypatch):
    """main_coclr.py skips loss.backward() until the queue is full: forwards under grad that nothing
    differentiates, each at another address, while the entry leaves warm-up.  The plan must come back once the
    run starts to train."""
    W = _W()

    def scenario(tw):
        xs = tw.upload(L.clips(2 * W + 6))
        for x in xs[:W + 2]:
            tw.step(x, differentiate=False)
        for x in xs[W + 2:]:
            tw.step(x)

    oracle, plan = L.run_twins(_s3d, scenario, monkeypatch)
    L.assert_not_vacuous(oracle)
    n = len(L.holders(plan.net))
    assert plan.disabled == [] and plan.delta[2] == 0
    assert plan.replays[-2:] == [n, n], "the plan never came back: %r" % (plan.replays,)
    assert plan.delta[1] >= 2 * n
    for ent in L.entries(plan.net):
        assert ent.fwd is not None and ent.bwd is not None and ent.run is None


def test_shape_cap(monkeypatch):
    from coclr_amd import engine
    W = _W()
    batches = (2, 1, 3, 4)
    assert len(batches) == engine._PLAN_MAX_SHAPES + 1

    def scenario(tw):
        per = [tw.upload(L.clips(W + 2, batch=b, seed=20 + b)) for b in batches]
        for r in range(W + 2):
            for xs in per:
                tw.step(xs[r])

    oracle, plan = L.run_twins(_s3d, scenario, monkeypatch)
    n = len(L.holders(plan.net))
    cap = engine._PLAN_MAX_SHAPES
    assert plan.delta == (cap * n, cap * n, 0), plan.delta
    for m in L.holders(plan.net):
        store = m.__dict__["_coclr_plan_entries"]
        assert len(store) == cap
        assert sorted(k[0][0] for k in store) == sorted(batches[:cap])       # the fourth shape never got in
        assert sum(e.pool is not None for e in store.values()) == cap
    assert [r for i, r in enumerate(plan.replays) if i % 4 == 3] == [0] * (W + 2)


def test_moved_parameter_storage(monkeypatch):
    W = _W()

    def scenario(tw):
        xs = tw.upload(L.clips(2 * (W + 2)))
        for i, x in enumerate(xs):
            if i == W + 2:
                w = tw.net.Mixed_4b.branch1[1].conv1.weight
                old = w.data_ptr()
                w.data = w.data.clone()
                assert w.data_ptr() != old
            tw.step(x)

    oracle, plan = L.run_twins(_s3d, scenario, monkeypatch)
    L.assert_not_vacuous(oracle)
    n = len(L.holders(plan.net))
    assert plan.delta == (2 * n, 2 * n, 0), plan.delta
    assert plan.replays == ([0] * (W + 1) + [n]) * 2


def test_batchnorm_modes_under_grad(monkeypatch):
    """Fine-tuning with frozen statistics (every BatchNorm in eval(), gradients on), then back to train()."""
    W = _W()

    def buffers(net):
        return {k: v.clone() for k, v in net.named_buffers()}

    def scenario(tw):
        bns = [m for m in tw.net.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
        xs = tw.upload(L.clips(2 * (W + 2)))
        for m in bns:
            m.eval()
        before = buffers(tw.net)
        for x in xs[:W + 2]:
            tw.step(x)
        after = buffers(tw.net)
        assert before.keys() == after.keys() and len(before) >= 3 * len(bns)
        for k in before:
            assert torch.equal(before[k], after[k]), "%s moved while its module was in eval()" % k
        for m in bns:
            m.train()
        for x in xs[W + 2:]:
            tw.step(x)
        assert any(not torch.equal(v, after[k]) for k, v in buffers(tw.net).items())

    oracle, plan = L.run_twins(_s3d, scenario, monkeypatch)
    L.assert_not_vacuous(oracle)
    n = len(L.holders(plan.net))
    assert plan.delta == (2 * n, 2 * n, 0), plan.delta


def test_pass_on_another_stream(monkeypatch):
    W = _W()

    def scenario(tw):
        xs = tw.upload(L.clips(W + 4))
        side = torch.cuda.Stream()
        for i, x in enumerate(xs):
            tw.step(x, stream=side if i == W + 2 else None)
        torch.cuda.synchronize()

    oracle, plan = L.run_twins(_s3d, scenario, monkeypatch)
    L.assert_not_vacuous(oracle)
    n = len(L.holders(plan.net))
    assert plan.replays == [0] * (W + 1) + [n, 0, n], plan.replays
    assert plan.delta == (n, 2 * n, 0)


@pytest.mark.parametrize("misuse", ["second_backward", "two_forwards"])
def test_graph_misuse_is_loud_and_leaves_the_module_usable(monkeypatch, misuse):
    """The aliasing contract: the activations of a planned pass live until the next forward of
    the module.  A second backward through one graph raises in both runs; two forwards followed by one backward
    over both graphs work interpreted and raise the error that names COCLR_PLAN=0 when planned.  Neither run
    updates on the misuse step, and the steps after it are ordinary replays."""
    W = _W()

    def scenario(tw):
        xs = tw.upload(L.clips(W + 2 + 2 + 2))
        for x in xs[:W + 2]:
            tw.step(x)
        if misuse == "second_backward":
            y = tw.forward(xs[W + 2])
            d = tw.dout(y)
            y.backward(d, retain_graph=True)
            with pytest.raises(RuntimeError, match="backward called twice"):
                y.backward(d)
        else:
            y1, y2 = tw.forward(xs[W + 2]), tw.forward(xs[W + 3])
            loss = y1.sum() + y2.sum()
            if tw.planned:
                with pytest.raises(RuntimeError, match="COCLR_PLAN=0"):
                    loss.backward()
            else:
                loss.backward()
        torch.cuda.synchronize()
        tw.zero()
        for x in xs[W + 4:]:
            tw.step(x)

    oracle, plan = L.run_twins(_s3d, scenario, monkeypatch)
    L.assert_not_vacuous(oracle)
    n = len(L.holders(plan.net))
    assert plan.replays[-2:] == [n, n] and plan.delta[0] == n and plan.delta[2] == 0
    assert all(not e.disabled for e in L.entries(plan.net))


class _Injector:
    """engine._run_closure, except that the armed call raises BEFORE it runs its closure: host-only -- every
    launch issued up to then is the product's own."""

    def __init__(self, inner):
        self.inner, self.count, self.fail_at = inner, 0, None

    def __call__(self, fn, run):
        if self.fail_at is not None and self.count == self.fail_at:
            self.fail_at = None
            raise RuntimeError("injected: tape entry %d" % self.count)
        self.count += 1
        return self.inner(fn, run)


def test_raise_while_the_backward_is_recorded(monkeypatch):
    """A backward pass that raises partway (out of memory, a collective error) on the very pass that records the
    backward log: the tape is half consumed.  The entry must not go on as if it held a whole tape."""
    from coclr_amd import engine
    W = _W()
    inj = _Injector(engine._run_closure)
    monkeypatch.setattr(engine, "_run_closure", inj)

    def scenario(tw):
        xs = tw.upload(L.clips(2 * W + 4))
        tape = None
        for i, x in enumerate(xs):
            inj.count = 0
            if i != W:
                tw.step(x)
                if i < W:                            # interpreted in both runs: one closure per tape entry
                    tape = tape or inj.count
                    assert inj.count == tape > 2
                continue
            rec0 = L.stats()[0]
            inj.fail_at = tape // 2                  # the middle of the tape
            y = tw.forward(x)
            kept = y.detach().clone()
            if tw.planned:
                assert L.stats()[0] - rec0 == len(L.holders(tw.net)) == 1, "not the recording pass"
                assert all(e.run is not None and e.bwd is None for e in L.entries(tw.net))
            with pytest.raises(RuntimeError, match="injected: tape entry"):
                y.backward(tw.dout(y))
            assert inj.fail_at is None and inj.count == tape // 2
            torch.cuda.synchronize()                 # the weight-gradient stream may still be running
            tw.zero()
            tw.log.append({"y": kept})

    oracle, plan = L.run_twins(_s3d, scenario, monkeypatch)
    L.assert_not_vacuous(oracle)
    assert len(plan.log) == 2 * W + 4
    for ent in L.entries(plan.net):
        cleared = ent.disabled and ent.run is None and ent.fwd is None and ent.bwd is None and ent.pool is None
        rerecorded = not ent.disabled and ent.run is None and ent.fwd is not None and ent.bwd is not None
        assert cleared or rerecorded, "the entry kept a half-consumed tape"
