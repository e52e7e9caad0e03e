"""GPU parity of the single-launch SGD step (coclr_sgd_step, csrc/optim.hip; coclr_amd/optim.py::SGD)
against torch's own torch.optim.SGD (saved before install(), foreach path) on the same GPU from the
same gradients.  Bar: 1e-6 relative per step (the Adam tests' bar); the kernel reproduces the foreach
arithmetic operation for operation, and the trajectories below are asserted bit-identical."""
import copy

import pytest
import torch

from _cases import check_close

pytestmark = pytest.mark.gpu


def _O():
    from coclr_amd import optim as O
    return O


def _pair(shapes, seed=0):
    g = torch.Generator().manual_seed(seed)
    host = [torch.randn(s, generator=g) for s in shapes]
    ps = [h.cuda().requires_grad_(True) for h in host]
    ref_ps = [h.cuda().requires_grad_(True) for h in host]
    return ps, ref_ps


def _grads(ps, ref_ps, gen, skip=()):
    for i, (p, rp) in enumerate(zip(ps, ref_ps)):
        if i in skip:
            p.grad = rp.grad = None
            continue
        gr = (torch.randn(rp.shape, generator=gen) * 0.1).cuda()
        p.grad, rp.grad = gr, gr.clone()


def _same(ps, ref_ps, what):
    for p, rp in zip(ps, ref_ps):
        check_close(p, rp, 1e-6, what)
        assert torch.equal(p.detach(), rp.detach()), what + ": not bit-identical"


def _state_same(opt, ref, ps, ref_ps):
    for p, rp in zip(ps, ref_ps):
        a, b = opt.state.get(p, {}), ref.state.get(rp, {})
        assert set(a) == set(b)
        if "momentum_buffer" in b:
            assert torch.equal(a["momentum_buffer"], b["momentum_buffer"])


SIZES = [(1,), (5,), (32768,), (32768 + 3,), (7, 3)]
OPTIONS = [
    dict(momentum=0.0),
    dict(momentum=0.9),
    dict(momentum=0.9, dampening=0.1),
    dict(momentum=0.9, nesterov=True),
    dict(momentum=0.9, weight_decay=1e-3),
    dict(momentum=0.0, weight_decay=1e-3),
    dict(momentum=0.9, dampening=0.1, weight_decay=1e-3, maximize=True),
    dict(momentum=0.9, nesterov=True, weight_decay=1e-3, maximize=True),
]


@pytest.mark.parametrize("opts", OPTIONS, ids=lambda o: "-".join("%s=%s" % kv for kv in o.items()))
def test_sgd_matches_torch(opts):
    """Per-tensor groups (eval/main_classifier.py:134-140: backbone at lr/10), every option, sizes of 1,
    5, _CHUNK and _CHUNK+3 elements, a parameter that has no gradient in some steps, an lr change."""
    O = _O()
    ps, ref_ps = _pair(SIZES)
    lrs = [0.01 if i % 2 else 0.1 for i in range(len(ps))]
    opt = O.SGD([{"params": p, "lr": lr} for p, lr in zip(ps, lrs)], lr=0.1, **opts)
    ref = O._TorchSGD([{"params": p, "lr": lr} for p, lr in zip(ref_ps, lrs)], lr=0.1, **opts)
    gen = torch.Generator().manual_seed(1)
    for step in range(6):
        skip = (1,) if step in (0, 3) else ()      # (5,) gets no gradient in steps 0 and 3
        if step == 4:
            for g in list(opt.param_groups) + list(ref.param_groups):
                g["lr"] = g["lr"] * 0.1
        _grads(ps, ref_ps, gen, skip)
        opt.step()
        ref.step()
        assert opt._plan is not None, "the HIP path must be the one that ran"
        _same(ps, ref_ps, "step %d" % step)
        _state_same(opt, ref, ps, ref_ps)
    if opts.get("momentum", 0) == 0:
        assert len(opt.state) == 0 and opt.state_dict()["state"] == {}


@pytest.mark.parametrize("opts", [dict(momentum=0.9, weight_decay=1e-3), dict(momentum=0.9, nesterov=True)],
                         ids=lambda o: "-".join("%s=%s" % kv for kv in o.items()))
def test_sgd_gradients_as_bucket_views(opts):
    """The gradients are views 4 bytes into one flat buffer each, as DDP's bucket views are: no row of the launch has its
    three pointers on a 16-byte boundary, every chunk takes the scalar loop, and the step stays bit-identical."""
    O = _O()
    ps, ref_ps = _pair([(5,), (32768 + 3,)])
    opt = O.SGD([{"params": p} for p in ps], lr=0.1, **opts)
    ref = O._TorchSGD([{"params": p} for p in ref_ps], lr=0.1, **opts)
    bucket = torch.zeros(1 + sum(p.numel() for p in ps) + 8, device="cuda")
    assert bucket.data_ptr() % 16 == 0
    gen = torch.Generator().manual_seed(6)
    for step in range(4):
        off = 1
        for p, rp in zip(ps, ref_ps):
            gr = (torch.randn(rp.shape, generator=gen) * 0.1).cuda()
            p.grad = bucket[off:off + p.numel()].view_as(p)
            p.grad.copy_(gr)
            rp.grad = gr
            assert p.grad.data_ptr() % 16 != 0 and p.grad.is_contiguous()
            off += p.numel() + 3                    # 1, 9: both one float past a 16-byte boundary
        opt.step()
        ref.step()
        assert opt._plan is not None, "the HIP path must be the one that ran"
        _same(ps, ref_ps, "step %d" % step)
        _state_same(opt, ref, ps, ref_ps)


def test_one_launch_per_step_and_no_foreach(monkeypatch):
    O = _O()
    from coclr_amd import ops
    calls = {"sgd": 0, "foreach": 0}
    inner = ops.sgd_step

    def counted(*a, **k):
        calls["sgd"] += 1
        return inner(*a, **k)
    monkeypatch.setattr(ops, "sgd_step", counted)
    for name in [n for n in dir(torch) if n.startswith("_foreach_")]:
        fn = getattr(torch, name)

        def wrap(*a, _fn=fn, **k):
            calls["foreach"] += 1
            return _fn(*a, **k)
        monkeypatch.setattr(torch, name, wrap)
    ps, ref_ps = _pair([(64, 3), (10,), (32768 + 3,)] * 20)
    opt = O.SGD([{"params": p} for p in ps], lr=0.05, momentum=0.9, weight_decay=1e-3)
    gen = torch.Generator().manual_seed(2)
    for step in range(3):
        _grads(ps, ref_ps, gen)
        before = dict(calls)
        opt.step()
        assert calls["sgd"] - before["sgd"] == 1
        assert calls["foreach"] == before["foreach"] == 0


def test_state_dict_round_trip_both_ways():
    O = _O()
    shapes = [(33, 7), (5,), (32768 + 3,)]
    ps, ref_ps = _pair(shapes)
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-3)
    opt = O.SGD([{"params": p} for p in ps], **kw)
    ref = O._TorchSGD([{"params": p} for p in ref_ps], **kw)
    gen = torch.Generator().manual_seed(3)
    for _ in range(2):
        _grads(ps, ref_ps, gen)
        opt.step()
        ref.step()
    sd, rsd = opt.state_dict(), ref.state_dict()
    assert sd["param_groups"] == rsd["param_groups"]
    assert sorted(sd["state"]) == sorted(rsd["state"]) == [0, 1, 2]
    for k in sd["state"]:
        assert list(sd["state"][k]) == ["momentum_buffer"]
        assert torch.equal(sd["state"][k]["momentum_buffer"], rsd["state"][k]["momentum_buffer"])
    # ours -> torch, torch -> ours; both continue in lock step with the uninterrupted pair
    ps2, ref_ps2 = [p.detach().clone().requires_grad_(True) for p in ps], \
        [p.detach().clone().requires_grad_(True) for p in ref_ps]
    # through a checkpoint (load_state_dict keeps device tensors it is handed: no shared buffers)
    t_from_ours = O._TorchSGD([{"params": p} for p in ref_ps2], **kw)
    t_from_ours.load_state_dict(copy.deepcopy(sd))
    ours_from_t = O.SGD([{"params": p} for p in ps2], **kw)
    ours_from_t.load_state_dict(copy.deepcopy(rsd))
    for _ in range(3):
        _grads(ps, ref_ps, gen)
        for a, b in zip(ps2 + ref_ps2, ps + ps):
            a.grad = b.grad.clone()
        for o in (opt, ref, t_from_ours, ours_from_t):
            o.step()
        assert ours_from_t._plan is not None
        _same(ps, ref_ps, "uninterrupted")
        _same(ps2, ref_ps, "torch state -> ours")
        _same(ref_ps2, ref_ps, "our state -> torch")


def test_leaves_and_reenters_the_native_path():
    """A step the kernel does not cover (explicit foreach; a CPU parameter) runs torch's own
    implementation on the same momentum buffers; the next covered step picks them up again."""
    O = _O()
    ps, ref_ps = _pair([(100,), (7, 3)])
    opt = O.SGD([{"params": p} for p in ps], lr=0.05, momentum=0.9, dampening=0.1)
    ref = O._TorchSGD([{"params": p} for p in ref_ps], lr=0.05, momentum=0.9, dampening=0.1)
    gen = torch.Generator().manual_seed(4)

    def step(native_expected):
        _grads(ps, ref_ps, gen)
        opt.step()
        ref.step()
        assert (opt._plan is not None) == native_expected
        _same(ps, ref_ps, "parameter")
        _state_same(opt, ref, ps, ref_ps)

    step(True)
    buf = opt.state[ps[0]]["momentum_buffer"]
    opt.param_groups[0]["foreach"] = True           # an explicit torch path: not ours
    step(False)
    assert opt.state[ps[0]]["momentum_buffer"] is buf, "torch's step keeps the buffer"
    opt.param_groups[0]["foreach"] = None
    step(True)
    step(True)
    # a CPU parameter in the optimiser: torch's implementation for the whole step, then back
    cpu = torch.randn(4, requires_grad=True)
    cpu_ref = cpu.detach().clone().requires_grad_(True)
    opt.add_param_group({"params": cpu})
    ref.add_param_group({"params": cpu_ref})
    cpu.grad = torch.ones(4)
    cpu_ref.grad = torch.ones(4)
    step(False)
    check_close(cpu, cpu_ref, 0, "cpu parameter")
    cpu.grad = cpu_ref.grad = None
    step(True)


@pytest.mark.parametrize("case", ["tensor_lr", "foreach_false", "fused", "differentiable", "sparse",
                                  "fp64", "two_devices"])
def test_fallthrough_cases_are_torch(case):
    O = _O()
    kw = dict(lr=0.05, momentum=0.9)
    shapes = [(10, 4), (6,)]
    ps, ref_ps = _pair(shapes)
    if case == "tensor_lr":
        kw["lr"] = torch.tensor(0.05)
    elif case == "foreach_false":
        kw["foreach"] = False
    elif case == "fused":
        kw["fused"] = True
    elif case == "differentiable":
        kw["differentiable"] = True
    elif case == "sparse":
        kw["momentum"] = 0.0
    elif case == "fp64":
        ps = [p.detach().double().requires_grad_(True) for p in ps]
        ref_ps = [p.detach().double().requires_grad_(True) for p in ref_ps]
    elif case == "two_devices":
        if torch.cuda.device_count() < 2:
            ps[1] = ps[1].detach().cpu().requires_grad_(True)      # host + device: not one device
            ref_ps[1] = ref_ps[1].detach().cpu().requires_grad_(True)
        else:
            ps[1] = ps[1].detach().to("cuda:1").requires_grad_(True)
            ref_ps[1] = ref_ps[1].detach().to("cuda:1").requires_grad_(True)
    opt = O.SGD([{"params": p} for p in ps], **kw)
    ref = O._TorchSGD([{"params": p} for p in ref_ps], **kw)
    gen = torch.Generator().manual_seed(5)
    for _ in range(3):
        if case == "sparse":
            for p, rp in zip(ps, ref_ps):
                d = (torch.randn(rp.shape, generator=gen) * (torch.rand(rp.shape, generator=gen) < 0.3)).cuda()
                p.grad, rp.grad = d.to_sparse(), d.to_sparse()
        else:
            for p, rp in zip(ps, ref_ps):
                gr = torch.randn(rp.shape, generator=gen, dtype=rp.dtype).to(rp.device)
                p.grad, rp.grad = gr, gr.clone()
        if case == "differentiable":
            assert opt._native_groups() is None     # torch's differentiable step needs graph-mode callers
            return
        opt.step()
        ref.step()
        assert opt._plan is None, "torch's implementation must be the one that ran"
        for p, rp in zip(ps, ref_ps):
            assert torch.equal(p.detach(), rp.detach())


def test_scoping_plain_module_stays_on_torch():
    """After install(), torch.optim.SGD over somebody else's nn.Linear is torch's step, step for step;
    over a LinearClassifier's parameters it is the native one."""
    O = _O()
    import model.classifier  # noqa: F401  (the shim installs the subclasses)
    assert torch.optim.SGD is O.ScopedSGD
    torch.manual_seed(0)
    lin = torch.nn.Linear(16, 4).cuda()
    opt = torch.optim.SGD(lin.parameters(), lr=0.1, momentum=0.9)
    x = torch.randn(8, 16, device="cuda")
    lin(x).square().sum().backward()
    opt.step()
    assert opt._ours is False and opt._plan is None
    from coclr_amd.model.classifier import LinearClassifier
    head = LinearClassifier(num_class=5, network="s3d", use_dropout=False, use_final_bn=True, use_l2_norm=True)
    head = head.cuda()
    ps = [p for n, p in head.named_parameters() if "backbone" not in n]
    opt2 = torch.optim.SGD([{"params": p} for p in ps], lr=0.1, momentum=0.9)
    for p in ps:
        p.grad = torch.randn_like(p)
    opt2.step()
    assert opt2._ours is True and opt2._plan is not None
