"""The step loop of tests/test_gpu_train_plan.py: one scenario, run twice from `copy.deepcopy` of one freshly built
backbone -- interpreted (engine.PLAN False: the oracle) and through the differentiated launch plan (engine.PLAN
True) -- and compared bit for bit: every step's output, every gradient, the final parameters and buffers."""
import copy

import torch

CLIP = (3, 16, 64, 64)
LR = 1e-4               # small: the weights (std 0.01) really change between replays and stay finite
DOUT_SCALE = 1e-2       # puts the weight gradients of the BatchNorm'd convolutions at O(1e-3..1)


def backbone(network, seed=0):
    from coclr_amd.backbone.select_backbone import select_backbone
    from test_gpu_infer_plan import _randomise_bn
    torch.manual_seed(seed)
    net, _ = select_backbone(network)
    net = net.cuda().train()
    _randomise_bn(net, seed + 1)
    return net


def clips(n, batch=2, seed=10, clip=CLIP):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(batch, *clip, generator=g) for _ in range(n)]


def holders(net):
    """The modules whose passes went through `engine._plan_entry` (one per autograd node)."""
    return [m for m in net.modules() if "_coclr_plan_entries" in m.__dict__]


def entries(net):
    return [e for m in holders(net) for e in m.__dict__["_coclr_plan_entries"].values()]


def stats():
    from coclr_amd import engine
    s = engine.PLAN_STATS
    return s["recorded"], s["replayed"], len(s["disabled"])


class Twin:
    """One of the two runs of a scenario.  `log` is what the runs are compared on; `replays` (launch-plan replays
    counted by each forward) is bookkeeping of the planned run only."""

    def __init__(self, net, planned):
        self.net, self.planned = net, planned
        self.params = list(net.parameters())
        self.log, self.replays = [], []
        self.held, self.seen_ptrs = [], set()
        self.delta = None
        self.marks = {}

    def upload(self, xs):
        """All inputs on the device before the first step and alive to the end: a distinct address per step."""
        xs = [x.cuda() for x in xs]
        self.held.extend(xs)
        return xs

    def dout(self, y):
        g = torch.Generator().manual_seed(1000 + len(self.log))
        return (torch.randn(y.shape, generator=g) * DOUT_SCALE).cuda()

    def forward(self, x):
        assert x.data_ptr() not in self.seen_ptrs, "step %d reuses an input address" % len(self.log)
        self.seen_ptrs.add(x.data_ptr())
        before = stats()[1]
        y = self.net(x)
        self.replays.append(stats()[1] - before)
        return y

    def grads(self, x=None):
        rec = {"g": [None if p.grad is None else p.grad.clone() for p in self.params]}
        if x is not None and x.requires_grad:
            rec["dx"] = x.grad.clone()
        return rec

    def update(self):
        for p in self.params:
            if p.grad is not None:
                p.data.add_(p.grad, alpha=-LR)
        self.zero()

    def zero(self):
        for p in self.params:
            p.grad = None

    def step(self, x, differentiate=True, update=True, stream=None):
        """Step `len(log)`: forward, backward with the step's seeded dout, gradients kept, weights moved."""
        if stream is not None:
            cur = torch.cuda.current_stream()
            stream.wait_stream(cur)
            with torch.cuda.stream(stream):
                self._pass(x, differentiate)
            cur.wait_stream(stream)
        else:
            self._pass(x, differentiate)
        if differentiate and update:
            self.update()

    def _pass(self, x, differentiate):
        y = self.forward(x)
        rec = {"y": y.detach().clone()}
        if differentiate:
            y.backward(self.dout(y))
            rec.update(self.grads(x))
        self.log.append(rec)

    def state(self):
        return {k: v.detach().clone() for k, v in self.net.state_dict().items()}


def run_twins(build, scenario, monkeypatch):
    """scenario(twin) on the interpreted and on the planned copy of build(); returns (oracle, planned) after
    comparing everything they logged and everything they ended with."""
    from coclr_amd import engine
    assert engine.PLAN, "launch plans are switched off (COCLR_PLAN=0 or no private memory pools)"
    base = build()
    twins = []
    for planned in (False, True):
        monkeypatch.setattr(engine, "PLAN", planned)
        tw = Twin(copy.deepcopy(base), planned)
        s0 = stats()
        disabled0 = list(engine.PLAN_STATS["disabled"])
        scenario(tw)
        torch.cuda.synchronize()
        tw.delta = tuple(b - a for a, b in zip(s0, stats()))
        tw.disabled = engine.PLAN_STATS["disabled"][len(disabled0):]
        tw.final = tw.state()
        twins.append(tw)
    oracle, plan = twins
    assert oracle.delta == (0, 0, 0) and not holders(oracle.net), "the oracle run went through a launch plan"
    assert_same(oracle, plan)
    return oracle, plan


def assert_same(oracle, plan):
    assert len(oracle.log) == len(plan.log) and len(oracle.log) > 0
    for i, (a, b) in enumerate(zip(oracle.log, plan.log)):
        assert a.keys() == b.keys(), "step %d" % i
        assert torch.isfinite(a["y"]).all(), "step %d: the oracle's output is not finite" % i
        assert torch.equal(a["y"], b["y"]), "output of step %d differs from the interpreted pass" % i
        if "dx" in a:
            assert torch.equal(a["dx"], b["dx"]), "input gradient of step %d" % i
        for j, (ga, gb) in enumerate(zip(a.get("g", ()), b.get("g", ()))):
            assert (ga is None) == (gb is None), "step %d, parameter %d: one run has no gradient" % (i, j)
            if ga is not None:
                assert torch.equal(ga, gb), "step %d: gradient of parameter %d" % (i, j)
        for j, (ga, gb) in enumerate(zip(a.get("late", ()), b.get("late", ()))):
            assert torch.equal(ga, gb), "step %d: gradient %d as read after the next forward" % (i, j)
    assert oracle.final.keys() == plan.final.keys()
    for k in oracle.final:
        assert torch.equal(oracle.final[k], plan.final[k]), "%s after the run" % k


def assert_not_vacuous(oracle):
    """The first and the last convolution weight received a gradient that is not zero."""
    convs = [i for i, p in enumerate(oracle.params) if p.dim() == 5]
    for i in (convs[0], convs[-1]):
        got = [rec["g"][i] for rec in oracle.log if "g" in rec and rec["g"][i] is not None]
        assert got and all(torch.isfinite(g).all() for g in got)
        assert max(float(g.abs().max()) for g in got) > 0
