"""torch.optim.Adam / torch.optim.SGD for the launch scripts' parameter structure, as one HIP launch.

main_nce.py:190-200 / main_coclr.py:205-213 build ONE param group per tensor (470 groups for
S3D InfoNCE, 235 of them with gradients) and call `optimizer.step()` (main_nce.py:331): torch's
implementation then runs its per-group loop 470 times -- hundreds of small launches and ~10 ms
of host time per step.  `Adam` below is a drop-in subclass (same constructor, same
`state_dict()` format: per-parameter `step` / `exp_avg` / `exp_avg_sq`) whose `step()` is a
single pointer-table kernel over every tensor (`coclr_adam_step`, csrc/optim.hip).

`install()` (called by the `model.pretrain` shim unless COCLR_PATCH_ADAM=0) makes
`torch.optim.Adam` resolve to this class, so the unmodified launch scripts pick it up.  Anything the
kernel does not cover (CPU parameters, amsgrad, maximize, sparse or non-fp32 tensors, a closure
that needs foreach semantics) goes to torch's own implementation unchanged; for CUDA fp32
parameters there is no silent fallback -- a missing library raises.

`SGD` is the same scheme for the classifier's fine-tuning loop (eval/main_classifier.py:134-140,159:
one param group per tensor, `optim.SGD(params, lr, weight_decay, momentum=0.9)`) over
`coclr_sgd_step`; `install()` (also called by the `model.classifier` shim) resolves `torch.optim.SGD`
to its scoped form unless COCLR_PATCH_SGD=0.
"""
import os
import weakref

import numpy as np
import torch

from . import ops

_CHUNK = 32768          # elements per workgroup
_TorchAdam = torch.optim.Adam
_TorchSGD = torch.optim.SGD
_MOMENTUM_MODELS = weakref.WeakSet()


_OWN_MODELS = weakref.WeakSet()


def register_momentum_model(model):
    """InfoNCE / UberNCE / CoCLR instances announce themselves so that `Adam(fold_momentum=True)`
    can find the (query, key) parameter pairs of model/pretrain.py:76-80."""
    _MOMENTUM_MODELS.add(model)
    _OWN_MODELS.add(model)


def register_model(model):
    """Any module of this package whose parameters the single-launch step may take (the linear-probe
    classifier).  `torch.optim.Adam` / `torch.optim.SGD` resolve to the subclasses process-wide once
    `model.pretrain` or `model.classifier` is imported; optimisers over parameters that belong to NO
    registered module behave exactly as torch's."""
    _OWN_MODELS.add(model)


def _owns_any(params):
    ids = {id(p) for p in params}
    for model in list(_OWN_MODELS):
        for p in model.parameters():
            if id(p) in ids:
                return True
    return False


def _upload_table(plan, gptrs):
    """Launch table of a plan = its static template with this step's gradient addresses in column 1,
    written into one of two pinned host buffers and copied to the device on the current stream
    (the other buffer may still be read by the previous step's copy)."""
    f = plan["flip"]
    ev = plan["events"][f]
    if ev is not None:
        ev.synchronize()                 # the copy that last read this pinned buffer
    tab = plan["host"][f].numpy()
    tab[:] = plan["template"]
    tab[:, 1] = np.asarray(gptrs, dtype=np.int64)[plan["row_param"]] + plan["row_off"]
    plan["table"].copy_(plan["host"][f], non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    plan["events"][f] = ev
    plan["flip"] = 1 - f
    plan["gptrs"] = gptrs


def _kernel_param(p, dev):
    """p (which has a gradient) can be read by the optimiser kernels as flat fp32 memory on `dev`
    (None: not decided yet)."""
    gr = p.grad
    return p.is_cuda and p.dtype == torch.float32 and not gr.is_sparse and \
        gr.dtype == torch.float32 and p.is_contiguous() and gr.is_contiguous() and \
        gr.device == p.device and (dev is None or p.device == dev)


class Adam(_TorchAdam):
    """torch.optim.Adam with a single-launch `step()` on MI355X.

    fold_momentum (default: env COCLR_FOLD_MOMENTUM, off): also compute the momentum-encoder
    update of the NEXT forward (p_k = p_k*m + p_q*(1-m), model/pretrain.py:76-80) in the same
    pass, while the fresh p_q is in registers; the model then skips its own update once.
    Bit-identical in a steady training loop.  Caveat (why it is opt-in): between `step()` and the
    next training forward the key encoder is one momentum step AHEAD of where the reference has
    it -- a checkpoint written in that window, or a no-grad forward, sees the updated keys."""

    _scoped = False     # ScopedAdam: the native step only for parameters of this package's modules

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0,
                 amsgrad=False, *, fold_momentum=None, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                         amsgrad=amsgrad, **kw)
        if fold_momentum is None:
            fold_momentum = os.environ.get("COCLR_FOLD_MOMENTUM", "0") == "1"
        self._fold = bool(fold_momentum)
        self._plan = None
        self._ours = None       # decided at the first step: do these parameters belong to this package?

    # -- eligibility ---------------------------------------------------------------------
    def _native_groups(self):
        """[(group, [params with grad])] if every parameter that has a gradient can take the
        kernel, else None (torch's implementation runs instead)."""
        if self._ours is None:
            self._ours = not self._scoped or os.environ.get("COCLR_ADAM_EVERYWHERE", "0") == "1" or \
                _owns_any(p for g in self.param_groups for p in g["params"])
        if not self._ours:
            return None       # somebody else's model: torch's own implementation, untouched
        out = []
        dev = None
        for g in self.param_groups:
            if g.get("amsgrad") or g.get("maximize") or g.get("differentiable") or \
                    g.get("capturable") or g.get("decoupled_weight_decay") or g.get("fused") or \
                    g.get("foreach") or torch.is_tensor(g["lr"]):
                return None       # options the kernel does not implement, or an explicit torch path
            ps = []
            for p in g["params"]:
                if p.grad is None:
                    continue
                if not _kernel_param(p, dev):
                    return None       # the kernel reads p and p.grad as flat fp32 memory, one device
                dev = p.device
                ps.append(p)
            if ps:
                out.append((g, ps))
        return out if out else None

    # -- plan: static part (params, state, chunking), refreshed when storage moves --------
    def _build_plan(self, groups):
        dev = groups[0][1][0].device
        params, hyper_of = [], []
        for gi, (g, ps) in enumerate(groups):
            for p in ps:
                params.append(p)
                hyper_of.append(gi)
        n = len(params)
        steps = torch.zeros(n, dtype=torch.float32, device=dev)
        host_steps = np.zeros(n, dtype=np.float32)
        for i, p in enumerate(params):
            st = self.state[p]
            if len(st) == 0:
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            else:
                host_steps[i] = float(st["step"])
                for key in ("exp_avg", "exp_avg_sq"):
                    if st[key].device != p.device or st[key].dtype != torch.float32 or \
                            not st[key].is_contiguous():
                        st[key] = st[key].to(device=p.device, dtype=torch.float32).contiguous()
        if host_steps.any():
            steps.copy_(torch.from_numpy(host_steps))
        for i, p in enumerate(params):
            self.state[p]["step"] = steps[i]          # 0-dim device view (torch's fused format)

        fold = None
        kptr = {}
        if self._fold:
            have = {id(p) for p in params}
            for model in list(_MOMENTUM_MODELS):
                pq = [p for p in model.encoder_q.parameters()]
                pk = [p for p in model.encoder_k.parameters()]
                # every (query, key) pair must be folded, or none: the model skips its own update
                # once the optimiser says it has applied it
                if pq and all(p.requires_grad and id(p) in have for p in pq) and \
                        all(k.is_cuda and k.is_contiguous() for k in pk):
                    kptr = {id(q): k for q, k in zip(pq, pk)}
                    fold = weakref.ref(model)
                    break
        rows, row_param, row_off = [], [], []
        for i, p in enumerate(params):
            st = self.state[p]
            k = kptr.get(id(p))
            numel = p.numel()
            for off in range(0, numel, _CHUNK):
                rows.append((p.data_ptr() + 4 * off, 0, st["exp_avg"].data_ptr() + 4 * off,
                             st["exp_avg_sq"].data_ptr() + 4 * off,
                             0 if k is None else k.data_ptr() + 4 * off,
                             min(_CHUNK, numel - off), i, 0))
                row_param.append(i)
                row_off.append(4 * off)
        host = [torch.empty(len(rows), 8, dtype=torch.int64).pin_memory() for _ in range(2)]
        template = np.array(rows, dtype=np.int64).reshape(-1, 8)
        self._plan = {
            "dev": dev, "params": params, "hyper_of": hyper_of, "groups": [g for g, _ in groups],
            "steps": steps, "template": template, "row_param": np.array(row_param, dtype=np.int64),
            "row_off": np.array(row_off, dtype=np.int64), "host": host, "events": [None, None],
            "flip": 0, "table": torch.empty(len(rows), 8, dtype=torch.int64, device=dev),
            "gptrs": None,
            # the kernel's "group" column is the PARAMETER slot (torch keeps one step counter per
            # parameter): hyper rows are the group's values repeated per parameter
            "hyper": torch.empty(n, 8, dtype=torch.float64, device=dev), "hyper_sig": None,
            "ids": torch.arange(n, dtype=torch.int32, device=dev), "n": n,
            "sig": [(p.data_ptr(), self.state[p]["exp_avg"].data_ptr(),
                     self.state[p]["exp_avg_sq"].data_ptr(),
                     0 if kptr.get(id(p)) is None else kptr[id(p)].data_ptr()) for p in params],
            "kparams": [kptr.get(id(p)) for p in params],
            "fold": fold,
            "keep": [self.state[p]["exp_avg"] for p in params] +
                    [self.state[p]["exp_avg_sq"] for p in params] + list(kptr.values()),
        }

    def _plan_valid(self, plan, params):
        """Same parameter objects at the same addresses, optimizer state untouched since the plan
        was built (load_state_dict / .to() replace the state tensors)."""
        if plan is None or len(plan["params"]) != len(params):
            return False
        state = self.state
        steps_ptr = plan["steps"].untyped_storage().data_ptr()
        for a, b, (pp, mp, vp, kp), k in zip(plan["params"], params, plan["sig"], plan["kparams"]):
            if a is not b or b.data_ptr() != pp or (k is not None and k.data_ptr() != kp):
                return False
            st = state[b]
            if not st or st["exp_avg"].data_ptr() != mp or st["exp_avg_sq"].data_ptr() != vp or \
                    not torch.is_tensor(st["step"]) or \
                    st["step"].untyped_storage().data_ptr() != steps_ptr:
                return False
        return True

    # -- step ------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        groups = self._native_groups()
        if groups is None:
            if self._plan is not None:
                # leaving the single-launch path (e.g. a sparse gradient appeared): torch's own
                # implementation wants its per-parameter step counters on the host
                for st in self.state.values():
                    if torch.is_tensor(st.get("step")) and st["step"].is_cuda:
                        st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
                self._plan = None
            super().step()
            return loss
        params = [p for _, ps in groups for p in ps]
        plan = self._plan
        if not self._plan_valid(plan, params):
            self._build_plan(groups)
            plan = self._plan
        # hyper-parameters: uploaded when a group's values change (lr schedules)
        hsig = tuple((g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"])
                     for g, _ in groups)
        if hsig != plan["hyper_sig"]:
            rows = np.zeros((plan["n"], 8), dtype=np.float64)
            for i, gi in enumerate(plan["hyper_of"]):
                rows[i, :5] = hsig[gi]
            plan["hyper"].copy_(torch.from_numpy(rows))
            plan["hyper_sig"] = hsig
        # gradient addresses: autograd hands out fresh tensors every step (zero_grad sets them to
        # None); the caching allocator usually returns the same blocks, so this rarely uploads
        gptrs = [p.grad.data_ptr() for p in params]
        if gptrs != plan["gptrs"]:
            _upload_table(plan, gptrs)
        model = plan["fold"]() if plan["fold"] is not None else None
        m = float(model.m) if model is not None else 0.0
        ops.adam_step(plan["table"], plan["table"].shape[0], plan["hyper"], plan["steps"],
                      plan["ids"], plan["n"], m, 1.0 - m if model is not None else 0.0,
                      keep=plan["keep"])
        if model is not None:
            model.__dict__["_momentum_folded"] = m
        return loss


class ScopedAdam(Adam):
    """What `torch.optim.Adam` resolves to after `install()`: `Adam`, except that an optimiser over
    parameters that belong to NO module of this package (InfoNCE / UberNCE / CoCLR / LinearClassifier
    register themselves) is torch's own implementation, step for step -- importing `model.pretrain`
    must not change how somebody else's model in the same process is optimised.
    `COCLR_ADAM_EVERYWHERE=1` lifts the restriction."""
    _scoped = True


class SGD(_TorchSGD):
    """torch.optim.SGD with a single-launch `step()` on MI355X (`coclr_sgd_step`, csrc/optim.hip).

    eval/main_classifier.py:134-140,159 fine-tunes with one param group per tensor (the backbone at
    lr/10) and `optim.SGD(params, lr, weight_decay, momentum=0.9)`: torch's implementation runs its
    per-group loop over ~233 groups per step.  Same constructor, same `state_dict()` (per-parameter
    `momentum_buffer`, only when momentum != 0), same arithmetic as torch's foreach path.  Anything
    the kernel does not cover (CPU parameters, sparse or non-fp32 gradients, parameters on several
    devices, a tensor lr / weight decay, an explicit `foreach` / `fused`, `differentiable`) runs
    torch's own implementation on the same state; momentum buffers carry over both ways."""

    _scoped = False     # ScopedSGD: the native step only for parameters of this package's modules

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, **kw):
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening,
                         weight_decay=weight_decay, nesterov=nesterov, **kw)
        self._plan = None
        self._ours = None       # decided at the first step: do these parameters belong to this package?

    def _native_groups(self):
        """[(group, [params with grad])] if every parameter that has a gradient can take the
        kernel, else None (torch's implementation runs instead)."""
        if self._ours is None:
            self._ours = not self._scoped or _owns_any(p for g in self.param_groups for p in g["params"])
        if not self._ours or getattr(self, "grad_scale", None) is not None or \
                getattr(self, "found_inf", None) is not None:
            return None
        out = []
        dev = None
        for g in self.param_groups:
            if g.get("differentiable") or g.get("fused") or g.get("foreach") is not None or \
                    any(torch.is_tensor(g[k]) for k in ("lr", "momentum", "dampening", "weight_decay")):
                return None
            ps = []
            for p in g["params"]:
                if p.grad is None:
                    continue
                if not _kernel_param(p, dev):
                    return None       # the kernel reads p and p.grad as flat fp32 memory, one device
                dev = p.device
                ps.append(p)
            if ps:
                out.append((g, ps))
        return out if out else None

    def _build_plan(self, groups):
        dev = groups[0][1][0].device
        params, hyper_of, bufs, rows, row_param, row_off = [], [], [], [], [], []
        first = False
        for gi, (g, ps) in enumerate(groups):
            for p in ps:
                buf = None
                fresh = 0
                if g["momentum"] != 0:
                    st = self.state[p]
                    buf = st.get("momentum_buffer")
                    if buf is None:
                        # torch's first step clones d_p into the buffer: the launch below writes it
                        buf = torch.empty_like(p, memory_format=torch.contiguous_format)
                        fresh = 1
                    elif buf.device != p.device or buf.dtype != torch.float32 or not buf.is_contiguous():
                        buf = buf.to(device=p.device, dtype=torch.float32).contiguous()
                    st["momentum_buffer"] = buf
                i = len(params)
                params.append(p)
                hyper_of.append(gi)
                bufs.append(buf)
                first = first or bool(fresh)
                numel = p.numel()
                for off in range(0, numel, _CHUNK):
                    rows.append((p.data_ptr() + 4 * off, 0, 0 if buf is None else buf.data_ptr() + 4 * off,
                                 min(_CHUNK, numel - off), i, fresh, 0, 0))
                    row_param.append(i)
                    row_off.append(4 * off)
        n = len(params)
        self._plan = {
            "params": params, "hyper_of": hyper_of, "bufs": bufs,
            "sig": [(p.data_ptr(), 0 if b is None else b.data_ptr()) for p, b in zip(params, bufs)],
            "template": np.array(rows, dtype=np.int64).reshape(-1, 8),
            "row_param": np.array(row_param, dtype=np.int64), "row_off": np.array(row_off, dtype=np.int64),
            "host": [torch.empty(len(rows), 8, dtype=torch.int64).pin_memory() for _ in range(2)],
            "events": [None, None], "flip": 0, "gptrs": None, "first": first,
            "table": torch.empty(len(rows), 8, dtype=torch.int64, device=dev),
            # one hyper row per PARAMETER slot (the group's values repeated)
            "hyper": torch.empty(n, 8, dtype=torch.float64, device=dev), "hyper_sig": None, "n": n,
            "keep": [b for b in bufs if b is not None],
        }

    def _plan_valid(self, plan, groups, params):
        """Same parameter objects at the same addresses, the same momentum buffers in the state
        (load_state_dict / torch's own step replace them), momentum switched on for the same ones."""
        if plan is None or len(plan["params"]) != len(params):
            return False
        i = 0
        for g, ps in groups:
            mom = g["momentum"] != 0
            for p in ps:
                pp, bp = plan["sig"][i]
                if plan["params"][i] is not p or p.data_ptr() != pp or mom != (bp != 0):
                    return False
                if mom:
                    buf = self.state[p].get("momentum_buffer")
                    if buf is None or buf.data_ptr() != bp:
                        return False
                i += 1
        return True

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        groups = self._native_groups()
        if groups is None:
            self._plan = None       # torch's step may replace or create momentum buffers
            super().step()
            return loss
        params = [p for _, ps in groups for p in ps]
        plan = self._plan
        if not self._plan_valid(plan, groups, params):
            self._build_plan(groups)
            plan = self._plan
        if plan["template"].shape[0] == 0:
            return loss             # only empty tensors: nothing to update
        # hyper-parameters: uploaded when a group's values change (adjust_learning_rate)
        hsig = tuple((g["lr"], g["momentum"], g["dampening"], g["weight_decay"], bool(g["nesterov"]),
                      bool(g["maximize"])) for g, _ in groups)
        if hsig != plan["hyper_sig"]:
            rows = np.zeros((plan["n"], 8), dtype=np.float64)
            for i, gi in enumerate(plan["hyper_of"]):
                rows[i, :6] = hsig[gi]
            plan["hyper"].copy_(torch.from_numpy(rows))
            plan["hyper_sig"] = hsig
        gptrs = [p.grad.data_ptr() for p in params]
        if gptrs != plan["gptrs"]:
            _upload_table(plan, gptrs)
        ops.sgd_step(plan["table"], plan["table"].shape[0], plan["hyper"], keep=plan["keep"])
        if plan["first"]:
            # the buffers exist now: later steps read them (the table is re-uploaded once)
            plan["template"][:, 5] = 0
            plan["first"] = False
            plan["gptrs"] = None
        return loss


class ScopedSGD(SGD):
    """What `torch.optim.SGD` resolves to after `install()`: `SGD`, except that an optimiser over
    parameters that belong to NO module of this package is torch's own implementation, step for step
    (the ScopedAdam rule)."""
    _scoped = True


def _notice(msg):
    if os.environ.get("COCLR_QUIET", "0") != "1":
        import sys
        print(msg, file=sys.stderr)


def install():
    """Make `torch.optim.Adam` (what main_nce.py:200 / main_coclr.py:213 / eval/main_classifier.py:157
    construct) and `torch.optim.SGD` (eval/main_classifier.py:159) resolve to the single-launch
    subclasses, scoped to this package's models (ScopedAdam / ScopedSGD).  Idempotent;
    COCLR_PATCH_ADAM=0 / COCLR_PATCH_SGD=0 leave the respective torch class untouched.  Returns
    whether Adam is patched."""
    if os.environ.get("COCLR_PATCH_SGD", "1") != "0" and torch.optim.SGD is not ScopedSGD:
        torch.optim.SGD = ScopedSGD
        _notice("coclr_amd: torch.optim.SGD resolves to the single-launch subclass for parameters of "
                "this package's modules (COCLR_PATCH_SGD=0 opts out)")
    if os.environ.get("COCLR_PATCH_ADAM", "1") == "0":
        return False
    if torch.optim.Adam is not ScopedAdam:
        torch.optim.Adam = ScopedAdam
        _notice("coclr_amd: torch.optim.Adam resolves to the single-launch subclass for parameters of "
                "InfoNCE / UberNCE / CoCLR / LinearClassifier modules (COCLR_PATCH_ADAM=0 opts out)")
    return True
