"""Optimizer steps as kernels over the parameter arena.

`ArenaAdamW` is torch.optim.AdamW's update (the reference's MAE / depth drivers:
`Models/mae/main_pretrain.py:179-180` with `add_weight_decay` groups, `train_depth.py:280`) and
`ArenaLARS` the reference's `Models/moco_v3/moco/optimizer.py:18-43`, each as one pass (LARS: norm
pass + apply pass) over the flat fp32 buffers of `engine.ParamArena` — instead of a multi-tensor
launch chain per parameter group.  Both take torch-style parameter groups, keep `param_groups`
(so `lr_sched.adjust_learning_rate` and friends work unchanged) and skip parameters that are frozen
or have no gradient in this step, as torch does.

`get_grad_norm_`, `clip_grad_norm_` and `ArenaAdamW.step(clip_grad=, skip_nonfinite=)` are the rest of
the reference's update (`Models/mae/util/misc.py:251-292`, NativeScalerWithGradNormCount: unscale_ ->
gradient norm / clip -> `scaler.step`): one pass over the gradient arena writes the norm, the clip
coefficient and the non-finite flag into a small device block, and the scale / AdamW kernels read them
there — no per-tensor launches and nothing read back by the host.

The north_star leaves the optimizer step host-side (torch); these are the optional fused variants.
The engine's operand caches are keyed on torch's version counters, which raw-pointer kernels do not
bump: `step()` advances `engine.weights_epoch` instead.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .engine import ParamArena, bump_weights_epoch
from .ops import ptr, stream


def _adopt_grads(a, params):
    """a gradient autograd produced with torch ops lives outside the gradient arena the kernels read:
    move it into the parameter's slice (parallel.DataParallel does the same)"""
    base, index = a.grad.data_ptr(), a._index
    for p in params:
        g = p.grad
        if g is not None and g.data_ptr() != base + 4 * index[id(p)]:  # (no view is built for one in place)
            v = a.grad_view(p)
            v.copy_(g)
            p.grad = v


class _GradNorm:
    """workspace + control block [norm, clip coefficient, found_inf, 0] of the arena norm kernels; the
    tensors handed out are VIEWS of the block: the next pass through the same object overwrites them"""

    def __init__(self, dev):
        L = _lib.load()
        self.ws = torch.empty(L.ssl4gie_grad_norm_workspace_bytes(), dtype=torch.uint8, device=dev)
        self.ctl = torch.zeros(4, device=dev)
        self.norm, self.coef, self.found_inf = self.ctl[0], self.ctl[1], self.ctl[2]

    def run(self, a, start, mask, S, max_norm=None, inv_scale=1.0):
        _lib.check(_lib.load().ssl4gie_grad_norm_arena(
            ptr(a.grad), ptr(start), ptr(mask), S, float(inv_scale), float(max_norm or 0.0), ptr(self.ws),
            ptr(self.ctl), a.numel, stream()), "grad_norm_arena")
        return self.norm

    def scale(self, a, start, mask, S):
        _lib.check(_lib.load().ssl4gie_grad_scale_arena(ptr(a.grad), ptr(start), ptr(mask), S, ptr(self.ctl),
                                                        a.numel, stream()), "grad_scale_arena")


def _norm_pass(target, max_norm, parameters=None):
    """the norm kernel over `target`'s gradients (an _ArenaOptimizer: its own active parameters; a model
    parallel.DataParallel or a ParamArena: every parameter with a gradient, or those of `parameters`
    that have one); with max_norm the gradients are then scaled in place.  Returns the _GradNorm."""
    if isinstance(target, _ArenaOptimizer):
        a = target._arena()
        start, mask, _, _, S = target._build_tables(a)
        gn = target._grad_norm(a)
    else:
        from .parallel import before_optimizer_step
        before_optimizer_step()
        if not isinstance(target, ParamArena) and not hasattr(target, "arena"):
            raise TypeError("get_grad_norm_ / clip_grad_norm_ take an engine model, a parallel.DataParallel "
                            f"or an arena optimizer, not {type(target).__name__}")
        a = target if isinstance(target, ParamArena) else target.arena()
        _adopt_grads(a, a.params)
        chosen = None if parameters is None else {id(p) for p in parameters}
        active = tuple(p.grad is not None and (chosen is None or id(p) in chosen) for p in a.params)
        st = a._grad_norm_state
        if st is None or st["active"] != active:
            # built when the set of parameters with gradients changes, not per step; pinned + non-blocking:
            # no host synchronisation
            host = (torch.tensor(list(a.offsets) + [a.numel], dtype=torch.int64).pin_memory(),
                    torch.tensor([1.0 if on else -1.0 for on in active]).pin_memory())
            gn = st["gn"] if st is not None else _GradNorm(a.data.device)
            st = {"active": active, "host": host, "gn": gn,
                  "dev": tuple(h.to(a.data.device, non_blocking=True) for h in host)}
            a._grad_norm_state = st
        (start, mask), S, gn = st["dev"], len(a.params), st["gn"]
    gn.run(a, start, mask, S, max_norm)
    if max_norm is not None:
        gn.scale(a, start, mask, S)
    return gn


@torch.no_grad()
def get_grad_norm_(model_or_optimizer):
    """L2 norm of all gradients (the reference's `misc.get_grad_norm_`, `misc.py:280-292`, norm_type 2)
    as a 0-d device tensor: ONE pass over the gradient arena, bit-identical from run to run, no host
    synchronisation.  An open data-parallel pass is closed first (the norm is that of the reduced
    gradients) and gradients living outside the arena are adopted.  The result is a view of a device
    block the next call overwrites: read or copy it before calling again."""
    return _norm_pass(model_or_optimizer, None).norm


@torch.no_grad()
def clip_grad_norm_(model_or_optimizer, max_norm):
    """`torch.nn.utils.clip_grad_norm_(parameters, max_norm)` over the arena: gradients are multiplied in
    place by min(1, max_norm / (norm + 1e-6)) (nothing is written when that is 1); returns the norm
    BEFORE clipping as a 0-d device tensor (same caveats as `get_grad_norm_`).  One difference from
    torch: max_norm <= 0 means "no clipping" (coefficient exactly 1, the kernels' convention), where
    torch would scale the gradients to zero."""
    return _norm_pass(model_or_optimizer, float(max_norm)).norm


class _ArenaOptimizer:
    """Base of the arena optimizers.  Each steps over a HULL (i0, i1, lo, hi) of the arena: the segments [i0, i1) and the
    elements [lo, hi) they span.  State buffers and launches cover the hull only: the kernels get `hi - lo` elements and
    a segment table rebased to `lo`; a parameter inside the hull that is not the optimizer's is inactive through
    seg_lr < 0, as a frozen one is.  By default the hull is the whole arena, (0, S, 0, numel).  A `_ranged` class (a
    linear probe's head: 0.77 M of ViT-B's 86 M elements) takes the hull of its own parameters; its `model` may be None:
    the arena is then found from the parameters (engine.arena_of) at step(), because a model builds its arena lazily."""

    _ranged = False
    _state_names = ()

    def __init__(self, model, params, defaults):
        self.model = model
        if isinstance(params, (list, tuple)) and params and isinstance(params[0], dict):
            groups = [dict(g) for g in params]
        else:
            groups = [{"params": list(params)}]
        for g in groups:
            g["params"] = list(g["params"])
            for k, v in defaults.items():
                g.setdefault(k, v)
        self.param_groups = groups
        self.defaults = dict(defaults)
        self._tables_key = None
        self._hyper = None
        self._hull_key = self._hull = None
        self._gn = None            # _GradNorm of get_grad_norm_ / clip_grad_norm_ / step(clip_grad=) through self
        self.step_count = 0

    def _own(self):
        return [p for g in self.param_groups for p in g["params"]]

    # ------------------------------------------------------------------ segment tables
    def _arena(self):
        # torch optimizers get this through the global pre-step hook parallel.py registers: close any
        # data-parallel pass still open and wait for the comm stream before gradients are read
        from .engine import arena_of
        from .parallel import before_optimizer_step
        before_optimizer_step()
        own = self._own()
        # ranged: pointer checks on the own parameters only, no walk over the model's parameters per step
        a = arena_of(own) if self._ranged else None
        if a is None:  # (ranged: not built yet, or the parameters moved) the model validates / rebuilds it
            if self.model is None:
                raise RuntimeError(f"{type(self).__name__}: its parameters do not live in one live engine arena (run a "
                                   "forward on the device first: the arena is built lazily)")
            a = self.model.arena()
            assert all(a.owns(p) for p in own), "every optimised parameter must live in the model's arena"
        _adopt_grads(a, own)
        return a

    def _grad_norm(self, a):
        if self._gn is None or self._gn.ctl.device != a.data.device:
            self._gn = _GradNorm(a.data.device)
        return self._gn

    def _build_tables(self, a, keep_active=False):
        """device tables [start | lr | wd | is_matrix] per arena parameter.  The layout (start, mat)
        and the active mask are rebuilt only when the arena or the set of parameters with gradients
        changes; a per-iteration learning-rate schedule (`lr_sched.adjust_learning_rate`) only
        rewrites the small pinned host tables and refreshes the device copies with two non-blocking
        copies on the compute stream — no host synchronisation per step.  keep_active: the ACTIVE mask
        of the previous step stays (gradients do not exist yet while the backward pass is running)."""
        n = len(a.params)
        hyper = tuple((g["lr"], g["weight_decay"]) for g in self.param_groups)
        if not keep_active:
            group_of = {id(p): gi for gi, g in enumerate(self.param_groups) for p in g["params"]}
            active = tuple(id(p) in group_of and p.requires_grad and p.grad is not None for p in a.params)
            if (id(a), active) != self._tables_key:
                dev = a.data.device
                pin = dev.type == "cuda"
                start = torch.tensor(list(a.offsets) + [a.numel], dtype=torch.int64)
                mat = torch.tensor([1.0 if (active[i] and p.ndim > 1) else 0.0 for i, p in enumerate(a.params)])
                if pin:  # kept alive in _host_layout: the copies below do not wait for the host
                    start, mat = start.pin_memory(), mat.pin_memory()
                self._host_layout = (start, mat)
                self._host = (torch.empty(n, pin_memory=pin), torch.empty(n, pin_memory=pin))
                self._dev = [start.to(dev, non_blocking=pin), torch.empty(n, device=dev), torch.empty(n, device=dev),
                             mat.to(dev, non_blocking=pin)]
                self._gidx = [group_of.get(id(p), -1) if active[i] else -1 for i, p in enumerate(a.params)]
                self._tables_key, self._hyper = (id(a), active), None
        if hyper != self._hyper:
            lr_h, wd_h = self._host
            lrs = [hyper[gi][0] if gi >= 0 else -1.0 for gi in self._gidx]
            wds = [hyper[gi][1] if gi >= 0 else 0.0 for gi in self._gidx]
            lr_h.copy_(torch.tensor(lrs))
            wd_h.copy_(torch.tensor(wds))
            self._dev[1].copy_(lr_h, non_blocking=True)
            self._dev[2].copy_(wd_h, non_blocking=True)
            self._hyper = hyper
        return tuple(self._dev) + (n,)

    def _tables(self, a, keep_active=False):
        """-> (start - lo [S + 1], lr [S], wd [S], mat [S], S, lo, hi) over the hull's S segments: slices of the
        whole-arena tables (a learning-rate schedule still only rewrites those), cut once per layout"""
        start, lr, wd, mat, n = self._build_tables(a, keep_active)
        if self._hull_key != self._tables_key:
            i0, i1 = 0, n
            if self._ranged:
                own = {id(p) for p in self._own()}
                idx = [i for i, p in enumerate(a.params) if id(p) in own]
                i0, i1 = min(idx), max(idx) + 1
            lo = a.offsets[i0]
            hi = a.offsets[i1] if i1 < n else a.numel
            rstart = (start[i0:i1 + 1] - lo).contiguous() if lo else start[i0:i1 + 1]
            self._hull = (rstart, lr[i0:i1], wd[i0:i1], mat[i0:i1], i1 - i0, lo, hi)
            self._hull_key = self._tables_key
        return self._hull

    def _state(self, name, a, lo, hi):
        """the hull-sized fp32 state buffer `name` on the arena's device (zeros when fresh).  A buffer of another
        size: the whole-arena optimizers start over with zeros (the arena was rebuilt), a ranged one refuses."""
        v = getattr(self, name)
        if v is None or (not self._ranged and v.numel() != hi - lo):
            v = torch.zeros(hi - lo, dtype=torch.float32, device=a.data.device)
        elif v.numel() != hi - lo:
            raise ValueError(f"{type(self).__name__}.{name} holds {v.numel()} elements, the hull of its parameters "
                             f"{hi - lo}: the state was saved for a different arena layout")
        elif v.device != a.data.device:
            v = v.to(a.data.device)
        setattr(self, name, v)
        return v

    def _finish_step(self, count=True):
        if count:
            self.step_count += 1
        bump_weights_epoch(touched=self._own())

    # ------------------------------------------------------------------ checkpointing
    def state_dict(self):
        """moments / momentum as flat hull-shaped fp32 tensors + step count + param_groups (without
        the parameter objects) — what `save_model` (`Models/mae/util/misc.py:301-307`) and
        `main_moco.py:310-316` store under "optimizer" for `--resume`"""
        groups = [{k: v for k, v in g.items() if k != "params"} | {"n_params": len(g["params"])}
                  for g in self.param_groups]
        state = {k: getattr(self, k) for k in self._state_names}
        return {"kind": type(self).__name__, "step_count": self.step_count, "param_groups": groups,
                "state": {k: (v.detach().clone() if v is not None else None) for k, v in state.items()}}

    def load_state_dict(self, sd):
        """the whole-arena optimizers check the buffers' size against the arena here; a ranged one at its next
        step() (its arena may not exist yet)"""
        assert sd["kind"] == type(self).__name__, (sd["kind"], type(self).__name__)
        assert len(sd["param_groups"]) == len(self.param_groups)
        for g, saved in zip(self.param_groups, sd["param_groups"]):
            assert saved["n_params"] == len(g["params"]), "parameter groups differ from the saved ones"
            g.update({k: v for k, v in saved.items() if k != "n_params"})
        a = None if self._ranged else self._arena()
        for k in self._state_names:
            v = sd["state"].get(k)
            if v is not None:
                assert a is None or v.numel() == a.numel, "optimizer state was saved for a different arena layout"
                v = v.detach().to(device=None if a is None else a.data.device, dtype=torch.float32).clone()
            setattr(self, k, v)
        self.step_count = int(sd["step_count"])
        self._hyper = None

    def zero_grad(self, set_to_none: bool = True):
        for g in self.param_groups:
            for p in g["params"]:
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()


class ArenaAdamW(_ArenaOptimizer):
    """`ArenaAdamW(model, params_or_groups, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
    overlap_backward=False)`

    overlap_backward: the update of a transformer block's parameters is enqueued on a side stream as
    soon as that block's backward kernels are (engine.GradSink.tracker), so it runs behind the rest of
    the backward pass in the CUs the data-gradient chain leaves idle; `step()` then updates whatever is
    left and joins the streams.  Same arithmetic, same result.  It engages from the second step on
    (the first one learns which parameters get gradients), only while every parameter is used ONCE per
    backward pass (two-view models accumulate over uses), never with gradient accumulation over
    several backward passes, and not under parallel.DataParallel (which owns the tracker: its
    gradient all-reduce has to come first).  Measured on the MAE ViT-B step it does NOT pay (24.1 vs
    23.9-24.0 ms, same box): the HBM-bound update competes with the backward GEMMs' operand traffic for
    about what it hides.  Kept, off by default, because the result is bitwise the plain step's
    (tests/test_gpu_optim.py) and a model with more idle CUs in its backward may differ.

    `step(clip_grad=None, skip_nonfinite=False)`: with either option the step is the reference scaler's
    update (`Models/mae/util/misc.py:259-268`) in three launches: the arena norm pass, the AdamW kernel
    reading its control block, and a one-thread counter update.  clip_grad: the update uses
    min(1, clip_grad / (norm + 1e-6)) * g, torch's `clip_grad_norm_` coefficient.  skip_nonfinite: if
    any active gradient element is inf or NaN NOTHING is updated (parameters, moments, bf16 copies) and
    the bias-correction step does not advance — `GradScaler.step`'s skip, decided on the device.
    `last_grad_norm` / `last_found_inf` are 0-d device tensors (views the next such step overwrites).
    On this fused path `p.grad` is left UNSCALED (torch's clip_grad_norm_ scales it in place; use
    `optim.clip_grad_norm_` + `step()` where the clipped gradient itself is needed) — the reference
    loop zeroes the gradients straight after the step.  Once such a step has been taken the count of
    applied updates lives on the device; `step_count` / `state_dict()` read it back (a synchronisation,
    at checkpoint time only).  Both options need every gradient before the first update: together with
    overlap_backward=True they raise ValueError."""

    _state_names = ("exp_avg", "exp_avg_sq")

    def __init__(self, model, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 overlap_backward=False):
        self._host_steps = 0       # count of applied updates while it lives on the host ...
        self._dev_steps = None     # ... and once a step(clip_grad= / skip_nonfinite=) moved it to the device
        self._ctl_plain = None     # control block [0, 1, 0, 0] of a plain step() behind the device-side count
        super().__init__(model, params, dict(lr=lr, weight_decay=weight_decay))
        self.betas, self.eps = betas, eps
        self.exp_avg = self.exp_avg_sq = None
        self._overlap = bool(overlap_backward)
        self._stream = None        # side stream of the in-backward updates
        self._done = []            # [lo, hi) ranges already updated in the current step
        self._step_tables = None   # device tables of the current step (built at its first use)
        self._seen = {}            # id(p) -> tracker calls in the current pass
        self._hooked = False
        self._lp = None
        self.last_grad_norm = self.last_found_inf = None

    # ------------------------------------------------------------------ count of applied updates
    # host-side until the first step(clip_grad= / skip_nonfinite=); then ONE int32 on the device, which
    # the device-counted kernel reads and advances (a skipped update must not advance the bias corrections)
    @property
    def step_count(self):
        return self._host_steps if self._dev_steps is None else int(self._dev_steps.item())

    @step_count.setter
    def step_count(self, n):
        self._host_steps = int(n)
        if self._dev_steps is not None:
            self._dev_steps.fill_(int(n))

    # ------------------------------------------------------------------ in-backward updates
    def _hook(self):
        if self._overlap and not self._hooked:
            sink = self.model.sink()
            if sink.tracker is None:
                sink.tracker = self._on_use_done
                self._hooked = True
            else:
                self._overlap = False  # somebody else (DataParallel) owns the engine's call-back

    def zero_grad(self, set_to_none: bool = True):
        super().zero_grad(set_to_none)
        self._hook()
        self._done, self._seen, self._step_tables = [], {}, None

    def _launch(self, a, lo, hi, st, ctl=None, skip_nonfinite=False):
        """the update of the elements [lo, hi): host-counted, or with `ctl` behind the control block and the device-side
        count, which it then advances"""
        start, lr, wd, _, S, _, _ = self._step_tables
        counted = ctl is not None
        _lib.check(_lib.load().ssl4gie_adamw_arena(
            ptr(a.data), ptr(a.grad), ptr(self.exp_avg), ptr(self.exp_avg_sq), ptr(start), ptr(lr), ptr(wd), S,
            self.betas[0], self.betas[1], self.eps, 0 if counted else self._host_steps + 1,
            ptr(self._dev_steps) if counted else 0, lo, hi, ptr(self._lp), ptr(ctl), int(bool(skip_nonfinite)),
            int(counted), st), "adamw_arena")

    @torch.no_grad()
    def _on_use_done(self, params):
        if not self._overlap or self.exp_avg is None or self._tables_key is None:
            return  # first step: plain update in step()
        for p in params:
            n = self._seen.get(id(p), 0) + 1
            self._seen[id(p)] = n
            if n > 1:  # a second use in one pass: gradients still accumulating — not this model
                self._overlap = False
                return
        a = self.model.arena()
        lo, hi = a.span(params)
        inside = [q for q, o in zip(a.params, a.offsets) if lo <= o < hi]
        ids = {id(p) for p in params}
        if any(id(q) not in ids for q in inside) or any(lo < h and l < hi for l, h in self._done):
            return  # not a contiguous run of exactly these parameters: left to step()
        if self._step_tables is None:
            self._lp = a.lp_flat_for_update()
            self._step_tables = self._tables(a, keep_active=True)
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=a.data.device)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(a.data.device))  # the block's backward, incl. its dW join
        self._stream.wait_event(ev)
        # ... unless the block's dW products were left on the library's weight-gradient stream
        # (SSL4GIE_BWD_NO_JOIN): wait for the latest block of either slot, as DataParallel does
        L = _lib.load()
        for slot in (0, 1):
            L.ssl4gie_wgrad_wait(slot, self._stream.cuda_stream)
        self._launch(a, lo, hi, self._stream.cuda_stream)
        self._done.append((lo, hi))

    def _step_ctl(self, a, clip_grad, skip_nonfinite):
        """norm pass (when an option asks for it) + the AdamW kernel behind the control block"""
        start, lr, _, _, S, lo, hi = self._step_tables
        dev = a.data.device
        if self._dev_steps is None:
            self._dev_steps = torch.full((1,), self._host_steps, dtype=torch.int32, device=dev)
        elif self._dev_steps.device != dev:  # the model moved: the count follows it (a copy between devices)
            self._dev_steps = self._dev_steps.to(dev)
        if clip_grad is not None or skip_nonfinite:
            gn = self._grad_norm(a)
            gn.run(a, start, lr, S, clip_grad)
            self.last_grad_norm, self.last_found_inf = gn.norm, gn.found_inf
            ctl = gn.ctl
        else:  # a plain step() after the counter moved to the device: coefficient 1, nothing found
            if self._ctl_plain is None or self._ctl_plain.device != dev:
                self._ctl_plain = torch.zeros(4, device=dev)
                self._ctl_plain[1] = 1.0
            ctl = self._ctl_plain
        self._launch(a, lo, hi, stream(), ctl, skip_nonfinite)

    @torch.no_grad()
    def step(self, clip_grad=None, skip_nonfinite=False):
        ctl_path = clip_grad is not None or skip_nonfinite
        if ctl_path and self._overlap:
            raise ValueError("ArenaAdamW(overlap_backward=True) applies updates while the backward pass is "
                             "still running; clip_grad / skip_nonfinite need the norm of EVERY gradient first")
        a = self._arena()
        key_before = self._tables_key
        tables = self._tables(a)
        if self._done and self._tables_key != key_before:
            raise RuntimeError("ArenaAdamW(overlap_backward=True): the set of parameters with gradients "
                               "changed between steps after part of this step was already applied")
        self._step_tables = tables
        lo, hi = tables[5:]
        for name in self._state_names:
            self._state(name, a, lo, hi)
        # the kernels also write the bf16 operand copy of what they update into the arena's flat shadow
        # (engine.ParamArena.lp_views): the next forward then only needs the batched transposes
        self._lp = a.lp_flat_for_update() if a.data.is_cuda else None
        counted = ctl_path or self._dev_steps is not None
        if counted:
            assert not self._done, "in-backward updates and the device-side step count do not mix"
            self._step_ctl(a, clip_grad, skip_nonfinite)
        else:
            st = stream()
            pos = lo
            for l, h in sorted(self._done) + [(hi, hi)]:  # the complement of the ranges done
                if l > pos:
                    self._launch(a, pos, l, st)
                pos = max(pos, h)
            if self._done:
                torch.cuda.current_stream(a.data.device).wait_stream(self._stream)
        self._done, self._seen, self._step_tables = [], {}, None
        self._finish_step(count=not counted)
        if self._lp is not None:
            a.lp_flat_is_current()


class _LARS(_ArenaOptimizer):
    """the LARS step over the hull: the three launches of ssl4gie_lars_arena, a hull-sized momentum buffer and
    workspace.  A subclass says where momentum and trust coefficient are kept."""

    _state_names = ("mu",)
    mu = _ws = None

    def _momentum_trust(self):
        raise NotImplementedError

    @torch.no_grad()
    def step(self):
        a = self._arena()
        start, lr, wd, mat, S, lo, hi = self._tables(a)
        mu = self._state("mu", a, lo, hi)
        L = _lib.load()
        nbytes = L.ssl4gie_lars_workspace_bytes(S)
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != a.data.device:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=a.data.device)
        momentum, trust = self._momentum_trust()
        _lib.check(L.ssl4gie_lars_arena(ptr(a.data) + 4 * lo, ptr(a.grad) + 4 * lo, ptr(mu), ptr(start), ptr(lr),
                                        ptr(wd), ptr(mat), S, float(momentum), float(trust), ptr(self._ws), hi - lo,
                                        stream()), "lars_arena")
        self._finish_step()


class ArenaLARS(_LARS):
    """`ArenaLARS(model, params_or_groups, lr=0, weight_decay=0, momentum=0.9, trust_coefficient=0.001)`: the
    reference's `Models/moco_v3/moco/optimizer.py:18-43` over the whole arena"""

    def __init__(self, model, params, lr=0.0, weight_decay=0.0, momentum=0.9, trust_coefficient=0.001):
        super().__init__(model, params, dict(lr=lr, weight_decay=weight_decay))
        self.momentum, self.trust = momentum, trust_coefficient

    def _momentum_trust(self):
        return self.momentum, self.trust


class RangedLARS(_LARS):
    """ArenaLARS's update over the hull of its parameters only: a hull-sized momentum buffer and workspace instead of
    arena-sized ones; momentum and trust coefficient are parameter-group defaults, as in the reference's signature,
    which `Models/mae/util/lars.py` gives it."""

    _ranged = True

    def __init__(self, model, params, lr=0.0, weight_decay=0.0, momentum=0.9, trust_coefficient=0.001):
        super().__init__(model, params, dict(lr=lr, weight_decay=weight_decay, momentum=momentum,
                                             trust_coefficient=trust_coefficient))
        if any(g["momentum"] != self.param_groups[0]["momentum"] or
               g["trust_coefficient"] != self.param_groups[0]["trust_coefficient"] for g in self.param_groups):
            raise NotImplementedError("LARS: momentum and trust_coefficient must be the same in every group")

    def _momentum_trust(self):
        g0 = self.param_groups[0]
        return g0["momentum"], g0["trust_coefficient"]


class ArenaSGD(_ArenaOptimizer):
    """`ArenaSGD(model, params_or_groups, lr, momentum=0, weight_decay=0)`: torch.optim.SGD as the linear-probe driver
    builds it (`Models/moco_v3/main_lincls.py:236-238`: momentum 0.9, weight decay 0 over fc's two parameters) in ONE
    launch of ssl4gie_sgd_arena over the hull of its parameters: d = g + wd p; buf = momentum buf + d; p -= lr buf.
    The momentum buffer starts at zero, which reproduces torch's first step (buf = d).  Nesterov momentum and
    dampening are not built."""

    _ranged = True
    _state_names = ("buf",)

    def __init__(self, model, params, lr, momentum=0.0, weight_decay=0.0, dampening=0.0, nesterov=False):
        if dampening != 0 or nesterov:
            raise NotImplementedError("ArenaSGD: dampening != 0 and nesterov=True are not built (DESIGN.md §8)")
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("ArenaSGD: lr, momentum and weight_decay must be >= 0")
        super().__init__(model, params, dict(lr=lr, weight_decay=weight_decay))
        self.momentum = float(momentum)
        self.buf = None

    @torch.no_grad()
    def step(self):
        a = self._arena()
        start, lr, wd, _, S, lo, hi = self._tables(a)
        buf = self._state("buf", a, lo, hi)
        _lib.check(_lib.load().ssl4gie_sgd_arena(ptr(a.data) + 4 * lo, ptr(a.grad) + 4 * lo, ptr(buf), ptr(start),
                                                 ptr(lr), ptr(wd), S, self.momentum, hi - lo, stream()), "sgd_arena")
        self._finish_step()
