"""Adam / AdamW over the flat parameter buffer.

The reference uses ``torch.optim.Adam(lr)`` (beta=(0.9,0.999), eps=1e-8,
weight_decay=0) stepped per batch and ``MultiStepLR(milestones, 0.1)`` stepped
per epoch (``distribute_train.py:99-110``).  ``FlatAdam`` is numerically the
same update but owns flat fp32 moment buffers aligned with
``parallel.FlatParameters`` so one fused HIP kernel (``ops.adam``) updates all
35.2M trainable parameters per step; it also folds the data-parallel 1/world
gradient average into that pass.  AdamW is the same kernel with decoupled
decay (``weight_decay > 0``); the default 0 keeps parity with the reference.

It subclasses ``torch.optim.Optimizer`` so torch LR schedulers drive every
group's ``lr`` and ``state_dict()`` is emitted in torch-Adam layout
(per-parameter ``step``/``exp_avg``/``exp_avg_sq``, one entry per group) for
Lightning-format checkpoints.

Parameter groups (``groups=[{"params", "name", "lr", "weight_decay"}, ...]``, at
most 16): the groups are scattered through the gradient-ready-order flat buffer,
so the group is looked up per 64-element chunk inside the one launch
(``ops.adam.flat_adam_dev_step`` given ``chunk_group`` uint8 per chunk and
``group_state`` fp32 ``[G, 4] = {lr, wd, 0, 0}`` on the device).  While every group
holds the same ``(lr, weight_decay)`` -- the single default group always does --
the step runs the ungrouped form, to which the grouped one is bitwise equal
group by group; a capture with more than one group always records the grouped
form, so a later scheduler step cannot invalidate the graph.
``build_param_groups`` makes the usual groups from a model: no weight decay on
norms, biases and embeddings, a smaller learning rate on the pretrained backbone.

Per-step schedule (``lr_schedule=dict(kind, warmup_steps, decay_steps, min_lr_ratio)``, off by default): linear warm-up,
then constant / linear / cosine / inverse-sqrt decay, as one factor ``lr_factor(t)`` on every group's base lr.  Nothing
per step comes from the host: one tiny launch in front of the Adam launch (``ops.adam.lr_schedule_dev``) forms the
factor on the device from the effective Adam step ``t`` -- the ``t`` of the bias corrections and of the EMA warm-up,
which does not count skipped steps -- and writes ``base_g * f`` where the Adam kernels read their lr.  ``param_groups``
keep the base learning rates, so ``MultiStepLR`` composes with it.

Layer-wise trust ratios (``layer_adapt=True``, off by default; LAMB, You et al. 2020): every tensor's Adam direction
``u = m_hat / (sqrt(v_hat) + eps) + wd * p`` is applied with the step ``lr * ||p|| / ||u||`` (the ratio is 1 when either
norm is 0 and for the tensors of a group that says ``layer_adapt: False`` -- ``build_param_groups`` says so for the
no-decay groups).  Three launches take the place of the Adam launch (``ops.adam.flat_lamb_dev_step``); clipping, the
schedule, the EMA and the groups work as before, and ``m, v`` and the step are Adam's, so checkpoints are
interchangeable.
"""
from __future__ import annotations

import math
import warnings
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ..parallel.flat import ALIGN, FlatParameters

MAX_GROUPS = 16          # ops.adam.MAX_GROUPS: group_state is at most [16, 4]
DEFAULT_GROUP = "all"    # how an unnamed group (the single default one) is called in lrs / layouts
LR_SCHEDULE_KINDS = ("constant", "linear", "cosine", "rsqrt")    # ops.adam.SCHED_KINDS, in the kernel's order


def lr_factor(kind: str, t, warmup, decay, min_ratio) -> float:
    """The per-step schedule factor of the effective Adam step ``t >= 1`` (skipped steps do not count), in fp64 -- the
    formula ``csrc/kernels/lr_schedule.hip`` evaluates on the device, operation by operation.  With ``W = warmup``,
    ``N = decay``, ``r = min_ratio``: ``t / W`` while ``t <= W`` (``W > 0``), then with
    ``q = min(1, (t - W) / (N - W))``

    * ``constant``: 1;
    * ``linear``: ``1 - (1 - r) q``;
    * ``cosine``: ``r + (1 - r) (1 + cos(pi q)) / 2``;
    * ``rsqrt``: ``max(r, sqrt(max(W, 1) / t))`` (``N`` unused).

    At ``q = 1`` the decaying kinds return ``r`` itself, not a rounding of it."""
    if kind not in LR_SCHEDULE_KINDS:
        raise ValueError(f"lr schedule kind must be one of {LR_SCHEDULE_KINDS}, got {kind!r}")
    t, W, N, r = float(t), float(warmup), float(decay), float(min_ratio)
    if not t >= 1.0:
        raise ValueError(f"the Adam step t must be >= 1, got {t!r}")
    if W > 0.0 and t <= W:
        return t / W
    if kind == "constant":
        return 1.0
    if kind == "rsqrt":
        return max(r, math.sqrt(max(W, 1.0) / t))
    q = (t - W) / (N - W)
    if q >= 1.0:
        return r
    if kind == "linear":
        return 1.0 - (1.0 - r) * q
    return r + (1.0 - r) * (1.0 + math.cos(math.pi * q)) * 0.5


def checked_lr_schedule(schedule: Optional[dict]) -> Optional[dict]:
    """``None`` (or kind ``"none"``): no schedule.  Otherwise the schedule as a dict of Python scalars
    ``{kind, warmup_steps, decay_steps, min_lr_ratio}`` after the refusals the kernel binding makes too."""
    if schedule is None or schedule.get("kind") in (None, "none"):
        return None
    extra = set(schedule) - {"kind", "warmup_steps", "decay_steps", "min_lr_ratio"}
    if extra:
        raise ValueError(f"lr_schedule has unknown keys {sorted(extra)}")
    kind = schedule["kind"]
    W, N, r = schedule.get("warmup_steps", 0), schedule.get("decay_steps", 0), schedule.get("min_lr_ratio", 0.0)
    if kind not in LR_SCHEDULE_KINDS:
        raise ValueError(f"lr_schedule kind must be one of {LR_SCHEDULE_KINDS} (or None), got {kind!r}")
    for name, v in (("warmup_steps", W), ("decay_steps", N)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"lr_schedule {name} must be an integer, got {v!r}")
    if W < 0:
        raise ValueError(f"lr_schedule warmup_steps must be >= 0, got {W!r}")
    if kind in ("linear", "cosine") and not N > W:
        raise ValueError(f"lr_schedule decay_steps must be > warmup_steps ({W}) for the {kind} schedule, got {N!r}")
    if not 0.0 <= float(r) <= 1.0:
        raise ValueError(f"lr_schedule min_lr_ratio must be in [0, 1], got {r!r}")
    return dict(kind=kind, warmup_steps=int(W), decay_steps=int(N), min_lr_ratio=float(r))


class FlatAdam(torch.optim.Optimizer):
    def __init__(self, flat: FlatParameters, lr: float = 5e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, all_params: Optional[Sequence[torch.nn.Parameter]] = None,
                 use_kernel: Optional[bool] = None, max_grad_norm: Optional[float] = None,
                 skip_nonfinite: bool = False, ema_decay: float = 0.0, ema_warmup: bool = True,
                 param_names: Optional[Dict[int, str]] = None, groups: Optional[Sequence[dict]] = None,
                 lr_schedule: Optional[dict] = None, layer_adapt: bool = False):
        lr_schedule = checked_lr_schedule(lr_schedule)
        if not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1) (0 = off), got {ema_decay!r}")
        self.flat = flat
        params = list(all_params) if all_params is not None else list(flat.params)
        decoupled = weight_decay > 0
        group_adapt = None
        if groups is not None:
            params = self._checked_groups(groups, params)
            decoupled = any(g.get("weight_decay", weight_decay) > 0 for g in params)
            # a group's layer_adapt flag is a property of the run, not of the checkpoint: it is kept here and the
            # param_groups (and with them state_dict()) hold the keys they always held
            group_adapt = [bool(g.pop("layer_adapt", True)) for g in params]
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                                      maximize=False, foreach=None, capturable=False, differentiable=False,
                                      fused=None, decoupled_weight_decay=decoupled))
        self.exp_avg = torch.zeros_like(flat.data)
        self.exp_avg_sq = torch.zeros_like(flat.data)
        self.step_count = 0
        # device-resident step counter + group 0's lr so a captured graph replays correctly
        self.dev_state = torch.zeros(2, dtype=torch.float32, device=flat.data.device)
        self._dev_groups = None     # ((lr, weight_decay), ...) per group as last written to the device
        self._dev_step = None
        # more than one group: the group of every 64-element chunk of the flat buffer (a parameter's padding belongs
        # to it; frozen parameters have no chunks) and the groups' {lr, wd, 0, 0} on the device
        self.chunk_group = self.group_state = None
        self._elem_cache = None     # CPU / no-kernel path: (host groups, lr per element, wd per element)
        if len(self.param_groups) > 1:
            group_of = {id(p): gi for gi, g in enumerate(self.param_groups) for p in g["params"]}
            table = torch.zeros(flat.numel // ALIGN, dtype=torch.uint8)
            ends = list(flat.offsets[1:]) + [flat.numel]
            for p, o, e in zip(flat.params, flat.offsets, ends):
                table[o // ALIGN:e // ALIGN] = group_of[id(p)]
            self.chunk_group = table.to(flat.data.device)
            self.group_state = torch.zeros(len(self.param_groups), 4, dtype=torch.float32, device=flat.data.device)
        self._kernel = None
        if use_kernel is None:
            use_kernel = flat.data.is_cuda
        if use_kernel:
            from ..ops import adam as adam_ops
            self._kernel = adam_ops
        # global-norm clipping / non-finite step skip, decided on the device (ops.adam.grad_norm_clip_): clip_state is
        # fp32[8] = {norm, coef, ok, skipped steps, clipped steps, consecutive skipped steps, 0, 0} on every backend
        self.max_grad_norm = float(max_grad_norm) if max_grad_norm is not None and max_grad_norm > 0 else 0.0
        self.skip_nonfinite = bool(skip_nonfinite)
        self.clip_enabled = self.max_grad_norm > 0.0 or self.skip_nonfinite
        self.clip_state = None
        self._partials = None
        if self.clip_enabled:
            self.clip_state = torch.zeros(8, dtype=torch.float32, device=flat.data.device)
            if self._kernel is not None:
                self._partials = torch.zeros(self._kernel.gradnorm_partials(flat.grad.numel()), dtype=torch.float64,
                                             device=flat.data.device)
        # exponential moving average of the trainable weights (off at 0): one more flat fp32 buffer, updated by the
        # same launch as Adam (flat_adam_dev_step given ema).  ema_state is fp32[4] = {omd_t of the last applied
        # update, its Adam step t, 0, 0} with omd = 1 - decay; under warm-up omd_t = max(omd, 9 / (10 + t)), i.e. the
        # decay min(decay, (1 + t) / (10 + t)).  BN running statistics and frozen parameters are not in the flat buffer
        # and are not averaged (torch.optim.swa_utils.AveragedModel's default).  The buffer is fp32: at decay 0.9999
        # an update with |p - ema| below about 1e-3 |ema| moves it by less than an ulp (as in timm and torch).
        self.ema_decay = float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self.ema_enabled = self.ema_decay > 0.0
        self.ema = self.ema_state = None
        self._omd = 1.0 - self.ema_decay                # formed in double, rounded to fp32 once
        self.param_names = param_names                  # {id(parameter): name} for ema_state_dict()
        if self.ema_enabled:
            self.ema = flat.data.detach().clone()
            self.ema_state = torch.zeros(4, dtype=torch.float32, device=flat.data.device)
        # per-step learning-rate schedule (off at None: no tensor, no launch), a run constant.  The groups' lr in
        # param_groups stay the BASE learning rates (what MultiStepLR scales per epoch); one launch per step
        # (ops.adam.lr_schedule_dev, before the Adam launch) writes base * f(t) into dev_state[1] / group_state[:, 0],
        # with t the effective Adam step as the device knows it.  lr_base is fp32[G], the device copy of the base
        # learning rates; sched_state is fp32[4] = {f of the last applied update, its t, 0, 0}
        self.lr_schedule = lr_schedule
        self.lr_base = self.sched_state = None
        if lr_schedule is not None:
            self.lr_base = torch.zeros(len(self.param_groups), dtype=torch.float32, device=flat.data.device)
            self.sched_state = torch.zeros(4, dtype=torch.float32, device=flat.data.device)
        # layer-wise trust ratios (LAMB; off by default: no tensor, no launch).  Tensor i of flat.params is the chunks
        # tensor_chunk_start[i] .. tensor_chunk_start[i + 1] of the flat buffer (its padding included);
        # tensor_adapt[i] = 0 keeps its trust ratio at 1 (the parameters of a group with layer_adapt: False).  The
        # step is then ops.adam.flat_lamb_dev_step -- three launches in the place of the Adam launch -- which leaves
        # trust fp32[nT] and norms fp32[nT, 2] = {||p||, ||u||} of the last applied update.  m, v and the step are
        # Adam's, so the state dict is too
        self.layer_adapt = bool(layer_adapt)
        self.kind = "lamb" if self.layer_adapt else "adam"
        self.tensor_chunk_start = self.tensor_adapt = self.chunk_tensor = None
        self.chunk_sums = self.trust = self.norms = None
        if self.layer_adapt:
            starts, adapt = self.layer_tables(flat, self.param_groups, group_adapt)
            dev = flat.data.device
            nT = len(adapt)
            if self._kernel is not None:
                self.tensor_chunk_start, self.tensor_adapt, self.chunk_tensor = self._kernel.lamb_tables(
                    starts, adapt, flat.numel, dev)
                self.chunk_sums = torch.zeros(flat.numel // ALIGN, 2, dtype=torch.float32, device=dev)
            else:
                self.tensor_chunk_start = torch.tensor(starts, dtype=torch.int32, device=dev)
                self.tensor_adapt = torch.tensor(adapt, dtype=torch.uint8, device=dev)
            self.trust = torch.ones(nT, dtype=torch.float32, device=dev)
            self.norms = torch.zeros(nT, 2, dtype=torch.float32, device=dev)

    @staticmethod
    def layer_tables(flat: FlatParameters, param_groups: Sequence[dict],
                     group_adapt: Optional[Sequence[bool]] = None) -> Tuple[List[int], List[int]]:
        """``(tensor_chunk_start [nT + 1], tensor_adapt [nT])`` of ``flat.params`` from ``flat.offsets``: a tensor owns
        the 64-float chunks from its offset to the next tensor's (its zero padding included), and is adapted unless its
        group says ``layer_adapt: False`` (``group_adapt[gi]``, default: every group adapts)."""
        starts = [o // ALIGN for o in flat.offsets] + [flat.numel // ALIGN]
        if group_adapt is None:
            return starts, [1] * len(flat.params)
        adapt_of = {id(p): int(group_adapt[gi]) for gi, g in enumerate(param_groups) for p in g["params"]}
        return starts, [adapt_of[id(p)] for p in flat.params]

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        loss = closure() if closure is not None else None
        g = self.param_groups[0]
        lr, (b1, b2), eps, wd = g["lr"], g["betas"], g["eps"], g["weight_decay"]
        capturing = self._kernel is not None and torch.cuda.is_current_stream_capturing()
        # {step, lr} (and every group's {lr, wd}) live on the device and the step is advanced by a device op, so the
        # eager step and a captured hipGraph replay run the identical kernel (the host writes them only when they
        # are out of date, e.g. after an lr-scheduler step -- never inside a capture)
        if self._kernel is not None and not capturing and self.device_state_stale():
            self.sync_device_state()
        self.step_count += 1
        t = self.step_count
        self.flat.gather_grads()
        # the route: the ungrouped kernels while all groups hold one (lr, wd); a capture with several groups always
        # records the grouped kernel (the graph outlives the next scheduler step)
        grouped = len(self.param_groups) > 1 and (capturing or not self.groups_uniform())
        if self._kernel is not None:
            self.dev_state[0:1].add_(1.0)
            self._dev_step = t
            if self.clip_enabled:
                self._kernel.grad_norm_clip_(self.flat.grad, self.clip_state, self._partials,
                                             max_norm=self.max_grad_norm, grad_scale=grad_scale,
                                             skip_nonfinite=self.skip_nonfinite)
            if self.lr_schedule is not None:
                # this step's lr of every group, from the device's own t: the Adam launch below reads what this writes
                self._kernel.lr_schedule_dev(self.dev_state, self.lr_base, self.sched_state,
                                             group_state=self.group_state, clip_state=self.clip_state,
                                             **self.lr_schedule)
            if self.layer_adapt:
                # the same forms and operands, three launches: moments + chunk sums, per-tensor norms, apply
                self._kernel.flat_lamb_dev_step(self.flat.data, self.flat.grad, self.exp_avg, self.exp_avg_sq,
                                                self.dev_state, tensor_chunk_start=self.tensor_chunk_start,
                                                tensor_adapt=self.tensor_adapt, chunk_tensor=self.chunk_tensor,
                                                chunk_sums=self.chunk_sums, trust=self.trust, norms=self.norms,
                                                ema=self.ema, ema_state=self.ema_state, clip_state=self.clip_state,
                                                group_state=self.group_state if grouped else None,
                                                chunk_group=self.chunk_group if grouped else None, beta1=b1,
                                                beta2=b2, eps=eps, weight_decay=wd, grad_scale=grad_scale,
                                                one_minus_decay=self._omd, warmup=self.ema_warmup)
                return loss
            # one launch in every form: clip_state and ema are None when off, the groups' tensors go only if grouped
            self._kernel.flat_adam_dev_step(self.flat.data, self.flat.grad, self.exp_avg, self.exp_avg_sq,
                                            self.dev_state, ema=self.ema, ema_state=self.ema_state,
                                            clip_state=self.clip_state,
                                            group_state=self.group_state if grouped else None,
                                            chunk_group=self.chunk_group if grouped else None, beta1=b1, beta2=b2,
                                            eps=eps, weight_decay=wd, grad_scale=grad_scale,
                                            one_minus_decay=self._omd, warmup=self.ema_warmup)
            return loss
        grad = self.flat.grad
        if grad_scale != 1.0:
            grad = grad * grad_scale
        if self.clip_enabled:
            # torch fallback of the clip kernels: same semantics, same clip_state layout (host reads are fine here)
            coef, ok = self._clip_verdict(grad)
            if not ok:
                return loss
            if coef != 1.0:
                grad = grad * coef
            t -= self.skipped_steps
        p = self.flat.data
        f = None
        if self.lr_schedule is not None:
            # the kernel's work on the host: the factor in fp64 rounded once, fp32 products with the base lrs
            f = self._apply_schedule_host(t)
            lr = float(torch.tensor(lr, dtype=torch.float32) * f)
        if grouped:
            lr_e, wd_e = self._per_element()         # the same update with lr and wd expanded per element
            if f is not None:
                lr_e = lr_e * f
        if self.layer_adapt:
            self._lamb_host(p, grad, lr_e if grouped else lr, wd_e if grouped else wd, b1, b2, eps, t)
        else:
            if grouped:
                p.mul_(1.0 - lr_e * wd_e)
            elif wd:
                p.mul_(1.0 - lr * wd)
            self._adam_host(p, grad, lr_e if grouped else lr, b1, b2, eps, t, grouped)
        if self.ema_enabled:
            # the kernel's recurrence in torch: omd_t in fp32 from the same t, ema += omd_t * (p - ema)
            omd_t = self._omd_t(t)
            self.ema_state.copy_(torch.stack([omd_t, torch.tensor(float(t)), torch.zeros(()), torch.zeros(())]))
            self.ema.add_((p - self.ema).mul_(omd_t.to(p.device)))
        return loss

    def _adam_host(self, p, grad, lr, b1, b2, eps, t, grouped):
        """CPU / no-kernel path: moments and the Adam update (``lr`` per element when ``grouped``)."""
        self.exp_avg.lerp_(grad, 1.0 - b1)
        self.exp_avg_sq.mul_(b2).addcmul_(grad, grad, value=1.0 - b2)
        bc1 = 1.0 - b1 ** t
        bc2 = 1.0 - b2 ** t
        denom = (self.exp_avg_sq.sqrt() / math.sqrt(bc2)).add_(eps)
        if grouped:
            p.sub_((lr / bc1) * (self.exp_avg / denom))
        else:
            p.addcdiv_(self.exp_avg, denom, value=-lr / bc1)

    def _lamb_host(self, p, grad, lr, wd, b1, b2, eps, t):
        """CPU / no-kernel path of the LAMB step: the kernels' update in torch, fp32 with fp64 norms (``lr`` and ``wd``
        scalars, or per element with several groups)."""
        self.exp_avg.mul_(b1).add_(grad, alpha=1.0 - b1)
        self.exp_avg_sq.mul_(b2).addcmul_(grad, grad, value=1.0 - b2)
        bc1 = 1.0 - b1 ** t
        bc2 = 1.0 - b2 ** t
        u = (self.exp_avg / bc1) / (self.exp_avg_sq.sqrt() / math.sqrt(bc2)).add_(eps) + wd * p
        starts = [int(c) * ALIGN for c in self.tensor_chunk_start.tolist()]
        adapt = self.tensor_adapt.tolist()
        pn = torch.stack([p[a:b].double().pow(2).sum().sqrt() for a, b in zip(starts[:-1], starts[1:])])
        un = torch.stack([u[a:b].double().pow(2).sum().sqrt() for a, b in zip(starts[:-1], starts[1:])])
        on = torch.tensor(adapt, dtype=torch.bool, device=p.device) & (pn > 0) & (un > 0)
        trust = torch.where(on, pn / torch.where(un > 0, un, torch.ones_like(un)), torch.ones_like(pn)).float()
        self.trust.copy_(trust)
        self.norms.copy_(torch.stack([pn, un], dim=1).float())
        sizes = torch.tensor([b - a for a, b in zip(starts[:-1], starts[1:])], device=p.device)
        p.sub_(lr * trust.repeat_interleave(sizes) * u)

    # -------------------------------------------------------------- layer-wise trust ratios
    def trust_ratios(self) -> Dict[str, torch.Tensor]:
        """The trust ratio of every tensor of ``flat.params`` at the last applied update, by name: 0-d device views
        (no sync).  Ones before the first update."""
        if self.trust is None:
            raise RuntimeError("layer-wise adaptation is off (layer_adapt = False)")
        return {name: self.trust[i] for i, name in enumerate(self._param_names())}

    def last_update_norms(self) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
        """``(||p||, ||u||)`` of every tensor as the last applied update measured them (the weights before that update
        and its direction before the trust ratio and the learning rate), by name: 0-d device views (no sync)."""
        if self.norms is None:
            raise RuntimeError("layer-wise adaptation is off (layer_adapt = False)")
        return {name: (self.norms[i, 0], self.norms[i, 1]) for i, name in enumerate(self._param_names())}

    def _clip_verdict(self, grad: torch.Tensor):
        """CPU / no-kernel path: norm of the (already averaged) gradient -> clip_state, returns (coef, ok)."""
        norm = float(grad.double().pow(2).sum().sqrt())
        finite = math.isfinite(norm)
        coef = 1.0
        if self.max_grad_norm > 0.0 and finite:
            coef = min(1.0, self.max_grad_norm / (norm + 1e-6))
        ok = not (self.skip_nonfinite and not finite)
        cs = self.clip_state.tolist()
        self.clip_state.copy_(torch.tensor([norm, coef, float(ok), cs[3] + (0.0 if ok else 1.0),
                                            cs[4] + (1.0 if ok and coef < 1.0 else 0.0),
                                            0.0 if ok else cs[5] + 1.0, 0.0, 0.0], dtype=torch.float32))
        return coef, ok

    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """Norm of the last step's data-parallel mean gradient before clipping: a 0-d device view, no sync."""
        return self.clip_state[0] if self.clip_state is not None else None

    @property
    def skipped_steps(self) -> int:
        return int(self.clip_state[3]) if self.clip_state is not None else 0

    @property
    def clipped_steps(self) -> int:
        return int(self.clip_state[4]) if self.clip_state is not None else 0

    # -------------------------------------------------------------- per-step learning-rate schedule
    def _apply_schedule_host(self, t: int) -> torch.Tensor:
        """What ``lr_schedule_dev`` writes for the effective Adam step ``t``, from the host (the CPU / no-kernel path,
        and a loaded checkpoint); returns the fp32 factor (a 0-d host tensor)."""
        f = torch.tensor(lr_factor(t=t, **self._factor_args()), dtype=torch.float32)
        base = torch.tensor([x[0] for x in self.host_groups()], dtype=torch.float32)
        scaled = (base * f).to(self.dev_state.device)
        self.lr_base.copy_(base)
        self.dev_state[1] = scaled[0]
        if self.group_state is not None:
            self.group_state[:, 0] = scaled
        self.sched_state.copy_(torch.stack([f, torch.tensor(float(t)), torch.zeros(()), torch.zeros(())]))
        return f

    def _factor_args(self) -> dict:
        s = self.lr_schedule
        return dict(kind=s["kind"], warmup=s["warmup_steps"], decay=s["decay_steps"], min_ratio=s["min_lr_ratio"])

    @property
    def current_lr(self) -> torch.Tensor:
        """The first group's learning rate as the Adam launch reads it (``dev_state[1]``): a 0-d device view, no sync.
        With a schedule it is base lr times the factor of the last applied update."""
        if self.lr_schedule is None and self._kernel is None:
            return torch.tensor(self.param_groups[0]["lr"], dtype=torch.float32)     # no device copy is kept here
        return self.dev_state[1]

    @property
    def current_lrs(self) -> Dict[str, torch.Tensor]:
        """``current_lr`` of every group by name (views of ``group_state[:, 0]`` with several groups)."""
        if self.group_state is None or (self.lr_schedule is None and self._kernel is None):
            return {self.group_names[0]: self.current_lr}
        return {n: self.group_state[gi, 0] for gi, n in enumerate(self.group_names)}

    @property
    def lr_factor_now(self) -> Optional[torch.Tensor]:
        """The schedule factor of the last applied update (``sched_state[0]``): a 0-d device view, no sync."""
        return self.sched_state[0] if self.sched_state is not None else None

    # -------------------------------------------------------------- exponential moving average of the weights
    @property
    def ema_decay_now(self) -> Optional[torch.Tensor]:
        """The decay the last applied update used (``1 - ema_state[0]``): a 0-d device tensor, no sync."""
        return 1.0 - self.ema_state[0] if self.ema_state is not None else None

    @property
    def ema_num_updates(self) -> int:
        """Adam step of the last applied EMA update (skipped steps do not count)."""
        return int(self.ema_state[1]) if self.ema_state is not None else 0

    @torch.no_grad()
    def reset_ema(self):
        """``ema <- data`` (the weights were replaced from outside and there is no average to restore)."""
        if self.ema is not None:
            self.ema.copy_(self.flat.data)

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """The average per trainable parameter, keyed by name, over the parameters and offsets ``state_dict()`` walks."""
        if self.ema is None:
            raise RuntimeError("the EMA is off (ema_decay = 0)")
        return {name: self.ema[o:o + p.numel()].view_as(p).detach().clone()
                for name, p, o in zip(self._param_names(), self.flat.params, self.flat.offsets)}

    @torch.no_grad()
    def load_ema_state_dict(self, sd: Dict[str, torch.Tensor], num_updates: Optional[int] = None):
        if self.ema is None:
            raise RuntimeError("the EMA is off (ema_decay = 0)")
        names = self._param_names()
        missing = [n for n in names if n not in sd]
        if missing:
            raise KeyError(f"EMA state lacks {len(missing)} parameters, e.g. {missing[0]!r}")
        for name, p, o in zip(names, self.flat.params, self.flat.offsets):
            self.ema[o:o + p.numel()].copy_(sd[name].reshape(-1))
        if num_updates is not None:
            # {omd_t, t} as the update that produced this average left them (the next update rewrites both)
            t = int(num_updates)
            omd_t = self._omd_t(t) if t > 0 else torch.zeros(())
            self.ema_state.copy_(torch.stack([omd_t, torch.tensor(float(t)), torch.zeros(()), torch.zeros(())]))

    def _omd_t(self, t: int) -> torch.Tensor:
        """One minus the decay of Adam step ``t`` as the kernel forms it, in fp32 (a 0-d host tensor)."""
        omd = torch.tensor(self._omd, dtype=torch.float32)
        if not self.ema_warmup:
            return omd
        f32 = lambda x: torch.tensor(float(x), dtype=torch.float32)
        return torch.maximum(omd, f32(9) / (f32(10) + f32(t)))

    def _param_names(self) -> List[str]:
        """Names of ``flat.params`` in flat order: the model's (``param_names``), else the ``state_dict()`` index."""
        if self.param_names is not None:
            return [self.param_names[id(p)] for p in self.flat.params]
        pos: Dict[int, int] = {}
        for g in self.param_groups:
            for p in g["params"]:
                pos.setdefault(id(p), len(pos))
        return [str(pos[id(p)]) for p in self.flat.params]

    # -------------------------------------------------------------- parameter groups
    @staticmethod
    def _checked_groups(groups: Sequence[dict], all_params: List[torch.nn.Parameter]) -> List[dict]:
        """``groups`` as torch param-group dicts, after checking that they partition ``all_params``."""
        groups = [dict(g, params=list(g["params"])) for g in groups]
        if not 1 <= len(groups) <= MAX_GROUPS:
            raise ValueError(f"FlatAdam takes 1 to {MAX_GROUPS} parameter groups, got {len(groups)}")
        seen: Dict[int, int] = {}
        for gi, g in enumerate(groups):
            extra = set(g) - {"params", "name", "lr", "weight_decay", "layer_adapt"}
            if extra:
                raise ValueError(f"parameter group {gi} has unknown keys {sorted(extra)}")
            for p in g["params"]:
                if id(p) in seen:
                    raise ValueError(f"a parameter of shape {tuple(p.shape)} is in two parameter groups "
                                     f"({seen[id(p)]} and {gi})")
                seen[id(p)] = gi
        missing = [p for p in all_params if id(p) not in seen]
        if missing:
            raise ValueError(f"{len(missing)} parameters are in no parameter group, e.g. one of shape "
                             f"{tuple(missing[0].shape)}")
        if len(seen) != len(all_params):
            raise ValueError(f"the parameter groups hold {len(seen) - len(all_params)} parameters that are not the "
                             f"optimizer's")
        return groups

    def host_groups(self) -> Tuple[Tuple[float, float], ...]:
        """``(lr, weight_decay)`` of every group as the host holds them now."""
        return tuple((float(g["lr"]), float(g["weight_decay"])) for g in self.param_groups)

    def groups_uniform(self) -> bool:
        hg = self.host_groups()
        return all(x == hg[0] for x in hg)

    @property
    def group_names(self) -> List[str]:
        return [g.get("name", DEFAULT_GROUP) for g in self.param_groups]

    def group_layout(self, groups: Optional[Sequence[dict]] = None) -> List[Tuple[str, int]]:
        """``[(name, number of parameters)]`` of this optimizer's groups, or of a ``state_dict()``'s."""
        groups = self.param_groups if groups is None else groups
        return [(g.get("name", DEFAULT_GROUP), len(g["params"])) for g in groups]

    def _per_element(self):
        """CPU / no-kernel path: fp32 ``lr`` and ``weight_decay`` per flat element, rebuilt when a group changes."""
        hg = self.host_groups()
        if self._elem_cache is None or self._elem_cache[0] != hg:
            idx = self.chunk_group.long().repeat_interleave(ALIGN)
            dev = self.flat.data.device
            self._elem_cache = (hg, torch.tensor([x[0] for x in hg], dtype=torch.float32, device=dev)[idx],
                                torch.tensor([x[1] for x in hg], dtype=torch.float32, device=dev)[idx])
        return self._elem_cache[1], self._elem_cache[2]

    def device_state_stale(self) -> bool:
        """Whether the device copies of the step and of any group's ``(lr, weight_decay)`` differ from the host's
        (an lr-scheduler step, a loaded checkpoint, an eager step the device did not count)."""
        return self._dev_step != self.step_count or self._dev_groups != self.host_groups()

    def write_device_state(self, step: int):
        """Host -> device write of {step, group 0's lr} and, with several groups, of every group's {lr, wd, 0, 0}
        (small H2D copies; outside any capture).  Under a schedule: of the step, the base lrs and every group's wd."""
        hg = self.host_groups()
        if self.lr_base is not None:
            # under a schedule the lr slots (dev_state[1], group_state[:, 0]) belong to the schedule op, which forms them
            # from lr_base before every Adam launch: the host writes the base learning rates there and leaves the
            # slots alone, so current_lr stays the lr of the last applied update
            self.lr_base.copy_(torch.tensor([x[0] for x in hg], dtype=torch.float32))
            self.dev_state[0:1].copy_(torch.tensor([float(step)]))
            if self.group_state is not None:
                self.group_state[:, 1:].copy_(torch.tensor([[x[1], 0.0, 0.0] for x in hg], dtype=torch.float32))
            self._dev_step = int(step)
            self._dev_groups = hg
            return
        self.dev_state.copy_(torch.tensor([float(step), hg[0][0]]))
        if self.group_state is not None:
            self.group_state.copy_(torch.tensor([[x[0], x[1], 0.0, 0.0] for x in hg], dtype=torch.float32))
        self._dev_step = int(step)
        self._dev_groups = hg

    def sync_device_state(self):
        self.write_device_state(self.step_count)

    def zero_grad(self, set_to_none: bool = True):
        self.flat.zero_grad(set_to_none)

    # -------------------------------------------------------------- torch-Adam layout (de)serialisation
    def state_dict(self) -> Dict:
        groups = []
        index: Dict[int, int] = {}
        for g in self.param_groups:
            ids = []
            for p in g["params"]:
                index.setdefault(id(p), len(index))
                ids.append(index[id(p)])
            d = {k: v for k, v in g.items() if k != "params"}
            d["params"] = ids
            groups.append(d)
        state = {}
        # skipped steps never reached the moments: the checkpoint carries the effective Adam step
        step = self.step_count - self.skipped_steps
        if self.step_count > 0:
            for p, o in zip(self.flat.params, self.flat.offsets):
                n = p.numel()
                state[index[id(p)]] = {"step": torch.tensor(float(step)),
                                       "exp_avg": self.exp_avg[o:o + n].view_as(p).detach().clone(),
                                       "exp_avg_sq": self.exp_avg_sq[o:o + n].view_as(p).detach().clone()}
        out = {"state": state, "param_groups": groups}
        if self.lr_schedule is not None:
            out["lr_schedule"] = dict(self.lr_schedule)      # its position is the effective step above
        if self.layer_adapt:
            out["optimizer_kind"] = self.kind                # absent: adam (the layout every earlier checkpoint has)
        return out

    def load_state_dict(self, sd: Dict):
        groups = sd["param_groups"]
        if "lr_schedule" in sd and checked_lr_schedule(sd["lr_schedule"]) != self.lr_schedule:
            # extending or reshaping a run is legitimate: the running optimizer's schedule holds
            warnings.warn(f"the loaded state was written under the lr schedule {sd['lr_schedule']}, this optimizer "
                          f"runs {self.lr_schedule}: continuing with the latter from the restored step")
        # torch's own refusals, with both layouts named: a checkpoint's groups must be this optimizer's
        if len(groups) != len(self.param_groups):
            raise ValueError(f"loaded state dict has a different number of parameter groups: it holds "
                             f"{self.group_layout(groups)}, the optimizer {self.group_layout()}")
        if any(len(sg["params"]) != len(g["params"]) or
               ("name" in sg and sg["name"] != g.get("name", sg["name"])) for g, sg in zip(self.param_groups, groups)):
            raise ValueError(f"loaded state dict contains a parameter group that doesn't match the optimizer's: it "
                             f"holds {self.group_layout(groups)}, the optimizer {self.group_layout()}")
        for g, sg in zip(self.param_groups, groups):
            for k, v in sg.items():
                if k != "params":
                    g[k] = v
        pos = {}
        for g in self.param_groups:
            for p in g["params"]:
                pos.setdefault(id(p), len(pos))
        steps = []
        with torch.no_grad():
            for p, o in zip(self.flat.params, self.flat.offsets):
                st = sd["state"].get(pos[id(p)], sd["state"].get(str(pos[id(p)])))
                if st is None:
                    continue
                n = p.numel()
                self.exp_avg[o:o + n].copy_(st["exp_avg"].reshape(-1))
                self.exp_avg_sq[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
                steps.append(int(float(st["step"])))
        self.step_count = max(steps) if steps else 0
        if self.clip_state is not None:
            self.clip_state.zero_()      # the host counter is the effective step again
            self._dev_step = None
        if self.sched_state is not None:
            # {f, t} as the restored step's update left them under this schedule (the next one rewrites both)
            if self.step_count > 0:
                self._apply_schedule_host(self.step_count)
            else:
                self.sched_state.zero_()


def backbone_parameters(model: torch.nn.Module) -> List[torch.nn.Parameter]:
    """The parameters a pretrained EfficientNet-B3 state dict fills (``models.efficientnet.pretrained_keys``, the list
    the loader itself walks), over every ``FiLMEfficientNet`` inside ``model``, in module order."""
    from ..models.efficientnet import FiLMEfficientNet, pretrained_keys
    out = []
    for mod in model.modules():
        if isinstance(mod, FiLMEfficientNet):
            named = dict(mod.named_parameters())
            out += [named[k] for k in pretrained_keys(mod) if k in named]
    return out


def build_param_groups(model: torch.nn.Module, lr: float, weight_decay: float, no_decay_norm_bias: bool = False,
                       backbone_lr_mult: float = 1.0) -> List[dict]:
    """The parameter groups of ``FlatAdam(groups=...)`` for ``model``, from names and module types alone (the same on
    every rank), every parameter -- frozen ones included -- in exactly one group, in ``model.parameters()`` order:

    * ``no_decay_norm_bias``: parameters with ``ndim <= 1`` (BatchNorm / LayerNorm scales and shifts, every conv and
      linear bias) and ``nn.Embedding`` weights get ``weight_decay = 0``;
    * ``backbone_lr_mult != 1``: the pretrained backbone (``backbone_parameters``; the FiLM layers are not in it)
      gets ``lr * backbone_lr_mult``.

    The two rules cross to at most four groups, ``new``, ``new_no_decay``, ``backbone``, ``backbone_no_decay``; empty
    ones are dropped.  With both rules off: the one unnamed group of ``FlatAdam`` without ``groups``."""
    if not backbone_lr_mult > 0:
        raise ValueError(f"backbone_lr_mult must be > 0, got {backbone_lr_mult!r}")
    params = list(model.parameters())
    split_lr = float(backbone_lr_mult) != 1.0
    if not no_decay_norm_bias and not split_lr:
        return [dict(params=params, lr=lr, weight_decay=weight_decay)]
    backbone = {id(p) for p in backbone_parameters(model)} if split_lr else set()
    embeddings = {id(m.weight) for m in model.modules() if isinstance(m, torch.nn.Embedding)}
    groups = {name: dict(name=name, params=[], lr=lr * (backbone_lr_mult if name.startswith("backbone") else 1.0),
                         weight_decay=0.0 if name.endswith("no_decay") else weight_decay)
              for name in ("new", "new_no_decay", "backbone", "backbone_no_decay")}
    for p in params:
        name = "backbone" if id(p) in backbone else "new"
        if no_decay_norm_bias and (p.ndim <= 1 or id(p) in embeddings):
            name += "_no_decay"
        groups[name]["params"].append(p)
    # under FlatAdam(layer_adapt=True) the no-decay groups keep the plain Adam step size (trust ratio 1), as in the
    # LAMB paper's BERT recipe; FlatAdam keeps the flag to itself, so param_groups and checkpoints do not carry it
    for name, g in groups.items():
        if name.endswith("no_decay"):
            g["layer_adapt"] = False
    return [g for g in groups.values() if g["params"]]


def multistep_lr(optimizer: torch.optim.Optimizer, milestones: List[int], gamma: float = 0.1):
    return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones, gamma=gamma, last_epoch=-1)
