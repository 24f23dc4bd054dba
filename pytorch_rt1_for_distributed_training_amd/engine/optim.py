"""Adam / AdamW over the flat parameter buffer.

The reference uses ``torch.optim.Adam(lr)`` (beta=(0.9,0.999), eps=1e-8,
weight_decay=0) stepped per batch and ``MultiStepLR(milestones, 0.1)`` stepped
per epoch (``distribute_train.py:99-110``).  ``FlatAdam`` is numerically the
same update but owns flat fp32 moment buffers aligned with
``parallel.FlatParameters`` so one fused HIP kernel (``ops.adam``) updates all
35.2M trainable parameters per step; it also folds the data-parallel 1/world
gradient average into that pass.  AdamW is the same kernel with decoupled
decay (``weight_decay > 0``); the default 0 keeps parity with the reference.

It subclasses ``torch.optim.Optimizer`` so torch LR schedulers drive
``param_groups[0]['lr']`` and ``state_dict()`` is emitted in torch-Adam layout
(per-parameter ``step``/``exp_avg``/``exp_avg_sq``) for Lightning-format
checkpoints.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch

from ..parallel.flat import FlatParameters


class FlatAdam(torch.optim.Optimizer):
    def __init__(self, flat: FlatParameters, lr: float = 5e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, all_params: Optional[Sequence[torch.nn.Parameter]] = None,
                 use_kernel: Optional[bool] = None, max_grad_norm: Optional[float] = None,
                 skip_nonfinite: bool = False, ema_decay: float = 0.0, ema_warmup: bool = True,
                 param_names: Optional[Dict[int, str]] = None):
        if not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1) (0 = off), got {ema_decay!r}")
        self.flat = flat
        params = list(all_params) if all_params is not None else list(flat.params)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                                      maximize=False, foreach=None, capturable=False, differentiable=False,
                                      fused=None, decoupled_weight_decay=weight_decay > 0))
        self.exp_avg = torch.zeros_like(flat.data)
        self.exp_avg_sq = torch.zeros_like(flat.data)
        self.step_count = 0
        # device-resident step counter + lr so a captured graph replays correctly
        self.dev_state = torch.zeros(2, dtype=torch.float32, device=flat.data.device)
        self._dev_lr = None
        self._dev_step = None
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
        # same launch as Adam (ops.adam.flat_adam_ema_dev_step).  ema_state is fp32[4] = {omd_t of the last applied
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

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        loss = closure() if closure is not None else None
        g = self.param_groups[0]
        lr, (b1, b2), eps, wd = g["lr"], g["betas"], g["eps"], g["weight_decay"]
        self.step_count += 1
        t = self.step_count
        self.flat.gather_grads()
        if self._kernel is not None:
            # {step, lr} live on the device and the step is advanced by a device op, so the eager step and a
            # captured hipGraph replay run the identical kernel (the host writes dev_state only when it is
            # out of date, e.g. after an lr-scheduler step -- never inside a capture)
            if not torch.cuda.is_current_stream_capturing() and (self._dev_step != t - 1 or self._dev_lr != lr):
                self.write_device_state(t - 1, lr)
            self.dev_state[0:1].add_(1.0)
            self._dev_step = t
            if self.clip_enabled:
                self._kernel.grad_norm_clip_(self.flat.grad, self.clip_state, self._partials,
                                             max_norm=self.max_grad_norm, grad_scale=grad_scale,
                                             skip_nonfinite=self.skip_nonfinite)
            if self.ema_enabled:
                self._kernel.flat_adam_ema_dev_step(self.flat.data, self.flat.grad, self.exp_avg, self.exp_avg_sq,
                                                    self.ema, self.dev_state, self.ema_state, self.clip_state,
                                                    beta1=b1, beta2=b2, eps=eps, weight_decay=wd,
                                                    grad_scale=grad_scale, one_minus_decay=self._omd,
                                                    warmup=self.ema_warmup)
                return loss
            if self.clip_enabled:
                self._kernel.flat_adam_clip_dev_step(self.flat.data, self.flat.grad, self.exp_avg, self.exp_avg_sq,
                                                     self.dev_state, self.clip_state, beta1=b1, beta2=b2, eps=eps,
                                                     weight_decay=wd, grad_scale=grad_scale)
                return loss
            self._kernel.flat_adam_dev_step(self.flat.data, self.flat.grad, self.exp_avg, self.exp_avg_sq,
                                            self.dev_state, beta1=b1, beta2=b2, eps=eps, weight_decay=wd,
                                            grad_scale=grad_scale)
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
        if wd:
            p.mul_(1.0 - lr * wd)
        self.exp_avg.lerp_(grad, 1.0 - b1)
        self.exp_avg_sq.mul_(b2).addcmul_(grad, grad, value=1.0 - b2)
        bc1 = 1.0 - b1 ** t
        bc2 = 1.0 - b2 ** t
        denom = (self.exp_avg_sq.sqrt() / math.sqrt(bc2)).add_(eps)
        p.addcdiv_(self.exp_avg, denom, value=-lr / bc1)
        if self.ema_enabled:
            # the kernel's recurrence in torch: omd_t in fp32 from the same t, ema += omd_t * (p - ema)
            omd_t = self._omd_t(t)
            self.ema_state.copy_(torch.stack([omd_t, torch.tensor(float(t)), torch.zeros(()), torch.zeros(())]))
            self.ema.add_((p - self.ema).mul_(omd_t.to(p.device)))
        return loss

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

    def write_device_state(self, step: int, lr: float):
        """Host -> device write of {step, lr} (a small H2D copy; outside any capture)."""
        self.dev_state.copy_(torch.tensor([float(step), float(lr)]))
        self._dev_step = int(step)
        self._dev_lr = float(lr)

    def sync_device_state(self):
        self.write_device_state(self.step_count, self.param_groups[0]["lr"])

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
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd: Dict):
        groups = sd["param_groups"]
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


def multistep_lr(optimizer: torch.optim.Optimizer, milestones: List[int], gamma: float = 0.1):
    return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones, gamma=gamma, last_epoch=-1)
