"""Fused flat Adam/AdamW (``csrc/kernels/adam.hip``)."""
from __future__ import annotations

import math

import torch

from ._ext import load


def flat_adam_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, *, lr: float, beta1: float,
                   beta2: float, eps: float, weight_decay: float, step: int, grad_scale: float = 1.0):
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    load().flat_adam(p, g, m, v, lr, beta1, beta2, eps, weight_decay, lr / bc1, 1.0 / math.sqrt(bc2), grad_scale)


CLIP_STATE_SLOTS = 8   # {norm, coef, ok, skipped steps, clipped steps, consecutive skipped steps, 0, 0}
EMA_STATE_SLOTS = 4    # {omd_t used by the last applied update, t of that update, 0, 0}
CHUNK = 64             # floats per chunk_group entry: parallel.flat.ALIGN, so a chunk lies inside one parameter
MAX_GROUPS = 16
GROUP_STATE_SLOTS = 4  # {lr, weight_decay, 0, 0} per group


def flat_adam_dev_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, state: torch.Tensor, *,
                       ema: torch.Tensor = None, ema_state: torch.Tensor = None, clip_state: torch.Tensor = None,
                       group_state: torch.Tensor = None, chunk_group: torch.Tensor = None, beta1: float, beta2: float,
                       eps: float, weight_decay: float = 0.0, grad_scale: float = 1.0, one_minus_decay: float = 1.0,
                       warmup: bool = True):
    """The same update with {step, lr} read from the device tensor ``state`` (hipGraph-replayable), in one launch of
    one kernel template; the optional tensors select the form and every combination of them is allowed.

    * ``clip_state`` fp32[8] (``grad_norm_clip_``'s verdict): untouched buffers when ok == 0,
      ``g = (g * grad_scale) * coef`` otherwise, and the Adam step ``t`` is ``state[0]`` minus the skipped steps.
    * ``ema`` and ``ema_state`` fp32[4], together: the launch also carries the exponential moving average of the
      weights, ``ema += omd_t * (p_new - ema)`` with ``omd_t = max(one_minus_decay, 9 / (10 + t))`` under ``warmup``
      (the decay ``min(decay, (1 + t) / (10 + t))``) and ``one_minus_decay`` without, ``t`` being the Adam step of this
      call as the device sees it.  ``ema_state`` receives ``{omd_t, t, 0, 0}``; a skipped step touches neither.
    * ``group_state`` fp32[G, 4] = ``{lr_g, wd_g, 0, 0}`` (``G <= 16``) and ``chunk_group`` uint8[n / 64], together:
      ``lr`` and ``weight_decay`` per parameter group, ``chunk_group`` naming the group of each 64-float chunk;
      ``state[1]`` (the ungrouped lr) and ``weight_decay`` are not read.

    Every form runs the same per-element code on the same operands, so ``p, m, v`` of an applied step do not depend
    on whether the average is carried, a verdict with ``coef == 1`` equals no verdict, and the elements of group ``g``
    come out as the ungrouped form leaves them over the whole buffer with ``(lr_g, wd_g)``, bit for bit."""
    load().flat_adam_dev(p, g, m, v, state, ema, ema_state, clip_state, group_state, chunk_group, beta1, beta2, eps,
                         weight_decay, grad_scale, float(one_minus_decay), bool(warmup))


MAX_LAMB_TENSORS = 65535   # chunk_tensor is uint16


def lamb_tables(tensor_chunk_start, tensor_adapt, n: int, device):
    """The checked device tables of ``flat_lamb_dev_step`` for a flat buffer of ``n`` floats: ``tensor_chunk_start``
    (``nT + 1`` integers: tensor ``i`` is the 64-float chunks ``start[i] .. start[i + 1]``; it must start at 0, never
    decrease and end at ``n / 64``) and ``tensor_adapt`` (``nT`` flags, 0 = the trust ratio of that tensor stays 1).
    Returns ``(tensor_chunk_start int32, tensor_adapt uint8, chunk_tensor uint16[n / 64])`` on ``device``."""
    tcs = torch.as_tensor(tensor_chunk_start, dtype=torch.int32, device="cpu").contiguous()
    ta = torch.as_tensor(tensor_adapt, device="cpu").to(torch.uint8).contiguous()
    return tuple(load().lamb_tables(tcs, ta, int(n), torch.device(device)))


def flat_lamb_dev_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, state: torch.Tensor, *,
                       tensor_chunk_start: torch.Tensor, tensor_adapt: torch.Tensor, chunk_tensor: torch.Tensor,
                       chunk_sums: torch.Tensor, trust: torch.Tensor, norms: torch.Tensor,
                       ema: torch.Tensor = None, ema_state: torch.Tensor = None, clip_state: torch.Tensor = None,
                       group_state: torch.Tensor = None, chunk_group: torch.Tensor = None, beta1: float, beta2: float,
                       eps: float, weight_decay: float = 0.0, grad_scale: float = 1.0, one_minus_decay: float = 1.0,
                       warmup: bool = True):
    """LAMB (layer-wise trust ratios, ``csrc/kernels/lamb.hip``) in the forms and with the keywords of
    ``flat_adam_dev_step``: ``m, v`` are Adam's, and with ``u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + wd * p`` every
    tensor ``i`` of the flat buffer moves by ``p -= (lr * r_i) * u``, ``r_i = ||p_i|| / ||u_i||`` (1 when either norm
    is 0 or ``tensor_adapt[i] == 0``).  Three launches (moments and per-chunk sums, per-tensor norms, apply), no host
    read, no atomics; ``g`` is not modified.

    * ``tensor_chunk_start`` int32[nT + 1], ``tensor_adapt`` uint8[nT], ``chunk_tensor`` uint16[n / 64]: what
      ``lamb_tables`` returns.
    * ``chunk_sums`` fp32[n / 64, 2]: workspace, ``{sum p^2, sum u^2}`` per 64-float chunk.
    * ``trust`` fp32[nT] and ``norms`` fp32[nT, 2] ``= {||p_i||, ||u_i||}`` (of the weights before the update).

    A skipped step (``clip_state[2] == 0``) writes nothing."""
    load().flat_lamb_dev(p, g, m, v, state, ema, ema_state, clip_state, group_state, chunk_group, tensor_chunk_start,
                         tensor_adapt, chunk_tensor, chunk_sums, trust, norms, beta1, beta2, eps, weight_decay,
                         grad_scale, float(one_minus_decay), bool(warmup))


def reference_lamb_step(p, g, m, v, tensor_chunk_start, tensor_adapt, *, lr, beta1, beta2, eps, weight_decay, step,
                        grad_scale=1.0, chunk_group=None):
    """Plain PyTorch oracle of the LAMB update in the dtype of its operands (fp64 for a referee), tensor by tensor.
    With ``chunk_group``, ``lr`` and ``weight_decay`` are per-group sequences expanded per element as in
    ``reference_adam_groups_step``; otherwise scalars.  Modifies ``p, m, v`` in place and returns
    ``(trust [nT], norms [nT, 2])`` in that dtype."""
    if chunk_group is not None:
        idx = chunk_group.to(device=p.device, dtype=torch.long).repeat_interleave(CHUNK)
        lr = torch.as_tensor(lr, dtype=p.dtype, device=p.device)[idx]
        wd = torch.as_tensor(weight_decay, dtype=p.dtype, device=p.device)[idx]
    else:
        lr = torch.full_like(p, lr)
        wd = torch.full_like(p, weight_decay)
    g = g * grad_scale
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    u = (m / (1 - beta1 ** step)) / (v.sqrt() / math.sqrt(1 - beta2 ** step) + eps) + wd * p
    starts = [int(x) * CHUNK for x in torch.as_tensor(tensor_chunk_start).tolist()]
    adapt = [int(x) for x in torch.as_tensor(tensor_adapt).tolist()]
    trust = torch.ones(len(adapt), dtype=p.dtype, device=p.device)
    norms = torch.zeros(len(adapt), 2, dtype=p.dtype, device=p.device)
    for i, (a, b) in enumerate(zip(starts[:-1], starts[1:])):
        norms[i, 0] = p[a:b].pow(2).sum().sqrt()
        norms[i, 1] = u[a:b].pow(2).sum().sqrt()
        if adapt[i] and norms[i, 0] > 0 and norms[i, 1] > 0:
            trust[i] = norms[i, 0] / norms[i, 1]
        p[a:b].sub_(lr[a:b] * trust[i] * u[a:b])
    return trust, norms


def gradnorm_partials(n: int) -> int:
    """Number of fp64 partial sums ``grad_norm_clip_`` needs for a gradient of ``n`` floats (a function of n alone)."""
    return int(load().gradnorm_partials(int(n)))


def grad_norm_clip_(grad: torch.Tensor, clip_state: torch.Tensor, partials: torch.Tensor, *, max_norm: float,
                    grad_scale: float = 1.0, skip_nonfinite: bool = False):
    """Global norm of ``grad * grad_scale`` in a fixed summation order (``csrc/kernels/gradnorm.hip``, two launches,
    no host read) -> ``clip_state`` fp32[8]: norm, clip coefficient (``max_norm <= 0``: always 1), ok (0 when
    ``skip_nonfinite`` and the norm is not finite) and the cumulative skipped / clipped / consecutive-skipped
    counters.  ``partials`` is an fp64 workspace of at least ``gradnorm_partials(grad.numel())`` elements."""
    ext = load()
    ext.grad_sumsq(grad, partials)
    ext.grad_clip_finalize(partials, ext.gradnorm_partials(grad.numel()), float(max_norm), float(grad_scale),
                           bool(skip_nonfinite), clip_state)


def flat_adam_clip_dev_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, state: torch.Tensor,
                            clip_state: torch.Tensor, *, beta1: float, beta2: float, eps: float, weight_decay: float,
                            grad_scale: float = 1.0):
    """``flat_adam_dev_step`` under ``clip_state``."""
    flat_adam_dev_step(p, g, m, v, state, clip_state=clip_state, beta1=beta1, beta2=beta2, eps=eps,
                       weight_decay=weight_decay, grad_scale=grad_scale)


def flat_adam_ema_dev_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, ema: torch.Tensor,
                           state: torch.Tensor, ema_state: torch.Tensor, clip_state: torch.Tensor = None, *,
                           beta1: float, beta2: float, eps: float, weight_decay: float, grad_scale: float = 1.0,
                           one_minus_decay: float, warmup: bool = True):
    """``flat_adam_dev_step`` with the average of the weights, with or without ``clip_state``."""
    flat_adam_dev_step(p, g, m, v, state, ema=ema, ema_state=ema_state, clip_state=clip_state, beta1=beta1,
                       beta2=beta2, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale,
                       one_minus_decay=one_minus_decay, warmup=warmup)


def flat_adam_groups_dev_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, state: torch.Tensor,
                              group_state: torch.Tensor, chunk_group: torch.Tensor, *, ema: torch.Tensor = None,
                              ema_state: torch.Tensor = None, clip_state: torch.Tensor = None, beta1: float,
                              beta2: float, eps: float, grad_scale: float = 1.0, one_minus_decay: float = 1.0,
                              warmup: bool = True):
    """``flat_adam_dev_step`` with ``lr`` and ``weight_decay`` per parameter group, in any of its forms."""
    flat_adam_dev_step(p, g, m, v, state, ema=ema, ema_state=ema_state, clip_state=clip_state,
                       group_state=group_state, chunk_group=chunk_group, beta1=beta1, beta2=beta2, eps=eps,
                       grad_scale=grad_scale, one_minus_decay=one_minus_decay, warmup=warmup)


SCHED_KINDS = ("constant", "linear", "cosine", "rsqrt")   # the kernel's kind argument is the index
SCHED_STATE_SLOTS = 4  # {factor of the last applied update, its Adam step t, 0, 0}


def lr_schedule_dev(state: torch.Tensor, lr_base: torch.Tensor, sched_state: torch.Tensor, *,
                    group_state: torch.Tensor = None, clip_state: torch.Tensor = None, kind: str, warmup_steps: int,
                    decay_steps: int = 0, min_lr_ratio: float = 0.0):
    """The per-step learning-rate schedule, formed on the device (``csrc/kernels/lr_schedule.hip``, one wave, run
    before the Adam op of the step): with ``t = state[0]`` (minus the skipped steps of ``clip_state``) and
    ``f = engine.optim.lr_factor(kind, t, warmup_steps, decay_steps, min_lr_ratio)`` evaluated in fp64 and rounded once
    to fp32, ``state[1] <- lr_base[0] * f``, ``group_state[g, 0] <- lr_base[g] * f`` (when given; fp32 ``[G, 4]`` for
    the ``G <= 16`` entries of ``lr_base``) and ``sched_state`` fp32[4] ``<- {f, t, 0, 0}``.  A skipped step
    (``clip_state[2] == 0``) writes nothing."""
    if kind not in SCHED_KINDS:
        raise ValueError(f"lr_schedule_dev: kind is {kind!r}, expected one of {SCHED_KINDS}")
    load().lr_schedule_dev(state, lr_base, sched_state, group_state, clip_state, SCHED_KINDS.index(kind),
                           int(warmup_steps), int(decay_steps), float(min_lr_ratio))


def reference_adam_groups_step(p, g, m, v, chunk_group, group_lr, group_wd, *, beta1, beta2, eps, step,
                               grad_scale=1.0):
    """Plain PyTorch oracle of the grouped update in the dtype of its operands (fp64 for a referee): the math of
    ``reference_adam_step`` with ``lr`` and ``weight_decay`` expanded per element from ``chunk_group``."""
    idx = chunk_group.to(device=p.device, dtype=torch.long).repeat_interleave(CHUNK)
    lr = torch.as_tensor(group_lr, dtype=p.dtype, device=p.device)[idx]
    wd = torch.as_tensor(group_wd, dtype=p.dtype, device=p.device)[idx]
    g = g * grad_scale
    p.mul_(1 - lr * wd)
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    denom = (v.sqrt() / math.sqrt(1 - beta2 ** step)).add_(eps)
    p.sub_(lr / (1 - beta1 ** step) * (m / denom))


def reference_ema_step(ema: torch.Tensor, p: torch.Tensor, omd_t) -> torch.Tensor:
    """fp64 oracle of one EMA update, ``ema + omd_t * (p - ema)``; returns fp64 and modifies nothing."""
    e = ema.double()
    return e + float(omd_t) * (p.double() - e)


def buffer_guard_(buf: torch.Tensor, shadow: torch.Tensor, clip_state: torch.Tensor):
    """ok ? ``shadow = buf`` : ``buf = shadow`` (one launch): rolls back what a skipped step's forward wrote."""
    load().buffer_guard_(buf, shadow, clip_state)


def reference_clip_coef(g: torch.Tensor, max_norm: float, grad_scale: float = 1.0) -> float:
    """fp64 oracle of the clip coefficient (``torch.nn.utils.clip_grad_norm_``'s formula) for ``g * grad_scale``."""
    norm = float(g.double().pow(2).sum().sqrt()) * float(grad_scale)
    if max_norm is None or max_norm <= 0 or not math.isfinite(norm):
        return 1.0
    return min(1.0, float(max_norm) / (norm + 1e-6))


def reference_adam_step(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    """Plain PyTorch fp32 oracle (same math as torch.optim.Adam / AdamW)."""
    g = g * grad_scale
    if weight_decay:
        p.mul_(1 - lr * weight_decay)
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    denom = (v.sqrt() / math.sqrt(1 - beta2 ** step)).add_(eps)
    p.addcdiv_(m, denom, value=-lr / (1 - beta1 ** step))
