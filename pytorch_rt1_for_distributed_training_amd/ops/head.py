"""Fused action head: gather -> logits -> CE -> argmax in ONE HIP kernel (``csrc/kernels/head.hip``).

Reference: the logits head runs over all ``T*L`` positions (``transformer.py:197``), the ``T*A`` rows that
predict action tokens are gathered, scored with ``cross_entropy(reduction='none')`` and argmax-decoded
(``transformer_network.py:304-322,310-312``).  Forward here is one kernel per 16 scored rows (MFMA GEMM,
log-softmax, CE, argmax, and the softmax-minus-onehot gradient all on chip); the backward scales that
gradient by ``dce`` (one small kernel), runs dh on hipBLASLt and dW on the MFMA wgrad kernel.

``label_smoothing`` / ``z_loss`` select the sibling kernel with the regularised objective (``head_ce_loss_fwd``:
``loss = lse - (1 - eps) z[t] - eps / V sum z + zeta lse^2`` next to the plain CE); the backward is the same, on that
kernel's ``G``.  ``token_hits_`` counts ``pred == target`` per action-token slot (token accuracy).
"""
from __future__ import annotations

import torch

from ._ext import load
from .linear import _bf, token_wgrad

BF = torch.bfloat16


class HeadCEFn(torch.autograd.Function):
    """(hidden [B,S,E] fp32, W [V,E], bias [V], positions int32 [P], targets int32 [B*P], label_smoothing, z_loss)
    -> (loss [B*P], pred, nll); with both options 0 the plain kernel runs, the loss is the CE and no nll is returned."""

    @staticmethod
    def forward(ctx, hidden, W, bias, positions, targets, label_smoothing=0.0, z_loss=0.0):
        ext = load()
        h = hidden.float().contiguous()
        Wb = _bf(W).contiguous()
        if label_smoothing == 0.0 and z_loss == 0.0:
            loss, pred, G, hb = ext.head_ce_fwd(h, positions, Wb, bias.float().contiguous(), targets)
            nll = None
        else:
            loss, nll, pred, G, hb = ext.head_ce_loss_fwd(h, positions, Wb, bias.float().contiguous(), targets,
                                                          float(label_smoothing), float(z_loss))
        ctx.save_for_backward(G, hb, Wb, positions)
        ctx.shape = h.shape
        ctx.set_materialize_grads(False)        # no zero-filled gradient for pred / nll
        if nll is None:
            ctx.mark_non_differentiable(pred)
            return loss, pred
        ctx.mark_non_differentiable(pred, nll)
        return loss, pred, nll

    @staticmethod
    def backward(ctx, dce, *_):
        G, hb, Wb, positions = ctx.saved_tensors
        B, S, E = ctx.shape
        dz = load().head_ce_scale(G, dce.float().contiguous())             # [R, V] bf16
        dh = torch.mm(dz, Wb)                                               # [R, E]
        dW = token_wgrad(dz, hb, True, ctx.needs_input_grad[1])           # [V, E] fp32, MFMA wgrad kernel
        db = load().colsum(dz)
        dhidden = torch.zeros(B, S, E, device=G.device, dtype=torch.float32)
        dhidden[:, positions.long()] = dh.view(B, -1, E).float()           # positions are unique
        return dhidden, dW, db, None, None, None, None


def head_supported(linear: torch.nn.Linear) -> bool:
    return load().head_ce_supported(linear.out_features, linear.in_features)


def head_loss(linear: torch.nn.Linear, hidden: torch.Tensor, positions: torch.Tensor, targets: torch.Tensor,
              targets32: torch.Tensor = None, label_smoothing: float = 0.0, z_loss: float = 0.0):
    """``(loss, pred, nll)`` per scored row of ``linear(hidden[:, positions])`` against ``targets`` (b, T*A);
    ``targets32`` is the int32 copy the fused tokenizer already wrote (no conversion launch).  With ``label_smoothing``
    and ``z_loss`` both 0 the plain ``head_ce_fwd`` kernel runs, the loss is the CE and ``nll`` is None; otherwise
    ``head_ce_loss_fwd`` scores the regularised objective and ``nll`` is the plain CE of the same rows, without a
    gradient."""
    pos = positions if positions.dtype == torch.int32 else positions.to(torch.int32)
    tgt = (targets32 if targets32 is not None else targets).reshape(-1).to(torch.int32).contiguous()
    out = HeadCEFn.apply(hidden, linear.weight, linear.bias, pos.contiguous(), tgt, float(label_smoothing),
                         float(z_loss))
    return out if len(out) == 3 else (out[0], out[1], None)


def head_ce(linear: torch.nn.Linear, hidden: torch.Tensor, positions: torch.Tensor, targets: torch.Tensor,
            targets32: torch.Tensor = None, label_smoothing: float = 0.0, z_loss: float = 0.0):
    """``head_loss`` in the form its callers had before the options: ``(ce, pred)`` with both options 0, as ever, and
    ``(loss, pred, nll)`` with the regularised objective."""
    loss, pred, nll = head_loss(linear, hidden, positions, targets, targets32, label_smoothing, z_loss)
    return (loss, pred) if nll is None else (loss, pred, nll)


def token_hits_(counters: torch.Tensor, pred: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """``counters`` (int64 [A, 2]) += {rows with pred == target, rows} per action-token slot ``r % A`` over the
    flattened rows, in place.  GPU counters always take the HIP launch (``head_token_hits_``; no atomics, safe to
    capture): rows of another integer type are converted to int32 first, and more than 32 slots are an error, not a
    fallback.  CPU counters get the same count in torch (``models.policy.token_hits_torch_``)."""
    p, t = pred.reshape(-1), targets.reshape(-1)
    if not counters.is_cuda:
        from ..models.policy import token_hits_torch_
        return token_hits_torch_(counters, p, t)
    if counters.shape[0] > 32:
        raise ValueError(f"token_hits_: the hit-count kernel serves at most 32 action-token slots, got "
                         f"{counters.shape[0]}")
    load().head_token_hits_(p.to(torch.int32).contiguous(), t.to(torch.int32).contiguous(), counters)
    return counters
