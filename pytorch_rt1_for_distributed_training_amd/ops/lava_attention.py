"""LAVA pixel-language cross attention on the HIP backend (``csrc/kernels/lavaxattn.hip``).

``CrossLayer`` attends with ONE language query per frame to the S pixel rows of the visual sentence.  With one query
the pixel LayerNorm, the K / V projections and the attention fold into one streamed pass over ``pixels`` (forward) and
one read plus the ``dpix`` write (backward); see the kernel file for the algebra.  The kernels return per-frame
vectors; the sums over frames -- the parameter gradients, [d, N] x [N, d] products -- are fp32 torch here, or with the
hip language backend (``lava_language.py``) one kernel of ``csrc/kernels/lavalang.hip``.
"""
from __future__ import annotations

import torch

from ._backend import resolve
from ._ext import available, load

HEADS = 2          # CrossLayer's head count


def supported(d_model: int, heads: int = HEADS) -> bool:
    """Whether the built extension serves this (d_model, heads)."""
    return available() and bool(load().lava_xattn_supported(int(d_model), int(heads)))


def resolve_backend(backend: str, d_model: int, heads: int = HEADS) -> str:
    """``torch | hip | auto`` -> ``torch | hip``.  ``hip`` needs a GPU, the extension and a supported shape and says
    which is missing; ``auto`` is ``hip`` exactly when all three hold."""
    return resolve(backend, lambda: supported(d_model, heads),
                   f"d_model={d_model}, heads={heads} (d_model=128, heads=2)")


class LavaCrossAttnFn(torch.autograd.Function):
    """(pixels [N, S, d], q [N, d], ln_pix weight, bias, eps, in_proj_weight [3d, d], in_proj_bias [3d]) -> the
    heads' context [N, d], i.e. ``nn.MultiheadAttention(q, LN(pixels), LN(pixels))`` before ``out_proj``."""

    @staticmethod
    def forward(ctx, pixels, q, ln_w, ln_b, eps, in_w, in_b):
        if not pixels.is_cuda:
            raise ValueError("the hip backend needs a GPU")
        pixels, q = pixels.contiguous(), q.contiguous()
        ln_w, ln_b, in_w, in_b = (t.detach().contiguous() for t in (ln_w, ln_b, in_w, in_b))
        out, z, lse, Q = load().lava_xattn_fwd(pixels, q, ln_w, ln_b, float(eps), in_w, in_b)
        ctx.save_for_backward(pixels, q, ln_w, ln_b, in_w, in_b, z, lse, Q)
        ctx.eps = float(eps)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dctx):
        pixels, q, ln_w, ln_b, in_w, in_b, z, lse, Q = ctx.saved_tensors
        dctx = dctx.contiguous()
        dpix, dq, dQ, u, w, e = load().lava_xattn_bwd(dctx, pixels, Q, z, lse, ln_w, ln_b, ctx.eps, in_w, in_b)
        n, d = q.shape
        dh = d // HEADS
        # the sums over frames: fp32 matmuls / sums over the kernels' per-frame outputs
        du = (ln_w * e).view(n, HEADS, d)                                # dL/du_h = g * e_h
        xv = ln_w * z + ln_b                                             # g * z_h + b, what W_v,h multiplies
        Qh, dch = Q.view(n, HEADS, dh), dctx.view(n, HEADS, dh)
        d_wq = dQ.t() @ q
        d_wk = (dh ** -0.5) * torch.einsum("nhi,nhk->hik", Qh, du).reshape(d, d)
        d_wv = torch.einsum("nhi,nhk->hik", dch, xv).reshape(d, d)
        d_in_w = torch.cat([d_wq, d_wk, d_wv], 0)
        d_in_b = torch.cat([dQ.sum(0), torch.zeros_like(ln_b), dctx.sum(0)], 0)   # the K bias shifts every score alike
        d_ln_w = (w * z + u * e).sum((0, 1))
        d_ln_b = w.sum((0, 1))
        return dpix, dq, d_ln_w, d_ln_b, None, d_in_w, d_in_b


class LavaCrossAttnHipSumsFn(LavaCrossAttnFn):
    """The same op; its backward leaves the sums over frames to ``lava_language.attn_param_grads``."""

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dctx):
        from .lava_language import attn_param_grads
        pixels, q, ln_w, ln_b, in_w, in_b, z, lse, Q = ctx.saved_tensors
        dctx = dctx.contiguous()
        dpix, dq, dQ, u, w, e = load().lava_xattn_bwd(dctx, pixels, Q, z, lse, ln_w, ln_b, ctx.eps, in_w, in_b)
        d_in_w, d_in_b, d_ln_w, d_ln_b = attn_param_grads(Q, dQ, q, dctx, u, w, z, e, ln_w, ln_b)
        return dpix, dq, d_ln_w, d_ln_b, None, d_in_w, d_in_b


def cross_attention(pixels, q, ln_pix, attn, hip_sums=False):
    """The op on a ``CrossLayer``'s own modules: ``ln_pix`` an ``nn.LayerNorm``, ``attn`` an
    ``nn.MultiheadAttention``; q [N, d] is ``ln_lang(lang)``.  ``hip_sums``: the parameter gradients' sums over frames
    on the HIP language kernels instead of torch."""
    fn = LavaCrossAttnHipSumsFn if hip_sums else LavaCrossAttnFn
    return fn.apply(pixels, q, ln_pix.weight, ln_pix.bias, ln_pix.eps, attn.in_proj_weight, attn.in_proj_bias)
