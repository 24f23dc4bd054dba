"""RT-1 masked attention on MFMA (``csrc/kernels/attention.hip``) and the fused transformer layer.

Forward is the HIP kernel (Q/K/V from ONE fused projection GEMM, mask computed
in-kernel, softmax + dropout + P@V on-chip, per-row log-sum-exp saved).  The
backward is a HIP kernel too (one workgroup per (batch, head)): it recomputes P
from Q, K and the saved LSE (no S x S tensor is kept from the forward),
regenerates the identical dropout mask from the same counter-based hash and
produces dQ, dK, dV with MFMAs (transposed operands via ds_read_b64_tr_b16).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from . import rng, switches
from ._ext import load
from .linear import _bf, proj, token_wgrad
from ..models.transformer import rt1_attention_mask

BF = torch.bfloat16
BWD_MAX_S = 96     # single-kernel attn_bwd covers S <= 96 (T <= 8); longer histories (<= 256) use attn_bwd_long
_MASKS = {}


def _allowed(S, L, Kimg, device):
    key = (S, L, Kimg, str(device))
    m = _MASKS.get(key)
    if m is None:
        steps = (S + L - 1) // L
        m = rt1_attention_mask(steps, Kimg, L - Kimg)[:S, :S].to(device=device, dtype=torch.bool)
        _MASKS[key] = m
    return m


def attn_probs(qkv, lse, L, Kimg, scale, drop_p, seed):
    """The probabilities that the forward applied to V (dropout included), fp32 [B, H, S, S], rebuilt from its qkv and
    stored lse by the ``attn_probs`` kernel: what the eager ``masked_attention(..., return_scores=True)`` returns."""
    return load().attn_probs(qkv, lse, L, Kimg, scale, drop_p, seed, _ctr(qkv))


class RT1AttentionFn(torch.autograd.Function):
    """``want_scores``: -> (out, probabilities [B, H, S, S] fp32), the second non-differentiable."""

    @staticmethod
    def forward(ctx, qkv, L: int, Kimg: int, drop_p: float, seed: int, want_scores: bool = False):
        qkv = qkv.contiguous()
        D = qkv.shape[-1]
        scale = 1.0 / math.sqrt(D)
        out, lse = load().attn_fwd(qkv, L, Kimg, scale, drop_p, seed, _ctr(qkv))
        ctx.save_for_backward(qkv, out, lse)
        ctx.args = (L, Kimg, drop_p, seed, scale)
        if want_scores:
            probs = attn_probs(qkv, lse, L, Kimg, scale, drop_p, seed)
            ctx.mark_non_differentiable(probs)
            return out, probs
        return out

    @staticmethod
    def backward(ctx, dout, *_):
        qkv, out, lse = ctx.saved_tensors
        L, Kimg, drop_p, seed, scale = ctx.args
        B, S, _, H, D = qkv.shape
        return attn_backward(qkv, out, dout.to(qkv.dtype).contiguous(), lse, L, Kimg, scale, drop_p, seed), \
            None, None, None, None, None

    @staticmethod
    def _backward_torch(qkv, out, lse, dout, L, Kimg, drop_p, seed, scale):
        """fp32 batched-GEMM backward with the kernels' keep-mask: the numerical oracle of the HIP backward."""
        B, S, _, H, D = qkv.shape
        q, k, v = qkv.float().permute(2, 0, 3, 1, 4).unbind(0)               # [B, H, S, D]
        allowed = _allowed(S, L, Kimg, qkv.device)
        s = torch.matmul(q, k.transpose(-1, -2)) * scale
        p = torch.exp(s.masked_fill(~allowed, float("-inf")) - lse[..., None])
        do = dout.float().permute(0, 2, 1, 3)                                  # [B, H, S, D]
        if drop_p > 0:
            keep = load().attn_keepmask(B * H, S, drop_p, seed, qkv, _ctr(qkv)).view(B, H, S, S).float() / (1.0 - drop_p)
            pd = p * keep
        else:
            keep = None
            pd = p
        dv = torch.matmul(pd.transpose(-1, -2), do)
        dpd = torch.matmul(do, v.transpose(-1, -2))
        dp = dpd * keep if keep is not None else dpd
        delta = (do * out.float().permute(0, 2, 1, 3)).sum(-1, keepdim=True)
        ds = p * (dp - delta)
        dq = torch.matmul(ds, k) * scale
        dk = torch.matmul(ds.transpose(-1, -2), q) * scale
        dqkv = torch.stack([dq, dk, dv], dim=0).permute(1, 3, 0, 2, 4).to(qkv.dtype).contiguous()
        return dqkv, None, None, None, None


def attn_backward(qkv, out, dout, lse, L, Kimg, scale, drop_p, seed):
    """dQKV on the HIP kernels: one workgroup per (b, h) with the S x S tiles in LDS for S <= 96 (T <= 8),
    the streamed dK/dV + dQ kernel pair (O(chunk) LDS) for longer histories up to the 256-position table."""
    S = qkv.shape[1]
    ext = load()
    if S <= BWD_MAX_S:
        return ext.attn_bwd(qkv, out, dout, lse, L, Kimg, scale, drop_p, seed, _ctr(qkv))
    return ext.attn_bwd_long(qkv, out, dout, lse, L, Kimg, scale, drop_p, seed, _ctr(qkv))


_QKV = {}     # data_ptr(q weight) -> (Wqkv [3HD, E], bqkv [3HD]) bf16, packed per step by FusedRT1._refresh_shadow


def set_qkv_packs(packs):
    global _QKV
    _QKV = packs


def _seed(p: float) -> int:
    """Per-call-site dropout salt; the per-step randomness is the device counter of ``ops.rng``."""
    return rng.next_salt() if p > 0 else 0


def _ctr(t: torch.Tensor) -> torch.Tensor:
    return rng.counter(t.device)


# the LayerNorm after each residual formed by the residual kernel itself, and the LN2 backward emitting the
# out-projection's bf16 gradient operand (+0.3 % step, 24 launches fewer: profiles/r5_tf_fuse_ln_ab.log; off: the
# standalone ln_fwd / drop_bwd launches)
TF_FUSE_LN = switches.on("tf_fuse_ln")
_EMPTY = {}


def _empty(dev):
    t = _EMPTY.get(dev)
    if t is None:
        t = torch.empty(0, device=dev)
        _EMPTY[dev] = t
    return t


class RT1LayerFn(torch.autograd.Function):
    """One pre-LN RT-1 decoder layer (reference ``transformer.py:112-144``) with an fp32 residual stream:

        x2 = x + Wo . attn(Wqkv . LN1(x)) + bo
        x3 = x2 + dropout(Wff . LN2(x2) + bff)

    The attention, LayerNorms, residual adds and dropout are HIP kernels (``attention.hip``, ``transformer.hip``); the
    projections are bf16 hipBLASLt GEMMs (fp32 accumulate) on the bf16 weight shadow.  Each residual kernel also forms
    the LayerNorm that follows it on the same rows (LN2 after the out-projection; the NEXT layer's LN1 after the FF),
    so no LayerNorm re-reads the residual stream: ``aux`` = (LN1(x), mean, rstd) when the previous layer formed them,
    ``next_ln`` = the next layer's (gamma, beta, eps), returned as three non-differentiable extra outputs (their
    gradient is the next layer's LayerNorm backward, which it runs itself from x3 and the saved statistics).  The LN2
    backward also emits the out-projection's bf16 gradient operand and its bias gradient.  The backward recomputes
    nothing but P inside the attention kernel.  With ``want_scores`` (the last entry of ``meta``) a fourth
    non-differentiable output holds the layer's attention probabilities (``attn_probs``, one more launch)."""

    @staticmethod
    def forward(ctx, x, g1, b1, wq, bq, wk, bk, wv, bv, wo, bo, g2, b2, wf, bff, aux_xn, aux_mu, aux_rs, meta):
        ext = load()
        L, Kimg, H, D, p_attn, p_ff, eps1, eps2, next_ln, want_scores = meta
        B, S, E = x.shape
        T = B * S
        x2d = x.reshape(T, E).float().contiguous()
        if aux_xn.numel():
            xn1, mu1, rs1 = aux_xn, aux_mu, aux_rs
        else:
            xn1, mu1, rs1 = ext.tf_ln_fwd(x2d, g1.float(), b1.float(), eps1)
        pk = _QKV.get(wq.data_ptr())
        if pk is not None:
            Wqkv, bqkv = pk                                                     # packed with the weight shadow
        else:
            Wqkv = torch.cat([_bf(wq), _bf(wk), _bf(wv)], 0)                   # [3*H*D, E]
            bqkv = torch.cat([bq, bk, bv]).to(BF)
        qkv = torch.addmm(bqkv, xn1, Wqkv.t()).view(B, S, 3, H, D)
        scale = 1.0 / math.sqrt(D)
        seed_a, seed_f = _seed(p_attn), _seed(p_ff)
        ctr = _ctr(x)
        o, lse = ext.attn_fwd(qkv, L, Kimg, scale, p_attn, seed_a, ctr)
        o2d = o.view(T, H * D)
        wo_b, wf_b = _bf(wo), _bf(wf)
        empty = _empty(x.device)
        nxt = (empty, empty, empty)
        if TF_FUSE_LN:
            x2, xn2, mu2, rs2 = ext.tf_resid(x2d, proj(o2d, wo_b), bo.float().contiguous(), 0.0, 0, None,
                                             g2.float(), b2.float(), eps2)
        else:
            (x2,) = ext.tf_resid(x2d, proj(o2d, wo_b), bo.float().contiguous(), 0.0, 0)
            xn2, mu2, rs2 = ext.tf_ln_fwd(x2, g2.float(), b2.float(), eps2)
        ff = proj(xn2, wf_b)
        if next_ln is not None and TF_FUSE_LN:
            gn, bn, epsn = next_ln
            x3, *nxt = ext.tf_resid(x2, ff, bff.float().contiguous(), p_ff, seed_f, ctr, gn.float(), bn.float(), epsn)
        else:
            (x3,) = ext.tf_resid(x2, ff, bff.float().contiguous(), p_ff, seed_f, ctr)
            if next_ln is not None:
                gn, bn, epsn = next_ln
                nxt = ext.tf_ln_fwd(x3, gn.float(), bn.float(), epsn)
        ctx.save_for_backward(x2d, xn1, mu1, rs1, qkv, o, lse, x2, xn2, mu2, rs2, Wqkv, wo_b, wf_b, g1, g2)
        ctx.meta = (L, Kimg, H, D, p_attn, p_ff, seed_a, seed_f, scale, B, S, E)
        ctx.set_materialize_grads(False)        # no zero-filled gradients for the three LN outputs
        if want_scores:
            # one extra launch, reading what this forward already holds; nothing above depends on it
            probs = attn_probs(qkv, lse, L, Kimg, scale, p_attn, seed_a)
            ctx.mark_non_differentiable(*nxt, probs)
            return (x3.view(B, S, E), *nxt, probs)
        ctx.mark_non_differentiable(*nxt)
        return (x3.view(B, S, E), *nxt)

    @staticmethod
    def backward(ctx, dx3, *_):
        ext = load()
        (x2d, xn1, mu1, rs1, qkv, o, lse, x2, xn2, mu2, rs2, Wqkv, wo_b, wf_b, g1, g2) = ctx.saved_tensors
        if dx3 is None:
            dx3 = torch.zeros_like(x2)
        L, Kimg, H, D, p_attn, p_ff, seed_a, seed_f, scale, B, S, E = ctx.meta
        T = B * S
        dx3 = dx3.reshape(T, E).float().contiguous()
        # FF branch: dropout, GEMM grads, LN2 (+ the residual grad)
        ctr = _ctr(dx3)
        dh, dbff = ext.tf_drop_bwd(dx3, p_ff, seed_f, ctr)
        nig = ctx.needs_input_grad
        dwf = token_wgrad(dh, xn2, True, nig[13])
        o2d = o.view(T, H * D)
        # LN2 backward (+ the residual grad dx3); its bf16 copy of dx2 is the out-projection's gradient operand
        if TF_FUSE_LN:
            dx2, dg2, db2, da, dbo = ext.tf_ln_bwd(proj(dh, wf_b, True), x2, mu2, rs2, g2.float(), dx3, True)
        else:
            dx2, dg2, db2 = ext.tf_ln_bwd(proj(dh, wf_b, True), x2, mu2, rs2, g2.float(), dx3)
            da, dbo = ext.tf_drop_bwd(dx2, 0.0, 0)
        # attention branch: out-projection, attention, QKV projection, LN1 (+ residual)
        dwo = token_wgrad(da, o2d, True, nig[9])
        do = proj(da, wo_b, True).view(B, S, H, D)
        dqkv = attn_backward(qkv, o, do, lse, L, Kimg, scale, p_attn, seed_a)
        dq2d = dqkv.view(T, 3 * H * D)
        dWqkv, dbqkv = token_wgrad(dq2d, xn1, ok=all(nig[3:9]), bias=True)
        dx, dg1, db1 = ext.tf_ln_bwd(proj(dq2d, Wqkv, True), x2d, mu1, rs1, g1.float(), dx2)
        n = H * D
        return (dx.view(B, S, E), dg1, db1, dWqkv[:n], dbqkv[:n], dWqkv[n:2 * n], dbqkv[n:2 * n],
                dWqkv[2 * n:], dbqkv[2 * n:], dwo, dbo, dg2, db2, dwf, dbff, None, None, None, None)


def fused_layer(layer, x: torch.Tensor, L: int, Kimg: int, training: bool, aux=None, next_norm=None, scores=None):
    """One fused layer: returns (x3, aux for the next layer or None).  ``aux`` = (LN1(x), mean, rstd) from the previous
    layer's epilogue; ``next_norm`` = the next layer's norm_1 (its LayerNorm is formed in this layer's epilogue).
    ``scores``: a list; a layer built with ``return_attention_scores`` appends its [B, H, S, S] fp32 probabilities."""
    att = layer.attn
    p_attn = att.dropout.p if training else 0.0
    p_ff = layer.dropout_1.p if training else 0.0
    nl = (next_norm.weight, next_norm.bias, next_norm.eps) if next_norm is not None else None
    want = scores is not None and layer._return_attention_scores
    meta = (L, Kimg, att.h, att.key_dim, p_attn, p_ff, layer.norm_1.eps, layer.norm_2.eps, nl, want)
    e = _empty(x.device)
    ax = aux if aux is not None else (e, e, e)
    out = RT1LayerFn.apply(x, layer.norm_1.weight, layer.norm_1.bias, att.q_linear.weight, att.q_linear.bias,
                           att.k_linear.weight, att.k_linear.bias, att.v_linear.weight, att.v_linear.bias,
                           att.out.weight, att.out.bias, layer.norm_2.weight, layer.norm_2.bias, layer.ff.weight,
                           layer.ff.bias, ax[0], ax[1], ax[2], meta)
    if want:
        scores.append(out[4].detach())
    return out[0], (tuple(out[1:4]) if nl is not None else None)


def fused_layer_supported(layer) -> bool:
    att = layer.attn
    return (layer.ff.in_features == 512 and layer.ff.out_features == 512 and att.key_dim == 128
            and att.value_dim == 128 and att.h * att.key_dim == att.q_linear.out_features)


def fused_qkv_weights(attn):
    w = torch.cat([attn.q_linear.weight, attn.k_linear.weight, attn.v_linear.weight], 0)
    b = torch.cat([attn.q_linear.bias, attn.k_linear.bias, attn.v_linear.bias], 0)
    return w, b


def transformer_layer(layer, x: torch.Tensor, L: int, Kimg: int, training: bool, scores=None) -> torch.Tensor:
    """One RT-1 layer (``_TransformerLayer``) with the fused QKV GEMM and the HIP attention; ``scores`` as in
    ``fused_layer``."""
    B, S, E = x.shape
    att = layer.attn
    x1 = layer.norm_1(x)
    w, b = fused_qkv_weights(att)
    qkv = F.linear(x1, w, b).view(B, S, 3, att.h, att.key_dim)
    p = att.dropout.p if training else 0.0
    if scores is not None and layer._return_attention_scores:
        o, probs = RT1AttentionFn.apply(qkv, L, Kimg, p, _seed(p), True)
        scores.append(probs.detach())
    else:
        o = RT1AttentionFn.apply(qkv, L, Kimg, p, _seed(p))
    x = x + att.out(o.reshape(B, S, att.h * att.value_dim))
    return x + layer.dropout_1(layer.ff(layer.norm_2(x)))
