"""The language rows of LAVA's pixel-language ``CrossLayer``s on the HIP backend (``csrc/kernels/lavalang.hip``).

Around the folded attention of ``lava_attention.py`` a layer works on ``[N, 128]`` rows only: ``ln_lang``, the out
projection, dropout, residual, ``ln_ffn``, the ReLU FFN, dropout and residual.  Here that is one launch forward (the
"tail", whose epilogue LayerNorm is the NEXT layer's ``ln_lang`` or, after the last layer, the model's ``fuse_norm``)
and one backward plus a fixed-order reduce; the attention's parameter gradients, sums over frames that
``LavaCrossAttnFn`` forms in torch, run in one more kernel of the same unit.  Layer 0's ``ln_lang`` is the only
LayerNorm left on its own.  Serves d_model = dff = 128 and 2 heads, fp32, and needs the hip attention backend.
"""
from __future__ import annotations

import torch

from ._backend import resolve
from ._ext import available, load

D_MODEL, DFF, HEADS = 128, 128, 2


def supported(d_model: int = D_MODEL, dff: int = DFF, heads: int = HEADS) -> bool:
    """Whether the built extension serves this (d_model, dff, heads)."""
    return available() and bool(load().lava_lang_supported(int(d_model), int(dff), int(heads)))


def resolve_backend(backend: str, d_model: int = D_MODEL, dff: int = DFF, heads: int = HEADS) -> str:
    """``torch | hip | auto`` -> ``torch | hip`` for cross layers of this shape."""
    return resolve(backend, lambda: supported(d_model, dff, heads),
                   f"d_model={d_model}, dff={dff}, heads={heads} (served: {D_MODEL}, {DFF}, {HEADS})")


def tile_rows() -> int:
    """Language rows one workgroup owns."""
    return int(load().lava_lang_tile_rows())


def partials(n: int) -> int:
    """Workgroup partials a backward over ``n`` rows writes and the reduce adds in order (1: no reduce launch)."""
    return int(load().lava_lang_partials(int(n)))


def _seed(p: float) -> int:
    """From torch's CPU generator (no device sync), so ``torch.manual_seed`` reproduces a step."""
    return int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if p > 0.0 else 0


class LavaRowNormFn(torch.autograd.Function):
    """(x [N, 128], weight, bias, eps) -> LayerNorm(x), one launch each way (+ the reduce)."""

    @staticmethod
    def forward(ctx, x, w, b, eps):
        if not x.is_cuda:
            raise ValueError("the hip backend needs a GPU")
        x, w, b = x.contiguous(), w.detach().contiguous(), b.detach().contiguous()
        ctx.save_for_backward(x, w)
        ctx.eps = float(eps)
        return load().lava_lang_ln_fwd(x, w, b, ctx.eps)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dx, dw, db = load().lava_lang_ln_bwd(dy.contiguous(), x, w, ctx.eps)
        return dx, dw, db, None


class LavaTailFn(torch.autograd.Function):
    """(lang, ctx [N, 128], out_proj W, b, ln_ffn w, b, eps, ff1 W, b, ff2 W, b, epilogue LN w, b or None, eps, p,
    seed) -> (out, LN_epi(out) or None).  Saved: x3, f1, ctx, out (for the epilogue), the weights and the seed."""

    @staticmethod
    def forward(ctx, lang, actx, wo, bo, gf, bf, epsf, w1, b1, w2, b2, ge, be, epse, p, seed):
        if not lang.is_cuda:
            raise ValueError("the hip backend needs a GPU")
        lang, actx = lang.contiguous(), actx.contiguous()
        wo, bo, gf, bf, w1, b1, w2, b2 = (t.detach().contiguous() for t in (wo, bo, gf, bf, w1, b1, w2, b2))
        if ge is not None:
            ge, be = ge.detach().contiguous(), be.detach().contiguous()
        out, ln_out, x3, f1 = load().lava_lang_tail_fwd(lang, actx, wo, bo, gf, bf, float(epsf), w1, b1, w2, b2, ge, be,
                                                        float(epse), float(p), int(seed))
        ctx.save_for_backward(x3, f1, actx, wo, gf, bf, w1, w2, ge, out if ge is not None else None)
        ctx.cfg = (float(epsf), float(epse), float(p), int(seed))
        return out, ln_out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout, dln):
        x3, f1, actx, wo, gf, bf, w1, w2, ge, out = ctx.saved_tensors
        epsf, epse, p, seed = ctx.cfg
        g = load().lava_lang_tail_bwd(dout.contiguous(), dln.contiguous() if ge is not None else None, x3, f1, out, actx,
                                      wo, gf, bf, epsf, w1, w2, ge, epse, p, seed)
        dlang, dctx, dwo, dbo, dgf, dbf, dw1, db1, dw2, db2, dge, dbe = g
        if ge is None:
            dge = dbe = None
        return dlang, dctx, dwo, dbo, dgf, dbf, None, dw1, db1, dw2, db2, dge, dbe, None, None, None


def attn_param_grads(Q, dQ, q, dctx, u, w, z, e, ln_w, ln_b):
    """The sums over frames of ``lava_xattn_bwd``'s per-frame outputs -> (d in_proj_weight [384, 128], d in_proj_bias
    [384] with an exactly zero K third, d ln_pix weight, d ln_pix bias), bitwise reproducible."""
    return tuple(load().lava_lang_attn_pgrad(Q, dQ, q, dctx, u, w, z, e, ln_w, ln_b))


def row_norm(x, ln):
    """``ln`` (an ``nn.LayerNorm``) of x [N, 128]."""
    return LavaRowNormFn.apply(x, ln.weight, ln.bias, ln.eps)


def tail(lang, actx, layer, epilogue=None):
    """A ``CrossLayer``'s rows after its attention, on the layer's own modules; ``epilogue`` is the ``nn.LayerNorm``
    applied to the result as a second output (None: no second output)."""
    p = float(layer.drop.p) if layer.training else 0.0
    ge, be, epse = (epilogue.weight, epilogue.bias, epilogue.eps) if epilogue is not None else (None, None, 0.0)
    return LavaTailFn.apply(lang, actx, layer.attn.out_proj.weight, layer.attn.out_proj.bias, layer.ln_ffn.weight,
                            layer.ln_ffn.bias, layer.ln_ffn.eps, layer.ff1.weight, layer.ff1.bias, layer.ff2.weight,
                            layer.ff2.bias, ge, be, epse, p, _seed(p))


def cross_stack(pixels, lang, layers, final_norm=None):
    """The stack of ``CrossLayer``s on (pixels [N, S, 128], lang [N, 128]) -> (the last layer's output, ``final_norm``
    of it or None).  Layer i's tail carries layer i + 1's ``ln_lang`` as its epilogue and the last one ``final_norm``."""
    from .lava_attention import cross_attention
    layers = list(layers)
    x, qn = lang, row_norm(lang, layers[0].ln_lang)
    for i, layer in enumerate(layers):
        nxt = layers[i + 1].ln_lang if i + 1 < len(layers) else final_norm
        actx = cross_attention(pixels, qn, layer.ln_pix, layer.attn, hip_sums=True)
        x, qn = tail(x, actx, layer, nxt)
    return x, qn
