"""PixelLangMSE's language-conditioned encoder on the HIP backend: the first stage over the channel-stacked frames
and the three language-gated stages are ``ops/lava_conv.py`` (``csrc/kernels/lavaconv.hip``); this module is the tail,
``LayerNorm(relu(mean_p(y4) * gate))`` as one launch each way (``csrc/kernels/lavapix.hip``), and the backend rule of
the whole encoder.
"""
from __future__ import annotations

import torch

from . import lava_conv
from ._backend import resolve
from ._ext import available, load

CHANNELS = (32, 64, 128, 256)


def supported(channels: int) -> bool:
    """Whether the built extension serves a tail of this width."""
    return available() and bool(load().lava_pixel_tail_supported(int(channels)))


def resolve_backend(backend: str, in_ch: int = 12, channels=CHANNELS) -> str:
    """``torch | hip | auto`` -> ``torch | hip`` for an encoder of these stage widths over ``in_ch`` stacked channels."""
    stages = tuple(zip([in_ch] + list(channels[:-1]), channels))
    return resolve(backend, lambda: all(lava_conv.supported(i, o) for i, o in stages) and supported(channels[-1]),
                   f"{in_ch} stacked channels into stages {tuple(channels)} (served: "
                   f"{lava_conv.FIRST_STAGE_CIN} into {CHANNELS})")


def lava_pixel_tail_fwd(y4, gate, ln_w, ln_b, eps):
    """-> (out [N, 256], mean [N, 256], stat [N, 2] = (mu, rstd)), fp32."""
    return tuple(load().lava_pixel_tail_fwd(y4, gate, ln_w, ln_b, float(eps)))


def lava_pixel_tail_bwd(dout, mean, stat, gate, ln_w, hp, wp):
    """-> (dy4 bf16 [N, hp, wp, 256], dgate [N, 256], dgamma [256], dbeta [256])."""
    return tuple(load().lava_pixel_tail_bwd(dout, mean, stat, gate, ln_w, int(hp), int(wp)))


class PixelTailFn(torch.autograd.Function):
    """(y4 NHWC bf16, gate fp32 [N, C], LayerNorm weight, bias) -> out fp32 [N, C]."""

    @staticmethod
    def forward(ctx, y4, gate, ln_w, ln_b, eps):
        if not y4.is_cuda:
            raise ValueError("the hip backend needs a GPU")
        y4, gate = y4.contiguous(), gate.detach().float().contiguous()
        ln_w, ln_b = ln_w.detach().contiguous(), ln_b.detach().contiguous()
        out, mean, stat = lava_pixel_tail_fwd(y4, gate, ln_w, ln_b, eps)
        ctx.save_for_backward(mean, stat, gate, ln_w)
        ctx.hw = y4.shape[1:3]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        mean, stat, gate, ln_w = ctx.saved_tensors
        dy4, dgate, dgamma, dbeta = lava_pixel_tail_bwd(dout.float().contiguous(), mean, stat, gate, ln_w, *ctx.hw)
        return dy4, dgate, dgamma, dbeta, None


def pixel_tail(y4, gate, norm):
    """The op on an ``nn.LayerNorm``'s own parameters."""
    return PixelTailFn.apply(y4, gate, norm.weight, norm.bias, norm.eps)
