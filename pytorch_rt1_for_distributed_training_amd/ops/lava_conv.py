"""One LAVA image-encoder stage, ``maxpool2(relu(conv3x3_same(x, W) + b))``, on the HIP backend
(``csrc/kernels/lavaconv.hip``): implicit-GEMM MFMA kernels with the ReLU and the VALID 2x2 pool in the epilogue, so
the full-resolution activation is never stored.  Activations are NHWC bf16; the first stage reads the frames
``[N, H, W, 3 s]`` (s = 1 .. 4 frames stacked channel-wise) as uint8 (``/255`` fused) or fp32.  The weights stay the
fp32 ``nn.Conv2d`` parameters.

The language-gated form of the later stages, ``maxpool2(relu(gate[n, c] * (conv3x3_same(x, W) + b)))`` with ``gate``
fp32 ``[N, cout]``, runs on the same kernels (a template flag): ``GatedConv3ReluPoolFn`` / ``gated_conv_relu_pool``.
"""
from __future__ import annotations

import torch

from ._backend import resolve
from ._ext import available, load

STAGES = ((3, 32), (32, 64), (64, 128), (128, 256))
FIRST_STAGE_CIN = (3, 6, 9, 12)                  # 1 .. 4 stacked RGB frames


def supported(cin: int, cout: int) -> bool:
    """Whether the built extension serves a stage of this (cin, cout)."""
    return available() and bool(load().lava_conv_supported(int(cin), int(cout)))


def resolve_backend(backend: str, stages=STAGES) -> str:
    """``torch | hip | auto`` -> ``torch | hip`` for an encoder made of these (cin, cout) stages."""
    return resolve(backend, lambda: all(supported(i, o) for i, o in stages),
                   f"conv stages {tuple(stages)} (served: {STAGES})")


def tile():
    """(rows, columns) of the conv tile one workgroup owns."""
    return tuple(load().lava_conv_tile())


def wgrad_partials(n, h, w, cin, cout) -> int:
    """Workgroup partials [9 cin, cout] fp32 that the weight gradient writes and reads back once."""
    return int(load().lava_conv_wgrad_partials(int(n), int(h), int(w), int(cin), int(cout)))


def lava_conv_fwd(x, weight, bias):
    """-> (y bf16, idx uint8) [N, H/2, W/2, cout]; idx 0..3 = winning window position, 4 = dead (y == 0)."""
    return tuple(load().lava_conv_fwd(x, weight, bias))


def lava_conv_dgrad(dy, idx, weight, hw=None):
    """-> dx bf16 [N, H, W, cin]; ``hw`` is the stage's input grid, (2 H/2, 2 W/2) when not given."""
    h, w = hw if hw is not None else (2 * dy.shape[1], 2 * dy.shape[2])
    return load().lava_conv_dgrad(dy, idx, weight, int(h), int(w))


def lava_conv_wgrad(x, dy, idx):
    """-> (dW fp32 [cout, cin, 3, 3], db fp32 [cout]), bitwise reproducible."""
    return tuple(load().lava_conv_wgrad(x, dy, idx))


class Conv3ReluPoolFn(torch.autograd.Function):
    """(x NHWC, weight [cout, cin, 3, 3], bias [cout]) -> (y NHWC bf16, idx uint8).  The backward needs x, the argmax
    bytes and the weight: a dead window (idx 4) is where the ReLU cut, so y itself is not kept."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        if not x.is_cuda:
            raise ValueError("the hip backend needs a GPU")
        x = x.contiguous()
        weight, bias = weight.detach().contiguous(), bias.detach().contiguous()
        y, idx = lava_conv_fwd(x, weight, bias)
        ctx.save_for_backward(x, idx, weight)
        ctx.mark_non_differentiable(idx)
        return y, idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy, _didx):
        x, idx, weight = ctx.saved_tensors
        dy = dy.to(torch.bfloat16).contiguous()
        dw = db = dx = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:           # a frozen encoder skips the launch
            dw, db = lava_conv_wgrad(x, dy, idx)
        if ctx.needs_input_grad[0] and x.shape[-1] >= 32:                # the frames have no gradient
            dx = lava_conv_dgrad(dy, idx, weight, x.shape[1:3])
        return dx, dw, db


def conv_relu_pool(x, conv):
    """The op on an ``nn.Conv2d``'s own parameters (3x3, padding 1, with bias)."""
    return Conv3ReluPoolFn.apply(x, conv.weight, conv.bias)[0]


def lava_conv_gated_fwd(x, weight, bias, gate):
    """-> (y bf16, idx uint8) of ``maxpool2(relu(gate[n, c] * (conv(x) + b)))``; dead (idx 4) = no gated value > 0."""
    return tuple(load().lava_conv_gated_fwd(x, weight, bias, gate))


def lava_conv_gated_dgrad(dy, idx, weight, gate, hw=None):
    """-> dx bf16 = conv^T of the operand ``(dy.float() * gate).bfloat16()`` routed by idx."""
    h, w = hw if hw is not None else (2 * dy.shape[1], 2 * dy.shape[2])
    return load().lava_conv_gated_dgrad(dy, idx, weight, gate, int(h), int(w))


def lava_conv_gated_wgrad(x, dy, idx, gate):
    """-> (dW, db) fp32 = sum_n gate[n] * (per-frame gradient), the gate applied in fp32; bitwise reproducible."""
    return tuple(load().lava_conv_gated_wgrad(x, dy, idx, gate))


def lava_conv_dgate(dy, y, gate, cin, hw=None):
    """-> dgate fp32 [N, cout] = (sum_p dy * y) / gate from the stage's own output y, 0 where gate == 0."""
    h, w = hw if hw is not None else (2 * dy.shape[1], 2 * dy.shape[2])
    return load().lava_conv_dgate(dy, y, gate, int(cin), int(h), int(w))


class GatedConv3ReluPoolFn(torch.autograd.Function):
    """(x NHWC bf16, weight [cout, cin, 3, 3], bias [cout], gate fp32 [N, cout]) -> (y NHWC bf16, idx uint8).  The
    backward keeps y as well: at a live winner y = gate * (conv + b), which is all the gate gradient needs."""

    @staticmethod
    def forward(ctx, x, weight, bias, gate):
        if not x.is_cuda:
            raise ValueError("the hip backend needs a GPU")
        x, gate = x.contiguous(), gate.detach().float().contiguous()
        weight, bias = weight.detach().contiguous(), bias.detach().contiguous()
        y, idx = lava_conv_gated_fwd(x, weight, bias, gate)
        ctx.save_for_backward(x, y, idx, weight, gate)
        ctx.mark_non_differentiable(idx)
        return y, idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy, _didx):
        x, y, idx, weight, gate = ctx.saved_tensors
        dy = dy.to(torch.bfloat16).contiguous()
        dx = dw = db = dg = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:           # a frozen conv skips the launch
            dw, db = lava_conv_gated_wgrad(x, dy, idx, gate)
        if ctx.needs_input_grad[0]:
            dx = lava_conv_gated_dgrad(dy, idx, weight, gate, x.shape[1:3])
        if ctx.needs_input_grad[3]:
            dg = lava_conv_dgate(dy, y, gate, x.shape[-1], x.shape[1:3])
        return dx, dw, db, dg


def gated_conv_relu_pool(x, conv, gate):
    """The gated op on an ``nn.Conv2d``'s own parameters (3x3, padding 1, with bias)."""
    return GatedConv3ReluPoolFn.apply(x, conv.weight, conv.bias, gate)[0]
