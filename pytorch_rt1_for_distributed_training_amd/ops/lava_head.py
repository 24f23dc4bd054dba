"""LAVA's policy head -- ``DenseResnet`` and the action projection -- on the HIP backend (``csrc/kernels/lavahead.hip``).

The head is a chain of short-wide linears on ``[B, .]`` rows: ``din -> width``, per block ``width -> width/4 ->
width/4 -> width`` with a ReLU before each linear and a residual around the block, then ``width -> action_size``.  Each
linear is one launch forward and one backward: the ReLU is the kernel's prologue on its input (what is stored between
the linears is the pre-activation), the residual add is the third linear's epilogue, and the block's first linear adds
the residual branch's gradient in its data-gradient epilogue, so a block's ``dx`` is written once.  Forward and backward
are ``2 + 3 * blocks`` launches each.  Serves fp32, ``din`` a multiple of 64, ``width`` a multiple of 256 (both up to
8192), ``action_size <= 8``; the modules' own parameters are used, so state dicts are the same on either backend.
"""
from __future__ import annotations

import torch

from ._backend import resolve
from ._ext import available, load

SERVED = "din a multiple of 64 and width a multiple of 256, both up to 8192, 1 <= action_size <= 8, fp32"


def supported(din: int, width: int = 1024, action_size: int = 2) -> bool:
    """Whether the built extension serves a head of this (din, width, action_size)."""
    return available() and bool(load().lava_head_supported(int(din), int(width), int(action_size)))


def resolve_backend(backend: str, din: int, width: int = 1024, action_size: int = 2) -> str:
    """``torch | hip | auto`` -> ``torch | hip`` for a head of this shape."""
    return resolve(backend, lambda: supported(din, width, action_size),
                   f"din={din}, width={width}, action_size={action_size} (served: {SERVED})")


def row_chunk() -> int:
    """Rows of the largest row chunk one workgroup owns; more rows walk several chunks."""
    return int(load().lava_head_row_chunk())


def _rows(x, what):
    if not x.is_cuda:
        raise ValueError("the hip backend needs a GPU")
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"{what}: x is {tuple(x.shape)} {x.dtype}, the hip head serves fp32 [B, din] ({SERVED})")
    return x.contiguous()


class LavaHeadLinearFn(torch.autograd.Function):
    """(x [B, K], weight [N, K], bias [N], relu_in, res [B, N] or None, carry) -> ``pro(x) W^T + b (+ res)`` with pro
    ReLU when ``relu_in``.  With ``carry`` the input is returned as a second output: a block hands THAT to its third
    linear as ``res``, so the gradient of the residual branch comes back here and is added in this backward's launch."""

    @staticmethod
    def forward(ctx, x, w, b, relu_in, res, carry):
        x, w, b = _rows(x, "lava_head linear"), w.detach().contiguous(), b.detach().contiguous()
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, w)
        ctx.relu_in, ctx.has_res = bool(relu_in), res is not None
        y = load().lava_head_linear_fwd(x, w, b, res.contiguous() if res is not None else None, ctx.relu_in)
        return (y, x.view_as(x)) if carry else y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy, dcarry=None):
        x, w = ctx.saved_tensors
        if dy is None:
            dy = x.new_zeros(x.shape[0], w.shape[0])
        dy = dy.contiguous()
        dx, dw, db = load().lava_head_linear_bwd(dy, x, w, dcarry.contiguous() if dcarry is not None else None,
                                                 ctx.relu_in)
        return dx, dw, db, None, dy if ctx.has_res else None, None


class LavaHeadProjFn(torch.autograd.Function):
    """(x [B, K], weight [A, K], bias [A]) -> ``x W^T + b`` for A <= 8: row dot products, one launch each way."""

    @staticmethod
    def forward(ctx, x, w, b):
        x, w, b = _rows(x, "lava_head projection"), w.detach().contiguous(), b.detach().contiguous()
        ctx.save_for_backward(x, w)
        return load().lava_head_proj_fwd(x, w, b)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        return tuple(load().lava_head_proj_bwd(dy.contiguous(), x, w))


def _check(din, head, action_projection=None):
    width, act = head.inp.out_features, action_projection.out_features if action_projection is not None else 1
    shapes = [(head.inp.in_features, width)] + [(l.in_features, l.out_features) for b in head.blocks
                                                 for l in (b[1], b[3], b[5])]
    want = [(din, width)] + [(width, width // 4), (width // 4, width // 4), (width // 4, width)] * len(head.blocks)
    proj_ok = action_projection is None or action_projection.in_features == width
    if shapes != want or not proj_ok or not supported(din, width, act):
        raise ValueError(f"the hip head does not serve din={din}, width={width}, action_size={act} with layers "
                         f"{shapes} (served: {SERVED})")


def dense_resnet(x, head):
    """``head`` (a ``DenseResnet``) of x [B, din] on the module's own parameters -> [B, width]."""
    _check(x.shape[-1] if x.dim() == 2 else -1, head)
    h = LavaHeadLinearFn.apply(x, head.inp.weight, head.inp.bias, False, None, False)
    for blk in head.blocks:
        l1, l2, l3 = blk[1], blk[3], blk[5]
        y, carried = LavaHeadLinearFn.apply(h, l1.weight, l1.bias, True, None, True)
        y = LavaHeadLinearFn.apply(y, l2.weight, l2.bias, True, None, False)
        h = LavaHeadLinearFn.apply(y, l3.weight, l3.bias, True, carried, False)
    return h


def dense_resnet_head(x, head, action_projection):
    """``action_projection(head(x))`` for a ``DenseResnet`` and its ``nn.Linear`` projection -> the action [B, A]."""
    _check(x.shape[-1] if x.dim() == 2 else -1, head, action_projection)
    return LavaHeadProjFn.apply(dense_resnet(x, head), action_projection.weight, action_projection.bias)
