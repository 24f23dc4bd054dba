"""The LAVA visual sentence on the HIP backend (``csrc/kernels/lavasent.hip``): the three level projections of
``SequenceLAVMSE.encode``, ``drop((A_l W_l^T + b_l) * sqrt(d) + pos)`` over fuse levels (2, 3, 4), written straight
into ``pixels`` fp32 ``[N, S, 128]`` from the hip encoder's NHWC bf16 stage outputs.  Level 4 (the 2x2 maxpool of
level 3) is never stored, and neither is a dropout mask: the backward recomputes both from ``L3`` and the seed.
"""
from __future__ import annotations

import torch

from ._backend import resolve
from ._ext import available, load

FUSE_LAYERS = (2, 3, 4)
CHANNELS = (128, 256, 256)
D_MODEL = 128


def supported(channels=CHANNELS, d_model: int = D_MODEL) -> bool:
    """Whether the built extension serves these level channels (the pooled level shares the third's) and d_model."""
    c = tuple(int(x) for x in channels)
    return (available() and len(c) == 3 and c[1] == c[2]
            and bool(load().lava_sentence_supported(c[0], c[1], int(d_model))))


def resolve_backend(backend: str, channels=CHANNELS, d_model: int = D_MODEL) -> str:
    """``torch | hip | auto`` -> ``torch | hip`` for a sentence of these level channels."""
    return resolve(backend, lambda: supported(channels, d_model),
                   f"level channels {tuple(channels)}, d_model={d_model} (served: {CHANNELS}, {D_MODEL})")


def tile_rows() -> int:
    """Sentence rows one workgroup owns."""
    return int(load().lava_sentence_tile_rows())


def wgrad_partials(n, h2, w2, h3, w3):
    """Workgroup partials per level (2, 3, 4) that the weight gradient writes and reads back once."""
    return tuple(load().lava_sentence_wgrad_partials(int(n), int(h2), int(w2), int(h3), int(w3)))


def lava_sentence_fwd(l2, l3, w2, b2, w3, b3, w4, b4, pos, p=0.0, seed=0):
    """-> pixels fp32 [N, S, 128], S = h2 w2 + h3 w3 + (h3 // 2)(w3 // 2)."""
    return load().lava_sentence_fwd(l2, l3, w2, b2, w3, b3, w4, b4, pos, float(p), int(seed))


def lava_sentence_bwd(dpix, l2, l3, w2, w3, w4, p=0.0, seed=0, data=True, weights=True):
    """-> (dL2, dL3 bf16 or None, None), (dW2, db2, dW3, db3, dW4, db4 fp32, bitwise reproducible, or six None)."""
    ext = load()
    dl = tuple(ext.lava_sentence_dgrad(dpix, l2, l3, w2, w3, w4, float(p), int(seed))) if data else (None, None)
    dw = tuple(ext.lava_sentence_wgrad(dpix, l2, l3, float(p), int(seed))) if weights else (None,) * 6
    return dl, dw


class LavaSentenceFn(torch.autograd.Function):
    """(L2, L3, W2, b2, W3, b3, W4, b4, pos, p, seed) -> pixels.  Saved: the two levels, the weights and the seed."""

    @staticmethod
    def forward(ctx, l2, l3, w2, b2, w3, b3, w4, b4, pos, p, seed):
        if not l2.is_cuda:
            raise ValueError("the hip backend needs a GPU")
        l2, l3 = l2.contiguous(), l3.contiguous()
        w2, b2, w3, b3, w4, b4 = (t.detach().float().contiguous() for t in (w2, b2, w3, b3, w4, b4))
        pix = lava_sentence_fwd(l2, l3, w2, b2, w3, b3, w4, b4, pos, p, seed)
        ctx.save_for_backward(l2, l3, w2, w3, w4)
        ctx.p, ctx.seed = float(p), int(seed)
        return pix

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dpix):
        l2, l3, w2, w3, w4 = ctx.saved_tensors
        need = ctx.needs_input_grad
        (dl2, dl3), dw = lava_sentence_bwd(dpix.float().contiguous(), l2, l3, w2, w3, w4, ctx.p, ctx.seed,
                                           data=need[0] or need[1], weights=any(need[2:8]))
        return (dl2, dl3) + dw + (None, None, None)


def visual_sentence(l2, l3, visual_proj, pos, p, training):
    """The op on the model's own ``nn.ModuleDict`` of level projections (keys "2", "3", "4"); ``pos`` fp32 [S, 128]
    is the three levels' position tables one after the other.  The dropout seed comes from torch's CPU generator (no
    device sync), so ``torch.manual_seed`` reproduces a step."""
    p = float(p) if training else 0.0
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if p > 0.0 else 0
    lin = [visual_proj[str(i)] for i in FUSE_LAYERS]
    return LavaSentenceFn.apply(l2, l3, lin[0].weight, lin[0].bias, lin[1].weight, lin[1].bias, lin[2].weight,
                                lin[2].bias, pos, p, seed)
