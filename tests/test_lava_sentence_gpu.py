"""The fused LAVA visual sentence (csrc/kernels/lavasent.hip, ops/lava_sentence.py) against the model's own expression
in fp64 on the CPU: F.max_pool2d, three F.linears on the flattened levels, scale, positions, cat.  Level values (post
ReLU, so dead windows and ties occur), weights and dpix are bf16-representable: what is left is accumulation order and
the bf16 store of dL2 / dL3.

Forward: |pixels - ref| <= 4 E, E the max error of the same expression in fp32 on the GPU (the 4x-eager rule; fp32
output, no relative term).  Backward: dW / db within 4x the fp32-GPU error of the same autograd expression, dL2 / dL3
within that plus 2^-8 |ref|, all bitwise equal over two runs; on dL3 every position that wins no pooling window must
carry the level-3 gradient alone.  Dropout: see test_dropout.

A workgroup of the weight gradient walks several row tiles as soon as a level has more tiles than partials, and the
partial count is capped by the bytes: BEYOND is the smallest such case, 65 rows of level 2 = two tiles, one partial."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

BEYOND = (1, 5, 13, 2, 2)
REFERENCE_FRAME = (2, 22, 40, 11, 20)
CASES = [(1, 1, 1, 2, 2), (2, 4, 5, 2, 2), (3, 7, 9, 3, 5), REFERENCE_FRAME, BEYOND]
EPS, SCALE = 2.0 ** -8, math.sqrt(128.0)
NAMES = ("L2", "L3", "W2", "W3", "W4", "b2", "b3", "b4")


def _sentence(l2, l3, ws, bs, pos):
    l4 = F.max_pool2d(l3.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    return torch.cat([F.linear(a.flatten(1, 2), w, b) * SCALE for a, w, b in zip((l2, l3, l4), ws, bs)], 1) + pos


@functools.lru_cache(maxsize=None)
def _case(n, h2, w2, h3, w3):
    """Inputs, the fp64 forward and the fp32-GPU forward error E."""
    from pytorch_rt1_for_distributed_training_amd.models.lava import sincos_2d
    gen = torch.Generator().manual_seed(1000 * h2 + 10 * w3 + n)
    l2 = torch.randn(n, h2, w2, 128, generator=gen).relu().bfloat16()
    l3 = torch.randn(n, h3, w3, 256, generator=gen).relu().bfloat16()
    ws = [(0.05 * torch.randn(128, c, generator=gen)).bfloat16().float() for c in (128, 256, 256)]
    bs = [0.05 * torch.randn(128, generator=gen) for _ in range(3)]
    pos = torch.cat([sincos_2d(128, h, w) for h, w in ((h2, w2), (h3, w3), (h3 // 2, w3 // 2))])
    dpix = torch.randn(n, pos.shape[0], 128, generator=gen).bfloat16().float()
    leaves = [l2, l3, *ws, *bs]
    ref = _sentence(l2.double(), l3.double(), [w.double() for w in ws], [b.double() for b in bs], pos.double())
    e32 = _sentence(l2.float().cuda(), l3.float().cuda(), [w.cuda() for w in ws], [b.cuda() for b in bs], pos.cuda())
    return leaves, pos, dpix, ref, float((e32.double().cpu() - ref).abs().max())


def _grads(leaves, pos, dout, dt, dev):
    t = [x.to(dev, dt).requires_grad_() for x in leaves]
    out = _sentence(t[0], t[1], t[2:5], t[5:8], pos.to(dev, dt))
    return [g.double().cpu() for g in torch.autograd.grad(out, t, dout.to(dev, dt))]


def _check_backward(case, dout, p, seed):
    """dout: the gradient that reaches the un-dropped sentence, mask / (1 - p) * dpix."""
    from pytorch_rt1_for_distributed_training_amd.ops import lava_sentence as ls
    leaves, pos, dpix, _, _ = _case(*case)
    ref, eag = _grads(leaves, pos, dout, torch.float64, "cpu"), _grads(leaves, pos, dout, torch.float32, "cuda")
    dev = [x.cuda() for x in leaves]
    runs = [ls.lava_sentence_bwd(dpix.cuda(), *dev[:5], p, seed) for _ in range(2)]
    (dl2, dl3), (dw2, db2, dw3, db3, dw4, db4) = runs[0]
    got = (dl2, dl3, dw2, dw3, dw4, db2, db3, db4)
    assert all(torch.equal(a, b) for a, b in zip(got, runs[1][0] + tuple(runs[1][1][i] for i in (0, 2, 4, 1, 3, 5))))
    assert dl2.dtype == dl3.dtype == torch.bfloat16 and dl2.shape == leaves[0].shape and dl3.shape == leaves[1].shape
    e_eag = [float((e - r).abs().max()) for e, r in zip(eag, ref)]
    for k, (name, g) in enumerate(zip(NAMES, got)):
        e_hip = (g.double().cpu() - ref[k]).abs()
        print(f"lava_sentence {name} {case} p={p}: hip={float(e_hip.max()):.3e} eager={e_eag[k]:.3e}")
        assert bool((e_hip <= (EPS if k < 2 else 0.0) * ref[k].abs() + 4 * e_eag[k]).all()), name
    # level 3 alone: the gradient of every position that wins no window (or lies outside the pooled area)
    l3, w3 = leaves[1].double(), leaves[3].double()
    n, h3, ww3 = l3.shape[:3]
    off = leaves[0].shape[1] * leaves[0].shape[2]
    only3 = (dout[:, off:off + h3 * ww3].double() @ w3 * SCALE).reshape(l3.shape)
    _, idx = F.max_pool2d(l3.permute(0, 3, 1, 2), 2, return_indices=True)
    no_win = torch.ones(n, 256, h3 * ww3, dtype=torch.bool).scatter_(2, idx.flatten(2), False)
    no_win = no_win.reshape(n, 256, h3, ww3).permute(0, 2, 3, 1)
    assert bool(((dl3.double().cpu() - only3).abs() <= EPS * only3.abs() + 4 * e_eag[1])[no_win].all())


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_sentence_matches_fp64(case):
    from pytorch_rt1_for_distributed_training_amd.ops import lava_sentence as ls
    leaves, pos, dpix, ref, E = _case(*case)
    n, h2, w2, h3, w3 = case
    if case == BEYOND:
        assert ls.wgrad_partials(*case)[0] == 1 < -(-n * h2 * w2 // ls.tile_rows()) == 2
    l2, l3, w_2, w_3, w_4, b_2, b_3, b_4 = (x.cuda() for x in leaves)
    pix = ls.lava_sentence_fwd(l2, l3, w_2, b_2, w_3, b_3, w_4, b_4, pos.cuda())
    assert pix.dtype == torch.float32 and pix.shape == ref.shape
    err = float((pix.double().cpu() - ref).abs().max())
    print(f"lava_sentence fwd {case}: hip={err:.3e} eager={E:.3e}")
    assert err <= 4 * E
    _check_backward(case, dpix, 0.0, 0)


@pytest.mark.gpu
def test_dropout():
    """p = 0.1 at the reference frame: an element is exactly 0 or within the forward bound of ref / (1 - p); the
    dropped share is within 0.003 of p (5 sigma at 294 400 elements); the seed fixes the mask; the backward under the
    seed matches the fp64 reference masked by the mask read off the forward output."""
    from pytorch_rt1_for_distributed_training_amd.ops import lava_sentence as ls
    leaves, pos, dpix, ref, E = _case(*REFERENCE_FRAME)
    l2, l3, w_2, w_3, w_4, b_2, b_3, b_4 = (x.cuda() for x in leaves)
    p, seed = 0.1, 20240517
    run = lambda s: ls.lava_sentence_fwd(l2, l3, w_2, b_2, w_3, b_3, w_4, b_4, pos.cuda(), p, s)
    out = run(seed)
    zero = (out == 0).cpu()
    err = (out.double().cpu() - ref / (1 - p)).abs()
    print(f"lava_sentence dropout: dropped={float(zero.float().mean()):.5f} err={float(err[~zero].max()):.3e} E={E:.3e}")
    assert bool((zero | (err <= 4 * E)).all())
    assert abs(float(zero.float().mean()) - p) <= 0.003
    assert torch.equal(out, run(seed)) and not torch.equal(out == 0, run(seed + 1) == 0)
    _check_backward(REFERENCE_FRAME, dpix * (~zero) / (1 - p), p, seed)
