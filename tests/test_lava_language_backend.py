"""LavaConfig.language_backend: the default keeps the model bit for bit, hip is refused where it cannot run (no GPU,
or without the hip attention backend whose per-frame outputs it consumes), auto falls back to torch there; on the GPU
a whole SequenceLAVMSE with the cross stack's language rows on csrc/kernels/lavalang.hip agrees with an fp64 CPU copy
under the 4x-eager rule of tests/test_lava_backend.py (same small model and the draw that file documents as a sound
yardstick: model seed 9, input seed 109)."""
import copy

import pytest
import torch
import torch.nn.functional as F

from pytorch_rt1_for_distributed_training_amd.models.lava import LavaConfig, SequenceLAVMSE

SMALL = dict(sequence_length=2, height=48, width=64, dropout=0.0)


def _obs(b=2, t=2, h=48, w=64):
    gen = torch.Generator().manual_seed(109)
    return {"rgb": torch.rand(b, t, h, w, 3, generator=gen),
            "instruction_embedding": torch.randn(b, t, 512, generator=gen)}, torch.randn(b, 2, generator=gen)


def test_default_is_torch_and_bitwise_unchanged():
    assert LavaConfig().language_backend == "torch"
    torch.manual_seed(0)
    model = SequenceLAVMSE(LavaConfig(**SMALL)).eval()
    assert model.language_backend == "torch" and all(l.language_backend == "torch" for l in model.cross)
    obs, _ = _obs()
    q = torch.randn(4, 1, 128)
    pix = torch.randn(4, 62, 128)
    want = q
    for l in model.cross:                                                # the stack as it was before the field
        x3 = want + l.attn(l.ln_lang(want), l.ln_pix(pix), l.ln_pix(pix), need_weights=False)[0]
        want = x3 + l.ff2(F.relu(l.ff1(l.ln_ffn(x3))))
    got = q
    for l in model.cross:
        got = l(pix, got)
    assert torch.equal(got, want)
    torch.manual_seed(0)
    assert torch.equal(model(obs), SequenceLAVMSE(LavaConfig(language_backend="torch", **SMALL)).eval()(obs))


@pytest.mark.parametrize("gpu", [False, pytest.param(True, marks=pytest.mark.gpu)])
def test_hip_is_refused_where_it_cannot_run_and_auto_falls_back(monkeypatch, gpu):
    if not gpu:
        monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # a CPU-only process
    match = "needs the hip attention backend" if gpu else "needs a GPU"
    with pytest.raises(ValueError, match=match):
        SequenceLAVMSE(LavaConfig(backend="torch", language_backend="hip", **SMALL))
    with pytest.raises(ValueError):
        SequenceLAVMSE(LavaConfig(language_backend="cuda", **SMALL))
    auto = SequenceLAVMSE(LavaConfig(backend="torch", language_backend="auto", **SMALL))
    assert auto.language_backend == "torch" and all(l.language_backend == "torch" for l in auto.cross)


def _loss_and_grads(model, obs, target):
    dev, dt = next(model.parameters()).device, next(model.parameters()).dtype
    obs = {k: v.to(dev, dt) for k, v in obs.items()}
    loss = F.mse_loss(model(obs), target.to(dev, dt))
    grads = torch.autograd.grad(loss, list(model.parameters()))
    return [("loss", loss.detach().double().cpu())] + [(n, g.double().cpu()) for (n, _), g in
                                                       zip(model.named_parameters(), grads)]


@pytest.mark.gpu
def test_model_on_hip_language_backend_matches_fp64():
    torch.manual_seed(9)
    base = SequenceLAVMSE(LavaConfig(**SMALL)).train()
    hip = SequenceLAVMSE(LavaConfig(backend="hip", language_backend="hip", **SMALL)).train()
    hip.load_state_dict(base.state_dict())
    assert hip.language_backend == "hip"
    assert SequenceLAVMSE(LavaConfig(backend="auto", language_backend="auto", **SMALL)).language_backend == "hip"
    obs, target = _obs()
    ref = _loss_and_grads(copy.deepcopy(base).double(), obs, target)
    eag = _loss_and_grads(copy.deepcopy(base).cuda(), obs, target)
    got = _loss_and_grads(hip.cuda(), obs, target)
    failures = []
    for (name, r), (_, e), (_, g) in zip(ref, eag, got):
        scale = float(r.abs().max())
        if scale == 0.0:
            err_e, err_g = float(e.abs().max()), float(g.abs().max())
            ok = err_g == 0.0
        else:
            err_e, err_g = float((e - r).abs().max()) / scale, float((g - r).abs().max()) / scale
            ok = err_g <= 4 * err_e
        print(f"lava_model hip language {name:42s} max|ref|={scale:.3e} eager={err_e:.3e} hip={err_g:.3e}")
        if not ok:
            failures.append(f"{name}: hip {err_g:.3e} > bound from eager {err_e:.3e}")
    assert not failures, failures
    # under no_grad the stack runs the same kernels: the same bits
    from pytorch_rt1_for_distributed_training_amd.ops.lava_language import cross_stack
    pix, lang = torch.randn(4, 62, 128, device="cuda"), torch.randn(4, 128, device="cuda")
    with_grad = [t.detach() for t in cross_stack(pix, lang, hip.cross, hip.fuse_norm)]
    with torch.no_grad():
        for a, b in zip(cross_stack(pix, lang, hip.cross, hip.fuse_norm), with_grad):
            assert torch.equal(a, b)
