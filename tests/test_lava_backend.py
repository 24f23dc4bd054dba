"""LavaConfig.backend: the default keeps the eager path bit for bit, hip is refused where it cannot run, and on the
GPU a whole SequenceLAVMSE routed through the folded attention kernels agrees with an fp64 CPU copy of the model
(metric and 4x-eager bound of tests/test_lava_xattn_gpu.py; eager is the same model with backend="torch" on the GPU).

The draw (model seed 9, input seed 109) is one at which the yardstick itself is sound: the 4x-eager bound on a scalar
such as the loss means something only where eager's own error is above fp32's rounding of the reference (2^-24
relative).  At the first draw tried (seeds 0 / 7) eager's fp32 loss happened to round onto the fp64 one (2.5e-09,
0.02 ulp), so 4x that was below what any fp32 result can hold -- eager on another machine, with other convolution
algorithms, missed its own bound there.  Of 16 draws measured (profiles/lava_xattn.log) eager and hip have the same
error distribution (encoder output 3.5e-07 .. 6.9e-07 both); this draw has the largest eager loss error (1.2e-06) and
was picked by that figure alone."""
import copy

import pytest
import torch
import torch.nn.functional as F

from pytorch_rt1_for_distributed_training_amd.models.lava import CrossLayer, LavaConfig, SequenceLAVMSE

SMALL = dict(sequence_length=2, height=48, width=64, dropout=0.0)        # sentence: 48 + 12 + 2 = 62 rows


def _obs(b=2, t=2, h=48, w=64):
    gen = torch.Generator().manual_seed(109)
    return {"rgb": torch.rand(b, t, h, w, 3, generator=gen),
            "instruction_embedding": torch.randn(b, t, 512, generator=gen)}, torch.randn(b, 2, generator=gen)


def test_default_backend_is_torch_and_bitwise_unchanged():
    assert LavaConfig().backend == "torch"
    torch.manual_seed(0)
    layer = CrossLayer(128, 2, 128, 0.0)
    assert layer.backend == "torch"
    pix, lang = torch.randn(3, 62, 128), torch.randn(3, 1, 128)
    p, q = layer.ln_pix(pix), layer.ln_lang(lang)                        # the layer as it was before the field
    x3 = lang + layer.attn(q, p, p, need_weights=False)[0]
    want = x3 + layer.ff2(F.relu(layer.ff1(layer.ln_ffn(x3))))
    assert torch.equal(layer(pix, lang), want)


def test_hip_needs_a_gpu_and_auto_falls_back(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # a CPU-only process
    with pytest.raises(ValueError, match="needs a GPU"):
        SequenceLAVMSE(LavaConfig(backend="hip", **SMALL))
    with pytest.raises(ValueError):
        SequenceLAVMSE(LavaConfig(backend="cuda", **SMALL))
    torch.manual_seed(0)
    auto = SequenceLAVMSE(LavaConfig(backend="auto", **SMALL)).eval()
    torch.manual_seed(0)
    base = SequenceLAVMSE(LavaConfig(**SMALL)).eval()
    assert auto.backend == "torch" and all(l.backend == "torch" for l in auto.cross)
    obs, _ = _obs()
    assert torch.equal(auto(obs), base(obs))


def _loss_and_grads(model, obs, target):
    dev, dt = next(model.parameters()).device, next(model.parameters()).dtype
    obs = {k: v.to(dev, dt) for k, v in obs.items()}
    loss = F.mse_loss(model(obs), target.to(dev, dt))
    grads = torch.autograd.grad(loss, list(model.parameters()))
    return [("loss", loss.detach().double().cpu())] + [(n, g.double().cpu()) for (n, _), g in
                                                       zip(model.named_parameters(), grads)]


@pytest.mark.gpu
def test_model_on_hip_backend_matches_fp64():
    torch.manual_seed(9)
    base = SequenceLAVMSE(LavaConfig(**SMALL)).train()
    hip = SequenceLAVMSE(LavaConfig(backend="hip", **SMALL)).train()
    hip.load_state_dict(base.state_dict())
    assert hip.backend == "hip" and SequenceLAVMSE(LavaConfig(backend="auto", **SMALL)).backend == "hip"
    obs, target = _obs()
    ref = _loss_and_grads(copy.deepcopy(base).double(), obs, target)
    eag = _loss_and_grads(copy.deepcopy(base).cuda(), obs, target)
    got = _loss_and_grads(hip.cuda(), obs, target)
    failures = []
    for (name, r), (_, e), (_, g) in zip(ref, eag, got):
        scale = float(r.abs().max())
        if scale == 0.0:
            err_e, err_g = float(e.abs().max()), float(g.abs().max())
            ok = err_g <= err_e
        else:
            err_e, err_g = float((e - r).abs().max()) / scale, float((g - r).abs().max()) / scale
            ok = err_g <= 4 * err_e
        print(f"lava_model hip {name:42s} max|ref|={scale:.3e} eager={err_e:.3e} hip={err_g:.3e}")
        if not ok:
            failures.append(f"{name}: hip {err_g:.3e} > bound from eager {err_e:.3e}")
    assert not failures, failures
    # under no_grad a cross layer runs the same kernels: the same bits (the temporal layers are not compared, torch
    # picks another attention kernel for them when no gradient is needed)
    pix, lang = torch.randn(4, 62, 128, device="cuda"), torch.randn(4, 1, 128, device="cuda")
    with_grad = hip.cross[0](pix, lang).detach()
    with torch.no_grad():
        assert torch.equal(hip.cross[0](pix, lang), with_grad)
