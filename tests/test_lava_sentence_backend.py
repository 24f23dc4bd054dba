"""LavaConfig.sentence_backend: the default stays the torch chain, hip is refused where it cannot run and says why,
both backends hold the same parameters, and on the GPU a small SequenceLAVMSE with the hip encoder AND the fused visual
sentence is at least as close to the fp64 CPU model as the torch model under bf16 autocast.  Loss error is relative;
for the visual_proj.* and image_encoder.* parameter gradients it is 1 - cosine.  Both figures are printed (pytest -s).

The draw is the one of tests/test_lava_encoder_backend.py (model seed 3, input seed 103): autocast rounds the level
projections' inputs and outputs to bf16 (2^-9 relative per value), orders of magnitude above fp32 rounding, for the
visual_proj tensors as for the encoder's, so no other seed had to be drawn."""
import copy

import pytest
import torch
import torch.nn.functional as F

from pytorch_rt1_for_distributed_training_amd.models.lava import LavaConfig, SequenceLAVMSE

SMALL = dict(sequence_length=2, height=36, width=44, dropout=0.0)


def _fake_gpu(monkeypatch):
    from pytorch_rt1_for_distributed_training_amd.ops import _backend, lava_conv, lava_sentence
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)        # construction launches nothing
    monkeypatch.setattr(_backend, "available", lambda: True)
    monkeypatch.setattr(lava_conv, "supported", lambda cin, cout: True)
    monkeypatch.setattr(lava_sentence, "supported", lambda *a: True)


def test_default_is_torch_and_hip_needs_a_gpu(monkeypatch):
    assert LavaConfig().sentence_backend == "torch"
    assert SequenceLAVMSE(LavaConfig(**SMALL)).sentence_backend == "torch"
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # a CPU-only process
    for enc in ("torch", "hip"):
        with pytest.raises(ValueError, match="needs a GPU"):
            SequenceLAVMSE(LavaConfig(encoder_backend=enc, sentence_backend="hip", **SMALL))
    assert SequenceLAVMSE(LavaConfig(sentence_backend="auto", **SMALL)).sentence_backend == "torch"


def test_hip_names_what_is_missing(monkeypatch):
    _fake_gpu(monkeypatch)
    with pytest.raises(ValueError, match="needs the hip encoder"):
        SequenceLAVMSE(LavaConfig(sentence_backend="hip", **SMALL))
    with pytest.raises(ValueError, match="pyramid_fuse_layers"):
        SequenceLAVMSE(LavaConfig(encoder_backend="hip", sentence_backend="hip", pyramid_fuse_layers=(3, 4), **SMALL))
    assert SequenceLAVMSE(LavaConfig(encoder_backend="hip", sentence_backend="auto", pyramid_fuse_layers=(3, 4),
                                     **SMALL)).sentence_backend == "torch"


def test_both_backends_hold_the_same_parameters(monkeypatch):
    _fake_gpu(monkeypatch)
    hip = SequenceLAVMSE(LavaConfig(encoder_backend="hip", sentence_backend="hip", **SMALL))
    base = SequenceLAVMSE(LavaConfig(**SMALL))
    assert hip.sentence_backend == "hip"
    assert {k: v.shape for k, v in hip.state_dict().items()} == {k: v.shape for k, v in base.state_dict().items()}


def _loss_and_grads(model, obs, target, autocast=False):
    p0 = next(model.parameters())
    obs = {k: v.to(p0.device, p0.dtype) for k, v in obs.items()}
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        loss = F.mse_loss(model(obs).float() if autocast else model(obs), target.to(p0.device, p0.dtype))
    named = list(model.named_parameters())
    grads = torch.autograd.grad(loss, [p for _, p in named])
    assert all(bool(torch.isfinite(g).all()) for g in grads) and bool(torch.isfinite(loss))
    return {"loss": loss.detach().double().cpu(), **{n: g.double().cpu() for (n, _), g in zip(named, grads)}}


@pytest.mark.gpu
def test_model_with_hip_sentence_is_no_worse_than_bf16_autocast():
    torch.manual_seed(3)
    base = SequenceLAVMSE(LavaConfig(**SMALL)).train()
    hip = SequenceLAVMSE(LavaConfig(encoder_backend="hip", sentence_backend="hip", **SMALL)).train()
    hip.load_state_dict(base.state_dict())                               # a torch-backend checkpoint loads
    assert hip.sentence_backend == "hip"
    gen = torch.Generator().manual_seed(103)
    obs = {"rgb": torch.rand(2, 2, 36, 44, 3, generator=gen),
           "instruction_embedding": torch.randn(2, 2, 512, generator=gen)}
    target = torch.randn(2, 2, generator=gen)
    ref = _loss_and_grads(copy.deepcopy(base).double(), obs, target)
    cast = _loss_and_grads(copy.deepcopy(base).cuda(), obs, target, autocast=True)
    got = _loss_and_grads(hip.cuda(), obs, target)

    def err(a, r):
        if r.dim() == 0:
            return float((a - r).abs() / r.abs())
        return 1.0 - float(F.cosine_similarity(a.flatten(), r.flatten(), dim=0))

    failures = []
    for name in ["loss"] + [n for n in ref if n.startswith(("visual_proj.", "image_encoder."))]:
        e_cast, e_hip = err(cast[name], ref[name]), err(got[name], ref[name])
        print(f"lava_sentence {name:32s} autocast={e_cast:.3e} hip={e_hip:.3e}")
        if not e_hip <= e_cast:
            failures.append(f"{name}: hip {e_hip:.3e} > autocast {e_cast:.3e}")
    assert not failures, failures
