"""PixelLangMSE.encoder_backend: the default stays the torch encoder bit for bit, hip is refused where it cannot run
(naming what is served), both backends hold the same parameters, and on the GPU the model with the language-gated
encoder on HIP (first stage over the stacked frames, gated stages, tail) is at least as close to the fp64 CPU model as
the torch model under bf16 autocast: relative error for the loss, 1 - cosine for every ``encoder.*`` parameter gradient,
the rule of test_lava_encoder_backend.py.  Both figures are printed (pytest -s).

The draw (model seed 3, input seed 103) was fixed before hip's numbers were seen."""
import copy

import pytest
import torch
import torch.nn.functional as F

from pytorch_rt1_for_distributed_training_amd.models.lava import PixelLangMSE, policy_head
from test_lava_encoder_backend import _loss_and_grads


def _obs(seed):
    gen = torch.Generator().manual_seed(seed)
    return {"rgb": torch.rand(2, 2, 64, 48, 3, generator=gen),
            "instruction_embedding": torch.randn(2, 2, 512, generator=gen)}, torch.randn(2, 2, generator=gen)


def test_default_is_torch_and_bitwise_unchanged():
    torch.manual_seed(0)
    model = PixelLangMSE(sequence_length=2).eval()
    enc, (obs, _) = model.encoder, _obs(103)
    assert enc.backend == "torch"
    x = obs["rgb"].reshape(2, 64, 48, 6).permute(0, 3, 1, 2)            # the forward as it was before the field
    lang = obs["instruction_embedding"][:, -1]
    for i, conv in enumerate(enc.convs):
        x = conv(x)
        if i:
            x = x * enc.fuses[i].proj(lang)[:, :, None, None]
        x = F.max_pool2d(F.relu(x), 2)
    want = policy_head(enc.norm(F.relu(x.mean(dim=(2, 3)) * enc.lang_gate(lang))), model.dense_resnet,
                       model.action_projection)
    assert torch.equal(model(obs), want)


def test_hip_is_refused_where_it_cannot_run(monkeypatch):
    from pytorch_rt1_for_distributed_training_amd.ops import _backend, lava_conv, lava_pixel
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # a CPU-only process
    with pytest.raises(ValueError, match="needs a GPU"):
        PixelLangMSE(sequence_length=2, encoder_backend="hip")
    assert PixelLangMSE(sequence_length=2, encoder_backend="auto").encoder.backend == "torch"
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)        # construction launches nothing
    monkeypatch.setattr(_backend, "available", lambda: True)
    monkeypatch.setattr(lava_conv, "supported", lambda cin, cout: True)
    monkeypatch.setattr(lava_pixel, "supported", lambda channels: True)
    with pytest.raises(ValueError, match=r"served for 3 \* sequence_length in \(3, 6, 9, 12\)"):
        PixelLangMSE(sequence_length=5, encoder_backend="hip")
    assert PixelLangMSE(sequence_length=5, encoder_backend="auto").encoder.backend == "torch"
    hip, base = PixelLangMSE(sequence_length=2, encoder_backend="hip"), PixelLangMSE(sequence_length=2)
    assert hip.encoder.backend == "hip"
    assert {k: v.shape for k, v in hip.state_dict().items()} == {k: v.shape for k, v in base.state_dict().items()}


@pytest.mark.gpu
def test_model_with_hip_encoder_is_no_worse_than_bf16_autocast():
    torch.manual_seed(3)
    base = PixelLangMSE(sequence_length=2).train()
    hip = PixelLangMSE(sequence_length=2, encoder_backend="hip").train()
    hip.load_state_dict(base.state_dict())                               # a torch-backend checkpoint loads
    assert hip.encoder.backend == "hip"
    obs, target = _obs(103)
    ref = _loss_and_grads(copy.deepcopy(base).double(), obs, target)
    cast = _loss_and_grads(copy.deepcopy(base).cuda(), obs, target, autocast=True)
    got = _loss_and_grads(hip.cuda(), obs, target)

    def err(a, r):
        if r.dim() == 0:
            return float((a - r).abs() / r.abs())
        return 1.0 - float(F.cosine_similarity(a.flatten(), r.flatten(), dim=0))

    failures = []
    for name in ["loss"] + [n for n in ref if n.startswith("encoder.")]:
        e_cast, e_hip = err(cast[name], ref[name]), err(got[name], ref[name])
        print(f"lava_pixel {name:32s} autocast={e_cast:.3e} hip={e_hip:.3e}")
        if not e_hip <= e_cast:
            failures.append(f"{name}: hip {e_hip:.3e} > autocast {e_cast:.3e}")
    assert not failures, failures
