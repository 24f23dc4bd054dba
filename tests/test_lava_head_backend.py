"""head_backend of LavaConfig and PixelLangMSE: the default keeps both models bit for bit, hip is refused where it
cannot run (no GPU, an unsupported width), auto falls back to torch there; on the GPU a small SequenceLAVMSE and a
PixelLangMSE with ONLY the head on csrc/kernels/lavahead.hip agree with their fp64 CPU copies, loss and every parameter
gradient, under the 4x-eager rule of tests/test_lava_language_backend.py (its small model, model seed 9, input seed
109), and the no_grad forward equals the grad-mode forward bitwise.

Known weakness of the model case, shared with tests/test_lava_backend.py: the loss is one scalar, and eager's own fp32
error on it moves between processes, so the 4x-eager bound on the loss moves with it.  Measured for [lava] over seven
processes on one MI355X: eager 4.8e-07 .. 1.3e-06, hip head 1.4e-06 .. 2.1e-06 (one ulp of the loss is 9.2e-08);
six passed, one failed at eager 4.8e-07 against hip 2.1e-06.  Every parameter gradient passed in all of them."""
import copy

import pytest
import torch

from pytorch_rt1_for_distributed_training_amd.models.lava import (DenseResnet, LavaConfig, PixelLangMSE, SequenceLAVMSE,
                                                               policy_head)
from test_lava_language_backend import SMALL, _loss_and_grads, _obs


def test_default_is_torch_and_bitwise_unchanged():
    assert LavaConfig().head_backend == "torch"
    obs, _ = _obs()
    for make in (lambda **k: SequenceLAVMSE(LavaConfig(**SMALL, **k)), lambda **k: PixelLangMSE(sequence_length=2, **k)):
        torch.manual_seed(0)
        model = make().eval()
        head = model.head if hasattr(model, "head") else model.dense_resnet
        assert head.backend == "torch"
        x = torch.randn(3, head.inp.in_features)
        want = head.inp(x)                                               # the head as it was before the field
        for b in head.blocks:
            want = want + b(want)
        assert torch.equal(model.action_projection(head(x)), model.action_projection(want))
        assert torch.equal(policy_head(x, head, model.action_projection), model.action_projection(want))
        torch.manual_seed(0)
        assert torch.equal(model(obs), make(head_backend="torch").eval()(obs))


@pytest.mark.parametrize("gpu", [False, pytest.param(True, marks=pytest.mark.gpu)])
def test_hip_is_refused_where_it_cannot_run_and_auto_falls_back(monkeypatch, gpu):
    if not gpu:
        monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # a CPU-only process
        with pytest.raises(ValueError, match="needs a GPU"):
            SequenceLAVMSE(LavaConfig(head_backend="hip", **SMALL))
        with pytest.raises(ValueError, match="needs a GPU"):
            PixelLangMSE(head_backend="hip")
    with pytest.raises(ValueError, match="needs a GPU" if not gpu else "does not serve .*served:"):
        SequenceLAVMSE(LavaConfig(head_backend="hip", dense_resnet_width=1000, **SMALL))
    with pytest.raises(ValueError):
        SequenceLAVMSE(LavaConfig(head_backend="cuda", **SMALL))
    assert SequenceLAVMSE(LavaConfig(head_backend="auto", dense_resnet_width=1000, **SMALL)).head.backend == "torch"
    assert PixelLangMSE(head_backend="auto").dense_resnet.backend == ("hip" if gpu else "torch")
    if gpu:
        from pytorch_rt1_for_distributed_training_amd.ops.lava_head import dense_resnet
        with pytest.raises(ValueError, match="served:"):
            dense_resnet(torch.randn(2, 100, device="cuda"), DenseResnet(100, 1024, 1).cuda())


def _compare(tag, ref, eag, got):
    failures = []
    for (name, r), (_, e), (_, g) in zip(ref, eag, got):
        scale = float(r.abs().max())
        if scale == 0.0:
            err_e, err_g = float(e.abs().max()), float(g.abs().max())
            ok = err_g == 0.0
        else:
            err_e, err_g = float((e - r).abs().max()) / scale, float((g - r).abs().max()) / scale
            ok = err_g <= 4 * err_e
        print(f"{tag} hip head {name:42s} max|ref|={scale:.3e} eager={err_e:.3e} hip={err_g:.3e}")
        if not ok:
            failures.append(f"{name}: hip {err_g:.3e} > bound from eager {err_e:.3e}")
    assert not failures, failures


def _pixel_obs():
    gen = torch.Generator().manual_seed(109)
    return {"rgb": torch.rand(2, 2, 64, 48, 3, generator=gen),
            "instruction_embedding": torch.randn(2, 2, 512, generator=gen)}, torch.randn(2, 2, generator=gen)


@pytest.mark.gpu
@pytest.mark.parametrize("network", ["lava", "pixel"])
def test_model_with_only_the_head_on_hip_matches_fp64(network):
    torch.manual_seed(9)
    if network == "lava":
        base, hip = SequenceLAVMSE(LavaConfig(**SMALL)).train(), SequenceLAVMSE(LavaConfig(head_backend="hip", **SMALL)).train()
        assert (hip.backend, hip.image_encoder.backend, hip.sentence_backend, hip.language_backend) == ("torch",) * 4
        (obs, target), head = _obs(), hip.head
    else:
        base, hip = PixelLangMSE(sequence_length=2).train(), PixelLangMSE(sequence_length=2, head_backend="hip").train()
        (obs, target), head = _pixel_obs(), hip.dense_resnet
    assert head.backend == "hip"
    hip.load_state_dict(base.state_dict())                               # the same names either way
    ref = _loss_and_grads(copy.deepcopy(base).double(), obs, target)
    eag = _loss_and_grads(copy.deepcopy(base).cuda(), obs, target)
    hip = hip.cuda()
    _compare(network, ref, eag, _loss_and_grads(hip, obs, target))
    x = torch.randn(5, head.inp.in_features, device="cuda")
    with_grad = policy_head(x, head, hip.action_projection).detach()
    with torch.no_grad():                                                # the same kernels: the same bits
        assert torch.equal(policy_head(x, head, hip.action_projection), with_grad)
