"""`attention_scores`, the TokenLearner maps and the engine's saliency on the hip backend, on the whole model:
test_parity_gpu's twin configuration (128x128, seq_len 2, 8 layers, dropout / drop-path / crop off) with
return_attention_scores=True.

Tolerance of the values against torch fp32: no fixed number.  Per layer, the floor is max|torch bf16-autocast - torch
fp32| on the same weights and batch (the floor the project already uses for gradient cosines, test_parity_gpu), and the
hip backend must stay within 2 x that floor: it rounds at different points (fp32 residual stream, bf16 operands of the
projections and of QK^T, fp32 probabilities where autocast stores bf16 ones).  The per-layer figures are written to
profiles/attn_scores_model.log."""
import math
import os

import pytest
import torch

import decoder_oracle as do
from test_parity_gpu import _batch, _cfgs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")


def _engine(cfg, state=None):
    from pytorch_rt1_for_distributed_training_amd.engine.step import TrainEngine
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    torch.manual_seed(0)
    m = build_rt1(cfg)
    if state is not None:
        m.load_state_dict(state)
    return TrainEngine(m, cfg, order_probe=False, device=DEV)


@pytest.fixture(scope="module")
def twins():
    ch, ct = _cfgs(return_attention_scores=True)
    eh = _engine(ch)
    state = eh.model.state_dict()
    et = _engine(ct, state)
    eb = _engine(ct.replace(dtype="bf16"), state)
    assert eh.backend == "hip" and et.backend == eb.backend == "torch"
    return eh, et, eb


def _forward(eng, batch):
    eng.model.train()
    with torch.no_grad():
        loss, _ = eng.forward_loss(batch)
    return loss, [a.detach().float() for a in eng.model.attention_scores]


def test_hip_scores_against_torch_fp32_within_twice_the_bf16_floor(twins):
    eh, et, eb = twins
    batch = _batch(eh.cfg, b=4)
    _, sh = _forward(eh, batch)
    _, st = _forward(et, batch)
    _, sb = _forward(eb, batch)
    m = eh.model
    S, L, K = 2 * m.tokens_per_step, m.tokens_per_step, m._tokens_per_context_image
    assert S == 22 and len(sh) == len(st) == len(sb) == 8
    al = do.allowed(S, L, K, DEV)
    lines, fails = [], []
    for i, (h, t, b) in enumerate(zip(sh, st, sb)):
        assert h.shape == t.shape == (4, 8, S, S) and eh.model.attention_scores[i].dtype == torch.float32
        assert not eh.model.attention_scores[i].requires_grad
        assert not h[:, :, ~al].any(), f"layer {i}: masked entries are not exact zeros"
        assert bool((h[:, :, al] > 0).all()), f"layer {i}: an allowed entry is zero with dropout off"
        # 22 fp32 additions of entries that are each within eps_p-scale (a few 1e-4 relative, tests/attn_probs_oracle.py) of
        # exp(s - lse), whose own sum is within the stored lse's error (the same scale) of 1
        dev = float((h.double().sum(-1) - 1).abs().max())
        assert dev <= S * 2.0 ** -24 + 1e-3, (i, dev)
        floor = float((b - t).abs().max())
        err = float((h - t).abs().max())
        lines.append(f"layer {i}: max|hip - torch fp32| {err:.3e} | floor max|torch bf16-autocast - torch fp32| {floor:.3e} "
                     f"| ratio {err / floor:.3f} (limit 2) | max|row sum - 1| {dev:.2e}")
        if err > 2 * floor:
            fails.append(lines[-1])
    print("\n" + "\n".join(lines))
    try:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "attn_scores_model.log"), "w") as f:
            f.write("attention_scores, 128x128, seq_len 2, 8 layers, b 4, dropout off (tests/test_attention_scores_gpu.py)\n"
                    + "\n".join(lines) + "\n")
    except OSError as e:
        print(f"profiles/attn_scores_model.log not written: {e}")
    assert not fails, fails
    # the maps: both backends expose [b, t, 8, P] fp32 softmaxes over the positions
    mh, mt = eh.model.token_maps, et.model.token_maps
    assert mh.shape == mt.shape == (4, 2, 8, mt.shape[-1]) and mh.dtype == mt.dtype == torch.float32
    P = mt.shape[-1]
    # fp32 softmax over P positions: the normaliser is a sum of P terms (P U32 relative, common to the row), each entry
    # one division or a 1-ulp reciprocal and a product (4 U32), and this sum adds P terms again
    for maps in (mh, mt):
        assert float((maps.sum(-1) - 1).abs().max()) <= (2 * P + 8) * 2.0 ** -24 and float(maps.min()) >= 0


def test_flag_on_is_bitwise_flag_off(twins):
    eh = twins[0]
    eo = _engine(eh.cfg.replace(return_attention_scores=False), eh.model.state_dict())
    batch = _batch(eh.cfg, b=4, seed=7)
    outs = []
    for e in (eh, eo):
        loss, _ = _forward(e, batch)
        m = e.model
        images = batch["train_observation"]["image"]
        ctx = batch["train_observation"]["natural_language_embedding"]
        with torch.no_grad():
            tok = m.tokenize_images(images, ctx)
            hid = m.transformer_hidden(m.assemble_tokens(tok))
            logits = m.action_logits(hid, m._predicted_positions).float()
        outs.append((loss.clone(), logits.clone()))
    assert eo.model.attention_scores == [] and eo.model.token_maps is None
    assert len(eh.model.attention_scores) == 8
    assert torch.equal(outs[0][0], outs[1][0]), (float(outs[0][0]), float(outs[1][0]))
    assert torch.equal(outs[0][1], outs[1][1]), float((outs[0][1] - outs[1][1]).abs().max())


def test_training_mode_scores_are_the_dropped_probabilities():
    """dropout_rate = 0.1, training: every layer returns what its forward multiplied V with."""
    ch, _ = _cfgs(return_attention_scores=True, dropout_rate=0.1)
    eh = _engine(ch)
    _, sh = _forward(eh, _batch(ch, b=4))
    al = do.allowed(22, 11, 8, DEV)
    n = int(al.sum()) * 32
    for i, h in enumerate(sh):
        assert not h[:, :, ~al].any()
        share = float((h[:, :, al] == 0).float().mean())
        # binomial(n, 0.1): 8 standard deviations
        assert abs(share - 0.1) < 8 * math.sqrt(0.09 / n), (i, share)
    # scores @ V is the attention output: through RT1AttentionFn at S = 22
    from pytorch_rt1_for_distributed_training_amd.ops.attention import RT1AttentionFn
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(4, 22, 3, 8, 128, generator=g).to(torch.bfloat16).to(DEV).requires_grad_(True)
    out, probs = RT1AttentionFn.apply(qkv, 11, 8, 0.1, 12345, True)
    assert probs.shape == (4, 8, 22, 22) and probs.dtype == torch.float32 and not probs.requires_grad
    share = float((probs[:, :, al] == 0).float().mean())
    assert abs(share - 0.1) < 8 * math.sqrt(0.09 / n), share
    v = qkv.detach()[:, :, 2].double()
    pv = torch.einsum("bhij,bjhd->bihd", probs.double(), v)
    pa = torch.einsum("bhij,bjhd->bihd", probs.double(), v.abs())
    # the forward rounds every probability to bf16 before P V and stores out in bf16: round-to-nearest on 8 significand
    # bits is do.REL = 2^-8 relative each (decoder_oracle's figure for the same two roundings); the forward's own p and
    # the kernel's are each within eps_p < 2^-11 of the exact one (tests/attn_probs_oracle.py: at most 3.7e-4 on randn
    # inputs), and the fp32 accumulation of 22 terms is do.SLACK = 2^-16
    bound = (do.REL + 2.0 ** -11 + do.SLACK) * pa + do.REL * pv.abs()
    err = (pv - out.detach().double()).abs()
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    out.float().sum().backward()
    assert bool(torch.isfinite(qkv.grad.float()).all())
    # the plain call is unchanged
    out2 = RT1AttentionFn.apply(qkv.detach(), 11, 8, 0.0, 0)
    assert torch.is_tensor(out2) and out2.shape == out.shape


def test_inference_engine_graph_replay_is_the_eager_step():
    from pytorch_rt1_for_distributed_training_amd.engine.infer import InferenceEngine
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    ch, _ = _cfgs(return_attention_scores=True, seq_len=3)
    torch.manual_seed(0)
    m1 = build_rt1(ch)
    m2 = build_rt1(ch)
    m2.load_state_dict(m1.state_dict())
    eg = InferenceEngine(m1, ch, device="cuda", backend="hip", graph=True)
    ee = InferenceEngine(m2, ch, device="cuda", backend="hip", graph=False)
    T, L, K, A = eg.T, eg.L, eg.K, eg.A
    gen = torch.Generator().manual_seed(3)
    seq = 0
    for step in range(10):
        if step == 6:
            eg.reset()
            ee.reset()
            seq = 0
            assert not eg.state_maps.any()
        img = torch.randint(0, 256, (1, 3, 128, 128), generator=gen, dtype=torch.uint8)
        ctx = torch.randn(1, 512, generator=gen)
        a = eg.step(img, ctx)
        b = ee.step(img, ctx)
        assert torch.equal(a["logits"], b["logits"]), step
        assert len(eg.last_attention) == len(ee.last_attention) == 8
        for x, y in zip(eg.last_attention, ee.last_attention):
            assert x.shape == (1, 8, T * L, T * L) and torch.equal(x, y), step
        assert torch.equal(eg.last_saliency, ee.last_saliency) and torch.equal(eg.state_maps, ee.state_maps), step
        ts = min(seq, T - 1)
        rows = torch.arange(K - 1 + ts * L, K - 1 + ts * L + A, device=DEV)
        w = eg.last_attention[-1][:, :, rows].mean(dim=(1, 2)).view(1, T, L)[:, :, :K]
        assert eg.last_saliency.shape == (1, T, *eg.fmap)
        maps = eg.state_maps[:, :ts + 1]
        assert float((maps.sum(-1) - 1).abs().max()) <= (2 * maps.shape[-1] + 8) * 2.0 ** -24, step
        assert abs(float(eg.last_saliency.sum((1, 2, 3))) - float(w.sum())) <= 1e-5, step
        assert float(w.sum()) > 0
        if seq < T - 1:
            assert not eg.last_saliency[:, seq + 1:].any() and not eg.state_maps[:, seq + 1:].any(), step
        seq = min(seq + 1, T)
