"""The oracle of the attention probabilities checks itself on the CPU: the eager fp32
`masked_attention(..., return_scores=True)` (what `TransformerNetwork.attention_scores` holds on the torch backend, and
what the `attn_probs` kernel reproduces on the hip backend) stays inside the element-wise fp64 bound of
tests/attn_probs_oracle.py,

    |P - P_ref| <= eps_p[b, h, i] P_ref + 2^-126,     P_ref = exp(scale32 q . k - lse) keep inv_keep where allowed, else 0,

whose derivation is in that module's docstring (eps_p is ref_attn_fwd's: expm1(2 delta_s) + 2 e_exp(xmax) + (S + 4) U32;
the score error is delta_s, and the argument's own rounding and e_exp(|arg|), |arg| <= xmax + ln S, fit inside
2 e_exp(xmax) + (S + 4) U32).  The bound is wide for an fp32 evaluation (the worst error printed below is well under 1 %
of it; eps_p is a few 1e-4) and narrow for a wrong key, mask, scale or row, which move an entry by factors.  Masked
entries must be exact zeros and, with p = 0, live rows sum to 1 within S 2^-24."""
import pytest
import torch

import attn_probs_oracle as apo
import decoder_oracle as do
from pytorch_rt1_for_distributed_training_amd.models.transformer import masked_attention

BF = torch.bfloat16
D = 128
SCALE = D ** -0.5
# (B, H, S, L, K)
CASES = [(2, 8, 66, 11, 8), (3, 3, 66, 11, 8), (2, 8, 165, 11, 8), (2, 8, 256, 11, 8), (2, 8, 253, 7, 4),
         (2, 8, 17, 11, 8), (2, 8, 66, 11, 11)]


@pytest.mark.parametrize("B,H,S,L,K", CASES)
def test_eager_scores_within_the_fp64_bound(B, H, S, L, K):
    g = torch.Generator().manual_seed(1000 * S + 100 * B + 10 * L + K)
    qkv = torch.randn(B, S, 3, H, D, generator=g).to(BF)
    r = do.ref_attn_fwd(qkv, L, K, SCALE)
    ref = apo.ref_probs(qkv, r["lse"], L, K, SCALE)
    q, k, v = (qkv[:, :, t].float().permute(0, 2, 1, 3) for t in range(3))
    al = do.allowed(S, L, K)
    _, P = masked_attention(q, k, v, al.to(torch.uint8), 0.0, False, return_scores=True)
    assert P.dtype == torch.float32 and P.shape == (B, H, S, S)
    worst, eps = apo.check_probs(P, ref, r["eps_p"], f"eager B{B} H{H} S{S} L{L} K{K}")
    print(f"\nattn_probs oracle | eager fp32 | B{B} H{H} S{S} L{L} K{K} | worst / bound {worst:.4f} | max eps_p {eps:.3e}",
          end="")
    assert not P[:, :, ~al].any(), "masked entries are not exact zeros"
    live = al.any(-1)
    sums = P.double().sum(-1)[:, :, live]
    assert float((sums - 1.0).abs().max()) <= S * 2.0 ** -24, float((sums - 1.0).abs().max())


def test_the_bound_rejects_a_wrong_key_mask_scale_and_row():
    """The oracle is not vacuous: the neighbouring key, a causal-only mask, scale / 2 and the neighbouring row each
    leave the bound."""
    B, H, S, L, K = 2, 8, 66, 11, 8
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B, S, 3, H, D, generator=g).to(BF)
    r = do.ref_attn_fwd(qkv, L, K, SCALE)
    ref = apo.ref_probs(qkv, r["lse"], L, K, SCALE)
    good = ref.float()
    apo.check_probs(good, ref, r["eps_p"], "fp32 image of the reference")
    q, k, v = (qkv[:, :, t].float().permute(0, 2, 1, 3) for t in range(3))
    al = do.allowed(S, L, K)
    wrong = {
        "key": masked_attention(q, torch.roll(k, 1, 2), v, al.to(torch.uint8), 0.0, False, True)[1],
        "mask": masked_attention(q, k, v, do.allowed(S, L, L).to(torch.uint8), 0.0, False, True)[1],
        "scale": masked_attention(q * 0.5, k, v, al.to(torch.uint8), 0.0, False, True)[1],
        "row": torch.roll(good, 1, 2) * al,
    }
    for name, P in wrong.items():
        with pytest.raises(AssertionError):
            apo.check_probs(P.float().contiguous(), ref, r["eps_p"], name)
