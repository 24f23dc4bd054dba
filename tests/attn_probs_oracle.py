"""fp64 reference and the element-wise bound of the attention probabilities (rt1_attn_probs_kernel, and the eager
`masked_attention(..., return_scores=True)` that it stands in for), built from tests/decoder_oracle.py.

Reference, from the bf16 qkv [B, S, 3, H, 128] and a log-sum-exp lse [B, H, S] (the fp64 one of ref_attn_fwd, or the fp32
one that attn_fwd stored: then it is an input of the kernel, as in the backward kernels, and carries no error here):

    P_ref[b, h, i, j] = exp(scale32 q_i . k_j - lse[b, h, i]) keep[b, h, i, j] inv_keep     where allowed(i, j),
                        0 where masked, and 0 on every row whose lse is -inf.

Bound, per element:      |P - P_ref| <= eps_p[b, h, i] P_ref + 2^-126,
with eps_p = expm1(2 delta_s) + 2 e_exp(xmax) + (S + 4) U32 of ref_attn_fwd, the figure that decoder_oracle's docstring
(lines 20-25 and 35) applies to the p that the backward kernels recompute as `__expf(sacc * scale - lrow)`.  It covers
this kernel, which evaluates the same expression in the same order, term by term:
  * the score `sacc * scale` (MFMA over 128 exact bf16 products, fp32 additions, one product) is off by at most delta_s,
    which the exponential turns into expm1(delta_s) <= expm1(2 delta_s) relative;
  * the subtraction `- lrow` rounds once, U32 |arg| absolute, and __expf at arg costs e_exp(|arg|) = 2^-23 (1 + |arg|)
    relative.  Here arg = s - lse with max_j s <= lse <= max_j s + ln S, so |arg| <= xmax + ln S (xmax: the largest row
    maximum minus score of the case, the argument range of the forward) and
        U32 |arg| + e_exp(|arg|) = U32 (2 + 3 |arg|) <= U32 (2 + 3 xmax + 3 ln S),
    against 2 e_exp(xmax) + (S + 4) U32 = U32 (8 + 4 xmax + S): it fits with U32 (6 + xmax + S - 3 ln S) to spare, and
    S - 3 ln S >= -0.3 for every S >= 1, so with more than 5 U32 to spare;
  * `p * keep` with keep = 0 or inv_keep = 1.f / (1.f - drop_p): the subtraction, the division and the product are
    3 U32, inside what the line above leaves;
  * 2^-126 is the smallest normal fp32: below it __expf flushes (v_exp_f32 has no denormal results), and a reference
    value there has no relative accuracy to ask for.
The eager path differs in form (softmax: exp(s - max) / sum) but not in the bound: that is the forward's own p, for which
eps_p was derived (expm1(2 delta_s): numerator and denominator both move; 2 e_exp; the S-term sum and the division).

Where the reference is exactly 0 (masked, dropped, dead row) the bound is 2^-126 on paper, but the checks ask for an
exact 0.0f: nothing is computed there.
"""
import torch

import decoder_oracle as do

TINY = 2.0 ** -126


def ref_probs(qkv, lse, L, Kimg, scale, p=0.0, keep=None):
    """P_ref [B, H, S, S] fp64 from the bf16 qkv and lse [B, H, S] (any float dtype); keep: attn_keep's [B H, S, S]."""
    B, S, _, H, _ = qkv.shape
    q, k, _ = do._planes(qkv)
    al = do.allowed(S, L, Kimg, qkv.device)
    s = do.scale32(scale) * (q @ k.transpose(-1, -2))
    ls = lse.double().view(B, H, S)
    live = torch.isfinite(ls)
    ok = al & live[..., None]
    P = torch.where(ok, torch.exp(s - torch.where(live, ls, torch.zeros_like(ls))[..., None]), torch.zeros_like(s))
    return P * do._keep4(keep, B, H, S, s) * do.inv_keep(p)


def check_probs(P, ref, eps_p, name):
    """fp32 P [B, H, S, S] against ref within eps_p[b, h, i] ref + 2^-126, exact zeros where ref is 0, nothing
    non-finite.  Returns (worst error / bound, largest eps_p)."""
    assert P.dtype == torch.float32 and ref.dtype == torch.float64 and P.shape == ref.shape, (name, P.dtype, P.shape)
    o = P.double()
    assert bool(torch.isfinite(o).all()), f"{name}: non-finite probabilities"
    zero = ref == 0
    assert not o[zero].any(), f"{name}: {int((o[zero] != 0).sum())} masked / dropped / dead entries are not exact zeros"
    bound = eps_p.double()[..., None] * ref + TINY
    ratio = ((o - ref).abs() / bound)
    worst, at = ratio.reshape(-1).max(0)
    if worst.item() > 1.0:
        idx = []
        f = at.item()
        for n in reversed(P.shape):
            idx.append(f % n)
            f //= n
        idx = tuple(reversed(idx))
        raise AssertionError(f"{name}: |P - ref| is {worst.item():.3f} x the bound {bound[idx].item():.6g} at "
                             f"[b, h, i, j] = {idx}: P {o[idx].item()!r}, ref {ref[idx].item()!r}")
    return worst.item(), eps_p.max().item() if eps_p.numel() else 0.0
