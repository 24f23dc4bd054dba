"""fp64 reference and element-wise oracle for the regularised action head (csrc/kernels/head.hip,
head_ce_loss_fwd_kernel): label smoothing eps and the z-loss zeta on top of the plain cross-entropy.

tests/decoder_oracle.py's method: the reference is fp64 from the STORED bf16 operand hb and the bf16 W, the bounds are
assembled from the kernel's own operation order, and nothing in a bound is read from the output under test.
decoder_oracle.ref_head supplies z, dz, ce, bound_ce (and through it e_lse) and the plain G; what is added here:

    loss = lse - (1 - eps) z[t] - (eps / V) sum_c z[c] + zeta lse^2
    G[c] = p_c (1 + 2 zeta lse) - (1 - eps) [c == t] - eps / V,         c := 1 + 2 zeta lse below

eps and zeta reach the kernel as fp32 values, so the reference uses their fp32 images (f32 below), as
decoder_oracle.scale32 does for the attention scale.

What the kernel rounds and where (head_ce_tile<NT, true>, the body of head_ce_loss_fwd_kernel, cited by statement):
  * gather, MFMA loop, `acc[nt][i] + bc`, max / argmax, `sm[i] += __expf(acc[nt][i] - gm[i])`, the shuffles, the 4
    partials, `lse[i] = gm[i] + __logf(s)`, `ce[r] = lse[i] - tl[row]`: the statements head_ce_fwd_kernel runs too.
    ref_head's dz (a logit), e_lse (the log-sum-exp, with e_exp and e_log inside) and bound_ce hold unchanged, and ce,
    pred, hb are bitwise head_ce_fwd's (asserted on the GPU against that kernel, not here).
  * `sz[i] += z` over the lane's NT tiles, `sz[i] += __shfl_xor(sz[i], o, 64)` four times, `red_z[0][row] + red_z[1][row]
    + red_z[2][row] + red_z[3][row]`: V - 1 fp32 additions of logits that are each off by dz[c]:
        |zs - sum_c z[c]| <= sum_c dz[c] + slack(V) sum_c |z[c]|.
  * `ome = 1.f - eps; epv = eps / (float)V` (V a power of two: exact) and
    `loss[r] = lse[i] - ome * tl[row] - epv * zs + zeta * lse[i] * lse[i]`: the error of lse enters through
    lse + zeta lse^2, whose change under lse -> lse + d is d (1 + 2 zeta lse + zeta d): e_lse (1 + 2 zeta |lse| + zeta
    e_lse); z[t] carries dz[t], weighted 1 - eps; zs its bound above, weighted eps / V.  The roundings of the
    statement itself (1 - eps, two products and a subtraction, a product and a subtraction, two products and an
    addition: 8 operations, with or without fma contraction, each relative to a partial result that is at most the sum
    of the absolute terms):  K U32 (|lse| + (1 - eps) |z[t]| + (eps / V) sum_c |z[c]| + zeta lse^2),  K = 8.
        |loss - ref| <= e_lse (1 + 2 zeta |lse| + zeta e_lse) + (1 - eps) dz[t]
                        + (eps / V) (sum_c dz[c] + slack(V) sum_c |z[c]|)
                        + K U32 (|lse| + (1 - eps) |z[t]| + (eps / V) sum_c |z[c]| + zeta lse^2)
  * `c = 1.f + 2.f * zeta * lse[i]` and `g = __expf(acc[nt][i] - lse[i]) * c - (col == tgt[i] ? ome : 0.f) - epv;
    grow[col] = f2bf(g)`: the exponential is ref_head's, relative error e = expm1(max_c dz + e_lse + ..) + e_exp (its
    `eps` term, recomputed here from the same quantities and tied to ref_head's bound_G by an assertion); c is off by
    2 zeta e_lse plus three roundings, the two
    subtractions and the product round relative to sm |c| + (1 - eps) onehot + eps / V (SLACK = 2^-16 covers those six
    fp32 roundings), and the store rounds to bf16:
        |G - ref| <= REL |ref| + (e + SLACK) (sm |c| + (1 - eps) onehot + eps / V) + 2 zeta e_lse sm.
  At eps = zeta = 0 both bounds fall back to ref_head's (the loss bound to bound_ce's terms, with K U32 in place of
  U32), and the kernel is then also held to head_ce_fwd's bits.

`emulate` is a torch fp32 model of the kernel (CPU tests): the same formulas in fp32 on the same operands, without
__expf / __logf (their terms e_exp, e_log are inside e_lse), with switches that each break one thing the oracle must see.
"""
import math

import torch

import decoder_oracle as do

BF = torch.bfloat16
REL, SLACK, U32 = do.REL, do.SLACK, do.U32
slack = do.slack
K_FINAL = 8

# the grid of tests/test_head_loss_gpu.py, shared with the CPU emulation test
HEAD_R = {1: (1, 1), 15: (3, 5), 16: (2, 8), 17: (1, 17), 90: (5, 18)}      # R = B * P
HEAD_S = 22
VOCABS = (256, 512, 1024)
OBJECTIVES = ((0.1, 0.0), (0.0, 1e-4), (0.1, 1e-4), (0.5, 1e-2))            # (eps, zeta)


def gen(*key):
    """tests/test_decoder_oracle_gpu.py's generator recipe."""
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31)
    return torch.Generator(device="cpu").manual_seed(seed)


def head_inputs(V, R, g, device="cpu"):
    """The operands as tests/test_decoder_oracle_gpu.py's head_inputs makes them (same draws in the same order; the
    GPU test asserts the equality), on any device: positions out of order with both ends of the sequence, targets that
    include column 0 and column V - 1."""
    B, P = HEAD_R[R]
    hidden = torch.randn(B, HEAD_S, 512, generator=g)
    W = (torch.randn(V, 512, generator=g) * 0.05).to(BF)
    bias = torch.randn(V, generator=g) * 0.2
    pos = torch.randperm(HEAD_S, generator=g)[:P]
    target = torch.randint(0, V, (R,), generator=g)
    if P >= 2:
        pos[0], pos[1] = HEAD_S - 1, 0
        target[0], target[-1] = V - 1, 0
    else:
        pos[0] = HEAD_S - 1 if V > 256 else 0
        target[0] = V - 1 if V == 512 else 0
    return (hidden.to(device), pos.int().to(device), W.to(device), bias.to(device), target.int().to(device)), (B, P)


def f32(x):
    """The fp32 image of a host scalar, as a Python float."""
    return torch.tensor(float(x), dtype=torch.float32).double().item()


def ref_head_loss(hb, W, bias, target, eps, zeta):
    """From the stored operand hb [R, 512] bf16: ref_head's dict plus loss, bound_loss [R]; G, bound_G, S_G [R, V] of
    the regularised objective (ce, bound_ce, pred, clear stay ref_head's: the plain cross-entropy)."""
    r = do.ref_head(hb, W, bias, target)
    z, dz = r["z"], r["dz"]
    R, V = z.shape
    eps, zeta = f32(eps), f32(zeta)
    t = target.long().view(R, 1)
    lse = torch.logsumexp(z, 1)
    zmax = z.amax(1)
    xmax = (zmax[:, None] - z).amax(1)
    dzm = dz.amax(1)
    zt, dzt = z.gather(1, t)[:, 0], dz.gather(1, t)[:, 0]
    # ref_head's e_lse and the relative error e of its exponentials, from the same quantities; each is tied to a bound
    # that ref_head returns, so a change there cannot go unnoticed here
    e_lse = dzm + do.e_exp(xmax) + do.e_log(V) + U32 * (zmax.abs() + lse.abs())
    assert torch.allclose(r["bound_ce"], U32 * r["ce"].abs() + e_lse + dzt, rtol=1e-12, atol=0.0)
    e = torch.expm1(dzm + e_lse + U32 * (zmax.abs() + lse.abs() + xmax)) + do.e_exp(xmax + math.log(V))
    sm = torch.exp(z - lse[:, None])
    onehot = torch.zeros_like(z).scatter_(1, t, 1.0)
    # ... and e to ref_head's bound of the plain G, which is the bound below at eps = zeta = 0
    plain_bound = REL * r["G"].abs() + (e[:, None] + SLACK) * (sm + onehot)
    assert torch.allclose(r["bound_G"], plain_bound, rtol=1e-12, atol=0.0)
    c = 1.0 + 2.0 * zeta * lse
    sabs = z.abs().sum(1)
    loss = lse - (1.0 - eps) * zt - (eps / V) * z.sum(1) + zeta * lse * lse
    b_loss = (e_lse * (1.0 + 2.0 * zeta * lse.abs() + zeta * e_lse) + (1.0 - eps) * dzt
              + (eps / V) * (dz.sum(1) + slack(V) * sabs)
              + K_FINAL * U32 * (lse.abs() + (1.0 - eps) * zt.abs() + (eps / V) * sabs + zeta * lse * lse))
    G = sm * c[:, None] - (1.0 - eps) * onehot - eps / V
    S_G = sm * c.abs()[:, None] + (1.0 - eps) * onehot + eps / V
    b_G = REL * G.abs() + (e[:, None] + SLACK) * S_G + 2.0 * zeta * (e_lse[:, None] * sm)
    out = dict(r)
    out.update(loss=loss, bound_loss=b_loss, G=G, bound_G=b_G, S_G=S_G, lse=lse, e_lse=e_lse)
    return out


def check_head_loss(loss, ce, G, r, name):
    """loss [R] fp32, ce [R] fp32 and G [R, V] bf16 against ref_head_loss's dict: every element within its hard bound,
    no share left out.  Returns the worst ratios {loss, ce, G}."""
    a = do.check_f32(loss, r["loss"], r["bound_loss"], "head loss " + name)
    b = do.check_f32(ce, r["ce"], r["bound_ce"], "head ce " + name)
    c = do.check_bf16(G, r["G"], r["bound_G"], "head G " + name, None, r["S_G"])
    return {"loss": a["worst"], "ce": b["worst"], "G": c["worst_hard"]}


def ratios(loss, G, r):
    """Largest |out - ref| / bound of loss and of G (figures for a log; the assertions are check_head_loss's)."""
    q = lambda out, ref, b: float(((out.double() - ref).abs() / b.clamp_min(1e-300)).max())
    return q(loss, r["loss"], r["bound_loss"]), q(G, r["G"], r["bound_G"])


MUTATIONS = ("no_uniform", "no_one_minus_eps", "no_c", "zeta_lse", "quarter_sum", "swap")


def emulate(hb, W, bias, target, eps, zeta, mutate=None):
    """torch fp32 model of head_ce_loss_fwd_kernel on the stored operands -> (loss, ce fp32 [R], G bf16 [R, V]).
    mutate (one of MUTATIONS) breaks one thing:
      no_uniform        the -eps / V term is missing from G
      no_one_minus_eps  the target term of G and of the loss has weight 1, not 1 - eps
      no_c              the factor 1 + 2 zeta lse is missing from G
      zeta_lse          zeta * lse in place of zeta * lse^2
      quarter_sum       the row sum of z misses the last wave's quarter of the columns
      swap              loss and ce change places"""
    assert mutate is None or mutate in MUTATIONS, mutate
    R, V = hb.shape[0], W.shape[0]
    f = torch.float32
    eps32, zeta32 = torch.tensor(eps, dtype=f), torch.tensor(zeta, dtype=f)
    z = hb.to(f) @ W.to(f).t() + bias.to(f)
    t = target.long().view(R, 1)
    m = z.amax(1)
    lse = m + torch.log(torch.exp(z - m[:, None]).sum(1))
    zt = z.gather(1, t)[:, 0]
    zs = (z[:, :3 * V // 4] if mutate == "quarter_sum" else z).sum(1)
    ome = torch.tensor(1.0, dtype=f) if mutate == "no_one_minus_eps" else 1.0 - eps32
    epv = eps32 / V
    ce = lse - zt
    reg = zeta32 * lse if mutate == "zeta_lse" else zeta32 * lse * lse
    loss = lse - ome * zt - epv * zs + reg
    c = torch.ones_like(lse) if mutate == "no_c" else 1.0 + 2.0 * zeta32 * lse
    onehot = torch.zeros_like(z).scatter_(1, t, 1.0)
    g = torch.exp(z - lse[:, None]) * c[:, None] - ome * onehot
    if mutate != "no_uniform":
        g = g - epv
    if mutate == "swap":
        loss, ce = ce, loss
    return loss, ce, g.to(BF)
