"""fp64 references and the element-wise oracle for the decoder kernels (csrc/kernels/attention.hip, transformer.hip,
head.hip).

Plain torch, CPU or GPU tensors, no extension call.  qkv is the fused projection [B, S, 3, H, D] bf16 (D = 128), out /
dout [B, S, H, D] bf16, lse [B, H, S] fp32; the row kernels work on [T, 512]; the head on hidden [B, S, 512] fp32, W
[V, 512] bf16.  Every reference returns fp64 values with, next to each, S: the same expression over absolute values
(glue_oracle's convention).  The references index [B, S, 3, H, D] directly, so a kernel that confuses bh / H with bh % H
or the q / k / v planes cannot pass.

What the kernels round and where, read from the .hip files and cited by line:
  attention forward (rt1_attn_fwd_kernel)
  * scores: `sacc[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[ks], kf, sacc[kb], 0, 0, 0)` over D / 32 = 4 chunks:
    exact bf16 products, 128 fp32 additions; then `sacc[kb][r] * scale` (one rounding; scale is the fp32 image of
    D^-0.5 and the reference uses that image).  Absolute error of a score <= slack(128) Sqk[i, j] =: within delta_s[i].
  * `__expf(sacc[kb][r] - mx[r])` compiles (hipcc -O3, gfx950; read in the disassembly) to v_sub_f32, v_mul_f32 by
    0x3fb8aa3b (log2 e) and v_exp_f32, with no range reduction around it.  With glue_oracle's premise "a 1-ulp v_exp"
    (2^-23 relative) and the rounding of the scaled argument (the product x log2(e) is off by U32 |x log2 e| plus the
    2^-25 relative error of the constant, which the exponential turns into <= 1.5 U32 |x| ln 2 log2 e relative):
        e_exp(x) = 2^-23 (1 + |x|),        x the argument, |x| <= the largest row maximum minus score of the case.
  * `sm[r] += e` then 4 shuffle additions: <= S fp32 additions of positive terms, S U32 relative; `p = sacc[kb][r] /
    sm[r]` and `p * inv_keep` with `inv_keep = 1.f / (1.f - drop_p)`: 4 more roundings.  A shift of every score of a
    row by <= delta_s moves the numerator and the denominator of p by e^(+-delta_s) each.  So, relative, before the
    bf16 image,     eps_p[i] = expm1(2 delta_s[i]) + 2 e_exp + (S + 4) U32
    (the issue's 2 delta_s + e_exp with the second e_exp of the denominator and the division / sum roundings that it
    left out; together they are below 2^-14 against REL = 2^-8).
  * `P[(4 * lg + r) * Sp + j] = f2bf(p)`: every Pd is rounded to bf16, REL relative, before the second MFMA, whose
    products are again exact and added in fp32 (`oacc[db] = ...mfma...(pf, vf, oacc[db], 0, 0, 0)`, <= S additions),
    and `orow[db * 16 + lr] = f2bf(oacc[db][r])` is the one store.
  * `lse[(int64_t)bh * S + i] = (sm[r] > 0.f) ? mx[r] + __logf(sm[r]) : -INFINITY`.  __logf compiles to v_log_f32 and a
    two-term product with ln 2 (v_mul_f32 by 0x3f317217 and a v_fma_f32 with the low part): a 1-ulp log2 (2^-23
    relative to |log2 sm|) and a product good to 2^-24.  sm itself carries S U32 + e_exp relative, which the logarithm
    turns into the same figure absolute:    e_log(n) = 2^-22 ln(n) + n U32    for a sum of n terms in [0, 1], one of
    them 1 (e_exp is added by the caller).  The log-sum-exp is 1-Lipschitz in the scores in max norm: delta_s[i].
  attention backward (rt1_attn_bwd_kernel, rt1_attn_bwd_dkdv_kernel, rt1_attn_bwd_dq_kernel)
  * `const float p = __expf(sacc[kb][r] * scale - lrow[r])` from the stored lse (an input here): the same eps_p bounds
    it.  `pd = p * keep` and `ds = p * (pacc[kb][r] * keep - drow[r]) * scale` with pacc = dO V^T on MFMA (128 fp32
    additions, relative to Sdp = |dO| |V|^T) and `delta[r] = acc` = dO . O in fp32 (`acc = ... + ...; wave_sum`, 128
    terms, relative to Sdelta): the error of one dS before its store is
        e_ds = eps_p S_ds + slack(128) P (Sdp keep + Sdelta) scale,   S_ds = P (|dPd| keep + |delta|) scale.
  * `Pds[...] = f2bf(pd); dSs[...] = f2bf(ds)` (`Tp[...] = f2bf(pd); Ts[...] = f2bf(ds)` in the streamed kernels):
    REL on each operand of the three products dV = Pd^T dO, dQ = dS K, dK = dS^T Q, which accumulate <= S exact
    products in fp32 and are stored once (`krow[db * 16 + lr] = f2bf(kacc[db][r])`).
  transformer.hip: all fp32, one store.
  * ln_fwd_kernel / resid_kernel: `s += v[j]` (8 serial additions) and wave_sum (6 more): mu is off by at most
    dmu = U32 |mu| + slack(512) mean|x|.  `v[j] -= m; q = fmaf(v[j], v[j], q)`: the variance is taken around the
    kernel's m, which adds (m - mu)^2 <= dmu^2 exactly, plus 3 U32 per square and the 14 additions:
    relative to var + eps, <= slack(512) + dmu^2 / (var + eps).  rsqrtf halves that and adds its ulp; with `+ eps`
    and the product by 1 / E:      e_rs = slack(512) + 2^-22 + dmu^2 / (var + eps),  |rs - ref| <= e_rs ref.
    `v[j] = fmaf(v[j] * r, gg[j], bb[j])` then store8: y carries the kernel's own m and r,
        |y - ref| <= REL |ref| + (e_rs |x - mu| + (1 + e_rs) dmu) rs |g| + SLACK S,   S = |x - mu| rs |g| + |b|,
    which is the issue's REL |ref| + slack(512) S with the error of mu (relative to mean|x|, not to |x - mu|) and of
    rs carried explicitly.
  * resid_kernel: `float h = av[j] + bb[j]; h = dropped(...) ? 0.f : h * ik; xv[j] += h`: three roundings and the two
    of ik: f32 bound with n = 5, S = |x| + keep (|a| + |bias|) / (1 - p).
  * ln_bwd_kernel: xhat = `(xv[j] - m) * r` from the stored mu / rs, `s1 += gd; s2 = fmaf(gd, xv[j], s2)` then
    wave_sum * (1 / E), `o[j] += r * (d[j] * gg[j] - s1 - xv[j] * s2)`: f32 bound with n = 512 relative to
    S = |dres| + rs (|gd| + mean|gd| + |xhat| mean|gd xhat|).  `ag[j] = fmaf(d[j], xv[j], ag[j]); ab[j] += d[j]` over
    the rows of the grid-stride loop, then 4 waves, then the partial rows: T additions, each term with its own
    evaluation error (extra = SLACK).  `as[j] += o[j]` sums the fp32 dx as stored.  `store8(dxb + ..., o)` rounds the
    stored dx: bit-equal to dx.to(bf16).
  * drop_bwd_kernel: `d[j] = dropped(...) ? 0.f : d[j] * ik` then store8: gemm_oracle's tight bound with n = 1;
    `acc[j] += d[j]` sums the unrounded values over T rows.
  head.hip (head_ce_fwd_kernel)
  * `store8(hb + (int64_t)r * E + c0 + 8 * i, t8)`: hb = bf16(hidden[b, pos[p]]) and the same image feeds the MFMA.
  * `acc[nt] = ...mfma...(a, bw, acc[nt], 0, 0, 0)` over 512 / 32 chunks and `acc[nt][i] + bc`: a logit is off by
    dz = U32 |z| + slack(513) Sz, Sz = |hb| |W|^T + |bias|.
  * `sm[i] += __expf(acc[nt][i] - gm[i])`, shuffles, 4 partials; `lse[i] = gm[i] + __logf(s)`;
    `ce[r] = lse[i] - tl[4 * lg + i]`: the log-sum-exp is 1-Lipschitz in the logits, so
        e_lse = max_c dz + e_exp + e_log(V) + U32 (|max z| + |lse|),    |ce - ref| <= U32 |ref| + e_lse + dz[target]:
    the f32 bound over 512 + V terms (513 in dz, V in e_log) plus e_exp and e_log.
  * `g = __expf(acc[nt][i] - lse[i]) - (col == tgt[i] ? 1.f : 0.f); grow[col] = f2bf(g)`: the argument is off by
    dz + e_lse and its own rounding, |argument| <= (max z - min z) + ln V:
        |G - ref| <= REL |ref| + (eps + SLACK)(softmax + onehot),   eps = expm1(max_c dz + e_lse + ..) + e_exp.
  * argmax: `if (z > mx[i])` in column order per lane, `om == mx[i] && oi < ix[i]` across lanes, `red_m[w][row] > m`
    across waves in column order: the first maximum.
  * head_ce_scale_kernel: `v[j] *= s; store8`: tight with n = 1.

Bounds.  REL = 2^-8, SLACK = 2^-16, BIAS_* are glue_oracle's, U32 = 2^-24 and slack(n) = max(SLACK, n U32)
gemm_oracle's, CAP = 2^-10 dw_oracle's CAP_DY.  For a product out = sum_j A[i, j] b[j, d] whose A is rounded to bf16:
  hard   |out - ref| <= REL |ref| + sum_j (REL |A| + e_A + slack(n) |A|) |b|      on every element;
  tight  REL |ref| + sum_j (e_A + slack(n) |A|) |b| + 4 REL sqrt(sum_j (A b)^2)   on all but CAP of the elements of a
         case: the n roundings are bounded by REL |A b| each, and Hoeffding's inequality for their sum at
         t = 4 REL sqrt(Q) gives 2 e^-8 = 6.7e-4 < 2^-10;
  bias   the mean signed bf16-ulp error of the forward's out over the elements with |ref| > BIAS_FLOOR S_out, in a case
         with >= BIAS_MIN_COUNT of them.  glue_oracle's BIAS_CAP = 0.01 is 10 sigma of the mean of 1e5 store errors
         uniform in +- 0.5 ulp, on the premise that the store is the only rounding that matters.  Here it is not: the
         bf16 images of Pd come before it, and where the terms of an element cancel (|ref| down to 2^-10 S_out) their
         sum is tens of ulps of that element.  The all-round-to-nearest emulation of tests/test_decoder_oracle.py gives
         -0.021 at S = 88, p = 0: noise of the statistic, not a bias of a store.  So, as gemm_oracle.assert_within
         does for the z-mode dx, the same 10-sigma rule is applied to the sigma this statistic has, from the number
         formats alone: the rounding of Pd[i, j] is uniform in +- REL Pd[i, j], variance (REL Pd[i, j])^2 / 3, and
         reaches the weighted sum of errors sum w (out - ref), w = sign(ref) / ulp(ref) on the counted elements, through
         sum_d w[i, d] v[j, d] (one rounded Pd feeds the 128 outputs of its row: the covariance is kept, not bounded):
             Var = sum_ij (REL Pd[i, j])^2 / 3 (sum_d w[i, d] v[j, d])^2 + n / 12,
             cap = max(BIAS_CAP, BIAS_SIGMAS sqrt(Var) / n),     asserted while cap <= BIAS_CAP_MAX = 0.25,
         half the shift of a truncating store (gemm_oracle's BIAS_SIGMAS = 10 and BIAS_CAP_MAX).  Nothing in the cap
         is read from the output under test;
  zero   where a bound is exactly 0 the output must be exactly 0 (fully masked rows at Kimg = 0, dK / dV of the
         trailing action tokens that no query attends to, rows whose every kept key was dropped).
"""
import math

import torch

import dw_oracle as dwo
import gemm_oracle as gm
import glue_oracle as go

BF = torch.bfloat16
REL, SLACK, U32 = go.REL, go.SLACK, gm.U32
CAP = dwo.CAP_DY
slack = gm.slack
D = 128
E = 512
M32 = 0xFFFFFFFF


def e_exp(x):
    """Relative error of __expf at argument x (tensor or float): see the docstring."""
    return 2.0 ** -23 * (1.0 + abs(x))


def e_log(n):
    """Absolute error of __logf of a sum of n terms in [0, 1] that holds a 1: see the docstring."""
    return 2.0 ** -22 * math.log(max(n, 2)) + n * U32


# ---- mask and hashes -------------------------------------------------------------------------------------------------
def allowed(S, L, Kimg, device="cpu"):
    """[S, S] bool: j <= i and not (act(i) and act(j)), act(p) = p % L >= Kimg (attn_allowed)."""
    p = torch.arange(S, device=device)
    act = (p % L) >= Kimg
    return (p[None, :] <= p[:, None]) & ~(act[:, None] & act[None, :])


def _mul(a, c):
    return (a * c) & M32       # int64 wraps mod 2^64: the low 32 bits are those of the 32-bit product


def _finish(x):
    x = x ^ (x >> 16)
    x = _mul(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul(x, 0x846CA68B)
    return x ^ (x >> 16)


def dev_seed(seed, counter):
    """salt + counter * golden (common.h dev_seed); counter None, an int or a 1-element int32 tensor."""
    if counter is None:
        return int(seed) & M32
    c = int(counter.item()) if torch.is_tensor(counter) else int(counter)
    return (int(seed) + (c & M32) * 0x9E3779B1) & M32


def _below(x, p):
    """(float)(x >> 8) * 2^-24 < (float)p, exactly: x >> 8 < 2^24 is an fp32 integer."""
    p32 = torch.tensor(float(p), dtype=torch.float32).double().item()
    return (x >> 8).double() * 2.0 ** -24 < p32


def attn_keep(seed, counter, BH, S, p, device="cpu"):
    """[BH, S, S] bool, True = kept: hash_uniform(seed, bh, i, j) >= p of attention.hip."""
    s = dev_seed(seed, counter)
    a = torch.arange(BH, dtype=torch.int64, device=device)[:, None, None]
    i = torch.arange(S, dtype=torch.int64, device=device)[None, :, None]
    j = torch.arange(S, dtype=torch.int64, device=device)[None, None, :]
    x = s ^ _mul(a, 0x9E3779B1) ^ _mul(i, 0x85EBCA77) ^ _mul(j, 0xC2B2AE3D)
    return ~_below(_finish(x), p)


def row_keep(seed, counter, T, p, device="cpu"):
    """[T, 512] bool, True = kept: !dropped(seed, row, col, p) of transformer.hip (mix32)."""
    s = dev_seed(seed, counter)
    r = torch.arange(T, dtype=torch.int64, device=device)[:, None]
    c = torch.arange(E, dtype=torch.int64, device=device)[None, :]
    x = s ^ _mul(r, 0x9E3779B1) ^ _mul(c, 0x85EBCA77) ^ 0x27D4EB2F
    return ~_below(_finish(x), p)


def inv_keep(p):
    p32 = torch.tensor(float(p), dtype=torch.float32).double().item()
    return 1.0 / (1.0 - p32) if p > 0 else 1.0


def scale32(scale):
    return torch.tensor(float(scale), dtype=torch.float32).double().item()


# ---- attention -------------------------------------------------------------------------------------------------------
def _planes(qkv):
    """q, k, v as [B, H, S, D] fp64."""
    return tuple(qkv[:, :, t].double().permute(0, 2, 1, 3) for t in range(3))


def _keep4(keep, B, H, S, like):
    if keep is None:
        return torch.ones(B, H, S, S, dtype=torch.float64, device=like.device)
    return keep.view(B, H, S, S).to(like.device).double()


def ref_attn_fwd(qkv, L, Kimg, scale, p=0.0, keep=None):
    """out = (softmax(scale q k^T, masked) * keep / (1 - p)) v and lse, fp64 from the bf16 qkv.  keep: attn_keep's
    [B H, S, S] (None: nothing dropped).  Returns a dict: out, S_out, Q (sum of squared terms) [B, S, H, D]; lse,
    delta_s, eps_p [B, H, S]."""
    B, S, _, H, _ = qkv.shape
    q, k, v = _planes(qkv)
    sc = scale32(scale)
    al = allowed(S, L, Kimg, qkv.device)
    s = sc * (q @ k.transpose(-1, -2))
    Sqk = torch.where(al, sc * (q.abs() @ k.abs().transpose(-1, -2)), torch.zeros_like(s))
    sm = torch.where(al, s, torch.full_like(s, float("-inf")))
    lse = torch.logsumexp(sm, -1)
    live = torch.isfinite(lse)
    P = torch.where(al & live[..., None], torch.exp(s - torch.where(live, lse, torch.zeros_like(lse))[..., None]),
                    torch.zeros_like(s))
    Pd = P * _keep4(keep, B, H, S, s) * inv_keep(p)
    delta_s = slack(D) * Sqk.amax(-1)
    mx = sm.amax(-1)
    xmax = torch.where(al & live[..., None], torch.where(live, mx, torch.zeros_like(mx))[..., None] - s,
                       torch.zeros_like(s)).amax(-1)
    eps_p = torch.expm1(2 * delta_s) + 2 * e_exp(xmax) + (S + 4) * U32
    tr = lambda t: t.permute(0, 2, 1, 3)
    return {"out": tr(Pd @ v), "S_out": tr(Pd @ v.abs()), "Q": tr((Pd * Pd) @ (v * v)), "lse": lse, "delta_s": delta_s,
            "eps_p": eps_p, "xmax": xmax.max().item() if xmax.numel() else 0.0, "n": S, "Pd": Pd, "v": v}


def bounds_attn_fwd(r):
    """(hard, tight) of out and the bound of lse from ref_attn_fwd's dict."""
    S = r["n"]
    eps = r["eps_p"].permute(0, 2, 1)[..., None]           # [B, S, H, 1]
    hard = REL * r["out"].abs() + (REL + eps + slack(S)) * r["S_out"]
    tight = REL * r["out"].abs() + (eps + slack(S)) * r["S_out"] + 4 * REL * torch.sqrt(r["Q"])
    fin = torch.isfinite(r["lse"])
    lse0 = torch.where(fin, r["lse"], torch.zeros_like(r["lse"]))
    b_lse = U32 * lse0.abs() + r["delta_s"] + e_exp(r["xmax"]) + e_log(S)
    return hard, tight, b_lse


def ref_attn_bwd(qkv, out, lse, dout, L, Kimg, scale, p=0.0, keep=None):
    """dqkv [B, S, 3, H, D] fp64 from qkv, dout and the STORED out / lse (the kernel's inputs), with its hard and tight
    bounds: dict ref / hard / tight."""
    B, S, _, H, _ = qkv.shape
    q, k, v = _planes(qkv)
    tr = lambda t: t.permute(0, 2, 1, 3)
    dO, O = tr(dout.double()), tr(out.double())
    sc, ik = scale32(scale), inv_keep(p)
    al = allowed(S, L, Kimg, qkv.device)
    zero = torch.zeros(B, H, S, S, dtype=torch.float64, device=qkv.device)
    s = sc * (q @ k.transpose(-1, -2))
    Sqk = torch.where(al, sc * (q.abs() @ k.abs().transpose(-1, -2)), zero)
    ls = lse.double().view(B, H, S)
    live = torch.isfinite(ls)
    arg = s - torch.where(live, ls, torch.zeros_like(ls))[..., None]
    ok = al & live[..., None]
    P = torch.where(ok, torch.exp(arg), zero)
    kp = _keep4(keep, B, H, S, s) * ik
    Pd = P * kp
    dPd = dO @ v.transpose(-1, -2)
    Sdp = dO.abs() @ v.abs().transpose(-1, -2)
    delta = (dO * O).sum(-1)[..., None]
    Sdelta = (dO.abs() * O.abs()).sum(-1)[..., None]
    dS = P * (dPd * kp - delta) * sc
    S_ds = P * (dPd.abs() * kp + delta.abs()) * sc
    delta_s = slack(D) * Sqk.amax(-1)
    xmax = torch.where(ok, arg.abs(), zero).amax(-1)
    eps = (torch.expm1(2 * delta_s) + 2 * e_exp(xmax) + (S + 4) * U32)[..., None]
    e_ds = eps * S_ds + slack(D) * P * (Sdp * kp + Sdelta) * sc
    sl = slack(S)
    T_ = lambda t: t.transpose(-1, -2)
    dV, dQ, dK = T_(Pd) @ dO, dS @ k, T_(dS) @ q
    hV = REL * dV.abs() + T_((REL + eps + sl) * Pd) @ dO.abs()
    tV = REL * dV.abs() + T_((eps + sl) * Pd) @ dO.abs() + 4 * REL * torch.sqrt(T_(Pd * Pd) @ (dO * dO))
    a_h, a_t = REL * dS.abs() + e_ds + sl * dS.abs(), e_ds + sl * dS.abs()
    hQ = REL * dQ.abs() + a_h @ k.abs()
    tQ = REL * dQ.abs() + a_t @ k.abs() + 4 * REL * torch.sqrt((dS * dS) @ (k * k))
    hK = REL * dK.abs() + T_(a_h) @ q.abs()
    tK = REL * dK.abs() + T_(a_t) @ q.abs() + 4 * REL * torch.sqrt(T_(dS * dS) @ (q * q))
    pack = lambda a, b, c: torch.stack([tr(a), tr(b), tr(c)], 2)       # [B, S, 3, H, D]
    return {"ref": pack(dQ, dK, dV), "hard": pack(hQ, hK, hV), "tight": pack(tQ, tK, tV)}


# ---- transformer.hip -------------------------------------------------------------------------------------------------
def ref_ln_fwd(x, g, b, eps):
    """LayerNorm of x [T, 512] fp32 -> dict y, S, bound_y [T, 512]; mu, rs, bound_mu, bound_rs [T]."""
    xd, gd, bd = x.double(), g.double(), b.double()
    mu = xd.mean(1)
    xc = xd - mu[:, None]
    var = (xc * xc).mean(1)
    rs = 1.0 / torch.sqrt(var + eps)
    dmu = U32 * mu.abs() + slack(E) * xd.abs().mean(1)
    e_rs = slack(E) + 2.0 ** -22 + dmu * dmu / (var + eps)
    y = xc * rs[:, None] * gd + bd
    S = xc.abs() * rs[:, None] * gd.abs() + bd.abs()
    by = REL * y.abs() + (e_rs[:, None] * xc.abs() + ((1 + e_rs) * dmu)[:, None]) * rs[:, None] * gd.abs() + SLACK * S
    return {"y": y, "S": S, "bound_y": by, "mu": mu, "rs": rs, "bound_mu": dmu, "bound_rs": e_rs * rs}


def ref_resid(x, a, bias, p=0.0, keep=None):
    """out = x + keep (a + bias) / (1 - p) -> (ref, S)."""
    h = a.double() + bias.double()
    ha = a.double().abs() + bias.double().abs()
    if p > 0:
        kp = keep.to(x.device).double() * inv_keep(p)
        h, ha = h * kp, ha * kp
    return x.double() + h, x.double().abs() + ha


def ref_ln_bwd(dy, x, mu, rs, g, dres=None):
    """dx = dres + rs (g dy - mean(g dy) - xhat mean(g dy xhat)) from the STORED mu / rs -> dict dx, S_dx [T, 512];
    dg, S_dg, db, S_db [512]."""
    d, gd_ = dy.double(), g.double()
    r = rs.double()[:, None]
    xh = (x.double() - mu.double()[:, None]) * r
    gd = d * gd_
    s1, s2 = gd.mean(1, keepdim=True), (gd * xh).mean(1, keepdim=True)
    a1, a2 = gd.abs().mean(1, keepdim=True), (gd * xh).abs().mean(1, keepdim=True)
    dx = r * (gd - s1 - xh * s2)
    S = r.abs() * (gd.abs() + a1 + xh.abs() * a2)
    if dres is not None:
        dx, S = dx + dres.double(), S + dres.double().abs()
    return {"dx": dx, "S_dx": S, "dg": (d * xh).sum(0), "S_dg": (d * xh).abs().sum(0), "db": d.sum(0),
            "S_db": d.abs().sum(0)}


def ref_drop_bwd(dout, p=0.0, keep=None):
    """dh = dout keep / (1 - p) -> (ref [T, 512], column sums, column sums of |ref|)."""
    v = dout.double()
    if p > 0:
        v = v * keep.to(dout.device).double() * inv_keep(p)
    return v, v.sum(0), v.abs().sum(0)


# ---- head.hip --------------------------------------------------------------------------------------------------------
def ref_head(hb, W, bias, target):
    """From the stored operand hb [R, 512] bf16: dict z, dz [R, V]; ce, bound_ce [R]; G, bound_G [R, V]; pred [R] (the
    first fp64 maximum) and clear [R], the rows whose top1 - top2 exceeds twice the logit bound."""
    h, w, bd = hb.double(), W.double(), bias.double()
    R, V = h.shape[0], w.shape[0]
    z = h @ w.t() + bd
    Sz = h.abs() @ w.abs().t() + bd.abs()
    dz = U32 * z.abs() + slack(E + 1) * Sz
    t = target.long().view(R, 1)
    lse = torch.logsumexp(z, 1)
    zmax = z.amax(1)
    xmax = (zmax[:, None] - z).amax(1)
    dzm = dz.amax(1)
    ce = lse - z.gather(1, t)[:, 0]
    # lse: 1-Lipschitz in z (dzm), the exponentials, the V-term sum and the logarithm, the final addition
    e_lse = dzm + e_exp(xmax) + e_log(V) + U32 * (zmax.abs() + lse.abs())
    b_ce = U32 * ce.abs() + e_lse + dz.gather(1, t)[:, 0]
    sm = torch.exp(z - lse[:, None])
    onehot = torch.zeros_like(z).scatter_(1, t, 1.0)
    G = sm - onehot
    eps = torch.expm1(dzm + e_lse + U32 * (zmax.abs() + lse.abs() + xmax)) + e_exp(xmax + math.log(V))
    b_G = REL * G.abs() + (eps[:, None] + SLACK) * (sm + onehot)
    top2 = z.topk(2, 1).values
    return {"z": z, "dz": dz, "ce": ce, "bound_ce": b_ce, "G": G, "bound_G": b_G, "S_G": sm + onehot,
            "pred": (z == zmax[:, None]).to(torch.uint8).argmax(1), "clear": (top2[:, 0] - top2[:, 1]) > 2 * dzm}


# ---- assertions ------------------------------------------------------------------------------------------------------
_ratio = gm._ratio


def _where(flat, shape):
    return go.Bf16Check._index(flat, shape, 0)


def check_bf16(out, ref, hard, name, tight=None, S=None, bias=False, pre_var=None):
    """bf16 out against ref with assembled bounds: every element within hard (a bound of exactly 0 admits only an exact
    0), at most CAP of the elements outside tight, and, with bias and S, the mean signed ulp error of the elements with
    |ref| > BIAS_FLOOR S within the cap once there are BIAS_MIN_COUNT of them.  pre_var(w): the variance that the
    roundings before the store give the weighted sum of errors sum w (out - ref) (see `bias` in the module docstring).
    Returns the figures."""
    assert out.dtype == BF and ref.dtype == torch.float64 and out.shape == ref.shape == hard.shape, (name, out.shape)
    o = out.double()
    bad = ~torch.isfinite(o)
    if bad.any():
        raise AssertionError(f"{name}: non-finite output at {_where(bad.reshape(-1).to(torch.uint8).argmax().item(), out.shape)}")
    err = (o - ref).abs()
    st = {"worst": 0.0, "worst_hard": 0.0, "share": 0.0, "mean_ulp": 0.0, "count": 0, "elements": out.numel()}
    if out.numel() == 0:
        return st
    m, i = _ratio(err, hard).reshape(-1).max(0)
    st["worst_hard"] = m.item()
    if m.item() > 1.0:
        i = i.item()
        raise AssertionError(f"{name}: |out - ref| = {err.reshape(-1)[i].item():.6g} is {m.item():.3f} x the hard bound "
                             f"{hard.reshape(-1)[i].item():.6g} at {_where(i, out.shape)}: out "
                             f"{o.reshape(-1)[i].item()!r}, ref {ref.reshape(-1)[i].item()!r}")
    tight = hard if tight is None else tight
    st["worst"] = _ratio(err, tight).max().item()
    outside = int((err > tight).sum().item())
    st["share"] = outside / out.numel()
    if outside > CAP * out.numel():
        raise AssertionError(f"{name}: {outside} of {out.numel()} elements ({st['share']:.3g}) outside the tight bound "
                             f"(cap {CAP:.3g}); the worst is {st['worst']:.3f} x its bound")
    if S is not None:
        q = ref.abs() > go.BIAS_FLOOR * S
        w = torch.sign(ref) / go.bf16_ulp(ref) * q
        st["count"] = n = int(q.sum().item())
        st["mean_ulp"] = (w * (o - ref)).sum().item() / max(n, 1)
        cap = go.BIAS_CAP
        if pre_var is not None and n > 0:
            cap = max(cap, gm.BIAS_SIGMAS * math.sqrt(pre_var(w) + n / 12.0) / n)
        st["bias_cap"] = cap
        if bias and n >= go.BIAS_MIN_COUNT and cap <= gm.BIAS_CAP_MAX and abs(st["mean_ulp"]) > cap:
            raise AssertionError(f"{name}: mean signed error {st['mean_ulp']:+.4f} bf16 ulp over {n} elements "
                                 f"(cap {cap:.4g}): the stores are biased")
    return st


def check_f32(out, ref, bound, name):
    """fp32 out within an assembled bound; -inf must meet -inf, a bound of 0 an exact value."""
    assert out.dtype == torch.float32 and ref.dtype == torch.float64 and out.shape == ref.shape == bound.shape, \
        (name, out.dtype, out.shape, ref.shape)
    o = out.double()
    inf = torch.isinf(ref)
    if not torch.equal(o[inf], ref[inf]):
        raise AssertionError(f"{name}: an infinite reference value is not met exactly")
    o, r = torch.where(inf, torch.zeros_like(o), o), torch.where(inf, torch.zeros_like(ref), ref)
    bad = ~torch.isfinite(o)
    if bad.any():
        raise AssertionError(f"{name}: non-finite output at {_where(bad.reshape(-1).to(torch.uint8).argmax().item(), out.shape)}")
    err = (o - r).abs()
    st = {"worst": 0.0, "worst_hard": 0.0, "share": 0.0, "mean_ulp": 0.0, "count": 0, "elements": out.numel()}
    if out.numel() == 0:
        return st
    m, i = _ratio(err, bound).reshape(-1).max(0)
    st["worst"] = st["worst_hard"] = m.item()
    if m.item() > 1.0:
        i = i.item()
        raise AssertionError(f"{name}: |out - ref| = {err.reshape(-1)[i].item():.6g} is {m.item():.3f} x the fp32 bound "
                             f"{bound.reshape(-1)[i].item():.6g} at {_where(i, out.shape)}: out "
                             f"{o.reshape(-1)[i].item()!r}, ref {r.reshape(-1)[i].item()!r}")
    return st


def check_attn_fwd(out, lse, r, name):
    """The forward's out (hard, tight with its cap, bias, exact zeros) and lse against ref_attn_fwd's dict."""
    hard, tight, b_lse = bounds_attn_fwd(r)
    a = check_f32(lse.view_as(r["lse"]), r["lse"], b_lse, name + " lse")

    def pre_var(w):
        m = w.permute(0, 2, 1, 3) @ r["v"].transpose(-1, -2)           # [B, H, i, j] = sum_d w[i, d] v[j, d]
        return (REL * REL / 3.0 * (r["Pd"] * m) ** 2).sum().item()

    b = check_bf16(out, r["out"], hard, name + " out", tight, r["S_out"], bias=True, pre_var=pre_var)
    b["lse"] = a["worst"]
    return b


def check_attn_bwd(dqkv, r, name):
    """dQ, dK, dV against ref_attn_bwd's dict; returns the worst figures of the three."""
    st = None
    for t, n in enumerate(("dQ", "dK", "dV")):
        s = check_bf16(dqkv[:, :, t], r["ref"][:, :, t], r["hard"][:, :, t], f"{name} {n}", r["tight"][:, :, t],
                       r["hard"][:, :, t] / REL)       # hard / REL >= |ref| + sum|term|: the floor of the ulp figure
        st = merge(st, s)
    return st


def check_ln_fwd(y, mu, rs, r, name):
    a = check_f32(mu, r["mu"], r["bound_mu"], name + " mu")
    b = check_f32(rs, r["rs"], r["bound_rs"], name + " rs")
    c = check_bf16(y, r["y"], r["bound_y"], name + " y", None, r["S"])
    c["worst"] = c["worst_hard"] = max(a["worst"], b["worst"], c["worst"])
    return c


def check_ln_bwd(dx, dg, db, r, T, name, dxb=None, dsum=None):
    st = check_f32(dx, r["dx"], U32 * r["dx"].abs() + slack(E) * r["S_dx"], name + " dx")
    st = merge(st, gm.assert_f32(dg, r["dg"], r["S_dg"], T, name + " dg", extra=SLACK))
    st = merge(st, gm.assert_f32(db, r["db"], r["S_db"], T, name + " db"))
    if dxb is not None:
        assert torch.equal(dxb, dx.to(BF)), f"{name}: dxb is not the bf16 image of the stored dx"
        d = dx.double()
        st = merge(st, gm.assert_f32(dsum, d.sum(0), d.abs().sum(0), T, name + " dsum"))
    return st


def frob(out, ref):
    return go.frob(out, ref)


def merge(into, st):
    """Worst figures of several checks of one case."""
    if into is None:
        return dict(st)
    for k in ("worst", "worst_hard", "share"):
        into[k] = max(into[k], st.get(k, 0.0))
    if st["count"] > into["count"]:
        into["count"], into["mean_ulp"] = st["count"], st["mean_ulp"]
    into["elements"] += st["elements"]
    return into


class Table:
    """The -s output: one line per case and one summary per entry point."""

    def __init__(self, entry):
        self.entry, self.rows = entry, []

    def add(self, case, st):
        self.rows.append(st)
        print(f"\ndecoder oracle | {self.entry:13s} | {case:60s} | worst/hard {st['worst_hard']:6.3f} | worst/tight "
              f"{st['worst']:6.3f} | outside {st['share']:.2e} (cap {CAP:.2e}) | mean ulp {st['mean_ulp']:+.4f}"
              + (f" (cap {st['bias_cap']:.4f} over {st['count']})" if "bias_cap" in st else ""), end="")
        return st

    def summary(self):
        r = self.rows
        if not r:
            return
        big = [s for s in r if s["count"] >= go.BIAS_MIN_COUNT]
        ulp = max((abs(s["mean_ulp"]) for s in big), default=0.0)
        print(f"\ndecoder oracle | {self.entry:13s} | SUMMARY {len(r):4d} cases | worst/hard "
              f"{max(s['worst_hard'] for s in r):6.3f} | worst/tight {max(s['worst'] for s in r):6.3f} | outside "
              f"{max(s['share'] for s in r):.2e} (cap {CAP:.2e}) | |mean ulp| {ulp:.4f} over {len(big)} cases of >= "
              f"{go.BIAS_MIN_COUNT} elements")
