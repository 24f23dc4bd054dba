"""fp64 references and the element-wise oracle for the TokenLearner kernels (csrc/kernels/tokenlearner.hip).

Plain torch, CPU or GPU tensors, no extension call.  x [N, P, 512] bf16, gamma / beta [512], W1 [64, 512] bf16, b1 [64],
W2 [8, 64], b2 [8] fp32; tl_fwd returns out [N, 8, 512] bf16, mu / rs [N, P], z1 [N, P, 64] bf16, s [N, 8, P]; tl_bwd
takes dO [N, 8, 512] bf16 and returns dx, dz1, xn (bf16), pw2 [N, 8, 65] (dW2 | db2) and pg [N, 2, 512] (dgamma, dbeta).
Every stage is checked against the fp64 function of its inputs AS STORED (mu / rs feed z1, z1 feeds s, s feeds out; the
backward starts from the stored s, z1, mu, rs and dx from the stored dz1).  Every reference returns fp64 values with,
next to each, S: the same expression over absolute values.

What the kernels round and where, read from tokenlearner.hip and cited by line:
  forward (tl_fwd_kernel)
  * `s += v[j]` (8 additions), wave_sum (6 more), `* (1.f / C)` exact: mu is off by dmu = U32 |mu| + slack(512) mean|x|.
    `q += (v[j] - m) * (v[j] - m)`: centred around the kernel's m, which adds (m - mu)^2 <= dmu^2; `rsqrtf(var + eps)`
    (v_rsq_f32, 1 ulp): decoder_oracle's  e_rs = slack(512) + 2^-22 + dmu^2 / (var + eps),  |rs - ref| <= e_rs ref:
    a few U32 plus half the relative error of var + eps.
  * `v[j] = (v[j] - m) * r * gam[c0 + j] + bet[c0 + j]; ab[j] = f2bf(v[j])`: the MFMA operand is rebuilt in fp32 (4
    roundings) from the STORED mu / rs and rounded to bf16; `acc[nt] = ...mfma_f32_16x16x32_bf16(a, b, acc[nt], ...)`
    over 16 chunks, `zb = f2bf(acc[nt][i] + bj)`: gemm_oracle's rebuilt-operand scheme, `hard` with K = 512 + 1 and its
    caps with fanout 64 (one operand feeds the 64 outputs of its row) and Kop = 512.
  * `Hs[p][j] = gelu_tanh(bf2f(zb))` from the stored z1; `s = fmaf(Hs[p][j], w[j], s)` from b2 over 64 units.
    gelu_tanh = 0.5 z (1 + tanhf(u)): tanhf within 2 ulp of a value <= 1 (2^-22) plus the error of u through
    tanh' (< 2^-23): d(1 + th) <= 2^-21 + 2 U32, so gelu is off by at most  e_gelu(z) = 2^-21 |z|  absolutely, and a
    logit by  da = U32 |a| + slack(65) Sa + sum_j e_gelu(z1[p, j]) |W2[t, j]|.
  * `e = __expf(Sl[t][p] - m); s += e` per lane, wave_sum, `inv = 1.f / wave_sum(s)`, `v = Sl[t][p] * inv`: relative
        eps_s[t] = expm1(2 max_p da) + 2 e_exp(spread) + (P + 8) U32
    (decoder_oracle's eps_p: the shift of every logit by <= da moves numerator and denominator by e^(+-da); e_exp(x) =
    2^-23 (1 + |x|) for v_exp_f32 with the scaled argument; P additions, the division, the product).  The caller keeps
    the logit spread <= 30.
  * `acc0[t] = fmaf(Sl[t][p], x0, acc0[t])` over p, `pack2(acc0[t], acc1[t])`: out = bf16 of an fp32 sum of P terms of
    the STORED s: gemm_oracle's tight bound with n = P.
  backward (tl_bwd_kernel<128> for P <= 128, <256> above)
  * `acc = ...mfma...(av, bv, acc, 0, 0, 0)` over 16 chunks: dS = dO . x in fp32, e_dS = slack(512) |dO| . |x|.
    `d = fmaf(Ss[t][p], dSs[t][p], d)`, wave_sum, `dSs[t][p] = Ss[t][p] * (dSs[t][p] - d)`: the softmax backward
    cancels, so its magnitude is A = s (|dS| + sum_p s |dS|) and
        e_da = s (e_dS + sum_p s e_dS) + (slack(P) + 3 U32) A.
  * `dh = fmaf(ds, w2[t], dh)` over 8 tokens, `d = f2bf(dh * gd)` with gd = gelu'(z1) from the same tanh: with
    d(th) <= 2^-21, Q(z) = 0.5 |z| k0 (1 + 3 k1 z^2):  e_gd = 2^-22 + 2^-19 Q + 4 U32 gd_abs,  gd_abs = 0.5 (1 + th) +
    Q (1 - th^2).  dz1:  REL |ref| + (E + slack(10) SA) gd_abs + SA e_gd,  SA = A^T |W2|, E = e_da^T |W2|.
  * `aw[t] = fmaf(ds, hz, aw[t])` over the positions of a group, 4 groups combined; `s += dSs[tid][p]`: pw2 = (dW2 |
    db2) are sums over P of da: sum_p e_da |h| + A e_gelu + slack(P + 4) sum_p A |h| (db2: h = 1).  db2 is
    mathematically zero; it is held to this S-relative bound like every other sum.
  * `xnv[i] = xh * gv[i] + bv[i]`, `xh = (xv[i] - m) * r` from the stored mu / rs, pack2: glue_oracle's bf16 bound.
  * dxn_half: `acc[ct] = ...mfma...(b, a, acc[ct], 0, 0, 0)` over H1 / 32 = 2 chunks from the STORED dz1 (Dz holds the
    same bf16 values that went to dz1_o): d = dz1 W1, exact products, 64 additions.  `g = acc[ct][i] * gv[i]; sg += g;
    sgx = fmaf(g, xh, sgx)` over 128 columns per lane and two shuffles, `* (1.f / C)`;  `pool[0] = fmaf(st[t], d4.x,
    pool[0])` over 8 tokens; `dxv[i] = r * (d * gv[i] - sg - xh * sgx) + pool[i]`, pack2.  Every addend's error is at
    most its reduction length in U32 relative to the addend taken absolute, 64 + 512 + 8 + 8 in all:
        |dx - ref| <= REL |ref| + slack(592) S,  S = r (D |gamma| + mean_c(D |gamma|) + |xh| mean_c(D |gamma| |xh|))
                                                     + sum_t s |dO|,   D = |dz1| |W1|.
  * `dgs[i] = d * xh; dbs[i] = d`, 4 shuffle additions over the 16 rows, `red[wave][0][c + i] += dgs[i]` over the
    wave's row blocks, 4 waves: pg = f32 sums over P of K = 64 products, n = P + 64 + 8, dgamma with extra = SLACK
    for xh.  Rows >= P of the last block are zeroed (`d = ok ? acc[ct][i] : 0.f`).
"""
import math

import torch

import decoder_oracle as do
import gemm_oracle as gm
import glue_oracle as go

BF = torch.bfloat16
REL, SLACK, U32, slack = go.REL, go.SLACK, gm.U32, gm.slack
C, H1, T, PMAX = 512, 64, 8, 256
K0, K1 = 0.7978845608028654, 0.044715
SPREAD_MAX = 30.0


def bwd_template(P):
    """PM of tl_bwd_kernel<PM> that rt1_tl_bwd launches."""
    return 128 if P <= 128 else 256


def _gelu(z):
    """gelu_tanh(z), gelu'(z), gd_abs and Q(z) in fp64."""
    th = torch.tanh(K0 * (z + K1 * z ** 3))
    q = 0.5 * z.abs() * K0 * (1 + 3 * K1 * z * z)
    gd = 0.5 * (1 + th) + 0.5 * z * (1 - th * th) * K0 * (1 + 3 * K1 * z * z)
    return 0.5 * z * (1 + th), gd, 0.5 * (1 + th) + q * (1 - th * th), q


# ---- forward ---------------------------------------------------------------------------------------------------------
def ref_stats(x, eps):
    """mu, rs [N, P] with their bounds (decoder_oracle.ref_ln_fwd's formulas)."""
    xd = x.double()
    mu = xd.mean(-1)
    var = ((xd - mu[..., None]) ** 2).mean(-1)
    rs = 1.0 / torch.sqrt(var + eps)
    dmu = U32 * mu.abs() + slack(C) * xd.abs().mean(-1)
    return mu, dmu, rs, (slack(C) + 2.0 ** -22 + dmu * dmu / (var + eps)) * rs


def operand_ln(x, mu, rs, gamma, beta):
    """The LN operand from the STORED mu / rs: (bf16-rounded fp64, unrounded fp64, S)."""
    xh = (x.double() - mu.double()[..., None]) * rs.double()[..., None]
    v = xh * gamma.double() + beta.double()
    return gm.bf16_round(v), v, xh.abs() * gamma.double().abs() + beta.double().abs()


def ref_logits(z1, W2, b2):
    """a [N, P, 8] from the STORED z1 with its bound da."""
    z, w, b = z1.double(), W2.double(), b2.double()
    h = _gelu(z)[0]
    a, Sa = h @ w.t() + b, h.abs() @ w.abs().t() + b.abs()
    return a, U32 * a.abs() + slack(H1 + 1) * Sa + (2.0 ** -21 * z.abs()) @ w.abs().t()


def ref_softmax(z1, W2, b2):
    """s [N, 8, P] from the STORED z1 with its bound; also the logit spread (the caller keeps it <= SPREAD_MAX)."""
    a, da = ref_logits(z1, W2, b2)
    P = a.shape[1]
    s = torch.softmax(a, 1)
    spread = (a.amax(1) - a.amin(1)).max().item()
    eps = torch.expm1(2 * da.amax(1)) + 2 * do.e_exp(spread) + (P + 8) * U32           # [N, 8]
    return s.transpose(1, 2), (eps[:, None, :] * s).transpose(1, 2), spread


def ref_pool(s, x):
    """out [N, 8, 512] = s x from the STORED s -> (ref, S)."""
    return s.double() @ x.double(), s.double().abs() @ x.double().abs()


def check_fwd(x, gamma, beta, eps, W1, b1, W2, b2, outs, name):
    """tl_fwd's five outputs, stage by stage; returns the worst figures (gemm_oracle's keys)."""
    out, mu, rs, z1, s = outs
    N, P, _ = x.shape
    m, dm, r, dr = ref_stats(x, eps)
    st = do.check_f32(mu, m, dm, name + " mu")
    st = do.merge(st, do.check_f32(rs, r, dr, name + " rs"))
    aq, _, _ = operand_ln(x, mu, rs, gamma, beta)
    ref, S, Tm = gm.ref_gemm(aq.reshape(N * P, C), W1, bias=b1, want_T=True)
    zs = gm.assert_gemm(z1.reshape(N * P, H1), ref, S, C + 1, name + " z1", T=Tm, kop=C)
    st["z1_tight"], st["z1_share"] = zs["worst"], zs["share"]
    sr, sb, spread = ref_softmax(z1, W2, b2)
    assert spread <= SPREAD_MAX, f"{name}: logit spread {spread:.1f} > {SPREAD_MAX}: choose other inputs"
    st["sum"] = st["worst"]                    # the Table's `sum` column: the worst of the fp32 stages (mu, rs, s) alone
    st = do.merge(st, {**zs, "worst": zs["worst_hard"]})
    ss = do.check_f32(s, sr, sb, name + " s")
    st["sum"] = max(st["sum"], ss["worst"])
    st = do.merge(st, ss)
    ref, S = ref_pool(s, x)
    st = do.merge(st, gm.assert_gemm(out.reshape(N * T, C), ref.reshape(N * T, C), S.reshape(N * T, C), P,
                                     name + " out"))
    return st


# ---- backward --------------------------------------------------------------------------------------------------------
def ref_bwd_head(x, dO, s, z1, W2):
    """From the STORED s and z1: dict of da [N, 8, P] with A, e_da; dz1 [N, P, 64] with its bound; pw2 [N, 8, 65] with
    its bound."""
    xd, g, sd, z, w = x.double(), dO.double(), s.double(), z1.double(), W2.double()
    P = xd.shape[1]
    dS, SdS = g @ xd.transpose(1, 2), g.abs() @ xd.abs().transpose(1, 2)          # [N, 8, P]
    e_dS = slack(C) * SdS
    dot = (sd * dS).sum(-1, keepdim=True)
    da = sd * (dS - dot)
    A = sd * (dS.abs() + (sd * dS.abs()).sum(-1, keepdim=True))
    e_da = sd * (e_dS + (sd * e_dS).sum(-1, keepdim=True)) + (slack(P) + 3 * U32) * A
    h, gd, gda, q = _gelu(z)
    dh = da.transpose(1, 2) @ w                                                   # [N, P, 64]
    SA, E = A.transpose(1, 2) @ w.abs(), e_da.transpose(1, 2) @ w.abs()
    dz = dh * gd
    e_gd = 2.0 ** -22 + 2.0 ** -19 * q + 4 * U32 * gda
    b_dz = REL * dz.abs() + (E + slack(T + 2) * SA) * gda + SA * e_gd
    h1 = torch.cat([h, torch.ones_like(h[..., :1])], -1)                          # db2: h = 1
    eh = torch.cat([2.0 ** -21 * z.abs(), torch.zeros_like(h[..., :1])], -1)
    pw2 = da @ h1
    b_pw = U32 * pw2.abs() + e_da @ h1.abs() + A @ eh + slack(P + 4) * (A @ h1.abs())
    return {"da": da, "A": A, "dz1": dz, "b_dz1": b_dz, "S_dz1": SA * gda, "pw2": pw2, "b_pw2": b_pw}


def ref_bwd_tail(x, dO, s, dz1, mu, rs, gamma, beta, W1):
    """From the STORED dz1, s, mu, rs: dict xn / S_xn, dx / S_dx [N, P, 512], pg / S_pg [N, 2, 512]."""
    xd, g, sd, gm_, bt = x.double(), dO.double(), s.double(), gamma.double(), beta.double()
    r = rs.double()[..., None]
    xh = (xd - mu.double()[..., None]) * r
    d, D = dz1.double() @ W1.double(), dz1.double().abs() @ W1.double().abs()    # [N, P, 512]
    gg, G = d * gm_, D * gm_.abs()
    sg, sgx = gg.mean(-1, keepdim=True), (gg * xh).mean(-1, keepdim=True)
    pool, Sp = sd.transpose(1, 2) @ g, sd.transpose(1, 2).abs() @ g.abs()
    dx = r * (gg - sg - xh * sgx) + pool
    S = r * (G + G.mean(-1, keepdim=True) + xh.abs() * (G * xh.abs()).mean(-1, keepdim=True)) + Sp
    return {"xn": xh * gm_ + bt, "S_xn": xh.abs() * gm_.abs() + bt.abs(), "dx": dx, "S_dx": S,
            "pg": torch.stack([(d * xh).sum(1), d.sum(1)], 1), "S_pg": torch.stack([(D * xh.abs()).sum(1), D.sum(1)], 1)}


def bound_dx(r):
    return REL * r["dx"].abs() + slack(H1 + C + 2 * T) * r["S_dx"]


def check_bwd(x, dO, s, z1, mu, rs, gamma, beta, W1, W2, outs, name):
    """tl_bwd's five outputs from the stored forward tensors; W1 is [64, 512] (the kernel takes its transpose)."""
    dx, dz1, xn, pw2, pg = outs
    N, P, _ = x.shape
    hd = ref_bwd_head(x, dO, s, z1, W2)
    st = do.check_bf16(dz1.reshape(N, P, H1), hd["dz1"], hd["b_dz1"], name + " dz1", S=hd["S_dz1"])
    sp = do.check_f32(pw2, hd["pw2"], hd["b_pw2"], name + " pw2")
    st = do.merge(st, sp)
    t = ref_bwd_tail(x, dO, s, dz1.reshape(N, P, H1), mu, rs, gamma, beta, W1)
    a = go.assert_bf16_exact(xn.reshape(N, P, C), t["xn"], t["S_xn"], name + " xn")
    st = do.merge(st, {"worst": a["worst"], "worst_hard": a["worst"], "share": 0.0, "count": a["count"],
                       "mean_ulp": a["mean_ulp"], "elements": a["elements"]})
    st = do.merge(st, do.check_bf16(dx, t["dx"], bound_dx(t), name + " dx", S=t["S_dx"], bias=True))
    sg = gm.assert_f32(pg[:, 0], t["pg"][:, 0], t["S_pg"][:, 0], P + H1 + 8, name + " dgamma", extra=SLACK)
    sb = gm.assert_f32(pg[:, 1], t["pg"][:, 1], t["S_pg"][:, 1], P + H1 + 8, name + " dbeta")
    st = do.merge(do.merge(st, sg), sb)
    st["sum"] = max(sp["worst"], sg["worst"], sb["worst"])      # `sum` column: the worst of the fp32 sums (pw2, pg) alone
    return st


# ---- inputs ----------------------------------------------------------------------------------------------------------
def make_inputs(N, P, gen, device="cpu", kind="normal"):
    """Rows with different means and scales (the LayerNorm matters), gamma in [0.5, 1.5]; kind: `normal`, `onehot` (W2
    large: a near-one-hot softmax, spread kept under 30) or `flat` (W2 tiny: a nearly flat one)."""
    r = lambda *s: torch.randn(*s, generator=gen)
    u = lambda *s: torch.rand(*s, generator=gen)
    x = (r(N, P, C) * (0.5 + 2.0 * u(N, P, 1)) + 1.5 * r(N, P, 1)).to(BF)
    w2s = {"normal": 0.5, "onehot": 5.0, "flat": 1e-3}[kind]
    d = {"x": x, "gamma": 0.5 + u(C), "beta": r(C) * 0.1, "eps": 1e-6, "W1": (r(H1, C) * C ** -0.5).to(BF),
         "b1": r(H1) * 0.1, "W2": r(T, H1) * w2s * H1 ** -0.5, "b2": r(T) * 0.1, "dO": r(N, T, C).to(BF)}
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in d.items()}
