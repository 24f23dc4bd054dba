"""fp64 references and the element-wise oracle for the squeeze-excitation kernels (csrc/kernels/se.hip).

Plain torch, CPU or GPU tensors, no extension call.  pool [N, C] holds frame SUMS, w1 [S, C], b1 [S], w2 [C, S], b2 [C],
h [N, S], gate [N, C], red [5, N, C], all fp32.  Every stage that reaches memory is checked against the fp64 function of
that stage's inputs AS STORED (h feeds gate, gate and h feed dh, dh feeds rb / dw1 / db1, rb feeds sdz / sdzx), so the
errors do not compound.  Every reference returns fp64 values with, next to each, S: the same expression over absolute
values (glue_oracle's convention).  inv_hw is taken as its fp32 image, the value the kernels multiply by.

What the kernels round and where, read from se.hip and cited by line:
  * se_rowdot_kernel: `acc[0][0] = fmaf(x0.w, w0.w, fmaf(x0.z, w0.z, ...))`: an fma chain over the channels of one K
    slice, one rounding per term, then one partial per slice (`pp[(int64_t)n * S + j] = acc[a][b]`).  Zero padding of
    the frame, unit and K tails happens at load (`if (n < N && c < ke) ... else 0`): a tail adds exact zeros.
    BWD forms dz while staging (`v.x *= g.x * (1.f - g.x)`): 3 roundings per operand, DZ_EPS = 3 U32.
  * se_rowmat_kernel: `sum[u] += part[k * NS_ + o[u]]` in slice order, then
      fwd  `hv = sum[u] * inv_hw + b1[j]`, stored by channel tile 0 (`if (blockIdx.y == 0) yout[o] = hv`):
           h is an fp32 sum of C terms + the slices + 2 operations: the f32 bound with n = C + slices + 2.
           `y = silu(hv)` = hv * rcp(1 + __expf(-hv)) (common.h sigmoidf_): v_exp_f32 of the scaled argument,
           2^-23 (1 + |x|) relative (decoder_oracle.e_exp), the addition, a 1-ulp rcp and the product:
               eps_silu(x) = 2^-23 (3 + |x|)   relative.
           `acc[a][b] = fmaf(y, vv[b], acc[a][b])` over S units, `sigmoidf_(acc + b2[c + b])`: the argument a of the
           sigmoid is off by da = max(SLACK, (S + 2) U32 + eps_silu(max|h|)) S_a, S_a = |silu(h)| |w2|^T + |b2| (this
           is slack(S + 2) S_a while (S + 2 + 2 (3 + max|h|)) U32 <= SLACK, i.e. for every |h| < 60), the sigmoid is
           1/4-Lipschitz, and its own evaluation adds  e_sig = gate (2^-23 (1 + |a|)(1 - gate) + 4 U32):
               |gate - ref| <= da / 4 + e_sig.
      bwd  `y = sum[u] * (sg * (1.f + x * (1.f - sg)))`, stored by channel tile 0: dh.  The factor silu'(x) carries the
           error of sg (E1 = 2^-23 (1 + |x|) + 3 U32) through 1 - sg, the product by x, the addition and the product by
           sg: absolutely <= sg (E1 + 2 U32)(1 + 2 |x|) =: e_sp(x).  So
               |dh - ref| <= U32 |ref| + (slack(C + slices + 2) + DZ_EPS) Sz silu'_abs(h) + Sz e_sp(h),
           Sz = |dz| |w2| and silu'_abs = sg (1 + |x| (1 - sg)).
           `r[b] = acc * inv_hw`: rb is an exact-operand product of the STORED dh over S units: f32, n = S + 1.
  * se_wsum_part_kernel: `a2[a][0] = fmaf(zz[a], hv.x, a2[a][0])`, `a1[a][0] = fmaf(dv.x, pp[a], a1[a][0])` over the
    frames of one slice; z = d * g * (1 - g) (DZ_EPS) and hv = x * sigmoidf_(x) (eps_silu) are formed while staging,
    dv = dh and pp = pool are stored operands.  `cz[a] += (double)zz[a]`, `c1[a] += (double)(gg[a] * v1[a] + rv[a] *
    v2[a])`, `jd[0] += (double)dv.x`: fp64 sums of fp32 terms.
  * se_wsum_fin_kernel: `a += pw2[k * CS + i]` in slice order, `dw1[o] = a * inv_hw`, `db2[c] = (float)z`,
    `mdz[c] = (float)(x / count)`.  dw2 / dw1 are f32 sums with n = N + slices (+ 1 for inv_hw); dw2's terms carry
    extra = DZ_EPS + eps_silu(max|h|).  db2, sdz, sdzx: U32 |ref| on the cast + SLACK per term (their terms are
    evaluated in fp32: 3 roundings); db1 sums stored values: U32 |ref| + 2^-40 sum|dh|.  mdz, mdzx: the same / count.
  * fallback kernels: se_bwd_dz_kernel `d = dsum[i] * g * (1.f - g)` (4 U32 |ref|), se_bwd_dh_kernel `d = dzf2[i] * (sg
    * (1.f + x * (1.f - sg)))` (U32 |ref| + |dzf2| e_sp), se_bwd_bnsum_kernel `r = rbraw[i] * inv_hw` (U32 |ref|);
    their column sums are fp64 sums of the stored values (`acc[0] += (double)d`) in a fixed order.

Nothing here is fitted to a kernel's output: the constants are glue_oracle's REL / SLACK, gemm_oracle's U32 and
slack(n), and the reduction lengths of plan(), which re-derives rd_splits, launch_rowmat and ws_splits.
"""
import torch

import decoder_oracle as do
import gemm_oracle as gm
import glue_oracle as go

U32, SLACK, slack = gm.U32, go.SLACK, gm.slack
DZ_EPS = 3 * U32

# se.hip's tile constants
RD_FT, RD_JT, RD_KC, RD_TARGET_WG = 32, 32, 64, 512
RM_CT, WIDE_FWD, WIDE_BWD = 128, 200, 300
WS_CT, WS_JT, WS_FC, WS_NS, WS_NS_MAX, WS_TARGET_WG = 64, 32, 32, 8, 32, 512
SE_BLOCK, FIN_GRID_MAX = 256, 1024
S_MAX, LDS_DEFAULT = 128, 64 * 1024
SE_NARROW_MAX = 4096


def _cd(a, b):
    return (a + b - 1) // b


def plan(N, C, S):
    """The launch plan of se_fwd / se_bwd for a shape, re-derived from rd_splits, launch_rowmat and ws_splits; the order
    of `as_list` is rt1_se_plan's."""
    base = _cd(N, RD_FT) * _cd(S, RD_JT)
    ks = min(max(_cd(RD_TARGET_WG, base), 1), _cd(C, RD_KC))
    kslice = _cd(_cd(C, ks), RD_KC) * RD_KC
    p = {"slices": _cd(C, kslice), "kslice": kslice}
    tiles32 = _cd(N, 32) * _cd(C, RM_CT)
    p["ft_fwd"] = 32 if tiles32 >= WIDE_FWD else 16
    p["ft_bwd"] = 32 if tiles32 >= WIDE_BWD else 16
    p["lds_fwd"] = (p["ft_fwd"] * S + RM_CT * (S | 1)) * 4
    p["lds_bwd"] = (p["ft_bwd"] * S + RM_CT * S) * 4
    wb = _cd(C, WS_CT) * _cd(S, WS_JT)
    ns = min(max(_cd(WS_TARGET_WG, wb), WS_NS), WS_NS_MAX)
    ns = min(ns, max(N, 1))
    p["nslice"] = _cd(N, ns)
    p["fslices"] = _cd(N, p["nslice"])
    total = 2 * C * S + C + S
    p["fin_grid"] = min(FIN_GRID_MAX, _cd(total, SE_BLOCK))
    p["fin_trips"] = _cd(total, p["fin_grid"] * SE_BLOCK)
    p["raise_lds"] = int(p["lds_fwd"] > LDS_DEFAULT or p["lds_bwd"] > LDS_DEFAULT)
    p["k_tail"] = C % RD_KC != 0
    p["as_list"] = [p["slices"], kslice, p["ft_fwd"], p["ft_bwd"], p["lds_fwd"], p["lds_bwd"], p["fslices"],
                    p["nslice"], p["fin_grid"], p["raise_lds"]]
    return p


def f32(x):
    return torch.tensor(float(x), dtype=torch.float32).double().item()


def eps_silu(hmax):
    return 2.0 ** -23 * (3.0 + hmax)


def _sp(x):
    """silu'(x), the same with its addends absolute, and e_sp(x) (see the docstring), fp64."""
    sg = torch.sigmoid(x)
    e1 = 2.0 ** -23 * (1 + x.abs()) + 3 * U32
    return sg * (1 + x * (1 - sg)), sg * (1 + x.abs() * (1 - sg)), sg * (e1 + 2 * U32) * (1 + 2 * x.abs())


def _hmax(h):
    return h.abs().max().item() if h.numel() else 0.0


# ---- references ------------------------------------------------------------------------------------------------------
def ref_h(pool, inv_hw, w1, b1):
    """h = (pool w1^T) inv_hw + b1 -> (ref, S)."""
    p, w, b, r = pool.double(), w1.double(), b1.double(), f32(inv_hw)
    return (p @ w.t()) * r + b, (p.abs() @ w.abs().t()) * r + b.abs()


def ref_gate(h, w2, b2):
    """gate = sigmoid(silu(h) w2^T + b2) from the STORED h -> (ref, bound)."""
    S = h.shape[1]
    x, w, b = h.double(), w2.double(), b2.double()
    y = x * torch.sigmoid(x)
    a, Sa = y @ w.t() + b, y.abs() @ w.abs().t() + b.abs()
    g = torch.sigmoid(a)
    da = max(SLACK, (S + 2) * U32 + eps_silu(_hmax(h))) * Sa
    return g, 0.25 * da + g * (2.0 ** -23 * (1 + a.abs()) * (1 - g) + 4 * U32)


def ref_dz(dsum, gate):
    g = gate.double()
    return dsum.double() * g * (1 - g)


def ref_dh(dsum, gate, h, w2, slices):
    """dh = ((dsum g (1 - g)) w2) silu'(h) from the STORED gate and h -> (ref, bound)."""
    C = gate.shape[1]
    dz, w, x = ref_dz(dsum, gate), w2.double(), h.double()
    sp, spa, esp = _sp(x)
    zw, Sz = dz @ w, dz.abs() @ w.abs()
    ref = zw * sp
    return ref, U32 * ref.abs() + (slack(C + slices + 2) + DZ_EPS) * Sz * spa + Sz * esp


def ref_rb(dh, w1, inv_hw):
    """rb = (dh w1) inv_hw from the STORED dh -> (ref, S)."""
    d, w, r = dh.double(), w1.double(), f32(inv_hw)
    return (d @ w) * r, (d.abs() @ w.abs()) * r


def ref_wsums(red, gate, h, dh, pool, rb, inv_hw, count):
    """The frame sums from the STORED gate, h, dh and rb: dict name -> (ref, sum|term|)."""
    r, g, x = red.double(), gate.double(), h.double()
    dz = r[0] * g * (1 - g)
    hs = x * torch.sigmoid(x)
    d, p, b, ih = dh.double(), pool.double(), rb.double(), f32(inv_hw)
    t1, a1 = g * r[1] + b * r[2], (g * r[1]).abs() + (b * r[2]).abs()
    t2, a2 = g * r[3] + b * r[4], (g * r[3]).abs() + (b * r[4]).abs()
    return {"dw2": (dz.t() @ hs, dz.abs().t() @ hs.abs()),
            "dw1": ((d.t() @ p) * ih, (d.abs().t() @ p.abs()) * ih),
            "db2": (dz.sum(0), dz.abs().sum(0)), "db1": (d.sum(0), d.abs().sum(0)),
            "sdz": (t1.sum(0), a1.sum(0)), "sdzx": (t2.sum(0), a2.sum(0)),
            "mdz": (t1.sum(0) / count, a1.sum(0) / count), "mdzx": (t2.sum(0) / count, a2.sum(0) / count)}


# ---- checks ----------------------------------------------------------------------------------------------------------
def check_fwd(pool, inv_hw, w1, b1, w2, b2, h, gate, name):
    """se_fwd's h and gate, stage by stage; returns the worst figures."""
    N, C = pool.shape
    p = plan(N, C, h.shape[1])
    r, Sh = ref_h(pool, inv_hw, w1, b1)
    st = gm.assert_f32(h, r, Sh, C + p["slices"] + 2, name + " h")
    g, bound = ref_gate(h, w2, b2)
    return do.merge(st, do.check_f32(gate, g, bound, name + " gate"))


def check_frame(dsum, gate, h, w1, w2, inv_hw, dh, rb, name):
    """se_bwd_frame's dh and rb."""
    N, C = gate.shape
    S = h.shape[1]
    r, bound = ref_dh(dsum, gate, h, w2, plan(N, C, S)["slices"])
    st = do.check_f32(dh, r, bound, name + " dh")
    r, Sr = ref_rb(dh, w1, inv_hw)
    return do.merge(st, gm.assert_f32(rb, r, Sr, S + 1, name + " rb"))


def _sum_bound(ref, sab, rel):
    return U32 * ref.abs() + rel * sab


def check_wsum(red, gate, h, dh, pool, rb, inv_hw, count, outs, name):
    """The eight frame sums of se_bwd (outs: dict name -> tensor) against the stored operands."""
    N, C = gate.shape
    S = h.shape[1]
    n = N + plan(N, C, S)["fslices"]
    r = ref_wsums(red, gate, h, dh, pool, rb, inv_hw, count)
    st = gm.assert_f32(outs["dw2"], *r["dw2"], n, name + " dw2", extra=DZ_EPS + eps_silu(_hmax(h)))
    s1 = gm.assert_f32(outs["dw1"], *r["dw1"], n + 1, name + " dw1")
    st = do.merge(st, s1)
    st["sum"] = max(st["sum"], s1["sum"])      # the Table's `sum` column: the worst of the two weight sums alone
    for k in ("db2", "sdz", "sdzx", "mdz", "mdzx"):
        st = do.merge(st, do.check_f32(outs[k], r[k][0], _sum_bound(*r[k], SLACK), f"{name} {k}"))
    return do.merge(st, do.check_f32(outs["db1"], r["db1"][0], _sum_bound(*r["db1"], 2.0 ** -40), name + " db1"))


def check_fallback_dz(dsum, gate, dz, db, name):
    r = ref_dz(dsum, gate)
    st = do.check_f32(dz, r, 4 * U32 * r.abs(), name + " dz")
    d = dz.double()
    return do.merge(st, do.check_f32(db, d.sum(0), _sum_bound(d.sum(0), d.abs().sum(0), 2.0 ** -40), name + " db"))


def check_fallback_dh(dzf2, h, dh, db, name):
    z = dzf2.double()
    sp, _, esp = _sp(h.double())
    r = z * sp
    st = do.check_f32(dh, r, U32 * r.abs() + z.abs() * esp, name + " dh")
    d = dh.double()
    return do.merge(st, do.check_f32(db, d.sum(0), _sum_bound(d.sum(0), d.abs().sum(0), 2.0 ** -40), name + " db"))


def check_fallback_bnsum(red, gate, rbraw, inv_hw, count, rb, sdz, sdzx, mdz, mdzx, name):
    r0 = rbraw.double() * f32(inv_hw)
    st = do.check_f32(rb, r0, U32 * r0.abs(), name + " rb")
    r, g, b = red.double(), gate.double(), rb.double()
    for o, i, div in ((sdz, 1, 1.0), (sdzx, 3, 1.0), (mdz, 1, count), (mdzx, 3, count)):
        t = (g * r[i] + b * r[i + 1]).sum(0) / div
        a = ((g * r[i]).abs() + (b * r[i + 1]).abs()).sum(0) / div
        st = do.merge(st, do.check_f32(o, t, _sum_bound(t, a, SLACK), name + " sums"))
    return st


BWD_NAMES = ("dw2", "db2", "dw1", "db1", "rb", "sdz", "sdzx", "mdz", "mdzx")      # se_bwd's return order
