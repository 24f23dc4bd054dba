"""fp64 references and the element-wise oracle for the MFMA product kernels (csrc/kernels/pwgemm.hip, pwtall.hip,
gemm.hip, gemm256.hip, wgrad.hip, pwbwd.hip, projbwd.hip).

Plain torch, CPU or GPU tensors, no extension call.  Activations are [M, K] bf16 (M = frames x pixels), weights [N, K]
bf16 (NT) or [K, N] (NN), per-channel vectors fp32, per-frame rows [M / hw, C] fp32.  Every reference returns (ref, S)
in fp64 with S the same expression over absolute values (glue_oracle's convention: the magnitude that the fp32
roundings are relative to); the weight-gradient reference also returns T, the largest single |term| of each output.

What the kernels round and where, read from the .hip files and cited by function:
  * Products.  Every kernel multiplies bf16 operands exactly inside v_mfma_f32_16x16x32_bf16 and adds in fp32
    (pw_gemm_kernel / pw_wide_kernel: `acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf, af[r][kc], ...)`;
    pw_tall_kernel, gemm.hip and gemm256.hip the same over 32-wide K chunks; wgrad_kernel over 64-row chunks of M).
    Zero padding of K / N / M tails happens at load time (load_a: `if (row < M && col < K) ... else 0`), so a tail
    adds exact zeros.
  * One store.  The fp32 accumulator is rounded to bf16 once (pw_gemm_kernel: `u.x = pack2(acc[r][nt][0], ...)`,
    pw_tall_kernel: `o.x = pack2(acc[r][t][0], acc[r][t][1])`).  bias, the second segment and res * rmul are added in
    fp32 BEFORE that rounding (pw_tall_kernel TAIL: `acc += b`, `acc = fmaf(res, f, acc)`): S carries them as addends.
    out_f32, the embed epilogue (pw_tall_kernel EPI 1: `o.x = acc + b.x + q.x`) and every weight gradient store fp32.
  * Statistics describe the STORED tensor: pw_gemm_kernel STATS reads the bf16 strip image back from LDS
    (`load8(cl + row * LDC + sc8 * 8, v)`) and sums v and v * v per workgroup; gemm.hip / gemm256.hip sum the packed
    values of their M tile.  ref_stats therefore takes the kernel's own stored C.  A workgroup of pw_gemm owns the
    strips s with (s / 4) % grid == blockIdx.x, one strip = 16 R rows (PwShape::R): pw_tile_index.
  * Prologue operands are bf16.  pw_gemm_kernel PRO (`x[j] = silu(fmaf(x[j], sc[j], sh[j])) * gv[j]` then pack2),
    pw_tall_kernel's prologue lambda and gemm.hip's operand load rebuild a = silu(y * scale + shift) * gate[frame] with
    bn_apply's formula and round it before the MFMA; pw_gemm_kernel BNB builds dy3 = k1 * (dout * (fmul * keep)) +
    k2 * y3 + k0 (`o[j] = fmaf(k1[j], g[j], fmaf(k2[j], yv[j], k0[j]))`) and stores it.  Where the kernel can store
    the operand (store_operand / store_a / dy3) the test checks the stored operand element-wise against
    glue_oracle.ref_bn_apply / ref_bn_bwd_apply and holds the product to `tight` against the fp64 product of that
    STORED operand.  wgrad_kernel's stage lambda (`f[j] = has_gate ? y * (second ? g1[j] : g0[j]) : y` then pack2) and
    pw_bwd's dy = bf16(k1 * dz + k2 * y + k0) never leave the kernel: the reference rounds the fp64 operand to bf16
    (operand_* below) and the check allows the operand to land on its other bf16 neighbour (`hard`).

Bounds.  REL = 2^-8 (half a bf16 ulp, relative) and SLACK = 2^-16 are glue_oracle's; U32 = 2^-24 is half an fp32 ulp.
  tight (bf16 out, exact bf16 operands)
        |out - ref| <= REL |ref| + max(SLACK, Ktot U32) S,   Ktot = K + K2.
        REL |ref| is the one round-to-nearest store.  The products are exact (8 x 8 significant bits fit fp32); each of
        the Ktot (+ bias, res) fp32 additions rounds to nearest, error <= U32 |partial sum| <= U32 S, in any order:
        Ktot U32 S.  The floor SLACK keeps glue_oracle's allowance for the res * rmul fma and short reductions.
  f32   (fp32 out)  |out - ref| <= U32 |ref| + max(SLACK, n U32) sum|term|, n the reduction length (K, or M for a
        weight gradient; the fixed-order sum over the splits adds <= splits more additions, counted in n by the caller).
  hard  tight (or f32) + 2 FLIP T, FLIP = 2^-7, T the largest single |term| of the output.  A prologue evaluated in
        fp32 can land on the other side of a bf16 rounding boundary than the fp64 reference; that moves the operand by
        one bf16 ulp <= 2^-7 |operand| and the output by <= 2^-7 |term|.  Two such operands per output are allowed.
  caps  on a rebuilt-operand route every element is within hard, and outside tight lie at most
        max(2 fanout, CAP elements) elements, CAP = 2^-10 (dw_oracle.CAP_DY), fanout = the number of outputs one operand
        feeds (the N outputs of its row for a data gradient, the Ci outputs of its channel for a weight gradient): two
        flipped operands are always allowed, as in `hard`.  Units (rows of dx, output channels of dW) that hold any
        element outside tight number at most max(2, 4 Kop P_FLIP units): a unit has Kop rebuilt operands, an operand
        flips when its fp32 evaluation error (~4 roundings, 4 U32 |v|) straddles a boundary of its 2^-8 |v| wide
        rounding cell, P_FLIP = 4 U32 / 2^-8 = 2^-14, and 4 is the headroom for S / |v| > 1.  A count of elements
        without the fanout would fail a clean kernel: one flipped dy[m, k] moves all N outputs of row m.
        Both counts are upper bounds with wide headroom, not estimates.  The floor 2 fanout only matters where
        CAP elements < 2 fanout (fewer than 2^11 rows): there CAP alone would allow no flipped operand at all, although
        the flip rate per operand does not depend on the shape.  The per-unit count with Kop = M (a weight gradient: every
        row of the operand feeds the channel) allows up to 4 M 2^-14 of the channels, a third of them at M = 1400: it
        binds only where a unit has few operands (the rows of dx, Kop = CE <= 288: 7 % of the rows).  What a weight
        gradient is really held to is `hard` on every element, whose flip term 2^-6 max|term| is small against the sum.
  bias  mean signed bf16-ulp error, glue_oracle's BIAS_CAP over >= BIAS_MIN_COUNT elements, unchanged.
  z-mode expand backward (pw_bwd_z, expand_bwd_z_wide): the reference is the exact chain and the bound carries what
        pwbwd.hip rounds, addend by addend: bound_z_dx, bound_z_dwe.  On the wide route pw_z_prep's stored wt / mk / r0
        are the exact operands of pw_tall_tail / gemm_tail, so that product is also held to tight against them.
  proj_bwd: S0 / S1 / S3 = sum_p dA[p, c] X_q[p, c] with dA = dy3 Wp formed after the pixel sum
        (proj_bwd_frame_kernel: `v[0] = fmaf(w, g0, v[0])` over the MFMA accumulators of dy3^T X_q) and X_q the bf16
        operands of operands_proj_bwd: f32 bound over HW Cout terms + 2 FLIP T, T = max_p (|dy3| |Wp|)[p, c] |X_q[p, c]|,
        one operand feeding one output (fanout 1).  S2 / S4 sum the UNROUNDED fp32 sg and sg * xh
        (`s2[j] += g[j]; s4[j] += gx[j]`): f32 bound over HW terms with extra = SLACK for each term's own evaluation
        (glue_oracle's allowance), relative to the terms with their addends taken absolute.
"""
import torch

import glue_oracle as go

BF = torch.bfloat16
U32 = 2.0 ** -24
FLIP = 2.0 ** -7
CAP = 2.0 ** -10
P_FLIP = 2.0 ** -14


# ---- helpers ---------------------------------------------------------------------------------------------------------
def bf16_round(v):
    return v.float().to(BF).double()


def slack(n):
    """Relative-to-S allowance of a length-n fp32 reduction."""
    return max(go.SLACK, n * U32)


def weight(N, K, gen, std=1.0, device="cpu"):
    """[N, K] bf16 weight with the arange(N) * 0.01 row offset of the older tests: a transposed store cannot pass."""
    w = torch.randn(N, K, generator=gen) * std + torch.arange(N)[:, None] * 0.01
    return w.to(BF).to(device)


def acts(M, K, gen, mean=0.25, std=1.0, device="cpu"):
    """[M, K] bf16 activations with a non-zero mean."""
    return (torch.randn(M, K, generator=gen) * std + mean).to(BF).to(device)


def _rows(t, hw):
    return t.double().repeat_interleave(hw, 0)


def _max_term(ad, wd, chunk=256):
    """T[m, n] = max_k |a[m, k] w[k, n]| for a [M, K], w [K, N] fp64, a few rows at a time."""
    out = torch.empty(ad.shape[0], wd.shape[1], dtype=torch.float64, device=ad.device)
    wa = wd.abs()
    for m0 in range(0, ad.shape[0], chunk):
        out[m0:m0 + chunk] = (ad[m0:m0 + chunk].abs()[:, :, None] * wa[None]).amax(1)
    return out


# ---- references ------------------------------------------------------------------------------------------------------
def ref_gemm(a, w, nn=False, bias=None, a2=None, w2=None, res=None, rmul=None, rhw=1, pos=None, want_T=False):
    """C = a w^T (w [N, K]; nn: w [K, N], C = a w) + a2 w2^T + bias + res * rmul[m / rhw] + pos[m % len(pos)].
    a / a2 may be bf16 or an fp64 operand from an operand_* builder.  Returns (ref, S) or (ref, S, T)."""
    ad = a.double()
    wd = w.double() if nn else w.double().t()
    ref, S = ad @ wd, ad.abs() @ wd.abs()
    T = _max_term(ad, wd) if want_T else None
    if a2 is not None:
        a2d, w2d = a2.double(), w2.double().t()
        ref, S = ref + a2d @ w2d, S + a2d.abs() @ w2d.abs()
        if want_T:
            T = torch.maximum(T, _max_term(a2d, w2d))
    if bias is not None:
        ref, S = ref + bias.double(), S + bias.double().abs()
    if res is not None:
        p = res.double() * _rows(rmul, rhw)
        ref, S = ref + p, S + p.abs()
    if pos is not None:
        p = pos.double()[torch.arange(ad.shape[0], device=ad.device) % pos.shape[0]]
        ref, S = ref + p, S + p.abs()
    return (ref, S, T) if want_T else (ref, S)


def pw_strip_rows(K, N, bnb=False):
    """16 R, the rows of one wave's strip in pw_gemm_kernel (PwShape::R)."""
    nt, kc = (N + 15) // 16, (K + 31) // 32
    r0 = 128 // (4 * (nt + (4 if bnb else 2) * kc))
    return 16 * min(max(r0, 1), 8)


def pw_tile_index(M, K, N, grid, device="cpu"):
    """Workgroup that owns each row of pw_gemm_kernel: strip s = m / 16R belongs to workgroup (s / 4) % grid."""
    return (torch.arange(M, device=device) // pw_strip_rows(K, N) // 4) % grid


def ref_stats(c_stored, rows_per_tile=None, tile_index=None, tiles=None):
    """Per-tile partial rows of sum c and sum c^2 of the STORED bf16 C [M, N]: tile p covers rows
    p * rows_per_tile .. (or the rows with tile_index == p); a tile without rows is zero.
    Returns (ps, sum|c|, pq, rows) with ps / sum|c| / pq [tiles, N] fp64 and rows [tiles] the rows of each tile."""
    M, N = c_stored.shape
    if tile_index is None:
        tile_index = torch.arange(M, device=c_stored.device) // rows_per_tile
        tiles = (M + rows_per_tile - 1) // rows_per_tile if tiles is None else tiles
    c = c_stored.double()
    idx = tile_index.to(c.device).long()

    def part(v):
        return torch.zeros(tiles, N, dtype=torch.float64, device=c.device).index_add_(0, idx, v)

    rows = torch.zeros(tiles, dtype=torch.float64, device=c.device).index_add_(0, idx, torch.ones_like(c[:, 0]))
    return part(c), part(c.abs()), part(c * c), rows


def ref_wgrad(dy, a, want_T=True, chunk=64):
    """dW[co, ci] = sum_m dy[m, co] a[m, ci].  Returns (ref, sum|term|, max|term|), each [Co, Ci] fp64; dy / a bf16 or
    fp64 operands."""
    d, x = dy.double(), a.double()
    ref, sab = d.t() @ x, d.abs().t() @ x.abs()
    T = None
    if want_T:
        T = torch.zeros_like(ref)
        for m0 in range(0, d.shape[0], chunk):
            T = torch.maximum(T, (d[m0:m0 + chunk].abs()[:, :, None] * x[m0:m0 + chunk].abs()[:, None, :]).amax(0))
    return ref, sab, T


def ref_colsum(x):
    """(sum_m x, sum_m |x|) [C]: the sx of gram, the bias gradient of wgrad(sums=True)."""
    return x.double().sum(0), x.double().abs().sum(0)


# ---- operand builders: (bf16-rounded value fp64, unrounded fp64, S of the operand) -----------------------------------
def operand_project(y, scale, shift, gate, hw, act=1):
    """a = act(y * scale + shift) [* gate[m / hw]] of the project prologues (pw_gemm PRO, pw_tall PRO, gemm, wgrad)."""
    M, K = y.shape
    hw = hw if gate is not None else M
    v, S = go.ref_bn_apply(y.view(M // hw, hw, K), scale, shift, act, gate)
    v, S = v.reshape(M, K), S.reshape(M, K)
    return bf16_round(v), v, S


def operand_bnbwd(dout, y3, fmul, keep, hw, gamma, mean, rstd, mdz, mdzx):
    """dy3 = k1 * (dout * fmul[frame] * keep[frame]) + k2 * y3 + k0 of pw_gemm_bnbwd (pw_gemm_kernel BNB)."""
    M, K = dout.shape
    one, zero = torch.ones_like(mean), torch.zeros_like(mean)
    v, S = go.ref_bn_bwd_apply(dout.view(M // hw, hw, K), y3.view(M // hw, hw, K), one, zero, mean, rstd, gamma, 0, mdz,
                               mdzx, rs=fmul, keep=keep)
    v, S = v.reshape(M, K), S.reshape(M, K)
    return bf16_round(v), v, S


def operand_pw_bwd_dy(dA, y, consts):
    """dy = k1 * dA * silu'(y * sc + sh) + k2 * y + k0 of pw_bwd (consts [5, CE] = sc, sh, k1, k2, k0)."""
    sc, sh, k1, k2, k0 = consts.double().view(5, -1)
    yd = y.double()
    z = yd * sc + sh
    s = torch.sigmoid(z)
    v = k1 * dA.double() * (s * (1 + z * (1 - s))) + k2 * yd + k0
    S = (k1 * dA.double()).abs() * (s * (1 + z.abs() * (1 - s))) + (k2 * yd).abs() + k0.abs()
    return bf16_round(v), v, S


# ---- assertions ------------------------------------------------------------------------------------------------------
def _ratio(err, bound):
    return torch.where(bound > 0, err / bound.clamp_min(1e-300),
                       torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))


class GemmCheck(go.Bf16Check):
    """Bf16Check over a bf16 [rows, columns] output with the K-dependent slack and, for rebuilt-operand routes
    (T given), the hard bound, the element cap with its fanout and the per-unit (per-row) count."""

    def __init__(self, name, n, kop=0):
        super().__init__(name)
        self.n, self.kop = n, kop
        self.worst_hard, self.where_hard = 0.0, None
        self.outside, self.units_outside, self.units, self.fanout = 0, 0, 0, 1
        self.rebuilt = False

    def add(self, out, ref, S, T=None, n0=0):
        assert out.dtype == BF and ref.dtype == torch.float64 and out.dim() == 2, self.name
        assert out.shape == ref.shape == S.shape, (self.name, out.shape, ref.shape, S.shape)
        o = out.double()
        bad = ~torch.isfinite(o)
        if bad.any():
            idx = self._index(bad.reshape(-1).to(torch.uint8).argmax().item(), out.shape, n0)
            raise AssertionError(f"{self.name}: non-finite output at (row, column) = {idx}")
        err = (o - ref).abs()
        tight = go.REL * ref.abs() + slack(self.n) * S
        ratio = _ratio(err, tight)
        m, i = ratio.reshape(-1).max(0)
        if m.item() > self.worst:
            i = i.item()
            self.worst = m.item()
            self.where = (self._index(i, out.shape, n0), o.reshape(-1)[i].item(), ref.reshape(-1)[i].item(),
                          tight.reshape(-1)[i].item())
        over = err > tight
        self.outside += int(over.sum().item())
        self.units_outside += int(over.any(1).sum().item())
        self.units += out.shape[0]
        self.fanout = out.shape[1]
        if T is not None:
            self.rebuilt = True
            hard = tight + 2 * FLIP * T
            rh = _ratio(err, hard)
            m, i = rh.reshape(-1).max(0)
            if m.item() > self.worst_hard:
                i = i.item()
                self.worst_hard = m.item()
                self.where_hard = (self._index(i, out.shape, n0), o.reshape(-1)[i].item(), ref.reshape(-1)[i].item(),
                                   hard.reshape(-1)[i].item())
        q = ref.abs() > go.BIAS_FLOOR * S
        signed = torch.sign(ref) * (o - ref) / go.bf16_ulp(ref)
        self.ulp_sum += signed[q].sum().item()
        self.count += int(q.sum().item())
        self.elements += out.numel()

    @property
    def share(self):
        return self.outside / max(self.elements, 1)

    def _fail(self, what, worst, where):
        idx, o, r, b = where
        raise AssertionError(f"{self.name}: |out - ref| = {abs(o - r):.6g} is {worst:.3f} x the {what} bound {b:.6g} "
                             f"at (row, column) = {idx}: out {o!r}, ref {r!r}")

    def finish(self):
        if not self.rebuilt:
            if self.worst > 1.0:
                self._fail("tight", self.worst, self.where)
        else:
            if self.worst_hard > 1.0:
                self._fail("hard", self.worst_hard, self.where_hard)
            allowed = max(2 * self.fanout, CAP * self.elements)
            if self.outside > allowed:
                idx, o, r, b = self.where
                raise AssertionError(f"{self.name}: {self.outside} of {self.elements} elements ({self.share:.3g}) outside "
                                     f"the tight bound, allowed {allowed:.3g}; the worst, {self.worst:.3f} x the bound "
                                     f"{b:.6g}, at (row, column) = {idx}: out {o!r}, ref {r!r}")
            units = max(2.0, 4 * self.kop * P_FLIP * self.units)
            if self.units_outside > units:
                raise AssertionError(f"{self.name}: {self.units_outside} of {self.units} rows hold an element outside "
                                     f"the tight bound (allowed {units:.3g})")
        if self.count >= go.BIAS_MIN_COUNT and abs(self.mean_ulp) > go.BIAS_CAP:
            raise AssertionError(f"{self.name}: mean signed error {self.mean_ulp:+.4f} bf16 ulp over {self.count} "
                                 f"elements (cap {go.BIAS_CAP}): the stores are biased")
        return {"worst": self.worst, "worst_hard": self.worst_hard if self.rebuilt else self.worst,
                "share": self.share, "mean_ulp": self.mean_ulp, "count": self.count, "elements": self.elements,
                "sum": 0.0}


def assert_gemm(out, ref, S, n, name, T=None, kop=0):
    """bf16 out [M, N] against (ref, S) with reduction length n; T: the rebuilt-operand scheme with kop operands per row."""
    chk = GemmCheck(name, n, kop)
    chk.add(out, ref, S, T)
    return chk.finish()


def assert_f32(out, ref, sab, n, name, T=None, kop=0, fanout=None, extra=0.0):
    """fp32 out (out_f32 / embed products, weight gradients, Gram moments, statistics partials) against (ref, sum|term|)
    with reduction length n: |out - ref| <= U32 |ref| + (max(SLACK, n U32) + extra) sum|term| (+ 2 FLIP T on a
    rebuilt-operand route, with the element cap and the per-unit count; a unit is `fanout` consecutive outputs, default
    one row).  extra: the relative fp32 evaluation error of each term where the terms are not exact products.
    Returns the observed figures."""
    assert out.dtype in (torch.float32, torch.float64) and ref.dtype == torch.float64, (name, out.dtype, ref.dtype)
    assert out.shape == ref.shape == sab.shape, \
        (name, out.dtype, out.shape, ref.shape, sab.shape)
    o = out.double()
    bad = ~torch.isfinite(o)
    if bad.any():
        idx = go.Bf16Check._index(bad.reshape(-1).to(torch.uint8).argmax().item(), out.shape, 0)
        raise AssertionError(f"{name}: non-finite output at {idx}")
    err = (o - ref).abs()
    tight = U32 * ref.abs() + (slack(n) + extra) * sab
    bound = tight if T is None else tight + 2 * FLIP * T
    ratio = _ratio(err, bound)
    m, i = ratio.reshape(-1).max(0)
    m, i = m.item(), i.item()
    worst_tight = _ratio(err, tight).max().item()
    if m > 1.0:
        idx = go.Bf16Check._index(i, out.shape, 0)
        raise AssertionError(f"{name}: |out - ref| = {err.reshape(-1)[i].item():.6g} is {m:.3f} x the "
                             f"{'hard' if T is not None else 'fp32'} bound {bound.reshape(-1)[i].item():.6g} at {idx}: "
                             f"out {o.reshape(-1)[i].item()!r}, ref {ref.reshape(-1)[i].item()!r}")
    over = err > tight
    outside = int(over.sum().item())
    if T is not None:
        fanout = out.shape[-1] if fanout is None else fanout
        allowed = max(2 * fanout, CAP * out.numel())
        if outside > allowed:
            raise AssertionError(f"{name}: {outside} of {out.numel()} elements outside the fp32 bound, allowed {allowed:.3g}")
        rows = over.reshape(-1, fanout).any(1)
        units = max(2.0, 4 * kop * P_FLIP * rows.numel())
        if int(rows.sum().item()) > units:
            raise AssertionError(f"{name}: {int(rows.sum().item())} of {rows.numel()} units hold an element outside the "
                                 f"fp32 bound (allowed {units:.3g})")
    return {"worst": worst_tight, "worst_hard": m, "share": outside / max(out.numel(), 1), "mean_ulp": 0.0, "count": 0,
            "elements": out.numel(), "sum": worst_tight}


def assert_stats(ps, pq, c_stored, name, rows_per_tile=None, tile_index=None):
    """The kernel's (ps, pq) partial rows against ref_stats of its own stored C; rows of tiles past the end are zero.
    Returns the worst ratio."""
    tiles = ps.shape[0]
    rs, ra, rq, rows = ref_stats(c_stored, rows_per_tile, tile_index, tiles)
    n = max(int(rows.max().item()), 1)
    a = assert_f32(ps, rs, ra, n, name + " ps")
    b = assert_f32(pq, rq, rq, n, name + " pq")
    empty = rows == 0
    if empty.any():
        assert not ps[empty].any() and not pq[empty].any(), f"{name}: partial rows of tiles without rows are not zero"
    return max(a["worst"], b["worst"])


BIAS_SIGMAS = 10.0        # glue_oracle's BIAS_CAP is 10 sigma of the mean of n = 1e5 uniform store errors
BIAS_CAP_MAX = 0.25       # half the shift of a truncating store: a wider cap could not tell one from noise


def z_dx_prevar(dz, We, consts):
    """Variance of the error that pw_bwd_z_kernel's dx carries BEFORE its store, per output, from the number formats
    alone: each k1 * dz is rounded to bf16 (`u.x = pack2(k1[0] * zv[0], ...)`), an error uniform in +- half an ulp of
    that product, variance ulp^2 / 12, which reaches output (m, ci) times We[ce, ci]:
        V[m, ci] = sum_ce ulp(k1 dz[m, ce])^2 / 12 * We[ce, ci]^2.
    The hi / lo image of Mk (2^-16 relative) and the fp32 additions are 2^8 times smaller and left out."""
    k1 = consts.double().view(5, -1)[2]
    return (go.bf16_ulp(k1 * dz.double()) ** 2 / 12.0) @ (We.double() ** 2)


def assert_within(out, ref, bound, name, S=None, pre_var=None):
    """|out - ref| <= bound element-wise for a bound assembled by the caller (the z-mode expand backward); out bf16 or
    fp32.  A bf16 output is given S, the sum of its absolute addends, and then gets Bf16Check's bias assertion: over the
    elements with |ref| > BIAS_FLOOR S, at least BIAS_MIN_COUNT of them, the mean signed error stays within the cap.  A
    truncating store moves that mean by -0.5 and can fit inside a bound that has headroom for bf16 images.

    The cap is BIAS_CAP where the store is the only rounding that matters (pre_var None).  BIAS_CAP = 0.01 is 10 sigma
    of the mean of 1e5 errors uniform in +- 0.5 ulp (sigma 0.289 / sqrt(n)), and that premise fails where roundings
    BEFORE the store are as large as the store's: with the bf16 image of k1 dz, an element's error measured in ulps of
    a ref that its addends partly cancel has a standard deviation of 0.4 (288 x 48) to 2.8 (144 x 24) ulp, up to 80 ulp
    at single elements, and the mean of 100,041 of them has sigma 0.0086.  The all-round-to-nearest fp32 emulation of
    tests/test_gemm_oracle.py gives -0.0118 on the data of the 144 x 24, M = 4200 GPU case, and so does the kernel, to
    four digits: noise of the statistic, not a bias of the store.  So with pre_var (the variance of the pre-store error
    of each element, from the number formats: z_dx_prevar) the same 10-sigma rule is applied to the sigma this output
    has: element i has sigma_i = sqrt(1 / 12 + pre_var_i / ulp_i^2) ulp; the elements of one row share their rounded
    operands, so their errors are taken as fully correlated (an upper bound, whatever the signs):
        sigma_mean = sqrt(sum_rows (sum_i sigma_i)^2) / n,      cap = max(BIAS_CAP, 10 sigma_mean),
    and the statistic is asserted only while cap <= BIAS_CAP_MAX = 0.25, half a truncating store's shift (the caller
    asserts that its bias-sized case gets there).  Nothing here is read from the output under test.

    S is left out where one rounded value feeds many outputs with the same sign (the wide route's single bf16 image of
    Mk under an x of non-zero mean); the store of that output has its bias asserted against the stored operands
    instead.  Returns the figures with the worst ratio, the cap used as `bias_cap`."""
    assert ref.dtype == torch.float64 and out.shape == ref.shape == bound.shape, (name, out.shape, ref.shape)
    assert S is None or out.dtype == BF, f"{name}: the bias statistic is for a bf16 output"
    assert pre_var is None or S is not None, name
    o = out.double()
    bad = ~torch.isfinite(o)
    if bad.any():
        idx = go.Bf16Check._index(bad.reshape(-1).to(torch.uint8).argmax().item(), out.shape, 0)
        raise AssertionError(f"{name}: non-finite output at {idx}")
    err = (o - ref).abs()
    m, i = _ratio(err, bound).reshape(-1).max(0)
    m, i = m.item(), i.item()
    if m > 1.0:
        idx = go.Bf16Check._index(i, out.shape, 0)
        raise AssertionError(f"{name}: |out - ref| = {err.reshape(-1)[i].item():.6g} is {m:.3f} x the bound "
                             f"{bound.reshape(-1)[i].item():.6g} at {idx}: out {o.reshape(-1)[i].item()!r}, "
                             f"ref {ref.reshape(-1)[i].item()!r}")
    st = {"worst": m, "worst_hard": m, "share": 0.0, "mean_ulp": 0.0, "count": 0, "elements": out.numel(), "sum": 0.0}
    if S is not None:
        assert S.shape == ref.shape, (name, S.shape, ref.shape)
        q = ref.abs() > go.BIAS_FLOOR * S
        signed = torch.sign(ref) * (o - ref) / go.bf16_ulp(ref)
        st["count"] = n = int(q.sum().item())
        st["mean_ulp"] = signed[q].sum().item() / max(n, 1)
        cap = go.BIAS_CAP
        if pre_var is not None and n > 0:
            assert pre_var.shape == ref.shape and ref.dim() == 2, (name, pre_var.shape)
            sig = torch.sqrt(1.0 / 12.0 + pre_var / go.bf16_ulp(ref) ** 2) * q
            cap = max(cap, BIAS_SIGMAS * torch.sqrt((sig.sum(1) ** 2).sum()).item() / n)
        st["bias_cap"] = cap
        if n >= go.BIAS_MIN_COUNT and cap <= BIAS_CAP_MAX and abs(st["mean_ulp"]) > cap:
            raise AssertionError(f"{name}: mean signed error {st['mean_ulp']:+.4f} bf16 ulp over {n} "
                                 f"elements (cap {cap:.4g}): the stores are biased")
    return st


def ref_expand_bwd_z(dz, x, We, consts, res=None, rmul=None, rhw=1):
    """The exact chain of the y-free expand backward (pwbwd.hip pw_bwd_z_kernel, backbone.expand_bwd_z_wide):
        dy1 = k1 dz + k2 (x We^T) + k0,   dx = dy1 We (+ res * rmul[m / rhw]),   dWe = dy1^T x
    with consts [5, CE] = sc, sh, k1, k2, k0.  Returns a dict of fp64 tensors: dx, dWe and the magnitudes of the three
    addends as the kernels form them (they cancel when x has a non-zero mean, so each is kept):
        A  = |k1 dz| |We|           (the dz product)          X  = |x| |Mk|,  Mk = We^T diag(k2) We
        Xa = |x| (|We|^T |k2| |We|) (what Mk's own fp32 sum is relative to)      R = |k0| |We|  (r0)
        W1 = |k1 dz|^T |x|,  W2 = |k2| (|We| (|x|^T |x|)),  W3 = |k0| (sum_m |x|)   (dWe's three addends)."""
    k1, k2, k0 = consts.double().view(5, -1)[2:]
    d, xd, W = dz.double(), x.double(), We.double()
    dy1 = k1 * d + k2 * (xd @ W.t()) + k0
    Mk = W.t() @ (k2[:, None] * W)
    Mka = W.abs().t() @ (k2.abs()[:, None] * W.abs())
    out = {"dx": dy1 @ W, "dWe": dy1.t() @ xd, "Mk": Mk, "Mk_abs": Mka, "r0": k0 @ W, "R": k0.abs() @ W.abs(),
           "A": (k1 * d).abs() @ W.abs(), "X": xd.abs() @ Mk.abs(), "Xa": xd.abs() @ Mka,
           "W1": (k1 * d).abs().t() @ xd.abs(), "W2": k2.abs()[:, None] * (W.abs() @ (xd.abs().t() @ xd.abs())),
           "W3": k0.abs()[:, None] * xd.abs().sum(0)[None], "P": torch.zeros_like(xd)}
    if res is not None:
        p = res.double() * _rows(rmul, rhw)
        out["dx"], out["P"] = out["dx"] + p, p.abs()
    return out


def S_z_dx(r):
    """The absolute addends of the z-mode dx as the kernels sum them: the dz product, x Mk, r0 and the residual."""
    return r["A"] + r["X"] + r["R"] + r["P"]


def bound_z_dx(r, CE, CIN, mk_rel):
    """dx of the z-mode expand backward against the exact chain.  The kernels evaluate
        dx = bf16-image(k1 dz . We) + x . bf16-image(Mk) + r0 + res * rmul, stored once:
      REL |ref|                      the store;
      REL A                          the bf16 image of the dz product: pw_bwd_z_kernel rounds each k1 * dz
                                     (`u.x = pack2(k1[0] * zv[0], ...)`), pw_z_prep_kernel each k1 * We
                                     (`wt[...] = f2bf(k1[ce2] * tile[tx][ty])`); half an ulp per term, REL |term|;
      mk_rel X                       the bf16 image of Mk: one rounding, REL, on the wide route
                                     (`mk[i * CIN + j] = f2bf(sum)`); the hi / lo pair of pw_bwd_prep_kernel
                                     (`mk[i] = hi; mk[CINP * KCP + i] = f2bf(a - bf2f(hi))`) leaves REL^2;
      CE U32 (Xa + R)                Mk and r0 are fp32 sums of CE terms;
      slack(CE + 2 CIN + 2)(A + X + R + P)   the fp32 accumulation over both segments (hi and lo), r0 and the residual."""
    return go.REL * r["dx"].abs() + go.REL * r["A"] + mk_rel * r["X"] + CE * U32 * (r["Xa"] + r["R"]) \
        + slack(CE + 2 * CIN + 2) * (r["A"] + r["X"] + r["R"] + r["P"])


def bound_z_dwe(r, M, CIN, parts, image):
    """dWe of the z-mode expand backward against the exact chain: dWe = [k1] S + k2 (We G) + k0 sx in fp32
    (pw_bwd_finish_kernel / pw_z_finish_kernel) with S, G, sx fp32 sums over M rows and `parts` partials, then CIN + 3
    more operations: U32 |ref| + slack(M + parts + CIN + 3)(W1 + W2 + W3); image: + REL W1 where S is summed over the
    bf16 image of k1 dz (pw_bwd_z_kernel; the wide route sums exact dz^T x and scales by k1 afterwards)."""
    b = U32 * r["dWe"].abs() + slack(M + parts + CIN + 3) * (r["W1"] + r["W2"] + r["W3"])
    return b + go.REL * r["W1"] if image else b


def operands_proj_bwd(y2, scale, shift, mean, rstd):
    """The three MFMA operands of proj_bwd_frame_kernel's stage lambda, X_0 = act = silu(z), X_1 = sg = silu'(z),
    X_2 = sg * xh with z = y2 * scale + shift, xh = (y2 - mean) * rstd: dict q -> (bf16-rounded fp64, unrounded, the
    value with its addends taken absolute).  y2 [M, Ce]."""
    y = y2.double()
    z = y * scale.double() + shift.double()
    s = torch.sigmoid(z)
    act, sg = z * s, s * (1 + z * (1 - s))
    sga = s * (1 + z.abs() * (1 - s))
    xh = (y - mean.double()) * rstd.double()
    xha = (y.abs() + mean.double().abs()) * rstd.double().abs()
    za = (y * scale.double()).abs() + shift.double().abs()
    return {0: (bf16_round(act), act, za * s), 1: (bf16_round(sg), sg, sga), 2: (bf16_round(sg * xh), sg * xh, sga * xha)}


class Table:
    """The -s output: one line per case and one summary per entry point."""

    def __init__(self, entry):
        self.entry, self.rows = entry, []

    def add(self, case, st):
        self.rows.append(st)
        print(f"\ngemm oracle | {self.entry:14s} | {case:58s} | worst/tight {st['worst']:6.3f} | worst/hard "
              f"{st['worst_hard']:6.3f} | outside {st['share']:.2e} (cap {CAP:.2e} or 2 x fanout) | sum {st.get('sum', 0.0):6.3f} | "
              f"mean ulp {st['mean_ulp']:+.4f}", end="")
        return st

    def summary(self):
        r = self.rows
        if not r:
            return
        big = [s for s in r if s["count"] >= go.BIAS_MIN_COUNT]
        ulp = max((abs(s["mean_ulp"]) for s in big), default=0.0)
        print(f"\ngemm oracle | {self.entry:14s} | SUMMARY {len(r):4d} cases | worst/tight "
              f"{max(s['worst'] for s in r):6.3f} | worst/hard {max(s['worst_hard'] for s in r):6.3f} | outside "
              f"{max(s['share'] for s in r):.2e} (cap {CAP:.2e} or 2 x fanout) | sum {max(s.get('sum', 0.0) for s in r):6.3f} | "
              f"|mean ulp| {ulp:.4f} over {len(big)} cases of >= {go.BIAS_MIN_COUNT} elements")
