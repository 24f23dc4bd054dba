"""fp64 references and the element-wise oracle for the depthwise kernels (csrc/kernels/dw_*.hip).

Plain torch, CPU or GPU tensors, no extension call.  Activations are NHWC bf16 [N, H, W, C], weights [C, k*k] fp32 with
tap t = kh*k + kw, pad (k-1)/2.  Every reference is a sum over the k*k taps of shifted slices of a zero-padded NHWC
tensor and returns (ref, S) with S the same tap sum over absolute values, S = sum_t |w_t| * S_operand_t (glue_oracle's
convention: the magnitude that the fp32 roundings are relative to).

What the kernels compute, read from the kernel units and cited by function (dw_fwd.hip: stage_tile_t, epilogue<EPI>,
dw_fwd_kernel, the dw_bwd_data kernel, dw_bwd_weight_kernel, dw_bwd_fused_kernel; dw_bwd_s1.hip: stage_dy_half,
dw_bwd_uni_kernel; dw_bwd_s2.hip: uni_s2_class; dw/dw_stage.h: zero_ring, stage_dy; dw/dw_uni.h: centre_silu):
  * Zero padding applies to the operand AFTER its prologue: stage_tile_t and stage_dy / stage_dy_half write zeros for
    the ring and for out-of-image pixels (zero_ring; `if (!ok[k]) v = 0`), the prologue runs only on loaded pixels
    (stage_tile_t: `if (PRO != PRO_COPY && (valid >> k & 1u))`).
  * A staged operand is bf16 (pack2 before `tile[p * cv + vv] = v` in stage_tile_t and stage_dy), so the operand
    functions below round the fp64 operand to bf16 before the tap sum.  One exception: the unified backward kernels
    build a = silu(bn1(x1)) for the WEIGHT product in fp32 registers and never round it (centre_silu:
    `a[r][j] = ok[r] ? z * t : 0`, used in the tap loops of dw_bwd_uni_kernel and uni_s2_class:
    `wacc[..] = in[j] * a[r][j] + wacc[..]`), so operand_bn_silu takes round=False for their weight gradient; the
    two-pass kernel (dw_bwd_fused_kernel) and dw_bwd_weight_kernel stage a through stage_tile as bf16.
  * Partial sums.  The forward's EPI_STATS sums the STORED bf16 outputs (dw_fwd_kernel: `unpack4x2(u, v)` of the
    packed word that was stored).  The EPI_BNBWD epilogue of dw_bwd_data and of the two-pass fused kernel rounds
    first (epilogue<EPI>: `o[j] = bf2f(f2bf(o[j]))`, "statistics describe the stored bf16 tensor") and sums
    dz = bf16(dx) * silu'(z), dz * xhat with xhat = y * rstd - mean * rstd.  The unified kernels do the same (the
    epilogues of dw_bwd_uni_kernel and uni_s2_class: `CV::unpack(o, of)`; `if (!zout) dz = dz * gp`).  With zout they
    store bf16(dx_fp32 * silu'(z)) -- the fp32 accumulator times silu', one rounding
    (`acc[r][j] = acc[r][j] * gp[r][j]` before the pack) -- and sum that stored dz.
  * res / rmul: `acc = rv * fm + acc` in fp32 before the one rounding of the store (dw_bwd_uni_kernel's epilogue).
  * silu'(z) = s (1 + z (1 - s)) has the addends 1 and z (1 - s), which cancel at z = -1.278: S of a dz output carries
    s (1 + |z| (1 - s)), not |silu'(z)|  (silu_grad_abs).

Bounds (REL = 2^-8 and SLACK = 2^-16 are glue_oracle's):
  tight  |out - ref| <= REL |ref| + SLACK S.  Accumulating <= 25 products in fp32 adds < 2^-19 S, inside the slack.
  hard   tight + 2^-7 F, F = sum_t |w_t * operand_t|: an fp32 evaluation of a prologue that lands on the other side of
         a bf16 rounding boundary moves that operand by one bf16 ulp <= 2^-7 |operand|.
Routes whose operands are exact bf16 inputs (cap = 0) hold every element to tight.  Rounded-intermediate routes hold
every element to hard, at most `cap` of the elements outside tight (CAP_PROLOGUE = 2^-12 where only a prologue operand
is rounded, CAP_DY = 2^-10 where dy is rebuilt) and no channel more than fanout * max(2, 16 * cap * elements of that
channel).  The per-channel allowance counts flipped OPERANDS: one operand that lands on its other bf16 neighbour
feeds up to fanout = k*k outputs, all of its own channel, so a count of outputs without that factor is wrong -- the
clean CPU emulation of tests/test_dw_oracle.py put 9 outputs of one channel outside tight with a single flip at k = 3,
over max(2, 16 * 2^-12 * 1848 = 7.2).  A faulty channel still stands out: it has most of its elements outside tight.
Sums: |sum - ref| <= 2^-16 sum|term| (+ 2^-6 max|term| where operands are rounded inside the kernel: two flips).
"""
import torch

import glue_oracle as go

BF = torch.bfloat16
FLIP = 2.0 ** -7
CAP_PROLOGUE = 2.0 ** -12
CAP_DY = 2.0 ** -10
SUM_REL = 2.0 ** -16
SUM_FLIP = 2.0 ** -6


# ---- inputs ----------------------------------------------------------------------------------------------------------
def out_hw(H, W, k, s):
    p = (k - 1) // 2
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def make_inputs(N, H, W, C, k, s, seed, device):
    """One set of operands for every depthwise entry point at input shape (N, H, W, C): seeded CPU generator,
    activations with a non-zero mean, weights 0.3 * randn.  Suffix 1 = BN1 (the producer of x1), 2 = BN2."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    Ho, Wo = out_hw(H, W, k, s)

    def randn(*sh):
        return torch.randn(*sh, generator=gen)

    def rand(*sh):
        return torch.rand(*sh, generator=gen)

    d = {}
    d["x"] = (randn(N, H, W, C) * 1.3 + 0.2).to(BF)                    # the depthwise input x1 / y1
    d["g"] = (randn(N, Ho, Wo, C) + 0.1).to(BF)                        # a bf16 dy
    d["dA"] = (randn(N, Ho, Wo, C) + 0.1).to(BF)
    d["y2"] = (randn(N, Ho, Wo, C) * 1.5 + 0.2).to(BF)
    d["res"] = (randn(N, H, W, C) * 1.3 + 0.2).to(BF)
    d["w"] = randn(C, k * k) * 0.3
    d["sc1"], d["sh1"] = rand(C) + 0.5, randn(C) * 0.2
    d["mu1"], d["rs1"] = randn(C) * 0.1, rand(C) + 0.5
    d["sc2"], d["sh2"] = rand(C) + 0.5, randn(C) * 0.2
    d["mu2"], d["rs2"], d["g2"] = randn(C) * 0.1, rand(C) + 0.5, rand(C) + 0.5
    d["mdz2"], d["mdzx2"] = randn(C) * 0.05, randn(C) * 0.05
    d["gate"], d["rb"] = rand(N, C), randn(N, C) * 0.1
    d["rmul"] = rand(N, C) + 0.5
    return {key: v.to(device).contiguous() for key, v in d.items()}


# ---- operands: (value fp64, S_operand) -------------------------------------------------------------------------------
def bf16_round(v):
    return v.float().to(BF).double()


def operand_raw(x):
    v = x.double()
    return v, v.abs()


def _flat(t):
    return t.reshape(t.shape[0], -1, t.shape[-1])


def operand_bn_silu(x, scale, shift, round=True):
    """silu(x*scale + shift) as the kernels stage it (bf16) or, round=False, as the unified kernels keep it in fp32."""
    a, S = go.ref_bn_apply(_flat(x), scale, shift, 1)
    a, S = a.reshape(x.shape), S.reshape(x.shape)
    return (bf16_round(a) if round else a), S


def operand_dy(d):
    """dy = BN2 backward-apply of (dA, y2, gate, rb) with SiLU, rebuilt by stage_dy and staged as bf16."""
    dA = d["dA"]
    v, S = go.ref_bn_bwd_apply(_flat(dA), _flat(d["y2"]), d["sc2"], d["sh2"], d["mu2"], d["rs2"], d["g2"], 1, d["mdz2"],
                               d["mdzx2"], rs=d["gate"], rb=d["rb"])
    return bf16_round(v.reshape(dA.shape)), S.reshape(dA.shape)


def silu_grad(x, scale, shift):
    return go._silu_grad(x.double() * scale.double() + shift.double())


def silu_grad_abs(x, scale, shift):
    """s (1 + |z| (1 - s)): silu'(z) with its addends taken absolute."""
    z = x.double() * scale.double() + shift.double()
    s = torch.sigmoid(z)
    return s * (1 + z.abs() * (1 - s))


# ---- tap sums --------------------------------------------------------------------------------------------------------
def _pad(a, p):
    N, H, W, C = a.shape
    out = torch.zeros(N, H + 2 * p, W + 2 * p, C, dtype=a.dtype, device=a.device)
    out[:, p:p + H, p:p + W] = a
    return out


def _fwd_sum(a, w, k, s):
    N, H, W, C = a.shape
    Ho, Wo = out_hw(H, W, k, s)
    ap = _pad(a, (k - 1) // 2)
    out = torch.zeros(N, Ho, Wo, C, dtype=torch.float64, device=a.device)
    for kh in range(k):
        for kw in range(k):
            out += w[:, kh * k + kw] * ap[:, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s]
    return out


def _bwd_sum(g, w, H, W, k, s):
    N, Ho, Wo, C = g.shape
    p = (k - 1) // 2
    dp = torch.zeros(N, H + 2 * p, W + 2 * p, C, dtype=torch.float64, device=g.device)
    for kh in range(k):
        for kw in range(k):
            dp[:, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s] += w[:, kh * k + kw] * g
    return dp[:, p:p + H, p:p + W].contiguous()


def ref_fwd(op, w, k, s):
    """out[n, oh, ow, c] = sum_t w[c, t] a[n, oh*s + kh - p, ow*s + kw - p, c].  op = (a, S_a).  Returns (ref, S)."""
    wd = w.double()
    return _fwd_sum(op[0], wd, k, s), _fwd_sum(op[1], wd.abs(), k, s)


def flip_fwd(op, w, k, s):
    """F of the hard bound for ref_fwd: sum_t |w_t a_t|."""
    return _fwd_sum(op[0].abs(), w.double().abs(), k, s)


def ref_bwd_data(op, w, H, W, k, s):
    """dx[n, ih, iw, c] = sum_{t: (ih + p - kh, iw + p - kw) = s (oh, ow)} w[c, t] dy[n, oh, ow, c].  op = (dy, S_dy)."""
    wd = w.double()
    return _bwd_sum(op[0], wd, H, W, k, s), _bwd_sum(op[1], wd.abs(), H, W, k, s)


def flip_bwd_data(op, w, H, W, k, s):
    return _bwd_sum(op[0].abs(), w.double().abs(), H, W, k, s)


def ref_bwd_weight(gop, aop, k, s):
    """dw[c, t] = sum_{n, oh, ow} dy[n, oh, ow, c] a[n, oh*s + kh - p, ow*s + kw - p, c].
    Returns (ref, sum |term|, max |term|), each [C, k*k]."""
    g, a = gop[0], aop[0]
    N, Ho, Wo, C = g.shape
    ap = _pad(a, (k - 1) // 2)
    ref, sab, mab = [], [], []
    for kh in range(k):
        for kw in range(k):
            term = g * ap[:, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s]
            ref.append(term.sum((0, 1, 2)))
            sab.append(term.abs().sum((0, 1, 2)))
            mab.append(term.abs().amax((0, 1, 2)))
    return torch.stack(ref, 1), torch.stack(sab, 1), torch.stack(mab, 1)


def ref_stats(out):
    """Column sums of the forward's (ps, pq) from the kernel's own stored output: (ref, sum |term|) for each."""
    o = out.double()
    return (o.sum((0, 1, 2)), o.abs().sum((0, 1, 2))), ((o * o).sum((0, 1, 2)),) * 2


def ref_bn_partials(stored, y, scale, shift, mean, rstd, zout=False):
    """Column sums of (pdz, pdzx) from the kernel's own stored bf16 tensor: dz = stored * silu'(y*scale + shift), or
    dz = stored where the kernel stored dz itself (zout); xhat = (y - mean) * rstd.  (ref, sum |term|) for each."""
    dz = stored.double()
    if not zout:
        dz = dz * silu_grad(y, scale, shift)
    t2 = dz * ((y.double() - mean.double()) * rstd.double())
    return (dz.sum((0, 1, 2)), dz.abs().sum((0, 1, 2))), (t2.sum((0, 1, 2)), t2.abs().sum((0, 1, 2)))


# ---- assertions ------------------------------------------------------------------------------------------------------
class DwCheck(go.Bf16Check):
    """Bf16Check over an NHWC output with, for the rounded-intermediate routes (cap > 0), the hard bound, the allowed
    share outside tight and the per-channel count.  cap = 0: every element within tight."""

    def __init__(self, name, cap=0.0, fanout=1):
        super().__init__(name)
        self.cap, self.fanout = cap, fanout
        self.worst_hard, self.where_hard = 0.0, None
        self.outside, self.per_channel, self.per_channel_n = 0, None, 0

    def add(self, out, ref, S, flip=None, n0=0):
        assert out.dim() == 4, self.name
        super().add(out, ref, S, n0)
        err = (out.double() - ref).abs()
        tight = go.REL * ref.abs() + go.SLACK * S
        over = err > tight
        self.outside += int(over.sum().item())
        pc = over.sum((0, 1, 2))
        self.per_channel = pc if self.per_channel is None else self.per_channel + pc
        self.per_channel_n += out.numel() // out.shape[-1]
        if self.cap > 0:
            assert flip is not None and flip.shape == ref.shape, self.name
            hard = tight + FLIP * flip
            ratio = torch.where(hard > 0, err / hard.clamp_min(1e-300),
                                torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
            m, i = ratio.reshape(-1).max(0)
            if m.item() > self.worst_hard:
                i = i.item()
                self.worst_hard = m.item()
                self.where_hard = (self._index(i, out.shape, n0), out.reshape(-1)[i].item(), ref.reshape(-1)[i].item(),
                                   hard.reshape(-1)[i].item())

    @property
    def share(self):
        return self.outside / max(self.elements, 1)

    def _fail(self, what, worst, where):
        idx, o, r, b = where
        raise AssertionError(f"{self.name}: |out - ref| = {abs(o - r):.6g} is {worst:.3f} x the {what} bound {b:.6g} "
                             f"at (n, h, w, c) = {idx}: out {o!r}, ref {r!r}")

    def finish(self):
        if self.cap == 0:
            if self.worst > 1.0:
                self._fail("tight", self.worst, self.where)
        else:
            if self.worst_hard > 1.0:
                self._fail("hard", self.worst_hard, self.where_hard)
            if self.share > self.cap:
                idx, o, r, b = self.where
                raise AssertionError(f"{self.name}: {self.outside} of {self.elements} elements ({self.share:.3g}) outside "
                                     f"the tight bound, cap {self.cap:.3g}; the worst, {self.worst:.3f} x the bound "
                                     f"{b:.6g}, at (n, h, w, c) = {idx}: out {o!r}, ref {r!r}")
            allowed = self.fanout * max(2, 16 * self.cap * self.per_channel_n)
            m, c = self.per_channel.max(0)
            if m.item() > allowed:
                raise AssertionError(f"{self.name}: channel {c.item()} holds {m.item()} of its {self.per_channel_n} "
                                     f"elements outside the tight bound (allowed {allowed:.3g})")
        if self.count >= go.BIAS_MIN_COUNT and abs(self.mean_ulp) > go.BIAS_CAP:
            raise AssertionError(f"{self.name}: mean signed error {self.mean_ulp:+.4f} bf16 ulp over {self.count} "
                                 f"elements (cap {go.BIAS_CAP}): the stores are biased")
        return {"worst": self.worst, "worst_hard": self.worst_hard if self.cap > 0 else self.worst, "share": self.share,
                "mean_ulp": self.mean_ulp, "count": self.count, "elements": self.elements}


def assert_dw(out, ref, S, name, cap=0.0, flip=None, fanout=1):
    chk = DwCheck(name, cap, fanout)
    chk.add(out, ref, S, flip)
    return chk.finish()


def sum_ratio(got, ref, sum_abs, max_abs=None):
    """max over the entries of |got - ref| / (2^-16 sum|term| [+ 2^-6 max|term|]) and its flat index."""
    bound = SUM_REL * sum_abs
    if max_abs is not None:
        bound = bound + SUM_FLIP * max_abs
    err = (got.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                        torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isfinite(got.double()), ratio, torch.full_like(ratio, float("inf")))
    m, i = ratio.reshape(-1).max(0)
    return m.item(), i.item(), bound


def assert_sums(got, ref, sum_abs, name, max_abs=None):
    """Column sums / weight gradient [C] or [C, k*k] against fp64.  Returns the worst ratio."""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    m, i, bound = sum_ratio(got, ref, sum_abs, max_abs)
    if m > 1.0:
        idx = go.Bf16Check._index(i, ref.shape, 0)
        raise AssertionError(f"{name}: |sum - ref| = {abs(got.reshape(-1)[i].item() - ref.reshape(-1)[i].item()):.6g} "
                             f"is {m:.3f} x the bound {bound.reshape(-1)[i].item():.6g} at (channel[, tap]) = {idx}: "
                             f"sum {got.reshape(-1)[i].item()!r}, ref {ref.reshape(-1)[i].item()!r}")
    return m
