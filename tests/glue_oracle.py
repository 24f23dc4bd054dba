"""fp64 references and the bf16-exactness oracle for the BN / block-tail glue passes (csrc/kernels/bn.hip, block.hip).

Plain torch, CPU or GPU tensors, no extension call: the references are written from the formulas in the kernel
comments.  Activations are [N, HW, C] bf16, per-channel vectors [C] fp32, per-frame rows [N, C] fp32, keep [N] fp32.
A reference works on any run of whole frames (pass y[n0:n1], rs[n0:n1], keep[n0:n1]), so a large tensor can be
checked frame by frame through Bf16Check.add without holding its fp64 image.

Every elementwise reference returns (ref, S).  S is the sum of the absolute values of the addends of the result, each
with its multipliers: the magnitude that the fp32 roundings of the kernel are relative to, which is much larger than
|ref| where the addends cancel.

The element-wise bound  |out - ref| <= 2^-8 |ref| + 2^-16 S  is derived, not measured:
  * the round-to-nearest bf16 store is off by at most half an ulp, and half a bf16 ulp is <= 2^-8 |value|;
  * the fp32 evaluation has <= ~10 roundings of 2^-24 each, a 1-ulp v_exp and a 1-ulp v_rcp, amplified by at most
    |z| <= ~8 inside silu'(z) = s (1 + z (1 - s)): together <= 2^-17 S, and 2^-16 leaves a factor 2.
The bias cap: a round-to-nearest error is uniform in +-0.5 ulp, so its mean over n >= 1e5 elements has
sigma = 0.289 / sqrt(n) < 0.001; the cap 0.01 is 10 sigma.  A truncating store gives -0.5.
"""
import torch

BF = torch.bfloat16
REL = 2.0 ** -8          # half a bf16 ulp, relative
SLACK = 2.0 ** -16       # fp32 evaluation error, relative to S
BIAS_FLOOR = 2.0 ** -10  # elements with |ref| > BIAS_FLOOR * S enter the bias statistic
BIAS_MIN_COUNT = 100_000
BIAS_CAP = 0.01


# ---- inputs (as tests/test_frame_gpu._inputs) ------------------------------------------------------------------------
def make_inputs(N, HW, C, seed, device):
    """One set of operands for every glue operation at shape (N, HW, C)."""
    gen = torch.Generator(device="cpu").manual_seed(seed)

    def randn(*s):
        return torch.randn(*s, generator=gen)

    def rand(*s):
        return torch.rand(*s, generator=gen)

    d = {}
    d["y"] = (randn(N, HW, C) * 1.3 + 0.2).to(BF)
    d["G"] = (randn(N, HW, C) * 0.1).to(BF)
    d["skip"] = (randn(N, HW, C) * 1.3 + 0.2).to(BF)
    d["scale"], d["shift"] = rand(C) + 0.5, randn(C) * 0.2
    d["mean"], d["rstd"], d["gamma"] = randn(C) * 0.1, rand(C) + 0.5, rand(C) + 0.5
    d["mdz"], d["mdzx"] = randn(C) * 0.05, randn(C) * 0.05
    d["rs"], d["rb"] = rand(N, C) + 0.5, randn(N, C) * 0.02
    d["fmul"], d["fadd"] = rand(N, C) + 0.5, randn(N, C) * 0.2
    keep = (rand(N) > 0.3).float() / 0.7
    # at least one dropped and one kept frame where there is room for both
    keep[0] = 1.0 / 0.7
    if N > 1:
        keep[N // 2] = 0.0
    d["keep"] = keep
    return {k: v.to(device).contiguous() for k, v in d.items()}


# ---- fp64 references -------------------------------------------------------------------------------------------------
def _row(t):
    return t.double()[:, None, :]


def _silu_grad(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def ref_bn_apply(y, scale, shift, act, rs=None):
    """out = act(y*scale + shift) [* rs[n, c]].  silu is 1.1-Lipschitz and |silu(z)| <= |z|, so S of z serves both."""
    a = y.double() * scale.double()
    z = a + shift.double()
    S = a.abs() + shift.double().abs()
    out = z * torch.sigmoid(z) if act else z
    if rs is not None:
        out = out * _row(rs)
        S = S * _row(rs).abs()
    return out, S


def bwd_consts(mean, rstd, gamma, mdz, mdzx):
    """k1 = gamma*rstd (gamma = 1 when absent), k2 = -k1*rstd*mdzx, k0 = -k1*(mdz - mean*rstd*mdzx)."""
    k1 = (gamma.double() if gamma is not None else 1.0) * rstd.double()
    k2 = -k1 * rstd.double() * mdzx.double()
    k0 = -k1 * (mdz.double() - mean.double() * rstd.double() * mdzx.double())
    return k1, k2, k0


def ref_bn_bwd_apply(G, y, scale, shift, mean, rstd, gamma, act, mdz, mdzx, rs=None, rb=None, keep=None):
    """dz = (G * rs[n,c] * keep[n] + rb[n,c]) [* silu'(y*scale+shift)];  dy = k1*dz + k2*y + k0."""
    yd = y.double()
    a = G.double()
    if rs is not None:
        a = a * _row(rs)
    if keep is not None:
        a = a * keep.double()[:, None, None]
    gabs = a.abs()
    if rb is not None:
        a = a + _row(rb)
        gabs = gabs + _row(rb).abs()
    sg = _silu_grad(yd * scale.double() + shift.double()) if act else 1.0
    k1, k2, k0 = bwd_consts(mean, rstd, gamma, mdz, mdzx)
    out = k1 * (a * sg) + k2 * yd + k0
    S = (k1 * sg).abs() * gabs + (k2 * yd).abs() + k0.abs()
    return out, S.expand_as(out)


def ref_block_tail(y3, scale, shift, keep=None, skip=None, fmul=None, fadd=None):
    """out = ((y3*scale + shift) * keep[n] + skip) * fmul[n,c] + fadd[n,c]."""
    a = y3.double() * scale.double()
    out = a + shift.double()
    S = a.abs() + shift.double().abs()
    if keep is not None:
        kp = keep.double()[:, None, None]
        out, S = out * kp, S * kp.abs()
    if skip is not None:
        out, S = out + skip.double(), S + skip.double().abs()
    if fmul is not None:
        out = out * _row(fmul) + _row(fadd)
        S = S * _row(fmul).abs() + _row(fadd).abs()
    return out, S.expand_as(out)


def ref_add_scaled(x, y, s):
    """x + y * s[n, c]."""
    p = y.double() * _row(s)
    return x.double() + p, x.double().abs() + p.abs()


def ref_bn_stats(x, P):
    """Partial rows [P, C] of sum x and sum x^2: block p covers rows p*rpb .. min(M, (p+1)*rpb), rpb = ceil(M / P);
    a block past the end writes zeros."""
    M, C = x.shape
    rpb = (M + P - 1) // P
    xd = torch.zeros(P * rpb, C, dtype=torch.float64, device=x.device)
    xd[:M] = x.double()
    xd = xd.view(P, rpb, C)
    return xd.sum(1), (xd * xd).sum(1)


def ref_bn_finalize(ps, pq, count, gamma, beta, eps, momentum=None, rmean=None, rvar=None):
    """Column sums over P -> scale, shift, mean, rstd (biased variance clamped at 0) and, given running statistics,
    their update with the unbiased variance."""
    mean = ps.double().sum(0) / count
    var_raw = pq.double().sum(0) / count - mean * mean
    var = var_raw.clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    gm = gamma.double() if gamma is not None else 1.0
    bt = beta.double() if beta is not None else 0.0
    out = {"scale": gm * rstd, "shift": bt - mean * gm * rstd, "mean": mean, "rstd": rstd, "var_raw": var_raw}
    if rmean is not None:
        unbiased = var * count / (count - 1.0) if count > 1 else var
        out["running_mean"] = (1 - momentum) * rmean.double() + momentum * mean
        out["running_var"] = (1 - momentum) * rvar.double() + momentum * unbiased
    return out


def ref_bn_bwd_finalize(pdz, pdzx, count, scale=None, shift=None, gamma=None, mean=None, rstd=None):
    """mdz = sum pdz / count, mdzx = sum pdzx / count, dbeta = sum pdz, dgamma = sum pdzx; with the BN vectors also
    consts [5, C] = [scale, shift, k1, k2, k0]."""
    a, b = pdz.double().sum(0), pdzx.double().sum(0)
    out = {"mdz": a / count, "mdzx": b / count, "dgamma": b, "dbeta": a}
    if scale is not None:
        k1, k2, k0 = bwd_consts(mean, rstd, gamma, out["mdz"], out["mdzx"])
        out["consts"] = torch.stack([scale.double(), shift.double(), k1, k2, k0])
    return out


# ---- assertions ------------------------------------------------------------------------------------------------------
def bf16_ulp(ref):
    """Spacing of bf16 (8 significant bits) at |ref|."""
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** -126))     # |ref| = m * 2^e with m in [0.5, 1)
    return torch.pow(2.0, (e - 8).double())


class Bf16Check:
    """assert_bf16_exact over one tensor or, through repeated add(), over a tensor taken a few frames at a time."""

    def __init__(self, name):
        self.name = name
        self.worst, self.where = 0.0, None
        self.ulp_sum, self.count, self.elements = 0.0, 0, 0

    def add(self, out, ref, S, n0=0):
        assert out.dtype == BF and ref.dtype == torch.float64 and out.shape == ref.shape == S.shape, self.name
        o = out.double()
        bad = ~torch.isfinite(o)
        if bad.any():
            idx = self._index(bad.reshape(-1).to(torch.uint8).argmax().item(), out.shape, n0)
            raise AssertionError(f"{self.name}: non-finite output at (n, row, channel) = {idx}")
        err = (o - ref).abs()
        bound = REL * ref.abs() + SLACK * S
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                            torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        m, i = ratio.reshape(-1).max(0)
        if m.item() > self.worst:
            i = i.item()
            self.worst = m.item()
            self.where = (self._index(i, out.shape, n0), o.reshape(-1)[i].item(), ref.reshape(-1)[i].item(),
                          bound.reshape(-1)[i].item())
        q = ref.abs() > BIAS_FLOOR * S
        signed = torch.sign(ref) * (o - ref) / bf16_ulp(ref)
        self.ulp_sum += signed[q].sum().item()
        self.count += int(q.sum().item())
        self.elements += out.numel()

    @staticmethod
    def _index(flat, shape, n0):
        idx = []
        for d in reversed(shape):
            idx.append(flat % d)
            flat //= d
        idx = idx[::-1]
        idx[0] += n0
        return tuple(idx)

    @property
    def mean_ulp(self):
        return self.ulp_sum / self.count if self.count else 0.0

    def finish(self):
        if self.worst > 1.0:
            idx, o, r, b = self.where
            raise AssertionError(f"{self.name}: |out - ref| = {abs(o - r):.6g} is {self.worst:.3f} x the bound "
                                 f"{b:.6g} at (n, row, channel) = {idx}: out {o!r}, ref {r!r}")
        if self.count >= BIAS_MIN_COUNT and abs(self.mean_ulp) > BIAS_CAP:
            raise AssertionError(f"{self.name}: mean signed error {self.mean_ulp:+.4f} bf16 ulp over {self.count} "
                                 f"elements (cap {BIAS_CAP}): the stores are biased")
        return {"worst": self.worst, "mean_ulp": self.mean_ulp, "count": self.count, "elements": self.elements}


def assert_bf16_exact(out, ref, S, name):
    """out (bf16) is ref (fp64) computed in fp32 and stored round-to-nearest: element-wise
    |out - ref| <= 2^-8 |ref| + 2^-16 S, no bias of the stores, nothing non-finite.  Returns the observed figures."""
    chk = Bf16Check(name)
    chk.add(out, ref, S)
    return chk.finish()


def assert_sum_close(a, ref, name):
    """Tolerance of tests/test_frame_gpu._close."""
    scale = ref.abs().max().item() + 1e-12
    torch.testing.assert_close(a.double(), ref, rtol=1e-4, atol=2e-5 * scale, msg=lambda m: f"{name}: {m}")


def frob(out, ref):
    """Relative Frobenius error, the metric of the older tests."""
    return ((out.double() - ref).norm() / ref.norm().clamp_min(1e-300)).item()
