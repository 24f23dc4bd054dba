"""The TokenLearner oracle can fail (CPU).  tokenlearner.hip's arithmetic is emulated in fp32 torch (bf16 LN operand,
32-wide fp32 chunks, bf16 z1 / dz1 / out / dx / xn stores, the same stored intermediates); the clean emulation passes
every check of tests/tl_oracle.py, the element caps of the rebuilt-operand z1 included, and every planted fault is
caught.  For each fault OLD records whether the relative Frobenius assertions of tests/test_kernels_gpu.py::
test_token_learner_kernels_match_eager (out 1e-2, dx 2e-2, parameter gradients 3e-2 against the unrounded chain) would
have seen it on the same data, and the test asserts that record."""
import pytest
import torch

import gemm_oracle as gm
import glue_oracle as go
import tl_oracle as tlo

BF = torch.bfloat16
OLD_FWD, OLD_DX, OLD_PARAM = 1e-2, 2e-2, 3e-2
C, H1, T = tlo.C, tlo.H1, tlo.T


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31)
    return torch.Generator(device="cpu").manual_seed(seed)


def chunked(a, b, width=32):
    acc = torch.zeros(*a.shape[:-1], b.shape[-1], dtype=torch.float32)
    for k0 in range(0, a.shape[-1], width):
        acc = acc + a[..., k0:k0 + width] @ b[..., k0:k0 + width, :]
    return acc


def truncate(x):
    return (x.float().view(torch.int32) & -65536).view(torch.float32).to(BF)


def gelu_parts(z):
    th = torch.tanh(tlo.K0 * (z + tlo.K1 * z * z * z))
    return 0.5 * z * (1 + th), 0.5 * (1 + th) + 0.5 * z * (1 - th * th) * tlo.K0 * (1 + 3 * tlo.K1 * z * z)


def emu_fwd(d, fault=None):
    x = d["x"].float()
    N, P, _ = x.shape
    mu = x.sum(-1) / C
    xc = x if fault == "uncentred" else x - mu[..., None]
    rs = torch.rsqrt((xc * xc).sum(-1) / C + d["eps"])
    a = ((x - mu[..., None]) * rs[..., None] * d["gamma"] + d["beta"]).to(BF).float()
    acc = chunked(a, d["W1"].float().t()) + d["b1"]
    z1 = truncate(acc) if fault == "z1_trunc" else acc.to(BF)
    logits = gelu_parts(z1.float())[0] @ d["W2"].t() + d["b2"]                   # [N, P, 8]
    if fault == "softmax_pad":                                                  # positions P .. 64-lane end join in
        pad = torch.zeros(N, (P + 63) // 64 * 64 - P, T)
        e = torch.exp(torch.cat([logits, pad], 1) - torch.cat([logits, pad], 1).amax(1, keepdim=True))
        s = (e / e.sum(1, keepdim=True))[:, :P]
    else:
        e = torch.exp(logits - logits.amax(1, keepdim=True))
        s = e / e.sum(1, keepdim=True)
    s = s.transpose(1, 2).contiguous()
    return (s @ x).to(BF), mu, rs, z1, s


def emu_bwd(d, fw, fault=None):
    _, mu, rs, z1, s = fw
    x, dO = d["x"].float(), d["dO"].float()
    N, P, _ = x.shape
    dS = chunked(dO, x.transpose(1, 2))
    dot = (s * dS).sum(-1, keepdim=True)
    if fault == "dot_wrong_token":
        dot = dot.roll(1, 1)
    da = s * (dS - dot)
    hz, gd = gelu_parts(z1.float())
    dz1 = ((da.transpose(1, 2) @ d["W2"]) * gd).to(BF)
    pw2 = da @ torch.cat([hz, torch.ones(N, P, 1)], -1)
    W1 = d["W1"].float()
    dd = dz1.float() @ W1
    if fault == "w1_half":
        dd[..., C // 2:] = dz1.float() @ W1[:, :C // 2]
    r = rs[..., None]
    xh = (x - mu[..., None]) * r
    g = dd * d["gamma"]
    sg, sgx = g.sum(-1, keepdim=True) / C, (g * xh).sum(-1, keepdim=True) / C
    st = s.clone()
    if fault == "pool_last_token":
        st[:, T - 1] = 0.0
    dx = (r * (g - sg - xh * sgx) + st.transpose(1, 2) @ dO).to(BF)
    xn = (xh * d["gamma"] + d["beta"]).to(BF)
    dg, db = (dd * xh).sum(1), dd.sum(1)
    if fault == "dgamma_pad" and P % 16:                                        # the rows P .. of the last block count
        k = 16 - P % 16
        dg = dg + k * dd[:, 0] * xh[:, P - 1]
        db = db + k * dd[:, 0]
    return dx, dz1.reshape(N * P, H1), xn.reshape(N * P, C), pw2, torch.stack([dg, db], 1)


def run_checks(d, fw, bw, name):
    st = tlo.check_fwd(d["x"], d["gamma"], d["beta"], d["eps"], d["W1"], d["b1"], d["W2"], d["b2"], fw, name)
    _, mu, rs, z1, s = fw
    return st, tlo.check_bwd(d["x"], d["dO"], s, z1, mu, rs, d["gamma"], d["beta"], d["W1"], d["W2"], bw, name)


@pytest.mark.parametrize("kind", ["normal", "onehot", "flat"])
@pytest.mark.parametrize("N,P", [(2, 1), (2, 15), (3, 17), (2, 100), (1, 129), (2, 256)])
def test_clean_emulation_passes(N, P, kind):
    d = tlo.make_inputs(N, P, gen(N, P, len(kind)), kind=kind)
    fw = emu_fwd(d)
    sf, sb = run_checks(d, fw, emu_bwd(d, fw), f"clean N{N} P{P} {kind}")
    assert sf["worst_hard"] <= 1.0 and sb["worst_hard"] <= 1.0
    s = fw[4]
    if kind == "onehot" and P >= 100:
        assert s.amax(-1).max() > 0.5, "the near-one-hot case is not peaked"
    if kind == "flat" and P > 1:
        assert (s.amax(-1) / s.amin(-1)).max() < 1.01, "the flat case is not flat"


def chain(d):
    """The unrounded fp64 chain (what the eager module computes): out, dx, dW2 | db2 summed over frames, dgamma, dbeta."""
    x = d["x"].double()
    mu = x.mean(-1)
    rs = 1.0 / torch.sqrt(((x - mu[..., None]) ** 2).mean(-1) + d["eps"])
    _, v, _ = tlo.operand_ln(x, mu, rs, d["gamma"], d["beta"])
    z1 = v @ d["W1"].double().t() + d["b1"].double()
    s = tlo.ref_softmax(z1, d["W2"], d["b2"])[0]
    hd = tlo.ref_bwd_head(x, d["dO"], s, z1, d["W2"])
    t = tlo.ref_bwd_tail(x, d["dO"], s, hd["dz1"], mu, rs, d["gamma"], d["beta"], d["W1"])
    return {"out": s @ x, "dx": t["dx"], "dW2": hd["pw2"].sum(0)[:, :H1], "pg": t["pg"].sum(0)}


def old_sees(d, fw, bw):
    r = chain(d)
    return (go.frob(fw[0], r["out"]) > OLD_FWD or go.frob(bw[0], r["dx"]) > OLD_DX
            or go.frob(bw[3].sum(0)[:, :H1], r["dW2"]) > OLD_PARAM or go.frob(bw[4].sum(0)[0], r["pg"][0]) > OLD_PARAM
            or go.frob(bw[4].sum(0)[1], r["pg"][1]) > OLD_PARAM)


# fault -> (forward fault?, (N, P), seen by the old Frobenius assertions on this data?)
FAULTS = {"softmax_pad": (True, (2, 100), True), "uncentred": (True, (2, 100), True),
          "z1_trunc": (True, (8, 225), False), "pool_last_token": (False, (2, 100), True),
          "dgamma_pad": (False, (2, 100), True), "w1_half": (False, (2, 100), True),
          "dot_wrong_token": (False, (2, 100), True)}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_fault_is_caught(fault):
    fwd, (N, P), OLD = FAULTS[fault]
    d = tlo.make_inputs(N, P, gen(N, P, 6))
    fw = emu_fwd(d, fault if fwd else None)
    bw = emu_bwd(d, fw, None if fwd else fault)
    with pytest.raises(AssertionError):
        run_checks(d, fw, bw, fault)
    assert old_sees(d, fw, bw) == OLD, f"{fault}: the old assertions {'miss' if OLD else 'see'} it on this data"
    clean = emu_fwd(d)
    assert not old_sees(d, clean, emu_bwd(d, clean)), "the old assertions fail the clean emulation"


def test_truncated_z1_is_caught_by_the_bias_statistic():
    N, P = FAULTS["z1_trunc"][1]
    d = tlo.make_inputs(N, P, gen(N, P, 6))
    fw = emu_fwd(d, "z1_trunc")
    with pytest.raises(AssertionError, match=" z1"):
        tlo.check_fwd(d["x"], d["gamma"], d["beta"], d["eps"], d["W1"], d["b1"], d["W2"], d["b2"], fw, "trunc")
    # the statistic on its own: a truncating store shifts the mean signed error by about -0.5 ulp
    aq = tlo.operand_ln(d["x"], fw[1], fw[2], d["gamma"], d["beta"])[0].reshape(N * P, C)
    ref, S = gm.ref_gemm(aq, d["W1"], bias=d["b1"])
    chk = gm.GemmCheck("trunc", C + 1, C)
    chk.add(fw[3].reshape(N * P, H1), ref, S)
    assert chk.count >= go.BIAS_MIN_COUNT and chk.mean_ulp < -0.25 and abs(chk.mean_ulp) > go.BIAS_CAP
    clean = emu_fwd(d)
    st = tlo.check_fwd(d["x"], d["gamma"], d["beta"], d["eps"], d["W1"], d["b1"], d["W2"], d["b2"], clean, "clean")
    assert st["count"] >= go.BIAS_MIN_COUNT, "the case is too small for the bias statistic"
    assert st["z1_share"] <= max(2 * H1 / (N * P * H1), gm.CAP)


def test_p_257_is_outside_the_templates():
    assert tlo.bwd_template(128) == 128 and tlo.bwd_template(129) == 256 and tlo.PMAX == 256
