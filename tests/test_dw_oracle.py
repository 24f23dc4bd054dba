"""The depthwise oracle (tests/dw_oracle.py) can fail: an fp32 emulation of each depthwise operation on the CPU (fp32
prologue, bf16 operand, fp32 tap sum, bf16 store) passes it clean -- worst ratio <= 1 against the hard bound, shares
outside tight inside their caps -- and is caught with each of eight planted faults:

  1 trunc    truncating bf16 store
  2 ring     padding ring filled before the BN+SiLU prologue (silu(shift) instead of 0)
  3 flip     one channel with flipped taps: the forward convolved with the data-gradient taps, the data gradient with
             unflipped taps (also on the rebuilt-dy route, where only the per-channel count and the hard bound see it)
  4 tail     the last channel vector of a short chunk (C = 152: chunks of 5, 5, 5, 4 vectors) left unwritten in a frame
  5 seam     one row at a tile seam taken from the neighbouring tile's row
  6 lastcol  the last output column missing its rightmost tap column (k3 at stride 2 on an even map: at stride 1, and
             for k5 at any width, that tap column is padding)
  7 parity   at stride 2, the two column parity classes of one data-gradient row swapped
  8 drop     one pixel of average size dropped from one channel's partial sum

The truncating store (Frobenius error 0.003) and the ring fault on a wide N = 1 map are asserted to stay below the 1e-2
that the older kernel tests accept.  Run with -s for the table: fault, Frobenius error, worst ratio to tight / hard,
share outside tight, verdict."""
import pytest
import torch

import dw_oracle as do
import glue_oracle as go

BF = torch.bfloat16
A = (4, 21, 22, 152)         # 281 k elements: the bias statistic is live; N*H*W = 1848 <= 8192 for the sums
B = (2, 20, 30, 144)         # stride 2, even map
RING = (1, 160, 640, 16)     # border pixels are 1.6 % of the map: the ring fault's Frobenius error falls below 1e-2
TILE_H, TILE_W = 8, 12       # the emulated tile seam of fault 5


def _inputs(shape, k, s, seed=77):
    return do.make_inputs(*shape, k, s, seed, "cpu")


# ---- fp32 emulation --------------------------------------------------------------------------------------------------
def _store(o, fault):
    if fault == "trunc":
        return (o.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32).to(BF)
    return o.to(BF)


def _silu32(x, sc, sh):
    z = x.float() * sc + sh
    return z * torch.sigmoid(z)


def _silu_grad32(x, sc, sh):
    z = x.float() * sc + sh
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def _pad32(a, p, fill=None):
    N, H, W, C = a.shape
    out = torch.zeros(N, H + 2 * p, W + 2 * p, C) if fill is None else fill.expand(N, H + 2 * p, W + 2 * p, C).clone()
    out[:, p:p + H, p:p + W] = a
    return out


def _fwd32(ap, w, k, s, Ho, Wo, lastcol=False):
    out = torch.zeros(ap.shape[0], Ho, Wo, ap.shape[3])
    for kh in range(k):
        for kw in range(k):
            term = w[:, kh * k + kw] * ap[:, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s]
            if lastcol and kw == k - 1:
                term[:, :, -1] = 0
            out += term
    return out


def _bwd32(g, w, H, W, k, s):
    N, Ho, Wo, C = g.shape
    p = (k - 1) // 2
    dp = torch.zeros(N, H + 2 * p, W + 2 * p, C)
    for kh in range(k):
        for kw in range(k):
            dp[:, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s] += w[:, kh * k + kw] * g
    return dp[:, p:p + H, p:p + W].contiguous()


def _taps(w, fault):
    if fault == "flip":
        w = w.clone()
        w[5] = w[5].flip(0)
    return w


def _spoil(out, fault):
    """Faults planted on the finished output."""
    if fault == "tail":
        out[0, :, :, -8:] = 0                                        # frame 0, the 4th vector of the 4-vector chunk
    if fault == "seam":
        out[1, TILE_H, TILE_W:2 * TILE_W] = out[1, TILE_H - 1, TILE_W:2 * TILE_W]
    if fault == "parity":
        row = out[1, 7].clone()
        out[1, 7, 0::2], out[1, 7, 1::2] = row[1::2], row[0::2]
    return out


def emu_fwd(d, k, s, pro, fault=None):
    x = d["x"]
    p = (k - 1) // 2
    if pro and fault == "ring":
        ap = _silu32(_pad32(x.float(), p), d["sc1"], d["sh1"]).to(BF).float()
    elif pro:
        ap = _pad32(_silu32(x, d["sc1"], d["sh1"]).to(BF).float(), p)
    else:
        ap = _pad32(x.float(), p)
    Ho, Wo = do.out_hw(x.shape[1], x.shape[2], k, s)
    return _spoil(_store(_fwd32(ap, _taps(d["w"], fault), k, s, Ho, Wo, fault == "lastcol"), fault), fault)


def _dy32(d):
    """stage_dy_v2's chain: a = k1 gate, b = k1 rb folded per frame, dy = silu'(z) (a dA + b) + (k2 y + k0)."""
    k1 = d["g2"] * d["rs2"]
    a, b = (d["gate"] * k1)[:, None, None, :], (d["rb"] * k1)[:, None, None, :]
    k2 = -k1 * d["rs2"] * d["mdzx2"]
    k0 = -k1 * (d["mdz2"] - d["mu2"] * d["rs2"] * d["mdzx2"])
    y = d["y2"].float()
    return (_silu_grad32(d["y2"], d["sc2"], d["sh2"]) * (a * d["dA"].float() + b) + (k2 * y + k0)).to(BF).float()


def emu_bwd_data(d, k, s, rebuilt, fault=None, zout=False):
    N, H, W, C = d["x"].shape
    g = _dy32(d) if rebuilt else d["g"].float()
    dx = _bwd32(g, _taps(d["w"], fault), H, W, k, s)
    if zout:
        dx = dx * _silu_grad32(d["x"], d["sc1"], d["sh1"])
    return _spoil(_store(dx, fault), fault)


def emu_bwd_weight(d, k, s, pro, rebuilt, round_a=True):
    x = d["x"]
    a = _silu32(x, d["sc1"], d["sh1"]) if pro else x.float()
    if round_a:
        a = a.to(BF).float()
    g = _dy32(d) if rebuilt else d["g"].float()
    N, Ho, Wo, C = g.shape
    ap = _pad32(a, (k - 1) // 2)
    return torch.stack([(g * ap[:, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s]).sum((0, 1, 2))
                        for kh in range(k) for kw in range(k)], 1)


def emu_bn_partials(stored, d, zout=False):
    dz = stored.float()
    if not zout:
        dz = dz * _silu_grad32(d["x"], d["sc1"], d["sh1"])
    xhat = d["x"].float() * d["rs1"] + (-d["mu1"] * d["rs1"])
    return dz.sum((0, 1, 2)), (dz * xhat).sum((0, 1, 2))


# ---- references ------------------------------------------------------------------------------------------------------
def _a_op(d, pro, round=True):
    return do.operand_bn_silu(d["x"], d["sc1"], d["sh1"], round) if pro else do.operand_raw(d["x"])


def ref_fwd(d, k, s, pro):
    op = _a_op(d, pro)
    ref, S = do.ref_fwd(op, d["w"], k, s)
    return ref, S, do.flip_fwd(op, d["w"], k, s), (do.CAP_PROLOGUE if pro else 0.0)


def ref_bwd_data(d, k, s, rebuilt, zout=False):
    N, H, W, C = d["x"].shape
    op = do.operand_dy(d) if rebuilt else do.operand_raw(d["g"])
    ref, S = do.ref_bwd_data(op, d["w"], H, W, k, s)
    F = do.flip_bwd_data(op, d["w"], H, W, k, s)
    if zout:
        sg = do.silu_grad(d["x"], d["sc1"], d["sh1"])
        ref, S, F = ref * sg, S * do.silu_grad_abs(d["x"], d["sc1"], d["sh1"]), F * sg.abs()
    return ref, S, F, (do.CAP_DY if rebuilt else do.CAP_PROLOGUE if zout else 0.0)


def _figures(out, ref, S, F, cap):
    chk = do.DwCheck("figures", cap)
    chk.add(out, ref, S, F)
    return chk.worst, (chk.worst_hard if cap > 0 else chk.worst), chk.share


ROWS = []


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\ndw oracle | operation                | fault   | frobenius | worst/tight | worst/hard | share outside | verdict")
    for r in ROWS:
        print(r)


def _report(op, fault, out, ref, S, F, cap, verdict):
    wt, wh, share = _figures(out, ref, S, F, cap)
    fro = go.frob(out, ref)
    ROWS.append(f"dw oracle | {op:24s} | {fault or 'clean':7s} | {fro:9.5f} | {wt:11.3f} | {wh:10.3f} | {share:13.3g} | "
                f"{verdict}")
    return fro


# name -> (shape, k, s, emulation(d, fault), reference(d))
OPS = {
    "fwd k3 s1":            (A, 3, 1, lambda d, f: emu_fwd(d, 3, 1, False, f), lambda d: ref_fwd(d, 3, 1, False)),
    "fwd k3 s1 bn+silu":    (A, 3, 1, lambda d, f: emu_fwd(d, 3, 1, True, f), lambda d: ref_fwd(d, 3, 1, True)),
    "fwd k5 s1 bn+silu":    (A, 5, 1, lambda d, f: emu_fwd(d, 5, 1, True, f), lambda d: ref_fwd(d, 5, 1, True)),
    "fwd k3 s2":            (B, 3, 2, lambda d, f: emu_fwd(d, 3, 2, False, f), lambda d: ref_fwd(d, 3, 2, False)),
    "fwd k5 s2 bn+silu":    (B, 5, 2, lambda d, f: emu_fwd(d, 5, 2, True, f), lambda d: ref_fwd(d, 5, 2, True)),
    "fwd ring map bn+silu": (RING, 3, 1, lambda d, f: emu_fwd(d, 3, 1, True, f), lambda d: ref_fwd(d, 3, 1, True)),
    "bwd_data k3 s1":       (A, 3, 1, lambda d, f: emu_bwd_data(d, 3, 1, False, f), lambda d: ref_bwd_data(d, 3, 1, False)),
    "bwd_data k5 s1":       (A, 5, 1, lambda d, f: emu_bwd_data(d, 5, 1, False, f), lambda d: ref_bwd_data(d, 5, 1, False)),
    "bwd_data k3 s2":       (B, 3, 2, lambda d, f: emu_bwd_data(d, 3, 2, False, f), lambda d: ref_bwd_data(d, 3, 2, False)),
    "bwd_data k5 s2":       (B, 5, 2, lambda d, f: emu_bwd_data(d, 5, 2, False, f), lambda d: ref_bwd_data(d, 5, 2, False)),
    "fused dx k3 s1":       (A, 3, 1, lambda d, f: emu_bwd_data(d, 3, 1, True, f), lambda d: ref_bwd_data(d, 3, 1, True)),
    "fused dx k5 s2":       (B, 5, 2, lambda d, f: emu_bwd_data(d, 5, 2, True, f), lambda d: ref_bwd_data(d, 5, 2, True)),
    "fused dz k5 s1 zout":  (A, 5, 1, lambda d, f: emu_bwd_data(d, 5, 1, True, f, True),
                             lambda d: ref_bwd_data(d, 5, 1, True, True)),
}
FAULTS = [("trunc", "fwd k3 s1"), ("trunc", "fwd k3 s1 bn+silu"), ("trunc", "fused dx k3 s1"),
          ("ring", "fwd ring map bn+silu"), ("ring", "fwd k3 s1 bn+silu"),
          ("flip", "fwd k3 s1"), ("flip", "fwd k5 s1 bn+silu"), ("flip", "bwd_data k3 s1"), ("flip", "bwd_data k5 s2"),
          ("flip", "fused dx k3 s1"), ("flip", "fused dz k5 s1 zout"),
          ("tail", "fwd k3 s1"), ("tail", "fwd k5 s1 bn+silu"), ("tail", "bwd_data k3 s1"), ("tail", "fused dx k3 s1"),
          ("seam", "fwd k3 s1"), ("seam", "fwd k3 s1 bn+silu"), ("seam", "bwd_data k5 s1"), ("seam", "fused dx k3 s1"),
          ("lastcol", "fwd k3 s2"),
          ("parity", "bwd_data k3 s2"), ("parity", "bwd_data k5 s2"), ("parity", "fused dx k5 s2")]


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(op):
        if op not in cache:
            shape, k, s, emu, ref = OPS[op]
            d = _inputs(shape, k, s)
            cache[op] = (d, emu, ref(d))
        return cache[op]
    return get


@pytest.mark.parametrize("op", list(OPS))
def test_clean_emulation_passes(cases, op):
    d, emu, (ref, S, F, cap) = cases(op)
    out = emu(d, None)
    st = do.assert_dw(out, ref, S, op, cap, F, OPS[op][1] ** 2)
    assert st["worst_hard"] <= 1.0 and st["share"] <= cap
    if OPS[op][0] in (A, RING):
        assert st["count"] >= go.BIAS_MIN_COUNT          # the bias assertion was not skipped
    _report(op, None, out, ref, S, F, cap, "passes")


@pytest.mark.parametrize("fault,op", FAULTS)
def test_planted_fault_is_caught(cases, fault, op):
    d, emu, (ref, S, F, cap) = cases(op)
    out = emu(d, fault)
    with pytest.raises(AssertionError) as e:
        do.assert_dw(out, ref, S, op, cap, F, OPS[op][1] ** 2)
    fro = _report(op, fault, out, ref, S, F, cap, "caught: " + str(e.value)[:100])
    if fault == "trunc" or (fault == "ring" and OPS[op][0] == RING):
        assert fro < 1e-2       # the Frobenius check of the older tests lets these through


# ---- sums ------------------------------------------------------------------------------------------------------------
def _avg_pixel(stored, c):
    """The pixel of channel c whose |value| is closest to the channel's mean |value|."""
    v = stored[..., c].double().abs()
    i = (v - v.mean()).abs().reshape(-1).argmin().item()
    return do.DwCheck._index(i, v.shape, 0)


def test_sums_clean_and_dropped_pixel(cases):
    """Fault 8 on the forward statistics and on the BN1 partials; the clean fp32 sums pass.  N*Ho*Wo = 1848 <= 8192: an
    average term is 1 / 1848 of sum|term|, 35 times the bound."""
    d, emu, _ = cases("fwd k3 s1 bn+silu")
    out = emu(d, None)
    assert out.shape[0] * out.shape[1] * out.shape[2] <= 8192
    of = out.float()
    (rs, ra), (rq, rqa) = do.ref_stats(out)
    ps, pq = of.sum((0, 1, 2)), (of * of).sum((0, 1, 2))
    m1 = do.assert_sums(ps, rs, ra, "ps")
    m2 = do.assert_sums(pq, rq, rqa, "pq")
    n, h, w = _avg_pixel(out, 9)
    bad_s, bad_q = ps.clone(), pq.clone()
    bad_s[9] -= of[n, h, w, 9]
    bad_q[9] -= of[n, h, w, 9] ** 2
    with pytest.raises(AssertionError, match=r"\(9,\)"):
        do.assert_sums(bad_s, rs, ra, "ps")
    with pytest.raises(AssertionError, match=r"\(9,\)"):
        do.assert_sums(bad_q, rq, rqa, "pq")
    ROWS.append(f"dw oracle | sums ps / pq: clean worst ratio {max(m1, m2):.3f}; one dropped pixel of channel 9: "
                f"{do.sum_ratio(bad_s, rs, ra)[0]:.1f} / {do.sum_ratio(bad_q, rq, rqa)[0]:.1f} x the bound, caught")
    # BN1 partials of the data gradient with its epilogue, from the stored dx
    d, emu, _ = cases("bwd_data k3 s1")
    dx = emu(d, None)
    for zout in (False, True):
        pdz, pdzx = emu_bn_partials(dx, d, zout)
        (r1, a1), (r2, a2) = do.ref_bn_partials(dx, d["x"], d["sc1"], d["sh1"], d["mu1"], d["rs1"], zout)
        m = max(do.assert_sums(pdz, r1, a1, "pdz"), do.assert_sums(pdzx, r2, a2, "pdzx"))
        n, h, w = _avg_pixel(dx, 100)
        bad = pdz.clone()
        bad[100] -= (dx[n, h, w, 100].float() * (1.0 if zout else _silu_grad32(d["x"], d["sc1"], d["sh1"])[n, h, w, 100]))
        with pytest.raises(AssertionError, match=r"\(100,\)"):
            do.assert_sums(bad, r1, a1, "pdz")
        ROWS.append(f"dw oracle | sums pdz / pdzx zout={zout}: clean worst ratio {m:.3f}; one dropped pixel of channel "
                    f"100: {do.sum_ratio(bad, r1, a1)[0]:.1f} x the bound, caught")


@pytest.mark.parametrize("k,s,pro,rebuilt,round_a", [(3, 1, False, False, True), (5, 1, True, False, True),
                                                     (3, 1, True, True, True), (5, 1, True, True, False),
                                                     (3, 2, True, True, False), (5, 2, False, False, True)])
def test_weight_gradient_clean_and_dropped_pixel(k, s, pro, rebuilt, round_a):
    """The weight gradient is a sum over N*Ho*Wo <= 8192 terms per (channel, tap); round_a=False is the unified kernels'
    fp32 silu operand.  A clean fp32 sum passes; dropping one average term is caught."""
    shape = A if s == 1 else B
    d = _inputs(shape, k, s)
    dw = emu_bwd_weight(d, k, s, pro, rebuilt, round_a)
    gop = do.operand_dy(d) if rebuilt else do.operand_raw(d["g"])
    ref, sab, mab = do.ref_bwd_weight(gop, _a_op(d, pro, round_a), k, s)
    assert gop[0].shape[0] * gop[0].shape[1] * gop[0].shape[2] <= 8192
    rounded = pro or rebuilt
    m = do.assert_sums(dw, ref, sab, "dw", mab if rounded else None)
    terms = gop[0].shape[0] * gop[0].shape[1] * gop[0].shape[2]
    bad = dw.clone()
    bad[11, 4] -= (sab[11, 4] / terms).float()          # one term of average size
    with pytest.raises(AssertionError, match=r"\(11, 4\)"):
        do.assert_sums(bad, ref, sab, "dw", mab if rounded else None)
    ROWS.append(f"dw oracle | dw k{k} s{s} pro={pro} dy rebuilt={rebuilt} round_a={round_a}: clean worst ratio {m:.3f}; "
                f"one dropped term: {do.sum_ratio(bad, ref, sab, mab if rounded else None)[0]:.1f} x the bound, caught")


def test_unrounded_silu_operand_matters():
    """The reference must know which kernels round a = silu(bn1(x1)) before the weight product: an fp32 sum over the
    unrounded operand misses the bf16-operand reference."""
    d = _inputs(A, 3, 1)
    dw = emu_bwd_weight(d, 3, 1, True, False, round_a=False)
    ref, sab, mab = do.ref_bwd_weight(do.operand_raw(d["g"]), _a_op(d, True, True), 3, 1)
    with pytest.raises(AssertionError):
        do.assert_sums(dw, ref, sab, "dw", mab)


def test_failure_names_the_element(cases):
    d, emu, (ref, S, F, cap) = cases("fwd k3 s1")
    out = emu(d, None)
    out[2, 13, 7, 77] = out[2, 13, 7, 77].float() * 1.02
    with pytest.raises(AssertionError, match=r"\(2, 13, 7, 77\).*out .*ref "):
        do.assert_dw(out, ref, S, "fwd", cap, F)
    out[0, 3, 9, 1] = float("nan")
    with pytest.raises(AssertionError, match=r"non-finite.*\(0, 3, 9, 1\)"):
        do.assert_dw(out, ref, S, "fwd", cap, F)


def test_per_channel_cap_sees_one_channel():
    """40 elements of one channel of 816 one bf16 ulp off: inside the hard bound and the global share (cap 2^-10 of
    163 200 = 159), over the channel's allowance of 9 * max(2, 16 * 2^-10 * 200 = 3.1) = 28."""
    d = _inputs((2, 10, 10, 816), 3, 1)
    ref, S, F, cap = ref_bwd_data(d, 3, 1, True)
    out = emu_bwd_data(d, 3, 1, True)
    do.assert_dw(out, ref, S, "fused dx", cap, F, 9)
    c = out[..., 33].contiguous()
    up, dn = (c.view(torch.int16) + 1).view(BF), (c.view(torch.int16) - 1).view(BF)
    r = ref[..., 33]
    far = torch.where((up.double() - r).abs() > (dn.double() - r).abs(), up, dn)       # the farther bf16 neighbour
    err = (far.double() - r).abs()
    tight = go.REL * r.abs() + go.SLACK * S[..., 33]
    pick = ((err > 1.1 * tight) & (err < 0.95 * (tight + do.FLIP * F[..., 33]))).reshape(-1).nonzero().reshape(-1)[:40]
    assert len(pick) == 40
    for i in pick.tolist():
        n, h, w = do.DwCheck._index(i, r.shape, 0)
        out[n, h, w, 33] = far[n, h, w]
    with pytest.raises(AssertionError, match="channel 33"):
        do.assert_dw(out, ref, S, "fused dx", cap, F, 9)
