"""The GEMM oracle (tests/gemm_oracle.py) can fail: fp32-math (32-wide K chunks, 64-row M chunks), bf16-store emulations
of a plain product, a two-segment product with a residual, a prologue product, statistics partials and a split weight
gradient pass it clean on the CPU and are caught with each of ten planted faults.

What the older Frobenius thresholds let through, computed here and asserted:
  * (a) a truncating bf16 store is Frobenius 0.003 (< 6e-3);
  * (c) one output row left at zero in M = 60161 rows is 0.0050: sqrt(1 / M) = 0.0041 on top of the 0.0017 of the
    roundings; sqrt(2 / M) = 0.0058 were the row garbage of the same magnitude.  Both < 6e-3, which needs
    M > 2 / 6e-3^2 = 55,556;
  * (e) the rmul row of the next frame over the last 3 rows of one frame is 0.0023 at M = 121,200 and 0.00167 at
    M = 2000, where the clean emulation has 0.00164: it cannot be told from the roundings at any shape;
  * (h) moves one tile's partial row into its neighbour: the column sums the older tests compare are unchanged.

Run with -s to see the table: fault, Frobenius error, worst err/bound, mean signed ulp error, verdict."""
import pytest
import torch

import gemm_oracle as gm
import glue_oracle as go

BF = torch.bfloat16
M, K, N, K2, HW = 2000, 264, 136, 40, 100          # K = 8 x 32 + 8: a K tail of 8; M = 31 x 64 + 16: a partial strip
STRIP = 64
OLD = 6e-3                                          # the relative Frobenius threshold of test_pwgemm_gpu.py


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


@pytest.fixture(scope="module")
def inp():
    g = _gen(20250)
    d = {"a": gm.acts(M, K, g), "w": gm.weight(N, K, g, K ** -0.5), "a2": gm.acts(M, K2, g),
         "w2": gm.weight(N, K2, g, K2 ** -0.5), "bias": torch.randn(N, generator=g),
         "res": gm.acts(M, N, g, 0.2, 1.3), "rmul": torch.rand(M // HW, N, generator=g) + 0.5,
         "y": gm.acts(M, K, g, 0.2, 1.3), "scale": torch.rand(K, generator=g) + 0.5,
         "shift": torch.randn(K, generator=g) * 0.2, "gate": torch.rand(M // HW, K, generator=g)}
    return d


def _store(acc, fault):
    if fault == "trunc":
        return (acc.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32).to(BF)
    return acc.to(BF)


def _mm(a, w, fault=None):
    """fp32 accumulation over 32-wide K chunks; (b) drops the last 8 columns of the K tail."""
    k = a.shape[1] - (8 if fault == "ktail" else 0)
    acc = torch.zeros(a.shape[0], w.shape[0])
    for c in range(0, k, 32):
        acc = acc + a[:, c:min(c + 32, k)].float() @ w[:, c:min(c + 32, k)].float().t()
    return acc


def _frame_rows(t, rows, hw, fault):
    """t[m / hw]; (e) the last 3 rows of frame 7 read frame 8's row."""
    fr = torch.arange(rows) // hw
    if fault == "frame":
        fr[8 * hw - 3:8 * hw] = 8
    return t[fr]


def _finish(acc, fault):
    out = _store(acc, fault)
    if fault == "strip":                                   # (c) the last partial row strip left at zero
        out[out.shape[0] // STRIP * STRIP:] = 0
    if fault == "swap":                                    # (d) two 4-column output groups swapped
        out[:, 8:12], out[:, 12:16] = out[:, 12:16].clone(), out[:, 8:12].clone()
    return out


def emu_plain(d, fault=None):
    return _finish(_mm(d["a"], d["w"], fault), fault)


def emu_tail(d, fault=None):
    acc = _mm(d["a"], d["w"], fault)
    if fault != "seg2":                                    # (g) the second segment skipped
        acc = acc + _mm(d["a2"], d["w2"])
    acc = acc + d["bias"] * (2 if fault == "bias2" else 1)  # (f) bias added to both segments
    acc = acc + d["res"].float() * _frame_rows(d["rmul"], M, HW, fault)
    return _finish(acc, fault)


def emu_pro(d, fault=None):
    z = d["y"].float() * d["scale"] + d["shift"]
    a = (z * torch.sigmoid(z) * _frame_rows(d["gate"], M, HW, fault)).to(BF)
    return _finish(_mm(a, d["w"], fault), fault)


def _ref(op, d):
    if op == "plain":
        return gm.ref_gemm(d["a"], d["w"]) + (None,)
    if op == "tail":
        return gm.ref_gemm(d["a"], d["w"], False, d["bias"], d["a2"], d["w2"], d["res"], d["rmul"], HW) + (None,)
    a = gm.operand_project(d["y"], d["scale"], d["shift"], d["gate"], HW)[0]
    return gm.ref_gemm(a, d["w"], want_T=True)


EMU = {"plain": emu_plain, "tail": emu_tail, "pro": emu_pro}
KTOT = {"plain": K, "tail": K + K2, "pro": K}
FAULTS = {"plain": ["trunc", "ktail", "strip", "swap"],
          "tail": ["trunc", "ktail", "strip", "swap", "frame", "bias2", "seg2"],
          "pro": ["trunc", "ktail", "strip", "swap", "frame"]}


def _check(op, out, ref, S, T):
    return gm.assert_gemm(out, ref, S, KTOT[op], op, T=T, kop=K)


def _report(op, fault, out, ref, S, T, verdict):
    chk = gm.GemmCheck("figures", KTOT[op], K)
    chk.add(out, ref, S, T)
    worst = chk.worst_hard if T is not None else chk.worst
    fro = go.frob(out, ref)
    print(f"\ngemm oracle | {op:6s} | {fault or 'clean':6s} | frobenius {fro:.5f} | worst err/bound {worst:9.3f} | "
          f"mean signed ulp {chk.mean_ulp:+.4f} | {verdict}")
    return fro


@pytest.mark.parametrize("op", list(EMU))
def test_clean_emulation_passes(inp, op):
    ref, S, T = _ref(op, inp)
    out = EMU[op](inp)
    st = _check(op, out, ref, S, T)
    assert st["count"] >= go.BIAS_MIN_COUNT                 # the bias assertion was not skipped
    assert st["worst_hard"] <= 1.0 and st["share"] <= gm.CAP
    _report(op, None, out, ref, S, T, f"passes, {st['share']:.2e} outside tight")


@pytest.mark.parametrize("op,fault", [(o, f) for o in EMU for f in FAULTS[o]])
def test_planted_fault_is_caught(inp, op, fault):
    ref, S, T = _ref(op, inp)
    out = EMU[op](inp, fault)
    with pytest.raises(AssertionError) as e:
        _check(op, out, ref, S, T)
    fro = _report(op, fault, out, ref, S, T, "caught: " + str(e.value)[:100])
    if fault == "trunc":
        assert fro < OLD            # the Frobenius check of the older tests lets a biased store through


def test_frobenius_hides_a_row_and_a_frame_slip():
    """(c) and (e) at row counts where the old 6e-3 threshold cannot see them; the oracle names the element."""
    g = _gen(7)
    k = n = 24
    w = gm.weight(n, k, g, k ** -0.5)
    m = 940 * STRIP + 1                                     # 60161 rows: the last strip holds one row
    assert (2.0 / m) ** 0.5 < OLD
    a = gm.acts(m, k, g)
    ref, S = gm.ref_gemm(a, w)
    out = _finish(_mm(a, w), "strip")
    fro = go.frob(out, ref)
    print(f"\ngemm oracle | plain  | strip  | M {m} | frobenius {fro:.5f} | sqrt(1/M) {m ** -0.5:.5f} sqrt(2/M) "
          f"{(2.0 / m) ** 0.5:.5f}")
    assert fro < OLD
    with pytest.raises(AssertionError, match=rf"\({m - 1}, \d+\)"):
        gm.assert_gemm(out, ref, S, k, "plain")
    hw, frames = 101, 1200
    m = hw * frames
    a = gm.acts(m, k, g)
    res, rmul = gm.acts(m, n, g, 0.2, 1.3), torch.rand(frames, n, generator=g) + 0.5
    ref, S = gm.ref_gemm(a, w, res=res, rmul=rmul, rhw=hw)
    out = (_mm(a, w) + res.float() * _frame_rows(rmul, m, hw, "frame")).to(BF)
    fro = go.frob(out, ref)
    print(f"\ngemm oracle | tail   | frame  | M {m} | frobenius {fro:.5f}")
    assert fro < OLD
    with pytest.raises(AssertionError, match=r"\(80[5-7], \d+\)"):
        gm.assert_gemm(out, ref, S, k, "tail")


# ---- statistics partials ---------------------------------------------------------------------------------------------
TILE = 128


def emu_stats(c, fault=None):
    tiles = (M + TILE - 1) // TILE
    cf = torch.zeros(tiles * TILE, N)
    cf[:M] = c.float()
    cf = cf.view(tiles, TILE, N)
    ps, pq = cf.sum(1), (cf * cf).sum(1)
    if fault == "pad":                      # (h) the partial M tile's rows are counted into the neighbouring row
        ps[-2], pq[-2] = ps[-2] + ps[-1], pq[-2] + pq[-1]
        ps[-1], pq[-1] = 0, 0
    return ps, pq


def test_stats_partials(inp):
    c = emu_plain(inp)
    ps, pq = emu_stats(c)
    worst = gm.assert_stats(ps, pq, c, "stats", rows_per_tile=TILE)
    print(f"\ngemm oracle | stats  | clean  | worst err/bound {worst:.3f} | passes")
    ps2, pq2 = emu_stats(c, "pad")
    with pytest.raises(AssertionError) as e:
        gm.assert_stats(ps2, pq2, c, "stats", rows_per_tile=TILE)
    # the column sums that the older tests compare do not see it
    torch.testing.assert_close(ps2.sum(0), c.float().sum(0), rtol=1e-4, atol=1e-2)
    print(f"\ngemm oracle | stats  | pad    | column sums unchanged | caught: {str(e.value)[:100]}")


def test_stats_by_tile_index():
    """Grid-stride ownership (pw_gemm): workgroup (s / 4) % grid owns strip s; a workgroup without a strip is zero."""
    g = _gen(3)
    k, n, m, grid = 24, 24, 700, 3
    c = gm.acts(m, n, g).contiguous()
    idx = gm.pw_tile_index(m, k, n, grid)
    assert gm.pw_strip_rows(k, n) == 128 and idx[0] == 0 and idx[512] == 1 and idx[-1] == 1
    ps = torch.zeros(grid, n).index_add_(0, idx, c.float())
    pq = torch.zeros(grid, n).index_add_(0, idx, c.float() ** 2)
    gm.assert_stats(ps, pq, c, "stats", tile_index=idx)
    ps[2, 5] = 1e-3
    with pytest.raises(AssertionError):
        gm.assert_stats(ps, pq, c, "stats", tile_index=idx)


# ---- split weight gradient -------------------------------------------------------------------------------------------
WM, CO, CI, SPLITS = 1990, 24, 40, 3


def emu_wgrad(dy, a, fault=None):
    rows = ((WM + SPLITS - 1) // SPLITS + 63) // 64 * 64          # 704: the last split ends in a 6-row chunk
    parts = []
    for s in range(SPLITS):
        acc = torch.zeros(CO, CI)
        lo, hi = s * rows, min((s + 1) * rows, WM)
        if fault == "twice" and s == 0:                            # (j) the split-boundary row counted twice
            hi += 1
        for m0 in range(lo, hi, 64):
            m1 = min(m0 + 64, hi)
            if fault == "chunk" and m1 - m0 < 64 and s == SPLITS - 1:   # (i) a partial last chunk dropped
                continue
            acc = acc + dy[m0:m1].float().t() @ a[m0:m1].float()
        parts.append(acc)
    return torch.stack(parts).sum(0)


@pytest.mark.parametrize("fault", [None, "chunk", "twice"])
def test_split_weight_gradient(fault):
    g = _gen(11)
    dy, a = gm.acts(WM, CO, g, 0.1), gm.acts(WM, CI, g)
    ref, sab, T = gm.ref_wgrad(dy, a)
    assert torch.equal(T, (dy.double().abs()[:, :, None] * a.double().abs()[:, None, :]).amax(0))
    out = emu_wgrad(dy, a, fault)
    old = ((out.double() - ref).abs().max() / ref.abs().max()).item()       # the metric of test_wgrad_kernel_matches_fp32
    if fault is None:
        st = gm.assert_f32(out, ref, sab, WM + SPLITS, "wgrad")
        print(f"\ngemm oracle | wgrad  | clean  | max err / max ref {old:.2e} | worst err/bound {st['worst']:.3f} | passes")
        return
    with pytest.raises(AssertionError) as e:
        gm.assert_f32(out, ref, sab, WM + SPLITS, "wgrad")
    print(f"\ngemm oracle | wgrad  | {fault:6s} | max err / max ref {old:.2e} | caught: {str(e.value)[:100]}")


# ---- the assertions themselves ---------------------------------------------------------------------------------------
def test_failure_names_the_element(inp):
    ref, S, _ = _ref("plain", inp)
    out = emu_plain(inp)
    out[1234, 77] = out[1234, 77].float() * 1.02
    with pytest.raises(AssertionError, match=r"\(1234, 77\)"):
        gm.assert_gemm(out, ref, S, K, "plain")
    out[3, 9] = float("nan")
    with pytest.raises(AssertionError, match=r"non-finite.*\(3, 9\)"):
        gm.assert_gemm(out, ref, S, K, "plain")
    f = ref.float()
    f[5, 6] = float("inf")
    with pytest.raises(AssertionError, match=r"non-finite.*\(5, 6\)"):
        gm.assert_f32(f, ref, S, K, "plain f32")


def test_cap_counts_per_row():
    """One flipped operand moves all N outputs of its row: two such rows pass (2 x fanout elements), three do not, and
    neither do the same elements spread over many rows; anything beyond hard fails at once."""
    m, n, k = 64, 24, 144
    ref = torch.full((m, n), 1.0, dtype=torch.float64)
    S, T = ref.clone(), ref.clone() * 0.5
    clean = ref.float().to(BF)
    up = torch.tensor(1.0 + 2.0 ** -7).to(BF)              # one bf16 ulp up: outside tight (2^-8 + slack), inside hard

    def run(o):
        return gm.assert_gemm(o, ref, S, k, "rows", T=T, kop=k)

    assert run(clean)["share"] == 0
    o = clean.clone()
    o[3], o[40] = up, up
    st = run(o)
    assert st["share"] == 2 * n / (m * n) and st["worst"] > 1 and st["worst_hard"] <= 1
    o[41] = up
    with pytest.raises(AssertionError, match="outside the tight bound"):
        run(o)
    o = clean.clone()
    o[:5, 0] = up                                          # 5 elements, far below 2 x fanout, but in 5 rows
    with pytest.raises(AssertionError, match="5 of 64 rows"):
        run(o)
    o = clean.clone()
    o[7, 7] = 1.0 + 2.0 ** -5
    with pytest.raises(AssertionError, match=r"hard bound.*\(7, 7\)"):
        run(o)


def test_exact_zero_needs_exact_zero():
    ref = torch.zeros(2, 8, dtype=torch.float64)
    out = torch.zeros(2, 8, dtype=BF)
    gm.assert_gemm(out, ref, ref.clone(), 8, "zeros")
    out[1, 3] = 1e-30
    with pytest.raises(AssertionError):
        gm.assert_gemm(out, ref, ref.clone(), 8, "zeros")


def test_operand_builders_match_the_glue_references(inp):
    d = inp
    a, raw, S = gm.operand_project(d["y"], d["scale"], d["shift"], d["gate"], HW)
    z = d["y"].double() * d["scale"].double() + d["shift"].double()
    want = z * torch.sigmoid(z) * d["gate"].double().repeat_interleave(HW, 0)
    assert torch.equal(raw, want) and torch.equal(a, want.float().to(BF).double())
    a1 = gm.operand_project(d["y"], d["scale"], d["shift"], None, 0, act=0)[1]
    assert torch.equal(a1, z)
    g = _gen(5)
    ce = 48
    dA, y = gm.acts(50, ce, g), gm.acts(50, ce, g, 0.3, 2.0)
    consts = torch.stack([torch.rand(ce, generator=g) + 0.5, torch.randn(ce, generator=g) * 0.3,
                          torch.rand(ce, generator=g) + 0.2, torch.randn(ce, generator=g) * 0.1,
                          torch.randn(ce, generator=g) * 0.1])
    v = gm.operand_pw_bwd_dy(dA, y, consts)[1]
    sc, sh, k1, k2, k0 = consts.double()
    u = y.double() * sc + sh
    s = torch.sigmoid(u)
    assert torch.allclose(v, k1 * (dA.double() * s * (1 + u * (1 - s))) + k2 * y.double() + k0, rtol=1e-13, atol=1e-13)
    fm, keep = torch.rand(5, ce, generator=g) + 0.5, torch.tensor([1 / 0.7, 0.0, 1 / 0.7, 1 / 0.7, 0.0])
    mean, rstd, gamma = torch.randn(ce, generator=g) * 0.1, torch.rand(ce, generator=g) + 0.5, torch.rand(ce, generator=g) + 0.5
    mdz, mdzx = torch.randn(ce, generator=g) * 0.1, torch.randn(ce, generator=g) * 0.1
    v = gm.operand_bnbwd(dA, y, fm, keep, 10, gamma, mean, rstd, mdz, mdzx)[1]
    k1, k2, k0 = go.bwd_consts(mean, rstd, gamma, mdz, mdzx)
    rs = (fm.double() * keep.double()[:, None]).repeat_interleave(10, 0)
    assert torch.allclose(v, k1 * (dA.double() * rs) + k2 * y.double() + k0, rtol=1e-13, atol=1e-13)


# ---- the y-free expand backward: a bound with headroom needs the bias assertion ------------------------------------------
def emu_pw_bwd_z_dx(dz, x, We, consts, trunc=False):
    """pw_bwd_z_kernel's dx in fp32: bf16(k1 dz) We + x (Mk_hi + Mk_lo) + r0, stored once."""
    k1, k2, k0 = consts[2], consts[3], consts[4]
    W = We.float()
    u = (k1 * dz.float()).to(BF)
    mk = (W * k2[:, None]).t() @ W
    hi = mk.to(BF)
    lo = (mk - hi.float()).to(BF)
    acc = u.float() @ W + x.float() @ hi.float() + x.float() @ lo.float() + k0 @ W
    return _store(acc, "trunc" if trunc else None)


def test_z_mode_truncating_store_trips_the_bias_assertion():
    """bound_z_dx carries REL A for the bf16 image of k1 dz, so a clean dx sits near half of it (0.56) and a truncating
    store (one more half ulp, always downwards) exceeds it at a handful of elements at best (1.05 here): the mean signed
    error, -0.5 ulp against a cap of 0.01, is what catches it reliably."""
    g = _gen(31)
    m, ce, cin = 5000, 144, 24                              # 120,000 outputs: the bias assertion applies
    dz, x, We = gm.acts(m, ce, g, 0.1), gm.acts(m, cin, g, 0.5), gm.weight(ce, cin, g, 0.2)
    consts = torch.stack([torch.rand(ce, generator=g) + 0.5, torch.randn(ce, generator=g) * 0.3,
                          torch.rand(ce, generator=g) + 0.2, torch.randn(ce, generator=g) * 0.1,
                          torch.randn(ce, generator=g) * 0.1])
    r = gm.ref_expand_bwd_z(dz, x, We, consts)
    bound, S, V = gm.bound_z_dx(r, ce, cin, go.REL ** 2), gm.S_z_dx(r), gm.z_dx_prevar(dz, We, consts)
    st = gm.assert_within(emu_pw_bwd_z_dx(dz, x, We, consts), r["dx"], bound, "pw_bwd_z dx", S=S, pre_var=V)
    assert st["count"] >= go.BIAS_MIN_COUNT and st["bias_cap"] <= gm.BIAS_CAP_MAX      # the bias assertion applied
    print(f"\ngemm oracle | z dx   | clean  | worst err/bound {st['worst']:9.3f} | mean signed ulp {st['mean_ulp']:+.4f} "
          f"(cap {st['bias_cap']:.4f}) | passes")
    out = emu_pw_bwd_z_dx(dz, x, We, consts, trunc=True)
    try:
        worst = gm.assert_within(out, r["dx"], bound, "pw_bwd_z dx")["worst"]        # the bound alone, no S
    except AssertionError:
        worst = None
    with pytest.raises(AssertionError) as e:
        gm.assert_within(out, r["dx"], bound, "pw_bwd_z dx", S=S, pre_var=V)
    if worst is not None:
        assert "stores are biased" in str(e.value)
    # the bias assertion on its own: with the element-wise bound out of the way it still fails, at -0.5 ulp
    with pytest.raises(AssertionError, match=r"mean signed error -0\.[45]\d+ bf16 ulp.*stores are biased"):
        gm.assert_within(out, r["dx"], 2 * bound, "pw_bwd_z dx", S=S, pre_var=V)
    # ... and the pre-store variance is the model's: the clean emulation's own scatter agrees with it
    o = emu_pw_bwd_z_dx(dz, x, We, consts).double()
    q = r["dx"].abs() > go.BIAS_FLOOR * S
    u = go.bf16_ulp(r["dx"])
    seen = (((o - r["dx"]) / u)[q] ** 2).mean().item()
    model = ((1.0 / 12.0 + V / u ** 2)[q]).mean().item()
    print(f"\ngemm oracle | z dx   | clean  | mean squared error {seen:.3f} ulp^2, model {model:.3f} ulp^2")
    assert 0.5 * model < seen < 1.5 * model
    print(f"\ngemm oracle | z dx   | trunc  | worst err/bound {'> 1' if worst is None else format(worst, '9.3f')} | "
          f"caught: {str(e.value)[:100]}")


def test_z_mode_clean_emulation_exceeds_the_store_only_bias_cap():
    """Why pw_bwd_z's dx gets a derived cap: on the operands of the GPU case 144 x 24, M = 4200 (the same seeded CPU
    generator, tests/test_gemm_oracle_gpu.py expand_inputs) the all-round-to-nearest emulation has a mean signed error
    of -0.0118 ulp over 100,041 elements, outside BIAS_CAP = 0.01 although nothing in it is biased: the rounded k1 dz
    makes single elements up to 80 ulp wide.  It is inside 10 sigma of the modelled variance."""
    ce, cin, m = 144, 24, 4200
    seed = 0
    for k in (22, ce, m, 0):
        seed = (seed * 1000003 + k) % (2 ** 31)
    g = _gen(seed)
    dz, _, x, We = gm.acts(m, ce, g, 0.1), gm.acts(m, ce, g, 0.3, 2.0), gm.acts(m, cin, g, 0.5), gm.weight(ce, cin, g, 0.2)
    consts = torch.stack([torch.rand(ce, generator=g) + 0.5, torch.randn(ce, generator=g) * 0.3,
                          torch.rand(ce, generator=g) + 0.2, torch.randn(ce, generator=g) * 0.1,
                          torch.randn(ce, generator=g) * 0.1])
    r = gm.ref_expand_bwd_z(dz, x, We, consts)
    st = gm.assert_within(emu_pw_bwd_z_dx(dz, x, We, consts), r["dx"], gm.bound_z_dx(r, ce, cin, go.REL ** 2), "pw_bwd_z dx",
                          S=gm.S_z_dx(r), pre_var=gm.z_dx_prevar(dz, We, consts))
    print(f"\ngemm oracle | z dx   | clean  | GPU case 144x24 M=4200 | mean signed ulp {st['mean_ulp']:+.4f} over {st['count']} "
          f"| store-only cap {go.BIAS_CAP} | derived cap {st['bias_cap']:.4f}")
    assert st["count"] >= go.BIAS_MIN_COUNT
    assert go.BIAS_CAP < abs(st["mean_ulp"]) < st["bias_cap"] <= gm.BIAS_CAP_MAX
