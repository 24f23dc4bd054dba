"""The BN / block-tail glue passes of csrc/kernels/bn.hip and block.hip against fp64 on every path (MI355X only).

Elementwise passes (bn_apply, bn_bwd_apply, block_tail, add_scaled_) are held to glue_oracle.assert_bf16_exact -- fp64
reference on the same bf16 inputs, element-wise |out - ref| <= 2^-8 |ref| + 2^-16 S, unbiased stores -- and to a bitwise
repeat; the statistics and finalizers to the tolerance of test_frame_gpu.  Each shape is there for what it reaches:

  (1, 1, 8)         1 vector: the `total - 1 == 0` clamp, divisor 1 in both FastDivs
  (3, 7, 40)        105 vectors: one partial round (< 256 lanes), nv = 5
  (2, 128, 64)      2048 vectors: exactly two full 1024-vector rounds, no tail
  (7, 1, 2304)      HW = 1: every row its own frame
  (3, 2000, 136)    nv = 17, frame boundaries inside a round
  (4, 361, 816)     nv = 102
  (5, 100, 1392)    nv = 174
  (5, 5625, 1200)   4 218 750 vectors > 4096 workgroups x 1024: workgroups 0..23 take a second grid-stride iteration,
                    the last of them with a masked tail; nv = 150 (FastDiv by a non-power-of-two).  One mode per
                    operation, the richest, checked frame by frame.
  (3, 37, 3080), (2, 50, 4096)   C > 3072: the VPT = 2 row kernels of bn_apply / bn_bwd_apply with a partial and a full
                    second vector (block_tail / add_scaled_ stay flat up to C = 8192)

The VPT = 1 row instantiations of bn_apply / bn_bwd_apply / block_tail and add_scaled_'s row kernel are reached only
from 0xF0000000 16-byte vectors up, a 64 GB tensor: nothing here allocates that, they stay untested.

Run with -s for the worst err/bound and the mean signed ulp error per operation."""
import functools

import pytest
import torch
import torch.nn.functional as F

import glue_oracle as go

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SMALL = [(1, 1, 8), (3, 7, 40), (2, 128, 64), (7, 1, 2304), (3, 2000, 136), (4, 361, 816), (5, 100, 1392)]
WIDE = [(3, 37, 3080), (2, 50, 4096)]
BIG = (5, 5625, 1200)
assert BIG[0] * BIG[1] * BIG[2] // 8 > 4096 * 256 * 4      # more vectors than one pass of the capped flat grid takes
assert all(3072 < C <= 4096 for _, _, C in WIDE)            # past use_flat, within bn_channels_ok
# (rs, rb, keep) forms of bn_bwd_apply's upstream gradient
FORMS = {"plain": (0, 0, 0), "se": (1, 1, 0), "rs": (1, 0, 0), "film_keep": (1, 0, 1), "rb": (0, 1, 0)}
SUMMARY = {}


@pytest.fixture(scope="module")
def ext():
    from pytorch_rt1_for_distributed_training_amd import ops
    return ops.load()


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for op, (worst, ulp, cnt, cases) in sorted(SUMMARY.items()):
        print(f"\nglue gpu | {op:12s} | {cases:4d} cases | worst err/bound {worst:.4f} | "
              f"mean signed ulp {ulp / max(cnt, 1):+.5f} over {cnt} elements")


@functools.lru_cache(maxsize=None)
def _small_inputs(N, HW, C):
    return go.make_inputs(N, HW, C, 1000 * N + HW + C, "cuda")


@pytest.fixture(scope="module")
def big():
    N, HW, C = BIG
    return go.make_inputs(N, HW, C, 1000 * N + HW + C, "cuda")


def _bits(t):
    return t.view(torch.int16)


def _frames(d, f):
    """The operands of frames f (a slice); per-channel vectors pass through."""
    per_frame = ("y", "G", "skip", "rs", "rb", "fmul", "fadd", "keep")
    return {k: (v[f] if k in per_frame else v) for k, v in d.items()}


def _check(op, name, d, run, ref_fn, framewise=False):
    """run() -> bf16 output; ref_fn(operands of some frames) -> (ref, S)."""
    out, again = run(), run()
    assert torch.equal(_bits(out), _bits(again)), f"{name}: two runs differ"
    chk = go.Bf16Check(name)
    N = d["y"].shape[0]
    for n in (range(N) if framewise else [None]):
        f = slice(None) if n is None else slice(n, n + 1)
        ref, S = ref_fn(_frames(d, f))
        chk.add(out[f], ref, S, n or 0)
    st = chk.finish()
    print(f"\n{name}: worst err/bound {st['worst']:.4f}, mean signed ulp {st['mean_ulp']:+.5f} ({st['count']})")
    w = SUMMARY.setdefault(op, [0.0, 0.0, 0, 0])
    w[0] = max(w[0], st["worst"])
    w[1] += st["mean_ulp"] * st["count"]
    w[2] += st["count"]
    w[3] += 1


# ---- bn_apply --------------------------------------------------------------------------------------------------------
def _bn_apply(ext, d, act, gated, framewise=False):
    HW = d["y"].shape[1]
    _check("bn_apply", f"bn_apply{tuple(d['y'].shape)} act={act} rs={gated}", d,
           lambda: ext.bn_apply(d["y"], d["scale"], d["shift"], act, d["rs"] if gated else None, HW if gated else 0),
           lambda q: go.ref_bn_apply(q["y"], q["scale"], q["shift"], act, q["rs"] if gated else None), framewise)


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("act", [1, 0])
@pytest.mark.parametrize("N,HW,C", SMALL)
def test_bn_apply(ext, N, HW, C, act, gated):
    _bn_apply(ext, _small_inputs(N, HW, C), act, gated)


@pytest.mark.parametrize("N,HW,C", WIDE)
def test_bn_apply_row_kernel(ext, N, HW, C):
    _bn_apply(ext, _small_inputs(N, HW, C), 1, True)
    _bn_apply(ext, _small_inputs(N, HW, C), 0, False)


def test_bn_apply_second_iteration(ext, big):
    _bn_apply(ext, big, 1, True, framewise=True)


# ---- bn_bwd_apply ----------------------------------------------------------------------------------------------------
def _bn_bwd_apply(ext, d, act, with_gamma, form, framewise=False):
    use_rs, use_rb, use_keep = form
    HW = d["y"].shape[1]

    def pick(q):
        return (q["rs"] if use_rs else None, q["rb"] if use_rb else None, q["keep"] if use_keep else None)

    def run():
        rs, rb, keep = pick(d)
        return ext.bn_bwd_apply(d["G"], rs, rb, HW if (use_rs or use_rb) else 0, d["y"], d["scale"], d["shift"],
                                d["mean"], d["rstd"], d["gamma"] if with_gamma else None, act, d["mdz"], d["mdzx"], keep)

    def ref(q):
        rs, rb, keep = pick(q)
        return go.ref_bn_bwd_apply(q["G"], q["y"], q["scale"], q["shift"], q["mean"], q["rstd"],
                                   q["gamma"] if with_gamma else None, act, q["mdz"], q["mdzx"], rs, rb, keep)

    _check("bn_bwd_apply", f"bn_bwd_apply{tuple(d['y'].shape)} act={act} gamma={with_gamma} (rs, rb, keep)={form}", d,
           run, ref, framewise)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("with_gamma", [True, False])
@pytest.mark.parametrize("act", [1, 0])
@pytest.mark.parametrize("N,HW,C", SMALL)
def test_bn_bwd_apply(ext, N, HW, C, act, with_gamma, form):
    _bn_bwd_apply(ext, _small_inputs(N, HW, C), act, with_gamma, FORMS[form])


@pytest.mark.parametrize("form", ["se", "film_keep"])
@pytest.mark.parametrize("act", [1, 0])
@pytest.mark.parametrize("N,HW,C", WIDE)
def test_bn_bwd_apply_row_kernel(ext, N, HW, C, act, form):
    _bn_bwd_apply(ext, _small_inputs(N, HW, C), act, True, FORMS[form])


def test_bn_bwd_apply_second_iteration(ext, big):
    _bn_bwd_apply(ext, big, 1, True, (1, 1, 1), framewise=True)     # every operand at once: G*rs*keep + rb


def test_bn_bwd_apply_keep_needs_rs(ext):
    d = _small_inputs(3, 7, 40)
    for rb in (None, d["rb"]):
        with pytest.raises(RuntimeError):
            ext.bn_bwd_apply(d["G"], None, rb, 7, d["y"], d["scale"], d["shift"], d["mean"], d["rstd"], d["gamma"], 1,
                             d["mdz"], d["mdzx"], d["keep"])


# ---- block_tail ------------------------------------------------------------------------------------------------------
def _block_tail(ext, d, use_keep, use_skip, use_film, top=False, framewise=False):
    sc = torch.ones_like(d["scale"]) if top else d["scale"]
    sh = torch.zeros_like(d["shift"]) if top else d["shift"]

    def args(q):
        return (q["y"], sc, sh, q["keep"] if use_keep else None, q["skip"] if use_skip else None,
                q["fmul"] if use_film else None, q["fadd"] if use_film else None)

    _check("block_tail", f"block_tail{tuple(d['y'].shape)} keep={use_keep} skip={use_skip} film={use_film} top={top}",
           d, lambda: ext.block_tail(*args(d)), lambda q: go.ref_block_tail(*args(q)), framewise)


@pytest.mark.parametrize("use_film", [False, True])
@pytest.mark.parametrize("use_skip", [False, True])
@pytest.mark.parametrize("use_keep", [False, True])
@pytest.mark.parametrize("N,HW,C", SMALL + WIDE)
def test_block_tail(ext, N, HW, C, use_keep, use_skip, use_film):
    _block_tail(ext, _small_inputs(N, HW, C), use_keep, use_skip, use_film)


@pytest.mark.parametrize("N,HW,C", SMALL + WIDE)
def test_block_tail_film_only(ext, N, HW, C):
    _block_tail(ext, _small_inputs(N, HW, C), False, False, True, top=True)     # the top layer: scale 1, shift 0


def test_block_tail_second_iteration(ext, big):
    _block_tail(ext, big, True, True, True, framewise=True)


def test_block_tail_fmul_needs_fadd(ext):
    d = _small_inputs(3, 7, 40)
    with pytest.raises(RuntimeError):
        ext.block_tail(d["y"], d["scale"], d["shift"], None, None, d["fmul"], None)


def test_block_tail_refuses_wide_rows(ext):
    """Above 8192 channels neither kernel covers a row (the row kernel wrote 4096 of them and returned the rest of the
    output unwritten): the binding refuses before anything is launched."""
    C = 8200
    y = torch.zeros(1, 1, C, device="cuda", dtype=BF)
    v = torch.zeros(C, device="cuda")
    with pytest.raises(RuntimeError, match="8192"):
        ext.block_tail(y, v, v, None, None, None, None)
    _block_tail(ext, _small_inputs(2, 3, 8192), True, True, True)      # the widest row it takes


# ---- add_scaled_ -----------------------------------------------------------------------------------------------------
def _add_scaled(ext, d, framewise=False):
    x, y, s = d["skip"], d["G"], d["fmul"]
    y0, s0 = y.clone(), s.clone()

    def run():
        x1 = x.clone()
        ext.add_scaled_(x1, y, s)
        return x1

    _check("add_scaled_", f"add_scaled_{tuple(x.shape)}", d, run,
           lambda q: go.ref_add_scaled(q["skip"], q["G"], q["fmul"]), framewise)
    assert torch.equal(_bits(y), _bits(y0)) and torch.equal(s.view(torch.int32), s0.view(torch.int32))


@pytest.mark.parametrize("N,HW,C", SMALL + WIDE)
def test_add_scaled(ext, N, HW, C):
    _add_scaled(ext, _small_inputs(N, HW, C))


def test_add_scaled_second_iteration(ext, big):
    _add_scaled(ext, big, framewise=True)


# ---- statistics and finalizers ---------------------------------------------------------------------------------------
# (128, 1024): first P and last C of the 4-channel finalize layout; (127, 1024), (128, 1032): just outside it
FIN = [(1, 8), (37, 144), (128, 1024), (127, 1024), (128, 1032), (2048, 40), (1024, 232), (2048, 1392), (4096, 2304),
       (130, 24)]
ROWS = 64      # rows behind one partial row


def _gen(P, C):
    return torch.Generator(device="cuda").manual_seed(100000 * P + C)


def _vec(gen, C, kind):
    r = torch.rand(C, device="cuda", generator=gen) if kind == "pos" else torch.randn(C, device="cuda", generator=gen)
    return r + 0.5 if kind == "pos" else r * 0.2


def _fwd_partials(P, C, gen):
    """Partial sums of ROWS values each (50 * randn) and sums of squares that go with them: Cauchy-Schwarz keeps
    sum q / count above mean^2, the second term adds a variance of about 1."""
    ps = torch.randn(P, C, device="cuda", generator=gen) * 50
    pq = ps * ps / ROWS + ROWS * (torch.rand(P, C, device="cuda", generator=gen) + 0.5)
    return ps, pq


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("P,C", FIN)
def test_bn_finalize(ext, P, C, affine):
    gen = _gen(P, C)
    ps, pq = _fwd_partials(P, C, gen)
    count = float(P * ROWS)
    gamma, beta = (_vec(gen, C, "pos"), _vec(gen, C, "any")) if affine else (None, None)
    rm, rv = _vec(gen, C, "any"), _vec(gen, C, "pos")
    ref = go.ref_bn_finalize(ps, pq, count, gamma, beta, 1e-5, 0.1, rm, rv)
    assert (ref["var_raw"] > 0.4).all()
    sc, sh, mu, rs = ext.bn_finalize(ps, pq, count, gamma, beta, 1e-5, 0.1, rm, rv)
    for a, k in ((sc, "scale"), (sh, "shift"), (mu, "mean"), (rs, "rstd"), (rm, "running_mean"), (rv, "running_var")):
        go.assert_sum_close(a, ref[k], f"bn_finalize {k}")
    # without running statistics: the same four vectors, bit for bit
    again = ext.bn_finalize(ps, pq, count, gamma, beta, 1e-5, 0.1, None, None)
    assert all(torch.equal(a, b) for a, b in zip((sc, sh, mu, rs), again))


def test_bn_finalize_clamps_negative_variance(ext):
    """A constant column: sum q / count - mean^2 is the rounding of the fp32 partials and nothing else.  Where it comes out
    negative the variance is 0, rstd = 1 / sqrt(eps) and the running variance decays; no NaN.  eps is far below the
    rounding here, so an unclamped variance would give sqrt of a negative number."""
    P, C, eps = 37, 144, 1e-12
    gen = _gen(P, C)
    ps, pq = _fwd_partials(P, C, gen)
    v = torch.rand(C, device="cuda", generator=gen) * 100 + 50         # one constant per column
    ps[:, :16] = (v * ROWS)[:16]                                        # exact in fp32: a power-of-two multiple
    pq[:, :16] = (v * v * ROWS)[:16]                                    # fp32 rounding of v^2, up or down
    count = float(P * ROWS)
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    ref = go.ref_bn_finalize(ps, pq, count, None, None, eps, 0.1, rm, rv)
    neg = ref["var_raw"] < -1e-6
    assert neg[:16].any() and not neg[16:].any(), "the constant columns must include a negative raw variance"
    sc, sh, mu, rs = ext.bn_finalize(ps, pq, count, None, None, eps, 0.1, rm, rv)
    for t in (sc, sh, mu, rs, rm, rv):
        assert torch.isfinite(t).all()
    go.assert_sum_close(rs[neg], torch.full_like(ref["rstd"][neg], eps ** -0.5), "rstd of a clamped column")
    go.assert_sum_close(rv[neg], torch.full_like(ref["rstd"][neg], 0.9), "running_var of a clamped column")
    ok = ref["var_raw"] > 0.5
    go.assert_sum_close(rs[ok], ref["rstd"][ok], "rstd of the other columns")
    go.assert_sum_close(mu, ref["mean"], "mean")


def _bwd_partials(P, C, gen):
    return (torch.randn(P, C, device="cuda", generator=gen) * 50, torch.randn(P, C, device="cuda", generator=gen) * 50)


@pytest.mark.parametrize("P,C", FIN)
def test_bn_bwd_finalize_new_and_pw(ext, P, C):
    gen = _gen(P, C)
    pa, pb = _bwd_partials(P, C, gen)
    count = float(P * ROWS)
    scale, shift, gamma = _vec(gen, C, "pos"), _vec(gen, C, "any"), _vec(gen, C, "pos")
    mean, rstd = _vec(gen, C, "any"), _vec(gen, C, "pos")
    ref = go.ref_bn_bwd_finalize(pa, pb, count, scale, shift, gamma, mean, rstd)
    new = ext.bn_bwd_finalize_new(pa, pb, count)
    assert len(new) == 4
    for a, k in zip(new, ("mdz", "mdzx", "dgamma", "dbeta")):
        go.assert_sum_close(a, ref[k], f"bn_bwd_finalize_new {k}")
    pw = ext.bn_bwd_finalize_pw(pa, pb, count, scale, shift, gamma, mean, rstd)
    assert len(pw) == 5 and tuple(pw[4].shape) == (5, C)
    for a, b, k in zip(new, pw, ("mdz", "mdzx", "dgamma", "dbeta")):
        assert torch.equal(a, b), f"bn_bwd_finalize_pw {k} differs from bn_bwd_finalize_new"
    for i, k in enumerate(("scale", "shift", "k1", "k2", "k0")):
        go.assert_sum_close(pw[4][i], ref["consts"][i], f"bn_bwd_finalize_pw consts[{i}] = {k}")
    assert torch.equal(pw[4][0], scale) and torch.equal(pw[4][1], shift)


@pytest.mark.parametrize("P,C", FIN)
def test_bn_bwd_finalize_accumulates(ext, P, C):
    gen = _gen(P, C)
    pa, pb = _bwd_partials(P, C, gen)
    count = float(P * ROWS)
    dg0 = torch.randn(C, device="cuda", generator=gen) * 100
    db0 = torch.randn(C, device="cuda", generator=gen) * 100
    dg, db = dg0.clone(), db0.clone()
    ref = go.ref_bn_bwd_finalize(pa, pb, count)
    mdz, mdzx = ext.bn_bwd_finalize(pa, pb, count, dg, db)
    go.assert_sum_close(mdz, ref["mdz"], "mdz")
    go.assert_sum_close(mdzx, ref["mdzx"], "mdzx")
    go.assert_sum_close(dg, dg0.double() + ref["dgamma"], "dgamma += ")
    go.assert_sum_close(db, db0.double() + ref["dbeta"], "dbeta += ")


@pytest.mark.parametrize("M,C,P", [(5000, 144, 37), (100, 40, 128), (3001, 1392, 1024), (2000, 2304, 8), (777, 3080, 5)])
def test_bn_stats(ext, M, C, P):
    """(100, 40, 128): more blocks than rows, the empty ones write zero rows; (3001, 1392, 1024): blocks past the end;
    (2000, 2304, 8) and (777, 3080, 5): two vectors per lane, the second full / partial."""
    gen = torch.Generator(device="cuda").manual_seed(M + C + P)
    x = (torch.randn(M, C, device="cuda", generator=gen) * 1.3 + 0.2).to(BF)
    ps, pq = ext.bn_stats(x, P)
    rs, rq = go.ref_bn_stats(x, P)
    go.assert_sum_close(ps, rs, "partial sums")
    go.assert_sum_close(pq, rq, "partial sums of squares")
    go.assert_sum_close(ps.double().sum(0), x.double().sum(0), "column sums")
    go.assert_sum_close(pq.double().sum(0), (x.double() ** 2).sum(0), "column sums of squares")
    used = (M + (M + P - 1) // P - 1) // ((M + P - 1) // P)
    assert torch.count_nonzero(ps[used:]) == 0 and torch.count_nonzero(pq[used:]) == 0
    again = ext.bn_stats(x, P)
    assert torch.equal(ps, again[0]) and torch.equal(pq, again[1])


def test_bn_backward_chain_matches_autograd(ext):
    """bn_bwd_reduce -> bn_bwd_finalize_new -> bn_bwd_apply against fp64 autograd of silu(batch_norm(y)) on the same bf16
    inputs.  S carries the absolute values through the chain: the two means enter as mean|dz| and mean|dz * xhat|, the
    magnitudes that the fp32 partial sums (P = 17 as the model picks for this M: 121 sequential adds per lane, at worst
    121 * 2^-24 < 2^-17 of them) and the roundings of the fp32 statistics are relative to."""
    M, C, P, eps = 4099, 816, 17, 1e-5
    gen = torch.Generator(device="cuda").manual_seed(M + C)
    y = (torch.randn(M, C, device="cuda", generator=gen) * 1.3 + 0.2).to(BF)
    G = (torch.randn(M, C, device="cuda", generator=gen) * 0.1).to(BF)
    gamma, beta = _vec(gen, C, "pos"), _vec(gen, C, "any")

    yd = y.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    F.silu(F.batch_norm(yd, None, None, g64, b64, True, 0.1, eps)).backward(G.double())
    with torch.no_grad():
        mean = yd.mean(0)
        rstd = 1.0 / torch.sqrt(yd.var(0, unbiased=False) + eps)
        k1 = g64 * rstd
        xh = (yd - mean) * rstd
        z = yd * k1 + (b64 - mean * k1)
        s = torch.sigmoid(z)
        dz = G.double() * (s * (1 + z * (1 - s)))
        A, B = dz.abs().mean(0), (dz * xh).abs().mean(0)
        S = k1 * (dz.abs() + A + (yd.abs() + mean.abs()) * rstd * B)
        sc, sh = k1.float(), (b64 - mean * k1).float()
        mu, rs = mean.float(), rstd.float()

    pa, pb = ext.bn_bwd_reduce(G, None, None, 0, y, sc, sh, mu, rs, 1, P)
    mdz, mdzx, dg, db = ext.bn_bwd_finalize_new(pa, pb, float(M))
    dy = ext.bn_bwd_apply(G, None, None, 0, y, sc, sh, mu, rs, gamma, 1, mdz, mdzx)
    go.assert_sum_close(mdz, dz.mean(0), "mdz")
    go.assert_sum_close(mdzx, (dz * xh).mean(0), "mdzx")
    go.assert_sum_close(dg, g64.grad, "dgamma")
    go.assert_sum_close(db, b64.grad, "dbeta")
    st = go.assert_bf16_exact(dy.view(1, M, C), yd.grad.view(1, M, C), S.view(1, M, C), "bn backward chain")
    print(f"\nbn backward chain: worst err/bound {st['worst']:.4f}, mean signed ulp {st['mean_ulp']:+.5f}")
    again = ext.bn_bwd_apply(G, None, None, 0, y, sc, sh, mu, rs, gamma, 1, mdz, mdzx)
    assert torch.equal(_bits(dy), _bits(again))
