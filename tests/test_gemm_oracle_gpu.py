"""Every route of the MFMA product kernels (pwgemm.hip, pwtall.hip, gemm.hip, wgrad.hip, pwbwd.hip, projbwd.hip) against
the element-wise fp64 oracle of tests/gemm_oracle.py, at the shapes where the kernels change path: K / N / M tails,
one row, one strip or tile +- 1 row, grid caps that leave waves without a strip, frames that straddle strips, every
tile variant and split count.  References are fp64 on the GPU; a case also asserts a bitwise repeat where the
reduction order is fixed.  Only shapes the host-side predicates admit are launched; a rejected shape is checked through
the predicate.  Run with -s for one line per case and one summary per entry point (profiles/gemm_oracle_gpu.log)."""
import pytest
import torch

import gemm_oracle as gm
import glue_oracle as go

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda"
TABLES = {}


@pytest.fixture(scope="module")
def ext():
    from pytorch_rt1_for_distributed_training_amd import ops
    yield ops.load()
    for t in TABLES.values():
        t.summary()
    print()


def table(entry):
    return TABLES.setdefault(entry, gm.Table(entry))


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31)
    return torch.Generator(device="cpu").manual_seed(seed)


def vec(n, g, lo=0.5, rand=True, std=1.0):
    v = torch.rand(n, generator=g) + lo if rand else torch.randn(n, generator=g) * std
    return v.to(DEV).contiguous()


def rows(f, n, g, lo=0.5):
    return (torch.rand(f, n, generator=g) + lo).to(DEV).contiguous()


def keep_mask(frames, g):
    """A drop-path mask with at least one kept and, where there is room, one dropped frame."""
    keep = (torch.rand(frames, generator=g) > 0.3).float() / 0.7
    keep[0] = 1.0 / 0.7
    if frames > 1:
        keep[frames // 2] = 0.0
    return keep.to(DEV)


def merge(into, st):
    """Worst figures of several checks of one case."""
    if into is None:
        return dict(st)
    for k in ("worst", "worst_hard", "share", "sum"):
        into[k] = max(into[k], st.get(k, 0.0))
    if st["count"] > into["count"]:
        into["count"], into["mean_ulp"] = st["count"], st["mean_ulp"]
    into["elements"] += st["elements"]
    return into


# ======================================================================================================================
# pw_gemm, skinny
# ======================================================================================================================
# (kc, N, the model's K): every PW_SHAPES specialisation.  Per kc also the smallest admitted K (32 (kc - 1) + 8: a
# K tail of 8 in the last chunk) and K = 32 kc exactly (no tail).
PW_SKINNY = [(2, 24, 40), (1, 40, 24), (1, 24, 24), (1, 144, 24), (1, 144, 32), (5, 24, 144), (5, 32, 144), (1, 192, 32),
             (6, 32, 192), (6, 48, 192), (2, 192, 48), (2, 288, 48), (9, 48, 288)]
PW_BLOCKS = [1, 3, 2048]     # 1 / 3 workgroups: grid-stride with the prefetch, waves without a strip; 2048: one pass


def pw_ms(K, N, bnb=False):
    """1, around one 16-row MFMA tile, one full pass of 4 waves x R x 16 rows - 1 / + 1, and about 1100 rows."""
    p = 4 * gm.pw_strip_rows(K, N, bnb)
    return sorted({1, 15, 16, 17, p - 1, p + 1, 1100})


def pw_ks(kc, K):
    return sorted({K, 32 * (kc - 1) + 8, 32 * kc})


@pytest.mark.parametrize("kc,N,Kmodel", PW_SKINNY)
def test_pw_gemm_skinny(ext, kc, N, Kmodel):
    tab = table("pw_gemm skinny")
    for K in pw_ks(kc, Kmodel):
        assert ext.pw_gemm_supported(K, N) and ext.pw_stats_supported(K, N)
        g = gen(1, K, N)
        w = gm.weight(N, K, g, K ** -0.5, DEV)
        chk, worst_sum = gm.GemmCheck(f"pw_gemm K={K} N={N}", K), 0.0
        for M in pw_ms(K, N):
            a = gm.acts(M, K, g, device=DEV)
            ref, S = gm.ref_gemm(a, w)
            strips = -(-M // gm.pw_strip_rows(K, N))
            for mb in PW_BLOCKS:
                c, ps, pq = ext.pw_gemm(a, w, mb, True)
                assert c.shape == (M, N) and c.dtype == BF
                chk.add(c, ref, S)
                assert chk.worst <= 1.0, (M, mb, chk.finish())
                assert torch.equal(ext.pw_gemm(a, w, mb)[0], c)                  # the plain kernel, and a repeat
                c2, ps2, pq2 = ext.pw_gemm(a, w, mb, True)
                assert torch.equal(c2, c) and torch.equal(ps2, ps) and torch.equal(pq2, pq)
                grid = min(max(-(-strips // 4), 1), mb)
                assert ps.shape == (grid, N) and pq.shape == (grid, N)
                worst_sum = max(worst_sum, gm.assert_stats(ps, pq, c, f"pw_gemm K={K} N={N} M={M} mb={mb}",
                                                           tile_index=gm.pw_tile_index(M, K, N, grid, DEV)))
        st = chk.finish()
        st["sum"] = worst_sum
        tab.add(f"K={K} N={N} M={pw_ms(K, N)} blocks={PW_BLOCKS} +stats", st)


def test_pw_gemm_predicates(ext):
    """The skinny kernel keys on (ceil(K / 32), N), the wide one on ceil(K / 32) in {3, 5, 8, 12} with N % 16 == 0 and
    N >= 256; statistics and the prologues exist on the skinny kernel only."""
    assert not ext.pw_gemm_supported(24, 48) and not ext.pw_gemm_supported(28, 24) and not ext.pw_gemm_supported(72, 24)
    assert not ext.pw_gemm_supported(96, 264) and not ext.pw_gemm_supported(96, 240)       # N % 16, N < 256
    assert not ext.pw_gemm_supported(128, 256) and not ext.pw_gemm_supported(392, 256)     # kc = 4, 13
    assert ext.pw_gemm_supported(96, 576) and not ext.pw_stats_supported(96, 576)
    assert not ext.pw_gemm_bnbwd_supported(144, 24) and not ext.pw_gemm_bnbwd_supported(40, 24)


@pytest.mark.parametrize("kc,N,Kmodel", PW_SKINNY)
def test_pw_gemm_project_prologue(ext, kc, N, Kmodel):
    """The stored operand against glue_oracle.ref_bn_apply element-wise, then C held to tight against the fp64 product
    of that STORED operand.  hw at the kernel's limit 16 R (a strip is exactly one frame), 16 R + 1 (every strip
    straddles two frames) and a large one; hw below 16 R is refused by the binding."""
    tab = table("pw_gemm prologue")
    K = Kmodel
    sr = gm.pw_strip_rows(K, N)
    g = gen(2, K, N)
    w = gm.weight(N, K, g, K ** -0.5, DEV)
    sc, sh = vec(K, g), vec(K, g, rand=False, std=0.3)
    for hw, frames in [(sr, 5), (sr + 1, 5), (1000, 2)]:
        M = hw * frames
        y = gm.acts(M, K, g, 0.2, 1.5, DEV)
        gate = rows(frames, K, g, 0.0)
        ref_a, S_a = go.ref_bn_apply(y.view(frames, hw, K), sc, sh, 1, gate)
        st = None
        for mb in PW_BLOCKS:
            c, ps, pq, a = ext.pw_gemm(y, w, mb, True, sc, sh, gate, hw, True)
            sa = go.assert_bf16_exact(a.view(frames, hw, K), ref_a, S_a, f"pw_gemm operand K={K} hw={hw} mb={mb}")
            ref, S = gm.ref_gemm(a, w)
            st = merge(st, gm.assert_gemm(c, ref, S, K, f"pw_gemm prologue K={K} N={N} hw={hw} mb={mb}"))
            st["worst"] = max(st["worst"], sa["worst"])
            st["worst_hard"] = max(st["worst_hard"], sa["worst"])
            grid = ps.shape[0]
            st["sum"] = max(st["sum"], gm.assert_stats(ps, pq, c, f"pw_gemm prologue stats K={K} N={N} hw={hw} mb={mb}",
                                                       tile_index=gm.pw_tile_index(M, K, N, grid, DEV)))
            assert torch.equal(ext.pw_gemm(y, w, mb, False, sc, sh, gate, hw)[0], c)      # without the store
        tab.add(f"K={K} N={N} hw={hw} frames={frames} blocks={PW_BLOCKS}", st)
    if sr > 1:
        y = gm.acts(5 * (sr - 1), K, g, device=DEV)
        with pytest.raises(RuntimeError):
            ext.pw_gemm(y, w, 64, False, sc, sh, rows(5, K, g), sr - 1)


PW_BNB = [(40, 24), (24, 24), (144, 24), (192, 32), (192, 48), (288, 48)]      # (N, K): PW_BNB_SHAPES at the model K


@pytest.mark.parametrize("N,K", PW_BNB)
@pytest.mark.parametrize("with_keep", [False, True])
def test_pw_gemm_bnbwd(ext, N, K, with_keep):
    """The stored dy3 against glue_oracle.ref_bn_bwd_apply element-wise; dA held to tight against the fp64 product of
    the stored dy3."""
    tab = table("pw_gemm_bnbwd")
    assert ext.pw_gemm_bnbwd_supported(K, N)
    sr = gm.pw_strip_rows(K, N, bnb=True)
    g = gen(3, K, N, with_keep)
    w = gm.weight(N, K, g, K ** -0.5, DEV)
    gamma, mean, rstd = vec(K, g), vec(K, g, rand=False, std=0.1), vec(K, g)
    mdz, mdzx = vec(K, g, rand=False, std=0.1), vec(K, g, rand=False, std=0.1)
    for hw, frames in [(sr, 5), (sr + 1, 5), (700, 3)]:
        M = hw * frames
        dout, y3 = gm.acts(M, K, g, 0.1, device=DEV), gm.acts(M, K, g, 0.2, 1.3, DEV)
        fmul = rows(frames, K, g)
        keep = keep_mask(frames, g) if with_keep else None
        _, raw, S_d = gm.operand_bnbwd(dout, y3, fmul, keep, hw, gamma, mean, rstd, mdz, mdzx)
        st = None
        for mb in PW_BLOCKS:
            dA, dy3 = ext.pw_gemm_bnbwd(dout, y3, w, fmul, keep, hw, gamma, mean, rstd, mdz, mdzx, mb)
            sa = go.assert_bf16_exact(dy3.view(frames, hw, K), raw.view(frames, hw, K), S_d.view(frames, hw, K),
                                      f"pw_gemm_bnbwd dy3 K={K} hw={hw} mb={mb}")
            ref, S = gm.ref_gemm(dy3, w)
            st = merge(st, gm.assert_gemm(dA, ref, S, K, f"pw_gemm_bnbwd K={K} N={N} hw={hw} mb={mb}"))
            st["worst"] = max(st["worst"], sa["worst"])
            st["worst_hard"] = max(st["worst_hard"], sa["worst"])
            again = ext.pw_gemm_bnbwd(dout, y3, w, fmul, keep, hw, gamma, mean, rstd, mdz, mdzx, mb)
            assert torch.equal(again[0], dA) and torch.equal(again[1], dy3)
        tab.add(f"K={K} N={N} hw={hw} frames={frames} keep={with_keep} blocks={PW_BLOCKS}", st)


# ======================================================================================================================
# pw_gemm, wide
# ======================================================================================================================
# kc of WIDE_KC_SHAPES -> (smallest admitted K, 32 kc)
PW_WIDE = [(3, 72, 96), (5, 136, 160), (8, 232, 256), (12, 360, 384)]


@pytest.mark.parametrize("kc,Kmin,Kmax", PW_WIDE)
def test_pw_gemm_wide(ext, kc, Kmin, Kmax):
    """N = 272 and 816 end in a partial 64- (kc <= 5) or 32-column chunk; M = 1, 37 and 1025 (several strips + 1 row);
    1 workgroup walks every strip, 64 give one strip each."""
    tab = table("pw_gemm wide")
    for K in (Kmin, Kmax):
        chk = gm.GemmCheck(f"pw_wide K={K}", K)
        for N in (256, 272, 816, 2304):
            assert ext.pw_gemm_supported(K, N) and not ext.pw_stats_supported(K, N)
            g = gen(4, K, N)
            w = gm.weight(N, K, g, K ** -0.5, DEV)
            for M in (1, 37, 1025):
                a = gm.acts(M, K, g, device=DEV)
                ref, S = gm.ref_gemm(a, w)
                for mb in (1, 64):
                    c = ext.pw_gemm(a, w, mb)[0]
                    chk.add(c, ref, S)
                    assert chk.worst <= 1.0, (N, M, mb, chk.finish())
                    assert torch.equal(ext.pw_gemm(a, w, mb)[0], c)
        tab.add(f"K={K} N=[256, 272, 816, 2304] M=[1, 37, 1025] blocks=[1, 64]", chk.finish())


# ======================================================================================================================
# pw_tall, pw_tall_tail, embed_fwd
# ======================================================================================================================
# (K, N): the smallest admitted shape; a K tail of 8 with N = 24; an N tail in the 128-column-slice path (N > 144);
# K = 25.5 x 32 with N = 8.5 x 16; the widest; the model's 576 -> 96
PW_TALL = [(256, 16), (264, 24), (520, 200), (816, 136), (2304, 384), (576, 96)]


def tall_bm(N):
    return 256 if N <= 96 else (192 if N <= 144 else 128)


@pytest.mark.parametrize("K,N", PW_TALL)
def test_pw_tall(ext, K, N):
    tab = table("pw_tall")
    assert ext.pw_tall_supported(K, N)
    g = gen(5, K, N)
    w = gm.weight(N, K, g, K ** -0.5, DEV)
    chk = gm.GemmCheck(f"pw_tall K={K} N={N}", K)
    ms = [1, tall_bm(N) - 1, tall_bm(N) + 1, 1500]
    for M in ms:
        a = gm.acts(M, K, g, device=DEV)
        ref, S = gm.ref_gemm(a, w)
        c = ext.pw_tall(a, w)[0]
        chk.add(c, ref, S)
        assert chk.worst <= 1.0, (M, chk.finish())
        assert torch.equal(ext.pw_tall(a, w)[0], c)
    tab.add(f"K={K} N={N} M={ms}", chk.finish())
    if (K, N) == (520, 200):
        # N > 144 with M >= 65536 takes the 128-column slices with 4 x 16 rows per wave (BM = 256) instead of 2 x 16:
        # 256 tiles + 1 row
        M = 65537
        a = gm.acts(M, K, g, device=DEV)
        ref, S = gm.ref_gemm(a, w)
        c = ext.pw_tall(a, w)[0]
        st = gm.assert_gemm(c, ref, S, K, f"pw_tall K={K} N={N} M={M}")
        assert st["count"] >= go.BIAS_MIN_COUNT and torch.equal(ext.pw_tall(a, w)[0], c)
        tab.add(f"K={K} N={N} M={M} (the BM = 256 slice kernel)", st)
    # the operand prologue, frames of 1, 7 and 100 rows (a workgroup's rows span many / several / two frames)
    M = 700
    sc, sh = vec(K, g), vec(K, g, rand=False, std=0.3)
    for hw in (1, 7, 100):
        y = gm.acts(M, K, g, 0.2, 1.5, DEV)
        gate = rows(M // hw, K, g, 0.0)
        c, a = ext.pw_tall(y, w, sc, sh, gate, hw, True)
        ref_a, S_a = go.ref_bn_apply(y.view(M // hw, hw, K), sc, sh, 1, gate)
        sa = go.assert_bf16_exact(a.view(M // hw, hw, K), ref_a, S_a, f"pw_tall operand K={K} hw={hw}")
        ref, S = gm.ref_gemm(a, w)
        st = gm.assert_gemm(c, ref, S, K, f"pw_tall prologue K={K} N={N} hw={hw}")
        st["worst"] = st["worst_hard"] = max(st["worst"], sa["worst"])
        (c2,) = ext.pw_tall(y, w, sc, sh, gate, hw, False)
        assert torch.equal(c2, c)
        tab.add(f"K={K} N={N} M={M} prologue hw={hw} stored and not", st)


def test_pw_tall_predicates(ext):
    assert not ext.pw_tall_supported(248, 16) and not ext.pw_tall_supported(256, 8)      # K < 256, N < 16
    assert not ext.pw_tall_supported(260, 16) and not ext.pw_tall_supported(256, 256)    # K % 8, K > N
    assert not ext.pw_tall_supported(512, 392)                                          # N > 384
    # pw_tall_tail serves the single-slice shapes only
    assert not ext.pw_tall_preferred(520, 200) and not ext.pw_tall_preferred(2304, 384)
    assert all(ext.pw_tall_preferred(k, n) for k, n in [(256, 16), (264, 24), (816, 136), (576, 96)])


@pytest.mark.parametrize("K,N", [(256, 16), (264, 24), (816, 136), (576, 96)])
def test_pw_tall_tail(ext, K, N):
    """Two reduction segments + bias (+ res * rmul[m / rhw]): K2 = 8 (one chunk, a tail of 8), 96 (three chunks) and 136
    (4.25); residual frames of 1 and 7 rows."""
    tab = table("pw_tall_tail")
    assert ext.pw_tall_preferred(K, N)
    g = gen(6, K, N)
    w = gm.weight(N, K, g, K ** -0.5, DEV)
    bias = vec(N, g, rand=False)
    ms = [1, tall_bm(N) - 1, tall_bm(N) + 1, 700]
    for K2 in (8, 96, 136):
        w2 = gm.weight(N, K2, g, K2 ** -0.5, DEV)
        chk = gm.GemmCheck(f"pw_tall_tail K={K} N={N} K2={K2}", K + K2)
        for M in ms:
            a, a2 = gm.acts(M, K, g, device=DEV), gm.acts(M, K2, g, device=DEV)
            ref, S = gm.ref_gemm(a, w, False, bias, a2, w2)
            c = ext.pw_tall_tail(a, w, a2, w2, bias)
            chk.add(c, ref, S)
            assert chk.worst <= 1.0, (M, "no res", chk.finish())
            assert torch.equal(ext.pw_tall_tail(a, w, a2, w2, bias), c)
            for rhw in (1, 7):
                if M % rhw:
                    continue
                res, rmul = gm.acts(M, N, g, 0.2, 1.3, DEV), rows(M // rhw, N, g)
                ref, S = gm.ref_gemm(a, w, False, bias, a2, w2, res, rmul, rhw)
                c = ext.pw_tall_tail(a, w, a2, w2, bias, res, rmul, rhw)
                assert torch.equal(ext.pw_tall_tail(a, w, a2, w2, bias, res, rmul, rhw), c)
                chk.add(c, ref, S)
                assert chk.worst <= 1.0, (M, rhw, chk.finish())
        tab.add(f"K={K} N={N} K2={K2} M={ms} res none / rhw 1 / rhw 7", chk.finish())


@pytest.mark.parametrize("B,S,K,N", [(1, 1, 8, 16), (3, 7, 40, 144), (5, 48, 520, 512)])
def test_embed_fwd(ext, B, S, K, N):
    """pw_tall's fp32 epilogue: tokens W^T + bias + pos[m % S]."""
    tab = table("embed_fwd")
    g = gen(7, K, N)
    x = gm.acts(B * S, K, g, device=DEV).view(B, S, K)
    w = gm.weight(N, K, g, K ** -0.5, DEV)
    bias, pos = vec(N, g, rand=False), (torch.randn(S + 2, N, generator=g)).to(DEV)
    out = ext.embed_fwd(x, w, bias, pos)
    ref, sab = gm.ref_gemm(x.view(B * S, K), w, bias=bias, pos=pos[:S])
    st = gm.assert_f32(out.view(B * S, N), ref, sab, K + 2, f"embed_fwd {B}x{S} K={K} N={N}")
    assert torch.equal(ext.embed_fwd(x, w, bias, pos), out)
    tab.add(f"B={B} S={S} K={K} N={N}", st)


# ======================================================================================================================
# gemm, gemm_tail
# ======================================================================================================================
# ragged M, N and K tiles in every configuration (128 x 128, 64 x 256, 256 x 64; BK = 64)
GEMM_SHAPES = [(1, 8, 8), (129, 264, 72), (300, 40, 24), (257, 136, 200), (513, 232, 1392)]
GEMM_BM = {0: 128, 1: 64, 2: 256}


@pytest.mark.parametrize("cfg", [0, 1, 2])
@pytest.mark.parametrize("nn", [False, True])
def test_gemm(ext, cfg, nn):
    tab = table("gemm")
    for M, N, K in GEMM_SHAPES:
        g = gen(8, M, N, K)
        a = gm.acts(M, K, g, device=DEV)
        w = gm.weight(N, K, g, K ** -0.5, DEV)
        b = w.t().contiguous() if nn else w
        bias = vec(N, g, rand=False)
        name = f"gemm cfg={cfg} nn={nn} {M}x{N}x{K}"
        ref, S = gm.ref_gemm(a, w)
        refb, Sb = gm.ref_gemm(a, w, bias=bias)
        (c,) = ext.gemm(a, b, nn, None, cfg=cfg)                              # the LDS-staged row stores
        st = gm.assert_gemm(c, ref, S, K, name)
        (cb,) = ext.gemm(a, b, nn, bias, cfg=cfg)                             # the MFMA-layout epilogue
        st = merge(st, gm.assert_gemm(cb, refb, Sb, K + 1, name + " bias"))
        (cf,) = ext.gemm(a, b, nn, bias, out_f32=True, cfg=cfg)
        st = merge(st, gm.assert_f32(cf, refb, Sb, K + 1, name + " f32"))
        cs, ps, pq = ext.gemm(a, b, nn, bias, stats=True, cfg=cfg)
        assert torch.equal(cs, cb) and ps.shape == (-(-M // GEMM_BM[cfg]), N)
        st["sum"] = max(st["sum"], gm.assert_stats(ps, pq, cs, name + " stats", rows_per_tile=GEMM_BM[cfg]))
        again = ext.gemm(a, b, nn, bias, stats=True, cfg=cfg)
        assert all(torch.equal(x, y) for x, y in zip(again, (cs, ps, pq)))
        assert torch.equal(ext.gemm(a, b, nn, None, cfg=cfg)[0], c)
        tab.add(f"cfg={cfg} {'NN' if nn else 'NT'} {M}x{N}x{K} plain / bias / f32 / stats", st)


@pytest.mark.parametrize("cfg", [0, 1, 2])
def test_gemm_prologue(ext, cfg):
    """A = silu(y * scale + shift) * gate[m / hw]: the stored operand against ref_bn_apply, C against the product of the
    stored operand; store_a off gives the same C.  hw = 1, 7, 100 with M = 700."""
    tab = table("gemm prologue")
    M = 700
    for _, N, K in GEMM_SHAPES[1:]:
        g = gen(9, N, K)
        w = gm.weight(N, K, g, K ** -0.5, DEV)
        sc, sh = vec(K, g), vec(K, g, rand=False, std=0.3)
        st = None
        for hw in (1, 7, 100):
            y = gm.acts(M, K, g, 0.2, 1.5, DEV)
            gate = rows(M // hw, K, g, 0.0)
            c, ps, pq, a = ext.gemm(y, w, False, None, sc, sh, gate, hw, stats=True, cfg=cfg, store_a=True)
            ref_a, S_a = go.ref_bn_apply(y.view(M // hw, hw, K), sc, sh, 1, gate)
            sa = go.assert_bf16_exact(a.view(M // hw, hw, K), ref_a, S_a, f"gemm operand cfg={cfg} K={K} hw={hw}")
            ref, S = gm.ref_gemm(a, w)
            st = merge(st, gm.assert_gemm(c, ref, S, K, f"gemm prologue cfg={cfg} {M}x{N}x{K} hw={hw}"))
            st["worst"] = max(st["worst"], sa["worst"])
            st["worst_hard"] = max(st["worst_hard"], sa["worst"])
            st["sum"] = max(st["sum"], gm.assert_stats(ps, pq, c, f"gemm prologue stats cfg={cfg} K={K} hw={hw}",
                                                       rows_per_tile=GEMM_BM[cfg]))
            (c2,) = ext.gemm(y, w, False, None, sc, sh, gate, hw, cfg=cfg)
            assert torch.equal(c2, c)
        tab.add(f"cfg={cfg} {M}x{N}x{K} hw=[1, 7, 100] store_a on / off +stats", st)


@pytest.mark.parametrize("cfg", [0, 1, 2])
def test_gemm_tail(ext, cfg):
    tab = table("gemm_tail")
    for M, N, K in [(1, 8, 8), (301, 264, 72), (301, 40, 24), (301, 136, 200), (511, 232, 1392)]:
        g = gen(10, M, N, K)
        a, w = gm.acts(M, K, g, device=DEV), gm.weight(N, K, g, K ** -0.5, DEV)
        bias = vec(N, g, rand=False)
        for K2 in (8, 40, 232):
            a2, w2 = gm.acts(M, K2, g, device=DEV), gm.weight(N, K2, g, K2 ** -0.5, DEV)
            chk = gm.GemmCheck(f"gemm_tail cfg={cfg} {M}x{N}x{K}+{K2}", K + K2 + 2)
            ref, S = gm.ref_gemm(a, w, False, bias, a2, w2)
            c = ext.gemm_tail(a, w, a2, w2, bias, cfg=cfg)
            chk.add(c, ref, S)
            assert torch.equal(ext.gemm_tail(a, w, a2, w2, bias, cfg=cfg), c)
            for rhw in (1, 7):
                if M % rhw:
                    continue
                res, rmul = gm.acts(M, N, g, 0.2, 1.3, DEV), rows(M // rhw, N, g)
                ref, S = gm.ref_gemm(a, w, False, bias, a2, w2, res, rmul, rhw)
                c = ext.gemm_tail(a, w, a2, w2, bias, res, rmul, rhw, cfg)
                chk.add(c, ref, S)
                assert torch.equal(ext.gemm_tail(a, w, a2, w2, bias, res, rmul, rhw, cfg), c)
            tab.add(f"cfg={cfg} {M}x{N}x{K}+{K2} res none / rhw 1 / rhw 7", chk.finish())


@pytest.mark.parametrize("bn", [128, 256])
def test_gemm256(ext, bn):
    """gemm256.hip (256-row tiles, K slabs of 32 / 64 through LDS-DMA): one row, ragged M / N / K tiles, NT with bias or
    statistics, NN, and the operand prologue at hw = 1, 7, 100."""
    tab = table("gemm256")
    for M, N, K in [(1, 8, 8), (257, 136, 200), (513, 264, 72)]:
        g = gen(26, M, N, K)
        a, w, bias = gm.acts(M, K, g, device=DEV), gm.weight(N, K, g, K ** -0.5, DEV), vec(N, g, rand=False)
        name = f"gemm256 bn={bn} {M}x{N}x{K}"
        ref, S = gm.ref_gemm(a, w)
        c, ps, pq = ext.gemm256(a, w, False, stats=True, bn=bn)
        st = gm.assert_gemm(c, ref, S, K, name)
        assert ps.shape == (-(-M // 256), N)
        st["sum"] = gm.assert_stats(ps, pq, c, name + " stats", rows_per_tile=256)
        assert torch.equal(ext.gemm256(a, w, False, bn=bn)[0], c)
        wt = w.t().contiguous()
        cn = ext.gemm256(a, wt, True, bn=bn)[0]
        st = merge(st, gm.assert_gemm(cn, ref, S, K, name + " NN"))
        assert torch.equal(ext.gemm256(a, wt, True, bn=bn)[0], cn)
        refb, Sb = gm.ref_gemm(a, w, bias=bias)
        cb = ext.gemm256(a, w, False, bias, bn=bn)[0]
        st = merge(st, gm.assert_gemm(cb, refb, Sb, K + 1, name + " bias"))
        assert torch.equal(ext.gemm256(a, w, False, bias, bn=bn)[0], cb)
        tab.add(f"bn={bn} {M}x{N}x{K} NT+stats / NN / bias", st)
    M = 700
    for N, K in [(136, 200), (264, 72)]:
        g = gen(27, N, K)
        w = gm.weight(N, K, g, K ** -0.5, DEV)
        sc, sh = vec(K, g), vec(K, g, rand=False, std=0.3)
        st = None
        for hw in (1, 7, 100):
            y, gate = gm.acts(M, K, g, 0.2, 1.5, DEV), rows(M // hw, K, g, 0.0)
            c, ps, pq, a = ext.gemm256(y, w, False, None, sc, sh, gate, hw, True, True, bn)
            ref_a, S_a = go.ref_bn_apply(y.view(M // hw, hw, K), sc, sh, 1, gate)
            sa = go.assert_bf16_exact(a.view(M // hw, hw, K), ref_a, S_a, f"gemm256 operand bn={bn} K={K} hw={hw}")
            ref, S = gm.ref_gemm(a, w)
            st = merge(st, gm.assert_gemm(c, ref, S, K, f"gemm256 prologue bn={bn} {M}x{N}x{K} hw={hw}"))
            st["worst"] = max(st["worst"], sa["worst"])
            st["worst_hard"] = max(st["worst_hard"], sa["worst"])
            st["sum"] = max(st["sum"], gm.assert_stats(ps, pq, c, f"gemm256 prologue stats bn={bn} K={K} hw={hw}",
                                                       rows_per_tile=256))
            assert torch.equal(ext.gemm256(y, w, False, None, sc, sh, gate, hw, bn=bn)[0], c)
        tab.add(f"bn={bn} {M}x{N}x{K} prologue hw=[1, 7, 100] store_a on / off +stats", st)


# ======================================================================================================================
# wgrad, gram, xgram
# ======================================================================================================================
# partial tiles in both directions for every variant (32 x 256, 64 x 128, 128 x 128, 64 x 256, 128 x 64, 128 x 256)
WG_SHAPES = [(8, 8), (24, 40), (136, 816), (384, 264)]
WG_SPLITS = [1, 3, 8, 16]        # 8 and 16 take the XCD-grouped 1-D grid


def wg_ms(splits):
    """One row; one 64-row chunk - 1 / exact / + 1; about 2000 (a partial last chunk); and, with
    rows per split = ceil(ceil(M / splits) / 64) * 64:
      64 (splits - 1) + 1: every split one chunk and the LAST SPLIT ONE ROW (splits = 3: 64, 64, 1);
      64 splits + 1:       the rows run out early and the LAST SPLIT IS EMPTY and must write zeros
                           (splits = 3, M = 193: 128, 65, 0)."""
    return sorted({1, 63, 64, 65, 64 * (splits - 1) + 1, 64 * splits + 1, 2000})


@pytest.mark.parametrize("variant", range(6))
@pytest.mark.parametrize("Co,Ci", WG_SHAPES)
def test_wgrad(ext, variant, Co, Ci):
    tab = table("wgrad")
    g = gen(11, Co, Ci)
    st = None
    for splits in WG_SPLITS:
        for M in wg_ms(splits):
            dy, a = gm.acts(M, Co, g, 0.1, device=DEV), gm.acts(M, Ci, g, device=DEV)
            ref, sab, _ = gm.ref_wgrad(dy, a, want_T=False)
            name = f"wgrad v{variant} {Co}x{Ci} M={M} splits={splits}"
            out = ext.wgrad(dy, a, variant=variant, splits=splits)
            assert out.shape == (Co, Ci) and out.dtype == torch.float32
            s_eff = min(splits, -(-M // 64))
            st = merge(st, gm.assert_f32(out, ref, sab, M + s_eff, name))
            assert torch.equal(ext.wgrad(dy, a, variant=variant, splits=splits), out)
            part = ext.wgrad(dy, a, variant=variant, splits=splits, partials=True)
            assert part.shape == (s_eff, Co, Ci)
            st = merge(st, gm.assert_f32(part.double().sum(0).float(), ref, sab, -(-M // s_eff) + 64, name + " partials"))
            sums = ext.wgrad(dy, a, variant=variant, splits=splits, sums=True)
            assert sums.shape == (Co * Ci + Co,)
            assert torch.equal(sums[:Co * Ci].view(Co, Ci), out)
            cs, ca = gm.ref_colsum(dy)
            st = merge(st, gm.assert_f32(sums[Co * Ci:], cs, ca, M + s_eff, name + " column sums"))
    tab.add(f"variant={variant} {Co}x{Ci} splits={WG_SPLITS} M=1..2000 (one-row and empty last split) dW / partials / sums", st)


@pytest.mark.parametrize("variant", range(6))
@pytest.mark.parametrize("act,with_gate", [(0, False), (0, True), (1, False), (1, True)])
def test_wgrad_prologue(ext, variant, act, with_gate):
    """a = act(y * scale + shift) [* gate[m / hw]] rebuilt in registers and never stored: the reference rounds the fp64
    operand to bf16 and the hard bound allows two operands per output on their other bf16 neighbour.  hw = 64 is the
    kernel's limit (a 64-row chunk is one frame), 65 and 127 make every chunk straddle two frames."""
    tab = table("wgrad prologue")
    for Co, Ci in WG_SHAPES:
        g = gen(12, Co, Ci, act, with_gate)
        sc, sh = vec(Ci, g), vec(Ci, g, rand=False, std=0.3)
        st = None
        for hw in (64, 65, 127, 200):
            frames = 7
            M = hw * frames
            dy, y = gm.acts(M, Co, g, 0.1, device=DEV), gm.acts(M, Ci, g, 0.2, 1.5, DEV)
            gate = rows(frames, Ci, g, 0.0) if with_gate else None
            a = gm.operand_project(y, sc, sh, gate, hw, act)[0]
            ref, sab, T = gm.ref_wgrad(dy, a)
            for splits in WG_SPLITS:
                name = f"wgrad v{variant} act={act} gate={with_gate} {Co}x{Ci} hw={hw} splits={splits}"
                out = ext.wgrad(dy, y, sc, sh, gate, act, hw, variant=variant, splits=splits)
                st = merge(st, gm.assert_f32(out.t(), ref.t(), sab.t(), M + splits, name, T=T.t(), kop=M, fanout=Co))
                assert torch.equal(ext.wgrad(dy, y, sc, sh, gate, act, hw, variant=variant, splits=splits), out)
        tab.add(f"variant={variant} act={act} gate={with_gate} {Co}x{Ci} hw=[64, 65, 127, 200] splits={WG_SPLITS}", st)
    if with_gate:
        y = gm.acts(63 * 2, 40, gen(13), device=DEV)
        with pytest.raises(RuntimeError):
            ext.wgrad(gm.acts(126, 24, gen(14), device=DEV), y, vec(40, gen(15)), vec(40, gen(16)), rows(2, 40, gen(17)), 1, 63)


@pytest.mark.parametrize("C", [8, 40, 136, 264])
def test_gram(ext, C):
    tab = table("gram")
    g = gen(18, C)
    st = None
    for variant in (-1, 0, 2, 5):
        for splits in (0, 1, 3, 8):
            for M in (1, 65, 64 * max(splits, 1) + 1, 2000):
                x = gm.acts(M, C, g, device=DEV)
                G, sx = ext.gram(x, variant, splits)
                ref, sab, _ = gm.ref_wgrad(x, x, want_T=False)
                name = f"gram C={C} M={M} v{variant} splits={splits}"
                st = merge(st, gm.assert_f32(G, ref, sab, M + 16, name))
                cs, ca = gm.ref_colsum(x)
                st = merge(st, gm.assert_f32(sx, cs, ca, M + 16, name + " sx"))
                again = ext.gram(x, variant, splits)
                assert torch.equal(again[0], G) and torch.equal(again[1], sx)
    tab.add(f"C={C} variants=[-1, 0, 2, 5] splits=[auto, 1, 3, 8] M=1..2000", st)


@pytest.mark.parametrize("cin", [8, 24, 40, 64])
def test_xgram(ext, cin):
    tab = table("xgram")
    g = gen(19, cin)
    st = None
    for M in (1, 63, 257, 3000):
        x = gm.acts(M, cin, g, device=DEV)
        out = ext.xgram(x)
        assert torch.equal(ext.xgram(x), out)
        ref, sab, _ = gm.ref_wgrad(x, x, want_T=False)
        cs, ca = gm.ref_colsum(x)
        st = merge(st, gm.assert_f32(out[:cin * cin].view(cin, cin), ref, sab, M, f"xgram cin={cin} M={M}"))
        st = merge(st, gm.assert_f32(out[cin * cin:], cs, ca, M, f"xgram cin={cin} M={M} sx"))
    tab.add(f"cin={cin} M=[1, 63, 257, 3000]", st)


# ======================================================================================================================
# exact-integer cases
# ======================================================================================================================
def int_operands(M, N, K):
    """Small-integer operands: every product and every partial sum is an integer below 2^24, exact in fp32 in any order,
    so the output must EQUAL the bf16-rounded fp64 product.  w is asymmetric (row != column)."""
    g = gen(20, M, N, K)
    a = torch.randint(-3, 4, (M, K), generator=g).to(BF).to(DEV)
    w = (torch.arange(N)[:, None] % 5 - 2 + (torch.arange(K)[None, :] % 3)).to(BF).to(DEV)
    return a, w, (a.double() @ w.double().t())


def test_exact_integers_pw_gemm_and_tall(ext):
    """One skinny shape per grid regime, two wide ones (a partial last chunk at 64 and at 32 columns), three pw_tall."""
    for M, N, K, mb in [(1100, 144, 24, 3), (1100, 48, 288, 2048), (1025, 816, 160, 64), (1025, 272, 384, 1)]:
        a, w, ref = int_operands(M, N, K)
        assert torch.equal(ext.pw_gemm(a, w, mb)[0], ref.to(BF)), (M, N, K)
    for M, N, K in [(700, 24, 264), (700, 136, 816), (300, 200, 520)]:
        a, w, ref = int_operands(M, N, K)
        assert torch.equal(ext.pw_tall(a, w)[0], ref.to(BF)), (M, N, K)


@pytest.mark.parametrize("cfg", [0, 1, 2])
def test_exact_integers_gemm(ext, cfg):
    for M, N, K in [(257, 136, 200), (300, 264, 72)]:
        a, w, ref = int_operands(M, N, K)
        assert torch.equal(ext.gemm(a, w, False, None, cfg=cfg)[0], ref.to(BF)), (M, N, K)
        assert torch.equal(ext.gemm(a, w.t().contiguous(), True, None, cfg=cfg)[0], ref.to(BF)), (M, N, K)
        assert torch.equal(ext.gemm(a, w, False, None, out_f32=True, cfg=cfg)[0], ref.float()), (M, N, K)


@pytest.mark.parametrize("variant", range(6))
def test_exact_integers_wgrad(ext, variant):
    for M, Co, Ci, splits in [(2000, 24, 40, 3), (1000, 136, 264, 8)]:
        dy, a = int_operands(M, 8, Co)[0], int_operands(M, 16, Ci)[0]          # [M, Co] and [M, Ci] integers in -3..3
        ref = (dy.double().t() @ a.double()).float()                           # |sum| <= 9 M < 2^24
        assert torch.equal(ext.wgrad(dy, a, variant=variant, splits=splits), ref), (M, Co, Ci)


# ======================================================================================================================
# pw_bwd, pw_bwd_z, expand_bwd_z_wide
# ======================================================================================================================
PWBWD = [(144, 24), (192, 32), (288, 48)]          # PWBWD_SHAPES
# one row, a 64-row strip - 1 / exact / + 1, 15.6 and 46.9 strips; 4200 x 24 outputs reach the bias statistic's 100,000
PWBWD_M = [1, 63, 64, 65, 1000, 3000, 4200]
PWBWD_GRID = [1, 3, 64]                            # one workgroup walks every strip; 3; one strip each


def expand_inputs(M, CE, CIN, g, hw=None):
    d = {"dA": gm.acts(M, CE, g, 0.1, device=DEV), "y": gm.acts(M, CE, g, 0.3, 2.0, DEV), "x": gm.acts(M, CIN, g, 0.5, device=DEV),
         "We": gm.weight(CE, CIN, g, 0.2, DEV),
         "consts": torch.stack([vec(CE, g), vec(CE, g, rand=False, std=0.3), vec(CE, g, 0.2), vec(CE, g, rand=False, std=0.1),
                                vec(CE, g, rand=False, std=0.1)]).contiguous()}
    d["dout"] = gm.acts(M, CIN, g, 0.2, 1.3, DEV) if hw else None
    d["fmul"] = rows(M // hw, CIN, g) if hw else None
    return d


def pwbwd_cases():
    for M in PWBWD_M:
        yield M, None
    for hw in (1, 8, 1000):                        # the skip path: every row its own frame, 8-row frames, 3 frames
        yield (3000 if hw == 1000 else 200), hw


@pytest.mark.parametrize("CE,CIN", PWBWD)
def test_pw_bwd(ext, CE, CIN):
    """dy = bf16(k1 dA silu'(y sc + sh) + k2 y + k0) is rebuilt in registers and never stored: the reference rounds the
    fp64 dy and dx / dWe are held to hard, with the caps per row of dx and per output channel of dWe."""
    tab = table("pw_bwd")
    assert ext.pw_bwd_supported(CE, CIN)
    for M, hw in pwbwd_cases():
        g = gen(21, CE, M, hw or 0)
        d = expand_inputs(M, CE, CIN, g, hw)
        dy = gm.operand_pw_bwd_dy(d["dA"], d["y"], d["consts"])[0]
        ref, S, T = gm.ref_gemm(dy, d["We"], nn=True, res=d["dout"], rmul=d["fmul"], rhw=hw or 1, want_T=True)
        wref, wsab, wT = gm.ref_wgrad(dy, d["x"])
        st = None
        for mb in PWBWD_GRID:
            name = f"pw_bwd {CE}x{CIN} M={M} hw={hw} grid={mb}"
            dx, dWe = ext.pw_bwd(d["dA"], d["y"], d["x"], d["We"], d["consts"], d["dout"], d["fmul"], hw or 1, mb)
            st = merge(st, gm.assert_gemm(dx, ref, S, CE + 1, name + " dx", T=T, kop=CE))
            parts = min(-(-M // 64), mb)
            sw = gm.assert_f32(dWe, wref, wsab, M + parts, name + " dWe", T=wT, kop=M)
            st["sum"] = max(st["sum"], sw["worst_hard"])
            again = ext.pw_bwd(d["dA"], d["y"], d["x"], d["We"], d["consts"], d["dout"], d["fmul"], hw or 1, mb)
            assert torch.equal(again[0], dx) and torch.equal(again[1], dWe)
        tab.add(f"{CE}x{CIN} M={M} skip hw={hw} grids={PWBWD_GRID} dx + dWe (sum = dWe / hard)", st)
    assert not ext.pw_bwd_supported(CE + 8, CIN) and not ext.pw_bwd_supported(CE, CIN + 8)


@pytest.mark.parametrize("CE,CIN", PWBWD)
def test_pw_bwd_z(ext, CE, CIN):
    """The y-free rewrite against the exact chain, with the bound of gemm_oracle.bound_z_dx / bound_z_dwe."""
    tab = table("pw_bwd_z")
    for M, hw in pwbwd_cases():
        g = gen(22, CE, M, hw or 0)
        d = expand_inputs(M, CE, CIN, g, hw)
        r = gm.ref_expand_bwd_z(d["dA"], d["x"], d["We"], d["consts"], d["dout"], d["fmul"], hw or 1)
        bdx, V = gm.bound_z_dx(r, CE, CIN, go.REL ** 2), gm.z_dx_prevar(d["dA"], d["We"], d["consts"])
        st = None
        for mb in PWBWD_GRID:
            name = f"pw_bwd_z {CE}x{CIN} M={M} hw={hw} grid={mb}"
            dx, dWe = ext.pw_bwd_z(d["dA"], d["x"], d["We"], d["consts"], d["dout"], d["fmul"], hw or 1, mb)
            sd = gm.assert_within(dx, r["dx"], bdx, name + " dx", S=gm.S_z_dx(r), pre_var=V)
            assert M != 4200 or (sd["count"] >= go.BIAS_MIN_COUNT and sd["bias_cap"] <= gm.BIAS_CAP_MAX), sd   # applied
            st = merge(st, sd)
            parts = min(-(-M // 64), mb)
            sw = gm.assert_within(dWe, r["dWe"], gm.bound_z_dwe(r, M, CIN, parts, True), name + " dWe")
            st["sum"] = max(st["sum"], sw["worst"])
            again = ext.pw_bwd_z(d["dA"], d["x"], d["We"], d["consts"], d["dout"], d["fmul"], hw or 1, mb)
            assert torch.equal(again[0], dx) and torch.equal(again[1], dWe)
        tab.add(f"{CE}x{CIN} M={M} skip hw={hw} grids={PWBWD_GRID} dx + dWe (sum = dWe)", st)


@pytest.mark.parametrize("CE,CIN", [(576, 96), (816, 136)])
@pytest.mark.parametrize("dgrad", ["z_wide", "z_gemm"])
def test_expand_bwd_z_wide(ext, CE, CIN, dgrad):
    """pw_z_prep's stored wt / mk / r0 element-wise; dx held to tight against the fp64 product of those STORED operands
    (pw_tall_tail, or gemm_tail with dgrad = z_gemm) and to bound_z_dx against the exact chain; dWe to bound_z_dwe."""
    from pytorch_rt1_for_distributed_training_amd.ops.backbone import expand_bwd_z_wide
    tab = table("expand_bwd_z_wide")
    for M, hw in [(300, None), (3001, None), (300, 100)]:
        g = gen(23, CE, M, hw or 0)
        d = expand_inputs(M, CE, CIN, g, hw)
        d["We"] = gm.weight(CE, CIN, g, 0.1, DEV)
        r = gm.ref_expand_bwd_z(d["dA"], d["x"], d["We"], d["consts"], d["dout"], d["fmul"], hw or 1)
        k1 = d["consts"][2].double()
        wt, mk, r0 = ext.pw_z_prep(d["We"], d["consts"].view(-1))
        wt_ref = (d["We"].double() * k1[:, None]).t()
        name = f"expand_bwd_z_wide {dgrad} {CE}x{CIN} M={M} hw={hw}"
        gm.assert_within(wt, wt_ref, (go.REL + go.SLACK) * wt_ref.abs(), name + " wt", S=wt_ref.abs())
        gm.assert_within(mk, r["Mk"], go.REL * r["Mk"].abs() + gm.slack(CE) * r["Mk_abs"], name + " mk", S=r["Mk_abs"])
        gm.assert_f32(r0, r["r0"], r["R"], CE, name + " r0")
        res = (d["dout"], d["fmul"], hw) if hw else None
        dx, dWe = expand_bwd_z_wide(d["dA"], d["x"], d["We"], d["consts"].view(-1), res=res, dgrad=dgrad)
        ref, S = gm.ref_gemm(d["dA"], wt, False, r0, d["x"], mk, d["dout"], d["fmul"], hw or 1)
        st = gm.assert_gemm(dx, ref, S, CE + CIN + 2, name + " dx / stored operands")      # incl. the bias of the store
        sx = gm.assert_within(dx, r["dx"], gm.bound_z_dx(r, CE, CIN, go.REL), name + " dx / exact chain")
        sw = gm.assert_within(dWe, r["dWe"], gm.bound_z_dwe(r, M, CIN, 16, False), name + " dWe")
        st["worst_hard"] = max(st["worst"], sx["worst"])
        st["sum"] = sw["worst"]
        tab.add(f"{dgrad} {CE}x{CIN} M={M} res hw={hw} (hard = exact chain, sum = dWe)", st)


# ======================================================================================================================
# proj_bwd
# ======================================================================================================================
@pytest.mark.parametrize("Cout", [24, 32, 48])
@pytest.mark.parametrize("Ce", [32, 40, 144, 288])       # 32: the 32-channel tile; 40: 40 of a 64-channel tile
def test_proj_bwd(ext, Cout, Ce):
    """(N, HW) = (1, 1): one pixel; (3, 63): a partial 64-row chunk per frame; (2, 1444): several row splits per
    frame.  The five sums and dWp element-wise against the fp64 formulas of test_proj_bwd_matches_fp32."""
    tab = table("proj_bwd")
    assert ext.proj_bwd_supported(Cout, Ce) and not ext.proj_bwd_supported(56, Ce)
    for N, HW in [(1, 1), (3, 63), (2, 1444)]:
        g = gen(24, Cout, Ce, HW)
        M = N * HW
        dy3 = gm.acts(M, Cout, g, 0.02, 0.1, DEV)
        y2 = gm.acts(M, Ce, g, 0.3, 1.5, DEV)
        Wp = gm.weight(Cout, Ce, g, Ce ** -0.5, DEV)
        gate = rows(N, Ce, g, 0.0)
        sc, sh, mu, rs = vec(Ce, g), vec(Ce, g, rand=False, std=0.2), vec(Ce, g, rand=False, std=0.1), vec(Ce, g)
        red, dW = ext.proj_bwd(dy3, y2.view(N, HW, Ce), Wp, gate, sc, sh, mu, rs)
        assert red.shape == (5, N, Ce) and dW.shape == (Cout, Ce)
        ops = gm.operands_proj_bwd(y2, sc, sh, mu, rs)
        dA = dy3.double() @ Wp.double()
        dAa = dy3.double().abs() @ Wp.double().abs()
        per = lambda t: t.view(N, HW, Ce).sum(1)
        name = f"proj_bwd Cout={Cout} Ce={Ce} N={N} HW={HW}"
        st = None
        for k, q in ((0, 0), (1, 1), (3, 2)):
            xr = ops[q][0]
            T = (dAa * xr.abs()).view(N, HW, Ce).amax(1)
            st = merge(st, gm.assert_f32(red[k], per(dA * xr), per(dAa * xr.abs()), HW * Cout + 32, f"{name} S{k}", T=T,
                                         kop=HW, fanout=1))
        for k, q in ((2, 1), (4, 2)):
            st = merge(st, gm.assert_f32(red[k], per(ops[q][1]), per(ops[q][2]), HW + 64, f"{name} S{k}", extra=go.SLACK))
        a = ops[0][0] * gate.double().repeat_interleave(HW, 0)
        wref, wsab, wT = gm.ref_wgrad(dy3, a)
        sw = gm.assert_f32(dW.t(), wref.t(), wsab.t(), M + 32, name + " dWp", T=wT.t(), kop=M)
        st["sum"] = max(st["worst_hard"], sw["worst_hard"])
        again = ext.proj_bwd(dy3, y2.view(N, HW, Ce), Wp, gate, sc, sh, mu, rs)
        assert torch.equal(again[0], red) and torch.equal(again[1], dW)
        tab.add(f"Cout={Cout} Ce={Ce} N={N} HW={HW} S0..S4 + dWp (sum = worst / hard)", st)


# ======================================================================================================================
# film_fwd, film_wgrad
# ======================================================================================================================
@pytest.mark.parametrize("M,cfg,splits,tile", [(100, 0, 1, 0), (130, 1, 3, 1), (257, 2, 3, 0)])
def test_film(ext, M, cfg, splits, tile):
    """The column-mapped fp32 product of gemm.hip (rt1_gemm_cmap) and the fp32-dy weight gradient of wgrad.hip
    (rt1_wgrad_dymap: dy rounded to bf16 at staging, its column sums taken before the rounding) at
    test_film_gpu.py's sizes [40, 40, 8, 8, 1392, 1392]."""
    from pytorch_rt1_for_distributed_training_amd.ops import backbone
    tab = table("film")
    sizes, K = [40, 40, 8, 8, 1392, 1392], 512
    N = sum(sizes)
    g = gen(25, M)
    x, w, b = gm.acts(M, K, g, device=DEV), gm.weight(N, K, g, K ** -0.5, DEV), vec(N, g, rand=False, std=0.1)
    cmap, rws = backbone._film_layout(sizes, M, x.device)
    flat = ext.film_fwd(x, K, w, b, cmap, M * N, cfg)
    add = torch.cat([torch.full((n,), 1.0 if j % 2 == 0 else 0.0) for j, n in enumerate(sizes)]).to(DEV)
    ref, sab = gm.ref_gemm(x, w, bias=b.double() + add.double())
    sab = sab - (b.double() + add.double()).abs() + b.double().abs() + add.double().abs()
    out = torch.cat([c.view(M, n) for c, n in zip(flat.split([n * M for n in sizes]), sizes)], 1)
    st = gm.assert_f32(out, ref, sab, K + 2, f"film_fwd M={M} cfg={cfg}")
    assert torch.equal(ext.film_fwd(x, K, w, b, cmap, M * N, cfg), flat)
    dflat = torch.randn(M * N, generator=g).to(DEV)
    dW, db = ext.film_wgrad(dflat, cmap, x, K, splits, tile)
    again = ext.film_wgrad(dflat, cmap, x, K, splits, tile)
    assert torch.equal(again[0], dW) and torch.equal(again[1], db)
    gy = torch.cat([c.view(M, n) for c, n in zip(dflat.split([n * M for n in sizes]), sizes)], 1)
    wref, wsab, _ = gm.ref_wgrad(gm.bf16_round(gy), x, want_T=False)
    st = merge(st, gm.assert_f32(dW, wref, wsab, M + splits, f"film_wgrad M={M} splits={splits} tile={tile}"))
    cs, ca = gm.ref_colsum(gy)
    st = merge(st, gm.assert_f32(db, cs, ca, M + splits, f"film_wgrad db M={M} splits={splits} tile={tile}"))
    tab.add(f"M={M} fwd cfg={cfg}, wgrad splits={splits} tile={tile}", st)
