"""The executors of ops/linear.py, one call per plan kind, against the fp64 oracle of tests/gemm_oracle.py (its bounds,
unchanged): the smallest shapes at which the planners pick each kind, asserted first so a changed rule cannot turn a
case into a second test of another kernel."""
import dataclasses

import pytest
import torch

import gemm_oracle as gm
import glue_oracle as go

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda"


@pytest.fixture(scope="module")
def L():
    from pytorch_rt1_for_distributed_training_amd.ops import linear
    return linear


def gen(*key):
    return torch.Generator(device="cpu").manual_seed(sum(int(k) * 1000003 ** i for i, k in enumerate(key)) % 2 ** 31)


class Consts:
    """Stands where backbone.BNCtx stands: hands the statistics partials back instead of finalizing them."""

    def train_consts(self, ps, pq, count):
        return "train", ps, pq, count

    def eval_consts(self):
        return ("eval",)


def operands(M, K, N, *key):
    g = gen(M, K, N, *key)
    return gm.acts(M, K, g, device=DEV), gm.weight(N, K, g, K ** -0.5, DEV)


# (M, K, N, kind, statistics in training, rows per statistics tile): M is no multiple of the 32-row strip (skinny), of
# the wide kernel's tile, just above pw_tall's 4096 rows, one row past gemm256's 256-row tile
PRODUCTS = [(205, 24, 144, "pw_gemm", "epilogue", None), (301, 96, 576, "pw_gemm", "bn_stats", 151),
            (4100, 576, 96, "pw_tall", "bn_stats", 242), (257, 384, 1536, "g256", "epilogue", 256),
            (301, 1536, 512, "library", "bn_stats", 151)]


@pytest.mark.parametrize("M,K,N,kind,stats,rpt", PRODUCTS)
def test_product(L, M, K, N, kind, stats, rpt):
    a, w = operands(M, K, N)
    ref, S = gm.ref_gemm(a, w)
    name = f"{kind} {M}x{K}x{N}"
    # training: the product + the BN statistics
    p = L.plan_product(M, K, N, True)
    assert (p.kind, p.stats) == (kind, stats), p
    y, (mode, ps, pq, count), A = L.lin_bn(a, w, Consts(), True)
    assert (mode, count, A) == ("train", M, None) and y.shape == (M, N) and y.dtype == BF
    gm.assert_gemm(y, ref, S, K, name + " training")
    if rpt is None:
        gm.assert_stats(ps, pq, y, name, tile_index=gm.pw_tile_index(M, K, N, ps.shape[0], DEV))
    else:
        assert rpt == -(-M // ps.shape[0]) or kind == "g256"
        gm.assert_stats(ps, pq, y, name, rows_per_tile=rpt)
    # eval and the plain product: the same kernel without the statistics, except g256, which only runs with them
    p0 = L.plan_product(M, K, N)
    assert (p0.kind, p0.stats) == ("pw_gemm" if kind == "g256" else kind, "none"), p0
    y0, consts, A = L.lin_bn(a, w, Consts(), False)
    assert consts == ("eval",) and A is None
    gm.assert_gemm(y0, ref, S, K, name + " eval")
    assert torch.equal(L.lin(a, w), y0)
    # a data gradient hands the weight over as the transposed view of the stored [K, N] one: the kernels take a
    # contiguous copy (the same operand), the library another layout of the same product
    yt = L.lin(a, w.t().contiguous().t())
    gm.assert_gemm(yt, ref, S, K, name + " transposed view")
    assert kind == "library" or torch.equal(yt, y0)


def test_product_prologue(L):
    """plan_block's proj_fwd "pw_gemm": the operand silu(bn2(y2)) * gate built in the GEMM, stored or not, with the
    statistics (training) or without."""
    frames, hw, K, N = 5, 41, 144, 24
    M = frames * hw
    y2, w = operands(M, K, N, 1)
    g = gen(M, K, N, 2)
    sc, sh = (torch.rand(K, generator=g) + 0.5).to(DEV), (torch.randn(K, generator=g) * 0.3).to(DEV)
    gate = torch.rand(frames, K, generator=g).to(DEV)
    ref_a, S_a = go.ref_bn_apply(y2.view(frames, hw, K), sc, sh, 1, gate)
    for training in (True, False):
        y, consts, A = L.lin_bn(y2, w, Consts(), training, pro=(sc, sh, gate, hw, True))
        go.assert_bf16_exact(A.view(frames, hw, K), ref_a, S_a, "stored operand")
        ref, S = gm.ref_gemm(A, w)
        gm.assert_gemm(y, ref, S, K, f"prologue training={training}")
        if training:
            assert consts[0] == "train" and consts[3] == M
            gm.assert_stats(consts[1], consts[2], y, "prologue", tile_index=gm.pw_tile_index(M, K, N, consts[1].shape[0], DEV))
        else:
            assert consts == ("eval",)
        y1, _, none = L.lin_bn(y2, w, Consts(), training, pro=(sc, sh, gate, hw, False))
        assert none is None and torch.equal(y1, y)
    with pytest.raises(ValueError):
        L.lin_bn(y2, w, Consts(), True, pro=(sc, sh, gate, hw, True), plan=L.Product("library"))


@pytest.mark.parametrize("M,K,N,nn,kind", [(1100, 512, 512, True, "gemm_hip"), (1100, 512, 1024, True, "gemm_hip"),
                                           (1100, 1024, 512, False, "library"), (1000, 512, 512, True, "library")])
def test_token_product(L, M, K, N, nn, kind):
    assert L.plan_token_product(M, K, N, nn).kind == kind
    a, w = operands(M, K, N, 3)
    ref, S = gm.ref_gemm(a, w)
    out = L.proj(a, w.t().contiguous(), True) if nn else L.proj(a, w)
    gm.assert_gemm(out, ref, S, K, f"proj {kind} {M}x{K}x{N} nn={nn}")


# (M, Co, Ci, plan): a _WGRAD_TILE entry with two splits, the automatic MFMA pick, the batched split-K with S = 2 and
# one leftover row, and channels that are no multiple of 8 for the single mm
WGRADS = [(2200, 96, 96, ("mfma", 1, 2)), (1000, 144, 24, ("mfma_auto", -1, 0)), (4101, 816, 136, ("bmm", -1, 2)),
          (301, 20, 12, ("mm", -1, 0))]


@pytest.mark.parametrize("M,Co,Ci,plan", WGRADS)
def test_wgrad(L, M, Co, Ci, plan):
    p = L.plan_wgrad(M, Co, Ci)
    assert dataclasses.astuple(p) == (*plan, "none"), p
    g = gen(M, Co, Ci, 4)
    dy, x = gm.acts(M, Co, g, 0.1, device=DEV), gm.acts(M, Ci, g, device=DEV)
    ref, sab, _ = gm.ref_wgrad(dy, x, want_T=False)
    name = f"wgrad {plan} {M}x{Co}x{Ci}"
    out = L.wgrad(dy, x)
    assert out.shape == (Co, Ci) and out.dtype == torch.float32
    gm.assert_f32(out, ref, sab, M + 16, name)
    gm.assert_f32(L.wgrad(dy, x, final=True), ref, sab, M + 16, name + " final")
    raw = L.wgrad(dy, x, raw=True)
    assert raw.dim() == 3 and raw.shape[1:] == (Co, Ci) and raw.is_contiguous()
    if plan[0] in ("mfma", "bmm"):
        assert raw.shape[0] == plan[2]
    gm.assert_f32(raw.double().sum(0), ref, sab, M + 16, name + " raw")
    if plan[0] == "bmm":            # the leftover row is in the first split only
        rows = M // plan[2]
        r1, s1, _ = gm.ref_wgrad(dy[rows:2 * rows], x[rows:2 * rows], want_T=False)
        gm.assert_f32(raw[1], r1, s1, rows, name + " second split")


@pytest.mark.parametrize("M,C,flags,plan", [(2200, 96, {}, ("mfma", 1, 2, "kernel")), (1000, 40, {}, ("mfma_auto", -1, 0, "kernel")),
                                            (2200, 96, {"gram_sx": False}, ("mfma", 1, 2, "colsum")),
                                            (4101, 384, {}, ("bmm", -1, 2, "colsum"))])
def test_gram(L, M, C, flags, plan):
    p = L.plan_wgrad(M, C, C, dataclasses.replace(L.FLAGS, **{"wgrad_mfma": True, "gram_sx": True, **flags}), gram=True)
    assert dataclasses.astuple(p) == plan, p
    x = gm.acts(M, C, gen(M, C, 5), device=DEV)
    G, sx = L.gram_moments(x, plan=p)
    ref, sab, _ = gm.ref_wgrad(x, x, want_T=False)
    gm.assert_f32(G, ref, sab, M + 16, f"gram {plan}")
    cs, ca = gm.ref_colsum(x)
    gm.assert_f32(sx, cs, ca, M + 16, f"gram {plan} sx")


@pytest.mark.parametrize("M,Co,Ci,bias,plan", [(1500, 512, 64, False, ("mfma", 1, 2, "none")),
                                               (2200, 2048, 64, True, ("mfma", 2, 2, "kernel")),
                                               (301, 20, 12, False, ("mm", -1, 0, "none")),
                                               (301, 20, 12, True, ("mm", -1, 0, "colsum"))])
def test_token_wgrad(L, M, Co, Ci, bias, plan):
    if not L.TF_WGRAD:
        plan = ("mm", -1, 0, "colsum" if bias else "none")
    assert dataclasses.astuple(L.plan_token_wgrad(M, Co, Ci, bias)) == plan
    g = gen(M, Co, Ci, 6)
    dy, x = gm.acts(M, Co, g, 0.1, device=DEV), gm.acts(M, Ci, g, device=DEV)
    ref, sab, _ = gm.ref_wgrad(dy, x, want_T=False)
    name = f"token wgrad {plan} {M}x{Co}x{Ci}"
    if bias:
        dW, db = L.token_wgrad(dy, x, bias=True)
        cs, ca = gm.ref_colsum(dy)
        gm.assert_f32(db, cs, ca, M + 16, name + " bias")
    else:
        dW = L.token_wgrad(dy, x, True)
        gm.assert_f32(L.token_wgrad(dy, x), ref, sab, M + 16, name + " not final")
    assert dW.shape == (Co, Ci) and dW.dtype == torch.float32
    gm.assert_f32(dW, ref, sab, M + 16, name)
