"""Every route of the decoder kernels (attention.hip, transformer.hip, head.hip) against the element-wise fp64 oracle of
tests/decoder_oracle.py: both ends of each Sp / 16 class of the attention forward and its switch from 8 to 4 waves, the
single-workgroup and the streamed backward, the partial workgroups and the grid-stride trips of the row kernels, the
three vocabulary variants of the head and its first-maximum rule on exact ties.  The dropout masks come from the integer
re-implementation of the hashes, never from a kernel.  References are fp64 on the GPU; every case also asserts a bitwise
repeat (all reductions are fixed-order).  Run with -s for one line per case and one summary per entry point
(profiles/decoder_oracle_gpu.log)."""
import pytest
import torch

import decoder_oracle as do
import gemm_oracle as gm
import glue_oracle as go

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda"
D = 128
SCALE = D ** -0.5
SEED = 77
TABLES = {}


@pytest.fixture(scope="module")
def ext():
    from pytorch_rt1_for_distributed_training_amd import ops
    yield ops.load()
    for t in TABLES.values():
        t.summary()
    print()


def table(entry):
    return TABLES.setdefault(entry, do.Table(entry))


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31)
    return torch.Generator(device="cpu").manual_seed(seed)


def counter(use):
    return torch.tensor([123457], dtype=torch.int32, device=DEV) if use else None


# ======================================================================================================================
# attention
# ======================================================================================================================
ATT_S = [1, 15, 16, 17, 32, 33, 64, 65, 66, 96, 97, 128, 129, 160, 161, 165, 192, 193, 220, 224, 225, 253, 256]


def fwd_route(S):
    """(NKB, waves) of rt1_attn_fwd: NKB = Sp / 16, 4 waves once the 8-wave LDS image passes 160 KB."""
    Sp = (S + 31) // 32 * 32
    return Sp // 16, 4 if (Sp * D * 2 + 8 * 16 * Sp) * 2 > 160 * 1024 else 8


def attn_case(ext, S, L, K, p, B=2, H=8, use_ctr=True):
    g = gen(S, L, K, int(p * 100), B, H)
    qkv = torch.randn(B, S, 3, H, D, generator=g).to(BF).to(DEV)
    dout = torch.randn(B, S, H, D, generator=g).to(BF).to(DEV)
    ctr = counter(use_ctr)
    nkb, waves = fwd_route(S)
    name = f"B{B} H{H} S{S} L{L} K{K} p{p} ctr{int(use_ctr)} NKB{nkb} waves{waves}"
    out, lse = ext.attn_fwd(qkv, L, K, SCALE, p, SEED, ctr)
    out2, lse2 = ext.attn_fwd(qkv, L, K, SCALE, p, SEED, ctr)
    assert torch.equal(out, out2) and torch.equal(lse, lse2), f"{name}: the forward does not repeat bitwise"
    keep = do.attn_keep(SEED, ctr, B * H, S, p, DEV) if p > 0 else None
    r = do.ref_attn_fwd(qkv, L, K, SCALE, p, keep)
    st = table("attn_fwd").add(name, do.check_attn_fwd(out, lse, r, "attn_fwd " + name))
    assert st["count"] < go.BIAS_MIN_COUNT or st["bias_cap"] <= gm.BIAS_CAP_MAX, \
        f"{name}: the bias statistic of a bias-sized case is not asserted (cap {st['bias_cap']:.3f})"
    rb = do.ref_attn_bwd(qkv, out, lse, dout, L, K, SCALE, p, keep)
    got = {}
    if S <= 96:
        got["attn_bwd"] = ext.attn_bwd
    got["attn_bwd_long"] = ext.attn_bwd_long
    for entry, fn in got.items():
        dq = fn(qkv, out, dout, lse, L, K, SCALE, p, SEED, ctr)
        assert torch.equal(dq, fn(qkv, out, dout, lse, L, K, SCALE, p, SEED, ctr)), \
            f"{name}: {entry} does not repeat bitwise"
        table(entry).add(name, do.check_attn_bwd(dq, rb, f"{entry} {name}"))
        if S % L == 0 and 0 < K < L:
            # no query attends to the action tokens of the last step: their dK / dV bounds are exactly 0
            assert not rb["hard"][:, S - (L - K):, 1:].any() and not dq[:, S - (L - K):, 1:].any(), \
                f"{entry} {name}: dK / dV of the trailing action tokens are not exact zeros"
        got[entry] = dq
    return out, lse, got


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", ATT_S)
def test_attention_every_class(ext, S, p):
    """(L, Kimg) = (11, 8) at both ends of every Sp / 16 class and at the switch to 4 waves; the forward oracle runs
    first, then attn_bwd (S <= 96) and attn_bwd_long on the same case."""
    attn_case(ext, S, 11, 8, p)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", [66, 165, 253])
def test_attention_sequence_not_a_multiple_of_the_step(ext, S, p):
    attn_case(ext, S, 7, 4, p)


@pytest.mark.parametrize("S", [66, 165])
def test_attention_pure_causal(ext, S):
    """Kimg = L: no action tokens, the mask is causal only."""
    attn_case(ext, S, 11, 11, 0.1)


@pytest.mark.parametrize("S", [66, 165])
def test_attention_fully_masked(ext, S):
    """Kimg = 0: every token is an action token, every row is fully masked: exact zeros and -inf."""
    out, lse, got = attn_case(ext, S, 11, 0, 0.1)
    assert not out.any() and bool((lse == float("-inf")).all())
    for entry, dq in got.items():
        assert not dq.any(), entry


@pytest.mark.parametrize("S", [66, 165])
def test_attention_host_seed_only(ext, S):
    """seed_dev None: the mask of the host seed alone."""
    attn_case(ext, S, 11, 8, 0.1, use_ctr=False)


def test_attention_three_heads_three_batches(ext):
    """H = 3, B = 3: bh / H and bh % H differ from every power-of-two layout."""
    attn_case(ext, 66, 11, 8, 0.1, B=3, H=3)


@pytest.mark.parametrize("S", [66, 256])
@pytest.mark.parametrize("use_ctr", [True, False])
def test_attn_keepmask_is_the_integer_hash(ext, S, use_ctr):
    """BH = 16: S = 66 in one pass, S = 256 past the 4096-workgroup cap of the grid-stride loop."""
    like = torch.empty(1, device=DEV)
    ctr = counter(use_ctr)
    keep = ext.attn_keepmask(16, S, 0.1, SEED, like, ctr)
    assert torch.equal(keep, ext.attn_keepmask(16, S, 0.1, SEED, like, ctr))
    ref = do.attn_keep(SEED, ctr, 16, S, 0.1, DEV)
    assert keep.shape == ref.shape and torch.equal(keep.bool(), ref), \
        f"{int((keep.bool() != ref).sum())} of {ref.numel()} keep bits differ"
    assert 0.88 < ref.double().mean().item() < 0.92
    blocks = (16 * S * S + 255) // 256
    print(f"\ndecoder oracle | attn_keepmask | BH16 S{S} ctr{int(use_ctr)} workgroups {min(blocks, 4096)} of {blocks} | "
          f"bit-equal, kept {ref.double().mean().item():.4f}", end="")


# ======================================================================================================================
# transformer.hip row kernels
# ======================================================================================================================
TF_T = [1, 3, 4, 5, 2047, 2048, 2049, 2051, 4100]


def rows_inputs(T):
    g = gen(T, 512)
    scale = 10.0 ** (torch.rand(T, 1, generator=g) * 2 - 1)               # per-row scale 0.1 .. 10
    d = {"x": (torch.randn(T, 512, generator=g) + 0.3) * scale,           # non-zero mean
         "a": (torch.randn(T, 512, generator=g) * scale).to(BF),
         "bias": torch.randn(512, generator=g) * 0.1,
         "g": torch.rand(512, generator=g) + 0.5, "b": torch.randn(512, generator=g) * 0.1,
         "dy": torch.randn(T, 512, generator=g).to(BF), "dres": torch.randn(T, 512, generator=g),
         "dout": torch.randn(T, 512, generator=g) * scale}
    return {k: v.to(DEV).contiguous() for k, v in d.items()}


def trips(T):
    wg = (T + 3) // 4
    return f"T{T} workgroups {min(wg, 512)} trips {(wg + 511) // 512}"


@pytest.mark.parametrize("T", TF_T)
def test_tf_ln_fwd_and_resid(ext, T):
    d = rows_inputs(T)
    y, mu, rs = ext.tf_ln_fwd(d["x"], d["g"], d["b"], 1e-6)
    y2, mu2, rs2 = ext.tf_ln_fwd(d["x"], d["g"], d["b"], 1e-6)
    assert torch.equal(y, y2) and torch.equal(mu, mu2) and torch.equal(rs, rs2)
    st = do.check_ln_fwd(y, mu, rs, do.ref_ln_fwd(d["x"], d["g"], d["b"], 1e-6), f"ln_fwd T{T}")
    table("tf_ln_fwd").add(trips(T), st)
    ctr = counter(True)
    for p in (0.0, 0.1):
        keep = do.row_keep(SEED, ctr, T, p, DEV) if p > 0 else None
        ref, S = do.ref_resid(d["x"], d["a"], d["bias"], p, keep)
        for ln in (False, True):
            name = f"{trips(T)} p{p} ln{int(ln)}"
            res = ext.tf_resid(d["x"], d["a"], d["bias"], p, SEED, ctr, d["g"] if ln else None, d["b"] if ln else None,
                               1e-6)
            again = ext.tf_resid(d["x"], d["a"], d["bias"], p, SEED, ctr, d["g"] if ln else None,
                                 d["b"] if ln else None, 1e-6)
            assert len(res) == (4 if ln else 1) and all(torch.equal(u, v) for u, v in zip(res, again)), name
            st = gm.assert_f32(res[0], ref, S, 5, "resid " + name)
            if ln:
                # the LayerNorm of the row just formed: the reference takes the STORED fp32 out
                st = do.merge(st, do.check_ln_fwd(res[1], res[2], res[3], do.ref_ln_fwd(res[0], d["g"], d["b"], 1e-6),
                                                  "resid " + name))
            table("tf_resid").add(name, st)
    # the zero pattern of x = 0, bias = 0, a = 1 is the mask itself
    zero = torch.zeros(T, 512, device=DEV)
    (pat,) = ext.tf_resid(zero, torch.ones(T, 512, device=DEV).to(BF), torch.zeros(512, device=DEV), 0.1, SEED, ctr)
    keep = do.row_keep(SEED, ctr, T, 0.1, DEV)
    assert torch.equal(pat != 0, keep), f"T{T}: {int(((pat != 0) != keep).sum())} mask bits differ from row_keep"
    (pat0,) = ext.tf_resid(zero, torch.ones(T, 512, device=DEV).to(BF), torch.zeros(512, device=DEV), 0.1, SEED, None)
    assert torch.equal(pat0 != 0, do.row_keep(SEED, None, T, 0.1, DEV)), f"T{T}: host-seed mask differs"


@pytest.mark.parametrize("T", TF_T)
def test_tf_ln_bwd_and_drop_bwd(ext, T):
    d = rows_inputs(T)
    _, mu, rs = ext.tf_ln_fwd(d["x"], d["g"], d["b"], 1e-6)
    for dres in (None, d["dres"]):
        r = do.ref_ln_bwd(d["dy"], d["x"], mu, rs, d["g"], dres)
        for want_bf in (False, True):
            name = f"{trips(T)} dres{int(dres is not None)} bf{int(want_bf)}"
            res = ext.tf_ln_bwd(d["dy"], d["x"], mu, rs, d["g"], dres, want_bf)
            again = ext.tf_ln_bwd(d["dy"], d["x"], mu, rs, d["g"], dres, want_bf)
            assert len(res) == (5 if want_bf else 3) and all(torch.equal(u, v) for u, v in zip(res, again)), name
            st = do.check_ln_bwd(res[0], res[1], res[2], r, T, "ln_bwd " + name, *(res[3:] if want_bf else ()))
            table("tf_ln_bwd").add(name, st)
    ctr = counter(True)
    for p in (0.0, 0.1):
        name = f"{trips(T)} p{p}"
        keep = do.row_keep(SEED, ctr, T, p, DEV) if p > 0 else None
        dh, dsum = ext.tf_drop_bwd(d["dout"], p, SEED, ctr)
        dh2, dsum2 = ext.tf_drop_bwd(d["dout"], p, SEED, ctr)
        assert torch.equal(dh, dh2) and torch.equal(dsum, dsum2), name
        ref, cs, ca = do.ref_drop_bwd(d["dout"], p, keep)
        if p > 0:
            assert torch.equal(dh != 0, keep & (d["dout"] != 0)), f"{name}: the zero pattern is not row_keep"
        st = gm.assert_gemm(dh, ref, ref.abs(), 1, "drop_bwd " + name)
        st = do.merge(st, gm.assert_f32(dsum, cs, ca, T, "drop_bwd sums " + name, extra=do.SLACK))
        table("tf_drop_bwd").add(name, st)


# ======================================================================================================================
# head.hip
# ======================================================================================================================
HEAD_R = {1: (1, 1), 15: (3, 5), 16: (2, 8), 17: (1, 17), 90: (5, 18)}      # R = B * P
HEAD_S = 22


def head_inputs(V, R, g):
    B, P = HEAD_R[R]
    hidden = torch.randn(B, HEAD_S, 512, generator=g)
    W = (torch.randn(V, 512, generator=g) * 0.05).to(BF)
    bias = torch.randn(V, generator=g) * 0.2
    pos = torch.randperm(HEAD_S, generator=g)[:P]
    target = torch.randint(0, V, (R,), generator=g)
    if P >= 2:
        pos[0], pos[1] = HEAD_S - 1, 0          # both ends of the sequence, out of order
        target[0], target[-1] = V - 1, 0
    else:
        pos[0] = HEAD_S - 1 if V > 256 else 0
        target[0] = V - 1 if V == 512 else 0
    return (hidden.to(DEV), pos.int().to(DEV), W.to(DEV), bias.to(DEV), target.int().to(DEV)), (B, P)


@pytest.mark.parametrize("R", sorted(HEAD_R))
@pytest.mark.parametrize("V", [256, 512, 1024])
def test_head_ce_every_vocabulary(ext, V, R):
    assert ext.head_ce_supported(V, 512)
    g = gen(V, R)
    (hidden, pos, W, bias, target), (B, P) = head_inputs(V, R, g)
    name = f"V{V} NT{V // 64} R{R} = B{B} x P{P}"
    ce, pred, G, hb = ext.head_ce_fwd(hidden, pos, W, bias, target)
    again = ext.head_ce_fwd(hidden, pos, W, bias, target)
    assert all(torch.equal(u, v) for u, v in zip((ce, pred, G, hb), again)), f"{name}: no bitwise repeat"
    assert torch.equal(hb, hidden[:, pos.long()].reshape(R, 512).to(BF)), f"{name}: hb is not bf16(hidden[b, pos[p]])"
    r = do.ref_head(hb, W, bias, target)
    st = do.check_f32(ce, r["ce"], r["bound_ce"], "head ce " + name)
    st = do.merge(st, do.check_bf16(G, r["G"], r["bound_G"], "head G " + name, None, r["S_G"]))
    clear = r["clear"]
    assert torch.equal(pred.long()[clear], r["pred"][clear]), f"{name}: argmax differs on a row without a near tie"
    dce = (torch.rand(R, generator=g) + 0.5).to(DEV)
    dz = ext.head_ce_scale(G, dce)
    assert torch.equal(dz, ext.head_ce_scale(G, dce))
    ref = G.double() * dce.double()[:, None]
    st = do.merge(st, gm.assert_gemm(dz, ref, ref.abs(), 1, "head_ce_scale " + name))
    table("head_ce").add(f"{name} clear rows {int(clear.sum())}", st)


@pytest.mark.parametrize("V", [256, 512, 1024])
@pytest.mark.parametrize("where", ["same lane", "same wave", "other wave"])
def test_head_argmax_takes_the_first_of_an_exact_tie(ext, V, where):
    """Two columns c1 < c2 with identical W rows and the same large bias are every row's maximum, bit for bit: pred is
    c1.  same lane: c2 = c1 + 16 (the strict > of the lane's own tiles); same wave: another lane of the wave (the
    shuffle's `oi < ix`); other wave: the cross-wave pass in column order."""
    g = gen(V, len(where))
    (hidden, pos, W, bias, target), _ = head_inputs(V, 17, g)
    c1 = 5
    c2 = {"same lane": c1 + 16, "same wave": c1 + 16 + 3, "other wave": c1 + 3 * (V // 4) + 7}[where]
    assert (c1 // (V // 4) == c2 // (V // 4)) == (where != "other wave")
    W[c2] = W[c1]
    bias[c1] = bias[c2] = 50.0
    ce, pred, G, hb = ext.head_ce_fwd(hidden, pos, W, bias, target)
    r = do.ref_head(hb, W, bias, target)
    top = r["z"].argmax(1)
    assert torch.equal(W[c1], W[c2]) and bool(((top == c1) | (top == c2)).all())
    assert bool((pred == c1).all()), f"V{V} {where}: pred {pred.tolist()} on an exact tie of columns {c1} and {c2}"
    do.check_f32(ce, r["ce"], r["bound_ce"], f"head ce tie V{V} {where}")
    do.check_bf16(G, r["G"], r["bound_G"], f"head G tie V{V} {where}", None, r["S_G"])
    print(f"\ndecoder oracle | head_ce tie   | V{V} {where}: columns {c1} and {c2} | pred == {c1} on every row", end="")
