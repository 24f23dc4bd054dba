"""The LAVA cross layers' language rows on csrc/kernels/lavalang.hip (ops/lava_language.py) against the layer's own
expression -- plain F.layer_norm, F.linear and relu with autograd -- in fp64 on the CPU.

Per tensor the metric is max |got - ref64| / max |ref64| and the bound is 4x the same metric of that expression in
fp32 eager on the GPU (tests/test_lava_xattn_gpu.py's rule); where the reference is identically zero the hip result
must be exactly zero.  Every output must be bitwise equal over two runs.  Both metrics are printed (pytest -s).

Tail cases: N = 1 (one row), 3 (a partial tile), 16 (one tile, one partial: no reduce), 17 (a second tile holding
one row: two partials) and 16 * cap + 17 with cap the partial count's limit read from the extension (workgroups walk
one or two tiles, the last tile holds one row).  The row LayerNorm (layer 0's ln_lang) rides along as a third output
on the same rows, so its two parameter gradients are checked with the tail's ten."""
import pytest
import torch
import torch.nn.functional as F

D = 128
PARAMS = ["wo", "bo", "gf", "bf", "w1", "b1", "w2", "b2", "ge", "be", "gl", "bl"]
EPS = 1e-5


def _inputs(n, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=gen)
    t = {"lang": 2.0 * r(n, D), "ctx": r(n, D), "dout": r(n, D), "dln": r(n, D), "dqn": r(n, D)}
    for k in ("wo", "w1", "w2"):
        t[k] = 0.1 * r(D, D)
    for k in ("bo", "b1", "b2", "bf", "be", "bl"):
        t[k] = 0.2 * r(D)
    for k in ("gf", "ge", "gl"):
        t[k] = 1.0 + 0.3 * r(D)
    return t


def _names(epi):
    params = [k for k in PARAMS if epi or k not in ("ge", "be")]
    return ["out", "qn"] + (["ln_out"] if epi else []) + ["dlang", "dctx"] + ["d" + k for k in params]


def _finish(t, leaves, out, ln_out, qn, epi, dev, dtype):
    c = lambda k: t[k].to(dev, dtype)
    loss = (out * c("dout")).sum() + (qn * c("dqn")).sum() + ((ln_out * c("dln")).sum() if epi else 0.0)
    params = [k for k in PARAMS if epi or k not in ("ge", "be")]
    grads = torch.autograd.grad(loss, [leaves[k] for k in ["lang", "ctx"] + params])
    return [x.detach().cpu() for x in [out, qn] + ([ln_out] if epi else []) + list(grads)]


def _eager(t, epi, dtype, dev, masks=None, p=0.0):
    v = {k: t[k].to(dev, dtype).requires_grad_() for k in ["lang", "ctx"] + PARAMS}
    m1, m2 = (m.to(dev, dtype) / (1.0 - p) for m in masks) if masks else (1.0, 1.0)
    x3 = v["lang"] + F.linear(v["ctx"], v["wo"], v["bo"]) * m1
    f1 = F.relu(F.linear(F.layer_norm(x3, (D,), v["gf"], v["bf"], EPS), v["w1"], v["b1"]))
    out = x3 + F.linear(f1, v["w2"], v["b2"]) * m2
    ln_out = F.layer_norm(out, (D,), v["ge"], v["be"], EPS) if epi else None
    qn = F.layer_norm(v["lang"], (D,), v["gl"], v["bl"], EPS)
    return _finish(t, v, out, ln_out, qn, epi, dev, dtype)


def _hip(t, epi, p=0.0, seed=0):
    from pytorch_rt1_for_distributed_training_amd.ops.lava_language import LavaRowNormFn, LavaTailFn
    v = {k: t[k].cuda().requires_grad_() for k in ["lang", "ctx"] + PARAMS}
    ge, be = (v["ge"], v["be"]) if epi else (None, None)
    out, ln_out = LavaTailFn.apply(v["lang"], v["ctx"], v["wo"], v["bo"], v["gf"], v["bf"], EPS, v["w1"], v["b1"],
                                   v["w2"], v["b2"], ge, be, EPS, p, seed)
    qn = LavaRowNormFn.apply(v["lang"], v["gl"], v["bl"], EPS)
    return _finish(t, v, out, ln_out, qn, epi, "cuda", torch.float32)


def _check(tag, names, ref, eag, got, again):
    failures = []
    for name, r, e, g, g2 in zip(names, ref, eag, got, again):
        assert torch.isfinite(g).all(), name
        assert torch.equal(g, g2), f"{name}: two runs differ"
        scale = float(r.abs().max())
        if scale == 0.0:
            err_e, err_g = float(e.abs().max()), float(g.abs().max())
            ok = err_g == 0.0
        else:
            err_e, err_g = float((e - r).abs().max()) / scale, float((g - r).abs().max()) / scale
            ok = err_g <= 4 * err_e
        print(f"lava_language {tag} {name:8s} max|ref|={scale:.3e} eager={err_e:.3e} hip={err_g:.3e}")
        if not ok:
            failures.append(f"{name}: hip {err_g:.3e} > bound from eager {err_e:.3e}")
    assert not failures, failures


def _sizes():
    from pytorch_rt1_for_distributed_training_amd.ops.lava_language import partials, tile_rows
    cap = partials(1 << 20)
    assert partials(16) == 1 and partials(17) == 2 and tile_rows() == 16
    return [1, 3, 16, 17, 16 * cap + 17]


@pytest.mark.gpu
@pytest.mark.parametrize("epi", [False, True], ids=["plain", "epilogue"])
@pytest.mark.parametrize("case", range(5))
def test_tail_matches_fp64(case, epi):
    n = _sizes()[case]
    t = _inputs(n, 100 + case)
    ref = _eager(t, epi, torch.float64, "cpu")
    eag = _eager(t, epi, torch.float32, "cuda")
    _check(f"tail N={n} epi={int(epi)}", _names(epi), [x.double() for x in ref], [x.double() for x in eag],
           [x.double() for x in _hip(t, epi)], [x.double() for x in _hip(t, epi)])


ATTN = ["d_in_w", "d_in_b", "d_ln_w", "d_ln_b"]


def _attn_sums(t, dtype, dev):
    """The expressions of LavaCrossAttnFn.backward."""
    Q, dQ, q, dctx, u, w, z, e, ln_w, ln_b = (t[k].to(dev, dtype) for k in
                                              ("Q", "dQ", "q", "dctx", "u", "w", "z", "e", "ln_w", "ln_b"))
    n, dh = q.shape[0], D // 2
    du, xv = (ln_w * e).view(n, 2, D), ln_w * z + ln_b
    Qh, dch = Q.view(n, 2, dh), dctx.view(n, 2, dh)
    d_wq = dQ.t() @ q
    d_wk = (dh ** -0.5) * torch.einsum("nhi,nhk->hik", Qh, du).reshape(D, D)
    d_wv = torch.einsum("nhi,nhk->hik", dch, xv).reshape(D, D)
    d_in_b = torch.cat([dQ.sum(0), torch.zeros_like(ln_b), dctx.sum(0)], 0)
    return [x.double().cpu() for x in (torch.cat([d_wq, d_wk, d_wv], 0), d_in_b, (w * z + u * e).sum((0, 1)),
                                       w.sum((0, 1)))]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 17])
def test_attention_parameter_gradients_match_fp64(n):
    from pytorch_rt1_for_distributed_training_amd.ops.lava_language import attn_param_grads
    gen = torch.Generator().manual_seed(7 + n)
    t = {k: torch.randn(n, D, generator=gen) for k in ("Q", "dQ", "q", "dctx")}
    t.update({k: torch.randn(n, 2, D, generator=gen) for k in ("u", "w", "z", "e")})
    t["ln_w"], t["ln_b"] = 1.0 + 0.3 * torch.randn(D, generator=gen), 0.3 * torch.randn(D, generator=gen)
    hip = lambda: [x.double().cpu() for x in attn_param_grads(*(t[k].cuda() for k in (
        "Q", "dQ", "q", "dctx", "u", "w", "z", "e", "ln_w", "ln_b")))]
    ref, eag, got, again = _attn_sums(t, torch.float64, "cpu"), _attn_sums(t, torch.float32, "cuda"), hip(), hip()
    assert float(got[1][D:2 * D].abs().max()) == 0.0                       # the K bias third
    _check(f"attn N={n}", ATTN, ref, eag, got, again)


@pytest.mark.gpu
def test_dropout_masks_and_backward():
    n, p = 160, 0.1                                                      # 5 sigma = 5 sqrt(p (1 - p) / (128 n)) = 0.0105
    t = _inputs(n, 42)
    got = _hip(t, True, p, 1234)
    # the masks are read off the forward's own tensors: site 0 dropped where x3 == lang, site 1 where out == x3
    from pytorch_rt1_for_distributed_training_amd.ops._ext import load
    c = {k: v.cuda() for k, v in t.items()}
    raw = lambda seed: load().lava_lang_tail_fwd(c["lang"], c["ctx"], c["wo"], c["bo"], c["gf"], c["bf"], EPS, c["w1"],
                                                 c["b1"], c["w2"], c["b2"], c["ge"], c["be"], EPS, p, seed)
    o1, _, x31, _ = raw(1234)
    o2, _, x32, _ = raw(1234)
    o3, _, x33, _ = raw(4321)
    assert torch.equal(o1.cpu(), got[0]) and torch.equal(o1, o2) and torch.equal(x31, x32)      # same seed, same bits
    m1, m2 = (x31 != c["lang"]).cpu(), (o1 != x31).cpu()
    sigma = (p * (1 - p) / (D * n)) ** 0.5
    for site, m in enumerate((m1, m2)):
        share = 1.0 - float(m.float().mean())
        print(f"lava_language dropout site {site}: dropped {share:.4f} (p = {p}, 5 sigma = {5 * sigma:.4f})")
        assert abs(share - p) <= 5 * sigma
    assert not torch.equal(m1, (x33 != c["lang"]).cpu()) and not torch.equal(m2, (o3 != x33).cpu())   # another seed
    assert not torch.equal(m1, m2)                                                                   # the two sites
    masks = (m1.double(), m2.double())
    ref = _eager(t, True, torch.float64, "cpu", masks, p)
    eag = _eager(t, True, torch.float32, "cuda", masks, p)
    _check(f"dropout N={n}", _names(True), [x.double() for x in ref], [x.double() for x in eag],
           [x.double() for x in got], [x.double() for x in _hip(t, True, p, 1234)])
