"""The depthwise kernels of csrc/kernels/dw_*.hip against the fp64 oracle of tests/dw_oracle.py on every kernel route
(MI355X only): element-wise bounds on every bf16 output, derived bounds on the weight gradient and on the column sums of
the partial rows, and a bitwise repeat (every reduction here has a fixed order).

A case is listed for the route it reaches; what ext.dw_tile_info can see (tile counts, a partial last tile, the LDS size
with the centre stage) is asserted, what it cannot see is the rule stated here:
  RING        the staged map has <= DW_RING_PIX = 2000 pixels (for the stride-2 backward kernels the staged map is dy)
  strips      stride-1 forward / data gradient: 5 outputs when W % 5 == 0 and W % 4 != 0, else 4
  k5 unified  4 channels per thread on maps above DWU2_MAX_PIX = 400 pixels, else 2 channels per thread with 5-output
              strips and the LDS centre stage when W % 5 == 0 and W % 4 != 0, 4-output strips with the centre prefetch
              otherwise
  chunks      make_geo: C <= 144 whole-row, 288 -> 12 vectors, 152 -> 5 (chunks 5, 5, 5, 4), 816 / 1392 -> 8 with a
              6-vector last chunk, 2304 -> 8

Run with -s: one line per case (route, worst ratio to tight and to hard, share outside tight, mean signed ulp, worst sum
ratio) and a summary per entry point; profiles/dw_oracle_gpu.log is that output."""
import functools

import pytest
import torch

import dw_oracle as do

pytestmark = pytest.mark.gpu

RING_PIX, U2_PIX = 2000, 400
SUMMARY = {}

# (route, (N, H, W, C), stride, max_blocks, kernel sizes)
PLAIN = [
    ("ring+r4+partial-strip", (2, 21, 22, 40), 1, 64, (3, 5)),        # 462 px; 22 % 4 = 2: a 2-output last strip
    ("noring+2x2tiles+partial", (1, 45, 46, 24), 1, 64, (3, 5)),      # 2070 px > 2000; 45, 46 > 40
    ("noring+r5", (1, 46, 45, 24), 1, 64, (3, 5)),                    # 2070 px; 45 % 5 == 0, 45 % 4 != 0
    ("r5", (3, 13, 25, 48), 1, 64, (3, 5)),                           # 25 % 5 == 0, 25 % 4 != 0
    ("r5+wholerow17", (4, 10, 10, 136), 1, 64, (3, 5)),               # 10 % 5 == 0, 10 % 4 != 0
    ("cv5+tail4", (3, 19, 19, 152), 1, 64, (3, 5)),
    ("cv5+tail4", (3, 19, 19, 152), 2, 64, (3, 5)),
    ("cv12", (2, 19, 21, 288), 1, 64, (3, 5)),
    ("cv8+tail6+multitile-wg", (6, 19, 19, 816), 2, 4, (3, 5)),       # 12 tiles on 4 workgroups per chunk
    ("cv8+tail6", (8, 10, 10, 1392), 1, 8, (5,)),
    ("cv8+widest", (5, 10, 10, 2304), 1, 5, (3,)),
    ("s2-odd", (2, 17, 33, 144), 2, 64, (3, 5)),
    ("s2-even", (2, 20, 30, 144), 2, 64, (3, 5)),
    ("s2+dy-noring+3x3tiles", (1, 91, 92, 16), 2, 64, (3, 5)),        # dy map 46 x 46 = 2116 px > 2000
]
FUSED_S1 = [
    ("k3-cpt8+ring", 3, (2, 21, 22, 40), 64),
    ("k3-cpt8+noring+2x2tiles", 3, (1, 45, 46, 24), 64),
    ("k3-cpt8+cv5+tail4", 3, (3, 19, 19, 152), 64),
    ("k3-cpt8+cv12", 3, (2, 19, 21, 288), 64),
    ("k3-cpt8+widest", 3, (5, 10, 10, 2304), 5),
    ("k5-cpt4", 5, (2, 19, 22, 40), 64),                              # 418 px > 400
    ("k5-cpt4+noring+2x2tiles", 5, (1, 45, 46, 24), 64),
    ("k5-cpt2-r4", 5, (2, 20, 20, 48), 64),                           # exactly 400 px; 20 % 4 == 0
    ("k5-cpt2-r4+cv5+tail4", 5, (3, 19, 19, 152), 64),
    ("k5-cpt2-r4+cv8+tail6", 5, (4, 19, 19, 816), 16),
    ("k5-cpt2-r5-centre", 5, (4, 10, 10, 136), 64),                   # W % 5 == 0, W % 4 != 0, <= 400 px
    ("k5-cpt2-r5-centre+tiles3x5", 5, (3, 15, 25, 96), 64),
    ("k5-cpt2-r5-centre", 5, (2, 13, 15, 40), 64),
    ("k5-cpt2-r5-centre+cv8+tail6", 5, (8, 10, 10, 1392), 8),
]
FUSED_S2 = [
    ("s2-odd+ring", (2, 17, 23, 40), 64),
    ("s2-even+ring", (2, 20, 30, 144), 64),
    ("s2-odd+cv5+tail4", (3, 19, 19, 152), 64),
    ("s2-even+cv12", (2, 38, 38, 288), 2048),
    ("s2+dy-noring+3x3tiles", (1, 91, 92, 16), 64),                   # dy map 46 x 46 = 2116 px > 2000
]


def _plain_cases():
    return [pytest.param(route, shape, s, mb, k, on, id=f"{route}-{'x'.join(map(str, shape))}-k{k}-s{s}-{'on' if on else 'off'}")
            for route, shape, s, mb, ks in PLAIN for k in ks for on in (True, False)]


@pytest.fixture(scope="module")
def ext():
    from pytorch_rt1_for_distributed_training_amd import ops
    return ops.load()


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for op, v in sorted(SUMMARY.items()):
        print(f"\ndw gpu | {op:22s} | {v['cases']:3d} cases | worst/tight {v['tight']:.4f} | worst/hard {v['hard']:.4f} | "
              f"largest share outside tight {v['share']:.3g} (cap {v['cap']:.3g}) | worst sum ratio {v['sum']:.4f}")


@functools.lru_cache(maxsize=None)
def _inputs(shape, k, s):
    N, H, W, C = shape
    return do.make_inputs(N, H, W, C, k, s, 7919 * N + 131 * H + 17 * W + C + k + s, "cuda")


def _cdiv(a, b):
    return (a + b - 1) // b


def _cv(C):
    """make_geo's channel vectors per workgroup."""
    nv = C // 8
    if nv <= 18:
        return nv
    if nv == 36:
        return 12
    cv, slots8 = 8, _cdiv(nv, 8) * 8
    if slots8 * 100 > nv * 115:
        slots = slots8
        for c in range(7, 3, -1):
            if _cdiv(nv, c) * c < slots:
                slots, cv = _cdiv(nv, c) * c, c
    return cv


def _record(op, name, st=None, cap=0.0, sums=()):
    v = SUMMARY.setdefault(op, {"cases": 0, "tight": 0.0, "hard": 0.0, "share": 0.0, "cap": 0.0, "sum": 0.0})
    worst_sum = max(sums, default=0.0)
    line = f"\n{name}:"
    if st is not None:
        line += (f" worst/tight {st['worst']:.4f}, worst/hard {st['worst_hard']:.4f}, share outside tight "
                 f"{st['share']:.3g} (cap {cap:.3g}), mean signed ulp {st['mean_ulp']:+.5f} ({st['count']})")
        v["tight"] = max(v["tight"], st["worst"])
        v["hard"], v["share"], v["cap"] = max(v["hard"], st["worst_hard"]), max(v["share"], st["share"]), max(v["cap"], cap)
    if sums:
        line += f", worst sum ratio {worst_sum:.4f}"
    v["cases"] += 1
    v["sum"] = max(v["sum"], worst_sum)
    print(line)


def _same(a, b, name):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x.view(torch.int16) if x.dtype == do.BF else x, y.view(torch.int16) if y.dtype == do.BF else y), \
            f"{name}: output {i} differs between two calls (the summation orders are fixed)"


def _fwd_route(ext, route, shape, k, s, mb, rows=None):
    """The forward (and stride-1 data-gradient) tile of a case against the route it is listed for."""
    N, H, W, C = shape
    Ho, Wo = do.out_hw(H, W, k, s)
    TH, TW, lds, _ = ext.dw_tile_info(0, H, W, C, k, s, 0)
    th, tw = _cdiv(Ho, TH), _cdiv(Wo, TW)
    if "2x2tiles" in route:
        assert th >= 2 and tw >= 2 and Ho % TH and Wo % TW, (route, TH, TW)
    if "3x3tiles" in route:
        assert th >= 3 and tw >= 3 and Ho % TH and Wo % TW, (route, TH, TW)
    if "noring" in route and s == 1:
        assert H * W > RING_PIX and th >= 2 and tw >= 2
    if route.startswith("ring"):
        assert H * W <= RING_PIX
    if "r5" in route:
        assert Wo % 5 == 0 and Wo % 4 != 0
    if "partial-strip" in route:
        assert Wo % 4 != 0 and Wo % 5 != 0
    if "multitile-wg" in route:
        assert N * th * tw > mb
        if rows is not None:
            assert rows == mb              # the partial rows: one per workgroup, each looping over several tiles
    if "cv5" in route:
        assert _cv(C) == 5 and (C // 8) % 5 == 4
    if "cv12" in route:
        assert _cv(C) == 12
    if "tail6" in route:
        assert _cv(C) == 8 and (C // 8) % 8 == 6


def _bn1(d, on):
    return (d["sc1"], d["sh1"], d["mu1"], d["rs1"]) if on else (None, None, None, None)


# ---- dw_fwd ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,shape,s,mb,k,pro", _plain_cases())
def test_dw_fwd(ext, route, shape, s, mb, k, pro):
    """out = dwconv(silu(x*scale + shift)) or dwconv(x); (ps, pq) column sums against the stored output."""
    d = _inputs(shape, k, s)
    sc, sh, _, _ = _bn1(d, pro)
    run = lambda: ext.dw_fwd(d["x"], d["w"], sc, sh, 1 if pro else 0, k, s, mb)
    out, ps, pq = run()
    _same((out, ps, pq), run(), "dw_fwd")
    _fwd_route(ext, route, shape, k, s, mb, ps.shape[0])
    op = do.operand_bn_silu(d["x"], sc, sh) if pro else do.operand_raw(d["x"])
    ref, S = do.ref_fwd(op, d["w"], k, s)
    cap = do.CAP_PROLOGUE if pro else 0.0
    name = f"dw_fwd {route} {shape} k{k} s{s} pro={int(pro)}"
    st = do.assert_dw(out, ref, S, name, cap, do.flip_fwd(op, d["w"], k, s) if pro else None, k * k)
    assert out.shape[0] * out.shape[1] * out.shape[2] <= 8192
    (rs, ra), (rq, rqa) = do.ref_stats(out)
    sums = (do.assert_sums(ps.double().sum(0), rs, ra, name + " ps"), do.assert_sums(pq.double().sum(0), rq, rqa, name + " pq"))
    _record("dw_fwd pro" if pro else "dw_fwd", name, st, cap, sums)


# ---- dw_bwd_data -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,shape,s,mb,k,epi", _plain_cases())
def test_dw_bwd_data(ext, route, shape, s, mb, k, epi):
    """dx from a bf16 dy: every element within tight, with and without the producer-BN epilogue, which stores the same dx
    and sums dz = bf16(dx) * silu'(bn1(x)), dz * xhat.  Stride 1 runs dw_fwd_kernel over dy with flipped taps, stride 2
    the parity-strip kernel."""
    d = _inputs(shape, k, s)
    N, H, W, C = shape
    sc, sh, mu, rs = _bn1(d, epi)
    run = lambda: ext.dw_bwd_data(d["g"], d["w"], H, W, k, s, d["x"] if epi else None, sc, sh, mu, rs, mb)
    res = run()
    _same(res, run(), "dw_bwd_data")
    if s == 1:
        _fwd_route(ext, route, shape, k, 1, mb)
    ref, S = do.ref_bwd_data(do.operand_raw(d["g"]), d["w"], H, W, k, s)
    name = f"dw_bwd_data {route} {shape} k{k} s{s} epi={int(epi)}"
    st = do.assert_dw(res[0], ref, S, name)
    sums = ()
    if epi:
        # (1, 91, 92, 16) sums 8372 pixels, 2 % over the 8192 of the other cases: a dropped average term is 7.8 bounds
        assert N * H * W <= 8192 or shape == (1, 91, 92, 16)
        (r1, a1), (r2, a2) = do.ref_bn_partials(res[0], d["x"], sc, sh, mu, rs)
        sums = (do.assert_sums(res[1].double().sum(0), r1, a1, name + " pdz"),
                do.assert_sums(res[2].double().sum(0), r2, a2, name + " pdzx"))
    _record("dw_bwd_data s%d%s" % (s, " epi" if epi else ""), name, st, 0.0, sums)


# ---- dw_bwd_weight ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,shape,s,mb,k,pro", _plain_cases())
def test_dw_bwd_weight(ext, route, shape, s, mb, k, pro):
    """dw[c, t] = sum dy * act(x*scale + shift) over N*Ho*Wo <= 8192 terms; the operand is staged as bf16."""
    d = _inputs(shape, k, s)
    sc, sh, _, _ = _bn1(d, pro)
    run = lambda: ext.dw_bwd_weight(d["g"], d["x"], sc, sh, 1 if pro else 0, k, s, mb)
    dw = run()
    _same((dw,), (run(),), "dw_bwd_weight")
    gop = do.operand_raw(d["g"])
    assert gop[0].shape[0] * gop[0].shape[1] * gop[0].shape[2] <= 8192
    aop = do.operand_bn_silu(d["x"], sc, sh) if pro else do.operand_raw(d["x"])
    ref, sab, mab = do.ref_bwd_weight(gop, aop, k, s)
    name = f"dw_bwd_weight {route} {shape} k{k} s{s} pro={int(pro)}"
    _record("dw_bwd_weight", name, sums=(do.assert_sums(dw, ref, sab, name, mab if pro else None),))


# ---- dw_bwd_fused ----------------------------------------------------------------------------------------------------
def _fused_args(d, k, bn1, mb, variant=None):
    sc, sh, mu, rs = _bn1(d, bn1)
    a = (d["dA"], d["y2"], d["gate"], d["rb"], d["sc2"], d["sh2"], d["mu2"], d["rs2"], d["g2"], d["mdz2"], d["mdzx2"],
         d["w"], k, d["x"], sc, sh, 1 if bn1 else 0, mu, rs, mb)
    return a if variant is None else a + (variant,)


def _check_fused(ext, op, name, d, shape, k, s, bn1, args, unified):
    """dx, dW and the BN1 partials of one fused backward call; zout and res / rmul where the route has them."""
    N, H, W, C = shape
    res = ext.dw_bwd_fused(*args)
    _same(res, ext.dw_bwd_fused(*args), name)
    dyop = do.operand_dy(d)
    ref, S = do.ref_bwd_data(dyop, d["w"], H, W, k, s)
    F = do.flip_bwd_data(dyop, d["w"], H, W, k, s)
    st = do.assert_dw(res[0], ref, S, name + " dx", do.CAP_DY, F, k * k)
    # the unified kernels keep a = silu(bn1(x1)) in fp32 for the weight product, the two-pass kernel stages it as bf16
    aop = do.operand_bn_silu(d["x"], d["sc1"], d["sh1"], round=not unified) if bn1 else do.operand_raw(d["x"])
    # (1, 91, 92, 16) sums 8372 pixels in its BN1 partials, 2 % over: a dropped average term is 7.8 bounds there
    assert dyop[0].shape[0] * dyop[0].shape[1] * dyop[0].shape[2] <= 8192
    assert N * H * W <= 8192 or shape == (1, 91, 92, 16)
    rw, sab, mab = do.ref_bwd_weight(dyop, aop, k, s)
    sums = [do.assert_sums(res[1], rw, sab, name + " dw", mab)]
    if bn1:
        (r1, a1), (r2, a2) = do.ref_bn_partials(res[0], d["x"], d["sc1"], d["sh1"], d["mu1"], d["rs1"])
        sums += [do.assert_sums(res[2].double().sum(0), r1, a1, name + " pdz"),
                 do.assert_sums(res[3].double().sum(0), r2, a2, name + " pdzx")]
    _record(op, name + " dx", st, do.CAP_DY, sums)
    if unified and bn1:
        # zout: the store is bf16(dx_fp32 * silu'(bn1(x1))) and the partials sum that stored dz
        rz = ext.dw_bwd_fused(*args, zout=True)
        _same(rz, ext.dw_bwd_fused(*args, zout=True), name + " zout")
        sg = do.silu_grad(d["x"], d["sc1"], d["sh1"])
        stz = do.assert_dw(rz[0], ref * sg, S * do.silu_grad_abs(d["x"], d["sc1"], d["sh1"]), name + " dz", do.CAP_DY,
                           F * sg.abs(), k * k)
        assert torch.equal(rz[1], res[1]), name + ": zout changed the weight gradient"
        (r1, a1), (r2, a2) = do.ref_bn_partials(rz[0], d["x"], d["sc1"], d["sh1"], d["mu1"], d["rs1"], zout=True)
        _record(op + " zout", name + " dz", stz, do.CAP_DY,
                (do.assert_sums(rz[2].double().sum(0), r1, a1, name + " zout pdz"),
                 do.assert_sums(rz[3].double().sum(0), r2, a2, name + " zout pdzx")))
    if unified and not bn1 and s == 1:
        # res / rmul: dx + res * rmul[n, c] in fp32 before the one rounding of the store; same weight gradient
        rr = ext.dw_bwd_fused(*args, res=d["res"], rmul=d["rmul"])
        _same(rr, ext.dw_bwd_fused(*args, res=d["res"], rmul=d["rmul"]), name + " res")
        add = d["res"].double() * d["rmul"].double()[:, None, None, :]
        str_ = do.assert_dw(rr[0], ref + add, S + add.abs(), name + " dx+res", do.CAP_DY, F, k * k)
        assert torch.equal(rr[1], res[1]), name + ": res / rmul changed the weight gradient"
        _record(op + " res", name + " dx+res", str_, do.CAP_DY)


def _uni_route(ext, route, shape, k):
    N, H, W, C = shape
    TH, TW, lds, _ = ext.dw_tile_info(1, H, W, C, k, 1, 0)
    cv = _cv(C)
    base = (TH + k - 1) * (TW + k - 1) * cv * 16 + k * k * cv * 32 + cv * 128
    centre = TH * TW * cv * 16
    if "centre" in route:
        assert H * W <= U2_PIX and W % 5 == 0 and W % 4 != 0 and lds == base + centre, (route, lds, base, centre)
    else:
        assert lds == base, (route, lds, base)
    if "cpt2-r4" in route:
        assert H * W <= U2_PIX and (W % 5 != 0 or W % 4 == 0)
    if "cpt4" in route:
        assert H * W > U2_PIX
    if "2x2tiles" in route:
        assert _cdiv(H, TH) >= 2 and _cdiv(W, TW) >= 2 and H % TH and W % TW and H * W > RING_PIX
    if "tiles3x5" in route:
        assert (_cdiv(H, TH), _cdiv(W, TW)) == (3, 5)
    if "ring" in route and "noring" not in route:
        assert H * W <= RING_PIX


@pytest.mark.parametrize("bn1", [True, False], ids=["bn1", "plain"])
@pytest.mark.parametrize("route,k,shape,mb", [pytest.param(r, k, sh, mb, id=f"{r}-{'x'.join(map(str, sh))}")
                                              for r, k, sh, mb in FUSED_S1])
@pytest.mark.parametrize("variant", [0, 1], ids=["twopass", "unified"])
def test_dw_bwd_fused(ext, variant, route, k, shape, mb, bn1):
    """The fused stride-1 backward: dy rebuilt from (dA, y2, gate, rb, BN2 constants) while staging, then dx, dW and the
    BN1 partials; variant 0 = dw_bwd_fused_kernel (two passes), 1 = dw_bwd_uni_kernel, where `route` names the form."""
    d = _inputs(shape, k, 1)
    if variant == 1:
        _uni_route(ext, route, shape, k)
    name = f"dw_bwd_fused v{variant} {route} {shape} k{k} bn1={int(bn1)}"
    _check_fused(ext, "dw_bwd_fused v%d" % variant, name, d, shape, k, 1, bn1, _fused_args(d, k, bn1, mb, variant),
                 variant == 1)


@pytest.mark.parametrize("bn1", [True, False], ids=["bn1", "plain"])
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("route,shape,mb", [pytest.param(r, sh, mb, id=f"{r}-{'x'.join(map(str, sh))}")
                                            for r, sh, mb in FUSED_S2])
def test_dw_bwd_fused_s2(ext, route, shape, mb, k, bn1):
    """The unified stride-2 backward (dw_bwd_uni_s2_kernel) over the four parity classes; zout with BN1."""
    d = _inputs(shape, k, 2)
    N, H, W, C = shape
    Ho, Wo = do.out_hw(H, W, k, 2)
    TH, TW, _, _ = ext.dw_tile_info(1, H, W, C, k, 2, 0)
    if "3x3tiles" in route:
        assert _cdiv(H, TH) >= 3 and _cdiv(W, TW) >= 3 and H % TH and W % TW and Ho * Wo > RING_PIX
    else:
        assert Ho * Wo <= RING_PIX
    assert ("odd" in route) == bool(H % 2) or "3x3" in route
    name = f"dw_bwd_fused_s2 {route} {shape} k{k} bn1={int(bn1)}"
    _check_fused(ext, "dw_bwd_fused s2", name, d, shape, k, 2, bn1, _fused_args(d, k, bn1, mb), True)
