"""The kernels PixelLangMSE's encoder adds (csrc/kernels/lavaconv.hip, lavapix.hip) against plain torch in fp64 on the
CPU, by the rules of test_lava_conv_gpu.py: operands rounded to bf16 first, tolerance 4x the max error of the same
expression in fp32 on the GPU (A) plus 2^-8 |ref| wherever a value is stored as bf16, the backward checked as the
linear map the forward fixed (dpre built from the kernel's own idx).

First stage over s = 2, 3, 4 channel-stacked frames, Cin = 3 s: y / idx, dW, db; the beyond-cap case has 1088 tiles
against the cap of 1024 partials.  Gated stages, v = g[n, c] * (conv + b) with g = randn (negatives in every frame) and
channels 0-7 of frame 0 exactly 0: y / idx against the window max of v, zero-gate channels exactly dead, dx against the
transpose conv of the test's own operand (dy.float() * g).bfloat16(), dW / db (gate folded in fp32 per frame), dg
against sum dy * y / g from the kernel's own y and exactly 0 where g == 0.  (128, 256, 80, 7, 9) has 80 one-tile frames
against a cap of 64 partials, so the two-item walks cross a frame boundary and fold.  dW / db are bitwise equal over
two runs.  Tail: out, dy4 (bf16 store), dgate, dgamma, dbeta."""
import pytest
import torch
import torch.nn.functional as F

from test_lava_conv_gpu import EPS, SHAPES, TH, TW, _windows

FIRST = [(ci, 32, *shp) for ci in (6, 9, 12) for shp in SHAPES] + [(12, 32, 8, 8 * TH, 17 * TW)]
GATED = [(ci, co, *shp) for ci, co in [(32, 64), (64, 128), (128, 256)] for shp in SHAPES[1:]] + [(128, 256, 80, 7, 9)]


def _case(cin, cout, n, h, w):
    """Inputs (bf16-representable), the gate (None for the first stage), the fp64 gated pre-activation v, the fp64
    forward and the fp32-GPU forward error A."""
    gen = torch.Generator().manual_seed(cin * 1000 + h * 10 + n)
    if cin < 32:                                                         # frames: uint8 for n = 2, fp32 otherwise
        x = torch.randint(0, 256, (n, h, w, cin), generator=gen, dtype=torch.uint8) if n == 2 else \
            torch.rand(n, h, w, cin, generator=gen)
        xv = (x.float() / 255.0 if n == 2 else x).bfloat16()
    else:
        x = xv = torch.randn(n, h, w, cin, generator=gen).bfloat16()
    wt = (torch.randn(cout, cin, 3, 3, generator=gen) * (2.0 / (9 * cin)) ** 0.5).bfloat16().float()
    b = 0.2 * torch.randn(cout, generator=gen)
    dy = torch.randn(n, h // 2, w // 2, cout, generator=gen).bfloat16()
    g = None
    if cin >= 32:
        g = torch.randn(n, cout, generator=gen)
        g[0, :8] = 0.0
    x64 = xv.double().permute(0, 3, 1, 2).contiguous()

    def gated(dt, dev):
        v = F.conv2d(x64.to(dev, dt), wt.to(dev, dt), b.to(dev, dt), padding=1)
        return v if g is None else v * g.to(dev, dt)[:, :, None, None]

    v = gated(torch.float64, "cpu")
    ref_y = F.max_pool2d(F.relu(v), 2)
    A = 4 * float((F.max_pool2d(F.relu(gated(torch.float32, "cuda")), 2).double().cpu() - ref_y).abs().max())
    return x, wt, b, dy, g, x64, v, ref_y, A


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,n,h,w", FIRST + GATED)
def test_stage_matches_fp64(cin, cout, n, h, w):
    from pytorch_rt1_for_distributed_training_amd.ops import lava_conv as lc
    assert lc.tile() == (TH, TW)
    x, wt, b, dy, g, x64, v, ref_y, A = _case(cin, cout, n, h, w)
    hp, wp = h // 2, w // 2
    xg, wg, bg, dyg = x.cuda(), wt.cuda(), b.cuda(), dy.cuda()
    gg = None if g is None else g.cuda()
    y, idx = lc.lava_conv_fwd(xg, wg, bg) if g is None else lc.lava_conv_gated_fwd(xg, wg, bg, gg)
    assert y.dtype == torch.bfloat16 and idx.dtype == torch.uint8 and y.shape == idx.shape == (n, hp, wp, cout)
    yc, ic = y.double().cpu().permute(0, 3, 1, 2), idx.long().cpu().permute(0, 3, 1, 2)
    err = (yc - ref_y).abs()
    print(f"lava_gated fwd ({cin},{cout}) {n}x{h}x{w}: err={float(err.max()):.3e} A={A:.3e} dead={float((ic == 4).float().mean()):.2f}")
    assert bool((err <= EPS * ref_y.abs() + A).all())
    win = _windows(v, hp, wp)
    wmax, live = win.amax(-1), ic < 4
    assert int(ic.max()) <= 4
    chosen = win.gather(-1, ic.clamp(max=3)[..., None])[..., 0]
    assert bool((chosen[live] >= wmax[live] - A).all()) and bool((wmax[~live] <= A).all())
    if g is not None:                                                    # a zero gate kills the channel exactly
        assert bool((y[0, :, :, :8] == 0).all()) and bool((idx[0, :, :, :8] == 4).all())

    def route(vals):                                                     # pooled values -> dpre by the kernel's own idx
        d = torch.zeros(n, cout, hp, wp, 4, dtype=torch.float64)
        d.scatter_(-1, ic.clamp(max=3)[..., None], (vals.double().permute(0, 3, 1, 2) * live)[..., None])
        dpre = torch.zeros_like(v)
        dpre[:, :, :2 * hp, :2 * wp] = d.reshape(n, cout, hp, wp, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, cout, 2 * hp, 2 * wp)
        return dpre

    def grads(dt, dev, gout, gate):
        leaves = [t.to(dev, dt).requires_grad_() for t in (x64, wt, b)]
        out = F.conv2d(leaves[0], leaves[1], leaves[2], padding=1)
        if gate is not None:
            out = out * gate.to(dev, dt)[:, :, None, None]
        return [t.double().cpu() for t in torch.autograd.grad(out, leaves, gout.to(dev, dt))]

    dpre = route(dy)
    ref, eag = grads(torch.float64, "cpu", dpre, g), grads(torch.float32, "cuda", dpre, g)
    wgrad = (lambda: lc.lava_conv_wgrad(xg, dyg, idx)) if g is None else (lambda: lc.lava_conv_gated_wgrad(xg, dyg, idx, gg))
    (dw, db), (dw2, db2) = wgrad(), wgrad()
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    got = [("dW", dw, ref[1], eag[1], 0.0), ("db", db, ref[2], eag[2], 0.0)]
    if g is not None:
        dop = route((dy.float() * g[:, None, None, :]).bfloat16())      # the operand the kernel forms, one rounding
        dx = lc.lava_conv_gated_dgrad(dyg, idx, wg, gg, (h, w))
        assert dx.dtype == torch.bfloat16 and dx.shape == (n, h, w, cin)
        got.append(("dx", dx.permute(0, 3, 1, 2), grads(torch.float64, "cpu", dop, None)[0],
                    grads(torch.float32, "cuda", dop, None)[0], EPS))
        dg = lc.lava_conv_dgate(dyg, y, gg, cin, (h, w))
        gz = g == 0
        assert dg.shape == (n, cout) and bool((dg.cpu()[gz] == 0).all())
        gs = torch.where(gz, torch.ones_like(g), g)
        r_dg = ((dy.double() * y.double().cpu()).sum((1, 2)) / gs.double()).masked_fill(gz, 0.0)
        e_dg = ((dyg.float() * y.float()).sum((1, 2)) / gs.cuda()).double().cpu().masked_fill(gz, 0.0)
        got.append(("dg", dg, r_dg, e_dg, 0.0))
    for name, t, r, e, rel in got:
        e_hip, e_eag = (t.double().cpu() - r).abs(), float((e - r).abs().max())
        print(f"lava_gated {name} ({cin},{cout}) {n}x{h}x{w}: hip={float(e_hip.max()):.3e} eager={e_eag:.3e}")
        assert bool((e_hip <= rel * r.abs() + 4 * e_eag).all()), name


@pytest.mark.gpu
@pytest.mark.parametrize("n,hp,wp", [(1, 1, 1), (3, 4, 3), (2, 11, 20)])
def test_tail_matches_fp64(n, hp, wp):
    from pytorch_rt1_for_distributed_training_amd.ops import lava_pixel as lp
    gen = torch.Generator().manual_seed(n * 100 + hp)
    y4 = torch.randn(n, hp, wp, 256, generator=gen).abs().bfloat16()
    g = (0.25 + torch.randn(n, 256, generator=gen).abs()) * (torch.randint(0, 2, (n, 256), generator=gen) * 2 - 1)
    lw, lb, dout = 1 + 0.2 * torch.randn(256, generator=gen), torch.randn(256, generator=gen), torch.randn(n, 256, generator=gen)

    def run(dt, dev):
        leaves = [t.to(dev, dt).requires_grad_() for t in (y4, g, lw, lb)]
        out = F.layer_norm(F.relu(leaves[0].mean((1, 2)) * leaves[1]), (256,), leaves[2], leaves[3], 1e-6)
        return [t.double().cpu() for t in [out.detach()] + list(torch.autograd.grad(out, leaves, dout.to(dev, dt)))]

    ref, eag = run(torch.float64, "cpu"), run(torch.float32, "cuda")
    out, mean, stat = lp.lava_pixel_tail_fwd(y4.cuda(), g.cuda(), lw.cuda(), lb.cuda(), 1e-6)
    dy4, dgate, dgamma, dbeta = lp.lava_pixel_tail_bwd(dout.cuda(), mean, stat, g.cuda(), lw.cuda(), hp, wp)
    assert dy4.dtype == torch.bfloat16 and dy4.shape == y4.shape
    for name, t, r, e, rel in zip(("out", "dy4", "dgate", "dgamma", "dbeta"), (out, dy4, dgate, dgamma, dbeta), ref,
                                  eag, (0.0, EPS, 0.0, 0.0, 0.0)):
        e_hip, e_eag = (t.double().cpu() - r).abs(), float((e - r).abs().max())
        print(f"lava_pixel tail {name} {n}x{hp}x{wp}: hip={float(e_hip.max()):.3e} eager={e_eag:.3e}")
        assert bool((e_hip <= rel * r.abs() + 4 * e_eag).all()), name
