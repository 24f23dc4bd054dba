"""Numerics of the fused HIP image encoder vs plain PyTorch fp32 references (MI355X only)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def ext():
    from pytorch_rt1_for_distributed_training_amd import ops
    return ops.load()


def rel_err(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-12))


@pytest.mark.parametrize("k,s,C,H,W,prologue,N,mb", [(3, 1, 40, 20, 30, False, 3, 64), (3, 2, 144, 17, 33, True, 3, 64),
                                                     (5, 1, 24, 12, 20, True, 3, 64), (5, 2, 192, 19, 19, True, 3, 64),
                                                     (3, 1, 2304, 5, 7, True, 3, 64), (5, 1, 136, 9, 9, False, 3, 64),
                                                     # multi-tile workgroups: the software-pipelined staging path
                                                     (5, 1, 1392, 10, 10, True, 40, 8), (3, 1, 576, 19, 19, False, 20, 8),
                                                     (5, 2, 816, 19, 19, True, 16, 4), (3, 1, 2304, 10, 10, True, 24, 5),
                                                     # widths divisible by 5 but not 4: 5-output strips (DW_R5_MASK)
                                                     (5, 1, 48, 13, 25, True, 3, 64), (3, 1, 40, 30, 150, False, 2, 64)])
def test_dwconv_fwd_bwd(ext, k, s, C, H, W, prologue, N, mb):
    torch.manual_seed(0)
    x = torch.randn(N, H, W, C, device="cuda").to(BF)
    w = torch.randn(C, 1, k, k, device="cuda") * 0.3
    scale = (torch.rand(C, device="cuda") + 0.5) if prologue else None
    shift = (torch.randn(C, device="cuda") * 0.2) if prologue else None
    act = 1 if prologue else 0
    out, ps, pq = ext.dw_fwd(x, w.view(C, k * k), scale, shift, act, k, s, mb)
    # reference
    xr = x.float().permute(0, 3, 1, 2).requires_grad_(False)
    a = F.silu(xr * scale[None, :, None, None] + shift[None, :, None, None]) if prologue else xr
    a = a.detach().requires_grad_(True)
    ref = F.conv2d(a, w, stride=s, padding=(k - 1) // 2, groups=C)
    assert out.shape == (N,) + tuple(ref.shape[2:]) + (C,)
    assert rel_err(out.permute(0, 3, 1, 2), ref) < 1e-2
    ref_bf = out.float()
    torch.testing.assert_close(ps.sum(0), ref_bf.sum((0, 1, 2)), rtol=1e-3, atol=1e-2)
    torch.testing.assert_close(pq.sum(0), (ref_bf ** 2).sum((0, 1, 2)), rtol=1e-3, atol=1e-2)
    # backward
    g = torch.randn_like(ref)
    ref.backward(g)
    gb = g.permute(0, 2, 3, 1).contiguous().to(BF)
    (dx,) = ext.dw_bwd_data(gb, w.view(C, k * k), H, W, k, s, None, None, None, None, None, mb)
    assert rel_err(dx.permute(0, 3, 1, 2), a.grad) < 1e-2
    # fused producer-BN backward epilogue: stores dx unchanged, and emits partial sums of
    # dz = dx * silu'(y*scale+shift) and dz * xhat for the producing BatchNorm's backward
    y_in = torch.randn(N, H, W, C, device="cuda").to(BF)
    sc2, sh2 = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.2
    mu2, rs2 = torch.randn(C, device="cuda") * 0.1, torch.rand(C, device="cuda") + 0.5
    dx2, pdz, pdzx = ext.dw_bwd_data(gb, w.view(C, k * k), H, W, k, s, y_in, sc2, sh2, mu2, rs2, mb)
    assert torch.equal(dx2, dx)
    u = y_in.float() * sc2 + sh2
    sg = torch.sigmoid(u)
    dz_ref = dx.float() * sg * (1 + u * (1 - sg))
    xhat = (y_in.float() - mu2) * rs2
    torch.testing.assert_close(pdz.sum(0), dz_ref.sum((0, 1, 2)), rtol=2e-3, atol=2e-2)
    torch.testing.assert_close(pdzx.sum(0), (dz_ref * xhat).sum((0, 1, 2)), rtol=2e-3, atol=2e-2)
    dw = ext.dw_bwd_weight(gb, x, scale, shift, act, k, s, mb)
    wr = w.clone().requires_grad_(True)
    F.conv2d(a.detach(), wr, stride=s, padding=(k - 1) // 2, groups=C).backward(g)
    assert rel_err(dw, wr.grad.view(C, k * k)) < 1e-2


@pytest.mark.parametrize("k,C,H,W,N,expand,mb", [(3, 40, 20, 30, 3, False, 64), (3, 24, 17, 23, 2, False, 64),
                                                  (3, 192, 19, 21, 3, True, 64), (5, 288, 13, 11, 4, True, 64),
                                                  (5, 1392, 10, 10, 6, True, 8), (3, 2304, 10, 10, 5, True, 5),
                                                  (5, 816, 19, 19, 4, True, 16), (3, 576, 19, 19, 8, True, 2048),
                                                  (3, 192, 75, 75, 2, True, 2048), (5, 1392, 10, 10, 40, True, 64),
                                                  (5, 96, 15, 25, 3, True, 64), (5, 40, 9, 15, 2, False, 64)])
@pytest.mark.parametrize("variant", [0, 1])
def test_dw_bwd_fused(ext, k, C, H, W, N, expand, mb, variant):
    """dw_bwd_fused (BN2 backward-apply prologue + stride-1 data and weight gradients in one kernel) against the
    unfused kernel sequence and a plain fp32 PyTorch reference; variant 0 = two-pass kernel, 1 = unified kernel."""
    torch.manual_seed(0)
    dev = "cuda"
    dA = torch.randn(N, H, W, C, device=dev).to(BF)
    y2 = (torch.randn(N, H, W, C, device=dev) * 1.5).to(BF)
    gate, rb = torch.rand(N, C, device=dev), torch.randn(N, C, device=dev) * 0.1
    sc2, sh2 = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.2
    mu2, rs2, g2 = torch.randn(C, device=dev) * 0.1, torch.rand(C, device=dev) + 0.5, torch.rand(C, device=dev) + 0.5
    mdz2, mdzx2 = torch.randn(C, device=dev) * 0.05, torch.randn(C, device=dev) * 0.05
    w = torch.randn(C, k * k, device=dev) * 0.3
    x1 = torch.randn(N, H, W, C, device=dev).to(BF)
    if expand:
        sc1, sh1 = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.2
        mu1, rs1, act = torch.randn(C, device=dev) * 0.1, torch.rand(C, device=dev) + 0.5, 1
    else:
        sc1 = sh1 = mu1 = rs1 = None
        act = 0
    res = ext.dw_bwd_fused(dA, y2, gate, rb, sc2, sh2, mu2, rs2, g2, mdz2, mdzx2, w, k, x1, sc1, sh1, act, mu1, rs1, mb,
                           variant)
    # unfused kernel sequence
    dy2 = ext.bn_bwd_apply(dA.view(-1, C), gate, rb, H * W, y2, sc2, sh2, mu2, rs2, g2, 1, mdz2, mdzx2).view(N, H, W, C)
    un = ext.dw_bwd_data(dy2, w, H, W, k, 1, x1 if expand else None, sc1, sh1, mu1, rs1, mb)
    dw_u = ext.dw_bwd_weight(dy2, x1, sc1, sh1, act, k, 1, mb)
    assert rel_err(res[0], un[0]) < 1e-2
    assert rel_err(res[1], dw_u) < 5e-3
    if expand:
        torch.testing.assert_close(res[2].sum(0), un[1].sum(0), rtol=1e-2, atol=1e-1)
        torch.testing.assert_close(res[3].sum(0), un[2].sum(0), rtol=1e-2, atol=1e-1)
    # fp32 reference of the whole chain
    yf = y2.float()
    u = yf * sc2 + sh2
    sg = torch.sigmoid(u)
    dz = (dA.float() * gate[:, None, None, :] + rb[:, None, None, :]) * sg * (1 + u * (1 - sg))
    k1 = g2 * rs2
    dy_ref = k1 * dz - k1 * rs2 * mdzx2 * yf - k1 * (mdz2 - mu2 * rs2 * mdzx2)
    a1 = F.silu(x1.float() * sc1 + sh1) if expand else x1.float()
    a1r = a1.permute(0, 3, 1, 2).detach().requires_grad_(True)
    wr = w.view(C, 1, k, k).clone().requires_grad_(True)
    F.conv2d(a1r, wr, padding=(k - 1) // 2, groups=C).backward(dy_ref.permute(0, 3, 1, 2))
    assert rel_err(res[0].permute(0, 3, 1, 2), a1r.grad) < 2e-2
    assert rel_err(res[1], wr.grad.view(C, k * k)) < 2e-2
    if expand:
        v = x1.float() * sc1 + sh1
        s1 = torch.sigmoid(v)
        dz1 = a1r.grad.permute(0, 2, 3, 1) * s1 * (1 + v * (1 - s1))
        torch.testing.assert_close(res[2].sum(0), dz1.sum((0, 1, 2)), rtol=3e-2, atol=0.5)
        if variant == 1:
            _check_zout(ext, res, (dA, y2, gate, rb, sc2, sh2, mu2, rs2, g2, mdz2, mdzx2, w, k, x1, sc1, sh1, act, mu1,
                                   rs1, mb, variant))


@pytest.mark.parametrize("k,C,H,W,N", [(3, 24, 30, 30, 3), (5, 40, 10, 10, 4)])
def test_dw_bwd_fused_residual_epilogue(ext, k, C, H, W, N):
    """res / rmul: the unified kernel's plain store adds the residual path's gradient res * rmul[n, c] (block 1's
    dout * FiLM multiplier) before rounding to bf16; same weight gradient as without it."""
    torch.manual_seed(0)
    dev = "cuda"
    dA = torch.randn(N, H, W, C, device=dev).to(BF)
    y2 = torch.randn(N, H, W, C, device=dev).to(BF)
    gate, rb = torch.rand(N, C, device=dev), torch.randn(N, C, device=dev) * 0.1
    sc2, sh2 = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.2
    mu2, rs2, g2 = torch.randn(C, device=dev) * 0.1, torch.rand(C, device=dev) + 0.5, torch.rand(C, device=dev) + 0.5
    mdz2, mdzx2 = torch.randn(C, device=dev) * 0.05, torch.randn(C, device=dev) * 0.05
    w = torch.randn(C, k * k, device=dev) * 0.3
    x1 = torch.randn(N, H, W, C, device=dev).to(BF)
    r = torch.randn(N, H, W, C, device=dev).to(BF)
    rmul = torch.rand(N, C, device=dev) + 0.5
    args = (dA, y2, gate, rb, sc2, sh2, mu2, rs2, g2, mdz2, mdzx2, w, k, x1, None, None, 0, None, None, 64, 1)
    plain = ext.dw_bwd_fused(*args)
    fused = ext.dw_bwd_fused(*args, res=r, rmul=rmul)
    ref = plain[0].float() + r.float() * rmul[:, None, None, :]
    assert rel_err(fused[0], ref) < 5e-3
    assert torch.equal(fused[1], plain[1])


def _check_zout(ext, res, args):
    """zout=True stores dz = dx * silu'(bn1(x1)) (the pw_bwd_z operand) instead of dx; same weight gradient and BN1
    partials."""
    x1, sc1, sh1 = args[13], args[14], args[15]
    rz = ext.dw_bwd_fused(*args, zout=True)
    v = x1.float() * sc1 + sh1
    s1 = torch.sigmoid(v)
    assert rel_err(rz[0], res[0].float() * s1 * (1 + v * (1 - s1))) < 1e-2
    assert torch.equal(rz[1], res[1])
    # bf16(dx) * silu' vs bf16(dx * silu'): the same sums up to one bf16 rounding per element
    torch.testing.assert_close(rz[2].sum(0), res[2].sum(0), rtol=3e-2, atol=0.5)
    torch.testing.assert_close(rz[3].sum(0), res[3].sum(0), rtol=3e-2, atol=0.5)


@pytest.mark.parametrize("k,C,H,W,N,expand,mb", [(3, 144, 20, 30, 3, True, 64), (5, 192, 19, 19, 3, True, 64),
                                                  (3, 288, 38, 38, 2, True, 2048), (5, 816, 19, 19, 4, True, 16),
                                                  (3, 40, 17, 23, 2, False, 64), (5, 24, 13, 11, 3, False, 64),
                                                  (3, 144, 150, 150, 1, True, 2048)])
def test_dw_bwd_fused_s2(ext, k, C, H, W, N, expand, mb):
    """Unified stride-2 depthwise backward (dw_bwd_uni_s2_kernel: BN2 backward-apply prologue, data and weight
    gradients over the four parity classes in one pass) against the unfused kernel sequence and fp32 PyTorch."""
    torch.manual_seed(0)
    dev = "cuda"
    Ho, Wo = (H + 2 * ((k - 1) // 2) - k) // 2 + 1, (W + 2 * ((k - 1) // 2) - k) // 2 + 1
    dA = torch.randn(N, Ho, Wo, C, device=dev).to(BF)
    y2 = (torch.randn(N, Ho, Wo, C, device=dev) * 1.5).to(BF)
    gate, rb = torch.rand(N, C, device=dev), torch.randn(N, C, device=dev) * 0.1
    sc2, sh2 = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.2
    mu2, rs2, g2 = torch.randn(C, device=dev) * 0.1, torch.rand(C, device=dev) + 0.5, torch.rand(C, device=dev) + 0.5
    mdz2, mdzx2 = torch.randn(C, device=dev) * 0.05, torch.randn(C, device=dev) * 0.05
    w = torch.randn(C, k * k, device=dev) * 0.3
    x1 = torch.randn(N, H, W, C, device=dev).to(BF)
    if expand:
        sc1, sh1 = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.2
        mu1, rs1, act = torch.randn(C, device=dev) * 0.1, torch.rand(C, device=dev) + 0.5, 1
    else:
        sc1 = sh1 = mu1 = rs1 = None
        act = 0
    res = ext.dw_bwd_fused(dA, y2, gate, rb, sc2, sh2, mu2, rs2, g2, mdz2, mdzx2, w, k, x1, sc1, sh1, act, mu1, rs1, mb)
    assert res[0].shape == x1.shape
    dy2 = ext.bn_bwd_apply(dA.view(-1, C), gate, rb, Ho * Wo, y2, sc2, sh2, mu2, rs2, g2, 1, mdz2, mdzx2)
    dy2 = dy2.view(N, Ho, Wo, C)
    un = ext.dw_bwd_data(dy2, w, H, W, k, 2, x1 if expand else None, sc1, sh1, mu1, rs1, mb)
    dw_u = ext.dw_bwd_weight(dy2, x1, sc1, sh1, act, k, 2, mb)
    assert rel_err(res[0], un[0]) < 1e-2
    assert rel_err(res[1], dw_u) < 5e-3
    if expand:
        torch.testing.assert_close(res[2].sum(0), un[1].sum(0), rtol=1e-2, atol=1e-1)
        torch.testing.assert_close(res[3].sum(0), un[2].sum(0), rtol=1e-2, atol=1e-1)
    a1 = F.silu(x1.float() * sc1 + sh1) if expand else x1.float()
    a1r = a1.permute(0, 3, 1, 2).detach().requires_grad_(True)
    wr = w.view(C, 1, k, k).clone().requires_grad_(True)
    F.conv2d(a1r, wr, stride=2, padding=(k - 1) // 2, groups=C).backward(dy2.float().permute(0, 3, 1, 2))
    assert rel_err(res[0].permute(0, 3, 1, 2), a1r.grad) < 2e-2
    assert rel_err(res[1], wr.grad.view(C, k * k)) < 2e-2
    if expand:
        _check_zout(ext, res, (dA, y2, gate, rb, sc2, sh2, mu2, rs2, g2, mdz2, mdzx2, w, k, x1, sc1, sh1, act, mu1, rs1,
                               mb, -1))


@pytest.mark.parametrize("N,C,S,HW", [(768, 40, 10, 22500), (768, 2304, 96, 100), (1536, 2304, 96, 100), (37, 816, 34, 361),
                                       (768, 144, 6, 5625), (5, 24, 6, 9)])
def test_se_fused(ext, N, C, S, HW):
    """se_fwd / se_bwd (the whole squeeze-excitation MLP and its backward glue) against fp32 PyTorch."""
    torch.manual_seed(0)
    dev = "cuda"
    pool_sum = torch.randn(N, C, device=dev) * HW * 0.3
    w1, b1 = torch.randn(S, C, device=dev) * C ** -0.5, torch.randn(S, device=dev) * 0.1
    w2, b2 = torch.randn(C, S, device=dev) * S ** -0.5, torch.randn(C, device=dev) * 0.1
    pool, h, gate = ext.se_fwd(pool_sum, 1.0 / HW, w1, b1, w2, b2)
    pr = pool_sum / HW
    hr = pr @ w1.t() + b1
    gr = torch.sigmoid(F.silu(hr) @ w2.t() + b2)
    assert pool.data_ptr() == pool_sum.data_ptr()          # the frame sums are kept (the backward scales by 1/HW)
    torch.testing.assert_close(h, hr, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(gate, gr, rtol=1e-4, atol=1e-5)
    red = torch.randn(5, N, C, device=dev)
    count = float(N * HW)
    dw2, db2, dw1, db1, rb, sdz, sdzx, mdz, mdzx = ext.se_bwd(red, gate, h, pool, 1.0 / HW, w1, w2, count)
    g = gate.double()
    dz = red[0].double() * g * (1 - g)
    hd = h.double()
    sg = torch.sigmoid(hd)
    dh = (dz @ w2.double()) * sg * (1 + hd * (1 - sg))
    rbr = (dh @ w1.double()) / HW
    r = red.double()
    sdz_r = (g * r[1] + rbr * r[2]).sum(0)
    sdzx_r = (g * r[3] + rbr * r[4]).sum(0)
    tol = dict(rtol=2e-4, atol=2e-4)
    torch.testing.assert_close(dw2.double(), dz.t() @ (hd * sg), **tol)
    torch.testing.assert_close(db2.double(), dz.sum(0), **tol)
    torch.testing.assert_close(dw1.double(), dh.t() @ pr.double(), **tol)
    torch.testing.assert_close(db1.double(), dh.sum(0), **tol)
    torch.testing.assert_close(rb.double(), rbr, **tol)
    torch.testing.assert_close(sdz.double(), sdz_r, **tol)
    torch.testing.assert_close(sdzx.double(), sdzx_r, **tol)
    torch.testing.assert_close(mdz.double(), sdz_r / count, **tol)
    torch.testing.assert_close(mdzx.double(), sdzx_r / count, **tol)
    # bitwise reproducible (fixed summation orders)
    again = ext.se_bwd(red, gate, h, pool, 1.0 / HW, w1, w2, count)
    assert all(torch.equal(a, b) for a, b in zip(again, (dw2, db2, dw1, db1, rb, sdz, sdzx, mdz, mdzx)))


@pytest.mark.parametrize("M,C", [(5000, 144), (3001, 1392), (2000, 2304), (4099, 816)])
def test_batchnorm_train_fwd_bwd(ext, M, C):
    torch.manual_seed(0)
    y = (torch.randn(M, C, device="cuda") * 2 + 0.5).to(BF)
    gamma = torch.rand(C, device="cuda") + 0.5
    beta = torch.randn(C, device="cuda")
    rm = torch.zeros(C, device="cuda")
    rv = torch.ones(C, device="cuda")
    ps, pq = ext.bn_stats(y, 37)
    sc, sh, mu, rs = ext.bn_finalize(ps, pq, float(M), gamma, beta, 1e-5, 0.1, rm, rv)
    out = ext.bn_apply(y, sc, sh, 1, None, 0)
    bn = torch.nn.BatchNorm2d(C).cuda()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    yr = y.float().view(M, C, 1, 1).requires_grad_(True)
    ref = F.silu(bn(yr))
    assert rel_err(out, ref.view(M, C)) < 1e-2
    torch.testing.assert_close(rm, bn.running_mean, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(rv, bn.running_var, rtol=1e-4, atol=1e-5)
    g = torch.randn(M, C, device="cuda")
    ref.backward(g.view(M, C, 1, 1))
    gb = g.to(BF)
    pa, pb = ext.bn_bwd_reduce(gb, None, None, 0, y, sc, sh, mu, rs, 1, 11)
    dg = torch.zeros(C, device="cuda")
    db = torch.zeros(C, device="cuda")
    mdz, mdzx = ext.bn_bwd_finalize(pa, pb, float(M), dg, db)
    dy = ext.bn_bwd_apply(gb, None, None, 0, y, sc, sh, mu, rs, gamma, 1, mdz, mdzx)
    assert rel_err(dy, yr.grad.view(M, C)) < 2e-2
    assert rel_err(dg, bn.weight.grad) < 1e-2
    assert rel_err(db, bn.bias.grad) < 1e-2


@pytest.mark.parametrize("u8,N,H,W,mb", [(True, 3, 37, 50, 64), (False, 3, 37, 50, 64), (True, 4, 64, 100, 2)])
def test_stem_with_shift(ext, u8, N, H, W, mb):
    torch.manual_seed(0)
    img = torch.randint(0, 256, (N, 3, H, W), device="cuda", dtype=torch.uint8)
    imgf = img.float() / 255.0
    w = torch.randn(40, 3, 3, 3, device="cuda") * 0.3
    dy, dx = -2, 3
    shift = torch.tensor([dy, dx], dtype=torch.int32, device="cuda")
    out, ps, pq = ext.stem_fwd(img if u8 else imgf, shift, w.view(40, 27), mb)
    from pytorch_rt1_for_distributed_training_amd.models.preprocess import shift_images
    xs = shift_images(imgf, dy, dx)
    wr = w.clone().requires_grad_(True)
    ref = F.conv2d(xs, wr, stride=2, padding=1)
    assert rel_err(out.permute(0, 3, 1, 2), ref) < 1e-2
    g = torch.randn_like(ref)
    ref.backward(g)
    dw = ext.stem_bwd_weight(img if u8 else imgf, shift, g.permute(0, 2, 3, 1).contiguous().to(BF), mb)
    assert rel_err(dw, wr.grad.view(40, 27)) < 1e-2


@pytest.mark.parametrize("shift", [(0, 0), (-5, -7), (3, 6), (7, -1), (-2, 13)])
def test_stem_vector_window_staging(ext, shift):
    """uint8 frames with W % 4 == 0 on a 4-byte aligned base are staged 4 columns per dword pair; a 1-byte offset copy
    of the same frames takes the element-wise path: forward, BN partials and the weight gradient must be bitwise
    equal, for positive and negative shifts (window columns on both frame edges)."""
    torch.manual_seed(1)
    N, H, W = 3, 36, 100
    img = torch.randint(0, 256, (N, 3, H, W), device="cuda", dtype=torch.uint8)
    raw = torch.empty(img.numel() + 1, device="cuda", dtype=torch.uint8)
    mis = raw[1:].view(N, 3, H, W)
    mis.copy_(img)
    assert mis.data_ptr() % 4 != 0 and img.data_ptr() % 4 == 0
    w = torch.randn(40, 27, device="cuda") * 0.3
    sh = torch.tensor(list(shift), dtype=torch.int32, device="cuda")
    a = ext.stem_fwd(img, sh, w, 64)
    b = ext.stem_fwd(mis, sh, w, 64)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    g = torch.randn(N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 40, device="cuda").to(BF)
    assert torch.equal(ext.stem_bwd_weight(img, sh, g, 64), ext.stem_bwd_weight(mis, sh, g, 64))


@pytest.mark.parametrize("u8,N,H,W", [(True, 3, 40, 56), (False, 2, 33, 47)])
def test_stem_wgrad_bn_backward_prologue(ext, u8, N, H, W):
    """bn_x / constants: the stem weight-gradient kernel rebuilds dy = bn_bwd_apply(g, x) while staging (block 0's
    stem BN backward, StemLink); bitwise equal to the bn_bwd_apply pass followed by the plain kernel."""
    torch.manual_seed(0)
    dev = "cuda"
    img = torch.randint(0, 256, (N, 3, H, W), device=dev, dtype=torch.uint8)
    img = img if u8 else img.float() / 255.0
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = torch.randn(N, Ho, Wo, 40, device=dev).to(BF)
    x = torch.randn(N, Ho, Wo, 40, device=dev).to(BF)
    sc, sh = torch.rand(40, device=dev) + 0.5, torch.randn(40, device=dev) * 0.2
    mu, rs, gam = torch.randn(40, device=dev) * 0.1, torch.rand(40, device=dev) + 0.5, torch.rand(40, device=dev) + 0.5
    mdz, mdzx = torch.randn(40, device=dev) * 0.05, torch.randn(40, device=dev) * 0.05
    shift = torch.tensor([1, -2], dtype=torch.int32, device=dev)
    dy = ext.bn_bwd_apply(g.view(-1, 40), None, None, 0, x.view(-1, 40), sc, sh, mu, rs, gam, 1, mdz, mdzx)
    ref = ext.stem_bwd_weight(img, shift, dy.view(N, Ho, Wo, 40).contiguous(), 64)
    fused = ext.stem_bwd_weight(img, shift, g, 64, x, sc, sh, mu, rs, gam, mdz, mdzx)
    assert torch.equal(fused, ref)


def _seeded(model, seed=1234):
    from tools.make_reference_golden import seeded_init
    seeded_init(model, seed)
    for m in model.modules():
        if type(m).__name__ == "StochasticDepth":
            m.p = 0.0
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0


def test_fused_encoder_matches_eager_fp32(ext):
    """Whole image tokenizer (stem, 26 MBConv+FiLM, top, conv1x1, FiLM, TokenLearner): forward tokens and
    parameter gradients vs the eager fp32 module.  A 26-block BN network amplifies bf16 rounding, so the
    criterion is relative: the fused bf16 path must be no worse than PyTorch's own bf16 autocast path
    (plus a small margin); BN running statistics must match closely."""
    import copy
    import pytorch_rt1_for_distributed_training_amd as rt1
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    from pytorch_rt1_for_distributed_training_amd.ops.fused_model import FusedRT1
    torch.manual_seed(0)
    cfg = rt1.RT1Config(height=96, width=128, seq_len=2, num_layers=1, dtype="bf16", backend="hip",
                        channels_last=False)
    ref = build_rt1(cfg).cuda()
    for m in ref.modules():   # drop-path masks are random: disable
        if type(m).__name__ == "StochasticDepth":
            m.p = 0.0
    amp = copy.deepcopy(ref)
    fused = copy.deepcopy(ref)
    fused.fused = FusedRT1(fused, cfg)
    for m_ in (ref, amp, fused):
        m_.train()
    b, t = 2, 2
    img = torch.randint(0, 256, (b, t, 3, 96, 128), device="cuda", dtype=torch.uint8)
    ctx = torch.randn(b, t, 512, device="cuda")
    tok_ref = ref.tokenize_images(img.float() / 255.0, ctx, shift=(3, -5))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        tok_amp = amp.tokenize_images(img.float() / 255.0, ctx, shift=(3, -5))
    tok_fused = fused.tokenize_images(img, ctx, shift=(3, -5))
    assert tok_fused.shape == tok_ref.shape == (b, t, 8, 512)
    e_fused, e_amp = rel_err(tok_fused, tok_ref), rel_err(tok_amp, tok_ref)
    print(f"encoder fwd rel err: fused {e_fused:.4f}  torch-bf16 {e_amp:.4f}")
    assert e_fused < 1.5 * e_amp + 0.02, (e_fused, e_amp)
    gw = torch.randn_like(tok_ref)
    for tok in (tok_ref, tok_amp, tok_fused):
        (tok.float() * gw).sum().backward()
    pr = dict(ref._image_tokenizer.named_parameters())
    pa = dict(amp._image_tokenizer.named_parameters())
    # Per parameter, the fused error is judged against the autocast error.  Both are single noisy samples
    # (a few frames; autocast itself is not bit-reproducible run to run), so: no parameter may be far
    # worse, and the typical ratio must stay near 1.  Parameters whose fp32 gradient is pure cancellation
    # noise (a conv bias feeding a BatchNorm: the true gradient is 0, autocast error > 100%) are skipped.
    worse, ratios = [], []
    for n, p in fused._image_tokenizer.named_parameters():
        if pr[n].grad is None:
            continue
        assert p.grad is not None, n
        ef, ea = rel_err(p.grad, pr[n].grad), rel_err(pa[n].grad, pr[n].grad)
        if ea > 1.0:
            continue
        ratios.append((ef + 0.01) / (ea + 0.01))
        if ef > 3.0 * ea + 0.05:
            worse.append((n, round(ef, 4), round(ea, 4)))
    assert not worse, worse[:20]
    ratios.sort()
    print(f"encoder grad err ratio fused/autocast: median {ratios[len(ratios) // 2]:.3f} max {ratios[-1]:.3f}")
    assert ratios[len(ratios) // 2] < 1.3, ratios[len(ratios) // 2]
    br = dict(ref._image_tokenizer.named_buffers())
    for n, bf in fused._image_tokenizer.named_buffers():
        if n.endswith("running_var"):
            assert rel_err(bf, br[n]) < 5e-2, n
        elif n.endswith("running_mean"):   # means can be ~0: compare on the scale of the running std
            sd = br[n[:-len("running_mean")] + "running_var"].sqrt()
            assert bool(((bf - br[n]).abs() <= 0.05 * sd + 1e-4).all()), n


# RouteFlags overrides of the per-block test below: the default route of every block, and the flag sets whose routes
# run the unfused depthwise sequence, the two-pass kernel, pw_bwd over y1, the library SE and the stored-A project
# backward.  tests/test_routes.py holds each set's route table and checks that together they reach every value of
# every BlockRoute stage at BLOCKS_NHW.
ROUTE_FLAG_SETS = {"default": {}, "dw_fused=0": {"dw_fused": False}, "dw_variant=0": {"dw_variant": 0},
                   "se_fused=0": {"se_fused": False}, "pw_pro=0": {"pw_pro": False}}
BLOCKS_NHW = (4, 48, 64)


@pytest.mark.parametrize("flag_set", list(ROUTE_FLAG_SETS))
def test_fused_mbconv_blocks_individually(ext, flag_set):
    """Each of the 26 MBConv(+FiLM) blocks on the SAME bf16 input as its eager fp32 oracle, on the route plan_block
    gives it under each flag set of ROUTE_FLAG_SETS."""
    import dataclasses
    from pytorch_rt1_for_distributed_training_amd.models.efficientnet import FiLMEfficientNet
    from pytorch_rt1_for_distributed_training_amd.ops.backbone import FLAGS, BlockMeta, BNCtx, MBConvFn, plan_block
    flags = dataclasses.replace(FLAGS, **ROUTE_FLAG_SETS[flag_set])
    torch.manual_seed(0)
    net = FiLMEfficientNet().cuda()
    _seeded(net)
    net.train()
    N, H, W = BLOCKS_NHW
    ctx = torch.randn(N, 512, device="cuda")
    x = torch.randn(N, 40, H, W, device="cuda")
    errs = []
    for i, (blk, film) in enumerate(zip(net.blocks, net.films)):
        xin = x.to(BF).float().detach().requires_grad_(True)
        ref = film(blk(xin), ctx)
        gmul, gadd = film.gamma_beta(ctx)
        fmul, fadd = gmul.detach().contiguous().requires_grad_(True), gadd.detach().contiguous().requires_grad_(True)
        sp = blk.spec
        e, dw, se, pj = blk.expand, blk.depthwise, blk.se, blk.project
        bns = ([BNCtx(e[1])] if e is not None else []) + [BNCtx(dw[1]), BNCtx(pj[1])]
        xf = xin.detach().permute(0, 2, 3, 1).contiguous().to(BF).requires_grad_(True)
        out = MBConvFn.apply(xf, fmul, fadd, None, e[0].weight if e is not None else None,
                             e[1].weight if e is not None else None, e[1].bias if e is not None else None,
                             dw[0].weight, dw[1].weight, dw[1].bias, se.fc1.weight, se.fc1.bias, se.fc2.weight,
                             se.fc2.bias, pj[0].weight, pj[1].weight, pj[1].bias,
                             BlockMeta(sp, bns, True, route=plan_block(sp, N, H, W, False, flags)))
        fwd = rel_err(out.permute(0, 3, 1, 2), ref)
        g = torch.randn_like(ref)
        gx_ref, = torch.autograd.grad(ref, [xin], g, retain_graph=True)
        ref_wgrads = torch.autograd.grad(ref, [dw[0].weight, pj[0].weight], g)
        gx, gdw, gpj = torch.autograd.grad(out, [xf, dw[0].weight, pj[0].weight], g.permute(0, 2, 3, 1).contiguous())
        errs.append((i, fwd, rel_err(gx.permute(0, 3, 1, 2), gx_ref), rel_err(gdw, ref_wgrads[0]),
                     rel_err(gpj, ref_wgrads[1])))
        x = ref.detach()
        H, W = x.shape[2:]
    worst = max(errs, key=lambda e: max(e[1:]))
    print("per-block rel errors (i, fwd, dx, dWd, dWp):", [tuple(round(v, 4) if isinstance(v, float) else v
                                                                for v in e) for e in errs])
    assert max(max(e[1:]) for e in errs) < 3e-2, worst


@pytest.mark.parametrize("N,C,S", [(768, 2304, 96), (37, 144, 6), (5, 40, 10)])
def test_se_backward_glue_kernels(ext, N, C, S):
    """se.hip: the fused SE / BN2 backward glue vs the torch expressions it replaces."""
    torch.manual_seed(N + C)
    red = torch.randn(5, N, C, device="cuda")
    gate = torch.rand(N, C, device="cuda")
    h = torch.randn(N, S, device="cuda")
    dzf2 = torch.randn(N, S, device="cuda")
    rbraw = torch.randn(N, C, device="cuda")
    dz, db = ext.se_bwd_dz(red[0], gate)
    dz_ref = red[0] * gate * (1 - gate)
    torch.testing.assert_close(dz, dz_ref)
    torch.testing.assert_close(db, dz_ref.double().sum(0).float(), rtol=1e-5, atol=1e-4)
    dh, db1 = ext.se_bwd_dh(dzf2, h)
    sg = torch.sigmoid(h)
    dh_ref = dzf2 * (sg * (1 + h * (1 - sg)))
    torch.testing.assert_close(dh, dh_ref, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(db1, dh_ref.double().sum(0).float(), rtol=1e-5, atol=1e-4)
    HW, M = 361, float(N * 361)
    rb, sdz, sdzx, mdz, mdzx = ext.se_bwd_bnsum(red, gate, rbraw, 1.0 / HW, M)
    rb_ref = rbraw / HW
    torch.testing.assert_close(rb, rb_ref)
    sdz_ref = (gate.double() * red[1] + rb_ref.double() * red[2]).sum(0)
    sdzx_ref = (gate.double() * red[3] + rb_ref.double() * red[4]).sum(0)
    torch.testing.assert_close(sdz, sdz_ref.float(), rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(sdzx, sdzx_ref.float(), rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(mdz, (sdz_ref / M).float(), rtol=1e-5, atol=1e-8)
    torch.testing.assert_close(mdzx, (sdzx_ref / M).float(), rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("N,HW,Cout,Ce", [(4, 1444, 48, 288), (3, 5625, 32, 192), (2, 22500, 24, 40),
                                          (5, 361, 24, 24), (3, 5625, 32, 144)])
def test_proj_bwd_matches_fp32(ext, N, HW, Cout, Ce):
    """projbwd.hip: the SE/BN2 backward sums (through dA = dy3 @ Wp) and dWp from (dy3, y2) per frame, against fp32
    PyTorch on the same bf16 inputs.  Row splits per frame (the 22500-pixel case), padded Cout (24 -> 32) and channel
    tails (40 of a 64-channel tile) included."""
    torch.manual_seed(1)
    dev = "cuda"
    M = N * HW
    dy3 = (torch.randn(M, Cout, device=dev) * 0.1).to(torch.bfloat16)
    y2 = (torch.randn(M, Ce, device=dev) * 1.5 + 0.3).to(torch.bfloat16)
    Wp = (torch.randn(Cout, Ce, device=dev) * Ce ** -0.5).to(torch.bfloat16)
    gate = torch.rand(N, Ce, device=dev)
    sc, sh = torch.rand(Ce, device=dev) + 0.5, torch.randn(Ce, device=dev) * 0.2
    mu, rs = torch.randn(Ce, device=dev) * 0.1, torch.rand(Ce, device=dev) + 0.5
    red, dW = ext.proj_bwd(dy3, y2.view(N, HW, Ce), Wp, gate, sc, sh, mu, rs)
    y = y2.double()
    z = y * sc.double() + sh.double()
    s = torch.sigmoid(z)
    act, sg = z * s, s * (1 + z * (1 - s))
    xh = (y - mu.double()) * rs.double()
    dA = dy3.double() @ Wp.double()
    per = lambda t: t.view(N, HW, Ce).sum(1)
    ref = torch.stack([per(dA * act), per(dA * sg), per(sg), per(dA * sg * xh), per(sg * xh)])
    g = gate.double().repeat_interleave(HW, 0)
    dW_ref = dy3.double().t() @ (act * g)
    # the MFMA operands act / sg / sg*xh are bf16-rounded (2^-9 relative per element, unbiased)
    for k in range(5):
        scale = ref[k].abs().max().item()
        torch.testing.assert_close(red[k].double(), ref[k], rtol=2e-2, atol=2e-3 * scale, msg=f"red[{k}]")
    torch.testing.assert_close(dW.double(), dW_ref, rtol=2e-2, atol=2e-3 * dW_ref.abs().max().item())
    again = ext.proj_bwd(dy3, y2.view(N, HW, Ce), Wp, gate, sc, sh, mu, rs)
    assert torch.equal(again[0], red) and torch.equal(again[1], dW)      # fixed summation orders
