"""fp64 references and the element-wise oracle for the stem kernels (csrc/kernels/stem.hip).

Plain torch, CPU or GPU tensors, no extension call.  img [N, 3, H, W] uint8 or fp32, w [40, 27] fp32 (tap = ci * 9 + kh *
3 + kw), shift (dy, dx) or None; out [N, Ho, Wo, 40] bf16 with Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, ps / pq
[grid, 40] fp32, dW [40, 27] fp32.

What the kernels round and where, read from stem.hip and cited by line:
  * Operands are exact.  uint8: `(float)v * (1.f / 255.f)` (to_unit, win_store: `(float)((b >> (8 * j)) & 255u) *
    (1.f / 255.f)`) then pack2 / f2bf: the staged value is TABLE[v] = bf16(fp32(v) * fp32(1 / 255)), formed here with the
    same two fp32 operations.  (All 256 bytes give the same bf16 under fp32 multiply by 1 / 255 and fp32 divide by 255:
    tests/test_stem_oracle.py.)  float: `inb[rowi * IWP + c] = f2bf(v)`: bf16(img).  Weights: `wa[nb][j] = f2bf(w[co *
    27 + 8 * lg + j])`.  The window is p(y, x) = img[y + dy][x + dx] where (y, x) and (y + dy, x + dx) are both inside
    the frame, else 0 (stage_window_bf16; win_load / win_store build the same values from aligned dword pairs).
  * forward: one `__builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[nb], bfr, 0)` per 16 channels: 27 exact products (and 5
    zero taps) added in fp32, `pack2(acc[0], acc[1])` the one store: gemm_oracle's tight bound with K = 27.
  * BN partials: `f = bf2f(f2bf(acc[i])); s[nb][i] += f; q[nb][i] = fmaf(f, f, q[nb][i])` for live pixels only (`live =
    oh < Ho && ow < Wo`), then 4 waves x 16 lanes in order: sums of the STORED values over the tiles the workgroup
    owns, tile t = (n tiles_h + th) tiles_w + tw, owner t % grid (`for (t = blockIdx.x; t < ntiles; t += gridDim.x)`):
    gemm_oracle.assert_stats with tile_index.
  * weight gradient: `acc[cb][tb] = ...mfma...(afr, bfr[tb], acc[cb][tb], 0, 0, 0)` with the pixels as the reduction
    axis, 4 waves summed in order (`a += red[(wv * 48 + co) * 32 + tap]`), one partial row per workgroup summed on the
    host side of the binding: an fp32 sum of N Ho Wo exact products, n = N Ho Wo + grid + 4.
  * BN-backward prologue (BN = true): `dz = g * silu_grad(fmaf(xv, scale, shift)); o[j] = fmaf(k1, dz, fmaf(k2, xv,
    k0))`, pack2: bn_bwd_apply's operations and rounding; held bitwise to bn_bwd_apply + the plain kernel (bn_bwd_apply
    itself is under glue_oracle).
"""
import torch
import torch.nn.functional as F

import gemm_oracle as gm

BF = torch.bfloat16
TOH, TOW, COUT, TAPS = 12, 32, 40, 27


def table():
    """bf16(fp32(v) * fp32(1 / 255)) for the 256 byte values, as fp64."""
    r = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(255.0, dtype=torch.float32)
    return (torch.arange(256, dtype=torch.float32) * r).to(BF).double()


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def tiles_hw(H, W):
    Ho, Wo = out_hw(H, W)
    return (Ho + TOH - 1) // TOH, (Wo + TOW - 1) // TOW


def grid(N, H, W, max_blocks):
    th, tw = tiles_hw(H, W)
    return max(1, min(N * th * tw, max_blocks))


def route(img, W):
    """`float`, `vec` (uint8, 4-byte aligned base, W % 4 == 0: dword pairs, software-pipelined) or `bytes`."""
    if img.dtype != torch.uint8:
        return "float"
    return "vec" if img.data_ptr() % 4 == 0 and W % 4 == 0 else "bytes"


def shifted(x, shift):
    """p[..., y, x] = x[..., y + dy, x + dx], zero outside; any dtype, any shift."""
    dy, dx = (0, 0) if shift is None else shift
    H, W = x.shape[-2:]
    out = torch.zeros_like(x)
    ya, yb, xa, xb = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if ya < yb and xa < xb:
        out[..., ya:yb, xa:xb] = x[..., ya + dy:yb + dy, xa + dx:xb + dx]
    return out


def operand(img, shift):
    """The exact staged window values [N, 3, H, W] fp64 of the shifted frame."""
    if img.dtype == torch.uint8:
        p = table().to(img.device)[img.long()]
    else:
        p = gm.bf16_round(img)
    return shifted(p, shift)


def patches(p):
    """[N Ho Wo, 27] fp64: the 27 taps of every output pixel (3 x 3, stride 2, pad 1), tap = ci * 9 + kh * 3 + kw."""
    N = p.shape[0]
    u = F.unfold(p, 3, padding=1, stride=2)              # [N, 27, Ho Wo]
    return u.transpose(1, 2).reshape(-1, TAPS)


def ref_fwd(img, shift, w):
    """out [N Ho Wo, 40] -> (ref, S, P) with P the patches (the weight gradient's operand)."""
    P = patches(operand(img, shift))
    wq = gm.bf16_round(w.view(COUT, TAPS))
    return P @ wq.t(), P.abs() @ wq.abs().t(), P


def tile_index(N, H, W, g, device="cpu"):
    """Workgroup that owns each output pixel, [N Ho Wo]."""
    Ho, Wo = out_hw(H, W)
    th, tw = tiles_hw(H, W)
    n = torch.arange(N, device=device)[:, None, None]
    oh = torch.arange(Ho, device=device)[None, :, None]
    ow = torch.arange(Wo, device=device)[None, None, :]
    return (((n * th + oh // TOH) * tw + ow // TOW) % g).reshape(-1)


def check_fwd(img, shift, w, max_blocks, outs, name):
    """stem_fwd's out (every element, tight, K = 27) and its BN partial rows; an all-zero window must give exact zeros."""
    out, ps, pq = outs
    N, _, H, W = img.shape
    g = grid(N, H, W, max_blocks)
    assert ps.shape == pq.shape == (g, COUT), (name, ps.shape, g)
    ref, S, P = ref_fwd(img, shift, w)
    o2 = out.reshape(-1, COUT)
    st = gm.assert_gemm(o2, ref, S, TAPS, name + " out")
    if not P.any():
        assert not o2.any() and not ps.any() and not pq.any(), f"{name}: an empty window must give exact zeros"
    st["sum"] = gm.assert_stats(ps, pq, o2, name, tile_index=tile_index(N, H, W, g, out.device))
    return st, P


def check_wgrad(dw, dy, P, n_extra, name):
    """dW [40, 27] against the fp64 sum over all pixels of dy[px, co] P[px, tap]; n_extra = grid + 4."""
    ref, sab, _ = gm.ref_wgrad(dy.reshape(-1, COUT), P, want_T=False)
    return gm.assert_f32(dw, ref, sab, P.shape[0] + n_extra, name + " dW")
