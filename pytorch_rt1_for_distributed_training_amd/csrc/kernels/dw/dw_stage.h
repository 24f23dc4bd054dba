// Device helpers of the depthwise kernels that every kernel unit uses: bf16 vector unpacking, the strip walk, the
// in-image rectangle of a staging window, the x-mode staging (the depthwise input recomputed from the block input on
// MFMA), the BN-backward epilogue constants, and the staging of dy rebuilt from (dA, y2).
#pragma once
#include "dw_common.h"

namespace rt1 {
namespace dw {

typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void unpack4x2(const uint4 u, f2 (&f)[4]) {
#if RT1_DW_TIMING & 1
    f[0] = f2{__uint_as_float(u.x), __uint_as_float(u.y)};
    f[1] = f2{__uint_as_float(u.y), __uint_as_float(u.z)};
    f[2] = f2{__uint_as_float(u.z), __uint_as_float(u.w)};
    f[3] = f2{__uint_as_float(u.w), __uint_as_float(u.x)};
    return;
#endif
    f[0] = f2{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u)};
    f[1] = f2{__uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
    f[2] = f2{__uint_as_float(u.z << 16), __uint_as_float(u.z & 0xffff0000u)};
    f[3] = f2{__uint_as_float(u.w << 16), __uint_as_float(u.w & 0xffff0000u)};
}

__device__ __forceinline__ void load4x2(const float* __restrict__ p, f2 (&o)[4]) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 b = *reinterpret_cast<const float4*>(p + 4);
    o[0] = f2{a.x, a.y}; o[1] = f2{a.z, a.w}; o[2] = f2{b.x, b.y}; o[3] = f2{b.z, b.w};
}

// Division-free walk over the strips grp = start, start + step, ... of a [rows x gw] strip grid, carrying two
// linear offsets (o1: LDS tile, o2: global output) with the given row / column-group strides.  The strip loops
// used `grp / groups_w` and recomputed both addresses with 32/64-bit multiplies per strip: ~30 % of the loop's
// VALU issue on the k3 layers (v_mul_lo_u32 / v_mad_u64_u32 are quarter rate).
struct StripWalk {
    int ty, gx, o1, o2;
    int dty, dgx, gw, d1, d2, w1, w2;
    __device__ __forceinline__ StripWalk(int start, int step, int gw_, int r1, int c1, int r2, int c2) {
        gw = gw_;
        ty = start / gw;
        gx = start - ty * gw;
        dty = step / gw;
        dgx = step - dty * gw;
        o1 = ty * r1 + gx * c1;
        o2 = ty * r2 + gx * c2;
        d1 = dty * r1 + dgx * c1;
        d2 = dty * r2 + dgx * c2;
        w1 = r1 - gw * c1;
        w2 = r2 - gw * c2;
    }
    __device__ __forceinline__ void next() {
        ty += dty;
        gx += dgx;
        o1 += d1;
        o2 += d2;
        if (gx >= gw) {
            gx -= gw;
            ++ty;
            o1 += w1;
            o2 += w2;
        }
    }
};

// The in-image rectangle [r0, r1) x [c0, c1) of an IH x IW staging window at (ih0, iw0) over an Hs x Ws map.  The
// staging loops walk only this rectangle (loads + prologue math on real pixels) and write the zero padding of the
// rest of the window (the "ring") with plain LDS stores: at 19 x 19 and 10 x 10, where a tile is most of a frame, the
// ring is 30-50 % of the window and used to cost the full load + BN-backward math per pixel.
// Maps above DW_RING_PIX pixels (75 x 75, 150 x 150) keep the whole-window walk with a per-pixel in-image test:
// their tiles are mostly interior (profiles/r4_dw_ring_ab.md).  The choice is a template argument, so each walk
// compiles as its own loop.
struct WinRect {
    int r0, r1, c0, c1;
    __device__ __forceinline__ WinRect(int ih0, int iw0, int IH, int IW, int Hs, int Ws)
        : r0(max(0, -ih0)), r1(max(max(0, -ih0), min(IH, Hs - ih0))), c0(max(0, -iw0)),
          c1(max(max(0, -iw0), min(IW, Ws - iw0))) {}
    __device__ __forceinline__ WinRect(int IH, int IW) : r0(0), r1(IH), c0(0), c1(IW) {}   // the whole window
    __device__ __forceinline__ int w() const { return c1 - c0; }
    __device__ __forceinline__ int npix() const { return (r1 - r0) * (c1 - c0); }
};

// zero the window pixels outside `q`: top rows, bottom rows, then the left / right columns of the middle rows.
// T = the LDS element type of one lane's vector, `lanes` vectors per pixel, this thread = vector `vv`, pixel start
// `pb` and step `PLs`
template <typename T>
__device__ __forceinline__ void zero_ring(T* tile, const WinRect& q, int IH, int IW, int lanes, int vv, int pb,
                                          int PLs, const T zero) {
    const int top = q.r0 * IW, bot = (IH - q.r1) * IW, wl = q.c0, sw = q.c0 + (IW - q.c1);
    const int n = top + bot + (q.r1 - q.r0) * sw;
    for (int i = pb; i < n; i += PLs) {
        int px;
        if (i < top) {
            px = i;
        } else if (i < top + bot) {
            px = q.r1 * IW + (i - top);
        } else {
            const int j = i - top - bot, r = j / sw, c = j - r * sw;
            px = (q.r0 + r) * IW + (c < wl ? c : q.c1 + (c - wl));
        }
        tile[px * lanes + vv] = zero;
    }
}

// ------------------------------------------------------------------ y1-free expand blocks ("x-mode")
// An expand block's depthwise input is a1 = silu(bn1(y1)) with y1 = x @ We^T, 6x wider than the block input x.
// In x-mode y1 never reaches HBM: the forward and the unified backward recompute it per staged tile from x on
// MFMA (v_mfma_f32_16x16x32_bf16, K = Cin <= 64 is one or two instructions per 16 x 16 output), and BN1's batch
// statistics come from x alone (mean(y1) = We mean(x), E[y1^2]_c = w_c^T (x^T x) w_c / M: xexpand.hip).  The
// forward's expand GEMM (write y1), the depthwise forward's read of y1 and the backward's read of y1 disappear;
// x (Cin channels) is read instead, with the tile halo.
//
// Orientation as in pwgemm.hip: C^T = We . x^T, MFMA-A = weight rows (channel c = lane & 15 of a 16-channel group),
// MFMA-B = x rows straight from HBM in operand layout (pixel = lane & 15, 8 input channels per 16-lane group), so
// each lane's accumulator holds 4 CONSECUTIVE channels of one pixel and is stored to the LDS tile as 8 bytes.
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// XK = KC * 16 + NG: KC 32-channel k chunks of x, NG 16-channel output groups (C8 = cv * 8 = NG * 16)
constexpr int xk_kc(int xk) { return xk >> 4; }
constexpr int xk_ng(int xk) { return xk & 15; }

// Write y1 (ACT: silu(bf16(y1) * sc + sh)) of the [IH x IW] pixel window at (ih0, iw0) for the chunk's channels
// [c0, c0 + nch) into LDS as bf16 [IH * IW][ldt]; pixels outside [0,H) x [0,W) are zero (the depthwise input is
// zero-padded AFTER the activation).  bnl = LDS [scale[C8], shift[C8]] (ACT only).  Each wave takes every 4th
// 16-pixel group; the next group's x fragments are loaded before the current group's MFMAs.
// LDS image of the chunk's expand-weight rows for stage_xmfma<.., WLDS = true>: [C8][KC * 32 + 8] bf16 (+16 B per
// row against bank aliasing), zero past Cin / the chunk's valid channels
template <int KC>
constexpr int xw_ld() { return KC * 32 + 8; }
template <int KC>
__device__ __forceinline__ void stage_xweights(bf16_t* __restrict__ wel, const XExp& xe, int C8, int c0, int nch) {
    constexpr int LDW = xw_ld<KC>();
    for (int i = threadIdx.x; i < C8 * KC * 4; i += BLOCK) {
        const int row = i / (KC * 4), col = (i - row * (KC * 4)) * 8;
        uint4 u = make_uint4(0, 0, 0, 0);
        if (row < nch && col < xe.cin) u = *reinterpret_cast<const uint4*>(xe.we + (int64_t)(c0 + row) * xe.cin + col);
        *reinterpret_cast<uint4*>(wel + row * LDW + col) = u;
    }
}

// WLDS: the weight fragments are read from the LDS image `wel` per MFMA (the unified backward kernels hold K x K
// weight-gradient accumulators in registers for the whole workgroup: NG * KC fragments on top spilled); otherwise
// they are loaded once per call into registers.
// ps: pixel step of the window (2 = one stride-2 parity class of the map: window (r, c) -> (ih0 + 2r, iw0 + 2c)).
// p0 / np: stage only the window's row-major pixels [p0, p0 + np) (np < 0: all), to tl rows 0 .. np-1.
template <int KC, int NG, bool ACT, bool WLDS = false>
__device__ __forceinline__ void stage_xmfma(bf16_t* __restrict__ tl, int ldt, const XExp& xe, int H, int W, int n,
                                            int ih0, int iw0, int IH, int IW, int c0, int nch,
                                            const float* __restrict__ bnl, const bf16_t* __restrict__ wel = nullptr,
                                            int ps = 1, int p0 = 0, int np = -1) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lh = lane >> 4;
    const int npix = np >= 0 ? np : IH * IW, ngrp = (npix + 15) >> 4;
    const int cin = xe.cin;
    bf16x8 wf[WLDS ? 1 : NG][KC];
    if constexpr (!WLDS) {
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) {
                const int c = g * 16 + lr, col = kc * 32 + lh * 8;
                wf[g][kc] = (c < nch && col < cin)
                                ? *reinterpret_cast<const bf16x8*>(xe.we + (int64_t)(c0 + c) * cin + col)
                                : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            }
    }
    const bf16_t* xb = xe.x + (int64_t)n * H * W * cin;
    auto load_x = [&](int grp, bf16x8 (&xf)[KC]) -> bool {
        const int p = grp * 16 + lr, pw = p0 + p;
        const int r = pw / IW, c = pw - r * IW;
        const int ih = ih0 + ps * r, iw = iw0 + ps * c;
        const bool ok = p < npix && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
            const int col = kc * 32 + lh * 8;
            xf[kc] = (ok && col < cin)
                         ? *reinterpret_cast<const bf16x8*>(xb + (uint32_t)(ih * W + iw) * (uint32_t)cin + col)
                         : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
        return ok;
    };
    int grp = wave;
    bf16x8 xc[KC], xn[KC];
    bool okc = false, okn = false;
    if (grp < ngrp) okc = load_x(grp, xc);
    for (; grp < ngrp; grp += 4) {
        if (grp + 4 < ngrp) okn = load_x(grp + 4, xn);
        const int p = grp * 16 + lr;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) {
                const bf16x8 wv = WLDS ? *reinterpret_cast<const bf16x8*>(wel + (g * 16 + lr) * xw_ld<KC>() + kc * 32 +
                                                                          lh * 8)
                                       : wf[WLDS ? 0 : g][kc];
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv, xc[kc], acc, 0, 0, 0);
            }
            const int ch = g * 16 + lh * 4;
            if (p < npix) {
                // y1 is a bf16 tensor, as when it was stored: one v_cvt_pk_bf16_f32 per channel pair
                uint2 u = make_uint2(pack2(acc[0], acc[1]), pack2(acc[2], acc[3]));
                if constexpr (ACT) {
                    // BN1 + SiLU as packed pairs, phase by phase over the two pairs (as stage_tile does): the affine,
                    // -z log2 e, +1 and z * s as v_pk_* ops around the per-element transcendentals
                    const float4 sc4 = *reinterpret_cast<const float4*>(bnl + ch);
                    const float4 sh4 = *reinterpret_cast<const float4*>(bnl + ldt + ch);
                    f2 z[2] = {f2{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u)},
                               f2{__uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)}};
                    z[0] = z[0] * f2{sc4.x, sc4.y} + f2{sh4.x, sh4.y};
                    z[1] = z[1] * f2{sc4.z, sc4.w} + f2{sh4.z, sh4.w};
                    f2 t[2];
#pragma unroll
                    for (int j = 0; j < 2; ++j) t[j] = z[j] * f2{-1.4426950408889634f, -1.4426950408889634f};
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        t[j] = f2{__builtin_amdgcn_exp2f(t[j].x), __builtin_amdgcn_exp2f(t[j].y)} + f2{1.f, 1.f};
#pragma unroll
                    for (int j = 0; j < 2; ++j) t[j] = f2{__builtin_amdgcn_rcpf(t[j].x), __builtin_amdgcn_rcpf(t[j].y)};
#pragma unroll
                    for (int j = 0; j < 2; ++j) z[j] = z[j] * t[j];
                    u = make_uint2(pack2(z[0].x, z[0].y), pack2(z[1].x, z[1].y));
                }
                if (!okc) u = make_uint2(0u, 0u);
                *reinterpret_cast<uint2*>(tl + p * ldt + ch) = u;
            }
        }
        if (grp + 4 < ngrp) {
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) xc[kc] = xn[kc];
            okc = okn;
        }
    }
}

// EPI_BNBWD constants (producer BN scale, shift, rstd and -mean*rstd) for the workgroup's cv*8 channels,
// staged once into LDS [4][cv*8] (registers would cost a wave of occupancy, per-pixel global loads cost
// 8 vector-memory instructions per output vector).
template <int EPI>
__device__ __forceinline__ void stage_epi_consts(float* ecl, const BnBwdEpi& e, int v0, int ncv, int cv) {
    if constexpr (EPI == EPI_BNBWD) {
        const int C8 = cv * 8;
        for (int i = threadIdx.x; i < C8; i += BLOCK) {
            const bool ok = i < ncv * 8;
            const int c = v0 * 8 + i;
            const float rr = ok ? e.rstd[c] : 0.f;
            ecl[i] = ok ? e.scale[c] : 0.f;
            ecl[C8 + i] = ok ? e.shift[c] : 0.f;
            ecl[2 * C8 + i] = rr;
            ecl[3 * C8 + i] = ok ? -e.mean[c] * rr : 0.f;
        }
    }
}

// A raw-buffer descriptor over [p, p + bytes): loads at offsets >= bytes return zeros (the hardware range check), so
// halo / out-of-image pixels need no branch and no pre-zeroed registers.  The inputs go through readfirstlane so the
// descriptor provably lives in SGPRs (no waterfall loop around each load).
constexpr uint32_t OOB = 0x7ffffff0u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wave_rsrc(const void* p, uint32_t bytes) {
    const uint64_t a = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    void* q = reinterpret_cast<void*>(((uint64_t)hi << 32) | lo);
    return __builtin_amdgcn_make_buffer_rsrc(q, (short)0, (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}
__device__ __forceinline__ uint4 buf_load16(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0);
    return make_uint4(v.x, v.y, v.z, v.w);
}

// stage_tile for dy: each thread owns one channel vector (its 48 constants in registers, folded per frame:
// a = k1*gate, b = k1*rb) and keeps SU pixels (2 x 16 B each) in flight.  Every pixel's two 16-B loads are issued
// unconditionally through buffer descriptors (offset OOB for halo pixels and idle channel lanes -> zeros) and the
// per-element math is packed f32 (two channels per instruction): ~half the VALU issue per element of per-pixel
// branches around scalar math.
template <int SU, bool RING>
__device__ __forceinline__ void stage_dy(uint4* tile, const DyBnBwd& d, const DwGeo& g, int n, int ih0, int iw0,
                                         int IH, int IW, int v0, int ncv) {
    const int cv = g.cv;
    const int t = threadIdx.x;
    const int vv = t % cv, PLs = BLOCK / cv;
    int pb = t / cv;
    if (pb >= PLs) return;
    const bool cvalid = vv < ncv;
    const int c0 = (v0 + (cvalid ? vv : 0)) * 8;
    // dy = (a g + b) silu'(z) + k2 y + k0,  z = y sc + sh,  silu'(z) = s (1 + z (1 - s)),  s = 1 / (1 + 2^(-z log2 e))
    f2 A[4], B[4], K2[4], K0[4], SC[4], SH[4];
    {
        float gm[8], rr[8], mu[8], mz[8], mx[8], a[8], b[8], sc[8], sh[8];
        load8f(d.gamma + c0, gm); load8f(d.rstd + c0, rr); load8f(d.mean + c0, mu);
        load8f(d.mdz + c0, mz); load8f(d.mdzx + c0, mx);
        load8f(d.gate + (int64_t)n * g.C + c0, a); load8f(d.rb + (int64_t)n * g.C + c0, b);
        load8f(d.scale + c0, sc); load8f(d.shift + c0, sh);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float k1x = gm[2 * j] * rr[2 * j], k1y = gm[2 * j + 1] * rr[2 * j + 1];
            A[j] = f2{a[2 * j] * k1x, a[2 * j + 1] * k1y};
            B[j] = f2{b[2 * j] * k1x, b[2 * j + 1] * k1y};
            K2[j] = f2{-k1x * rr[2 * j] * mx[2 * j], -k1y * rr[2 * j + 1] * mx[2 * j + 1]};
            K0[j] = f2{-k1x * (mz[2 * j] - mu[2 * j] * rr[2 * j] * mx[2 * j]),
                       -k1y * (mz[2 * j + 1] - mu[2 * j + 1] * rr[2 * j + 1] * mx[2 * j + 1])};
            SC[j] = f2{sc[2 * j], sc[2 * j + 1]};
            SH[j] = f2{sh[2 * j], sh[2 * j + 1]};
        }
    }
#if RT1_DW_TIMING & 32
    const uint32_t fbytes = 0u;   // timing-only build: every staging load is out of range (no HBM traffic)
#else
    const uint32_t fbytes = (uint32_t)g.H * g.W * g.C * 2u;
#endif
    const __amdgpu_buffer_rsrc_t rg = wave_rsrc(d.dA + (int64_t)n * g.H * g.W * g.C, fbytes);
    const __amdgpu_buffer_rsrc_t ry = wave_rsrc(d.y + (int64_t)n * g.H * g.W * g.C, fbytes);
    const uint32_t cb = (uint32_t)c0 * 2u;
    const WinRect q = RING ? WinRect(ih0, iw0, IH, IW, g.H, g.W) : WinRect(IH, IW);
    if constexpr (RING) zero_ring(tile, q, IH, IW, cv, vv, pb, PLs, make_uint4(0, 0, 0, 0));
    const int npix = q.npix(), qw = q.w();
    if (npix == 0) return;
    int row = pb / qw, col = pb - row * qw;
    const int dr = PLs / qw, dc = PLs - dr * qw;
    for (; pb < npix; pb += PLs * SU) {
        uint4 ug[SU], uy[SU];
        bool ok[SU];
        int px[SU];
#pragma unroll
        for (int k = 0; k < SU; ++k) {
            const int ih = ih0 + q.r0 + row, iw = iw0 + q.c0 + col;
            if constexpr (RING) px[k] = (q.r0 + row) * IW + q.c0 + col;
            ok[k] = cvalid && pb + k * PLs < npix &&
                    (RING || ((unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W));
            const uint32_t off = ok[k] ? (uint32_t)(ih * g.W + iw) * (uint32_t)g.C * 2u + cb : OOB;
            ug[k] = buf_load16(rg, off);
            uy[k] = buf_load16(ry, off);
            row += dr;
            col += dc;
            if (col >= qw) { col -= qw; ++row; }
        }
#pragma unroll
        for (int k = 0; k < SU; ++k) {
            const int p = RING ? px[k] : pb + k * PLs;
            if (pb + k * PLs >= npix) break;
            f2 gv[4], yv[4];
            unpack4x2(ug[k], gv);
            unpack4x2(uy[k], yv);
            f2 o[4];
            // the four channel pairs' dependency chains advanced step by step, so every packed op has three
            // independent ones between it and its producer (one at a time, dependent packed-fp32 ops back to back
            // cost an s_nop each: 67 per 4-pixel staging round in the k3 unified backward)
            const f2 one = f2{1.f, 1.f};
            f2 z[4], t[4], lin[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = yv[j] * SC[j] + SH[j];
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = z[j] * f2{-1.4426950408889634f, -1.4426950408889634f};   // -z log2 e
#pragma unroll
            for (int j = 0; j < 4; ++j) lin[j] = K2[j] * yv[j] + K0[j];
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = f2{__builtin_amdgcn_exp2f(t[j].x), __builtin_amdgcn_exp2f(t[j].y)};
#pragma unroll
            for (int j = 0; j < 4; ++j) gv[j] = A[j] * gv[j] + B[j];
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = t[j] + one;
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = f2{__builtin_amdgcn_rcpf(t[j].x), __builtin_amdgcn_rcpf(t[j].y)};   // s
#pragma unroll
            for (int j = 0; j < 4; ++j) yv[j] = one - t[j];
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = z[j] * yv[j] + one;
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = t[j] * z[j];                                                   // silu'(z)
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = z[j] * gv[j] + lin[j];
            uint4 v = make_uint4(pack2(o[0].x, o[0].y), pack2(o[1].x, o[1].y), pack2(o[2].x, o[2].y),
                                 pack2(o[3].x, o[3].y));
            if (!ok[k]) v = make_uint4(0, 0, 0, 0);
            tile[p * cv + vv] = v;
        }
    }
}

}  // namespace dw
}  // namespace rt1
