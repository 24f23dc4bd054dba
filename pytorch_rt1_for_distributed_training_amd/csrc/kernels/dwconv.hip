// Depthwise k x k convolution (k in {3,5}, stride in {1,2}, pad (k-1)/2) on
// channels-last bf16 activations, with the surrounding BatchNorm work fused
// (26 depthwise convs of the FiLM-EfficientNet-B3; memory-bound,
// vector ALU, not MFMA work).
//
// forward    out = dwconv(act(x*scale + shift))    (BN+SiLU prologue optional)
//            epilogue EPI_STATS: per-workgroup partial (sum, sumsq) of out for the next BN
// bwd data   s=1: the SAME kernel with the kernel flipped (a stride-1 transposed
//            depthwise conv is a correlation with the flipped taps, same padding);
//            s=2: parity-strip kernel (each output strip has one stride-2 phase);
//            epilogue EPI_BNBWD: dz = dx * silu'(y_in*scale+shift), partials of
//            sum dz and sum dz*xhat for the producing BatchNorm's backward
// bwd weight dw[c, tap] = sum dy * act(x*scale+shift), strips of R outputs per thread
//
// Tiling (CDNA4): a 256-thread workgroup owns CV<=8 channel vectors (8 bf16 =
// 16 B, so one pixel's chunk is a 128-B line) x a spatial tile.  The input tile
// + halo is staged ONCE into LDS with the prologue already applied (one exp per
// input element, not k*k), then each thread produces R outputs along W for 8
// channels, streaming the LDS row once per kernel row (weights of that row in
// registers).  Workgroups loop over tiles (grid <= ~8/CU) so the partial rows
// stay few and are reduced by bn_finalize.
#include <algorithm>
#include <array>
#include <cstdlib>
#include <unordered_map>

#include "common.h"
#include "dw/dw_plan.h"

using namespace rt1;
using namespace rt1::dw;

namespace {

constexpr int BLOCK = 256;
constexpr int EPI_NONE = 0, EPI_STATS = 1, EPI_BNBWD = 2;

struct DwGeo {
    int N, H, W, C, Ho, Wo, k, s, pad;
    int nv;      // C / 8
    int cv;      // channel vectors per workgroup chunk
    int chunks;  // ceil(nv / cv)
};

struct BnBwdEpi {   // producer-BN constants for EPI_BNBWD
    const bf16_t* y;
    const float *scale, *shift, *mean, *rstd;
    int zout;        // unified backward kernels: store dz = dx * silu'(z) instead of dx (pwbwd.hip pw_bwd_z input)
    // unified stride-1 backward without the BN1 epilogue (non-expand residual blocks): dx += res * rmul[n, c], the
    // residual path's gradient (dout * FiLM multiplier) added before the store instead of an add_scaled_ pass
    const bf16_t* res = nullptr;
    const float* rmul = nullptr;
};

typedef float f2 __attribute__((ext_vector_type(2)));

// Timing-only builds (tools/bench_dw_phases.py, values wrong): a bit mask of phases removed -- 1 bf16 unpack,
// 2 LDS staging, 4 tap loop, 8 epilogue, 16 backward strip centre, 32 staging loads
#ifndef RT1_DW_TIMING
#define RT1_DW_TIMING 0
#endif

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
constexpr int DW_RING_PIX = 2000;
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

// Stage an [IH x IW] pixel window (origin ih0, iw0; zero outside [0,Hs) x [0,Ws)) of cv channel vectors
// into LDS, with the BN+activation prologue applied when scale != nullptr.  Each thread owns ONE channel
// vector (per-channel constants in registers) and keeps SU 16-byte loads in flight before it writes
// any of them: the window is ~10 loads per thread, and issuing them one at a time exposed the full
// HBM latency per load.
constexpr int DW_FULLROW_MAX = 18;   // channel vectors up to which a workgroup owns the whole pixel row (make_geo)
constexpr int DW_SU = 4;      // 16-byte loads in flight per thread while staging a tile
// PRO: 0 = copy, 1 = x*scale+shift, 2 = silu(x*scale+shift) -- a compile-time prologue: the run-time `act`
// select cost a v_cndmask plus the dead SiLU's moves per element in the hottest loop of every dw kernel
enum StagePro : int { PRO_COPY = 0, PRO_AFFINE = 1, PRO_SILU = 2 };
template <int SU, int PRO, bool RING>
__device__ __forceinline__ void stage_tile_t(uint4* tile, const bf16_t* __restrict__ x, const DwGeo& g, int n, int ih0,
                                             int iw0, int IH, int IW, int Hs, int Ws, int v0, int ncv,
                                             const float* __restrict__ scale, const float* __restrict__ shift) {
    const int cv = g.cv;
    const int t = threadIdx.x;
    const int vv = t % cv, PLs = BLOCK / cv;
    int pb = t / cv;
    if (pb >= PLs) return;
    const bool cvalid = vv < ncv;
    const int c0 = (v0 + (cvalid ? vv : 0)) * 8;
    f2 SC[4], SH[4];
    if constexpr (PRO != PRO_COPY) {
        load4x2(scale + c0, SC);
        load4x2(shift + c0, SH);
    }
    const bf16_t* xb = x + (int64_t)n * Hs * Ws * g.C + c0;
    const WinRect q = RING ? WinRect(ih0, iw0, IH, IW, Hs, Ws) : WinRect(IH, IW);
    if constexpr (RING) zero_ring(tile, q, IH, IW, cv, vv, pb, PLs, make_uint4(0, 0, 0, 0));
    const int npix = q.npix(), qw = q.w();
    if (npix == 0) return;
    // in-rectangle pixel i = pb + k*PLs walked as (row, col) with a division-free step of (dr, dc)
    int row = pb / qw, col = pb - row * qw;
    const int dr = PLs / qw, dc = PLs - dr * qw;
    for (; pb < npix; pb += PLs * SU) {
        uint4 u[SU];
        int px[SU];
        unsigned valid = 0;
#pragma unroll
        for (int k = 0; k < SU; ++k) {
            const int ih = ih0 + q.r0 + row, iw = iw0 + q.c0 + col;
            if constexpr (RING) px[k] = (q.r0 + row) * IW + q.c0 + col;
            u[k] = make_uint4(0, 0, 0, 0);
            if (cvalid && pb + k * PLs < npix && (RING || ((unsigned)ih < (unsigned)Hs && (unsigned)iw < (unsigned)Ws))) {
                u[k] = *reinterpret_cast<const uint4*>(xb + (uint32_t)(ih * Ws + iw) * (uint32_t)g.C);
                valid |= 1u << k;
            }
            row += dr;
            col += dc;
            if (col >= qw) { col -= qw; ++row; }
        }
#pragma unroll
        for (int k = 0; k < SU; ++k) {
            const int p = RING ? px[k] : pb + k * PLs;
            if (pb + k * PLs >= npix) break;
            uint4 v = u[k];
            if (PRO != PRO_COPY && (valid >> k & 1u)) {
                // packed pairs, phase by phase over the 4 pairs: the affine, -z log2 e, +1 and z * s as v_pk_* ops
                // (they were scalar f32 ops around the transcendentals), each with independent ops between it and
                // its producer
                f2 z[4];
                unpack4x2(v, z);
#pragma unroll
                for (int j = 0; j < 4; ++j) z[j] = z[j] * SC[j] + SH[j];
                if constexpr (PRO == PRO_SILU) {
                    f2 t[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) t[j] = z[j] * f2{-1.4426950408889634f, -1.4426950408889634f};
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        t[j] = f2{__builtin_amdgcn_exp2f(t[j].x), __builtin_amdgcn_exp2f(t[j].y)} + f2{1.f, 1.f};
#pragma unroll
                    for (int j = 0; j < 4; ++j) t[j] = f2{__builtin_amdgcn_rcpf(t[j].x), __builtin_amdgcn_rcpf(t[j].y)};
#pragma unroll
                    for (int j = 0; j < 4; ++j) z[j] = z[j] * t[j];
                }
                v.x = pack2(z[0].x, z[0].y); v.y = pack2(z[1].x, z[1].y); v.z = pack2(z[2].x, z[2].y);
                v.w = pack2(z[3].x, z[3].y);
            }
            tile[p * cv + vv] = v;
        }
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

struct XExp {
    const bf16_t* x;     // [N, H, W, Cin] block input (the depthwise input map's resolution)
    const bf16_t* we;    // [Ce, Cin] bf16 expand weight
    int cin;
};

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

// run-time dispatch on the (workgroup-uniform) prologue; RING: walk only the in-image rectangle (WinRect)
template <int SU = DW_SU, bool RING = false>
__device__ __forceinline__ void stage_tile(uint4* tile, const bf16_t* __restrict__ x, const DwGeo& g, int n, int ih0,
                                           int iw0, int IH, int IW, int Hs, int Ws, int v0, int ncv,
                                           const float* __restrict__ scale, const float* __restrict__ shift, int act) {
    if (!scale)
        stage_tile_t<SU, PRO_COPY, RING>(tile, x, g, n, ih0, iw0, IH, IW, Hs, Ws, v0, ncv, scale, shift);
    else if (act == ACT_SILU)
        stage_tile_t<SU, PRO_SILU, RING>(tile, x, g, n, ih0, iw0, IH, IW, Hs, Ws, v0, ncv, scale, shift);
    else
        stage_tile_t<SU, PRO_AFFINE, RING>(tile, x, g, n, ih0, iw0, IH, IW, Hs, Ws, v0, ncv, scale, shift);
}

// reduce (s, q)[8] over the pixel lanes and write this workgroup's partial row
__device__ __forceinline__ void write_partials(float* red, const float (&s)[8], const float (&q)[8], int PL, int pl,
                                               int cv, int lane_cv, int ncv, int v0, int C, float* __restrict__ ps,
                                               float* __restrict__ pq) {
    __syncthreads();
    const int C8 = cv * 8;
    for (int i = threadIdx.x; i < PL * C8 * 2; i += BLOCK) red[i] = 0.f;
    __syncthreads();
    if (pl < PL) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            red[pl * C8 + lane_cv * 8 + j] = s[j];
            red[PL * C8 + pl * C8 + lane_cv * 8 + j] = q[j];
        }
    }
    __syncthreads();
    for (int cc = threadIdx.x; cc < ncv * 8; cc += BLOCK) {
        float a = 0.f, b = 0.f;
        for (int p = 0; p < PL; ++p) {
            a += red[p * C8 + cc];
            b += red[PL * C8 + p * C8 + cc];
        }
        ps[(int64_t)blockIdx.x * C + v0 * 8 + cc] = a;
        pq[(int64_t)blockIdx.x * C + v0 * 8 + cc] = b;
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

// epilogue for one output vector o[8] at element offset `off`; ecl = this lane's constants, C8 = row stride
template <int EPI>
__device__ __forceinline__ void epilogue(float (&o)[8], bf16_t* __restrict__ out, int64_t off, const uint4 ypre,
                                         const float* ecl, int C8, float (&s)[8], float (&q)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = bf2f(f2bf(o[j]));   // statistics describe the stored bf16 tensor
    store8(out + off, o);
    if constexpr (EPI == EPI_STATS) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            s[j] += o[j];
            q[j] = fmaf(o[j], o[j], q[j]);
        }
    } else if constexpr (EPI == EPI_BNBWD) {
        float yv[8], sc[8], sh[8], rr[8], mr[8];
        unpack8(ypre, yv);
        load8f(ecl, sc);
        load8f(ecl + C8, sh);
        load8f(ecl + 2 * C8, rr);
        load8f(ecl + 3 * C8, mr);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float dz = o[j] * silu_grad(fmaf(yv[j], sc[j], sh[j]));
            s[j] += dz;
            q[j] = fmaf(dz, fmaf(yv[j], rr[j], mr[j]), q[j]);
        }
    }
}

// ------------------------------------------------------------------ forward (and s=1 backward data)
// XK != 0 (x-mode): the staged tile is silu(bn1(x @ We^T)) recomputed on MFMA from xe (`x` is unused, scale /
// shift are BN1's constants, staged once into LDS)
template <int K, int S, int R, int EPI, int XK = 0, bool RG = false>
__global__ __launch_bounds__(BLOCK, 3) void dw_fwd_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ scale,
                                                       const float* __restrict__ shift, int act, DwGeo g, int TH,
                                                       int TW, bf16_t* __restrict__ out, float* __restrict__ psum,
                                                       float* __restrict__ psq, BnBwdEpi e, XExp xe) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int IH = (TH - 1) * S + K, IW = (TW - 1) * S + K;
    const int cv = g.cv;
    uint4* tile = reinterpret_cast<uint4*>(smem);
    float* wl = reinterpret_cast<float*>(smem + (size_t)IH * IW * cv * 16);
    float* ecl = wl + K * K * cv * 8;
    float* red = reinterpret_cast<float*>(smem);  // aliases the tile once the last tile is consumed

    const int v0 = blockIdx.y * cv;
    const int ncv = min(cv, g.nv - v0);
    const int t = threadIdx.x;
    const int lane_cv = t % cv, pl = t / cv, PL = BLOCK / cv;
    const int groups_w = TW / R;
    const StripWalk walk0(pl, PL, groups_w, S * IW * cv, R * S * cv, g.Wo * g.C, R * g.C);

    for (int i = t; i < K * K * cv * 8; i += BLOCK) {
        const int tap = i / (cv * 8), cc = i % (cv * 8);
        wl[i] = (cc < ncv * 8) ? w[(int64_t)(v0 * 8 + cc) * K * K + tap] : 0.f;
    }
    const int tiles_h = (g.Ho + TH - 1) / TH, tiles_w = (g.Wo + TW - 1) / TW;
    const int64_t ntiles = (int64_t)g.N * tiles_h * tiles_w;
    float s_acc[8], q_acc[8];
    f2 s2[4], q2[4];                                   // EPI_STATS: the forward's per-channel-pair sums
#pragma unroll
    for (int j = 0; j < 4; ++j) s2[j] = q2[j] = f2{0.f, 0.f};
    stage_epi_consts<EPI>(ecl, e, v0, ncv, cv);
    if constexpr (XK != 0) {
        for (int i = t; i < cv * 8; i += BLOCK) {
            const bool ok = i < ncv * 8;
            ecl[i] = ok ? scale[v0 * 8 + i] : 0.f;
            ecl[cv * 8 + i] = ok ? shift[v0 * 8 + i] : 0.f;
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) s_acc[j] = q_acc[j] = 0.f;

    for (int64_t tile_id = blockIdx.x; tile_id < ntiles; tile_id += gridDim.x) {
        const int n = (int)(tile_id / (tiles_h * tiles_w));
        const int rem = (int)(tile_id - (int64_t)n * tiles_h * tiles_w);
        const int oh0 = (rem / tiles_w) * TH, ow0 = (rem % tiles_w) * TW;
        __syncthreads();
        if constexpr (XK != 0)
            stage_xmfma<xk_kc(XK), xk_ng(XK), true>(reinterpret_cast<bf16_t*>(tile), cv * 8, xe, g.H, g.W, n,
                                                    oh0 * S - g.pad, ow0 * S - g.pad, IH, IW, v0 * 8, ncv * 8, ecl);
        else
#if !(RT1_DW_TIMING & 2)
            stage_tile<DW_SU, RG>(tile, x, g, n, oh0 * S - g.pad, ow0 * S - g.pad, IH, IW, g.H, g.W, v0, ncv, scale,
                                      shift, act);
#else
            ;
#endif
        __syncthreads();
        if (lane_cv >= ncv || pl >= PL) continue;
        const int c0 = (v0 + lane_cv) * 8;
        const int64_t tbase = (((int64_t)n * g.Ho + oh0) * g.Wo + ow0) * g.C + c0;
        for (StripWalk it = walk0; it.ty < TH; it.next()) {
            const int tx = it.gx * R;
            if (oh0 + it.ty >= g.Ho) break;                 // rows only grow along the walk
            const int64_t obase = tbase + it.o2;
            // EPI_BNBWD reads the producer's pre-BN tensor at every output: issue those loads now so their
            // latency hides behind the taps instead of stalling the epilogue
            // (not for k5 s1: its 4x5 accumulator/weight rows leave no registers for the early loads)
            constexpr bool PREF = EPI == EPI_BNBWD && !(K == 5 && S == 1);
            uint4 ypre[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                ypre[r] = make_uint4(0, 0, 0, 0);
                if (PREF && ow0 + tx + r < g.Wo)
                    ypre[r] = *reinterpret_cast<const uint4*>(e.y + obase + (int64_t)r * g.C);
            }
            // channel pairs as float2: the packed-f32 FMA (v_pk_fma_f32) takes its operands straight from the
            // unpacked register pairs, with no SLP re-packing moves
            f2 acc2[R][4];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc2[r][j] = f2{0.f, 0.f};
            const uint4* trow = tile + it.o1 + lane_cv;
            const float* wrow_p = wl + lane_cv * 8;
#if RT1_DW_TIMING & 4
#pragma unroll 1
            for (int kh = 0; kh < 0; ++kh, trow += IW * cv, wrow_p += K * cv * 8) {
#else
#pragma unroll 1
            for (int kh = 0; kh < K; ++kh, trow += IW * cv, wrow_p += K * cv * 8) {
#endif
                f2 wrow[K][4];
#pragma unroll
                for (int kw = 0; kw < K; ++kw) load4x2(wrow_p + kw * cv * 8, wrow[kw]);
                constexpr int NIN = (R - 1) * S + K;
#pragma unroll
                for (int qq = 0; qq < NIN; ++qq) {
                    f2 in[4];
                    unpack4x2(trow[qq * cv], in);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int kw = qq - r * S;
                        if (kw >= 0 && kw < K) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) acc2[r][j] = in[j] * wrow[kw][j] + acc2[r][j];
                        }
                    }
                }
            }
            float acc[R][8];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) { acc[r][2 * j] = acc2[r][j].x; acc[r][2 * j + 1] = acc2[r][j].y; }
            if constexpr (EPI == EPI_BNBWD && !PREF) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (ow0 + tx + r < g.Wo) ypre[r] = *reinterpret_cast<const uint4*>(e.y + obase + (int64_t)r * g.C);
            }
#if RT1_DW_TIMING & 8
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (acc[r][0] == 1234.5f) out[obase + (int64_t)r * g.C] = (bf16_t)1;
            if constexpr (false)
#endif
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int ow = ow0 + tx + r;
                if (ow >= g.Wo) continue;
                if constexpr (EPI == EPI_BNBWD) {
                    epilogue<EPI>(acc[r], out, obase + (int64_t)r * g.C, ypre[r], ecl + lane_cv * 8, cv * 8, s_acc,
                                  q_acc);
                } else {
                    // forward: ONE pack of the channel pairs for the store; the BN2 statistics of the stored bf16
                    // values come from unpacking that word (2 ops per pair) into packed-fp32 sums.  The float[8]
                    // epilogue rounded every element through a scalar convert + shift and packed again for the
                    // store: ~36 VALU per output vector, now ~20 (the same sums, bit for bit)
                    const uint4 u = make_uint4(pack2(acc2[r][0].x, acc2[r][0].y), pack2(acc2[r][1].x, acc2[r][1].y),
                                               pack2(acc2[r][2].x, acc2[r][2].y), pack2(acc2[r][3].x, acc2[r][3].y));
                    *reinterpret_cast<uint4*>(out + obase + (int64_t)r * g.C) = u;
                    if constexpr (EPI == EPI_STATS) {
                        f2 v[4];
                        unpack4x2(u, v);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            s2[j] = s2[j] + v[j];
                            q2[j].x = fmaf(v[j].x, v[j].x, q2[j].x);
                            q2[j].y = fmaf(v[j].y, v[j].y, q2[j].y);
                        }
                    }
                }
            }
        }
    }
    if constexpr (EPI == EPI_STATS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s_acc[2 * j] = s2[j].x; s_acc[2 * j + 1] = s2[j].y;
            q_acc[2 * j] = q2[j].x; q_acc[2 * j + 1] = q2[j].y;
        }
    }
    if constexpr (EPI != EPI_NONE) write_partials(red, s_acc, q_acc, PL, pl, cv, lane_cv, ncv, v0, g.C, psum, psq);
}

// ------------------------------------------------------------------ stride-2 backward data
// dx[ih, iw] = sum_{kh,kw: (ih+pad-kh), (iw+pad-kw) even} w[kh,kw] * dy[(ih+pad-kh)/2, (iw+pad-kw)/2]
// A thread strip = 4 outputs of ONE column parity (iw0, iw0+2, iw0+4, iw0+6): all share the valid kw set,
// and their dy columns are consecutive -> a stride-1 correlation over the dy row.
template <int K, int EPI>
__global__ __launch_bounds__(BLOCK, EPI == EPI_NONE ? 4 : 3) void dw_bwd_data_s2_kernel(const bf16_t* __restrict__ dy,
                                                               const float* __restrict__ w, DwGeo g, int TH, int TW,
                                                               bf16_t* __restrict__ dx, float* __restrict__ pdz,
                                                               float* __restrict__ pdzx, BnBwdEpi e) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int R = 4;
    // dy rows/cols touching input rows [ih0, ih0+TH): oh in [floor((ih0+pad-K+1)/2), floor((ih0+TH-1+pad)/2)]
    const int DH = (TH + K) / 2 + 1, DW = (TW + K) / 2 + 1;
    const int cv = g.cv;
    uint4* tile = reinterpret_cast<uint4*>(smem);
    float* wl = reinterpret_cast<float*>(smem + (size_t)DH * DW * cv * 16);
    float* ecl = wl + K * K * cv * 8;
    float* red = reinterpret_cast<float*>(smem);

    const int v0 = blockIdx.y * cv;
    const int ncv = min(cv, g.nv - v0);
    const int t = threadIdx.x;
    const int lane_cv = t % cv, pl = t / cv, PL = BLOCK / cv;
    const int ngroups = TH * (TW / 8) * 2;

    for (int i = t; i < K * K * cv * 8; i += BLOCK) {
        const int tap = i / (cv * 8), cc = i % (cv * 8);
        wl[i] = (cc < ncv * 8) ? w[(int64_t)(v0 * 8 + cc) * K * K + tap] : 0.f;
    }
    const int tiles_h = (g.H + TH - 1) / TH, tiles_w = (g.W + TW - 1) / TW;
    const int64_t ntiles = (int64_t)g.N * tiles_h * tiles_w;
    float s_acc[8], q_acc[8];
    stage_epi_consts<EPI>(ecl, e, v0, ncv, cv);
#pragma unroll
    for (int j = 0; j < 8; ++j) s_acc[j] = q_acc[j] = 0.f;

    for (int64_t tile_id = blockIdx.x; tile_id < ntiles; tile_id += gridDim.x) {
        const int n = (int)(tile_id / (tiles_h * tiles_w));
        const int rem = (int)(tile_id - (int64_t)n * tiles_h * tiles_w);
        const int ih0 = (rem / tiles_w) * TH, iw0 = (rem % tiles_w) * TW;   // TH, TW even
        const int oh_lo = (ih0 + g.pad - (K - 1)) >> 1;                     // floor (arith shift)
        const int ow_lo = (iw0 + g.pad - (K - 1)) >> 1;
        __syncthreads();
        stage_tile(tile, dy, g, n, oh_lo, ow_lo, DH, DW, g.Ho, g.Wo, v0, ncv, nullptr, nullptr, 0);
        __syncthreads();
        if (lane_cv >= ncv || pl >= PL) continue;
        for (int grp = pl; grp < ngroups; grp += PL) {
            const int ty = grp / ((TW / 8) * 2);
            const int rem2 = grp % ((TW / 8) * 2);
            const int par = rem2 & 1, xb = (rem2 >> 1) * 8;
            const int ih = ih0 + ty;
            if (ih >= g.H) continue;
            const int iwb = iw0 + xb + par;                                  // first column of the strip
            const int c0 = (v0 + lane_cv) * 8;
            const int64_t obase = (((int64_t)n * g.H + ih) * g.W + iwb) * g.C + c0;
            uint4 ypre[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                ypre[r] = make_uint4(0, 0, 0, 0);
                if (EPI == EPI_BNBWD && iwb + 2 * r < g.W)
                    ypre[r] = *reinterpret_cast<const uint4*>(e.y + obase + (int64_t)2 * r * g.C);
            }
            f2 acc2[R][4];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc2[r][j] = f2{0.f, 0.f};
#pragma unroll
            for (int kh = 0; kh < K; ++kh) {
                const int nh = ih + g.pad - kh;
                if (nh & 1) continue;
                const int oh = nh >> 1;                                      // may be <0 or >=Ho: tile holds zeros
                const uint4* trow = tile + (oh - oh_lo) * DW * cv + lane_cv;
#pragma unroll
                for (int kw = 0; kw < K; ++kw) {
                    const int nw = iwb + g.pad - kw;
                    if (nw & 1) continue;                                    // same for the whole strip
                    const int oc = (nw >> 1) - ow_lo;                        // dy column of strip element 0
                    f2 wv[4];
                    load4x2(wl + (kh * K + kw) * cv * 8 + lane_cv * 8, wv);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        f2 in[4];
                        unpack4x2(trow[(oc + r) * cv], in);
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc2[r][j] = in[j] * wv[j] + acc2[r][j];
                    }
                }
            }
            float acc[R][8];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) { acc[r][2 * j] = acc2[r][j].x; acc[r][2 * j + 1] = acc2[r][j].y; }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int iw = iwb + 2 * r;
                if (iw < g.W)
                    epilogue<EPI>(acc[r], dx, obase + (int64_t)2 * r * g.C, ypre[r], ecl + lane_cv * 8, cv * 8, s_acc,
                                  q_acc);
            }
        }
    }
    if constexpr (EPI != EPI_NONE) write_partials(red, s_acc, q_acc, PL, pl, cv, lane_cv, ncv, v0, g.C, pdz, pdzx);
}

// ------------------------------------------------------------------ backward weight
// Thread role = (channel vector, kernel row kh, strip lane).  A strip = R consecutive output pixels of
// one row: its R dy vectors and the (R-1)*S+K input vectors of the kernel row are each read once
// from LDS, and feed K x 8 accumulators.  Partials: dwp[blockIdx.x][c][tap].
template <int K, int S, int R>
__global__ __launch_bounds__(BLOCK, 3) void dw_bwd_weight_kernel(const bf16_t* __restrict__ dy,
                                                              const bf16_t* __restrict__ x,
                                                              const float* __restrict__ scale,
                                                              const float* __restrict__ shift, int act, DwGeo g,
                                                              int TH, int TW, float* __restrict__ dwp) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int IH = (TH - 1) * S + K, IW = (TW - 1) * S + K;
    const int cv = g.cv;
    uint4* xt = reinterpret_cast<uint4*>(smem);
    uint4* dt = xt + IH * IW * cv;
    float* red = reinterpret_cast<float*>(smem);

    const int v0 = blockIdx.y * cv;
    const int ncv = min(cv, g.nv - v0);
    const int t = threadIdx.x;
    const int per = cv * K;
    const int lane_cv = t % cv, kh = (t / cv) % K, pl = t / per, PL = BLOCK / per;
    const int groups_w = TW / R;
    // o1: input-row origin of the strip in xt (this thread's kernel row kh folded in), o2: its dy in dt
    const StripWalk walk0(pl, PL, groups_w, S * IW * cv, R * S * cv, TW * cv, R * cv);
    const int xoff = kh * IW * cv + lane_cv;

    const int tiles_h = (g.Ho + TH - 1) / TH, tiles_w = (g.Wo + TW - 1) / TW;
    const int64_t ntiles = (int64_t)g.N * tiles_h * tiles_w;
    f2 acc2[K][4];
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc2[a][j] = f2{0.f, 0.f};

    for (int64_t tile_id = blockIdx.x; tile_id < ntiles; tile_id += gridDim.x) {
        const int n = (int)(tile_id / (tiles_h * tiles_w));
        const int rem = (int)(tile_id - (int64_t)n * tiles_h * tiles_w);
        const int oh0 = (rem / tiles_w) * TH, ow0 = (rem % tiles_w) * TW;
        __syncthreads();
        stage_tile(xt, x, g, n, oh0 * S - g.pad, ow0 * S - g.pad, IH, IW, g.H, g.W, v0, ncv, scale, shift, act);
        stage_tile<2>(dt, dy, g, n, oh0, ow0, TH, TW, g.Ho, g.Wo, v0, ncv, nullptr, nullptr, 0);
        __syncthreads();
        if (pl >= PL || lane_cv >= ncv) continue;
        for (StripWalk it = walk0; it.ty < TH; it.next()) {
            f2 d[R][4];
            const uint4* drow = dt + it.o2 + lane_cv;
#pragma unroll
            for (int r = 0; r < R; ++r) unpack4x2(drow[r * cv], d[r]);
            const uint4* xrow = xt + it.o1 + xoff;
            constexpr int NIN = (R - 1) * S + K;
#pragma unroll
            for (int qq = 0; qq < NIN; ++qq) {
                f2 in[4];
                unpack4x2(xrow[qq * cv], in);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int kw = qq - r * S;
                    if (kw >= 0 && kw < K) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc2[kw][j] = d[r][j] * in[j] + acc2[kw][j];
                    }
                }
            }
        }
    }
    __syncthreads();
    const int C8 = cv * 8, KK = K * K;
    for (int i = t; i < PL * C8 * KK; i += BLOCK) red[i] = 0.f;
    __syncthreads();
    if (pl < PL && lane_cv < ncv) {
#pragma unroll
        for (int kw = 0; kw < K; ++kw)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                red[(pl * C8 + lane_cv * 8 + j) * KK + kh * K + kw] = (j & 1) ? acc2[kw][j >> 1].y : acc2[kw][j >> 1].x;
    }
    __syncthreads();
    for (int i = t; i < ncv * 8 * KK; i += BLOCK) {
        float a = 0.f;
        for (int p = 0; p < PL; ++p) a += red[p * C8 * KK + i];
        dwp[(int64_t)blockIdx.x * g.C * KK + (int64_t)v0 * 8 * KK + i] = a;
    }
}

// ------------------------------------------------------------------ fused stride-1 backward
// One pass for the whole depthwise backward of a stride-1 MBConv block:
//   dy  = BN2-backward-apply(dA, y2)       rebuilt while staging (dy is never written to HBM)
//   dx  = correlation(dy, flipped taps)    + EPI_BNBWD epilogue (BN1 partials) as the stride-1 data kernel
//   dW += dy (x) act(x1*scale1 + shift1)   as the weight kernel, from the same staged tiles
// Unfused this is bn_bwd_apply (read dA, y2; write dy) + data (read dy, y1; write dx) + weight (read dy, y1):
// 8 activation passes.  Fused: dA, y2, x1 read once, dx written once (4), and dy costs no HBM traffic at all.
struct DyBnBwd {   // dy = k1 * (dA * gate + rb) * silu'(y*scale + shift) + k2 * y + k0   (bn_bwd_apply_flat_kernel)
    const bf16_t *dA, *y;
    const float *gate, *rb;                       // [N, C] per-frame
    const float *scale, *shift, *mean, *rstd, *gamma, *mdz, *mdzx;   // [C]
};

constexpr int DWF_SU = 4;     // pixels (2 x 16-B loads each) in flight per thread while staging dy
constexpr int DWF_OCC = 2;    // workgroups / CU the fused kernel's register budget targets
#ifndef DW_CENTRE_PREFETCH
#define DW_CENTRE_PREFETCH 1
#endif
// Unified stride-1 backward, y1 in HBM: the tile's strip centres x1 [TH x TW][C8] are copied into LDS by LDS-DMA
// (global_load_lds, no VGPRs, all in flight during the dy staging) instead of global loads at every strip's start that
// each wait a full HBM round trip.  The centre tile's LDS shrinks the dy tile (more halo), so it pays only where the
// tile covers the whole 10 x 10 map anyway: the 2-channel 5-output k5 form, -9 % on blocks 19-23; on the 19 x 19 .. 150 x
// 150 maps the smaller tiles cost 7-27 % (profiles/r6_dw_centre_stage_ab.log).
#ifndef DW_CENTRE_STAGE
#define DW_CENTRE_STAGE 1
#endif
typedef __attribute__((address_space(3))) void dw_lds_void;
constexpr bool centre_stage_on(int cpt, int r) { return DW_CENTRE_STAGE && cpt == 2 && r == 5; }

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

// stage_dy over HALF vectors (4 channels, 8-byte loads / stores): the per-channel constants of 4 channels (24
// VGPRs instead of 48) and 8-byte loads in flight -- the staging of the 2-channel k5 unified backward, whose K x K
// weight-gradient accumulators stay live across it (the 8-channel staging pushed it past 168 VGPRs, 3 workgroups/CU)
template <int SU, bool RING>
__device__ __forceinline__ void stage_dy_half(uint4* tile, const DyBnBwd& d, const DwGeo& g, int n, int ih0, int iw0,
                                              int IH, int IW, int v0, int ncv) {
    const int cv = g.cv, ch = 2 * cv;
    const int t = threadIdx.x;
    const int hv = t % ch, PLs = BLOCK / ch;
    int pb = t / ch;
    if (pb >= PLs) return;
    const bool cvalid = (hv >> 1) < ncv;
    const int c0 = v0 * 8 + (cvalid ? hv : 0) * 4;
    f2 A[2], B[2], K2[2], K0[2], SC[2], SH[2];
    {
        float gm[4], rr[4], mu[4], mz[4], mx[4], a[4], b[4], sc[4], sh[4];
        auto ld4 = [](const float* p, float (&o)[4]) {
            const float4 v = *reinterpret_cast<const float4*>(p);
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        };
        ld4(d.gamma + c0, gm); ld4(d.rstd + c0, rr); ld4(d.mean + c0, mu);
        ld4(d.mdz + c0, mz); ld4(d.mdzx + c0, mx);
        ld4(d.gate + (int64_t)n * g.C + c0, a); ld4(d.rb + (int64_t)n * g.C + c0, b);
        ld4(d.scale + c0, sc); ld4(d.shift + c0, sh);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
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
    const uint32_t fbytes = (uint32_t)g.H * g.W * g.C * 2u;
    const __amdgpu_buffer_rsrc_t rg = wave_rsrc(d.dA + (int64_t)n * g.H * g.W * g.C, fbytes);
    const __amdgpu_buffer_rsrc_t ry = wave_rsrc(d.y + (int64_t)n * g.H * g.W * g.C, fbytes);
    const uint32_t cb = (uint32_t)c0 * 2u;
    uint2* tl = reinterpret_cast<uint2*>(tile);
    const WinRect q = RING ? WinRect(ih0, iw0, IH, IW, g.H, g.W) : WinRect(IH, IW);
    if constexpr (RING) zero_ring(tl, q, IH, IW, ch, hv, pb, PLs, make_uint2(0, 0));
    const int npix = q.npix(), qw = q.w();
    if (npix == 0) return;
    int row = pb / qw, col = pb - row * qw;
    const int dr = PLs / qw, dc = PLs - dr * qw;
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    for (; pb < npix; pb += PLs * SU) {
        u32x2 ug[SU], uy[SU];
        bool ok[SU];
        int px[SU];
#pragma unroll
        for (int k = 0; k < SU; ++k) {
            const int ih = ih0 + q.r0 + row, iw = iw0 + q.c0 + col;
            if constexpr (RING) px[k] = (q.r0 + row) * IW + q.c0 + col;
            ok[k] = cvalid && pb + k * PLs < npix &&
                    (RING || ((unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W));
            const uint32_t off = ok[k] ? (uint32_t)(ih * g.W + iw) * (uint32_t)g.C * 2u + cb : OOB;
            ug[k] = __builtin_amdgcn_raw_buffer_load_b64(rg, (int)off, 0, 0);
            uy[k] = __builtin_amdgcn_raw_buffer_load_b64(ry, (int)off, 0, 0);
            row += dr;
            col += dc;
            if (col >= qw) { col -= qw; ++row; }
        }
        // the SU pixels' two channel pairs advanced phase by phase (8 independent packed chains; pair by pair the
        // dependent packed ops each cost an s_nop)
        f2 o[SU][2];
        {
            const f2 one = f2{1.f, 1.f};
            f2 gv[SU][2], yv[SU][2], z[SU][2], t[SU][2];
#pragma unroll
            for (int k = 0; k < SU; ++k) {
                gv[k][0] = f2{__uint_as_float(ug[k].x << 16), __uint_as_float(ug[k].x & 0xffff0000u)};
                gv[k][1] = f2{__uint_as_float(ug[k].y << 16), __uint_as_float(ug[k].y & 0xffff0000u)};
                yv[k][0] = f2{__uint_as_float(uy[k].x << 16), __uint_as_float(uy[k].x & 0xffff0000u)};
                yv[k][1] = f2{__uint_as_float(uy[k].y << 16), __uint_as_float(uy[k].y & 0xffff0000u)};
            }
#pragma unroll
            for (int k = 0; k < SU; ++k)
#pragma unroll
                for (int j = 0; j < 2; ++j) z[k][j] = yv[k][j] * SC[j] + SH[j];
#pragma unroll
            for (int k = 0; k < SU; ++k)
#pragma unroll
                for (int j = 0; j < 2; ++j) t[k][j] = z[k][j] * f2{-1.4426950408889634f, -1.4426950408889634f};
#pragma unroll
            for (int k = 0; k < SU; ++k)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    t[k][j] = f2{__builtin_amdgcn_exp2f(t[k][j].x), __builtin_amdgcn_exp2f(t[k][j].y)};
                    o[k][j] = K2[j] * yv[k][j] + K0[j];
                }
#pragma unroll
            for (int k = 0; k < SU; ++k)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    t[k][j] = t[k][j] + one;
                    gv[k][j] = A[j] * gv[k][j] + B[j];
                }
#pragma unroll
            for (int k = 0; k < SU; ++k)
#pragma unroll
                for (int j = 0; j < 2; ++j) t[k][j] = f2{__builtin_amdgcn_rcpf(t[k][j].x), __builtin_amdgcn_rcpf(t[k][j].y)};
#pragma unroll
            for (int k = 0; k < SU; ++k)
#pragma unroll
                for (int j = 0; j < 2; ++j) yv[k][j] = one - t[k][j];
#pragma unroll
            for (int k = 0; k < SU; ++k)
#pragma unroll
                for (int j = 0; j < 2; ++j) z[k][j] = z[k][j] * yv[k][j] + one;
#pragma unroll
            for (int k = 0; k < SU; ++k)
#pragma unroll
                for (int j = 0; j < 2; ++j) z[k][j] = t[k][j] * z[k][j];
#pragma unroll
            for (int k = 0; k < SU; ++k)
#pragma unroll
                for (int j = 0; j < 2; ++j) o[k][j] = z[k][j] * gv[k][j] + o[k][j];
        }
#pragma unroll
        for (int k = 0; k < SU; ++k) {
            const int p = RING ? px[k] : pb + k * PLs;
            if (pb + k * PLs >= npix) break;
            uint2 v = make_uint2(pack2(o[k][0].x, o[k][0].y), pack2(o[k][1].x, o[k][1].y));
            if (!ok[k]) v = make_uint2(0, 0);
            tl[p * ch + hv] = v;
        }
    }
}

template <int K, int R, int EPI>
__global__ __launch_bounds__(BLOCK, DWF_OCC) void dw_bwd_fused_kernel(DyBnBwd d, const bf16_t* __restrict__ x1,
                                                             const float* __restrict__ scale1,
                                                             const float* __restrict__ shift1, int act1,
                                                             const float* __restrict__ wflip, DwGeo g, int TH, int TW,
                                                             bf16_t* __restrict__ dx, float* __restrict__ pdz,
                                                             float* __restrict__ pdzx, BnBwdEpi e,
                                                             float* __restrict__ dwp) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int P = (K - 1) / 2, KK = K * K;
    const int IH = TH + K - 1, IW = TW + K - 1;
    const int cv = g.cv;
    uint4* dt = reinterpret_cast<uint4*>(smem);
    uint4* at = dt + IH * IW * cv;
    float* wl = reinterpret_cast<float*>(at + IH * IW * cv);
    float* ecl = wl + KK * cv * 8;
    float* red = reinterpret_cast<float*>(smem);  // aliases the tiles once the last tile is consumed

    const int v0 = blockIdx.y * cv;
    const int ncv = min(cv, g.nv - v0);
    const int t = threadIdx.x;
    const int lane_cv = t % cv, pl = t / cv, PL = BLOCK / cv;               // data-part role
    const int kh = (t / cv) % K, plw = t / (cv * K), PLW = BLOCK / (cv * K);  // weight-part role
    const int groups_w = TW / R;
    const StripWalk dwalk0(pl, PL, groups_w, IW * cv, R * cv, g.W * g.C, R * g.C);
    // weight part: o1 = a1 row origin of the strip, o2 = its dy (tile centre, P rows / columns in)
    const StripWalk wwalk0(plw, PLW, groups_w, IW * cv, R * cv, IW * cv, R * cv);
    const int aoff = kh * IW * cv + lane_cv, doff = (P * IW + P) * cv + lane_cv;

    for (int i = t; i < KK * cv * 8; i += BLOCK) {
        const int tap = i / (cv * 8), cc = i % (cv * 8);
        wl[i] = (cc < ncv * 8) ? wflip[(int64_t)(v0 * 8 + cc) * KK + tap] : 0.f;
    }
    const int tiles_h = (g.H + TH - 1) / TH, tiles_w = (g.W + TW - 1) / TW;
    const int64_t ntiles = (int64_t)g.N * tiles_h * tiles_w;
    float s_acc[8], q_acc[8];
    stage_epi_consts<EPI>(ecl, e, v0, ncv, cv);
#pragma unroll
    for (int j = 0; j < 8; ++j) s_acc[j] = q_acc[j] = 0.f;
    f2 wacc[K][4];
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) wacc[a][j] = f2{0.f, 0.f};

    for (int64_t tile_id = blockIdx.x; tile_id < ntiles; tile_id += gridDim.x) {
        const int n = (int)(tile_id / (tiles_h * tiles_w));
        const int rem = (int)(tile_id - (int64_t)n * tiles_h * tiles_w);
        const int oh0 = (rem / tiles_w) * TH, ow0 = (rem % tiles_w) * TW;
        __syncthreads();
        stage_dy<DWF_SU, false>(dt, d, g, n, oh0 - P, ow0 - P, IH, IW, v0, ncv);
        stage_tile(at, x1, g, n, oh0 - P, ow0 - P, IH, IW, g.H, g.W, v0, ncv, scale1, shift1, act1);
        __syncthreads();
        if (lane_cv >= ncv) continue;
        // ---- data gradient: stride-1 correlation of dy with the flipped taps (dw_fwd_kernel<K, 1, R, EPI>)
        const int64_t tbase = (((int64_t)n * g.H + oh0) * g.W + ow0) * g.C + (v0 + lane_cv) * 8;
        for (StripWalk it = dwalk0; it.ty < TH; it.next()) {
            const int tx = it.gx * R;
            if (oh0 + it.ty >= g.H) break;
            const int64_t obase = tbase + it.o2;
            f2 acc2[R][4];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc2[r][j] = f2{0.f, 0.f};
            const uint4* trow = dt + it.o1 + lane_cv;
            const float* wrow_p = wl + lane_cv * 8;
#pragma unroll 1
            for (int kr = 0; kr < K; ++kr, trow += IW * cv, wrow_p += K * cv * 8) {
                f2 wrow[K][4];
#pragma unroll
                for (int kw = 0; kw < K; ++kw) load4x2(wrow_p + kw * cv * 8, wrow[kw]);
                constexpr int NIN = R - 1 + K;
#pragma unroll
                for (int qq = 0; qq < NIN; ++qq) {
                    f2 in[4];
                    unpack4x2(trow[qq * cv], in);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int kw = qq - r;
                        if (kw >= 0 && kw < K) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) acc2[r][j] = in[j] * wrow[kw][j] + acc2[r][j];
                        }
                    }
                }
            }
            float acc[R][8];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) { acc[r][2 * j] = acc2[r][j].x; acc[r][2 * j + 1] = acc2[r][j].y; }
            uint4 ypre[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                ypre[r] = make_uint4(0, 0, 0, 0);
                if (EPI == EPI_BNBWD && ow0 + tx + r < g.W)
                    ypre[r] = *reinterpret_cast<const uint4*>(e.y + obase + (int64_t)r * g.C);
            }
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (ow0 + tx + r < g.W)
                    epilogue<EPI>(acc[r], dx, obase + (int64_t)r * g.C, ypre[r], ecl + lane_cv * 8, cv * 8, s_acc, q_acc);
        }
        // ---- weight gradient: dW[c, kh, kw] += dy[o] * a1[o + (kh, kw) - P]  (dw_bwd_weight_kernel<K, 1, R>)
        if (plw >= PLW) continue;
        for (StripWalk it = wwalk0; it.ty < TH; it.next()) {
            f2 dv[R][4];
            const uint4* drow = dt + it.o2 + doff;
#pragma unroll
            for (int r = 0; r < R; ++r) unpack4x2(drow[r * cv], dv[r]);
            const uint4* xrow = at + it.o1 + aoff;
            constexpr int NIN = R - 1 + K;
#pragma unroll
            for (int qq = 0; qq < NIN; ++qq) {
                f2 in[4];
                unpack4x2(xrow[qq * cv], in);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int kw = qq - r;
                    if (kw >= 0 && kw < K) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) wacc[kw][j] = dv[r][j] * in[j] + wacc[kw][j];
                    }
                }
            }
        }
    }
    if constexpr (EPI != EPI_NONE) write_partials(red, s_acc, q_acc, PL, pl, cv, lane_cv, ncv, v0, g.C, pdz, pdzx);
    __syncthreads();
    const int C8 = cv * 8;
    for (int i = t; i < PLW * C8 * KK; i += BLOCK) red[i] = 0.f;
    __syncthreads();
    if (plw < PLW && lane_cv < ncv) {
#pragma unroll
        for (int kw = 0; kw < K; ++kw)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                red[(plw * C8 + lane_cv * 8 + j) * KK + kh * K + kw] = (j & 1) ? wacc[kw][j >> 1].y : wacc[kw][j >> 1].x;
    }
    __syncthreads();
    for (int i = t; i < ncv * 8 * KK; i += BLOCK) {
        float a = 0.f;
        for (int p = 0; p < PLW; ++p) a += red[p * C8 * KK + i];
        dwp[(int64_t)blockIdx.x * g.C * KK + (int64_t)v0 * 8 * KK + i] = a;
    }
}

// ------------------------------------------------------------------ unified stride-1 backward
// dw_bwd_fused_kernel runs the data and the weight gradient as two passes over its staged tiles: a halo'd copy of
// act(x1) feeds the weight part, x1 is read a second time (and its sigmoid recomputed) by the BN1 epilogue, and every
// dy vector is unpacked twice.  PMC counters put that kernel at ~700 VALU instructions per output vector and ~65 %
// VALU busy (profiles/r2_pmc_dw_twopass.txt): it is issue-bound, not HBM-bound.  Both gradients walk the SAME dy
// neighbourhood of a centre pixel i:
//     dx[i]          = sum_t' wflip[t'] dy[i + t' - P]
//     dW[flip(t')]  += a[i] * dy[i + t' - P]            (a = act(x1 * scale1 + shift1))
// so one strip loop unpacks each dy vector once and feeds both products; a[i] is built in registers from x1 at the
// R strip centres with ONE sigmoid per element, shared with the BN1 epilogue's silu'; and only dy is staged in LDS
// (a bigger tile for the same budget, less halo).  The K x K weight accumulators of a thread's CPT channels stay in
// registers for the whole workgroup: k5 layers use CPT = 4 channels per thread (100 accumulators), k3 layers 8.
template <int CPT> struct ChanVec;
template <> struct ChanVec<8> {
    typedef uint4 T;
    static __device__ __forceinline__ void unpack(const T u, f2 (&f)[4]) { unpack4x2(u, f); }
    static __device__ __forceinline__ T zero() { return make_uint4(0, 0, 0, 0); }
    static __device__ __forceinline__ T pack(const f2 (&f)[4]) {
        return make_uint4(pack2(f[0].x, f[0].y), pack2(f[1].x, f[1].y), pack2(f[2].x, f[2].y), pack2(f[3].x, f[3].y));
    }
    static __device__ __forceinline__ void loadf(const float* __restrict__ p, f2 (&o)[4]) { load4x2(p, o); }
};
template <> struct ChanVec<4> {
    typedef uint2 T;
    static __device__ __forceinline__ void unpack(const T u, f2 (&f)[2]) {
#if RT1_DW_TIMING & 1   // timing-only build: the bf16 -> f32 unpack of the strip loop removed (values wrong)
        f[0] = f2{__uint_as_float(u.x), __uint_as_float(u.y)};
        f[1] = f2{__uint_as_float(u.y), __uint_as_float(u.x)};
#else
        f[0] = f2{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u)};
        f[1] = f2{__uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
#endif
    }
    static __device__ __forceinline__ T zero() { return make_uint2(0, 0); }
    static __device__ __forceinline__ T pack(const f2 (&f)[2]) {
        return make_uint2(pack2(f[0].x, f[0].y), pack2(f[1].x, f[1].y));
    }
    static __device__ __forceinline__ void loadf(const float* __restrict__ p, f2 (&o)[2]) {
        const float4 a = *reinterpret_cast<const float4*>(p);
        o[0] = f2{a.x, a.y};
        o[1] = f2{a.z, a.w};
    }
};

template <> struct ChanVec<2> {   // 2 channels per thread (k5 at higher occupancy: 25 x 2 weight accumulators)
    typedef uint32_t T;
    static __device__ __forceinline__ void unpack(const T u, f2 (&f)[1]) {
        f[0] = f2{__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)};
    }
    static __device__ __forceinline__ T zero() { return 0u; }
    static __device__ __forceinline__ T pack(const f2 (&f)[1]) { return pack2(f[0].x, f[0].y); }
    static __device__ __forceinline__ void loadf(const float* __restrict__ p, f2 (&o)[1]) {
        const float2 a = *reinterpret_cast<const float2*>(p);
        o[0] = f2{a.x, a.y};
    }
};

constexpr int DWU_SU = 4;     // dy pixels in flight per thread while staging (2: -4 %, 6 / 8 spill; profiles/r2_dw_uni_su_ab.log)
constexpr int DWU_OCC = 2;    // workgroups / CU the unified kernel's register and LDS budgets target
constexpr int DWU2_SU = 4;    // half-vector dy pixels in flight per thread while staging (2-channel form)
constexpr int DWU2_OCC = 3;   // ... its 2-channel-per-thread k5 form (fewer registers: 3 workgroups / CU)
// An offset the compiler cannot see through: keeps loop-invariant LDS reads (weights, BN constants) inside the
// strip loop.  Hoisted, the 25 x 4 weights of a k5 thread alone took 100 VGPRs and the kernel spilled.
__device__ __forceinline__ int opaque(int x) {
    asm volatile("" : "+v"(x));
    return x;
}
__device__ __forceinline__ void pin(f2& v) { asm volatile("" : "+v"(v)); }

// Strip centres' BN1 + SiLU for the unified backward kernels: z = y * sc + sh, a = silu(z) (zero where !ok: no weight
// contribution past the right edge), gp = silu'(z) = s (1 + z (1 - s)).  Written phase by phase over all R x NV channel
// pairs so that each packed op has independent ones between it and its producer: computed pair by pair, the chain's
// back-to-back dependent packed-fp32 ops each cost an s_nop (as in stage_dy; profiles/r6_dw_phased_ab.log).
template <int R, int NV>
__device__ __forceinline__ void centre_silu(const f2 (&y)[R][NV], const f2 (&sc)[NV], const f2 (&sh)[NV],
                                            const bool (&ok)[R], f2 (&a)[R][NV], f2 (&gp)[R][NV]) {
    const f2 one = f2{1.f, 1.f};
    f2 z[R][NV], t[R][NV];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < NV; ++j) z[r][j] = y[r][j] * sc[j] + sh[j];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < NV; ++j) t[r][j] = z[r][j] * f2{-1.4426950408889634f, -1.4426950408889634f};
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < NV; ++j)
            t[r][j] = f2{__builtin_amdgcn_exp2f(t[r][j].x), __builtin_amdgcn_exp2f(t[r][j].y)} + one;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < NV; ++j) t[r][j] = f2{__builtin_amdgcn_rcpf(t[r][j].x), __builtin_amdgcn_rcpf(t[r][j].y)};
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            a[r][j] = ok[r] ? z[r][j] * t[r][j] : f2{0.f, 0.f};
            gp[r][j] = one - t[r][j];
        }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < NV; ++j) gp[r][j] = z[r][j] * gp[r][j] + one;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < NV; ++j) gp[r][j] = t[r][j] * gp[r][j];
}

// XK != 0 (x-mode, expand blocks): the strip centres' y1 comes from a [TH x TW][C8] LDS tile recomputed per tile
// on MFMA from xe (stage_xmfma), not from x1 in HBM
template <int K, int R, int EPI, int CPT, int XK = 0, bool RG = false>
__global__ __launch_bounds__(BLOCK, CPT == 2 ? DWU2_OCC : DWU_OCC) void dw_bwd_uni_kernel(DyBnBwd d, const bf16_t* __restrict__ x1,
                                                                        const float* __restrict__ w, DwGeo g,
                                                                        int TH, int TW, BnBwdEpi e,
                                                                        bf16_t* __restrict__ dx, float* __restrict__ pdz,
                                                                        float* __restrict__ pdzx,
                                                                        float* __restrict__ dwp, int red_taps, XExp xe,
                                                                        int sb) {
    using CV = ChanVec<CPT>;
    using V = typename CV::T;
    constexpr int P = (K - 1) / 2, KK = K * K, NV = CPT / 2, HPV = 8 / CPT;
    static_assert(XK == 0 || EPI == EPI_BNBWD, "x-mode is for expand blocks (BN1 epilogue)");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int IH = TH + K - 1, IW = TW + K - 1;
    const int cv = g.cv, C8 = cv * 8, nlc = cv * HPV;
    uint4* dt = reinterpret_cast<uint4*>(smem);
    float* wl = reinterpret_cast<float*>(dt + IH * IW * cv);
    float* ecl = wl + KK * C8;
    bf16_t* yl = reinterpret_cast<bf16_t*>(ecl + (EPI == EPI_BNBWD ? 4 * C8 : 0));   // x-mode y1 centre tile
    bf16_t* wel = yl + (sb > 0 ? sb * R : TH * TW) * C8;                               // x-mode We rows
    float* red = reinterpret_cast<float*>(smem);  // aliases the tile once the last tile is consumed

    const int v0 = blockIdx.y * cv;
    const int ncv = min(cv, g.nv - v0);
    const int t = threadIdx.x;
    if constexpr (XK != 0) stage_xweights<xk_kc(XK)>(wel, xe, C8, v0 * 8, ncv * 8);
    const int lane_c = t % nlc, pl = t / nlc, PL = BLOCK / nlc;   // CPT channels of lane_c, strip lane pl
    const int cofs = lane_c * CPT;                                  // channel offset inside the chunk
    const bool active = lane_c / HPV < ncv && pl < PL;
    const int groups_w = TW / R;
    // o1: the strip window's origin in the dy tile (V units), o2: its first output in global memory (elements)
    const StripWalk walk0(pl, PL, groups_w, IW * nlc, R * nlc, g.W * g.C, R * g.C);

    for (int i = t; i < KK * C8; i += BLOCK) {   // the flipped taps, read straight from the unflipped weight
        const int tap = i / C8, cc = i % C8;
        wl[i] = (cc < ncv * 8) ? w[(int64_t)(v0 * 8 + cc) * KK + (KK - 1 - tap)] : 0.f;
    }
    stage_epi_consts<EPI>(ecl, e, v0, ncv, cv);   // [scale1, shift1, rstd1, -mean1 * rstd1]
    const int tiles_h = (g.H + TH - 1) / TH, tiles_w = (g.W + TW - 1) / TW;
    const int64_t ntiles = (int64_t)g.N * tiles_h * tiles_w;
    f2 wacc[KK][NV], s_acc[NV], q_acc[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        s_acc[j] = q_acc[j] = f2{0.f, 0.f};
#pragma unroll
        for (int a = 0; a < KK; ++a) wacc[a][j] = f2{0.f, 0.f};
    }

    constexpr bool CS = XK == 0 && centre_stage_on(CPT, R);
    for (int64_t tile_id = blockIdx.x; tile_id < ntiles; tile_id += gridDim.x) {
        const int n = (int)(tile_id / (tiles_h * tiles_w));
        const int rem = (int)(tile_id - (int64_t)n * tiles_h * tiles_w);
        const int oh0 = (rem / tiles_w) * TH, ow0 = (rem % tiles_w) * TW;
        __syncthreads();
        if constexpr (CS) {
            // centre tile -> yl [TH * TW][C8] by LDS-DMA: entry i = (pixel i / cv, vector i % cv); one wave
            // instruction lands 64 consecutive entries (1 KiB) at yl + i0 * 16.  Pixels past the map's edge and idle
            // vectors of a short chunk read the frame's first vector instead (never used: their strips are masked)
            const int nvec = TH * TW * cv, lane = t & 63;
            const bf16_t* fb = x1 + (int64_t)n * g.H * g.W * g.C;
            for (int i0 = (t >> 6) * 64; i0 < nvec; i0 += BLOCK) {
                const int i = i0 + lane;
                if (i < nvec) {
                    const int px = i / cv, v = i - px * cv;
                    const int py = px / TW, pxx = px - py * TW;
                    const bool ok = v < ncv && oh0 + py < g.H && ow0 + pxx < g.W;
                    const bf16_t* src = ok ? fb + ((int64_t)(oh0 + py) * g.W + ow0 + pxx) * g.C + (v0 + v) * 8 : fb;
                    __builtin_amdgcn_global_load_lds(src, (dw_lds_void*)(yl + (size_t)i0 * 8), 16, 0, 0);
                }
            }
        }
#if !(RT1_DW_TIMING & 2)   // timing-only build (tools/bench_dw_phases.py): no dy staging
        if constexpr (CPT == 2) stage_dy_half<DWU2_SU, RG>(dt, d, g, n, oh0 - P, ow0 - P, IH, IW, v0, ncv);
        else stage_dy<DWU_SU, RG>(dt, d, g, n, oh0 - P, ow0 - P, IH, IW, v0, ncv);
#endif
        if constexpr (CS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the centre DMA has landed
        // x-mode: the strips in bands of sb (a whole number of PL-strip rounds); strip s = ty * groups_w + gx has its R
        // centres at the row-major centre pixels [s R, s R + R), so a band's y1 is one contiguous pixel run.  Otherwise
        // one band of all strips.
        const int nstrips = TH * groups_w, sbw = (XK != 0 && sb > 0) ? sb : nstrips;
        for (int s0 = 0; s0 < nstrips; s0 += sbw) {
        const int s1 = XK != 0 ? min(nstrips, s0 + sbw) : nstrips;
        if constexpr (XK != 0) {
            if (s0 > 0) __syncthreads();                      // the previous band's centre reads are done
            stage_xmfma<xk_kc(XK), xk_ng(XK), false, true>(yl, C8, xe, g.H, g.W, n, oh0, ow0, TH, TW, v0 * 8, ncv * 8,
                                                           nullptr, wel, 1, s0 * R, (s1 - s0) * R);
        }
        __syncthreads();
        if (!active) {
            if constexpr (XK != 0) continue;
            else break;
        }
        const int64_t tbase = (((int64_t)n * g.H + oh0) * g.W + ow0) * g.C + v0 * 8 + cofs;
        // x1 at a strip's R centres (zero past the right / bottom edge).  CPREF: the NEXT strip's centres are loaded
        // while this strip computes -- loaded at the strip's start, every strip waits a full HBM round trip (plus the
        // previous strip's stores, vmcnt counts both) right before its sigmoids.  Only the 2-channel R = 4 form
        // (19 x 19 k5 layers) has the registers: -3.6..-4.2 % there; the 4- / 8-channel and R = 5 forms spill and
        // lose 3-36 % (profiles/r6_dw_prefetch_ab.log)
        auto centre_load = [&](const StripWalk& w, V (&dst)[R]) {
            const bool rowok = w.ty < TH && oh0 + w.ty < g.H;
#pragma unroll
            for (int r = 0; r < R; ++r)
                dst[r] = (rowok && ow0 + w.gx * R + r < g.W)
                             ? *reinterpret_cast<const V*>(x1 + tbase + w.o2 + (int64_t)r * g.C)
                             : CV::zero();
        };
        constexpr bool CPREF = XK == 0 && !CS && DW_CENTRE_PREFETCH && CPT == 2 && R == 4;
        V ynext[R];
        if constexpr (CPREF) centre_load(walk0, ynext);
        int si = s0 + pl;
        for (StripWalk it = (XK != 0 && s0) ? StripWalk(s0 + pl, PL, groups_w, IW * nlc, R * nlc, g.W * g.C, R * g.C)
                                            : walk0;
             (XK == 0 || si < s1) && it.ty < TH; it.next(), si += (XK != 0 ? PL : 0)) {
            const int tx = it.gx * R;
            if (oh0 + it.ty >= g.H) break;                    // rows only grow along the walk
            const int64_t obase = tbase + it.o2;
            const int co = opaque(cofs);
            // ---- strip centres: a = act(x1*scale1 + shift1) (zero past the right edge: no weight contribution)
            V yr[R];
            if constexpr (CPREF) {
#pragma unroll
                for (int r = 0; r < R; ++r) yr[r] = ynext[r];
                StripWalk nx = it;
                nx.next();
                centre_load(nx, ynext);
            } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
#if RT1_DW_TIMING & 16   // timing-only build: no strip-centre loads
                yr[r] = CV::zero();
#else
                if constexpr (XK != 0)
                    yr[r] = *reinterpret_cast<const V*>(yl + ((si - s0) * R + r) * C8 + co);
                else if constexpr (CS)   // past the right edge: zero (the EPI_NONE weight product uses x1 raw)
                    yr[r] = (ow0 + tx + r < g.W) ? *reinterpret_cast<const V*>(yl + (it.ty * TW + tx + r) * C8 + co)
                                                 : CV::zero();
                else
                    yr[r] = (ow0 + tx + r < g.W) ? *reinterpret_cast<const V*>(x1 + obase + (int64_t)r * g.C)
                                                 : CV::zero();
#endif
            }
            }
            f2 a[R][NV], gp[R][NV];
#if RT1_DW_TIMING & 16   // ... and no BN1 + SiLU recompute
            if constexpr (false) {
#else
            if constexpr (EPI == EPI_BNBWD) {
#endif
                f2 sc[NV], sh[NV];
                CV::loadf(ecl + co, sc);
                CV::loadf(ecl + C8 + co, sh);
                f2 y[R][NV];
                bool ok[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    CV::unpack(yr[r], y[r]);
                    ok[r] = ow0 + tx + r < g.W;
                }
                centre_silu<R, NV>(y, sc, sh, ok, a, gp);
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) CV::unpack(yr[r], a[r]);
            }
            // ---- one pass over the dy window: data and weight products from each unpacked vector
            f2 acc[R][NV];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < NV; ++j) acc[r][j] = f2{0.f, 0.f};
            const V* trow = reinterpret_cast<const V*>(dt) + it.o1 + lane_c;
#if RT1_DW_TIMING & 4     // timing-only build: no tap loop
#pragma unroll
            for (int kr = 0; kr < 0; ++kr) {
#else
#pragma unroll
            for (int kr = 0; kr < K; ++kr) {
#endif
                f2 wrow[K][NV];
#pragma unroll
                for (int kw = 0; kw < K; ++kw) CV::loadf(wl + (kr * K + kw) * C8 + co, wrow[kw]);
                constexpr int NIN = R - 1 + K;
#pragma unroll
                for (int qq = 0; qq < NIN; ++qq) {
                    f2 in[NV];
                    CV::unpack(trow[(kr * IW + qq) * nlc], in);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int kw = qq - r;
                        if (kw >= 0 && kw < K) {
#pragma unroll
                            for (int j = 0; j < NV; ++j) {
                                acc[r][j] = in[j] * wrow[kw][j] + acc[r][j];
                                wacc[kr * K + kw][j] = in[j] * a[r][j] + wacc[kr * K + kw][j];
                            }
                        }
                    }
                }
                // one kernel row at a time: pin this row's products here.  Left free, LLVM sinks the data products
                // into the epilogue's `ow < W` branch, so every row's unpacked dy stays live to the end of the strip
                // and the K*K*CPT weight accumulators no longer fit beside them (the kernel spilled 180-460 VGPRs)
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int j = 0; j < NV; ++j) pin(acc[r][j]);
#pragma unroll
                for (int kw = 0; kw < K; ++kw)
#pragma unroll
                    for (int j = 0; j < NV; ++j) pin(wacc[kr * K + kw][j]);
            }
            // ---- epilogue: store dx (bf16); BN1 backward partials of dz = dx * silu'(z), dz * xhat
            f2 rr[NV], mr[NV];
            if constexpr (EPI == EPI_BNBWD) {
                CV::loadf(ecl + 2 * C8 + co, rr);
                CV::loadf(ecl + 3 * C8 + co, mr);
            }
#if RT1_DW_TIMING & 8      // timing-only build: no stores / statistics (a data-dependent guard keeps the products)
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (acc[r][0].x == 1234.5f) dx[obase + (int64_t)r * g.C] = (bf16_t)1;
            if constexpr (false)
#endif
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (ow0 + tx + r >= g.W) continue;
                if constexpr (EPI == EPI_BNBWD) {
                    if (e.zout) {
#pragma unroll
                        for (int j = 0; j < NV; ++j) acc[r][j] = acc[r][j] * gp[r][j];
                    }
                }
                if constexpr (EPI == EPI_NONE) {
                    if (e.res) {
                        f2 rv[NV], fm[NV];
                        CV::unpack(*reinterpret_cast<const V*>(e.res + obase + (int64_t)r * g.C), rv);
                        CV::loadf(e.rmul + (int64_t)n * g.C + v0 * 8 + co, fm);
#pragma unroll
                        for (int j = 0; j < NV; ++j) acc[r][j] = rv[j] * fm[j] + acc[r][j];
                    }
                }
                const V o = CV::pack(acc[r]);
                *reinterpret_cast<V*>(dx + obase + (int64_t)r * g.C) = o;
                if constexpr (EPI == EPI_BNBWD) {
                    f2 of[NV], y[NV];
                    CV::unpack(o, of);                        // statistics describe the stored bf16 tensor
                    CV::unpack(yr[r], y);
#pragma unroll
                    for (int j = 0; j < NV; ++j) {
                        f2 dz = of[j];
                        if (!e.zout) dz = dz * gp[r][j];
                        s_acc[j] = s_acc[j] + dz;
                        q_acc[j] = dz * (y[j] * rr[j] + mr[j]) + q_acc[j];
                    }
                }
            }
        }
        if constexpr (XK == 0) break;                       // one band
        }   // band
    }
    // ---- workgroup reductions over the strip lanes (fixed order): BN1 partials, then the weight taps in passes
    const int nc = ncv * 8;
    if constexpr (EPI != EPI_NONE) {
        __syncthreads();
        if (active) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                red[pl * C8 + cofs + 2 * j] = s_acc[j].x;
                red[pl * C8 + cofs + 2 * j + 1] = s_acc[j].y;
                red[(PL + pl) * C8 + cofs + 2 * j] = q_acc[j].x;
                red[(PL + pl) * C8 + cofs + 2 * j + 1] = q_acc[j].y;
            }
        }
        __syncthreads();
        for (int cc = t; cc < nc; cc += BLOCK) {
            float sa = 0.f, sb = 0.f;
            for (int p = 0; p < PL; ++p) {
                sa += red[p * C8 + cc];
                sb += red[(PL + p) * C8 + cc];
            }
            pdz[(int64_t)blockIdx.x * g.C + v0 * 8 + cc] = sa;
            pdzx[(int64_t)blockIdx.x * g.C + v0 * 8 + cc] = sb;
        }
    }
    for (int t0 = 0; t0 < KK; t0 += red_taps) {
        const int tn = min(red_taps, KK - t0);
        __syncthreads();
        if (active) {
#pragma unroll
            for (int tap = 0; tap < KK; ++tap) {
                if (tap < t0 || tap >= t0 + tn) continue;
                float* rp = red + ((tap - t0) * PL + pl) * C8 + cofs;
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    rp[2 * j] = wacc[tap][j].x;
                    rp[2 * j + 1] = wacc[tap][j].y;
                }
            }
        }
        __syncthreads();
        for (int i = t; i < tn * nc; i += BLOCK) {
            const int tt = i / nc, cc = i - tt * nc;
            float s = 0.f;
            for (int p = 0; p < PL; ++p) s += red[(tt * PL + p) * C8 + cc];
            // accumulator tap t' of the flipped kernel is tap KK-1-t' of the weight
            dwp[(int64_t)blockIdx.x * g.C * KK + (int64_t)(v0 * 8 + cc) * KK + (KK - 1 - (t0 + tt))] = s;
        }
    }
}

// ------------------------------------------------------------------ unified stride-2 backward
// The same single pass for the stride-2 blocks (2, 5, 8, 18), over the INPUT pixels i (strip centres):
//     dx[i]       = sum_{t: i + P - t even} w[t] dy[(i + P - t) / 2]
//     dW[t]      += a[i] * dy[(i + P - t) / 2]
// A centre only meets the taps of its parity class (row parity PR, column parity PC): the workgroup walks the four
// classes one after another, each a compile-time sub-kernel ((K+1)/2 or K/2 taps per axis) over the strips of that
// class (R centres 2 apart along W: their dy columns are consecutive), so no lane branches on parity.  dy is staged
// once per tile at the output resolution with the BN2 backward-apply prologue (stage_dy), a quarter of the centres'
// pixel count plus halo.
template <int K, int R, int EPI, int CPT, int PR, int PC, bool XM>
__device__ __forceinline__ void uni_s2_class(const uint4* __restrict__ dt, const float* __restrict__ wl,
                                             const float* __restrict__ ecl, const bf16_t* __restrict__ x1,
                                             bf16_t* __restrict__ dx, const DwGeo& g, int C8, int nlc, int lane_c,
                                             int cofs, int pl, int PL, int TH, int TW, int DW, int ih0, int iw0,
                                             int oh_lo, int ow_lo, int64_t tbase, f2 (&wacc)[K * K][CPT / 2],
                                             f2 (&s_acc)[CPT / 2], f2 (&q_acc)[CPT / 2], int zout,
                                             const bf16_t* __restrict__ yl) {
    using CV = ChanVec<CPT>;
    using V = typename CV::T;
    constexpr int P = (K - 1) / 2, NV = CPT / 2;
    // valid taps of this class: kh = KH0, KH0 + 2, ... (NKH of them); kw likewise
    constexpr int KH0 = (PR + P) & 1, KW0 = (PC + P) & 1;
    constexpr int NKH = (K - KH0 + 1) / 2, NKW = (K - KW0 + 1) / 2;
    constexpr int KWMAX = KW0 + 2 * (NKW - 1);
    constexpr int NIN = R + NKW - 1;
    const int groups_w = TW / (2 * R);
    // o1: dy-tile element (V units) of class row cr / strip gx; o2: global element offset of its first centre
    StripWalk it(pl, PL, groups_w, DW * nlc, R * nlc, 2 * g.W * g.C, 2 * R * g.C);
    const int64_t cbase = tbase + ((int64_t)PR * g.W + PC) * g.C;
    for (; 2 * it.ty + PR < TH; it.next()) {
        const int ih = ih0 + PR + 2 * it.ty;
        if (ih >= g.H) break;                                  // rows only grow along the walk
        const int iwb = iw0 + PC + 2 * R * it.gx;
        const int64_t obase = cbase + it.o2;
        const int co = opaque(cofs);
        V yr[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if constexpr (XM)   // x-mode: this class's centres in LDS, [TH/2][TW/2] (class row ty, column R gx + r)
                yr[r] = *reinterpret_cast<const V*>(yl + (it.ty * (TW / 2) + R * it.gx + r) * C8 + co);
            else
                yr[r] = (iwb + 2 * r < g.W) ? *reinterpret_cast<const V*>(x1 + obase + (int64_t)2 * r * g.C)
                                            : CV::zero();
        }
        f2 a[R][NV], gp[R][NV];
        if constexpr (EPI == EPI_BNBWD) {
            f2 sc[NV], sh[NV];
            CV::loadf(ecl + co, sc);
            CV::loadf(ecl + C8 + co, sh);
            f2 y[R][NV];
            bool ok[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                CV::unpack(yr[r], y[r]);
                ok[r] = iwb + 2 * r < g.W;
            }
            centre_silu<R, NV>(y, sc, sh, ok, a, gp);
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) CV::unpack(yr[r], a[r]);
        }
        f2 acc[R][NV];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < NV; ++j) acc[r][j] = f2{0.f, 0.f};
        // dy row of tap kh: (ih + P - kh)/2 - oh_lo; column of (r, kw): (iwb + P - kw)/2 + r - ow_lo
        const int row0 = ((ih + P - KH0) >> 1) - oh_lo, col0 = ((iwb + P - KWMAX) >> 1) - ow_lo;
        const V* tw = reinterpret_cast<const V*>(dt) + (row0 * DW + col0) * nlc + lane_c;
#pragma unroll
        for (int ih_ = 0; ih_ < NKH; ++ih_) {
            const int kh = KH0 + 2 * ih_;
            f2 wrow[NKW][NV];
#pragma unroll
            for (int jw = 0; jw < NKW; ++jw) CV::loadf(wl + (kh * K + KWMAX - 2 * jw) * C8 + co, wrow[jw]);
            const V* trow = tw - ih_ * DW * nlc;               // kh + 2 -> one dy row up
#pragma unroll
            for (int q = 0; q < NIN; ++q) {
                f2 in[NV];
                CV::unpack(trow[q * nlc], in);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int jw = q - r;                       // kw = KWMAX - 2 jw
                    if (jw >= 0 && jw < NKW) {
#pragma unroll
                        for (int j = 0; j < NV; ++j) {
                            acc[r][j] = in[j] * wrow[jw][j] + acc[r][j];
                            wacc[kh * K + KWMAX - 2 * jw][j] = in[j] * a[r][j] + wacc[kh * K + KWMAX - 2 * jw][j];
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < NV; ++j) pin(acc[r][j]);
#pragma unroll
            for (int jw = 0; jw < NKW; ++jw)
#pragma unroll
                for (int j = 0; j < NV; ++j) pin(wacc[kh * K + KWMAX - 2 * jw][j]);
        }
        f2 rr[NV], mr[NV];
        if constexpr (EPI == EPI_BNBWD) {
            CV::loadf(ecl + 2 * C8 + co, rr);
            CV::loadf(ecl + 3 * C8 + co, mr);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (iwb + 2 * r >= g.W) continue;
            if constexpr (EPI == EPI_BNBWD) {
                if (zout) {
#pragma unroll
                    for (int j = 0; j < NV; ++j) acc[r][j] = acc[r][j] * gp[r][j];
                }
            }
            const V o = CV::pack(acc[r]);
            *reinterpret_cast<V*>(dx + obase + (int64_t)2 * r * g.C) = o;
            if constexpr (EPI == EPI_BNBWD) {
                f2 of[NV], y[NV];
                CV::unpack(o, of);
                CV::unpack(yr[r], y);
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    f2 dz = of[j];
                        if (!zout) dz = dz * gp[r][j];
                    s_acc[j] = s_acc[j] + dz;
                    q_acc[j] = dz * (y[j] * rr[j] + mr[j]) + q_acc[j];
                }
            }
        }
    }
}

template <int K, int R, int EPI, int CPT, int XK = 0, bool RG = false>
__global__ __launch_bounds__(BLOCK, DWU_OCC) void dw_bwd_uni_s2_kernel(DyBnBwd d, const bf16_t* __restrict__ x1,
                                                                           const float* __restrict__ w, DwGeo g,
                                                                           int TH, int TW, BnBwdEpi e,
                                                                           bf16_t* __restrict__ dx,
                                                                           float* __restrict__ pdz,
                                                                           float* __restrict__ pdzx,
                                                                           float* __restrict__ dwp, int red_taps,
                                                                           XExp xe) {
    constexpr int P = (K - 1) / 2, KK = K * K, NV = CPT / 2, HPV = 8 / CPT;
    static_assert(XK == 0 || EPI == EPI_BNBWD, "x-mode is for expand blocks (BN1 epilogue)");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int DH = (TH + K) / 2 + 1, DW = (TW + K) / 2 + 1;
    const int cv = g.cv, C8 = cv * 8, nlc = cv * HPV;
    uint4* dt = reinterpret_cast<uint4*>(smem);
    float* wl = reinterpret_cast<float*>(dt + DH * DW * cv);
    float* ecl = wl + KK * C8;
    bf16_t* yl = reinterpret_cast<bf16_t*>(ecl + (EPI == EPI_BNBWD ? 4 * C8 : 0));   // x-mode y1 centre tile
    bf16_t* wel = yl + (TH / 2) * (TW / 2) * C8;                                       // x-mode We rows
    float* red = reinterpret_cast<float*>(smem);

    const int v0 = blockIdx.y * cv;
    const int ncv = min(cv, g.nv - v0);
    const int t = threadIdx.x;
    if constexpr (XK != 0) stage_xweights<xk_kc(XK)>(wel, xe, C8, v0 * 8, ncv * 8);
    const int lane_c = t % nlc, pl = t / nlc, PL = BLOCK / nlc;
    const int cofs = lane_c * CPT;
    const bool active = lane_c / HPV < ncv && pl < PL;
    DwGeo go = g;                 // dy lives at the output resolution (stage_dy reads H, W as the map size)
    go.H = g.Ho;
    go.W = g.Wo;

    for (int i = t; i < KK * C8; i += BLOCK) {
        const int tap = i / C8, cc = i % C8;
        wl[i] = (cc < ncv * 8) ? w[(int64_t)(v0 * 8 + cc) * KK + tap] : 0.f;
    }
    stage_epi_consts<EPI>(ecl, e, v0, ncv, cv);
    const int tiles_h = (g.H + TH - 1) / TH, tiles_w = (g.W + TW - 1) / TW;
    const int64_t ntiles = (int64_t)g.N * tiles_h * tiles_w;
    f2 wacc[KK][NV], s_acc[NV], q_acc[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        s_acc[j] = q_acc[j] = f2{0.f, 0.f};
#pragma unroll
        for (int a = 0; a < KK; ++a) wacc[a][j] = f2{0.f, 0.f};
    }
    for (int64_t tile_id = blockIdx.x; tile_id < ntiles; tile_id += gridDim.x) {
        const int n = (int)(tile_id / (tiles_h * tiles_w));
        const int rem = (int)(tile_id - (int64_t)n * tiles_h * tiles_w);
        const int ih0 = (rem / tiles_w) * TH, iw0 = (rem % tiles_w) * TW;   // TH, TW even
        const int oh_lo = (ih0 + P - (K - 1)) >> 1, ow_lo = (iw0 + P - (K - 1)) >> 1;
        __syncthreads();
        stage_dy<DWU_SU, RG>(dt, d, go, n, oh_lo, ow_lo, DH, DW, v0, ncv);
        const int64_t tbase = (((int64_t)n * g.H + ih0) * g.W + iw0) * g.C + v0 * 8 + cofs;
        if constexpr (XK != 0) {
            // x-mode: y1 of ONE parity class's centres at a time ([TH/2][TW/2]: a quarter of the tile in LDS)
#define CLS(PR_, PC_)                                                                                              \
    if (PR_ | PC_) __syncthreads();                                                                                \
    stage_xmfma<xk_kc(XK), xk_ng(XK), false, true>(yl, C8, xe, g.H, g.W, n, ih0 + PR_, iw0 + PC_, TH / 2, TW / 2,   \
                                                   v0 * 8, ncv * 8, nullptr, wel, 2);                              \
    __syncthreads();                                                                                               \
    if (active)                                                                                                    \
        uni_s2_class<K, R, EPI, CPT, PR_, PC_, true>(dt, wl, ecl, x1, dx, g, C8, nlc, lane_c, cofs, pl, PL, TH, TW, DW, \
                                                     ih0, iw0, oh_lo, ow_lo, tbase, wacc, s_acc, q_acc, e.zout, yl)
            CLS(0, 0);
            CLS(0, 1);
            CLS(1, 0);
            CLS(1, 1);
#undef CLS
            continue;
        }
        __syncthreads();
        if (!active) continue;
#define CLS(PR_, PC_)                                                                                              \
    uni_s2_class<K, R, EPI, CPT, PR_, PC_, false>(dt, wl, ecl, x1, dx, g, C8, nlc, lane_c, cofs, pl, PL, TH, TW, DW, \
                                                  ih0, iw0, oh_lo, ow_lo, tbase, wacc, s_acc, q_acc, e.zout, yl)
        CLS(0, 0);
        CLS(0, 1);
        CLS(1, 0);
        CLS(1, 1);
#undef CLS
    }
    const int nc = ncv * 8;
    if constexpr (EPI != EPI_NONE) {
        __syncthreads();
        if (active) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                red[pl * C8 + cofs + 2 * j] = s_acc[j].x;
                red[pl * C8 + cofs + 2 * j + 1] = s_acc[j].y;
                red[(PL + pl) * C8 + cofs + 2 * j] = q_acc[j].x;
                red[(PL + pl) * C8 + cofs + 2 * j + 1] = q_acc[j].y;
            }
        }
        __syncthreads();
        for (int cc = t; cc < nc; cc += BLOCK) {
            float sa = 0.f, sb = 0.f;
            for (int p = 0; p < PL; ++p) {
                sa += red[p * C8 + cc];
                sb += red[(PL + p) * C8 + cc];
            }
            pdz[(int64_t)blockIdx.x * g.C + v0 * 8 + cc] = sa;
            pdzx[(int64_t)blockIdx.x * g.C + v0 * 8 + cc] = sb;
        }
    }
    for (int t0 = 0; t0 < KK; t0 += red_taps) {
        const int tn = min(red_taps, KK - t0);
        __syncthreads();
        if (active) {
#pragma unroll
            for (int tap = 0; tap < KK; ++tap) {
                if (tap < t0 || tap >= t0 + tn) continue;
                float* rp = red + ((tap - t0) * PL + pl) * C8 + cofs;
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    rp[2 * j] = wacc[tap][j].x;
                    rp[2 * j + 1] = wacc[tap][j].y;
                }
            }
        }
        __syncthreads();
        for (int i = t; i < tn * nc; i += BLOCK) {
            const int tt = i / nc, cc = i - tt * nc;
            float s = 0.f;
            for (int p = 0; p < PL; ++p) s += red[(tt * PL + p) * C8 + cc];
            dwp[(int64_t)blockIdx.x * g.C * KK + (int64_t)(v0 * 8 + cc) * KK + t0 + tt] = s;
        }
    }
}

// ================================================================== launch plan (dw/dw_plan.h)
DwGeo make_geo(int N, int H, int W, int C, int k, int s) {
    DwGeo g;
    g.N = N; g.H = H; g.W = W; g.C = C; g.k = k; g.s = s; g.pad = (k - 1) / 2;
    g.Ho = (H + 2 * g.pad - k) / s + 1;
    g.Wo = (W + 2 * g.pad - k) / s + 1;
    g.nv = C / 8;
    // channel vectors per workgroup: 8 (a pixel's chunk = one 128-B line) unless that leaves > 15 % of the
    // lanes idle, e.g. 144 channels = 3 x 6 vectors instead of 8+8+2.  (Smaller chunks misalign the
    // pixel rows with the 128-B lines, which measured slower for 288/816/1392 channels: 2-11 % idle.)
    g.cv = g.nv;
    if (g.nv > 8) {
        g.cv = 8;
        const int slots8 = (g.nv + 7) / 8 * 8;
        if (slots8 * 100 > g.nv * 115) {
            int slots = slots8;
            for (int cv = 7; cv >= 4; --cv) {
                const int sl = (g.nv + cv - 1) / cv * cv;
                if (sl < slots) { slots = sl; g.cv = cv; }
            }
        }
    }
    // Up to 18 vectors (144 channels) one workgroup takes the whole pixel row.  Measured on block 2 (144 ch,
    // k3 s2, 150x150): forward -35 %, stride-2 backward data -55 % against 3 chunks of 6; 192 / 288 channels
    // get slower whole-row (fewer strip lanes per workgroup), so they keep the 8-vector chunks.
    if (g.nv <= DW_FULLROW_MAX) g.cv = g.nv;
    // 288 channels: 3 chunks of 12 vectors beat 5 chunks of 8 by 10 % over the three kernels (blocks 6-8);
    // the other widths measured best as above (profiles/r1_dw_chunking_ab.log)
    if (g.nv == 36) g.cv = 12;
    g.chunks = (g.nv + g.cv - 1) / g.cv;
    return g;
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// x-mode specialisation key of a layer (Cin input channels, C = Ce depthwise channels): KC * 16 + NG with the
// channel chunk C8 = cv * 8 = NG * 16; 0 = no x-mode shape (Cin % 8, Cin > 64 or a chunk that is not 16-aligned)
int xk_of(int cin, int C, int k, int s) {
    const DwGeo g = make_geo(1, 8, 8, C, k, s);
    const int C8 = g.cv * 8, kc = (cin + 31) / 32, ng = C8 / 16;
    if (cin <= 0 || cin % 8 || kc > 2 || C8 % 16 || ng > 15) return 0;
    return kc * 16 + ng;
}

// is (k, xk) one of the compiled x-mode specialisations of this stride
bool x_supported(int k, int s, int xk) {
#define X(KK, XX) if (k == KK && xk == XX) return true;
    if (s == 1) { DW_XMODE_S1(X) } else { DW_XMODE_S2(X) }
#undef X
    return false;
}

// ---------------------------------------------------------------- tile selection
// A workgroup's 256 threads form `slots` strip lanes; a tile of G strips takes ceil(G / slots) rounds,
// so a tile shape that leaves the last round mostly idle (35 strips on 32 lanes) costs nearly 2x.
// The shape is chosen per layer by minimising a per-thread instruction-slot model over all tile
// shapes that fit the LDS budget (3 workgroups/CU):
//   cost = tiles * (ceil(strips / slots) * strip_cost + ceil(staged vectors / 256) * stage_cost + sync)
// strip/stage costs are VALU instruction counts read off the gfx950 ISA of each kernel.
constexpr int DW_R5_MASK = 1;   // profiles/r3_dw_r5_ab.log: forward +0.3 %; the k5 unified backward at R=5 spills 69 VGPRs, -1.6 %
constexpr int DWU_LDS_KB = 76;     // unified backward: one staged dy tile, 2 workgroups / CU
// The k5 unified backward (y1 in HBM, not x-mode) with 2 channels per thread -- 50 weight-gradient
// accumulators instead of 100, so DWU2_OCC workgroups / CU fit (tiles within DWU2_LDS_KB of LDS)
constexpr int DWU2_LDS_KB = 52;
// is used per layer on maps of <= DWU2_MAX_PIX pixels, where its third workgroup per CU pays (10x10: 570 -> 502 us,
// 19x19 x 576: 731 -> 703 us; 38x38: 1461 -> 1600 us, profiles/r4_dw_c2_ab.log).
constexpr int DWU2_MAX_PIX = 400;
inline int uni_kind(int K, int xk, int H, int W) {
    if (K == 5 && xk == 0 && H * W <= DWU2_MAX_PIX) return TK_BWD_U2;
    return (K == 3 ? DWU_CPT3 : DWU_CPT5) == 4 ? TK_BWD_U4 : TK_BWD_U8;
}
inline bool is_uni2(int kind) { return kind == TK_BWD_V4 || kind == TK_BWD_V8; }
// 5-output strips on maps whose width is a multiple of 5 but not of 4 (150, 75, 10): the strips then tile the row
// exactly (10x10: no third of a 12-wide tile idles) and each staged input vector feeds one more output.
// DW_R5_MASK: 1 = forward / stride-1 data-gradient kernels, 2 = unified k5 backward.  x-mode kernels keep their one
// strip length.
inline bool r5_fits(int W, int xk, int bit) { return xk == 0 && W > 0 && W % 5 == 0 && W % 4 != 0 && (DW_R5_MASK & bit); }
inline int uni_r(int K, int W, int xk, int cpt) {
    // the 2-channel form has the registers for 5-output strips on the 10-wide maps (no idle third of a 12-wide tile)
    if (K == 5 && cpt == 2 && xk == 0 && W > 0 && W % 5 == 0 && W % 4 != 0) return 5;
    return K == 3 ? DWU_R3 : (r5_fits(W, xk, 2) ? 5 : DWU_R5);
}
inline int uni2_kind(int K) { return (K == 3 ? DWV_CPT3 : DWV_CPT5) == 4 ? TK_BWD_V4 : TK_BWD_V8; }
inline int uni2_r(int K) { return K == 3 ? DWV_R3 : DWV_R5; }
inline int kind_cpt(int kind) {
    return kind == TK_BWD_U2 ? 2 : (kind == TK_BWD_U4 || kind == TK_BWD_V4) ? 4 : 8;
}
// variant: 0 = two-pass fused kernel, 1 = unified kernel, -1 = per-layer default.  The unified kernel builds its
// operand as BN1 + SiLU exactly when the BN1 epilogue is on (expand blocks) and uses x1 raw otherwise.
inline bool use_uni(int variant, bool pro, bool epi) {
    if (pro != epi) return false;
    return variant != 0;
}
inline int fwd_r(int S, int Wo, int xk) { return S == 1 && r5_fits(Wo, xk, 1) ? 5 : DW_R1; }
struct TileChoice { int TH, TW, sb = 0; };   // sb: x-mode stride-1 backward strips per band (0 = all)

constexpr int DW_LDS_KB = 52;      // LDS per workgroup the tile search may use (occupancy = 160 KB / this)
constexpr size_t LDS_BUDGET = DW_LDS_KB * 1024;
constexpr int DWF_LDS_KB = 76;     // fused backward: two staged tiles, 2 workgroups / CU

// R: the strip length of the request (unified kernels only).  xk != 0 (x-mode): the forward adds BN1's staged
// constants, the unified backward kernels the y1 centre buffer (stride 1: a band of sb strips, or the whole tile;
// stride 2: one parity class, TH/2 x TW/2) and the We image
size_t tile_lds(int kind, int K, int S, int cv, bool epi, int R, int TH, int TW, int xk, int sb) {
    const size_t ec = epi ? (size_t)cv * 8 * 4 * 4 : 0;
    const size_t ypix = is_uni2(kind) ? (size_t)(TH / 2) * (TW / 2) : (sb > 0 ? (size_t)sb * R : (size_t)TH * TW);
    const size_t xt = xk ? ypix * cv * 16 + (size_t)cv * 8 * ((xk >> 4) * 32 + 8) * 2 : 0;
    if (kind == TK_FWD) {
        const int IH = (TH - 1) * S + K, IW = (TW - 1) * S + K;
        const size_t a = (size_t)IH * IW * cv * 16 + (size_t)K * K * cv * 8 * 4 + ec + (xk ? (size_t)cv * 8 * 2 * 4 : 0);
        const size_t red = (size_t)(BLOCK / cv) * cv * 8 * 2 * 4;
        return a > red ? a : red;
    }
    if (kind == TK_BWD_W) {
        const int IH = (TH - 1) * S + K, IW = (TW - 1) * S + K;
        const size_t a = (size_t)IH * IW * cv * 16 + (size_t)TH * TW * cv * 16;
        const size_t red = (size_t)(BLOCK / (cv * K)) * cv * 8 * K * K * 4;
        return a > red ? a : red;
    }
    if (is_uni2(kind)) {
        const int DH = (TH + K) / 2 + 1, DW = (TW + K) / 2 + 1, cpt = kind_cpt(kind);
        const size_t a = (size_t)DH * DW * cv * 16 + (size_t)K * K * cv * 8 * 4 + ec + xt;
        const size_t red = (size_t)(BLOCK / (cv * 8 / cpt)) * cv * 8 * 2 * 4;
        return a > red ? a : red;
    }
    if (is_uni(kind)) {
        const int IH = TH + K - 1, IW = TW + K - 1, cpt = kind_cpt(kind);
        const size_t cs = (!xk && centre_stage_on(cpt, R)) ? (size_t)TH * TW * cv * 16 : 0;
        const size_t a = (size_t)IH * IW * cv * 16 + (size_t)K * K * cv * 8 * 4 + ec + xt + cs;
        const size_t red = (size_t)(BLOCK / (cv * 8 / cpt)) * cv * 8 * 2 * 4;   // 2 rows of partials (>= 1 tap)
        return a > red ? a : red;
    }
    if (kind == TK_BWD_F) {
        const int IH = TH + K - 1, IW = TW + K - 1;
        const size_t a = 2 * (size_t)IH * IW * cv * 16 + (size_t)K * K * cv * 8 * 4 + ec;
        const size_t r1 = (size_t)(BLOCK / cv) * cv * 8 * 2 * 4, r2 = (size_t)(BLOCK / (cv * K)) * cv * 8 * K * K * 4;
        const size_t red = r1 > r2 ? r1 : r2;
        return a > red ? a : red;
    }
    const int DH = (TH + K) / 2 + 1, DW = (TW + K) / 2 + 1;
    const size_t a = (size_t)DH * DW * cv * 16 + (size_t)K * K * cv * 8 * 4 + ec;
    const size_t red = (size_t)(BLOCK / cv) * cv * 8 * 2 * 4;
    return a > red ? a : red;
}

// the cheapest tile of a Ho x Wo map for strips of R outputs
TileChoice search_tile(int kind, int R, int Ho, int Wo, int K, int S, int cv, bool pro, bool epi, int xk) {
    const bool uni = is_uni(kind);
    const bool uni2 = is_uni2(kind);
    const int NIN = (R - 1) * S + K;
    const int wstep = kind == TK_BWD_S2 ? 8 : uni2 ? 2 * R : R, hstep = (kind == TK_BWD_S2 || uni2) ? 2 : 1;
    int slots, strip;
    if (kind == TK_FWD) {
        slots = BLOCK / cv;
        strip = K * (8 * NIN + 4 * R * K + 12) + R * (epi ? 60 : 24);
    } else if (kind == TK_BWD_W) {
        slots = BLOCK / (cv * K);
        strip = 8 * R + 8 * NIN + 4 * R * K + 12;
    } else if (uni2) {
        // per strip of R centres: ~K/2 dy rows of (R + K/2 - 1) vectors, R * K/2 taps per row, data + weight products
        const int cpt = kind_cpt(kind), kh = (K + 1) / 2;
        slots = BLOCK / (cv * 8 / cpt);
        strip = kh * ((R + kh - 1) * (cpt + 2) + R * kh * cpt) + R * (epi ? 14 * cpt : 2 * cpt);
    } else if (uni) {
        // one strip: K rows of (R+K-1) dy vectors unpacked once, R*K data + R*K weight packed FMAs per channel pair,
        // plus the centres' prologue (sigmoid) and the epilogue per output
        const int cpt = kind_cpt(kind);
        slots = BLOCK / (cv * 8 / cpt);
        strip = K * (NIN * (cpt + 2) + R * K * cpt) + R * (epi ? 14 * cpt : 2 * cpt);
    } else if (kind == TK_BWD_F) {
        // data strip on BLOCK/cv lanes + weight strip on BLOCK/(cv K) lanes, expressed per data lane
        slots = BLOCK / cv;
        strip = K * (8 * NIN + 4 * R * K + 12) + R * (epi ? 60 : 24) + K * (8 * R + 8 * NIN + 4 * R * K + 12);
    } else {
        slots = BLOCK / cv;
        const int taps = ((K + 1) / 2) * ((K + 1) / 2);
        strip = taps * (4 * 8 + 4 * 4 + 4) + R * (epi ? 60 : 24);
    }
    const int stage = (uni || uni2) ? 110 : kind == TK_BWD_F ? (pro ? 90 : 30) + 110 : (pro ? 90 : 30);
    const size_t budget = kind == TK_BWD_U2 ? (size_t)DWU2_LDS_KB * 1024
                        : (uni || uni2) ? (size_t)DWU_LDS_KB * 1024
                              : kind == TK_BWD_F ? (size_t)DWF_LDS_KB * 1024 : LDS_BUDGET;
    const int wmax = (Wo + wstep - 1) / wstep * wstep;
    const int hmax = (Ho + hstep - 1) / hstep * hstep;
    TileChoice best{hstep, wstep};
    double best_cost = 1e300;
    // x-mode stride-1 backward: also search the band size, in whole rounds of `slots` strips (the y1 buffer holds
    // one band's centres); nr = 0: one band of all strips
    const int nrmax = (xk && uni) ? 6 : 0;
    for (int TW = wstep; TW <= wmax && TW <= 40; TW += wstep) {
        for (int TH = hstep; TH <= hmax && TH <= 40; TH += hstep) {
          bool fits_any = false;
          for (int nr = nrmax; nr >= 0; --nr) {        // smallest buffer first
            const int all = TH * (TW / R);
            const int sbv = nr > 0 ? nr * slots : 0;
            if (nr > 0 && sbv >= all) continue;
            if (tile_lds(kind, K, S, cv, epi, R, TH, TW, xk, sbv) > budget) continue;
            fits_any = true;
            const int nb = sbv > 0 ? cdiv(all, sbv) : 1;
            const int tiles = cdiv(Ho, TH) * cdiv(Wo, TW);
            int strips, staged;
            if (uni2) {
                strips = TH * (TW / R) / 2;
                staged = ((TH + K) / 2 + 1) * ((TW + K) / 2 + 1) * cv;
            } else if (uni) {
                strips = TH * (TW / R);
                staged = (TH + K - 1) * (TW + K - 1) * cv;
            } else if (kind == TK_FWD || kind == TK_BWD_F) {
                strips = TH * (TW / R);
                staged = ((TH - 1) * S + K) * ((TW - 1) * S + K) * cv;
            } else if (kind == TK_BWD_W) {
                strips = TH * (TW / R);
                staged = ((TH - 1) * S + K) * ((TW - 1) * S + K) * cv + TH * TW * cv;
            } else {
                strips = TH * (TW / 8) * 2;
                staged = ((TH + K) / 2 + 1) * ((TW + K) / 2 + 1) * cv;
            }
            // x-mode backward: the y1 centres cost a pack + 8-byte LDS store per 4 channels of a pixel, and each
            // band / parity class one more barrier
            const int xstage = (xk && (uni || uni2)) ? cdiv(TH * TW * cv, BLOCK) * 40 + (uni2 ? 4 : nb) * 100 : 0;
            const double cost = (double)tiles * ((double)cdiv(strips, slots) * strip +
                                                 (double)cdiv(staged, BLOCK) * stage + xstage + 150.0);
            if (cost < best_cost * 0.999) {
                best_cost = cost;
                best = TileChoice{TH, TW, sbv};
            }
          }
          if (!fits_any) break;                          // taller tiles only need more
        }
    }
    return best;
}

int clamp_grid(int64_t tiles, int max_blocks_x) {
    int64_t gx = tiles < max_blocks_x ? tiles : max_blocks_x;
    return (int)(gx < 1 ? 1 : gx);
}

// Total-workgroup target across the channel chunks (grid.y).  Small maps with many channels (10x10 x 1392)
// have one tile per frame: 768 tiles x 22 chunks = 17k one-tile workgroups that each pay the weight load,
// constant staging and partial-row write for a single 14x14 tile.  Capping grid.x at TARGET / chunks makes
// every workgroup loop over several tiles (and shrinks the partial rows).  0 = no cap.
constexpr int DW_WG_TARGET = 3072;   // tools/gpu_ab.sh sweep: 3072-4096 best on the 19x19 / 10x10 layers (-15..-25 %)
constexpr int DW_CAP_MIN_CHUNKS = 8;   // wide layers only: the high-resolution ones (<= 5 chunks) want every workgroup
int chunk_cap(int max_blocks_x, int chunks) {
    if (DW_WG_TARGET <= 0 || chunks < DW_CAP_MIN_CHUNKS) return max_blocks_x;
    const int cap = (DW_WG_TARGET + chunks - 1) / chunks;
    return cap < max_blocks_x ? cap : max_blocks_x;
}

// Everything of a plan but the frame count and the grid (which only scale with N): one frame's plan.  `tiles` =
// tiles per frame.
DwPlan plan_frame(int op, int H, int W, int C, int k, int s, bool pro, bool epi, bool unified, int cin, int& tiles) {
    if (op == OP_BWD_FUSED_S1) s = 1;
    if (op == OP_BWD_FUSED_S2) s = 2;
    const DwGeo g = make_geo(1, H, W, C, k, s);
    DwPlan p{};
    p.N = 1; p.H = H; p.W = W; p.C = C; p.Ho = g.Ho; p.Wo = g.Wo; p.k = k; p.s = s; p.pad = g.pad;
    p.nv = g.nv; p.cv = g.cv; p.chunks = g.chunks;
    p.cpt = 8;
    bool ok = (k == 3 || k == 5) && (s == 1 || s == 2);
    int mh = g.Ho, mw = g.Wo, S = s;      // the tiled map and the stride of the tile search
    switch (op) {
    case OP_FWD_X:
        p.xk = xk_of(cin, C, k, s);
        ok = ok && x_supported(k, s, p.xk);
        [[fallthrough]];
    case OP_FWD:
        p.kind = TK_FWD;
        p.R = s == 1 ? fwd_r(s, g.Wo, p.xk) : 2;
        p.ring = op == OP_FWD && H * W <= DW_RING_PIX;
        break;
    case OP_BWD_DATA:          // grid over the INPUT space (the backward output)
        mh = H; mw = W; pro = false;
        if (s == 1) {          // as a forward over dy (H == Ho) with flipped taps
            p.kind = TK_FWD;
            p.R = fwd_r(1, W, 0);
            p.ring = g.Ho * g.Wo <= DW_RING_PIX;
        } else {
            p.kind = TK_BWD_S2;
            p.R = 4;
            S = 2;
        }
        break;
    case OP_BWD_WEIGHT:
        p.kind = TK_BWD_W;
        p.R = s == 1 ? DW_R1 : 2;
        epi = false;
        break;
    case OP_BWD_FUSED_S1: {    // grid over the H x W map
        mh = H; mw = W;
        const bool uni = use_uni(unified ? 1 : 0, pro, epi);
        p.xk = (cin > 0 && uni) ? xk_of(cin, C, k, 1) : 0;
        p.kind = uni ? uni_kind(k, p.xk, H, W) : TK_BWD_F;
        p.cpt = kind_cpt(p.kind);
        p.R = uni ? uni_r(k, W, p.xk, p.cpt) : DW_R1;
        p.ring = uni && H * W <= DW_RING_PIX;
        // x-mode (y1 recomputed from the block input): unified kernel with the BN1 epilogue only
        if (cin > 0) ok = ok && uni && epi && x_supported(k, 1, p.xk);
        break;
    }
    case OP_BWD_FUSED_S2:      // grid over the INPUT map (the dx / centre space)
        mh = H; mw = W; pro = epi;
        p.xk = cin > 0 ? xk_of(cin, C, k, 2) : 0;
        p.kind = uni2_kind(k);
        p.cpt = kind_cpt(p.kind);
        p.R = uni2_r(k);
        p.ring = g.Ho * g.Wo <= DW_RING_PIX;   // the staged dy map
        if (cin > 0) ok = ok && epi && x_supported(k, 2, p.xk);
        break;
    default:
        ok = false;
        p.kind = TK_FWD;
        p.R = DW_R1;
    }
    const TileChoice tc = search_tile(p.kind, p.R, mh, mw, k, S, g.cv, pro, epi, p.xk);
    p.TH = tc.TH; p.TW = tc.TW; p.sb = tc.sb;
    if (op == OP_BWD_FUSED_S2 && ((tc.TH & 1) || (tc.TW % (2 * p.R)))) ok = false;
    p.lds = (int)tile_lds(p.kind, k, S, g.cv, epi, p.R, tc.TH, tc.TW, p.xk, tc.sb);
    if (is_uni(p.kind) || is_uni2(p.kind)) {
        const size_t per_tap = (size_t)(BLOCK / (g.cv * 8 / p.cpt)) * g.cv * 8 * 4;
        p.red_taps = (int)std::min<size_t>((size_t)k * k, (size_t)p.lds / per_tap);
    }
    tiles = cdiv(mh, tc.TH) * cdiv(mw, tc.TW);
    p.err = ok ? 0 : (int)hipErrorInvalidValue;
    return p;
}

}  // namespace

namespace rt1 {
namespace dw {

DwPlan dw_plan(int op, int N, int H, int W, int C, int k, int s, int pro, int epi, int variant, int cin,
               int max_blocks_x) {
    // per-thread memo keyed on the whole request but N / max_blocks_x: the tile search runs once per key and the
    // launch path stays O(1)
    typedef std::array<int, 10> Key;
    struct Hash {
        size_t operator()(const Key& a) const {
            size_t h = 1469598103934665603ull;
            for (int v : a) h = (h ^ (size_t)(unsigned)v) * 1099511628211ull;
            return h;
        }
    };
    struct Entry { DwPlan p; int tiles; };
    thread_local std::unordered_map<Key, Entry, Hash> memo;
    const Key key{op, H, W, C, k, s, pro != 0, epi != 0, variant != 0, cin};
    auto it = memo.find(key);
    if (it == memo.end()) {
        Entry e;
        e.p = plan_frame(op, H, W, C, k, s, pro != 0, epi != 0, variant != 0, cin, e.tiles);
        it = memo.emplace(key, e).first;
    }
    DwPlan p = it->second.p;
    p.N = N;
    p.grid_x = clamp_grid((int64_t)N * it->second.tiles, chunk_cap(max_blocks_x, p.chunks));
    return p;
}

}  // namespace dw
}  // namespace rt1

namespace {

// the kernels' view of a plan's geometry
inline DwGeo geo_of(const DwPlan& p) {
    return DwGeo{p.N, p.H, p.W, p.C, p.Ho, p.Wo, p.k, p.s, p.pad, p.nv, p.cv, p.chunks};
}

template <int EPI>
int launch_fwd(const DwPlan& p, const bf16_t* x, const float* w, const float* scale, const float* shift, int act,
               int grid_x, bf16_t* out, float* ps, float* pq, BnBwdEpi e, hipStream_t st) {
    if (p.err) return p.err;
    const DwGeo g = geo_of(p);
    dim3 grid(grid_x, p.chunks);
#define L(KK, SS, RR)                                                                                               \
    if (p.k == KK && p.s == SS && p.R == RR) {                                                                      \
        if (p.ring)                                                                                                 \
            hipLaunchKernelGGL((dw_fwd_kernel<KK, SS, RR, EPI, 0, true>), grid, dim3(BLOCK), p.lds, st, x, w,       \
                               scale, shift, act, g, p.TH, p.TW, out, ps, pq, e, XExp{nullptr, nullptr, 0});        \
        else                                                                                                        \
            hipLaunchKernelGGL((dw_fwd_kernel<KK, SS, RR, EPI>), grid, dim3(BLOCK), p.lds, st, x, w, scale, shift,  \
                               act, g, p.TH, p.TW, out, ps, pq, e, XExp{nullptr, nullptr, 0});                      \
        return (int)hipGetLastError();                                                                              \
    }
    L(3, 1, 5) L(3, 1, DW_R1) L(3, 2, 2) L(5, 1, 5) L(5, 1, DW_R1) L(5, 2, 2)
#undef L
    return (int)hipErrorInvalidValue;
}

}  // namespace

extern "C" {

// Grid helpers: the caller sizes the per-workgroup partial buffers from these.  `pro` / `epi` select the cost model
// of the variant that will run.
int rt1_dw_grid(int N, int H, int W, int C, int k, int s, int max_blocks_x, int pro, int epi) {
    return dw_plan(OP_FWD, N, H, W, C, k, s, pro, epi, 0, 0, max_blocks_x).grid_x;
}

int rt1_dw_wgrad_grid(int N, int H, int W, int C, int k, int s, int max_blocks_x, int pro) {
    return dw_plan(OP_BWD_WEIGHT, N, H, W, C, k, s, pro, 0, 0, 0, max_blocks_x).grid_x;
}

int rt1_dw_bwd_grid(int N, int H, int W, int C, int k, int s, int max_blocks_x, int epi) {
    return dw_plan(OP_BWD_DATA, N, H, W, C, k, s, 0, epi, 0, 0, max_blocks_x).grid_x;
}

int rt1_dw_bwd_fused_grid(int N, int H, int W, int C, int k, int max_blocks_x, int pro, int epi, int variant,
                          int cin) {
    return dw_plan(OP_BWD_FUSED_S1, N, H, W, C, k, 1, pro, epi, variant, cin, max_blocks_x).grid_x;
}

int rt1_dw_bwd_fused_s2_grid(int N, int H, int W, int C, int k, int max_blocks_x, int epi, int cin) {
    return dw_plan(OP_BWD_FUSED_S2, N, H, W, C, k, 2, epi, epi, 1, cin, max_blocks_x).grid_x;
}

int rt1_dw_grid_x(int N, int H, int W, int C, int k, int s, int cin, int max_blocks_x) {
    return dw_plan(OP_FWD_X, N, H, W, C, k, s, 1, 0, 0, cin, max_blocks_x).grid_x;
}

int rt1_dw_bwd_uses_uni(int variant, int pro, int epi) { return use_uni(variant, pro != 0, epi != 0) ? 1 : 0; }

int rt1_dw_x_supported(int cin, int C, int k, int s) { return dw_plan(OP_FWD_X, 1, 8, 8, C, k, s, 1, 0, 0, cin, 1).err == 0; }

// Tile picked for a layer (host-side introspection for tools / tests): which = 0 forward, 1 unified backward
// (stride 1 or 2); cin > 0 selects x-mode.  out = {TH, TW, LDS bytes, strips per band (0 = all)}.
int rt1_dw_tile_info(int which, int H, int W, int C, int k, int s, int cin, int* out) {
    const DwPlan p = which == 0 ? dw_plan(cin > 0 ? OP_FWD_X : OP_FWD, 1, H, W, C, k, s, 1, 0, 0, cin, 1)
                                : dw_plan(s == 2 ? OP_BWD_FUSED_S2 : OP_BWD_FUSED_S1, 1, H, W, C, k, s, 1, 1, 1, cin, 1);
    if (cin > 0 && !p.xk) return (int)hipErrorInvalidValue;
    out[0] = p.TH;
    out[1] = p.TW;
    out[2] = p.lds;
    out[3] = p.sb;
    return 0;
}

int rt1_dw_fwd(const bf16_t* x, const float* w, const float* scale, const float* shift, int act, int N, int H, int W,
               int C, int k, int s, int grid_x, bf16_t* out, float* psum, float* psq, hipStream_t st) {
    const DwPlan p = dw_plan(OP_FWD, N, H, W, C, k, s, scale != nullptr, 0, 0, 0, grid_x);
    BnBwdEpi e{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    return psum ? launch_fwd<EPI_STATS>(p, x, w, scale, shift, act, grid_x, out, psum, psq, e, st)
                : launch_fwd<EPI_NONE>(p, x, w, scale, shift, act, grid_x, out, psum, psq, e, st);
}

// wflip: the kernel with taps reversed (host prepares it) -- used for s == 1
int rt1_dw_bwd_data(const bf16_t* dy, const float* w, const float* wflip, int N, int H, int W, int C, int k, int s,
                    int grid_x, bf16_t* dx, const bf16_t* y_in, const float* scale, const float* shift,
                    const float* mean, const float* rstd, float* pdz, float* pdzx, hipStream_t st) {
    const int epi = y_in != nullptr;
    const DwPlan p = dw_plan(OP_BWD_DATA, N, H, W, C, k, s, 0, epi, 0, 0, grid_x);
    BnBwdEpi e{y_in, scale, shift, mean, rstd, 0};
    if (p.kind == TK_FWD)
        return epi ? launch_fwd<EPI_BNBWD>(p, dy, wflip, nullptr, nullptr, 0, grid_x, dx, pdz, pdzx, e, st)
                   : launch_fwd<EPI_NONE>(p, dy, wflip, nullptr, nullptr, 0, grid_x, dx, pdz, pdzx, e, st);
    if (p.err) return p.err;
    const DwGeo g = geo_of(p);
    dim3 grid(grid_x, p.chunks);
#define L(KK, EE)                                                                                                   \
    hipLaunchKernelGGL((dw_bwd_data_s2_kernel<KK, EE>), grid, dim3(BLOCK), p.lds, st, dy, w, g, p.TH, p.TW, dx, pdz, \
                       pdzx, e)
    if (k == 3) { if (epi) L(3, EPI_BNBWD); else L(3, EPI_NONE); }
    else if (k == 5) { if (epi) L(5, EPI_BNBWD); else L(5, EPI_NONE); }
    else return (int)hipErrorInvalidValue;
#undef L
    return (int)hipGetLastError();
}

// ---- x-mode forward: out = dwconv(silu(bn1(x @ we^T))) with the BN2-stat epilogue; y1 is never stored
int rt1_dw_fwd_x(const bf16_t* x, int cin, const bf16_t* we, const float* w, const float* scale1, const float* shift1,
                 int N, int H, int W, int C, int k, int s, int grid_x, bf16_t* out, float* psum, float* psq,
                 hipStream_t st) {
    const DwPlan p = dw_plan(OP_FWD_X, N, H, W, C, k, s, 1, 0, 0, cin, grid_x);
    if (p.err || !scale1 || !shift1 || !psum || !psq) return (int)hipErrorInvalidValue;
    const DwGeo g = geo_of(p);
    const BnBwdEpi e{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    const XExp xe{x, we, cin};
    dim3 grid(grid_x, p.chunks);
#define L(KK, SS, RR, XX)                                                                                           \
    if (p.k == KK && p.s == SS && p.xk == XX && p.R == RR) {                                                        \
        hipLaunchKernelGGL((dw_fwd_kernel<KK, SS, RR, EPI_STATS, XX>), grid, dim3(BLOCK), p.lds, st, nullptr, w,    \
                           scale1, shift1, (int)ACT_SILU, g, p.TH, p.TW, out, psum, psq, e, xe);                    \
        return (int)hipGetLastError();                                                                              \
    }
#define X1(KK, XX) L(KK, 1, DW_R1, XX)
#define X2(KK, XX) L(KK, 2, 2, XX)
    DW_XMODE_S1(X1) DW_XMODE_S2(X2)
#undef X2
#undef X1
#undef L
    return (int)hipErrorInvalidValue;
}

int rt1_dw_bwd_weight(const bf16_t* dy, const bf16_t* x, const float* scale, const float* shift, int act, int N, int H,
                      int W, int C, int k, int s, int grid_x, float* dwp, hipStream_t st) {
    const DwPlan p = dw_plan(OP_BWD_WEIGHT, N, H, W, C, k, s, scale != nullptr, 0, 0, 0, grid_x);
    if (p.err) return p.err;
    const DwGeo g = geo_of(p);
    dim3 grid(grid_x, p.chunks);
#define L(KK, SS, RR)                                                                                               \
    hipLaunchKernelGGL((dw_bwd_weight_kernel<KK, SS, RR>), grid, dim3(BLOCK), p.lds, st, dy, x, scale, shift, act, \
                       g, p.TH, p.TW, dwp)
    if (k == 3 && s == 1) L(3, 1, DW_R1);
    else if (k == 3 && s == 2) L(3, 2, 2);
    else if (k == 5 && s == 1) L(5, 1, DW_R1);
    else if (k == 5 && s == 2) L(5, 2, 2);
    else return (int)hipErrorInvalidValue;
#undef L
    return (int)hipGetLastError();
}

// dA, y2 [N, Ho, Wo, C]; x1 [N, H, W, C]; w unflipped [C, k*k].  BN1 epilogue (and BN1+SiLU operand) when mean1 is set.
int rt1_dw_bwd_fused_s2(const bf16_t* dA, const bf16_t* y2, const float* gate, const float* rb, const float* scale2,
                        const float* shift2, const float* mean2, const float* rstd2, const float* gamma2,
                        const float* mdz2, const float* mdzx2, const float* w, const bf16_t* x1, const float* scale1,
                        const float* shift1, const float* mean1, const float* rstd1, int N, int H, int W, int C, int k,
                        int grid_x, bf16_t* dx, float* pdz, float* pdzx, float* dwp, hipStream_t st, int zout,
                        const bf16_t* xin, const bf16_t* we, int cin) {
    const bool epi = mean1 != nullptr;
    if (epi != (scale1 != nullptr) || (zout && !epi)) return (int)hipErrorInvalidValue;
    // x-mode: y1 recomputed from (xin, we); the plan accepts it with the BN1 epilogue only
    if (xin && (cin <= 0 || !we)) return (int)hipErrorInvalidValue;
    const DwPlan p = dw_plan(OP_BWD_FUSED_S2, N, H, W, C, k, 2, epi, epi, 1, xin ? cin : 0, grid_x);
    if (p.err) return p.err;
    const DwGeo g = geo_of(p);
    DyBnBwd d{dA, y2, gate, rb, scale2, shift2, mean2, rstd2, gamma2, mdz2, mdzx2};
    BnBwdEpi e{epi ? x1 : nullptr, scale1, shift1, mean1, rstd1, zout ? 1 : 0};
    dim3 grid(grid_x, p.chunks);
    const XExp xe{xin, we, cin};
#define LV1(KK, RR, EE, CC, XX, RGV)                                                                                \
    hipLaunchKernelGGL((dw_bwd_uni_s2_kernel<KK, RR, EE, CC, XX, RGV>), grid, dim3(BLOCK), p.lds, st, d, x1, w, g,   \
                       p.TH, p.TW, e, dx, pdz, pdzx, dwp, p.red_taps, xe)
#define LV(KK, RR, EE, CC, XX)                                                                                      \
    if (p.k == KK && p.R == RR && epi == (EE == EPI_BNBWD) && p.cpt == CC && p.xk == XX) {                          \
        if (p.ring) LV1(KK, RR, EE, CC, XX, true); else LV1(KK, RR, EE, CC, XX, false);                             \
        return (int)hipGetLastError();                                                                              \
    }
#define XV(KK, XX) LV(KK, (KK == 3 ? DWV_R3 : DWV_R5), EPI_BNBWD, (KK == 3 ? DWV_CPT3 : DWV_CPT5), XX)
    DW_XMODE_S2(XV)
    LV(3, DWV_R3, EPI_BNBWD, DWV_CPT3, 0) LV(3, DWV_R3, EPI_NONE, DWV_CPT3, 0)
    LV(5, DWV_R5, EPI_BNBWD, DWV_CPT5, 0) LV(5, DWV_R5, EPI_NONE, DWV_CPT5, 0)
#undef XV
#undef LV
#undef LV1
    return (int)hipErrorInvalidValue;
}

// dA, y2: the block's dA (grad of the project-conv input before the gate) and the dw output (pre-BN2);
// gate / rb [N, C] and the BN2 constants rebuild dy; x1 (+ scale1 / shift1 / act1) is the dw input;
// y_in/mean1/rstd1 non-null selects the BN1 epilogue (expand blocks).  dwp: [grid_x][C * k * k] partials.
int rt1_dw_bwd_fused(const bf16_t* dA, const bf16_t* y2, const float* gate, const float* rb, const float* scale2,
                     const float* shift2, const float* mean2, const float* rstd2, const float* gamma2,
                     const float* mdz2, const float* mdzx2, const float* w, const float* wflip, const bf16_t* x1,
                     const float* scale1, const float* shift1, int act1, const float* mean1, const float* rstd1, int N,
                     int H, int W, int C, int k, int grid_x, bf16_t* dx, float* pdz, float* pdzx, float* dwp,
                     hipStream_t st, int variant, int zout, const bf16_t* xin, const bf16_t* we, int cin,
                     const bf16_t* res, const float* rmul) {
    const bool pro = scale1 != nullptr, epi = mean1 != nullptr;
    // x-mode (y1 recomputed from xin, we): the plan accepts it for the unified kernel with the BN1 epilogue only
    if (xin && (cin <= 0 || !we)) return (int)hipErrorInvalidValue;
    const DwPlan p = dw_plan(OP_BWD_FUSED_S1, N, H, W, C, k, 1, pro, epi, variant, xin ? cin : 0, grid_x);
    if (p.err) return p.err;
    const bool uni = is_uni(p.kind);
    // the residual epilogue lives in the unified kernel's plain (no BN1) store
    if (res && (epi || !rmul || !uni)) return (int)hipErrorInvalidValue;
    // dz output (zout) only from the unified kernel's BN1 epilogue
    if (zout && !(epi && uni)) return (int)hipErrorInvalidValue;
    const DwGeo g = geo_of(p);
    DyBnBwd d{dA, y2, gate, rb, scale2, shift2, mean2, rstd2, gamma2, mdz2, mdzx2};
    BnBwdEpi e{epi ? x1 : nullptr, scale1, shift1, mean1, rstd1, zout ? 1 : 0, res, rmul};
    dim3 grid(grid_x, p.chunks);
    if (uni) {   // w: unflipped (the kernel flips while staging it)
        if (epi && act1 != ACT_SILU) return (int)hipErrorInvalidValue;   // the centre prologue is BN + SiLU
        const XExp xe{xin, we, cin};
#define LU1(KK, RR, EE, CC, XX, RGV)                                                                                \
    hipLaunchKernelGGL((dw_bwd_uni_kernel<KK, RR, EE, CC, XX, RGV>), grid, dim3(BLOCK), p.lds, st, d, x1, w, g,      \
                       p.TH, p.TW, e, dx, pdz, pdzx, dwp, p.red_taps, xe, p.sb)
#define LU(KK, RR, EE, CC, XX)                                                                                      \
    if (p.k == KK && p.R == RR && epi == (EE == EPI_BNBWD) && p.cpt == CC && p.xk == XX) {                          \
        if (p.ring) LU1(KK, RR, EE, CC, XX, true); else LU1(KK, RR, EE, CC, XX, false);                             \
        return (int)hipGetLastError();                                                                              \
    }
#define XU(KK, XX) LU(KK, (KK == 3 ? DWU_R3 : DWU_R5), EPI_BNBWD, (KK == 3 ? DWU_CPT3 : DWU_CPT5), XX)
        DW_XMODE_S1(XU)
        LU(3, DWU_R3, EPI_BNBWD, DWU_CPT3, 0) LU(3, DWU_R3, EPI_NONE, DWU_CPT3, 0)
        LU(5, 5, EPI_BNBWD, 2, 0) LU(5, 5, EPI_NONE, 2, 0)
        LU(5, 4, EPI_BNBWD, 2, 0) LU(5, 4, EPI_NONE, 2, 0)
        LU(5, 5, EPI_BNBWD, DWU_CPT5, 0) LU(5, 5, EPI_NONE, DWU_CPT5, 0)
        LU(5, DWU_R5, EPI_BNBWD, DWU_CPT5, 0) LU(5, DWU_R5, EPI_NONE, DWU_CPT5, 0)
#undef XU
#undef LU
#undef LU1
        return (int)hipErrorInvalidValue;
    }
    if (y2 == nullptr) return (int)hipErrorInvalidValue;   // copy staging (dA = dy) is a unified-kernel mode
#define L(KK, EE)                                                                                                   \
    hipLaunchKernelGGL((dw_bwd_fused_kernel<KK, DW_R1, EE>), grid, dim3(BLOCK), p.lds, st, d, x1, scale1, shift1,   \
                       act1, wflip, g, p.TH, p.TW, dx, pdz, pdzx, e, dwp)
    if (k == 3) { if (epi) L(3, EPI_BNBWD); else L(3, EPI_NONE); }
    else if (k == 5) { if (epi) L(5, EPI_BNBWD); else L(5, EPI_NONE); }
    else return (int)hipErrorInvalidValue;
#undef L
    return (int)hipGetLastError();
}

}  // extern "C"
