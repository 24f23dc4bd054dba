// Depthwise conv, unified stride-1 backward: the data and the weight gradient from one pass over the staged dy.  Its
// launcher rt1_dw_bwd_fused also dispatches the two-pass form (dw_fwd.hip launch_bwd_twopass) where the plan picks it.
#include "dw/dw_uni.h"

using namespace rt1;
using namespace rt1::dw;

namespace {

// ------------------------------------------------------------------ unified stride-1 backward
// dw_bwd_fused_kernel (dw_fwd.hip) runs the data and the weight gradient as two passes over its staged tiles: a halo'd copy of
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

#ifndef DW_CENTRE_PREFETCH   // the next strip's centres loaded while this strip computes (CPREF in dw_bwd_uni_kernel)
#define DW_CENTRE_PREFETCH 1
#endif
typedef __attribute__((address_space(3))) void dw_lds_void;   // LDS-DMA destination of the centre stage (dw_common.h)
constexpr int DWU2_SU = 4;   // half-vector dy pixels in flight per thread while staging (2-channel form)

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

}  // namespace

extern "C" {

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
    return launch_bwd_twopass(p, d, x1, scale1, shift1, act1, wflip, grid_x, dx, pdz, pdzx, e, epi, dwp, st);
}

}  // extern "C"
