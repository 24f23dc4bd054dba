// Depthwise conv, whole stride-2 backward in one launch: the unified kernel over the four parity classes of the
// input pixels, with its launcher rt1_dw_bwd_fused_s2.
#include "dw/dw_uni.h"

using namespace rt1;
using namespace rt1::dw;

namespace {

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

}  // namespace

extern "C" {

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

}  // extern "C"
