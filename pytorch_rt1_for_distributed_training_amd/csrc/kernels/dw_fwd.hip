// Depthwise conv, the kernels that stage an input tile with stage_tile (the tiling scheme is described in
// dw/dw_common.h): the forward kernel, which is also the stride-1 data gradient and the x-mode forward, the stride-2
// data gradient, the weight gradient, and the two-pass fused stride-1 backward, which runs the data and the weight
// part over the same staged tiles.  Every launcher reads its tile, LDS bytes and strip shape from dw_plan (dw_plan.hip).
#include "dw/dw_stage.h"

using namespace rt1;
using namespace rt1::dw;

namespace {

// Stage an [IH x IW] pixel window (origin ih0, iw0; zero outside [0,Hs) x [0,Ws)) of cv channel vectors
// into LDS, with the BN+activation prologue applied when scale != nullptr.  Each thread owns ONE channel
// vector (per-channel constants in registers) and keeps SU 16-byte loads in flight before it writes
// any of them: the window is ~10 loads per thread, and issuing them one at a time exposed the full
// HBM latency per load.
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
constexpr int DWF_SU = 4;     // pixels (2 x 16-B loads each) in flight per thread while staging dy

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

// the two-pass form of rt1_dw_bwd_fused (dw_bwd_s1.hip), which has validated the request and built d and e
int rt1::dw::launch_bwd_twopass(const DwPlan& p, const DyBnBwd& d, const bf16_t* x1, const float* scale1,
                                const float* shift1, int act1, const float* wflip, int grid_x, bf16_t* dx, float* pdz,
                                float* pdzx, const BnBwdEpi& e, bool epi, float* dwp, hipStream_t st) {
    const DwGeo g = geo_of(p);
    const int k = p.k;
    dim3 grid(grid_x, p.chunks);
#define L(KK, EE)                                                                                                   \
    hipLaunchKernelGGL((dw_bwd_fused_kernel<KK, DW_R1, EE>), grid, dim3(BLOCK), p.lds, st, d, x1, scale1, shift1,   \
                       act1, wflip, g, p.TH, p.TW, dx, pdz, pdzx, e, dwp)
    if (k == 3) { if (epi) L(3, EPI_BNBWD); else L(3, EPI_NONE); }
    else if (k == 5) { if (epi) L(5, EPI_BNBWD); else L(5, EPI_NONE); }
    else return (int)hipErrorInvalidValue;
#undef L
    return (int)hipGetLastError();
}

extern "C" {

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

}  // extern "C"
