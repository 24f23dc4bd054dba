// Depthwise conv, host only: the launch plan of dw/dw_plan.h (geometry, kernel family, strip shape, tile search, LDS
// bytes, grid) and the exported functions that only read it.  No kernel and no device helper is compiled here.
#include <algorithm>
#include <array>
#include <unordered_map>

#include "dw/dw_common.h"

using namespace rt1;
using namespace rt1::dw;

namespace {

constexpr int DW_RING_PIX = 2000;    // maps up to this many pixels stage only the in-image rectangle (WinRect, dw_stage.h)
constexpr int DW_FULLROW_MAX = 18;   // channel vectors up to which a workgroup owns the whole pixel row (make_geo)

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
// The k5 unified backward (y1 in HBM, not x-mode) with 2 channels per thread -- 50 weight-gradient
// accumulators instead of 100, so DWU2_OCC workgroups / CU fit (tiles within DWU2_LDS_KB of LDS) --
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

constexpr size_t LDS_BUDGET = DW_LDS_KB * 1024;

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

}  // extern "C"
