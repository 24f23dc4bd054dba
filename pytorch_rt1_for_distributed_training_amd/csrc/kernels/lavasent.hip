// LAVA visual sentence as ONE op (gfx950, wave64): the three level projections of SequenceLAVMSE.encode written
// straight into the pixel rows the cross attention reads,
//   pixels[n, off_l + r, :] = drop((A_l[n, r, :] W_l^T + b_l) * sqrt(128) + pos[off_l + r, :]),
// for fuse levels (2, 3, 4), channels (128, 256, 256), d_model = 128.  A_2 = L2 and A_3 = L3 are the encoder's NHWC
// bf16 stage outputs read as [N * hw, C] matrices; A_4, the VALID 2x2 maxpool of L3, is built while staging and never
// stored.  All products run on v_mfma_f32_16x16x32_bf16 with fp32 accumulation; the weights are rounded to bf16 once
// by the caller.
//
// Work split.  A 256-lane workgroup (4 waves) owns TM = 64 consecutive rows of ONE level (a tile may straddle frames,
// never levels) and 128 output columns; wave = (column half, row half), 2 row x 4 column fragments, 32 accumulator
// VGPRs.  The product is computed TRANSPOSED: the weight rows are the MFMA A operand and the activation rows the B
// operand, both plain 16-byte LDS reads of 8 consecutive k, and a lane's accumulator is four consecutive output
// COLUMNS of one row.  The weight rows are laid into LDS in a permuted order so that the lane's two fragments of a
// column pair are 8 consecutive columns: every global store of `pixels` is a 16-byte piece and the four lanes of a
// row write 128 contiguous bytes.  Bias, scale, positions and dropout are register work on those pieces.
//
// K is STREAMED in chunks of 64: weight chunk [128][64] + row chunk [64][64] are 27 KB of LDS (row stride 72 bf16:
// the 16 rows of a fragment start 36 banks apart), against 101 KB for all of K = 256 at once, which would leave one
// workgroup per CU to a kernel that is bound by bytes.  With the chunks LDS allows five; the registers (130-150 VGPRs
// plus 40-44 AGPRs as built) allow two, and that is the occupancy the kernel runs at.  The next chunk's global loads
// are issued into registers before the current chunk's MFMAs and written to LDS after them.  The weights (160 KB in
// all) are re-read per tile from L2.
//
// Data gradient: the SAME kernel template.  The operand is g = mask * dpix rounded to bf16 while staging (so a
// bf16-representable dpix enters exactly); dA_l = g W_l is again the transposed product with W_l^T rows as the A
// operand, 128 output columns at a time (K = 256: two passes over the tile's g, the second from L2); the factor
// sqrt(128) / (1 - p) multiplies the fp32 accumulators.  Launch 1 serves level 2 (dL2, bf16) and level 4 (its product
// into an fp32 workspace [N h4 w4, 256]); launch 2 serves level 3, whose epilogue recomputes the winner of the row's
// pooling window from L3 (strict >, first candidate in row-major order, as F.max_pool2d) and adds the workspace row
// where the row is the winner -- a gather, no atomics.  dL2 / dL3 stores are 16-byte pieces too.
//
// Weight gradient: its own kernel.  One pass feeding both products from one staged (g, A) tile needs the [128][K]
// fp32 partial (128 VGPRs per lane at K = 256) next to the 64 dA accumulators and both staging sets: it fits the
// 512-register file only at one wave per SIMD with nothing left for loads in flight, so the pass is split in two and
// dpix is read twice.  A workgroup walks a fixed contiguous range of one level's row tiles, stages g [64][128] and
// A [64][K] row-major (level 4 pooled again from L3), reads both through the LDS transpose read with K = rows, and
// keeps dW^T in registers over the whole range (wave = a quarter of the k columns, all 128 c).  db is the column sum
// of the same rounded g, kept in four registers per lane by the staging threads.  Each workgroup writes one fp32
// partial [128 K + 128]; a second launch adds them in a fixed order and scales: bitwise reproducible.  The partial
// count per level is min(tiles, 256, operand bytes / (2 x partial bytes)): what is written and read back never
// exceeds what the pass reads (one partial is the floor).
//
// Dropout is transformer.hip's counter hash keyed on (seed, global row n S + r, column); no mask is stored, p = 0
// takes no hash.  Every kernel is built without packed fp32 (common.h NO_PACKED_FP32).
#include "common.h"

using namespace rt1;

namespace {

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bf16x4 lds_v4;

constexpr int BLOCK = 256;
constexpr int TM = 64;                            // rows per tile
constexpr int D = 128;                            // d_model
constexpr int KC = 64;                            // streamed K chunk
constexpr int LDT = KC + 8;                       // LDS row stride of both chunk tiles (bf16)
constexpr int LDG = D + 8;                        // weight-gradient g tile
constexpr int CAP = 256;                          // weight-gradient partials per level: one workgroup per CU
constexpr float kScale = 11.313708498984761f;     // sqrt(128)

enum Mode : int { FWD = 0, DGRAD = 1 };

__device__ __forceinline__ void block_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ bf16x8 tr_read8(const bf16_t* base0, const bf16_t* base1) {
    const bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)base0);
    const bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)base1);
    return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// transformer.hip's dropout hash
__device__ __forceinline__ uint32_t mix32(uint32_t seed, uint32_t a, uint32_t b) {
    uint32_t x = seed ^ (a * 0x9E3779B1u) ^ (b * 0x85EBCA77u) ^ 0x27d4eb2fu;
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ bool dropped(uint32_t seed, uint32_t row, uint32_t col, float p) {
    return (float)(mix32(seed, row, col) >> 8) * (1.0f / 16777216.0f) < p;
}

template <typename T>
__device__ __forceinline__ T sel(int l, T a, T b, T c) { return l == 0 ? a : (l == 1 ? b : c); }

// ---- the 2x2 pool of bf16 pairs: strict >, so a tie keeps the earlier candidate -------------------------------------
__device__ __forceinline__ uint32_t max2(uint32_t a, uint32_t b) {
    const uint32_t lo = __uint_as_float(b << 16) > __uint_as_float(a << 16) ? (b & 0xffffu) : (a & 0xffffu);
    const uint32_t hi = __uint_as_float(b & 0xffff0000u) > __uint_as_float(a & 0xffff0000u) ? (b & 0xffff0000u)
                                                                                              : (a & 0xffff0000u);
    return lo | hi;
}
__device__ __forceinline__ uint4 pool4(const uint4 c0, const uint4 c1, const uint4 c2, const uint4 c3) {
    uint4 o;
    o.x = max2(max2(max2(c0.x, c1.x), c2.x), c3.x);
    o.y = max2(max2(max2(c0.y, c1.y), c2.y), c3.y);
    o.z = max2(max2(max2(c0.z, c1.z), c2.z), c3.z);
    o.w = max2(max2(max2(c0.w, c1.w), c2.w), c3.w);
    return o;
}
// whether candidate `pos` is the one pool4 picked, per channel
__device__ __forceinline__ void winner8(const uint4 c0, const uint4 c1, const uint4 c2, const uint4 c3, int pos,
                                        bool (&win)[8]) {
    float f0[8], f1[8], f2[8], f3[8];
    unpack8(c0, f0); unpack8(c1, f1); unpack8(c2, f2); unpack8(c3, f3);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        float best = f0[q];
        int bi = 0;
        if (f1[q] > best) { best = f1[q]; bi = 1; }
        if (f2[q] > best) { best = f2[q]; bi = 2; }
        if (f3[q] > best) { best = f3[q]; bi = 3; }
        win[q] = bi == pos;
    }
}

// mask * dpix of 8 consecutive columns, rounded to bf16 (RNE)
__device__ __forceinline__ uint4 mask_round8(const uint4 lo, const uint4 hi, uint32_t seed, uint32_t grow, int col,
                                             float p) {
    float f[8] = {__uint_as_float(lo.x), __uint_as_float(lo.y), __uint_as_float(lo.z), __uint_as_float(lo.w),
                  __uint_as_float(hi.x), __uint_as_float(hi.y), __uint_as_float(hi.z), __uint_as_float(hi.w)};
    if (p > 0.f) {
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (dropped(seed, grow, (uint32_t)(col + q), p)) f[q] = 0.f;
    }
    return make_uint4(pack2(f[0], f[1]), pack2(f[2], f[3]), pack2(f[4], f[5]), pack2(f[6], f[7]));
}

// ---- forward and data gradient: one template ----------------------------------------------------------------------

struct SentArgs {
    const bf16_t* L2;         // FWD: [N h2 w2, 128]
    const bf16_t* L3;         // FWD: [N h3 w3, 256] (levels 3, 4); DGRAD: the pool winners of level 3
    const float* dpix;        // DGRAD: [N, S, 128]
    const bf16_t* W0;         // FWD: W_l bf16 [128][K_l]; DGRAD: W_l^T bf16 [K_l][128]
    const bf16_t* W1;
    const bf16_t* W2;
    const float* b0;          // FWD: [128]
    const float* b1;
    const float* b2;
    const float* pos;         // FWD: [S, 128]
    float* pix;               // FWD: [N, S, 128]
    bf16_t* dL2;              // DGRAD
    bf16_t* dL3;
    float* ws;                // DGRAD: level-4 product fp32 [N h4 w4, 256], written by level 4, read by level 3
    int M0, M1, M2;           // rows per level, N * hw_l
    int hw0, hw1, hw2;        // rows per frame and level
    int off1, off2;           // first sentence row of levels 3 and 4 (level 2 starts at 0)
    int T0, T1, T2;           // tiles of this launch per level (0: the level is not served by this launch)
    int S, h3, w3, h4, w4;
    float p;
    uint32_t seed;
};

// LDS row of weight row c (0..127): fragment (pair jp, half ab) holds rows lh * 8 + ab * 4 + e of the pair's 32, so
// the two fragments of a pair give a lane 8 consecutive output columns
__device__ __forceinline__ int wrow(int c) {
    return (c & 64) + ((((c >> 5) & 1) * 2 + ((c >> 2) & 1)) * 16) + ((c >> 3) & 3) * 4 + (c & 3);
}

template <int MODE>
__global__ NO_PACKED_FP32 __launch_bounds__(BLOCK) void lava_sent_kernel(SentArgs a) {
    __shared__ __attribute__((aligned(16))) bf16_t Wl[D * LDT];
    __shared__ __attribute__((aligned(16))) bf16_t Al[TM * LDT];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 15, lh = lane >> 4;
    const int ch = wave & 1, rh = wave >> 1;
    int lvl = 0, tile = blockIdx.x;
    if (tile >= a.T0) {
        tile -= a.T0;
        lvl = 1;
        if (tile >= a.T1) {
            tile -= a.T1;
            lvl = 2;
        }
    }
    const int K = lvl == 0 ? 128 : 256;
    const int M = sel(lvl, a.M0, a.M1, a.M2), hw = sel(lvl, a.hw0, a.hw1, a.hw2), off = sel(lvl, 0, a.off1, a.off2);
    const bf16_t* __restrict__ W = sel(lvl, a.W0, a.W1, a.W2);
    const int m0 = tile * TM;
    const int RED = MODE == FWD ? K : D;           // reduced dimension, streamed in chunks of 64
    const int nkc = RED / KC, steps = (MODE == FWD ? 1 : K / D) * nkc;
    const bool pool = MODE == FWD && lvl == 2;
    const float ik = a.p > 0.f ? 1.0f / (1.0f - a.p) : 1.0f;

    // the thread's two 16-byte items of a row chunk: row, its 8 k, where the row starts in memory
    int64_t abase[2];
    uint32_t agrow[2];
    bool aval[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int item = t + i * BLOCK, row = item >> 3, m = m0 + row;
        aval[i] = m < M;
        const int mm = aval[i] ? m : 0, n = mm / hw, r = mm - n * hw;
        agrow[i] = (uint32_t)(n * a.S + off + r);
        if constexpr (MODE == DGRAD) {
            abase[i] = (int64_t)agrow[i] * D;
        } else if (pool) {
            const int y4 = r / a.w4, x4 = r - y4 * a.w4;
            abase[i] = (((int64_t)n * a.h3 + 2 * y4) * a.w3 + 2 * x4) * 256;
        } else {
            abase[i] = (int64_t)mm * K;
        }
    }
    const bf16_t* __restrict__ act = lvl == 0 ? a.L2 : a.L3;

    constexpr int AR = MODE == FWD ? 4 : 2;        // 16-byte loads in flight per item: pool candidates / 8 floats
    u32x4 wr[4];                                   // native vectors: an array of the uint4 struct stays in memory here
    uint4 ar[2][AR];
    auto issue = [&](int s) __attribute__((always_inline)) {
        const int ob = s / nkc, kc = s - ob * nkc;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int item = t + i * BLOCK, row = item >> 3, v = item & 7;
            wr[i] = *reinterpret_cast<const u32x4*>(W + (int64_t)(ob * D + row) * RED + kc * KC + v * 8);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int v = (t + i * BLOCK) & 7;
            const int64_t o = abase[i] + kc * KC + v * 8;
#pragma unroll
            for (int c = 0; c < AR; ++c) ar[i][c] = make_uint4(0, 0, 0, 0);
            if (!aval[i]) continue;
            if constexpr (MODE == DGRAD) {
                ar[i][0] = *reinterpret_cast<const uint4*>(a.dpix + o);
                ar[i][1] = *reinterpret_cast<const uint4*>(a.dpix + o + 4);
            } else if (!pool) {
                ar[i][0] = *reinterpret_cast<const uint4*>(act + o);
            } else {
                ar[i][0] = *reinterpret_cast<const uint4*>(act + o);
                ar[i][1] = *reinterpret_cast<const uint4*>(act + o + 256);
                ar[i][2] = *reinterpret_cast<const uint4*>(act + o + (int64_t)a.w3 * 256);
                ar[i][3] = *reinterpret_cast<const uint4*>(act + o + (int64_t)a.w3 * 256 + 256);
            }
        }
    };
    auto commit = [&](int kc) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int item = t + i * BLOCK, row = item >> 3, v = item & 7;
            *reinterpret_cast<u32x4*>(Wl + wrow(row) * LDT + v * 8) = wr[i];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int item = t + i * BLOCK, row = item >> 3, v = item & 7;
            uint4 val = ar[i][0];
            if constexpr (MODE == DGRAD) val = mask_round8(ar[i][0], ar[i][1], a.seed, agrow[i], kc * KC + v * 8, a.p);
            if constexpr (MODE == FWD)
                if (pool) val = pool4(ar[i][0], ar[i][1], ar[i][2], ar[i][3]);
            *reinterpret_cast<uint4*>(Al + row * LDT + v * 8) = val;
        }
    };

    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    issue(0);
    for (int s = 0; s < steps; ++s) {
        const int ob = s / nkc, kc = s - ob * nkc;
        block_sync();                              // the previous chunk's fragment reads are done
        commit(kc);
        block_sync();
        if (s + 1 < steps) issue(s + 1);           // in flight during this chunk's MFMAs
#pragma unroll
        for (int kk = 0; kk < KC / 32; ++kk) {
            bf16x8 fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
                fb[i] = *reinterpret_cast<const bf16x8*>(Al + (rh * 32 + i * 16 + lr) * LDT + kk * 32 + lh * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bf16x8 fa =
                    *reinterpret_cast<const bf16x8*>(Wl + (ch * 64 + j * 16 + lr) * LDT + kk * 32 + lh * 8);
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb[i], acc[i][j], 0, 0, 0);
            }
        }
        if (kc != nkc - 1) continue;

        // epilogue of output block ob: the lane holds row rh * 32 + i * 16 + lr, columns ch * 64 + jp * 32 + lh * 8 + 0..7
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = m0 + rh * 32 + i * 16 + lr;
            if (m < M) {
                const int n = m / hw, r = m - n * hw;
#pragma unroll
                for (int jp = 0; jp < 2; ++jp) {
                    const int col = ch * 64 + jp * 32 + lh * 8;
                    const f32x4 v0 = acc[i][jp * 2], v1 = acc[i][jp * 2 + 1];
                    float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                    if constexpr (MODE == FWD) {
                        const int srow = off + r;
                        const uint32_t grow = (uint32_t)(n * a.S + srow);
                        const float* __restrict__ bias = sel(lvl, a.b0, a.b1, a.b2);
                        float bv[8], pv[8];
                        load8f(bias + col, bv);
                        load8f(a.pos + (int64_t)srow * D + col, pv);
#pragma unroll
                        for (int q = 0; q < 8; ++q) {
                            v[q] = (v[q] + bv[q]) * kScale + pv[q];
                            if (a.p > 0.f) v[q] = dropped(a.seed, grow, (uint32_t)(col + q), a.p) ? 0.f : v[q] * ik;
                        }
                        float* dst = a.pix + (int64_t)grow * D + col;
                        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
                        *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
                    } else {
                        const int k = ob * D + col;
                        const float sc = kScale * ik;
#pragma unroll
                        for (int q = 0; q < 8; ++q) v[q] *= sc;
                        if (lvl == 2) {
                            float* dst = a.ws + (int64_t)m * 256 + k;
                            *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
                            *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
                        } else if (lvl == 0) {
                            store8(a.dL2 + (int64_t)m * D + k, v);
                        } else {
                            const int y = r / a.w3, x = r - y * a.w3;
                            if (y < 2 * a.h4 && x < 2 * a.w4) {    // the row is inside a pooling window
                                const bf16_t* c = a.L3 + (((int64_t)n * a.h3 + (y & ~1)) * a.w3 + (x & ~1)) * 256 + k;
                                const uint4 c0 = *reinterpret_cast<const uint4*>(c);
                                const uint4 c1 = *reinterpret_cast<const uint4*>(c + 256);
                                const uint4 c2 = *reinterpret_cast<const uint4*>(c + (int64_t)a.w3 * 256);
                                const uint4 c3 = *reinterpret_cast<const uint4*>(c + (int64_t)a.w3 * 256 + 256);
                                bool win[8];
                                winner8(c0, c1, c2, c3, (y & 1) * 2 + (x & 1), win);
                                float g4[8];
                                load8f(a.ws + (((int64_t)n * a.h4 + (y >> 1)) * a.w4 + (x >> 1)) * 256 + k, g4);
#pragma unroll
                                for (int q = 0; q < 8; ++q) v[q] += win[q] ? g4[q] : 0.f;
                            }
                            store8(a.dL3 + (int64_t)m * 256 + k, v);
                        }
                    }
                    // one piece's loads at a time: clustering all four pieces' loads ahead costs more registers
                    // than the kernel has
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------

struct WgradArgs {
    const float* dpix;        // [N, S, 128]
    const bf16_t* L2;
    const bf16_t* L3;
    float* part0;             // [P_l][128 K_l + 128]: dW_l [128][K_l], then db_l
    float* part1;
    float* part2;
    int P0, P1, P2;
    int M0, M1, M2;
    int hw0, hw1, hw2;
    int off1, off2;
    int S, h3, w3, h4, w4;
    float p;
    uint32_t seed;
};

template <int K, bool POOL>
__device__ __forceinline__ void wgrad_body(const WgradArgs& a, const bf16_t* __restrict__ act, float* __restrict__ part,
                                           int M, int hw, int off, int pidx, int P, bf16_t* Gl, bf16_t* Al) {
    constexpr int LDA = K + 8, KTW = K / 64, AV = K / 8, AI = TM * AV / BLOCK;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 15, lh = lane >> 4;
    const int q4 = lr >> 2, p4 = lr & 3;
    const int tiles = (M + TM - 1) / TM;
    const int t0 = (int)((int64_t)pidx * tiles / P), t1 = (int)((int64_t)(pidx + 1) * tiles / P);
    const int grow0 = t >> 5, cg = (t & 31) * 4;  // g staging: 4 columns of every 8th row

    f32x4 acc[KTW][8];
#pragma unroll
    for (int i = 0; i < KTW; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dbacc[4] = {0.f, 0.f, 0.f, 0.f};

    for (int tile = t0; tile < t1; ++tile) {
        const int m0 = tile * TM;
        block_sync();                              // the previous tile's fragment reads are done
#pragma unroll
        for (int i = 0; i < TM / 8; ++i) {
            const int row = grow0 + 8 * i, m = m0 + row;
            uint2 val = make_uint2(0, 0);
            if (m < M) {
                const int n = m / hw, r = m - n * hw;
                const uint32_t grow = (uint32_t)(n * a.S + off + r);
                float4 g = *reinterpret_cast<const float4*>(a.dpix + (int64_t)grow * D + cg);
                if (a.p > 0.f) {
                    if (dropped(a.seed, grow, (uint32_t)cg, a.p)) g.x = 0.f;
                    if (dropped(a.seed, grow, (uint32_t)(cg + 1), a.p)) g.y = 0.f;
                    if (dropped(a.seed, grow, (uint32_t)(cg + 2), a.p)) g.z = 0.f;
                    if (dropped(a.seed, grow, (uint32_t)(cg + 3), a.p)) g.w = 0.f;
                }
                val = make_uint2(pack2(g.x, g.y), pack2(g.z, g.w));
                dbacc[0] += __uint_as_float(val.x << 16);
                dbacc[1] += __uint_as_float(val.x & 0xffff0000u);
                dbacc[2] += __uint_as_float(val.y << 16);
                dbacc[3] += __uint_as_float(val.y & 0xffff0000u);
            }
            *reinterpret_cast<uint2*>(Gl + row * LDG + cg) = val;
        }
#pragma unroll
        for (int i = 0; i < AI; ++i) {
            const int item = t + i * BLOCK, row = item / AV, v = item - row * AV, m = m0 + row;
            uint4 val = make_uint4(0, 0, 0, 0);
            if (m < M) {
                if constexpr (POOL) {
                    const int n = m / hw, r = m - n * hw, y4 = r / a.w4, x4 = r - y4 * a.w4;
                    const bf16_t* c = act + (((int64_t)n * a.h3 + 2 * y4) * a.w3 + 2 * x4) * 256 + v * 8;
                    val = pool4(*reinterpret_cast<const uint4*>(c), *reinterpret_cast<const uint4*>(c + 256),
                                *reinterpret_cast<const uint4*>(c + (int64_t)a.w3 * 256),
                                *reinterpret_cast<const uint4*>(c + (int64_t)a.w3 * 256 + 256));
                } else {
                    val = *reinterpret_cast<const uint4*>(act + (int64_t)m * K + v * 8);
                }
            }
            *reinterpret_cast<uint4*>(Al + row * LDA + v * 8) = val;
        }
        block_sync();
#pragma unroll
        for (int s = 0; s < TM / 32; ++s) {
            const int ra = s * 32 + lh * 8 + q4;   // the lane's two transpose-read rows are ra and ra + 4
            bf16x8 fd[8];
#pragma unroll
            for (int ct = 0; ct < 8; ++ct) {
                const bf16_t* gp = Gl + ra * LDG + ct * 16 + p4 * 4;
                fd[ct] = tr_read8(gp, gp + 4 * LDG);
            }
#pragma unroll
            for (int kt = 0; kt < KTW; ++kt) {
                const bf16_t* ap = Al + ra * LDA + (wave * KTW + kt) * 16 + p4 * 4;
                const bf16x8 fa = tr_read8(ap, ap + 4 * LDA);
#pragma unroll
                for (int ct = 0; ct < 8; ++ct)
                    acc[kt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fd[ct], acc[kt][ct], 0, 0, 0);
            }
        }
    }

    // lane holds dW[c = ct * 16 + lr][k = (wave * KTW + kt) * 16 + lh * 4 + 0..3]
    float* pp = part + (int64_t)pidx * (D * K + D);
#pragma unroll
    for (int kt = 0; kt < KTW; ++kt)
#pragma unroll
        for (int ct = 0; ct < 8; ++ct) {
            const f32x4 v = acc[kt][ct];
            *reinterpret_cast<float4*>(pp + (ct * 16 + lr) * K + (wave * KTW + kt) * 16 + lh * 4) =
                make_float4(v[0], v[1], v[2], v[3]);
        }
    block_sync();                                  // the g tile becomes the 8 row groups' column sums
    float* red = reinterpret_cast<float*>(Gl);
#pragma unroll
    for (int q = 0; q < 4; ++q) red[grow0 * D + cg + q] = dbacc[q];
    block_sync();
    if (t < D) {
        float sum = 0.f;
#pragma unroll
        for (int g = 0; g < 8; ++g) sum += red[g * D + t];
        pp[D * K + t] = sum;
    }
}

__global__ NO_PACKED_FP32 __launch_bounds__(BLOCK) void lava_sent_wgrad_kernel(WgradArgs a) {
    __shared__ __attribute__((aligned(16))) bf16_t Gl[TM * LDG];
    __shared__ __attribute__((aligned(16))) bf16_t Al[TM * (256 + 8)];
    int pidx = blockIdx.x;
    if (pidx < a.P0) {
        wgrad_body<128, false>(a, a.L2, a.part0, a.M0, a.hw0, 0, pidx, a.P0, Gl, Al);
    } else if (pidx < a.P0 + a.P1) {
        wgrad_body<256, false>(a, a.L3, a.part1, a.M1, a.hw1, a.off1, pidx - a.P0, a.P1, Gl, Al);
    } else {
        wgrad_body<256, true>(a, a.L3, a.part2, a.M2, a.hw2, a.off2, pidx - a.P0 - a.P1, a.P2, Gl, Al);
    }
}

struct ReduceArgs {
    const float* part0;
    const float* part1;
    const float* part2;
    float* dW0;
    float* dW1;
    float* dW2;
    float* db0;
    float* db1;
    float* db2;
    int P0, P1, P2;
    float scale;
};

// partials in a fixed order (four interleaved chains, combined as a fixed tree), scaled -> dW_l [128][K_l], db_l [128]
__global__ NO_PACKED_FP32 __launch_bounds__(BLOCK) void lava_sent_wgrad_reduce_kernel(ReduceArgs a) {
    const int lvl = blockIdx.y, K = lvl == 0 ? 128 : 256, E = D * K + D;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= E) return;
    const float* src = sel(lvl, a.part0, a.part1, a.part2) + i;
    const int P = sel(lvl, a.P0, a.P1, a.P2);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int p = 0;
    for (; p + 3 < P; p += 4) {
        s0 += src[(int64_t)p * E];
        s1 += src[(int64_t)(p + 1) * E];
        s2 += src[(int64_t)(p + 2) * E];
        s3 += src[(int64_t)(p + 3) * E];
    }
    for (; p < P; ++p) s0 += src[(int64_t)p * E];
    const float v = ((s0 + s1) + (s2 + s3)) * a.scale;
    if (i < D * K) sel(lvl, a.dW0, a.dW1, a.dW2)[i] = v;
    else sel(lvl, a.db0, a.db1, a.db2)[i - D * K] = v;
}

struct Geo {
    int M[3], hw[3], T[3], P[3];
    int off1, off2, S, h4, w4;
};

// false when a shape cannot be served (or an index would overflow 32 bits)
bool geometry(int64_t N, int64_t h2, int64_t w2, int64_t h3, int64_t w3, Geo& g) {
    constexpr int64_t LIM = (int64_t)1 << 20;
    if (N < 1 || h2 < 1 || w2 < 1 || h3 < 2 || w3 < 2 || h2 > LIM || w2 > LIM || h3 > LIM || w3 > LIM) return false;
    const int64_t h4 = h3 / 2, w4 = w3 / 2;
    const int64_t hw[3] = {h2 * w2, h3 * w3, h4 * w4};
    const int64_t S = hw[0] + hw[1] + hw[2];
    if (N * S > INT32_MAX - TM) return false;      // every global row n S + r and every tile's last row fit an int
    const int Kl[3] = {128, 256, 256};
    for (int l = 0; l < 3; ++l) {
        g.hw[l] = (int)hw[l];
        g.M[l] = (int)(N * hw[l]);
        g.T[l] = (g.M[l] + TM - 1) / TM;
        // what the pass reads of this level against one partial written and read back
        const int64_t bytes = (int64_t)g.M[l] * (D * 4 + Kl[l] * 2), per = 2 * (int64_t)(D * Kl[l] + D) * 4;
        int64_t P = bytes / per;
        if (P > CAP) P = CAP;
        if (P > g.T[l]) P = g.T[l];
        g.P[l] = (int)(P < 1 ? 1 : P);
    }
    g.off1 = (int)hw[0];
    g.off2 = (int)(hw[0] + hw[1]);
    g.S = (int)S;
    g.h4 = (int)h4;
    g.w4 = (int)w4;
    return true;
}

}  // namespace

extern "C" int rt1_lava_sentence_supported(int c2, int c3, int d) { return c2 == 128 && c3 == 256 && d == D ? 1 : 0; }

extern "C" int rt1_lava_sentence_tile_rows() { return TM; }

// P[3]: workgroup partials of the weight gradient per level (2, 3, 4); returns 0 for an unserved shape
extern "C" int rt1_lava_sentence_wgrad_partials(int64_t N, int64_t h2, int64_t w2, int64_t h3, int64_t w3,
                                                int64_t* P) {
    Geo g;
    if (P == nullptr || !geometry(N, h2, w2, h3, w3, g)) return 0;
    for (int l = 0; l < 3; ++l) P[l] = g.P[l];
    return 1;
}

extern "C" int rt1_lava_sentence_fwd(const uint16_t* L2, const uint16_t* L3, const uint16_t* wp2, const uint16_t* wp3,
                                     const uint16_t* wp4, const float* b2, const float* b3, const float* b4,
                                     const float* pos, int64_t N, int64_t h2, int64_t w2, int64_t h3, int64_t w3,
                                     float p, uint32_t seed, float* pix, hipStream_t stream) {
    Geo g;
    if (L2 == nullptr || L3 == nullptr || wp2 == nullptr || wp3 == nullptr || wp4 == nullptr || b2 == nullptr ||
        b3 == nullptr || b4 == nullptr || pos == nullptr || pix == nullptr || !geometry(N, h2, w2, h3, w3, g) ||
        !(p >= 0.f && p < 1.f))
        return (int)hipErrorInvalidValue;
    SentArgs a{L2, L3, nullptr, wp2, wp3, wp4, b2, b3, b4, pos, pix, nullptr, nullptr, nullptr,
               g.M[0], g.M[1], g.M[2], g.hw[0], g.hw[1], g.hw[2], g.off1, g.off2, g.T[0], g.T[1], g.T[2],
               g.S, (int)h3, (int)w3, g.h4, g.w4, p, seed};
    hipLaunchKernelGGL(lava_sent_kernel<FWD>, dim3(g.T[0] + g.T[1] + g.T[2]), dim3(BLOCK), 0, stream, a);
    return (int)hipGetLastError();
}

// wt_l: W_l^T bf16 [K_l][128]; ws: fp32 [N h4 w4, 256]
extern "C" int rt1_lava_sentence_dgrad(const float* dpix, const uint16_t* L3, const uint16_t* wt2, const uint16_t* wt3,
                                       const uint16_t* wt4, int64_t N, int64_t h2, int64_t w2, int64_t h3, int64_t w3,
                                       float p, uint32_t seed, float* ws, uint16_t* dL2, uint16_t* dL3,
                                       hipStream_t stream) {
    Geo g;
    if (dpix == nullptr || L3 == nullptr || wt2 == nullptr || wt3 == nullptr || wt4 == nullptr || ws == nullptr ||
        dL2 == nullptr || dL3 == nullptr || !geometry(N, h2, w2, h3, w3, g) || !(p >= 0.f && p < 1.f))
        return (int)hipErrorInvalidValue;
    SentArgs a{nullptr, L3, dpix, wt2, wt3, wt4, nullptr, nullptr, nullptr, nullptr, nullptr, dL2, dL3, ws,
               g.M[0], g.M[1], g.M[2], g.hw[0], g.hw[1], g.hw[2], g.off1, g.off2, g.T[0], 0, g.T[2],
               g.S, (int)h3, (int)w3, g.h4, g.w4, p, seed};
    hipLaunchKernelGGL(lava_sent_kernel<DGRAD>, dim3(g.T[0] + g.T[2]), dim3(BLOCK), 0, stream, a);   // levels 2, 4
    a.T0 = 0;
    a.T1 = g.T[1];
    a.T2 = 0;
    hipLaunchKernelGGL(lava_sent_kernel<DGRAD>, dim3(g.T[1]), dim3(BLOCK), 0, stream, a);            // level 3
    return (int)hipGetLastError();
}

// part: fp32 workspace of sum_l P_l (128 K_l + 128) floats
extern "C" int rt1_lava_sentence_wgrad(const float* dpix, const uint16_t* L2, const uint16_t* L3, int64_t N,
                                       int64_t h2, int64_t w2, int64_t h3, int64_t w3, float p, uint32_t seed,
                                       float* part, float* dW2, float* dW3, float* dW4, float* db2, float* db3,
                                       float* db4, hipStream_t stream) {
    Geo g;
    if (dpix == nullptr || L2 == nullptr || L3 == nullptr || part == nullptr || dW2 == nullptr || dW3 == nullptr ||
        dW4 == nullptr || db2 == nullptr || db3 == nullptr || db4 == nullptr || !geometry(N, h2, w2, h3, w3, g) ||
        !(p >= 0.f && p < 1.f))
        return (int)hipErrorInvalidValue;
    float* part1 = part + (int64_t)g.P[0] * (D * 128 + D);
    float* part2 = part1 + (int64_t)g.P[1] * (D * 256 + D);
    WgradArgs a{dpix, L2, L3, part, part1, part2, g.P[0], g.P[1], g.P[2], g.M[0], g.M[1], g.M[2],
                g.hw[0], g.hw[1], g.hw[2], g.off1, g.off2, g.S, (int)h3, (int)w3, g.h4, g.w4, p, seed};
    hipLaunchKernelGGL(lava_sent_wgrad_kernel, dim3(g.P[0] + g.P[1] + g.P[2]), dim3(BLOCK), 0, stream, a);
    ReduceArgs r{part, part1, part2, dW2, dW3, dW4, db2, db3, db4, g.P[0], g.P[1], g.P[2],
                 kScale / (1.0f - p)};
    hipLaunchKernelGGL(lava_sent_wgrad_reduce_kernel, dim3((D * 256 + D + BLOCK - 1) / BLOCK, 3), dim3(BLOCK), 0,
                       stream, r);
    return (int)hipGetLastError();
}
