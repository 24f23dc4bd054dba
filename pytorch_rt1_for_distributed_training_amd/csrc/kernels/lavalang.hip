// LAVA cross-layer LANGUAGE path (gfx950, wave64): everything a CrossLayer does on its [N, 128] language rows around
// the folded attention of lavaxattn.hip, d_model = dff = 128, 2 heads, fp32 in and out.
//
//   x3  = lang + drop1(ctx Wo^T + bo)            h = LN_ffn(x3)            f1 = relu(h W1^T + b1)
//   out = x3 + drop2(f1 W2^T + b2)               ln_out = LN_epi(out)      (optional: the next layer's ln_lang, or the
//                                                                           model's fuse_norm after the last layer)
//
// The kernels:
//   tail forward    one launch, saves x3 and f1 (relu' is f1 > 0); LayerNorm statistics are recomputed in the backward
//                   (a 128-float row in registers: cheaper than another saved tensor and its launch-side allocation)
//   tail backward   one launch: LN_epi backward folded into dout, dW2 / db2 / df1, dW1 / db1 / dh, LN_ffn backward,
//                   dWo / dbo, dctx, dlang and the four LayerNorm parameter gradients
//   attention parameter gradients   the sums over frames of lavaxattn.hip's per-frame outputs (d in_proj weight / bias,
//                   d ln_pix weight / bias), which that unit leaves to its caller
//   row LayerNorm forward / backward   layer 0's ln_lang, the only LayerNorm that is not some tail's epilogue
//   reduce          workgroup partials added in partial order; skipped when there is one partial
//
// Work split.  Rows are independent apart from the parameter sums and N is small (16 .. 256 frames), so the unit is
// bound by latency, not by bytes or FLOPs: one 256-lane workgroup owns a 16-row tile and runs the whole chain on it
// without a trip to memory in between.  The row tile lives in LDS as [16][132] fp32 (the stride keeps the 16 rows of
// a 16-byte read on distinct banks).  The [16, 128] x [128, 128] products run on v_mfma_f32_16x16x4_f32: fp32
// operands, so the path keeps the fp32-level error the model tests hold it to.  Wave w owns output columns
// 32 w .. 32 w + 31 (two 16 x 16 accumulators).  The order of the reduced index inside a matrix instruction is free as
// long as both operands agree, so lane group g = lane / 16 takes k = 16 t + 4 g + c for step (t, c): the lane's four
// A values of a t are ONE 16-byte LDS read of the row tile, and for W^T products so are its four B values.
//
// The weight is streamed through LDS in slabs of the reduced index: two of 64 in the forward ([128][68], 34 KB, X W^T)
// and four of 32 in the backward ([32][132], 17 KB, X W), whose five row tiles would not leave a 64 KB workgroup room
// for more.  A thread's 16-byte loads of the next slab -- the next product's first slab included -- are issued before
// the current slab's matrix instructions and written to LDS after them.
//
// LayerNorm, bias, dropout and the residuals are row work between the products: 16 lanes (one DPP row) per row, 8
// columns per lane, the fixed butterfly of lavaxattn.hip for the two row reductions.
//
// Parameter gradients are A^T B over the tile's 16 rows: four K-steps per 16 x 16 output tile, wave w owning output
// rows 32 w .. 32 w + 31 and all 128 columns (16 accumulators per weight, 48 for the three weights of a kernel, kept
// in registers over the tiles a workgroup walks).  Output column 64 half + 4 r + c belongs to accumulator (half, c) of
// lane r, so the B operand of eight tiles is two 16-byte reads and a partial is stored in 16-byte pieces.  The column
// sums (bias and LayerNorm parameter gradients) are 16-term sums in row order by the thread that owns the column.
// Each workgroup writes one partial [3][128][128] + [8][128]; the reduce adds them in partial order: no atomics, a
// result is a function of the inputs alone, bitwise.  The partial count is min(tiles, 256 CUs, 8 MiB / partial bytes)
// = at most 41: what the reduce reads back stays a few microseconds of HBM time however many frames there are.
// The attention parameter gradients use the same A^T B routine on other operands.
//
// Dropout is lavasent.hip's counter hash keyed on (seed, 2 row + site, column), site 0 after the out projection and
// site 1 after the FFN; no mask is stored, p = 0 takes no hash.  Every kernel is built without packed fp32 (common.h
// NO_PACKED_FP32): such a kernel inlines only always_inline callees, so the bodies call __forceinline__ functions and
// builtins only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kD = 128;
constexpr int kThreads = 256;
constexpr int kRows = 16;                         // rows of a tile
constexpr int kLdx = kD + 4;                      // LDS row stride of a row tile
constexpr int kTile = kRows * kLdx;
constexpr int kSlabFwd = 64;                      // reduced indices per weight slab: forward (X W^T, [128][SLAB + 4])
constexpr int kSlabBwd = 32;                      // backward (X W, [SLAB][132]): its five row tiles leave LDS for 32
constexpr int kLdNN = kD + 4;
constexpr int kMat = kD * kD;
constexpr int kVecs = 8;
constexpr int kE = 3 * kMat + kVecs * kD;         // floats of one partial
constexpr int kCus = 256;
constexpr int64_t kPartBytes = (int64_t)8 << 20;  // what the partials of one launch may occupy
constexpr int kCap = (int)(kPartBytes / (kE * 4)) < kCus ? (int)(kPartBytes / (kE * 4)) : kCus;
constexpr float kInvD = 1.f / kD;

template <int CTRL>
__device__ __forceinline__ float dpp(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}

__device__ __forceinline__ void block_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// sum over the 16 lanes of a DPP row in a fixed order; every lane ends with the same bits (lavaxattn.hip)
__device__ __forceinline__ float row_sum16(float x) {
    x += dpp<0xB1>(x);
    x += dpp<0x4E>(x);
    x += dpp<0x141>(x);
    x += dpp<0x140>(x);
    return x;
}

// lane l of a row's 16 holds columns 4l .. 4l+3 and 64+4l .. 64+4l+3
__device__ __forceinline__ int col_of(int l, int i) { return (i < 4 ? 0 : 60) + 4 * l + i; }

__device__ __forceinline__ void load_vec(const float* p, int l, float (&o)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p + 4 * l);
    const f32x4 b = *reinterpret_cast<const f32x4*>(p + 64 + 4 * l);
    o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = a[3]; o[4] = b[0]; o[5] = b[1]; o[6] = b[2]; o[7] = b[3];
}

__device__ __forceinline__ void store_vec(float* p, int l, const float (&v)[8]) {
    *reinterpret_cast<f32x4*>(p + 4 * l) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p + 64 + 4 * l) = f32x4{v[4], v[5], v[6], v[7]};
}

__device__ __forceinline__ void zero8(float (&v)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = 0.f;
}

__device__ __forceinline__ float dot8(const float (&a)[8], const float (&b)[8]) {
    float s = a[0] * b[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) s = fmaf(a[i], b[i], s);
    return s;
}

__device__ __forceinline__ float sum8(const float (&x)[8]) {
    return ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]));
}

// LayerNorm of one row without the affine, in place; returns rstd
__device__ __forceinline__ float normalise(float (&x)[8], float eps) {
    const float mean = row_sum16(sum8(x)) * kInvD;
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] -= mean;
    const float rstd = rsqrtf(fmaf(row_sum16(dot8(x, x)), kInvD, eps));
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] *= rstd;
    return rstd;
}

// dx += the LayerNorm's input gradient from dy (w.r.t. its output), its weight g, the normalised row and rstd
__device__ __forceinline__ void ln_backward_add(const float (&dy)[8], const float (&g)[8], const float (&xh)[8],
                                                float rstd, float (&dx)[8]) {
    float d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = dy[i] * g[i];
    const float m1 = row_sum16(sum8(d)) * kInvD, m2 = row_sum16(dot8(d, xh)) * kInvD;
#pragma unroll
    for (int i = 0; i < 8; ++i) dx[i] = fmaf(rstd, d[i] - m1 - xh[i] * m2, dx[i]);
}

// lavasent.hip's dropout hash
__device__ __forceinline__ uint32_t mix32(uint32_t seed, uint32_t a, uint32_t b) {
    uint32_t x = seed ^ (a * 0x9E3779B1u) ^ (b * 0x85EBCA77u) ^ 0x27d4eb2fu;
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ bool dropped(uint32_t seed, uint32_t key, uint32_t col, float p) {
    return (float)(mix32(seed, key, col) >> 8) * (1.0f / 16777216.0f) < p;
}
// v * mask / (1 - p) at (row, site) for the lane's 8 columns
__device__ __forceinline__ void drop8(float (&v)[8], uint32_t seed, int row, int site, int l, float p) {
    if (p > 0.f) {
        const float ik = 1.0f / (1.0f - p);
#pragma unroll
        for (int i = 0; i < 8; ++i)
            v[i] = dropped(seed, 2u * (uint32_t)row + (uint32_t)site, (uint32_t)col_of(l, i), p) ? 0.f : v[i] * ik;
    }
}

// ---- weight slabs ----------------------------------------------------------------------------------------------------
// NT: Y = X W^T, slab s = columns 64 s .. of every W row.  NN: Y = X W, slab s = rows 64 s .. of W.

template <bool NT, int SLAB>
__device__ __forceinline__ void slab_issue(const float* __restrict__ W, int s, int t, f32x4 (&pre)[SLAB / 8]) {
    constexpr int V = SLAB / 4;                    // 16-byte items per NT slab row
#pragma unroll
    for (int i = 0; i < SLAB / 8; ++i) {
        const int item = t + i * kThreads;
        const int off = NT ? (item / V) * kD + SLAB * s + 4 * (item % V) : (SLAB * s + (item >> 5)) * kD + 4 * (item & 31);
        pre[i] = *reinterpret_cast<const f32x4*>(W + off);
    }
}

template <bool NT, int SLAB>
__device__ __forceinline__ void slab_commit(float* Wl, int t, const f32x4 (&pre)[SLAB / 8]) {
    constexpr int V = SLAB / 4;
#pragma unroll
    for (int i = 0; i < SLAB / 8; ++i) {
        const int item = t + i * kThreads;
        const int off = NT ? (item / V) * (SLAB + 4) + 4 * (item % V) : (item >> 5) * kLdNN + 4 * (item & 31);
        *reinterpret_cast<f32x4*>(Wl + off) = pre[i];
    }
}

// acc[jt] += X[:, slab s] (slab): output columns 32 wave + 16 jt + r; the lane holds rows 4 g .. 4 g + 3 of them
template <bool NT, int SLAB>
__device__ __forceinline__ void slab_mma(const float* Xs, const float* Wl, int s, int t, f32x4 (&acc)[2]) {
    const int lane = t & 63, r = lane & 15, g = lane >> 4, nb = 32 * (t >> 6);
#pragma unroll
    for (int tt = 0; tt < SLAB / 16; ++tt) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(Xs + r * kLdx + SLAB * s + 16 * tt + 4 * g);
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) {
            if constexpr (NT) {
                const f32x4 b = *reinterpret_cast<const f32x4*>(Wl + (nb + 16 * jt + r) * (SLAB + 4) + 16 * tt + 4 * g);
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], b[c], acc[jt], 0, 0, 0);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float b = Wl[(16 * tt + 4 * g + c) * kLdNN + nb + 16 * jt + r];
                    acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], b, acc[jt], 0, 0, 0);
                }
            }
        }
    }
}

// One product.  `pre` holds slab 0 of W on entry and slab 0 of Wnext (when there is one) on exit.  The first barrier
// also publishes the row tile the caller has just written.
template <bool NT, int SLAB>
__device__ __forceinline__ void product(const float* __restrict__ W, const float* __restrict__ Wnext, const float* Xs,
                                        float* Wl, int t, f32x4 (&pre)[SLAB / 8], f32x4 (&acc)[2]) {
    acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < kD / SLAB; ++s) {
        block_sync();                              // the previous slab's reads are done
        slab_commit<NT, SLAB>(Wl, t, pre);
        block_sync();
        if (s + 1 < kD / SLAB) slab_issue<NT, SLAB>(W, s + 1, t, pre);
        else if (Wnext != nullptr) slab_issue<NT, SLAB>(Wnext, 0, t, pre);
        slab_mma<NT, SLAB>(Xs, Wl, s, t, acc);
    }
}

// the accumulators of a product into a row tile
__device__ __forceinline__ void acc_store(float* T, int t, const f32x4 (&acc)[2]) {
    const int lane = t & 63, r = lane & 15, g = lane >> 4, nb = 32 * (t >> 6);
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int q = 0; q < 4; ++q) T[(4 * g + q) * kLdx + nb + 16 * jt + r] = acc[jt][q];
}

// ---- A^T B over the 16 rows of two tiles -----------------------------------------------------------------------------
// acc[rt][4 half + c][q] is dW[32 wave + 16 rt + 4 g + q][64 half + 4 r + c]
__device__ __forceinline__ void atb(const float* TA, const float* TB, int t, f32x4 (&acc)[2][8]) {
    const int lane = t & 63, r = lane & 15, g = lane >> 4, mb = 32 * (t >> 6);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int ro = (4 * s + g) * kLdx;
        const float a[2] = {TA[ro + mb + r], TA[ro + mb + 16 + r]};
        const f32x4 b[2] = {*reinterpret_cast<const f32x4*>(TB + ro + 4 * r),
                            *reinterpret_cast<const f32x4*>(TB + ro + 64 + 4 * r)};
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    acc[rt][4 * h + c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt], b[h][c], acc[rt][4 * h + c], 0, 0, 0);
    }
}

__device__ __forceinline__ void atb_zero(f32x4 (&acc)[2][8]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

__device__ __forceinline__ void atb_store(float* __restrict__ dst, int t, const f32x4 (&acc)[2][8]) {
    const int lane = t & 63, r = lane & 15, g = lane >> 4, mb = 32 * (t >> 6);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<f32x4*>(dst + (mb + 16 * rt + 4 * g + q) * kD + 64 * h + 4 * r) =
                    f32x4{acc[rt][4 * h][q], acc[rt][4 * h + 1][q], acc[rt][4 * h + 2][q], acc[rt][4 * h + 3][q]};
}

// column k of a tile summed over its 16 rows in row order
__device__ __forceinline__ float col_sum(const float* T, int k) {
    float s = T[k];
#pragma unroll
    for (int i = 1; i < kRows; ++i) s += T[i * kLdx + k];
    return s;
}

// the tiles [t0, t1) of partial p of P
__device__ __forceinline__ void tile_range(int N, int p, int P, int& t0, int& t1) {
    const int tiles = (N + kRows - 1) / kRows;
    t0 = (int)((int64_t)p * tiles / P);
    t1 = (int)((int64_t)(p + 1) * tiles / P);
}

// ---- row LayerNorm (layer 0's ln_lang) -------------------------------------------------------------------------------

__global__ NO_PACKED_FP32 __launch_bounds__(kThreads) void lava_lang_ln_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b, float eps, int N,
    float* __restrict__ y) {
    const int t = threadIdx.x, l = t & 15, row = blockIdx.x * kRows + (t >> 4);
    float v[8], gv[8], bv[8];
    zero8(v);
    if (row < N) load_vec(x + (int64_t)row * kD, l, v);
    load_vec(g, l, gv);
    load_vec(b, l, bv);
    normalise(v, eps);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = fmaf(v[i], gv[i], bv[i]);
    if (row < N) store_vec(y + (int64_t)row * kD, l, v);
}

// dx, and the partial [2][128] = (d weight, d bias) of this workgroup's tiles
__global__ NO_PACKED_FP32 __launch_bounds__(kThreads) void lava_lang_ln_bwd_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ g, float eps, int N, int P,
    float* __restrict__ dx, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float T[2][kTile];
    const int t = threadIdx.x, l = t & 15, rl = t >> 4;
    int t0, t1;
    tile_range(N, blockIdx.x, P, t0, t1);
    float gv[8];
    load_vec(g, l, gv);
    float vs = 0.f;
    for (int tile = t0; tile < t1; ++tile) {
        const int row = tile * kRows + rl;
        float xv[8], dv[8], o[8], pr[8];
        zero8(xv); zero8(dv); zero8(o);
        if (row < N) {
            load_vec(x + (int64_t)row * kD, l, xv);
            load_vec(dy + (int64_t)row * kD, l, dv);
        }
        const float rstd = normalise(xv, eps);
        ln_backward_add(dv, gv, xv, rstd, o);
        if (row < N) store_vec(dx + (int64_t)row * kD, l, o);
#pragma unroll
        for (int i = 0; i < 8; ++i) pr[i] = dv[i] * xv[i];
        store_vec(T[0] + rl * kLdx, l, pr);
        store_vec(T[1] + rl * kLdx, l, dv);
        block_sync();
        vs += col_sum(T[t >> 7], t & 127);
        block_sync();
    }
    part[(int64_t)blockIdx.x * (2 * kD) + t] = vs;
}

// ---- tail forward ----------------------------------------------------------------------------------------------------

struct TailFwd {
    const float* lang;   // [N, 128]
    const float* ctx;    // [N, 128]
    const float* Wo; const float* bo;
    const float* gf; const float* bf;       // LN_ffn
    const float* W1; const float* b1;
    const float* W2; const float* b2;
    const float* ge; const float* be;       // the epilogue LayerNorm (EPI)
    float* x3; float* f1; float* out; float* ln_out;
    float epsf, epse, p;
    uint32_t seed;
    int N;
};

template <bool EPI>
__global__ NO_PACKED_FP32 __launch_bounds__(kThreads) void lava_lang_tail_fwd_kernel(TailFwd a) {
    __shared__ __attribute__((aligned(16))) float Wl[kD * (kSlabFwd + 4)];
    __shared__ __attribute__((aligned(16))) float Xa[kTile];
    __shared__ __attribute__((aligned(16))) float Xb[kTile];
    const int t = threadIdx.x, l = t & 15, rl = t >> 4, m0 = blockIdx.x * kRows, row = m0 + rl;
    const int lane = t & 63, r = lane & 15, g = lane >> 4, nb = 32 * (t >> 6);
    const bool valid = row < a.N;
    f32x4 pre[kSlabFwd / 8], acc[2];
    slab_issue<true, kSlabFwd>(a.Wo, 0, t, pre);
    float x3v[8], v[8], w[8];
    zero8(x3v); zero8(v);
    if (valid) {
        load_vec(a.lang + (int64_t)row * kD, l, x3v);
        load_vec(a.ctx + (int64_t)row * kD, l, v);
    }
    store_vec(Xa + rl * kLdx, l, v);
    product<true, kSlabFwd>(a.Wo, a.W1, Xa, Wl, t, pre, acc);
    acc_store(Xb, t, acc);
    block_sync();
    // x3 = lang + drop1(y + bo); h = LN_ffn(x3) -> Xa
    load_vec(Xb + rl * kLdx, l, v);
    load_vec(a.bo, l, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] += w[i];
    drop8(v, a.seed, row, 0, l, a.p);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        x3v[i] += v[i];
        v[i] = x3v[i];
    }
    if (valid) store_vec(a.x3 + (int64_t)row * kD, l, x3v);
    normalise(v, a.epsf);
    {
        float gv[8];
        load_vec(a.gf, l, gv);
        load_vec(a.bf, l, w);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = fmaf(v[i], gv[i], w[i]);
    }
    store_vec(Xa + rl * kLdx, l, v);
    product<true, kSlabFwd>(a.W1, a.W2, Xa, Wl, t, pre, acc);
    // f1 = relu(. + b1), straight from the accumulators -> Xb and memory
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) {
        const int col = nb + 16 * jt + r;
        const float bias = a.b1[col];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = 4 * g + q;
            const float f = fmaxf(acc[jt][q] + bias, 0.f);
            Xb[i * kLdx + col] = f;
            if (m0 + i < a.N) a.f1[(int64_t)(m0 + i) * kD + col] = f;
        }
    }
    product<true, kSlabFwd>(a.W2, nullptr, Xb, Wl, t, pre, acc);
    acc_store(Xa, t, acc);
    block_sync();
    // out = x3 + drop2(y + b2)
    load_vec(Xa + rl * kLdx, l, v);
    load_vec(a.b2, l, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] += w[i];
    drop8(v, a.seed, row, 1, l, a.p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] += x3v[i];
    if (valid) store_vec(a.out + (int64_t)row * kD, l, v);
    if constexpr (EPI) {
        float gv[8];
        normalise(v, a.epse);
        load_vec(a.ge, l, gv);
        load_vec(a.be, l, w);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = fmaf(v[i], gv[i], w[i]);
        if (valid) store_vec(a.ln_out + (int64_t)row * kD, l, v);
    }
}

// ---- tail backward ---------------------------------------------------------------------------------------------------

struct TailBwd {
    const float* dout;   // [N, 128]
    const float* dln;    // [N, 128], d ln_out (EPI)
    const float* x3; const float* f1; const float* out; const float* ctx;
    const float* Wo; const float* gf; const float* bf;
    const float* W1; const float* W2; const float* ge;
    float* dlang; float* dctx;
    float* part;         // [P][kE]: dWo, dW1, dW2, then dbo, db1, db2, d gf, d bf, d ge, d be, 0
    float epsf, epse, p;
    uint32_t seed;
    int N, P;
};

template <bool EPI>
__global__ NO_PACKED_FP32 __launch_bounds__(kThreads) void lava_lang_tail_bwd_kernel(TailBwd a) {
    __shared__ __attribute__((aligned(16))) float Wl[kSlabBwd * kLdNN];
    __shared__ __attribute__((aligned(16))) float T[5][kTile];
    const int t = threadIdx.x, l = t & 15, rl = t >> 4, k = t & 127;
    const int lane = t & 63, r = lane & 15, g = lane >> 4, nb = 32 * (t >> 6);
    const bool lo = t < kD;                        // the threads that own a column of the column sums
    int t0, t1;
    tile_range(a.N, blockIdx.x, a.P, t0, t1);
    f32x4 accW[3][2][8];
    atb_zero(accW[0]); atb_zero(accW[1]); atb_zero(accW[2]);
    float vs[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float gfv[8];
    load_vec(a.gf, l, gfv);
    for (int tile = t0; tile < t1; ++tile) {
        const int m0 = tile * kRows, row = m0 + rl;
        const bool valid = row < a.N;
        f32x4 pre[kSlabBwd / 8], acc[2];
        slab_issue<false, kSlabBwd>(a.W2, 0, t, pre);
        // dO = dout + LN_epi backward (d ln_out -> T2, times the normalised out -> T4); dy2 = drop2-masked dO -> T0;
        // f1 -> T1; h = LN_ffn(x3) -> T3
        float dO[8], xh[8], v[8], w[8];
        zero8(dO); zero8(xh); zero8(v);
        if (valid) {
            load_vec(a.dout + (int64_t)row * kD, l, dO);
            load_vec(a.x3 + (int64_t)row * kD, l, xh);
            load_vec(a.f1 + (int64_t)row * kD, l, v);
        }
        store_vec(T[1] + rl * kLdx, l, v);
        if constexpr (EPI) {
            float o[8], dl[8], gev[8];
            zero8(o); zero8(dl);
            if (valid) {
                load_vec(a.out + (int64_t)row * kD, l, o);
                load_vec(a.dln + (int64_t)row * kD, l, dl);
            }
            load_vec(a.ge, l, gev);
            const float rstd = normalise(o, a.epse);
            ln_backward_add(dl, gev, o, rstd, dO);
            store_vec(T[2] + rl * kLdx, l, dl);
#pragma unroll
            for (int i = 0; i < 8; ++i) dl[i] *= o[i];
            store_vec(T[4] + rl * kLdx, l, dl);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = dO[i];
        drop8(v, a.seed, row, 1, l, a.p);
        store_vec(T[0] + rl * kLdx, l, v);
        const float rstd3 = normalise(xh, a.epsf);
        load_vec(a.bf, l, w);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = fmaf(xh[i], gfv[i], w[i]);
        store_vec(T[3] + rl * kLdx, l, v);
        block_sync();
        if (lo) {
            if constexpr (EPI) {
                vs[5] += col_sum(T[4], k);
                vs[6] += col_sum(T[2], k);
            }
            vs[2] += col_sum(T[0], k);
        }
        atb(T[0], T[1], t, accW[2]);               // dW2 += dy2^T f1
        product<false, kSlabBwd>(a.W2, a.W1, T[0], Wl, t, pre, acc);
        // d(h W1^T + b1) = relu' * df1 -> T2
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = (4 * g + q) * kLdx + nb + 16 * jt + r;
                T[2][o] = T[1][o] > 0.f ? acc[jt][q] : 0.f;
            }
        block_sync();
        if (lo) vs[1] += col_sum(T[2], k);
        atb(T[2], T[3], t, accW[1]);               // dW1 += that^T h
        product<false, kSlabBwd>(a.W1, a.Wo, T[2], Wl, t, pre, acc);
        acc_store(T[0], t, acc);                   // dh
        block_sync();
        // LN_ffn backward: dx3 = dO + ...; dlang = dx3; dy1 = drop1-masked dx3 -> T1; ctx -> T3
        load_vec(T[0] + rl * kLdx, l, v);
        ln_backward_add(v, gfv, xh, rstd3, dO);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] *= xh[i];
        store_vec(T[4] + rl * kLdx, l, v);
        if (valid) store_vec(a.dlang + (int64_t)row * kD, l, dO);
        drop8(dO, a.seed, row, 0, l, a.p);
        store_vec(T[1] + rl * kLdx, l, dO);
        zero8(v);
        if (valid) load_vec(a.ctx + (int64_t)row * kD, l, v);
        store_vec(T[3] + rl * kLdx, l, v);
        block_sync();
        if (lo) {
            vs[3] += col_sum(T[4], k);
            vs[4] += col_sum(T[0], k);
            vs[0] += col_sum(T[1], k);
        }
        atb(T[1], T[3], t, accW[0]);               // dWo += dy1^T ctx
        product<false, kSlabBwd>(a.Wo, nullptr, T[1], Wl, t, pre, acc);
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = m0 + 4 * g + q;
                if (i < a.N) a.dctx[(int64_t)i * kD + nb + 16 * jt + r] = acc[jt][q];
            }
        block_sync();                              // the next tile rewrites the row tiles
    }
    float* pp = a.part + (int64_t)blockIdx.x * kE;
#pragma unroll
    for (int m = 0; m < 3; ++m) atb_store(pp + m * kMat, t, accW[m]);
    if (lo) {
#pragma unroll
        for (int i = 0; i < 7; ++i) pp[3 * kMat + i * kD + k] = vs[i];
        pp[3 * kMat + 7 * kD + k] = 0.f;
    }
}

// ---- attention parameter gradients -----------------------------------------------------------------------------------

struct AttnPg {
    const float* Q; const float* dQ; const float* q; const float* dctx;      // [N, 128]
    const float* u; const float* w; const float* z; const float* e;          // [N, 2, 128]
    const float* g; const float* b;                                          // ln_pix
    float* part;         // [P][kE]: d in_proj_weight [384][128], d in_proj_bias [384], d ln weight, d ln bias, 0, 0, 0
    int N, P;
};

__global__ NO_PACKED_FP32 __launch_bounds__(kThreads) void lava_lang_attn_pgrad_kernel(AttnPg a) {
    // 0 dQ, 1 q, 2 scale Q, 3 dctx, 4 + h: g e_h; once dQ^T q is taken, h: g z_h + b replaces tiles 0 and 1
    __shared__ __attribute__((aligned(16))) float T[6][kTile];
    // hh: the head of the thread's column work, and of its wave's output rows 32 wave .. (waves 2 h, 2 h + 1)
    const int t = threadIdx.x, l = t & 15, rl = t >> 4, k = t & 127, hh = t >> 7;
    int t0, t1;
    tile_range(a.N, blockIdx.x, a.P, t0, t1);
    f32x4 accW[3][2][8];
    atb_zero(accW[0]); atb_zero(accW[1]); atb_zero(accW[2]);
    float lnw = 0.f, lnb = 0.f, bsum = 0.f;
    const float gk = a.g[k], bk = a.b[k];
    for (int tile = t0; tile < t1; ++tile) {
        const int m0 = tile * kRows, row = m0 + rl;
        float v[4][8];
#pragma unroll
        for (int j = 0; j < 4; ++j) zero8(v[j]);
        if (row < a.N) {
            load_vec(a.dQ + (int64_t)row * kD, l, v[0]);
            load_vec(a.q + (int64_t)row * kD, l, v[1]);
            load_vec(a.Q + (int64_t)row * kD, l, v[2]);
            load_vec(a.dctx + (int64_t)row * kD, l, v[3]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) v[2][i] *= 0.125f;             // 1 / sqrt(64), exact
#pragma unroll
        for (int j = 0; j < 4; ++j) store_vec(T[j] + rl * kLdx, l, v[j]);
        float xvr[kRows];
#pragma unroll
        for (int i = 0; i < kRows; ++i) {
            float du = 0.f, xv = 0.f;
            if (m0 + i < a.N) {
                const int64_t o = ((int64_t)(m0 + i) * 2 + hh) * kD + k;
                const float wv = a.w[o], zv = a.z[o], uv = a.u[o], ev = a.e[o];
                lnw += fmaf(wv, zv, uv * ev);
                lnb += wv;
                du = gk * ev;
                xv = fmaf(gk, zv, bk);
            }
            T[4 + hh][i * kLdx + k] = du;
            xvr[i] = xv;
        }
        block_sync();
        bsum += col_sum(T[hh == 0 ? 0 : 3], k);
        atb(T[0], T[1], t, accW[0]);               // d W_q += dQ^T q
        atb(T[2], T[4 + hh], t, accW[1]);          // d W_k,h += scale Q_h^T (g e_h)
        block_sync();
#pragma unroll
        for (int i = 0; i < kRows; ++i) T[hh][i * kLdx + k] = xvr[i];
        block_sync();
        atb(T[3], T[hh], t, accW[2]);              // d W_v,h += dctx_h^T (g z_h + b)
        block_sync();
    }
    float* pp = a.part + (int64_t)blockIdx.x * kE;
#pragma unroll
    for (int m = 0; m < 3; ++m) atb_store(pp + m * kMat, t, accW[m]);
    float* s = T[0];                               // the two heads' LayerNorm sums, added head 0 first
    s[t] = lnw;
    s[kThreads + t] = lnb;
    block_sync();
    float* pv = pp + 3 * kMat;
    pv[(hh == 0 ? 0 : 2) * kD + k] = bsum;         // d b_q, d b_v
    if (hh == 0) {
        pv[kD + k] = 0.f;                          // the K bias shifts every score of a head alike
        pv[3 * kD + k] = s[k] + s[kD + k];
        pv[4 * kD + k] = s[kThreads + k] + s[kThreads + kD + k];
    } else {
        pv[5 * kD + k] = 0.f;
        pv[6 * kD + k] = 0.f;
        pv[7 * kD + k] = 0.f;
    }
}

// ---- reduce: out[i] = sum_p part[p][i], four interleaved chains combined as a fixed tree ------------------------------

__global__ NO_PACKED_FP32 __launch_bounds__(kThreads) void lava_lang_reduce_kernel(const float* __restrict__ part, int P,
                                                                                   int E, float* __restrict__ out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= E) return;
    const float* src = part + i;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int p = 0;
    for (; p + 3 < P; p += 4) {
        s0 += src[(int64_t)p * E];
        s1 += src[(int64_t)(p + 1) * E];
        s2 += src[(int64_t)(p + 2) * E];
        s3 += src[(int64_t)(p + 3) * E];
    }
    for (; p < P; ++p) s0 += src[(int64_t)p * E];
    out[i] = (s0 + s1) + (s2 + s3);
}

bool bad_rows(int64_t N) { return N < 1 || N > INT32_MAX - kRows; }

int partials(int64_t N) {
    const int64_t tiles = (N + kRows - 1) / kRows;
    return (int)(tiles < kCap ? tiles : kCap);
}

// one partial is written straight into `out`
void reduce(const float* part, int P, int E, float* out, hipStream_t stream) {
    if (P > 1)
        hipLaunchKernelGGL(lava_lang_reduce_kernel, dim3((E + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, part,
                           P, E, out);
}

}  // namespace

extern "C" int rt1_lava_lang_supported(int d, int dff, int H) { return d == kD && dff == kD && H == 2; }

extern "C" int rt1_lava_lang_tile_rows() { return kRows; }

extern "C" int rt1_lava_lang_partials(int64_t N) { return bad_rows(N) ? 0 : partials(N); }

extern "C" int rt1_lava_lang_grad_floats() { return kE; }

extern "C" int rt1_lava_lang_ln_fwd(const float* x, const float* g, const float* b, float eps, int64_t N, float* y,
                                    hipStream_t stream) {
    if (x == nullptr || g == nullptr || b == nullptr || y == nullptr || bad_rows(N)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(lava_lang_ln_fwd_kernel, dim3((unsigned)((N + kRows - 1) / kRows)), dim3(kThreads), 0, stream, x,
                       g, b, eps, (int)N, y);
    return (int)hipGetLastError();
}

// part: [P][256] (unused when P == 1); dgb: [256] = d weight, d bias
extern "C" int rt1_lava_lang_ln_bwd(const float* dy, const float* x, const float* g, float eps, int64_t N, float* part,
                                    float* dx, float* dgb, hipStream_t stream) {
    if (dy == nullptr || x == nullptr || g == nullptr || part == nullptr || dx == nullptr || dgb == nullptr ||
        bad_rows(N))
        return (int)hipErrorInvalidValue;
    const int P = partials(N);
    hipLaunchKernelGGL(lava_lang_ln_bwd_kernel, dim3(P), dim3(kThreads), 0, stream, dy, x, g, eps, (int)N, P, dx,
                       P > 1 ? part : dgb);
    reduce(part, P, 2 * kD, dgb, stream);
    return (int)hipGetLastError();
}

// ge == nullptr: no epilogue LayerNorm (be, ln_out unused)
extern "C" int rt1_lava_lang_tail_fwd(const float* lang, const float* ctx, const float* Wo, const float* bo,
                                      const float* gf, const float* bf, float epsf, const float* W1, const float* b1,
                                      const float* W2, const float* b2, const float* ge, const float* be, float epse,
                                      float p, uint32_t seed, int64_t N, float* x3, float* f1, float* out,
                                      float* ln_out, hipStream_t stream) {
    if (lang == nullptr || ctx == nullptr || Wo == nullptr || bo == nullptr || gf == nullptr || bf == nullptr ||
        W1 == nullptr || b1 == nullptr || W2 == nullptr || b2 == nullptr || x3 == nullptr || f1 == nullptr ||
        out == nullptr || (ge != nullptr && (be == nullptr || ln_out == nullptr)) || bad_rows(N) ||
        !(p >= 0.f && p < 1.f))
        return (int)hipErrorInvalidValue;
    TailFwd a{lang, ctx, Wo, bo, gf, bf, W1, b1, W2, b2, ge, be, x3, f1, out, ln_out, epsf, epse, p, seed, (int)N};
    const dim3 grid((unsigned)((N + kRows - 1) / kRows));
    if (ge != nullptr) hipLaunchKernelGGL(lava_lang_tail_fwd_kernel<true>, grid, dim3(kThreads), 0, stream, a);
    else hipLaunchKernelGGL(lava_lang_tail_fwd_kernel<false>, grid, dim3(kThreads), 0, stream, a);
    return (int)hipGetLastError();
}

// dln == nullptr: no epilogue LayerNorm (out, ge unused).  part: [P][kE] (unused when P == 1); grads: [kE] = dWo, dW1,
// dW2 [128][128], then dbo, db1, db2, d gf, d bf, d ge, d be, 0 [128]
extern "C" int rt1_lava_lang_tail_bwd(const float* dout, const float* dln, const float* x3, const float* f1,
                                      const float* out, const float* ctx, const float* Wo, const float* gf,
                                      const float* bf, float epsf, const float* W1, const float* W2, const float* ge,
                                      float epse, float p, uint32_t seed, int64_t N, float* part, float* dlang,
                                      float* dctx, float* grads, hipStream_t stream) {
    if (dout == nullptr || x3 == nullptr || f1 == nullptr || ctx == nullptr || Wo == nullptr || gf == nullptr ||
        bf == nullptr || W1 == nullptr || W2 == nullptr || part == nullptr || dlang == nullptr || dctx == nullptr ||
        grads == nullptr || (dln != nullptr && (out == nullptr || ge == nullptr)) || bad_rows(N) ||
        !(p >= 0.f && p < 1.f))
        return (int)hipErrorInvalidValue;
    const int P = partials(N);
    TailBwd a{dout, dln, x3, f1, out, ctx, Wo, gf, bf, W1, W2, ge, dlang, dctx, P > 1 ? part : grads,
              epsf, epse, p, seed, (int)N, P};
    if (dln != nullptr) hipLaunchKernelGGL(lava_lang_tail_bwd_kernel<true>, dim3(P), dim3(kThreads), 0, stream, a);
    else hipLaunchKernelGGL(lava_lang_tail_bwd_kernel<false>, dim3(P), dim3(kThreads), 0, stream, a);
    reduce(part, P, kE, grads, stream);
    return (int)hipGetLastError();
}

// grads: [kE] = d in_proj_weight [384][128], d in_proj_bias [384], d ln_pix weight, bias [128], 0 [3][128]
extern "C" int rt1_lava_lang_attn_pgrad(const float* Q, const float* dQ, const float* q, const float* dctx,
                                        const float* u, const float* w, const float* z, const float* e, const float* g,
                                        const float* b, int64_t N, float* part, float* grads, hipStream_t stream) {
    if (Q == nullptr || dQ == nullptr || q == nullptr || dctx == nullptr || u == nullptr || w == nullptr ||
        z == nullptr || e == nullptr || g == nullptr || b == nullptr || part == nullptr || grads == nullptr ||
        bad_rows(N))
        return (int)hipErrorInvalidValue;
    const int P = partials(N);
    AttnPg a{Q, dQ, q, dctx, u, w, z, e, g, b, P > 1 ? part : grads, (int)N, P};
    hipLaunchKernelGGL(lava_lang_attn_pgrad_kernel, dim3(P), dim3(kThreads), 0, stream, a);
    reduce(part, P, kE, grads, stream);
    return (int)hipGetLastError();
}
