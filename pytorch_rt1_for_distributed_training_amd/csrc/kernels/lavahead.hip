// LAVA policy head (gfx950, wave64): DenseResnet + action_projection, a chain of short-wide linears on [B, .] rows,
// fp32 in and out.
//
//   h  = x Win^T + bin                                                    din -> width
//   h += relu(relu(relu(h) W1^T + b1) W2^T + b2) W3^T + b3   per block     width -> width/4 -> width/4 -> width
//   action = h Wa^T + ba                                                  width -> action_size (<= 8)
//
// Few rows (B = 4 .. a few hundred), fat weights (5.2 MB at width 1024): the opposite of lavalang.hip, whose row tile
// streams 64 KB of weights through LDS per workgroup.  Here the OUTPUT COLUMNS are split, not the rows.
//
// Forward linear, Y = pro(X) W^T + b (+ R), one launch.  A 256-lane workgroup owns a tile of 16 output columns and all
// rows of a row chunk; its four waves split the reduced index K into quarters, each wave keeps one 16 x 16 fp32
// accumulator per 16-row M-tile (v_mfma_f32_16x16x4_f32, fp32 operands), and waves 1 .. 3 hand their accumulators to
// wave 0 through LDS, which adds them in wave order and runs the epilogue (bias, residual R = the block input).  pro
// is identity or ReLU on the A operand as it is loaded: what a linear stores is its pre-activation, which the backward
// needs for relu' anyway.  lavalang.hip's k-ordering: lane group g = lane / 16 takes k = 16 t + 4 g + c for step
// (t, c), so with W [Nout, K] (k contiguous) a lane's four B values are ONE 16-byte global load and its four A values
// one 16-byte load of an X row.  An element of W is needed by one workgroup of a row chunk only: it goes from memory
// straight to registers and is used for every M-tile of the chunk; nothing but the wave sum passes through LDS.
//
// Column tile and row chunk.  The tile is 16 columns, the width of the matrix instruction, for every layer: at
// Nout = 256 that is already only 16 tiles, and a wider tile would halve the workgroups.  The price is that every
// workgroup reads all of its chunk's X; whether those re-reads are served by L2 has not been measured, and the
// 256-row kernels reach only 75-140 GB/s.  What is chosen from Nout and B is the row chunk (M-tiles
// per workgroup, a template parameter so the accumulators stay in registers): 16 rows for B <= 16; 64 rows for
// B <= 64 and for every B when Nout <= 256 (the 1024 -> 256 and 256 -> 256 layers: 16 column tiles x B / 64 chunks
// keeps 64 workgroups busy at B = 256, and a workgroup reads a quarter of X instead of all of it; the 1 MB weight is
// then read once per chunk); 256 rows (64 accumulator registers) otherwise, where Nout = 1024 gives 64 column
// tiles on its own.  Larger B walks several chunks as blockIdx.y.
//
// Backward of a linear, one launch, two roles by blockIdx range; both read dY and X.
//   data gradient    dX = dY W: the forward's routine with the roles of K and Nout exchanged (a 16-column tile of K,
//                    waves split Nout; W^T is read as four 4-byte loads per step, 64 contiguous bytes per lane group).
//                    The epilogue multiplies by relu'(X > 0) where the forward had the ReLU prologue and adds the
//                    residual branch's gradient for a block's first linear, so a block's dx is written once.
//   weight gradient  dW = dY^T pro(X): a WAVE owns a 16 (Nout) x 64 (K) tile of dW and reduces over all B rows itself,
//                    four rows per matrix instruction in row order.  Output column 4 r + c belongs to accumulator c of
//                    lane r, so the B operand of the four accumulators is one 16-byte load of an X row and dW is
//                    stored in 16-byte pieces.  db is the same sum against a column of ones (one more matrix
//                    instruction per step) in the waves that own k = 0.  No split-K partials, no workspace, no
//                    reduce launch: dW and db are written once.
//
// Action projection, action_size <= 8: too narrow for a matrix tile.  Forward: a wave per row, each lane 16-byte
// pieces of the row against every Wa row, a fixed DPP / readlane tree over the 64 lanes.  Backward, one launch, two
// roles: dWa / dba, a workgroup per 64 columns with 16 row groups walking the rows 16 apart and added in group order
// through LDS; dh [B, width], a workgroup per row.
//
// No kernel uses scratch, there are no atomics, and every output is a function of the inputs alone, bitwise.  Every
// kernel is built without packed fp32 (common.h NO_PACKED_FP32): such a kernel inlines only always_inline callees, so
// the bodies call __forceinline__ functions and builtins only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kCT = 16;                           // output columns of a workgroup
constexpr int kChunk = 256;                       // rows of the largest row chunk
constexpr int kWK = 64;                           // K columns of a wave's dW tile
constexpr int kMaxDim = 8192;                     // din, width
constexpr int kMaxRows = 1 << 20;
constexpr int kMaxAct = 8;
constexpr int kPK = 64;                           // columns of a projection-backward workgroup
constexpr int kPG = 16;                           // its row groups

template <int CTRL>
__device__ __forceinline__ float dpp(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}

__device__ __forceinline__ void block_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// sum over the 64 lanes in a fixed order: lavaxattn.hip's butterfly inside a DPP row, then the four rows in row order
__device__ __forceinline__ float wave_sum64(float x) {
    x += dpp<0xB1>(x);
    x += dpp<0x4E>(x);
    x += dpp<0x141>(x);
    x += dpp<0x140>(x);
    const int v = __float_as_int(x);
    return ((__int_as_float(__builtin_amdgcn_readlane(v, 0)) + __int_as_float(__builtin_amdgcn_readlane(v, 16))) +
            __int_as_float(__builtin_amdgcn_readlane(v, 32))) + __int_as_float(__builtin_amdgcn_readlane(v, 48));
}

__device__ __forceinline__ float relu(float v) { return v < 0.f ? 0.f : v; }     // NaN stays NaN, like torch

// acc[mt] += pro(A)[m0 + 16 mt + r][j] Op[j][c0 + r] over j in [16 t0, 16 t1); Op = W^T for W [., ldw] with j
// contiguous (NT: the forward) or Op = W with W [j][ldw] (NN: the data gradient).  Rows >= rows read as zero.
template <int MT, bool NN, bool PRO>
__device__ __forceinline__ void tile_mma(const float* __restrict__ A, int lda, int rows, int m0,
                                         const float* __restrict__ W, int ldw, int c0, int t0, int t1, int lane,
                                         f32x4 (&acc)[MT]) {
    const int r = lane & 15, g = lane >> 4;
    for (int t = t0; t < t1; ++t) {
        const int j = 16 * t + 4 * g;
        f32x4 b;
        if constexpr (NN) {
#pragma unroll
            for (int c = 0; c < 4; ++c) b[c] = W[(int64_t)(j + c) * ldw + c0 + r];
        } else {
            b = *reinterpret_cast<const f32x4*>(W + (int64_t)(c0 + r) * ldw + j);
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            if (m0 + 16 * mt >= rows) continue;                          // the same for the whole workgroup
            const int row = m0 + 16 * mt + r;
            f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
            if (row < rows) a = *reinterpret_cast<const f32x4*>(A + (int64_t)row * lda + j);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(PRO ? relu(a[c]) : a[c], b[c], acc[mt], 0, 0, 0);
        }
    }
}

// the four waves' accumulators added in wave order into wave 0's; red: [3][MT][4][64]
template <int MT>
__device__ __forceinline__ void wave_order_sum(f32x4 (&acc)[MT], float* red, int wave, int lane) {
    if (wave > 0) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int q = 0; q < 4; ++q) red[(((wave - 1) * MT + mt) * 4 + q) * 64 + lane] = acc[mt][q];
    }
    block_sync();
    if (wave == 0) {
#pragma unroll
        for (int w = 0; w < kWaves - 1; ++w)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[mt][q] += red[((w * MT + mt) * 4 + q) * 64 + lane];
    }
}

template <int MT>
__device__ __forceinline__ void acc_zero(f32x4 (&acc)[MT]) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// ---- forward linear --------------------------------------------------------------------------------------------------

struct LinFwd {
    const float* x;      // [B, K], the pre-activation when PRO
    const float* w;      // [N, K]
    const float* b;      // [N]
    const float* res;    // [B, N] or nullptr
    float* y;            // [B, N]
    int B, K, N;
};

template <int MT, bool PRO>
__global__ NO_PACKED_FP32 __launch_bounds__(kThreads) void lava_head_linear_fwd_kernel(LinFwd a) {
    __shared__ float red[(kWaves - 1) * MT * 4 * 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int c0 = blockIdx.x * kCT, m0 = blockIdx.y * (16 * MT), steps = a.K / (16 * kWaves);
    f32x4 acc[MT];
    acc_zero<MT>(acc);
    tile_mma<MT, false, PRO>(a.x, a.K, a.B, m0, a.w, a.K, c0, wave * steps, (wave + 1) * steps, lane, acc);
    wave_order_sum<MT>(acc, red, wave, lane);
    if (wave != 0) return;
    const int col = c0 + r;
    const float bias = a.b[col];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = m0 + 16 * mt + 4 * g + q;
            if (row < a.B) {
                const int64_t o = (int64_t)row * a.N + col;
                float v = acc[mt][q] + bias;
                if (a.res != nullptr) v += a.res[o];
                a.y[o] = v;
            }
        }
}

// ---- backward of a linear --------------------------------------------------------------------------------------------

struct LinBwd {
    const float* dy;     // [B, N]
    const float* x;      // [B, K], what the forward read
    const float* w;      // [N, K]
    const float* rg;     // [B, K] or nullptr: the gradient the residual branch brings to x
    float* dx;           // [B, K]
    float* dw;           // [N, K]
    float* db;           // [N]
    int B, K, N;
    int dblocks;         // workgroups of the data gradient: (K / 16) column tiles x row chunks
};

template <int MT, bool PRO>
__global__ NO_PACKED_FP32 __launch_bounds__(kThreads) void lava_head_linear_bwd_kernel(LinBwd a) {
    __shared__ float red[(kWaves - 1) * MT * 4 * 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    if ((int)blockIdx.x < a.dblocks) {
        const int ktiles = a.K / kCT, c0 = ((int)blockIdx.x % ktiles) * kCT, m0 = ((int)blockIdx.x / ktiles) * (16 * MT);
        const int steps = a.N / (16 * kWaves);
        f32x4 acc[MT];
        acc_zero<MT>(acc);
        tile_mma<MT, true, false>(a.dy, a.N, a.B, m0, a.w, a.K, c0, wave * steps, (wave + 1) * steps, lane, acc);
        wave_order_sum<MT>(acc, red, wave, lane);
        if (wave != 0) return;
        const int col = c0 + r;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = m0 + 16 * mt + 4 * g + q;
                if (row < a.B) {
                    const int64_t o = (int64_t)row * a.K + col;
                    float v = acc[mt][q];
                    if (PRO) v = a.x[o] > 0.f ? v : 0.f;
                    if (a.rg != nullptr) v += a.rg[o];
                    a.dx[o] = v;
                }
            }
        return;
    }
    // dW tile of this wave: rows n0 .. n0 + 15 of dW, columns k0 .. k0 + 63; acc[c][q] is dW[n0 + 4 g + q][k0 + 4 r + c]
    const int ntiles = a.N / 16, id = ((int)blockIdx.x - a.dblocks) * kWaves + wave;
    if (id >= ntiles * (a.K / kWK)) return;
    const int n0 = (id % ntiles) * 16, k0 = (id / ntiles) * kWK;
    const bool bias = k0 == 0;
    f32x4 acc[4], accb = f32x4{0.f, 0.f, 0.f, 0.f};
    acc_zero<4>(acc);
    for (int s = 0; s < a.B; s += 4) {
        const int row = s + g;
        float dv = 0.f;
        f32x4 xv = f32x4{0.f, 0.f, 0.f, 0.f};
        if (row < a.B) {
            dv = a.dy[(int64_t)row * a.N + n0 + r];
            xv = *reinterpret_cast<const f32x4*>(a.x + (int64_t)row * a.K + k0 + 4 * r);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(dv, PRO ? relu(xv[c]) : xv[c], acc[c], 0, 0, 0);
        if (bias) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(dv, 1.f, accb, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        *reinterpret_cast<f32x4*>(a.dw + (int64_t)(n0 + 4 * g + q) * a.K + k0 + 4 * r) =
            f32x4{acc[0][q], acc[1][q], acc[2][q], acc[3][q]};
        if (bias && r == 0) a.db[n0 + 4 * g + q] = accb[q];
    }
}

// ---- action projection -----------------------------------------------------------------------------------------------

// y[row][a] = x[row] . w[a] + b[a]: a wave per row
__global__ NO_PACKED_FP32 __launch_bounds__(kThreads) void lava_head_proj_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, int B, int K, int A,
    float* __restrict__ y) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, row = blockIdx.x * kWaves + wave;
    if (row >= B) return;
    float s[kMaxAct];
#pragma unroll
    for (int i = 0; i < kMaxAct; ++i) s[i] = 0.f;
    for (int k = 4 * lane; k < K; k += 256) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (int64_t)row * K + k);
#pragma unroll
        for (int i = 0; i < kMaxAct; ++i)
            if (i < A) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (int64_t)i * K + k);
                s[i] = fmaf(xv[3], wv[3], fmaf(xv[2], wv[2], fmaf(xv[1], wv[1], fmaf(xv[0], wv[0], s[i]))));
            }
    }
#pragma unroll
    for (int i = 0; i < kMaxAct; ++i)
        if (i < A) {
            const float v = wave_sum64(s[i]);
            if (lane == 0) y[(int64_t)row * A + i] = v + b[i];
        }
}

struct ProjBwd {
    const float* dy;     // [B, A]
    const float* x;      // [B, K]
    const float* w;      // [A, K]
    float* dx;           // [B, K]
    float* dw;           // [A, K]
    float* db;           // [A]
    int B, K, A;
    int wblocks;         // K / 64 workgroups of the parameter gradients, then one per row for dx
};

__global__ NO_PACKED_FP32 __launch_bounds__(kThreads) void lava_head_proj_bwd_kernel(ProjBwd a) {
    __shared__ __attribute__((aligned(16))) float red[kPG][kMaxAct][kPK];
    __shared__ double redb[kPG][kMaxAct];             // dba: at most 8 sums over B rows, kept in fp64
    const int t = threadIdx.x;
    if ((int)blockIdx.x >= a.wblocks) {
        const int row = (int)blockIdx.x - a.wblocks;
        for (int k = 4 * t; k < a.K; k += 4 * kThreads) {
            f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int i = 0; i < a.A; ++i) {
                const float d = a.dy[(int64_t)row * a.A + i];
                const f32x4 wv = *reinterpret_cast<const f32x4*>(a.w + (int64_t)i * a.K + k);
#pragma unroll
                for (int c = 0; c < 4; ++c) s[c] = fmaf(d, wv[c], s[c]);
            }
            *reinterpret_cast<f32x4*>(a.dx + (int64_t)row * a.K + k) = s;
        }
        return;
    }
    // row group rg takes rows rg, rg + 16, ..; lane l of it the columns k0 + 4 l .. + 3
    const int k0 = blockIdx.x * kPK, rg = t >> 4, l = t & 15;
    f32x4 acc[kMaxAct];
    double sb[kMaxAct];
#pragma unroll
    for (int i = 0; i < kMaxAct; ++i) {
        acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        sb[i] = 0.0;
    }
    for (int row = rg; row < a.B; row += kPG) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(a.x + (int64_t)row * a.K + k0 + 4 * l);
#pragma unroll
        for (int i = 0; i < kMaxAct; ++i)
            if (i < a.A) {
                const float d = a.dy[(int64_t)row * a.A + i];
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[i][c] = fmaf(d, xv[c], acc[i][c]);
                sb[i] += (double)d;
            }
    }
#pragma unroll
    for (int i = 0; i < kMaxAct; ++i) {
        *reinterpret_cast<f32x4*>(&red[rg][i][4 * l]) = acc[i];
        if (l == 0) redb[rg][i] = sb[i];
    }
    block_sync();
    for (int o = t; o < kMaxAct * kPK; o += kThreads) {
        const int i = o / kPK, kk = o % kPK;
        if (i < a.A) {
            float s = red[0][i][kk];
#pragma unroll
            for (int p = 1; p < kPG; ++p) s += red[p][i][kk];
            a.dw[(int64_t)i * a.K + k0 + kk] = s;
        }
    }
    if (blockIdx.x == 0 && t < a.A) {
        double s = redb[0][t];
#pragma unroll
        for (int p = 1; p < kPG; ++p) s += redb[p][t];
        a.db[t] = (float)s;
    }
}

bool bad_dims(int64_t B, int64_t K, int64_t N) {
    return B < 1 || B > kMaxRows || K < 64 || K > kMaxDim || K % 64 != 0 || N < 64 || N > kMaxDim || N % 64 != 0;
}

// M-tiles per workgroup (see the header): 1, 4 or 16
int mtiles(int64_t B, int64_t cols) { return B <= 16 ? 1 : (B <= 64 || cols <= 256) ? 4 : kChunk / 16; }

}  // namespace

extern "C" int rt1_lava_head_supported(int din, int width, int action_size) {
    return din >= 64 && din <= kMaxDim && din % 64 == 0 && width >= 256 && width <= kMaxDim && width % 256 == 0 &&
           action_size >= 1 && action_size <= kMaxAct;
}

extern "C" int rt1_lava_head_row_chunk() { return kChunk; }

extern "C" int rt1_lava_head_linear_fwd(const float* x, const float* w, const float* b, const float* res, int64_t B,
                                        int64_t K, int64_t N, int relu_in, float* y, hipStream_t stream) {
    if (x == nullptr || w == nullptr || b == nullptr || y == nullptr || bad_dims(B, K, N))
        return (int)hipErrorInvalidValue;
    LinFwd a{x, w, b, res, y, (int)B, (int)K, (int)N};
    const int mt = mtiles(B, N);
    const dim3 grid((unsigned)(N / kCT), (unsigned)((B + 16 * mt - 1) / (16 * mt))), block(kThreads);
#define RT1_HEAD_FWD(MT)                                                                                     \
    if (relu_in) hipLaunchKernelGGL((lava_head_linear_fwd_kernel<MT, true>), grid, block, 0, stream, a);    \
    else hipLaunchKernelGGL((lava_head_linear_fwd_kernel<MT, false>), grid, block, 0, stream, a)
    if (mt == 1) { RT1_HEAD_FWD(1); }
    else if (mt == 4) { RT1_HEAD_FWD(4); }
    else { RT1_HEAD_FWD(16); }
#undef RT1_HEAD_FWD
    return (int)hipGetLastError();
}

extern "C" int rt1_lava_head_linear_bwd(const float* dy, const float* x, const float* w, const float* rg, int64_t B,
                                        int64_t K, int64_t N, int relu_in, float* dx, float* dw, float* db,
                                        hipStream_t stream) {
    if (dy == nullptr || x == nullptr || w == nullptr || dx == nullptr || dw == nullptr || db == nullptr ||
        bad_dims(B, K, N))
        return (int)hipErrorInvalidValue;
    const int mt = mtiles(B, K);
    const int64_t dblocks = (K / kCT) * ((B + 16 * mt - 1) / (16 * mt));
    const int64_t wblocks = ((N / 16) * (K / kWK) + kWaves - 1) / kWaves;
    if (dblocks + wblocks > INT32_MAX) return (int)hipErrorInvalidValue;
    LinBwd a{dy, x, w, rg, dx, dw, db, (int)B, (int)K, (int)N, (int)dblocks};
    const dim3 grid((unsigned)(dblocks + wblocks)), block(kThreads);
#define RT1_HEAD_BWD(MT)                                                                                     \
    if (relu_in) hipLaunchKernelGGL((lava_head_linear_bwd_kernel<MT, true>), grid, block, 0, stream, a);    \
    else hipLaunchKernelGGL((lava_head_linear_bwd_kernel<MT, false>), grid, block, 0, stream, a)
    if (mt == 1) { RT1_HEAD_BWD(1); }
    else if (mt == 4) { RT1_HEAD_BWD(4); }
    else { RT1_HEAD_BWD(16); }
#undef RT1_HEAD_BWD
    return (int)hipGetLastError();
}

extern "C" int rt1_lava_head_proj_fwd(const float* x, const float* w, const float* b, int64_t B, int64_t K, int64_t A,
                                      float* y, hipStream_t stream) {
    if (x == nullptr || w == nullptr || b == nullptr || y == nullptr || bad_dims(B, K, 64) || A < 1 || A > kMaxAct)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(lava_head_proj_fwd_kernel, dim3((unsigned)((B + kWaves - 1) / kWaves)), dim3(kThreads), 0,
                       stream, x, w, b, (int)B, (int)K, (int)A, y);
    return (int)hipGetLastError();
}

extern "C" int rt1_lava_head_proj_bwd(const float* dy, const float* x, const float* w, int64_t B, int64_t K, int64_t A,
                                      float* dx, float* dw, float* db, hipStream_t stream) {
    if (dy == nullptr || x == nullptr || w == nullptr || dx == nullptr || dw == nullptr || db == nullptr ||
        bad_dims(B, K, 64) || A < 1 || A > kMaxAct)
        return (int)hipErrorInvalidValue;
    const int wblocks = (int)(K / kPK);
    ProjBwd a{dy, x, w, dx, dw, db, (int)B, (int)K, (int)A, wblocks};
    hipLaunchKernelGGL(lava_head_proj_bwd_kernel, dim3((unsigned)(wblocks + B)), dim3(kThreads), 0, stream, a);
    return (int)hipGetLastError();
}
