// LAVA pixel-language cross attention with ONE query token per frame, folded so that neither the normalised pixels
// nor K / V are ever formed (gfx950, wave64).  d = 128, H = 2 heads of 64 (the only shape CrossLayer builds).
//
// With x^_j the LayerNorm of pixel row j before its affine (g, b), Q = W_q q + b_q and scale = 1 / sqrt(64):
//
//   u_h = scale W_k,h^T Q_h            c_h = scale Q_h . b_k,h
//   s_j,h = x^_j . (g * u_h) + b . u_h + c_h                      the score of row j, a 128-float dot per head
//   z_h = sum_j a_j,h x^_j             ctx_h = W_v,h (g * z_h + b) + b_v,h          (sum_j a_j,h = 1)
//
// and in the backward, with w_h = W_v,h^T dctx_h:
//
//   t_j,h = x^_j . (g * w_h)           ds_j,h = a_j,h (t_j,h - (g * w_h) . z_h)     (the b . w_h terms cancel)
//   dx^_j = sum_h a_j,h (g * w_h) + ds_j,h (g * u_h)              dpix_j = rstd_j (dx^_j - m1 - x^_j m2)
//   m1 = mean(dx^_j) = sum_h a_j,h mean(g * w_h) + ds_j,h mean(g * u_h)             no reduction: frame constants
//   m2 = mean(dx^_j * x^_j) = sum_h (a_j,h t_j,h + ds_j,h x^_j . (g * u_h)) / d     no reduction: the row's own dots
//   e_h = sum_j ds_j,h x^_j            dQ_h = scale W_k,h (g * e_h)                 dq = W_q^T dQ
//
// A layer's forward is one streamed read of pixels [N, S, d]; its backward one read and one dpix write.
//
// Work split.  Frames alone do not fill the card (16 per device in the reference config), so the grid is frames x row
// chunks of kChunk = 128 rows, flash-decoding style.  A workgroup is 256 lanes = 16 row groups of 16 lanes (one DPP
// row); a pixel row is 512 B = 2 x float4 per lane (columns 4l .. 4l+3 and 64+4l .. 64+4l+3, so each load instruction
// of a group covers 256 contiguous bytes and a wave covers 4 adjacent rows).  Group r takes rows r, r + 16, ... of the
// chunk, four rows' loads issued before the first is used.  Every per-row reduction (forward: mean, variance, two
// scores; backward: those and the two t) is the fixed DPP butterfly of lamb.hip inside the 16 lanes, which leaves the
// same bits in all of them.  The folded vectors g * u_h, g * w_h are frame constants in registers, 8 floats per lane
// each; z_h (online softmax, the usual rescale) and e_h accumulate in registers and the 16 groups are combined through
// LDS once per chunk, in group order.  Per chunk the forward leaves a partial (max m, sum l, z[H][d]) and the backward
// e[H][d]; a one-workgroup-per-frame kernel combines them IN CHUNK ORDER.  No atomics anywhere: a result is a function
// of the inputs alone, bitwise.  dpix needs no combine (rows are independent given the saved log-sum-exp).
//
// MFMA does not fit: the row-side products have two useful output columns (the heads), a matrix instruction would
// spend 14 / 16 or 30 / 32 of its columns on zeros and the kernel is bound by the pixel stream anyway.
//
// The per-frame d x d matvecs live in the one-workgroup-per-frame kernels: the prologue (q -> Q -> u, c; in the
// backward also dctx -> w and the frame constants) and the combine (z -> ctx; e -> dQ -> dq).  A product W x reads
// W's rows with a 16-lane group per output and the row butterfly; a product W^T x gives lane k column k.  The sums
// over FRAMES (dW_q, dW_k, dW_v, the bias gradients, dgamma, dbeta) are left to the caller: they are [d, N] x [N, d]
// over this file's per-frame outputs Q, dQ, u, w, z, e.
//
// A frame of identical rows has variance 0: a lane adds its 8 values as a tree and the butterfly doubles, so the mean
// of identical values is exact, x^ = 0, every score is the frame constant and a = 1 / S; nothing divides by the
// variance (rstd = rsqrt(0 + eps)).
//
// Every kernel is built without packed fp32 (common.h NO_PACKED_FP32), so the unit carries no v_pk_*_f32 at all; such
// a kernel inlines only always_inline callees, so the bodies call __forceinline__ functions and builtins and fill
// float4 by member.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace {

constexpr int kD = 128, kH = 2, kDh = 64;
constexpr int kThreads = 256;
constexpr int kGroups = kThreads / 16;            // row groups of one workgroup
constexpr int kChunk = 128;                       // pixel rows per workgroup
constexpr int kRowsPerGroup = kChunk / kGroups;   // 8
constexpr int kBatch = 4;                         // rows of a group whose loads are in flight together
constexpr float kScale = 0.125f;                  // 1 / sqrt(kDh)
constexpr float kInvD = 1.f / kD;
constexpr int kFc = 8;                            // frame constants: c'_h, (g w_h).z_h, mean(g u_h), mean(g w_h)

template <int CTRL>
__device__ __forceinline__ float dpp(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}

// __syncthreads() spelled out: under NO_PACKED_FP32 the header's function would be a call
__device__ __forceinline__ void block_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// sum over the 16 lanes of a DPP row in a fixed order; every lane of the row ends with the same bits (lamb.hip)
__device__ __forceinline__ float row_sum16(float x) {
    x += dpp<0xB1>(x);     // quad_perm [1, 0, 3, 2]: lane ^ 1
    x += dpp<0x4E>(x);     // quad_perm [2, 3, 0, 1]: lane ^ 2
    x += dpp<0x141>(x);    // row_half_mirror: the other quad of the half row
    x += dpp<0x140>(x);    // row_mirror: the other half row
    return x;
}

// lane l of a group holds columns 4l .. 4l+3 and 64+4l .. 64+4l+3 of a 128-float vector
__device__ __forceinline__ void load_vec(const float* __restrict__ p, int l, float (&o)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p + 4 * l);
    const float4 b = *reinterpret_cast<const float4*>(p + 64 + 4 * l);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}

__device__ __forceinline__ void store_vec(float* __restrict__ p, int l, const float (&v)[8]) {
    float4 a, b;
    a.x = v[0]; a.y = v[1]; a.z = v[2]; a.w = v[3]; b.x = v[4]; b.y = v[5]; b.z = v[6]; b.w = v[7];
    *reinterpret_cast<float4*>(p + 4 * l) = a;
    *reinterpret_cast<float4*>(p + 64 + 4 * l) = b;
}

__device__ __forceinline__ float dot8(const float (&a)[8], const float (&b)[8]) {
    float s = a[0] * b[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) s = fmaf(a[i], b[i], s);
    return s;
}

// LayerNorm of one row without the affine, in place; returns rstd.  The lane sum is a tree and the butterfly doubles,
// so the mean of identical values is exact.
__device__ __forceinline__ float normalise(float (&x)[8], float eps) {
    const float mean = row_sum16(((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]))) * kInvD;
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] -= mean;
    const float rstd = rsqrtf(fmaf(row_sum16(dot8(x, x)), kInvD, eps));
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] *= rstd;
    return rstd;
}

// y = W[i, :] . x for row i of a row-major [128, 128] block, x = sx + (i / 64) * stride_h (a vector per head) in
// LDS, by the 16-lane group that calls it; every lane of the group returns y.  A workgroup covers the 128 rows with
// i = it * kGroups + group, it < kD / kGroups.
__device__ __forceinline__ float row_dot(const float* __restrict__ W, const float* sx, int stride_h, int i, int l) {
    float wr[8], xr[8];
    load_vec(W + (int64_t)i * kD, l, wr);
    load_vec(sx + (i >> 6) * stride_h, l, xr);
    return row_sum16(dot8(wr, xr));
}

// y_h[k] = sum_i W[h * 64 + i, k] x[h * 64 + i] for thread (h, k) = (t >> 7, t & 127), x in LDS
__device__ __forceinline__ float cols_dot_head(const float* __restrict__ W, const float* sx) {
    const int h = threadIdx.x >> 7, k = threadIdx.x & 127;
    float acc = 0.f;
#pragma unroll 8
    for (int i = 0; i < kDh; ++i) acc = fmaf(W[(int64_t)(h * kDh + i) * kD + k], sx[h * kDh + i], acc);
    return acc;
}

// One workgroup per frame.  Forward: q -> Q -> u_h and c'_h = b . u_h + scale Q_h . b_k,h.  Backward: Q is the saved
// one; also dctx -> w_h and the constants (g w_h) . z_h, mean(g u_h), mean(g w_h).
template <bool BWD>
__global__ NO_PACKED_FP32 __launch_bounds__(kThreads) void lava_xattn_prologue_kernel(
    const float* __restrict__ q, const float* __restrict__ dctx, const float* __restrict__ z,
    const float* __restrict__ g, const float* __restrict__ b, const float* __restrict__ W,
    const float* __restrict__ bias, float* __restrict__ Q, float* __restrict__ u, float* __restrict__ w,
    float* __restrict__ fc) {
    __shared__ __attribute__((aligned(16))) float s_in[kD];
    __shared__ __attribute__((aligned(16))) float s_Q[kD];
    __shared__ __attribute__((aligned(16))) float s_u[kH][kD];
    __shared__ __attribute__((aligned(16))) float s_w[kH][kD];
    const int n = blockIdx.x, t = threadIdx.x, l = t & 15, gi = t >> 4;
    const float* Wq = W;
    const float* Wk = W + kD * kD;
    const float* Wv = W + 2 * kD * kD;
    if constexpr (BWD) {
        if (t < kD) {
            s_Q[t] = Q[(int64_t)n * kD + t];
            s_in[t] = dctx[(int64_t)n * kD + t];
        }
        block_sync();
    } else {
        if (t < kD) s_in[t] = q[(int64_t)n * kD + t];
        block_sync();
#pragma unroll 2
        for (int it = 0; it < kD / kGroups; ++it) {
            const int i = it * kGroups + gi;
            const float v = row_dot(Wq, s_in, 0, i, l) + bias[i];      // both heads read the same q: stride 0
            if (l == 0) {
                s_Q[i] = v;
                Q[(int64_t)n * kD + i] = v;
            }
        }
        block_sync();
    }
    {
        const float uv = kScale * cols_dot_head(Wk, s_Q);
        s_u[t >> 7][t & 127] = uv;
        u[(int64_t)n * kH * kD + t] = uv;
        if constexpr (BWD) {
            const float wv = cols_dot_head(Wv, s_in);
            s_w[t >> 7][t & 127] = wv;
            w[(int64_t)n * kH * kD + t] = wv;
        }
    }
    block_sync();
    if (gi < kH) {            // one 16-lane group per head
        const int h = gi;
        float gv[8], bv[8], uv[8];
        load_vec(g, l, gv);
        load_vec(b, l, bv);
        load_vec(s_u[h], l, uv);
        float qb = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) qb = fmaf(s_Q[h * kDh + 4 * l + j], bias[kD + h * kDh + 4 * l + j], qb);
        const float bu = row_sum16(dot8(bv, uv));
        const float gu = row_sum16(dot8(gv, uv));
        qb = row_sum16(qb);
        float gwz = 0.f, gw = 0.f;
        if constexpr (BWD) {
            float wv[8], zv[8];
            load_vec(s_w[h], l, wv);
            load_vec(z + ((int64_t)n * kH + h) * kD, l, zv);
#pragma unroll
            for (int i = 0; i < 8; ++i) wv[i] *= gv[i];
            gwz = row_sum16(dot8(wv, zv));
            gw = row_sum16(((wv[0] + wv[1]) + (wv[2] + wv[3])) + ((wv[4] + wv[5]) + (wv[6] + wv[7])));
        }
        if (l == 0) {
            float* f = fc + (int64_t)n * kFc;
            f[h] = fmaf(kScale, qb, bu);
            f[4 + h] = gu * kInvD;
            if constexpr (BWD) {
                f[2 + h] = gwz;
                f[6 + h] = gw * kInvD;
            }
        }
    }
}

// Forward over one chunk of one frame: the partial (m, l, z[H][d]) of the online softmax over its rows.
__global__ NO_PACKED_FP32 __launch_bounds__(kThreads) void lava_xattn_fwd_rows_kernel(
    const float* __restrict__ pix, const float* __restrict__ g, const float* __restrict__ u,
    const float* __restrict__ fc, float eps, int S, int C, float* __restrict__ pm, float* __restrict__ pl,
    float* __restrict__ pz) {
    __shared__ __attribute__((aligned(16))) float s_z[kGroups][kH][kD];
    __shared__ float s_m[kGroups][kH], s_l[kGroups][kH];
    const int n = blockIdx.x / C, c = blockIdx.x - n * C;
    const int t = threadIdx.x, l = t & 15, gi = t >> 4;
    float gu[kH][8];
    {
        float gv[8];
        load_vec(g, l, gv);
#pragma unroll
        for (int h = 0; h < kH; ++h) {
            load_vec(u + ((int64_t)n * kH + h) * kD, l, gu[h]);
#pragma unroll
            for (int i = 0; i < 8; ++i) gu[h][i] *= gv[i];
        }
    }
    const float cc[kH] = {fc[(int64_t)n * kFc], fc[(int64_t)n * kFc + 1]};
    const float* base = pix + (int64_t)n * S * kD;
    const int row0 = c * kChunk + gi;
    float m[kH], ls[kH], zz[kH][8];
#pragma unroll
    for (int h = 0; h < kH; ++h) {
        m[h] = -INFINITY;
        ls[h] = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) zz[h][i] = 0.f;
    }
#pragma unroll
    for (int b0 = 0; b0 < kRowsPerGroup; b0 += kBatch) {
        float x[kBatch][8];
#pragma unroll
        for (int j = 0; j < kBatch; ++j)      // a row past the end reads row S - 1 and is not used
            load_vec(base + (int64_t)min(row0 + (b0 + j) * kGroups, S - 1) * kD, l, x[j]);
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            if (row0 + (b0 + j) * kGroups < S) {       // uniform over the 16 lanes of the group
                normalise(x[j], eps);
#pragma unroll
                for (int h = 0; h < kH; ++h) {
                    const float s = row_sum16(dot8(x[j], gu[h])) + cc[h];
                    // one exponential per row and head: the larger of (m, s) keeps weight 1
                    const float dlt = s - m[h];
                    const float ex = expf(-fabsf(dlt));
                    const bool up = dlt > 0.f;
                    const float corr = up ? ex : 1.f, p = up ? 1.f : ex;
                    m[h] = up ? s : m[h];
                    ls[h] = fmaf(ls[h], corr, p);
#pragma unroll
                    for (int i = 0; i < 8; ++i) zz[h][i] = fmaf(p, x[j][i], zz[h][i] * corr);
                }
            }
        }
    }
#pragma unroll
    for (int h = 0; h < kH; ++h) {
        store_vec(s_z[gi][h], l, zz[h]);
        if (l == 0) {
            s_m[gi][h] = m[h];
            s_l[gi][h] = ls[h];
        }
    }
    block_sync();
    // thread (h, k) combines the 16 groups in group order; group 0 always has a row, so M is a score
    const int h = t >> 7, k = t & 127;
    float M = s_m[0][h];
#pragma unroll
    for (int r = 1; r < kGroups; ++r) M = fmaxf(M, s_m[r][h]);
    float acc = 0.f, L = 0.f;
#pragma unroll
    for (int r = 0; r < kGroups; ++r) {
        const float wgt = expf(s_m[r][h] - M);          // 0 for a group without rows (m = -inf)
        acc = fmaf(wgt, s_z[r][h][k], acc);
        L = fmaf(wgt, s_l[r][h], L);
    }
    const int64_t pc = (int64_t)blockIdx.x * kH + h;
    pz[pc * kD + k] = acc;
    if (k == 0) {
        pm[pc] = M;
        pl[pc] = L;
    }
}

// One workgroup per frame: the chunk partials in chunk order -> z, log-sum-exp; then ctx_h = W_v,h (g z_h + b) + b_v,h.
__global__ NO_PACKED_FP32 __launch_bounds__(kThreads) void lava_xattn_fwd_combine_kernel(
    const float* __restrict__ pm, const float* __restrict__ pl, const float* __restrict__ pz, int C,
    const float* __restrict__ g, const float* __restrict__ b, const float* __restrict__ W,
    const float* __restrict__ bias, float* __restrict__ z, float* __restrict__ lse, float* __restrict__ ctx) {
    __shared__ __attribute__((aligned(16))) float s_xv[kH][kD];
    const int n = blockIdx.x, t = threadIdx.x, h = t >> 7, k = t & 127;
    const int64_t p0 = (int64_t)n * C * kH + h;
    float M = pm[p0];
    for (int c = 1; c < C; ++c) M = fmaxf(M, pm[p0 + (int64_t)c * kH]);
    float acc = 0.f, L = 0.f;
    for (int c = 0; c < C; ++c) {
        const int64_t pc = p0 + (int64_t)c * kH;
        const float wgt = expf(pm[pc] - M);
        acc = fmaf(wgt, pz[pc * kD + k], acc);
        L = fmaf(wgt, pl[pc], L);
    }
    const float zk = acc / L;
    z[((int64_t)n * kH + h) * kD + k] = zk;
    if (k == 0) lse[(int64_t)n * kH + h] = M + logf(L);
    s_xv[h][k] = fmaf(g[k], zk, b[k]);
    block_sync();
#pragma unroll 2
    for (int it = 0; it < kD / kGroups; ++it) {
        const int i = it * kGroups + (t >> 4);
        const float y = row_dot(W + 2 * kD * kD, &s_xv[0][0], kD, i, t & 15);
        if ((t & 15) == 0) ctx[(int64_t)n * kD + i] = y + bias[2 * kD + i];
    }
}

// Backward over one chunk of one frame: dpix of its rows and the partial e[H][d] = sum_j ds_j,h x^_j.
__global__ NO_PACKED_FP32 __launch_bounds__(kThreads) void lava_xattn_bwd_rows_kernel(
    const float* __restrict__ pix, const float* __restrict__ g, const float* __restrict__ u,
    const float* __restrict__ w, const float* __restrict__ fc, const float* __restrict__ lse, float eps, int S, int C,
    float* __restrict__ dpix, float* __restrict__ pe) {
    __shared__ __attribute__((aligned(16))) float s_e[kGroups][kH][kD];
    const int n = blockIdx.x / C, c = blockIdx.x - n * C;
    const int t = threadIdx.x, l = t & 15, gi = t >> 4;
    float gu[kH][8], gw[kH][8];
    {
        float gv[8];
        load_vec(g, l, gv);
#pragma unroll
        for (int h = 0; h < kH; ++h) {
            load_vec(u + ((int64_t)n * kH + h) * kD, l, gu[h]);
            load_vec(w + ((int64_t)n * kH + h) * kD, l, gw[h]);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                gu[h][i] *= gv[i];
                gw[h][i] *= gv[i];
            }
        }
    }
    const float* f = fc + (int64_t)n * kFc;
    // c'_h - lse_h: the row's probability is exp(x^ . (g u_h) + this)
    const float cl[kH] = {f[0] - lse[(int64_t)n * kH], f[1] - lse[(int64_t)n * kH + 1]};
    const float gwz[kH] = {f[2], f[3]}, mgu[kH] = {f[4], f[5]}, mgw[kH] = {f[6], f[7]};
    const float* base = pix + (int64_t)n * S * kD;
    float* dbase = dpix + (int64_t)n * S * kD;
    const int row0 = c * kChunk + gi;
    float e[kH][8];
#pragma unroll
    for (int h = 0; h < kH; ++h)
#pragma unroll
        for (int i = 0; i < 8; ++i) e[h][i] = 0.f;
#pragma unroll
    for (int b0 = 0; b0 < kRowsPerGroup; b0 += kBatch) {
        float x[kBatch][8];
#pragma unroll
        for (int j = 0; j < kBatch; ++j)
            load_vec(base + (int64_t)min(row0 + (b0 + j) * kGroups, S - 1) * kD, l, x[j]);
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const int r = row0 + (b0 + j) * kGroups;
            if (r < S) {
                const float rstd = normalise(x[j], eps);
                float a[kH], ds[kH], m1 = 0.f, m2 = 0.f;
#pragma unroll
                for (int h = 0; h < kH; ++h) {
                    const float sp = row_sum16(dot8(x[j], gu[h]));
                    const float th = row_sum16(dot8(x[j], gw[h]));
                    a[h] = expf(sp + cl[h]);
                    ds[h] = a[h] * (th - gwz[h]);
                    m1 = fmaf(a[h], mgw[h], fmaf(ds[h], mgu[h], m1));
                    m2 = fmaf(a[h], th, fmaf(ds[h], sp, m2));
                }
                m2 *= kInvD;
                float dx[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float dxh = fmaf(a[0], gw[0][i], fmaf(ds[0], gu[0][i], fmaf(a[1], gw[1][i], ds[1] * gu[1][i])));
                    dx[i] = rstd * (dxh - m1 - x[j][i] * m2);
                    e[0][i] = fmaf(ds[0], x[j][i], e[0][i]);
                    e[1][i] = fmaf(ds[1], x[j][i], e[1][i]);
                }
                store_vec(dbase + (int64_t)r * kD, l, dx);
            }
        }
    }
#pragma unroll
    for (int h = 0; h < kH; ++h) store_vec(s_e[gi][h], l, e[h]);
    block_sync();
    const int h = t >> 7, k = t & 127;
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < kGroups; ++r) acc += s_e[r][h][k];
    pe[((int64_t)blockIdx.x * kH + h) * kD + k] = acc;
}

// One workgroup per frame: e = the chunk partials in chunk order; dQ_h = scale W_k,h (g e_h); dq = W_q^T dQ.
__global__ NO_PACKED_FP32 __launch_bounds__(kThreads) void lava_xattn_bwd_combine_kernel(
    const float* __restrict__ pe, int C, const float* __restrict__ g, const float* __restrict__ W,
    float* __restrict__ e, float* __restrict__ dQ, float* __restrict__ dq) {
    __shared__ __attribute__((aligned(16))) float s_du[kH][kD];
    __shared__ __attribute__((aligned(16))) float s_dQ[kD];
    const int n = blockIdx.x, t = threadIdx.x, h = t >> 7, k = t & 127;
    float acc = 0.f;
    for (int c = 0; c < C; ++c) acc += pe[(((int64_t)n * C + c) * kH + h) * kD + k];
    e[((int64_t)n * kH + h) * kD + k] = acc;
    s_du[h][k] = g[k] * acc;
    block_sync();
#pragma unroll 2
    for (int it = 0; it < kD / kGroups; ++it) {
        const int i = it * kGroups + (t >> 4);
        const float v = kScale * row_dot(W + kD * kD, &s_du[0][0], kD, i, t & 15);
        if ((t & 15) == 0) {
            s_dQ[i] = v;
            dQ[(int64_t)n * kD + i] = v;
        }
    }
    block_sync();
    if (t < kD) {
        float a0 = 0.f;
#pragma unroll 8
        for (int i = 0; i < kD; ++i) a0 = fmaf(W[(int64_t)i * kD + t], s_dQ[i], a0);
        dq[(int64_t)n * kD + t] = a0;
    }
}

bool bad_shape(int64_t N, int64_t S) {
    return N < 1 || S < 1 || S > INT32_MAX - kChunk || N * ((S + kChunk - 1) / kChunk) > INT32_MAX;
}

}  // namespace

extern "C" int rt1_lava_xattn_supported(int d, int H) { return d == kD && H == kH; }

extern "C" int64_t rt1_lava_xattn_chunks(int64_t S) { return S < 1 ? 0 : (S + kChunk - 1) / kChunk; }

extern "C" int rt1_lava_xattn_fwd(const float* pix, const float* q, const float* g, const float* b, float eps,
                                  const float* W, const float* bias, int64_t N, int64_t S, float* Q, float* u,
                                  float* fc, float* pm, float* pl, float* pz, float* z, float* lse, float* ctx,
                                  hipStream_t stream) {
    if (pix == nullptr || q == nullptr || g == nullptr || b == nullptr || W == nullptr || bias == nullptr ||
        Q == nullptr || u == nullptr || fc == nullptr || pm == nullptr || pl == nullptr || pz == nullptr ||
        z == nullptr || lse == nullptr || ctx == nullptr || bad_shape(N, S))
        return (int)hipErrorInvalidValue;
    const int C = (int)rt1_lava_xattn_chunks(S);
    hipLaunchKernelGGL(lava_xattn_prologue_kernel<false>, dim3((unsigned)N), dim3(kThreads), 0, stream, q, nullptr,
                       nullptr, g, b, W, bias, Q, u, nullptr, fc);
    hipLaunchKernelGGL(lava_xattn_fwd_rows_kernel, dim3((unsigned)(N * C)), dim3(kThreads), 0, stream, pix, g, u, fc,
                       eps, (int)S, C, pm, pl, pz);
    hipLaunchKernelGGL(lava_xattn_fwd_combine_kernel, dim3((unsigned)N), dim3(kThreads), 0, stream, pm, pl, pz, C, g,
                       b, W, bias, z, lse, ctx);
    return (int)hipGetLastError();
}

extern "C" int rt1_lava_xattn_bwd(const float* dctx, const float* pix, const float* Q, const float* z,
                                  const float* lse, const float* g, const float* b, float eps, const float* W,
                                  const float* bias, int64_t N, int64_t S, float* u, float* w, float* fc, float* pe,
                                  float* dpix, float* e, float* dQ, float* dq, hipStream_t stream) {
    if (dctx == nullptr || pix == nullptr || Q == nullptr || z == nullptr || lse == nullptr || g == nullptr ||
        b == nullptr || W == nullptr || bias == nullptr || u == nullptr || w == nullptr || fc == nullptr ||
        pe == nullptr || dpix == nullptr || e == nullptr || dQ == nullptr || dq == nullptr || bad_shape(N, S))
        return (int)hipErrorInvalidValue;
    const int C = (int)rt1_lava_xattn_chunks(S);
    hipLaunchKernelGGL(lava_xattn_prologue_kernel<true>, dim3((unsigned)N), dim3(kThreads), 0, stream, nullptr, dctx,
                       z, g, b, W, bias, const_cast<float*>(Q), u, w, fc);
    hipLaunchKernelGGL(lava_xattn_bwd_rows_kernel, dim3((unsigned)(N * C)), dim3(kThreads), 0, stream, pix, g, u, w,
                       fc, lse, eps, (int)S, C, dpix, pe);
    hipLaunchKernelGGL(lava_xattn_bwd_combine_kernel, dim3((unsigned)N), dim3(kThreads), 0, stream, pe, C, g, W, e,
                       dQ, dq);
    return (int)hipGetLastError();
}
