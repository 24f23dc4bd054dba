// Tail of PixelLangMSE's language-conditioned encoder (gfx950, wave64): from the last gated conv stage's output
// y4 [N, P, 256] (NHWC bf16, P = hp * wp pooled pixels) to the encoder's output row,
//   m = mean_p y4,  r = relu(m * gate),  out = LayerNorm(r) (eps inside the square root),
// one launch forward and one launch backward, fp32 throughout.  C = 256 = one channel per lane of a 256-lane workgroup.
//
// Work split.  One workgroup per frame.  The pixel sum reads y4 as 16-byte vectors: 32 channel vectors x 8 pixel lanes,
// four loads in flight per lane (a serial chain over P would be latency-bound), fp32 sums, the 8 pixel lanes combined
// through LDS in a fixed order.  From there lane c owns channel c; the LayerNorm sums are wave sums combined across
// the four waves in a fixed order (two passes: mean, then the centred second moment).
//
// Backward.  LayerNorm backward with the same workgroup sums, the ReLU mask from m * gate > 0, dgate = d * m,
// dm = d * gate, and dy4[n, p, :] = bf16(dm / P) for every pixel, written as 16-byte vectors from an LDS copy of the
// row.  dgamma / dbeta leave as per-frame rows [N][2][256]; a second small kernel adds them over N on four chains
// combined in a fixed order.  No atomics: every output is a bitwise function of the inputs.
//
// Built without packed fp32 like the other LAVA kernels (common.h NO_PACKED_FP32).
#include "common.h"

using namespace rt1;

namespace {

constexpr int BLOCK = 256;
constexpr int kC = 256;                           // channels = lanes
constexpr int kPL = 8;                            // pixel lanes of the mean
constexpr int kInFlight = 4;                      // 16-byte loads in flight per lane

__device__ __forceinline__ void block_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// sum over the 256 lanes, the same value in every lane; s4 is 4 floats of LDS, free again on return
__device__ __forceinline__ float block_sum(float v, float* s4, int t) {
    v = wave_sum(v);
    block_sync();
    if ((t & 63) == 0) s4[t >> 6] = v;
    block_sync();
    return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

__global__ NO_PACKED_FP32 __launch_bounds__(BLOCK) void lava_pixel_tail_fwd_kernel(
    const bf16_t* __restrict__ y4, const float* __restrict__ gate, const float* __restrict__ lnw,
    const float* __restrict__ lnb, float eps, int P, float* __restrict__ out, float* __restrict__ mean,
    float* __restrict__ stat) {
    __shared__ float red[kPL][kC];
    __shared__ float s4[4];
    const int t = threadIdx.x, cv = t & 31, pl = t >> 5;
    const int64_t n = blockIdx.x;
    const bf16_t* src = y4 + n * P * kC + cv * 8;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int p0 = pl; p0 < P; p0 += kPL * kInFlight) {
        uint4 v[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            const int p = p0 + kPL * u;
            v[u] = make_uint4(0, 0, 0, 0);
            if (p < P) v[u] = *reinterpret_cast<const uint4*>(src + (int64_t)p * kC);
        }
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            float f[8];
            unpack8(v[u], f);
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += f[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[pl][cv * 8 + e] = s[e];
    block_sync();
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < kPL; ++r) sum += red[r][t];
    const float m = sum / (float)P;
    const float r = fmaxf(m * gate[n * kC + t], 0.f);
    const float mu = block_sum(r, s4, t) / (float)kC;
    const float d = r - mu;
    const float var = block_sum(d * d, s4, t) / (float)kC;
    const float rstd = 1.f / sqrtf(var + eps);
    out[n * kC + t] = d * rstd * lnw[t] + lnb[t];
    mean[n * kC + t] = m;
    if (t == 0) {
        stat[n * 2] = mu;
        stat[n * 2 + 1] = rstd;
    }
}

__global__ NO_PACKED_FP32 __launch_bounds__(BLOCK) void lava_pixel_tail_bwd_kernel(
    const float* __restrict__ dout, const float* __restrict__ mean, const float* __restrict__ stat,
    const float* __restrict__ gate, const float* __restrict__ lnw, int P, bf16_t* __restrict__ dy4,
    float* __restrict__ dgate, float* __restrict__ rows) {
    __shared__ __attribute__((aligned(16))) bf16_t drow[kC];
    __shared__ float s4[4];
    const int t = threadIdx.x;
    const int64_t n = blockIdx.x;
    const float m = mean[n * kC + t], g = gate[n * kC + t], mu = stat[n * 2], rstd = stat[n * 2 + 1];
    const float pre = m * g, r = fmaxf(pre, 0.f);
    const float xhat = (r - mu) * rstd, go = dout[n * kC + t], dxh = go * lnw[t];
    const float s1 = block_sum(dxh, s4, t) / (float)kC;
    const float s2 = block_sum(dxh * xhat, s4, t) / (float)kC;
    const float d = pre > 0.f ? rstd * (dxh - s1 - xhat * s2) : 0.f;
    dgate[n * kC + t] = d * m;
    rows[(n * 2) * kC + t] = go * xhat;
    rows[(n * 2 + 1) * kC + t] = go;
    drow[t] = f2bf(d * g / (float)P);
    block_sync();
    const int cv = t & 31, pl = t >> 5;
    const uint4 v = *reinterpret_cast<const uint4*>(drow + cv * 8);
    bf16_t* dst = dy4 + n * P * kC + cv * 8;
    for (int p = pl; p < P; p += kPL) *reinterpret_cast<uint4*>(dst + (int64_t)p * kC) = v;
}

// rows [N][2 * 256] -> dgamma | dbeta [2 * 256]: four interleaved chains over N, combined in a fixed order
__global__ NO_PACKED_FP32 __launch_bounds__(BLOCK) void lava_pixel_tail_colsum_kernel(
    const float* __restrict__ rows, int64_t N, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * BLOCK + threadIdx.x;            // < 2 * kC
    const float* src = rows + c;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int64_t n = 0;
    for (; n + 3 < N; n += 4) {
        a0 += src[n * 2 * kC];
        a1 += src[(n + 1) * 2 * kC];
        a2 += src[(n + 2) * 2 * kC];
        a3 += src[(n + 3) * 2 * kC];
    }
    for (; n < N; ++n) a0 += src[n * 2 * kC];
    const float v = (a0 + a1) + (a2 + a3);
    if (c < kC) dgamma[c] = v;
    else dbeta[c - kC] = v;
}

bool shape_ok(int64_t N, int64_t P) { return N >= 1 && N <= INT32_MAX && P >= 1 && P <= INT32_MAX; }

}  // namespace

extern "C" int rt1_lava_pixel_tail_supported(int channels) { return channels == kC ? 1 : 0; }

// y4 bf16 [N, P, 256], gate fp32 [N, 256], LayerNorm weight / bias fp32 [256] -> out fp32 [N, 256]; mean fp32
// [N, 256] and stat fp32 [N, 2] = (mu, rstd) are what the backward reads
extern "C" int rt1_lava_pixel_tail_fwd(const uint16_t* y4, const float* gate, const float* lnw, const float* lnb,
                                       float eps, int64_t N, int64_t P, float* out, float* mean, float* stat,
                                       hipStream_t stream) {
    if (y4 == nullptr || gate == nullptr || lnw == nullptr || lnb == nullptr || out == nullptr || mean == nullptr ||
        stat == nullptr || !shape_ok(N, P))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(lava_pixel_tail_fwd_kernel, dim3((unsigned)N), dim3(BLOCK), 0, stream, y4, gate, lnw, lnb, eps,
                       (int)P, out, mean, stat);
    return (int)hipGetLastError();
}

// dout fp32 [N, 256] -> dy4 bf16 [N, P, 256], dgate fp32 [N, 256], dgamma / dbeta fp32 [256]; rows fp32 [N, 2, 256]
// is a workspace
extern "C" int rt1_lava_pixel_tail_bwd(const float* dout, const float* mean, const float* stat, const float* gate,
                                       const float* lnw, int64_t N, int64_t P, uint16_t* dy4, float* dgate,
                                       float* rows, float* dgamma, float* dbeta, hipStream_t stream) {
    if (dout == nullptr || mean == nullptr || stat == nullptr || gate == nullptr || lnw == nullptr ||
        dy4 == nullptr || dgate == nullptr || rows == nullptr || dgamma == nullptr || dbeta == nullptr ||
        !shape_ok(N, P))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(lava_pixel_tail_bwd_kernel, dim3((unsigned)N), dim3(BLOCK), 0, stream, dout, mean, stat, gate,
                       lnw, (int)P, dy4, dgate, rows);
    hipLaunchKernelGGL(lava_pixel_tail_colsum_kernel, dim3(2 * kC / BLOCK), dim3(BLOCK), 0, stream, rows, N, dgamma,
                       dbeta);
    return (int)hipGetLastError();
}
