// Global gradient norm, clip coefficient / non-finite verdict, and the BN-buffer guard (gfx950).
//
// The training step is one captured hipGraph, so gradient clipping and the "skip a non-finite step" decision are
// taken on the device: two launches turn the flat fp32 gradient buffer into a small device-resident `clip_state`
// that the clip variant of the fused Adam (adam.hip) and the buffer guard below obey.
//
//   grad_sumsq     P workgroups x 256 lanes grid-stride over the buffer with 16 B loads, four in flight per lane.
//                  Each lane keeps four fp32 accumulators (one per load slot; at 35.2M parameters a chain is ~17
//                  float4, i.e. ~68 non-negative terms); everything after that is fp64 in a fixed order: the four
//                  accumulators, the lane shuffles (offsets 32..1), the 4 waves through LDS, one fp64 partial per
//                  workgroup.  No atomics: P and therefore the whole summation order depend on n alone
//                  (rt1_gradnorm_partials), so the norm is bitwise reproducible, eager or replayed, on every rank.
//   clip_finalize  one workgroup: lane t sums its contiguous run of partials in index order, lane 0 sums the 256 runs
//                  in index order, then writes clip_state (fp32[8]):
//                    0 norm = grad_scale * sqrt(sum)   1 coef   2 ok   3 skipped steps   4 clipped steps
//                    5 consecutive skipped steps       6, 7 zero
//   buffer_guard   ok ? shadow = buf : buf = shadow -- rolls the BN running statistics of a skipped step back.
//
// Inf and NaN propagate (x*x is +inf for either infinity, NaN stays NaN, nothing here compares or clamps), so a
// single bad element makes the norm non-finite.  The squares are formed in fp32: a finite element of magnitude above
// sqrt(FLT_MAX) ~ 1.8e19 overflows to +inf and the step then counts as non-finite as well.  A gradient of that size
// is not trainable anyway, so this is accepted rather than paying for fp64 squares on the memory-bound path.
//
// Memory-bound: 4n bytes read (141 MB at 35.2M parameters, 22-28 us at 6.3-5 TB/s).
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;          // float4 loads in flight per lane
constexpr int kMaxPartials = 2048;  // the grid cap of flat_adam_kernel: 8 workgroups x 256 CUs

__device__ __forceinline__ float sq4(float acc, const float4 x) {
    acc = fmaf(x.x, x.x, acc);
    acc = fmaf(x.y, x.y, acc);
    acc = fmaf(x.z, x.z, acc);
    return fmaf(x.w, x.w, acc);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;   // lane 0 holds the sum
}

__global__ __launch_bounds__(kThreads) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n4, int64_t n,
                                                              double* __restrict__ partials) {
    __shared__ double wsum[kThreads / 64];
    const float4* g4 = reinterpret_cast<const float4*>(g);
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (; i + (kUnroll - 1) * stride < n4; i += kUnroll * stride) {
        const float4 x0 = g4[i], x1 = g4[i + stride], x2 = g4[i + 2 * stride], x3 = g4[i + 3 * stride];
        a0 = sq4(a0, x0);
        a1 = sq4(a1, x1);
        a2 = sq4(a2, x2);
        a3 = sq4(a3, x3);
    }
    for (; i < n4; i += stride) a0 = sq4(a0, g4[i]);
    double s = (((double)a0 + (double)a1) + (double)a2) + (double)a3;
    // scalar tail (n % 4 elements; flat buffers are 64-element aligned, so normally empty)
    if (blockIdx.x == 0 && n4 * 4 + threadIdx.x < n) {
        const float x = g[n4 * 4 + threadIdx.x];
        s += (double)(x * x);
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ __launch_bounds__(kThreads) void grad_clip_finalize_kernel(const double* __restrict__ partials, int P,
                                                                      float max_norm, float grad_scale,
                                                                      int skip_nonfinite, float* __restrict__ clip_state) {
    __shared__ double runs[kThreads];
    const int per = (P + kThreads - 1) / kThreads;
    double s = 0.0;
    for (int k = 0; k < per; ++k) {
        const int j = (int)threadIdx.x * per + k;
        if (j < P) s += partials[j];
    }
    runs[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum = 0.0;
    for (int t = 0; t < kThreads; ++t) sum += runs[t];
    const float norm = (float)((double)grad_scale * sqrt(sum));
    const bool finite = isfinite(norm);
    float coef = 1.f;
    if (max_norm > 0.f && finite) coef = fminf(1.f, (float)((double)max_norm / ((double)norm + 1e-6)));
    const float ok = (skip_nonfinite && !finite) ? 0.f : 1.f;
    float4* cs = reinterpret_cast<float4*>(clip_state);
    const float4 prev = cs[0];
    const float4 prev2 = cs[1];
    float4 lo, hi;
    lo.x = norm;
    lo.y = coef;
    lo.z = ok;
    lo.w = prev.w + (1.f - ok);
    hi.x = prev2.x + ((ok != 0.f && coef < 1.f) ? 1.f : 0.f);
    hi.y = ok != 0.f ? 0.f : prev2.y + 1.f;
    hi.z = 0.f;
    hi.w = 0.f;
    cs[0] = lo;
    cs[1] = hi;
}

__global__ __launch_bounds__(kThreads) void buffer_guard_kernel(float* __restrict__ buf, float* __restrict__ shadow,
                                                                int64_t n4, int64_t n,
                                                                const float* __restrict__ clip_state) {
    const bool ok = clip_state[2] != 0.f;      // uniform: one verdict per step
    float* dst = ok ? shadow : buf;
    const float* src = ok ? buf : shadow;
    float4* d4 = reinterpret_cast<float4*>(dst);
    const float4* s4 = reinterpret_cast<const float4*>(src);
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += stride) d4[i] = s4[i];
    for (int64_t j = n4 * 4 + (int64_t)blockIdx.x * kThreads + threadIdx.x; j < n; j += stride) dst[j] = src[j];
}

}  // namespace

extern "C" int rt1_gradnorm_partials(int64_t n) {
    if (n <= 0) return 0;
    const int64_t per_block = (int64_t)kThreads * kUnroll * 4;     // floats one workgroup covers per trip
    int64_t blocks = n / per_block + (n % per_block != 0);         // no n + per_block - 1: n may be near INT64_MAX
    if (blocks > kMaxPartials) blocks = kMaxPartials;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

extern "C" int rt1_grad_sumsq(const float* g, int64_t n, double* partials, hipStream_t stream) {
    const int P = rt1_gradnorm_partials(n);
    if (P <= 0 || g == nullptr || partials == nullptr) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)P), dim3(kThreads), 0, stream, g, n / 4, n, partials);
    return (int)hipGetLastError();
}

extern "C" int rt1_grad_clip_finalize(const double* partials, int P, float max_norm, float grad_scale,
                                      int skip_nonfinite, float* clip_state, hipStream_t stream) {
    if (P < 1 || P > kMaxPartials || partials == nullptr || clip_state == nullptr) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(kThreads), 0, stream, partials, P, max_norm,
                       grad_scale, skip_nonfinite, clip_state);
    return (int)hipGetLastError();
}

extern "C" int rt1_buffer_guard(float* buf, float* shadow, int64_t n, const float* clip_state, hipStream_t stream) {
    if (n <= 0 || buf == nullptr || shadow == nullptr || clip_state == nullptr) return (int)hipErrorInvalidValue;
    const int64_t n4 = n / 4;
    int64_t blocks = n4 / kThreads + (n4 % kThreads != 0);
    if (blocks > kMaxPartials) blocks = kMaxPartials;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(buffer_guard_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, buf, shadow, n4, n,
                       clip_state);
    return (int)hipGetLastError();
}
