// Layer-wise trust ratios (LAMB, You et al. 2020) over the flat fp32 parameter buffer (gfx950, wave64).
//
// Adam's update direction of every parameter tensor is rescaled so that its norm is the tensor's own:
//
//   m = fma(beta1, m, (1 - beta1) g')            g' = (g * grad_scale) * clip coefficient, adam.hip's expressions
//   v = fma(beta2, v, (1 - beta2) g' g')
//   u = (m / bc1) / (sqrt(v) * inv_sqrt_bc2 + eps) + wd * p
//   r_i = ||p_i|| / ||u_i||  over tensor i; 1 when either norm is 0 or the tensor is not adapted
//   p = p - (lr * r_i) u                         ema = fma(omd_t, p - ema, ema) when the average is carried
//
// A norm per tensor needs the whole tensor before any of it is updated, so the step is three launches; none reads the
// host, none uses an atomic, and the order of every sum is a function of the buffer layout alone (bitwise reproducible,
// eager or replayed from a hipGraph):
//
//   lamb_moments  reads p, g, m, v (16 B per lane), writes m, v, forms u in registers and leaves one fp32 pair
//                 {sum p^2, sum u^2} per 64-float chunk in chunk_sums [n / 64, 2].  The flat buffer pads every tensor
//                 to 64 floats, so a chunk -- the 16 lanes of one DPP row -- lies inside one tensor.  A lane adds its
//                 four squares in element order; the row adds its 16 lanes by four DPP exchanges (quad xor 1, quad xor
//                 2, half-row mirror, row mirror), a fixed butterfly that leaves the same bits in all 16 lanes.  g is
//                 not modified and u is never stored.  24 B/elem.
//   lamb_trust    one workgroup per tensor: lane k sums a contiguous run of the tensor's chunk pairs in index order in
//                 fp64, lane 0 sums the 256 runs in index order (as grad_clip_finalize does), then trust[i] and
//                 norms[i] = {||p||, ||u||}.  8 B per 64 elements read; microseconds.
//   lamb_apply    reads p, m, v (and ema), forms u again with lamb_u -- the device function lamb_moments used, on the
//                 same m, v, p bits, so the u that is applied is the u that was measured -- looks up the tensor of its
//                 chunk and writes p (and ema; ema_state as adam.hip records it).  16 B/elem, 24 with the average.
//                 The lookup is a uint16 entry per chunk (chunk_tensor, 1/128 B per element).
//
// 40 B/elem (48 with the average) against Adam's 28 (36).  The forms {CLIP, EMA, GROUPS} are those of flat_adam_kernel
// and are chosen with if constexpr; a skipped step (clip_state[2] == 0) leaves every workgroup of all three kernels
// after that one load, before any other.  n is a multiple of 64 (no scalar tail) and every table entry is clamped where it is used as an
// index, so no table content can make a kernel read outside its buffers; no store is indexed by table content.
//
// lamb_apply is built without packed fp32 (common.h NO_PACKED_FP32): the compiler otherwise packs its four updates as
// v_pk_fma_f32 with a high-element op_sel, a form this project does not ship (tools/isa_audit.py).  A kernel with that
// attribute inlines only always_inline callees -- a lambda or make_float4 becomes a call with scratch -- so its body
// calls nothing but __forceinline__ functions.  lamb_moments has no such instruction and keeps the default target.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; 256 lanes per workgroup; scratch 0, no call and
// occupancy 8 waves per SIMD in every instantiation):
//   lamb_moments<CLIP, GROUPS>              55-56 VGPRs, no LDS
//   lamb_trust<CLIP>                        60 VGPRs, 4096 B LDS (the fp64 runs)
//   lamb_apply<CLIP, EMA, GROUPS>           57-60 VGPRs, no LDS
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;    // the grid cap of flat_adam_kernel: 8 workgroups x 256 CUs

struct LambArgs {
    float beta1, beta2, eps, weight_decay, grad_scale;
};

// bias corrections of the Adam step t, as flat_adam_kernel<DEV> forms them
struct Corrections {
    float bc1, inv_sqrt_bc2;
};

__device__ __forceinline__ Corrections corrections(float t, float beta1, float beta2) {
    Corrections c;
    c.bc1 = -expm1f(t * logf(beta1));                         // 1 - beta^t without cancellation
    c.inv_sqrt_bc2 = rsqrtf(-expm1f(t * logf(beta2)));
    return c;
}

// The update direction of one element.  Both kernels that need it call this one function, and every operation in it
// is spelled out (no expression the compiler could contract one way here and another way there).
__device__ __forceinline__ float lamb_u(float p, float m, float v, float wd, float eps, const Corrections& c) {
    const float denom = fmaf(sqrtf(v), c.inv_sqrt_bc2, eps);
    return fmaf(wd, p, (m / c.bc1) / denom);
}

template <int CTRL>
__device__ __forceinline__ float dpp(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}

// sum over the 16 lanes of a DPP row in a fixed order; every lane of the row ends with the same bits
__device__ __forceinline__ float row_sum16(float x) {
    x += dpp<0xB1>(x);     // quad_perm [1, 0, 3, 2]: lane ^ 1
    x += dpp<0x4E>(x);     // quad_perm [2, 3, 0, 1]: lane ^ 2
    x += dpp<0x141>(x);    // row_half_mirror: the other quad of the half row
    x += dpp<0x140>(x);    // row_mirror: the other half row
    return x;
}

template <bool CLIP, bool GROUPS>
__global__ __launch_bounds__(kThreads) void lamb_moments_kernel(const float* __restrict__ p,
                                                                const float* __restrict__ g, float* __restrict__ m,
                                                                float* __restrict__ v, int64_t n4, LambArgs a,
                                                                const float* __restrict__ state,
                                                                const float* __restrict__ clip_state,
                                                                const float4* __restrict__ group_state,
                                                                const uint8_t* __restrict__ chunk_group, int G,
                                                                float2* __restrict__ chunk_sums) {
    if constexpr (CLIP) {
        if (clip_state[2] == 0.f) return;
    }
    float t = state[0];
    float gs = 1.f;
    if constexpr (CLIP) {
        gs = a.grad_scale;
        a.grad_scale = clip_state[1];      // applied second, as in flat_adam_kernel
        t -= clip_state[3];
    }
    const Corrections c = corrections(t, a.beta1, a.beta2);
    float wd = a.weight_decay;
    auto elem = [&](float pp, float gg, float& mm, float& vv) -> float {
        if constexpr (CLIP) gg *= gs;
        gg *= a.grad_scale;
        mm = fmaf(a.beta1, mm, (1.f - a.beta1) * gg);
        vv = fmaf(a.beta2, vv, (1.f - a.beta2) * gg * gg);
        return lamb_u(pp, mm, vv, wd, a.eps, c);
    };
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    const float4* p4 = reinterpret_cast<const float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    // n4 and the stride are multiples of 16 and a row starts at a multiple of 16: the 16 lanes of a row run the same
    // trips, so the row exchange below never reads a lane that has left the loop
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += stride) {
        if constexpr (GROUPS) wd = group_state[min((int)chunk_group[i >> 4], G - 1)].y;
        const float4 pp = p4[i], gg = g4[i];
        float4 mm = m4[i], vv = v4[i];
        const float ux = elem(pp.x, gg.x, mm.x, vv.x);
        const float uy = elem(pp.y, gg.y, mm.y, vv.y);
        const float uz = elem(pp.z, gg.z, mm.z, vv.z);
        const float uw = elem(pp.w, gg.w, mm.w, vv.w);
        m4[i] = mm; v4[i] = vv;
        float sp = fmaf(pp.w, pp.w, fmaf(pp.z, pp.z, fmaf(pp.y, pp.y, pp.x * pp.x)));
        float su = fmaf(uw, uw, fmaf(uz, uz, fmaf(uy, uy, ux * ux)));
        sp = row_sum16(sp);
        su = row_sum16(su);
        if ((threadIdx.x & 15) == 0) chunk_sums[i >> 4] = make_float2(sp, su);
    }
}

template <bool CLIP>
__global__ __launch_bounds__(kThreads) void lamb_trust_kernel(const float2* __restrict__ chunk_sums, int C,
                                                              const int32_t* __restrict__ tensor_chunk_start,
                                                              const uint8_t* __restrict__ tensor_adapt,
                                                              const float* __restrict__ clip_state,
                                                              float* __restrict__ trust, float2* __restrict__ norms) {
    __shared__ double runs_p[kThreads];
    __shared__ double runs_u[kThreads];
    if constexpr (CLIP) {
        if (clip_state[2] == 0.f) return;
    }
    const int i = blockIdx.x;
    const int c0 = min(max(tensor_chunk_start[i], 0), C);
    const int c1 = min(max(tensor_chunk_start[i + 1], c0), C);
    const int per = (c1 - c0 + kThreads - 1) / kThreads;
    double sp = 0.0, su = 0.0;
    for (int k = 0; k < per; ++k) {
        const int64_t j = (int64_t)c0 + (int64_t)threadIdx.x * per + k;
        if (j < c1) {
            const float2 s = chunk_sums[j];
            sp += (double)s.x;
            su += (double)s.y;
        }
    }
    runs_p[threadIdx.x] = sp;
    runs_u[threadIdx.x] = su;
    __syncthreads();
    if (threadIdx.x != 0) return;
    sp = 0.0;
    su = 0.0;
    for (int k = 0; k < kThreads; ++k) {
        sp += runs_p[k];
        su += runs_u[k];
    }
    const double np = sqrt(sp), nu = sqrt(su);
    float r = 1.f;
    if (tensor_adapt[i] != 0 && np > 0.0 && nu > 0.0) r = (float)(np / nu);
    trust[i] = r;
    norms[i] = make_float2((float)np, (float)nu);
}

template <bool CLIP, bool EMA, bool GROUPS>
__global__ NO_PACKED_FP32 __launch_bounds__(kThreads) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m,
                                                              const float* __restrict__ v, float* __restrict__ ema,
                                                              int64_t n4, LambArgs a, const float* __restrict__ state,
                                                              const float* __restrict__ clip_state,
                                                              float* __restrict__ ema_state, float omd, int warmup,
                                                              const float4* __restrict__ group_state,
                                                              const uint8_t* __restrict__ chunk_group, int G,
                                                              const float* __restrict__ trust,
                                                              const uint16_t* __restrict__ chunk_tensor, int nT) {
    if constexpr (CLIP) {
        if (clip_state[2] == 0.f) return;
    }
    float t = state[0];
    if constexpr (CLIP) t -= clip_state[3];
    const Corrections c = corrections(t, a.beta1, a.beta2);
    float lr = 0.f, wd = a.weight_decay, omd_t = 0.f;
    if constexpr (!GROUPS) lr = state[1];
    if constexpr (EMA) {
        omd_t = warmup ? fmaxf(omd, 9.f / (10.f + t)) : omd;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            float4 rec;                          // filled by member: under NO_PACKED_FP32 nothing but always_inline
            rec.x = omd_t;                       // functions is inlined into this kernel, make_float4 would be a call
            rec.y = t;
            rec.z = 0.f;
            rec.w = 0.f;
            *reinterpret_cast<float4*>(ema_state) = rec;
        }
    }
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* m4 = reinterpret_cast<const float4*>(m);
    const float4* v4 = reinterpret_cast<const float4*>(v);
    float4* e4 = reinterpret_cast<float4*>(ema);
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += stride) {
        const int64_t chunk = i >> 4;
        if constexpr (GROUPS) {
            const float4 gc = group_state[min((int)chunk_group[chunk], G - 1)];
            lr = gc.x;
            wd = gc.y;
        }
        const float step = lr * trust[min((int)chunk_tensor[chunk], nT - 1)];
        float4 pp = p4[i];
        const float4 mm = m4[i], vv = v4[i];
        pp.x = fmaf(-step, lamb_u(pp.x, mm.x, vv.x, wd, a.eps, c), pp.x);
        pp.y = fmaf(-step, lamb_u(pp.y, mm.y, vv.y, wd, a.eps, c), pp.y);
        pp.z = fmaf(-step, lamb_u(pp.z, mm.z, vv.z, wd, a.eps, c), pp.z);
        pp.w = fmaf(-step, lamb_u(pp.w, mm.w, vv.w, wd, a.eps, c), pp.w);
        p4[i] = pp;
        if constexpr (EMA) {
            float4 ee = e4[i];
            ee.x = fmaf(omd_t, pp.x - ee.x, ee.x);
            ee.y = fmaf(omd_t, pp.y - ee.y, ee.y);
            ee.z = fmaf(omd_t, pp.z - ee.z, ee.z);
            ee.w = fmaf(omd_t, pp.w - ee.w, ee.w);
            e4[i] = ee;
        }
    }
}

unsigned grid_of(int64_t n4) {
    return (unsigned)std::min<int64_t>(std::max<int64_t>((n4 + kThreads - 1) / kThreads, 1), kMaxBlocks);
}

using ApplyKernel = decltype(&lamb_apply_kernel<false, false, false>);

template <bool GROUPS>
ApplyKernel apply_kernel(bool clip, bool avg) {
    return clip ? (avg ? lamb_apply_kernel<true, true, GROUPS> : lamb_apply_kernel<true, false, GROUPS>)
                : (avg ? lamb_apply_kernel<false, true, GROUPS> : lamb_apply_kernel<false, false, GROUPS>);
}

bool bad_layout(int64_t n, bool groups, const void* chunk_group, int G) {
    return n <= 0 || n % 64 != 0 || n / 64 > INT32_MAX || groups != (chunk_group != nullptr) ||
           (groups && (G < 1 || G > 16));
}

}  // namespace

extern "C" int rt1_lamb_moments(const float* p, const float* g, float* m, float* v, int64_t n, const float* state,
                                const float* clip_state, const float* group_state, const uint8_t* chunk_group, int G,
                                float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                float* chunk_sums, hipStream_t stream) {
    const bool groups = group_state != nullptr, clip = clip_state != nullptr;
    if (p == nullptr || g == nullptr || m == nullptr || v == nullptr || state == nullptr || chunk_sums == nullptr ||
        bad_layout(n, groups, chunk_group, G))
        return (int)hipErrorInvalidValue;
    const LambArgs a{beta1, beta2, eps, weight_decay, grad_scale};
    auto kernel = groups ? (clip ? lamb_moments_kernel<true, true> : lamb_moments_kernel<false, true>)
                         : (clip ? lamb_moments_kernel<true, false> : lamb_moments_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(grid_of(n / 4)), dim3(kThreads), 0, stream, p, g, m, v, n / 4, a, state,
                       clip_state, reinterpret_cast<const float4*>(group_state), chunk_group, G,
                       reinterpret_cast<float2*>(chunk_sums));
    return (int)hipGetLastError();
}

extern "C" int rt1_lamb_trust(const float* chunk_sums, int64_t n, const int32_t* tensor_chunk_start,
                              const uint8_t* tensor_adapt, int nT, const float* clip_state, float* trust,
                              float* norms, hipStream_t stream) {
    if (chunk_sums == nullptr || tensor_chunk_start == nullptr || tensor_adapt == nullptr || trust == nullptr ||
        norms == nullptr || nT < 1 || nT > 65535 || bad_layout(n, false, nullptr, 0))
        return (int)hipErrorInvalidValue;
    auto kernel = clip_state != nullptr ? lamb_trust_kernel<true> : lamb_trust_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)nT), dim3(kThreads), 0, stream,
                       reinterpret_cast<const float2*>(chunk_sums), (int)(n / 64), tensor_chunk_start, tensor_adapt,
                       clip_state, trust, reinterpret_cast<float2*>(norms));
    return (int)hipGetLastError();
}

extern "C" int rt1_lamb_apply(float* p, const float* m, const float* v, int64_t n, const float* state,
                              const float* clip_state, float* ema, float* ema_state, const float* group_state,
                              const uint8_t* chunk_group, int G, const float* trust, const uint16_t* chunk_tensor,
                              int nT, float beta1, float beta2, float eps, float weight_decay, float one_minus_decay,
                              int warmup, hipStream_t stream) {
    const bool groups = group_state != nullptr, clip = clip_state != nullptr, avg = ema != nullptr;
    if (p == nullptr || m == nullptr || v == nullptr || state == nullptr || trust == nullptr ||
        chunk_tensor == nullptr || (avg && ema_state == nullptr) || nT < 1 || nT > 65535 ||
        bad_layout(n, groups, chunk_group, G))
        return (int)hipErrorInvalidValue;
    const LambArgs a{beta1, beta2, eps, weight_decay, 1.f};
    ApplyKernel kernel = groups ? apply_kernel<true>(clip, avg) : apply_kernel<false>(clip, avg);
    hipLaunchKernelGGL(kernel, dim3(grid_of(n / 4)), dim3(kThreads), 0, stream, p, m, v, ema, n / 4, a, state,
                       clip_state, ema_state, one_minus_decay, warmup, reinterpret_cast<const float4*>(group_state),
                       chunk_group, G, trust, chunk_tensor, nT);
    return (int)hipGetLastError();
}
