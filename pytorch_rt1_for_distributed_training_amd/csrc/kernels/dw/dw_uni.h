// Device helpers of the unified backward kernels (dw_bwd_s1.hip, dw_bwd_s2.hip) only: a thread's CPT channels of one
// pixel as a vector type, the register-pressure pins of the strip loop, and the strip centres' BN1 + SiLU.
#pragma once
#include "dw_stage.h"

namespace rt1 {
namespace dw {

template <int CPT> struct ChanVec;
template <> struct ChanVec<8> {
    typedef uint4 T;
    static __device__ __forceinline__ void unpack(const T u, f2 (&f)[4]) { unpack4x2(u, f); }
    static __device__ __forceinline__ T zero() { return make_uint4(0, 0, 0, 0); }
    static __device__ __forceinline__ T pack(const f2 (&f)[4]) {
        return make_uint4(pack2(f[0].x, f[0].y), pack2(f[1].x, f[1].y), pack2(f[2].x, f[2].y), pack2(f[3].x, f[3].y));
    }
    static __device__ __forceinline__ void loadf(const float* __restrict__ p, f2 (&o)[4]) { load4x2(p, o); }
};
template <> struct ChanVec<4> {
    typedef uint2 T;
    static __device__ __forceinline__ void unpack(const T u, f2 (&f)[2]) {
#if RT1_DW_TIMING & 1   // timing-only build: the bf16 -> f32 unpack of the strip loop removed (values wrong)
        f[0] = f2{__uint_as_float(u.x), __uint_as_float(u.y)};
        f[1] = f2{__uint_as_float(u.y), __uint_as_float(u.x)};
#else
        f[0] = f2{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u)};
        f[1] = f2{__uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
#endif
    }
    static __device__ __forceinline__ T zero() { return make_uint2(0, 0); }
    static __device__ __forceinline__ T pack(const f2 (&f)[2]) {
        return make_uint2(pack2(f[0].x, f[0].y), pack2(f[1].x, f[1].y));
    }
    static __device__ __forceinline__ void loadf(const float* __restrict__ p, f2 (&o)[2]) {
        const float4 a = *reinterpret_cast<const float4*>(p);
        o[0] = f2{a.x, a.y};
        o[1] = f2{a.z, a.w};
    }
};

template <> struct ChanVec<2> {   // 2 channels per thread (k5 at higher occupancy: 25 x 2 weight accumulators)
    typedef uint32_t T;
    static __device__ __forceinline__ void unpack(const T u, f2 (&f)[1]) {
        f[0] = f2{__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)};
    }
    static __device__ __forceinline__ T zero() { return 0u; }
    static __device__ __forceinline__ T pack(const f2 (&f)[1]) { return pack2(f[0].x, f[0].y); }
    static __device__ __forceinline__ void loadf(const float* __restrict__ p, f2 (&o)[1]) {
        const float2 a = *reinterpret_cast<const float2*>(p);
        o[0] = f2{a.x, a.y};
    }
};

constexpr int DWU_SU = 4;     // dy pixels in flight per thread while staging (2: -4 %, 6 / 8 spill; profiles/r2_dw_uni_su_ab.log)
// An offset the compiler cannot see through: keeps loop-invariant LDS reads (weights, BN constants) inside the
// strip loop.  Hoisted, the 25 x 4 weights of a k5 thread alone took 100 VGPRs and the kernel spilled.
__device__ __forceinline__ int opaque(int x) {
    asm volatile("" : "+v"(x));
    return x;
}
__device__ __forceinline__ void pin(f2& v) { asm volatile("" : "+v"(v)); }

// Strip centres' BN1 + SiLU for the unified backward kernels: z = y * sc + sh, a = silu(z) (zero where !ok: no weight
// contribution past the right edge), gp = silu'(z) = s (1 + z (1 - s)).  Written phase by phase over all R x NV channel
// pairs so that each packed op has independent ones between it and its producer: computed pair by pair, the chain's
// back-to-back dependent packed-fp32 ops each cost an s_nop (as in stage_dy; profiles/r6_dw_phased_ab.log).
template <int R, int NV>
__device__ __forceinline__ void centre_silu(const f2 (&y)[R][NV], const f2 (&sc)[NV], const f2 (&sh)[NV],
                                            const bool (&ok)[R], f2 (&a)[R][NV], f2 (&gp)[R][NV]) {
    const f2 one = f2{1.f, 1.f};
    f2 z[R][NV], t[R][NV];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < NV; ++j) z[r][j] = y[r][j] * sc[j] + sh[j];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < NV; ++j) t[r][j] = z[r][j] * f2{-1.4426950408889634f, -1.4426950408889634f};
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < NV; ++j)
            t[r][j] = f2{__builtin_amdgcn_exp2f(t[r][j].x), __builtin_amdgcn_exp2f(t[r][j].y)} + one;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < NV; ++j) t[r][j] = f2{__builtin_amdgcn_rcpf(t[r][j].x), __builtin_amdgcn_rcpf(t[r][j].y)};
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            a[r][j] = ok[r] ? z[r][j] * t[r][j] : f2{0.f, 0.f};
            gp[r][j] = one - t[r][j];
        }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < NV; ++j) gp[r][j] = z[r][j] * gp[r][j] + one;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < NV; ++j) gp[r][j] = t[r][j] * gp[r][j];
}

}  // namespace dw
}  // namespace rt1
