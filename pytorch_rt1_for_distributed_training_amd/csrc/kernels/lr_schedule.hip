// Per-step learning-rate schedule (linear warm-up, then constant / linear / cosine / inverse-sqrt decay) formed on the
// device (gfx950), in front of the fused Adam launch of adam.hip.
//
// The Adam kernels read lr from device memory (state[1], group_state[g][0]) so that a captured hipGraph step stays
// valid; this kernel rewrites those slots every step from the groups' BASE learning rates (lr_base, device memory too:
// MultiStepLR changes them between replays) times one factor f(t).  t is the effective Adam step of the update being
// applied -- state[0] after its increment, minus the skipped steps of clip_state -- i.e. the t of the bias corrections
// and of the EMA warm-up, which only the device knows when steps can be skipped.
//
// One workgroup of one wave.  Every lane forms t and f (64 identical evaluations, once per step); lane g < G owns
// group g.  f is evaluated in fp64 with the accurate library cos / sqrt and without contraction, then rounded ONCE to
// fp32, so the host formula (engine.optim.lr_factor, fp64 math) reproduces it to within one fp32 ulp; the products
// lr_base[g] * f are single fp32 multiplies, so they are bitwise what the host gets from the stored factor.
//
//   warm-up (W > 0, t <= W):  f = t / W                         (the first update uses 1 / W, f(W) = 1)
//   after it, q = min(1, (t - W) / (N - W)):
//     constant  f = 1
//     linear    f = 1 - (1 - r) q                               (q >= 1: f = r exactly)
//     cosine    f = r + (1 - r) (1 + cos(pi q)) / 2             (q >= 1: f = r exactly)
//     rsqrt     f = max(r, sqrt(max(W, 1) / t))                 (N unused)
//
// A skipped step (clip_state[2] == 0) leaves before any store, as the Adam kernels do.  All stores are ordinary
// vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

enum { KIND_CONSTANT = 0, KIND_LINEAR = 1, KIND_COSINE = 2, KIND_RSQRT = 3 };

__global__ __launch_bounds__(64) void lr_schedule_kernel(float* state, const float* __restrict__ clip_state,
                                                         const float* __restrict__ lr_base, float* group_state,
                                                         float* sched_state, int G, int kind, double W, double N,
                                                         double r) {
#pragma clang fp contract(off)
    if (clip_state != nullptr && clip_state[2] == 0.f) return;
    float tf = state[0];
    if (clip_state != nullptr) tf -= clip_state[3];
    const double t = fmax((double)tf, 1.0);      // t >= 1 by construction; never divide by 0
    double f;
    if (W > 0.0 && t <= W) {
        f = t / W;
    } else if (kind == KIND_CONSTANT) {
        f = 1.0;
    } else if (kind == KIND_RSQRT) {
        f = fmax(r, sqrt(fmax(W, 1.0) / t));
    } else {
        const double q = (t - W) / (N - W);
        if (q >= 1.0)
            f = r;
        else if (kind == KIND_LINEAR)
            f = 1.0 - (1.0 - r) * q;
        else
            f = r + (1.0 - r) * (1.0 + cos(3.141592653589793 * q)) * 0.5;
    }
    const float ff = (float)f;
    const int g = threadIdx.x;
    if (g == 0) {
        state[1] = lr_base[0] * ff;
        *reinterpret_cast<float4*>(sched_state) = make_float4(ff, (float)t, 0.f, 0.f);
    }
    if (group_state != nullptr && g < G) group_state[4 * g] = lr_base[g] * ff;
}

}  // namespace

// state fp32[>= 2] = {step, lr}; lr_base fp32[G], 1 <= G <= 16; group_state fp32[G, 4] or nullptr; sched_state fp32[4],
// 16-byte aligned; clip_state fp32[8] or nullptr.  kind 0..3 = constant, linear, cosine, rsqrt; warmup >= 0;
// decay > warmup for linear and cosine; 0 <= min_ratio <= 1.
extern "C" int rt1_lr_schedule_dev(float* state, const float* clip_state, const float* lr_base, float* group_state,
                                   float* sched_state, int G, int kind, int64_t warmup, int64_t decay,
                                   double min_ratio, hipStream_t stream) {
    if (state == nullptr || lr_base == nullptr || sched_state == nullptr || G < 1 || G > 16 || kind < KIND_CONSTANT ||
        kind > KIND_RSQRT || warmup < 0 || !(min_ratio >= 0.0 && min_ratio <= 1.0) ||
        ((kind == KIND_LINEAR || kind == KIND_COSINE) && decay <= warmup))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(64), 0, stream, state, clip_state, lr_base, group_state,
                       sched_state, G, kind, (double)warmup, (double)decay, min_ratio);
    return (int)hipGetLastError();
}
