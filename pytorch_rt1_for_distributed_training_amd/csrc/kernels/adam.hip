// Fused Adam / AdamW over the flat fp32 parameter buffer (gfx950).
//
// Replaces torch.optim.Adam's per-tensor foreach launches (reference
// distribute_train.py:100): ONE launch updates every trainable
// parameter.  Memory-bound: per element it reads p, g, m, v and writes p, m, v
// (28 B/elem -> 35.2M params = 0.99 GB, ~0.16 ms at 6.3 TB/s).  Loads and
// stores are float4 (16 B/lane), the grid is capped at 8 waves x 256 CUs and
// grid-strides the rest (CDNA guide G11/G13).
//
// The data-parallel 1/world average (grad_scale) and the bias corrections are
// folded in; with weight_decay > 0 the decay is decoupled (AdamW).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace {

struct AdamArgs {
    float lr, beta1, beta2, eps, weight_decay;
    float step_size;      // lr / (1 - beta1^t)
    float inv_sqrt_bc2;   // 1 / sqrt(1 - beta2^t)
    float grad_scale;
};

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamArgs& a) {
    g *= a.grad_scale;
    if (a.weight_decay != 0.f) p *= (1.f - a.lr * a.weight_decay);
    m = fmaf(a.beta1, m, (1.f - a.beta1) * g);
    v = fmaf(a.beta2, v, (1.f - a.beta2) * g * g);
    const float denom = sqrtf(v) * a.inv_sqrt_bc2 + a.eps;
    p -= a.step_size * (m / denom);
}

// Every form of the update is one instantiation of flat_adam_kernel; what is optional is chosen with if constexpr, so a
// form carries no instruction of another and all of them run the same adam_elem on the same operands:
//
//   DEV     {step, lr} are read from the device tensor state (captured-graph replays) and the bias corrections are
//           formed here; without it (the host-argument form, no other flag) AdamArgs arrives complete.
//   CLIP    the verdict of gradnorm.hip's clip_state {norm, coef, ok, skipped, ...} is obeyed: a skipped step (ok == 0)
//           touches nothing -- every workgroup leaves before its first load, the branch is uniform -- and does not
//           advance the bias correction (t = step - skipped steps, as a skipped optimizer.step() under torch's
//           GradScaler); otherwise g = (g * grad_scale) * coef, which with coef == 1 is bit for bit the plain update.
//   EMA     the launch also carries an exponential moving average of the weights: after p, m, v are stored,
//           ema = fma(omd_t, p_new - ema, ema) (36 B/elem instead of 28).  omd is one minus the decay; with warm-up
//           omd_t = max(omd, 9 / (10 + t)), i.e. the decay min(decay, (1 + t) / (10 + t)), where t is the Adam step
//           this call performs.  Lane 0 of workgroup 0 records {omd_t, t, 0, 0} in ema_state with one ordinary vector
//           store; a skipped step writes neither.
//   GROUPS  lr and weight_decay PER ELEMENT.  The flat buffer pads every parameter to 64 floats, so a 64-float chunk
//           belongs to one parameter and with it to one group: chunk_group[n / 64] (uint8, 1/256 B of traffic per
//           element) names the group of each chunk, group_state fp32 [G, 4] = {lr_g, wd_g, 0, 0} holds the groups'
//           constants (G <= 16: 256 B, read straight from global memory -- every wave of the grid reads the same few
//           lines, which stay in the vector L1 / L2).  A lane's float4 i lies in chunk i >> 4, so the 16 lanes of a
//           chunk read one table byte and one float4 of constants; a table entry >= G is read as G - 1 (never out of
//           bounds).  state[1] and a.weight_decay are not read, and n is a multiple of 64: there is no scalar tail.
template <bool DEV, bool CLIP, bool EMA, bool GROUPS>
__global__ __launch_bounds__(256) void flat_adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v,
                                                        float* __restrict__ ema, int64_t n4, int64_t n, AdamArgs a,
                                                        const float* __restrict__ state,
                                                        const float* __restrict__ clip_state,
                                                        float* __restrict__ ema_state, float omd, int warmup,
                                                        const float4* __restrict__ group_state,
                                                        const uint8_t* __restrict__ chunk_group, int G) {
    static_assert(DEV || !(CLIP || EMA || GROUPS), "the host-argument form has no options");
    float gs = 1.f, bc1 = 1.f, omd_t = 0.f;
    if constexpr (DEV) {
        float t = state[0];
        if constexpr (CLIP) {
            if (clip_state[2] == 0.f) return;
            gs = a.grad_scale;
            a.grad_scale = clip_state[1];  // adam_elem's own multiply applies the clip coefficient second
            t -= clip_state[3];
        }
        bc1 = -expm1f(t * logf(a.beta1));                        // 1 - beta^t without cancellation
        a.inv_sqrt_bc2 = rsqrtf(-expm1f(t * logf(a.beta2)));
        if constexpr (!GROUPS) {
            a.lr = state[1];
            a.step_size = a.lr / bc1;
        }
        if constexpr (EMA) {
            omd_t = warmup ? fmaxf(omd, 9.f / (10.f + t)) : omd;
            if (blockIdx.x == 0 && threadIdx.x == 0)
                *reinterpret_cast<float4*>(ema_state) = make_float4(omd_t, t, 0.f, 0.f);
        }
    }
    auto elem = [&](float& pp, float gg, float& mm, float& vv) { adam_elem(pp, CLIP ? gg * gs : gg, mm, vv, a); };
    auto avg = [&](float& ee, float pp) { ee = fmaf(omd_t, pp - ee, ee); };
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    float4* e4 = reinterpret_cast<float4*>(ema);
    for (int64_t i = i0; i < n4; i += stride) {
        if constexpr (GROUPS) {
            const float4 gc = group_state[min((int)chunk_group[i >> 4], G - 1)];
            a.lr = gc.x;
            a.weight_decay = gc.y;
            a.step_size = gc.x / bc1;
        }
        float4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i];
        elem(pp.x, gg.x, mm.x, vv.x);
        elem(pp.y, gg.y, mm.y, vv.y);
        elem(pp.z, gg.z, mm.z, vv.z);
        elem(pp.w, gg.w, mm.w, vv.w);
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
        if constexpr (EMA) {
            float4 ee = e4[i];
            avg(ee.x, pp.x);
            avg(ee.y, pp.y);
            avg(ee.z, pp.z);
            avg(ee.w, pp.w);
            e4[i] = ee;
        }
    }
    if constexpr (!GROUPS) {   // scalar tail (flat buffers are 64-element aligned, so normally empty)
        for (int64_t j = n4 * 4 + i0; j < n; j += stride) {
            float pp = p[j], mm = m[j], vv = v[j];
            elem(pp, g[j], mm, vv);
            p[j] = pp; m[j] = mm; v[j] = vv;
            if constexpr (EMA) {
                float ee = ema[j];
                avg(ee, pp);
                ema[j] = ee;
            }
        }
    }
}

using Kernel = decltype(&flat_adam_kernel<false, false, false, false>);

template <bool GROUPS>
Kernel dev_kernel(bool clip, bool avg) {
    return clip ? (avg ? flat_adam_kernel<true, true, true, GROUPS> : flat_adam_kernel<true, true, false, GROUPS>)
                : (avg ? flat_adam_kernel<true, false, true, GROUPS> : flat_adam_kernel<true, false, false, GROUPS>);
}

// the grid is capped at 8 workgroups x 256 CUs and is never empty
int launch(Kernel kernel, hipStream_t stream, float* p, const float* g, float* m, float* v, float* ema, int64_t n,
           const AdamArgs& a, const float* state, const float* clip_state, float* ema_state, float omd, int warmup,
           const float* group_state, const uint8_t* chunk_group, int G) {
    const int64_t n4 = n / 4;
    const int64_t blocks = std::min<int64_t>(std::max<int64_t>((n4 + 255) / 256, 1), 2048);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p, g, m, v, ema, n4, n, a, state,
                       clip_state, ema_state, omd, warmup, reinterpret_cast<const float4*>(group_state), chunk_group,
                       G);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int rt1_flat_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, float step_size, float inv_sqrt_bc2,
                             float grad_scale, hipStream_t stream) {
    const AdamArgs a{lr, beta1, beta2, eps, weight_decay, step_size, inv_sqrt_bc2, grad_scale};
    return launch(flat_adam_kernel<false, false, false, false>, stream, p, g, m, v, nullptr, n, a, nullptr, nullptr,
                  nullptr, 0.f, 0, nullptr, nullptr, 0);
}

// The device-state forms.  clip_state == nullptr: no verdict to obey; ema == nullptr: no average (ema_state unused);
// group_state == chunk_group == nullptr: one group, lr from state[1] and weight_decay from the argument; with groups
// n % 64 == 0, 1 <= G <= 16, and state[1] and weight_decay are not read.
extern "C" int rt1_flat_adam_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* state,
                                 const float* clip_state, float* ema, float* ema_state, const float* group_state,
                                 const uint8_t* chunk_group, int G, float beta1, float beta2, float eps,
                                 float weight_decay, float grad_scale, float one_minus_decay, int warmup,
                                 hipStream_t stream) {
    const bool groups = group_state != nullptr, clip = clip_state != nullptr, avg = ema != nullptr;
    if (state == nullptr || (avg && ema_state == nullptr) || groups != (chunk_group != nullptr) ||
        (groups && (n <= 0 || n % 64 != 0 || G < 1 || G > 16)))
        return (int)hipErrorInvalidValue;
    const AdamArgs a{0.f, beta1, beta2, eps, weight_decay, 0.f, 1.f, grad_scale};
    return launch(groups ? dev_kernel<true>(clip, avg) : dev_kernel<false>(clip, avg), stream, p, g, m, v, ema, n, a,
                  state, clip_state, ema_state, one_minus_decay, warmup, group_state, chunk_group, G);
}

