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

__global__ __launch_bounds__(256) void flat_adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v,
                                                        int64_t n4, int64_t n, AdamArgs a,
                                                        const float* __restrict__ state) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    if (state) {   // {step, lr} on the device (captured-graph replays)
        const float t = state[0], lr = state[1];
        a.lr = lr;
        a.step_size = lr / -expm1f(t * logf(a.beta1));          // 1 - beta^t without cancellation
        a.inv_sqrt_bc2 = rsqrtf(-expm1f(t * logf(a.beta2)));
    }
    for (; i < n4; i += stride) {
        float4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i];
        adam_elem(pp.x, gg.x, mm.x, vv.x, a);
        adam_elem(pp.y, gg.y, mm.y, vv.y, a);
        adam_elem(pp.z, gg.z, mm.z, vv.z, a);
        adam_elem(pp.w, gg.w, mm.w, vv.w, a);
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
    }
    // scalar tail (flat buffers are 64-element aligned, so normally empty)
    for (int64_t j = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
        float pp = p[j], mm = m[j], vv = v[j];
        adam_elem(pp, g[j], mm, vv, a);
        p[j] = pp; m[j] = mm; v[j] = vv;
    }
}

// The same update under the verdict of gradnorm.hip's clip_state {norm, coef, ok, skipped, ...}: a skipped step
// (ok == 0) touches nothing -- every workgroup leaves before its first load, the branch is uniform -- and does not
// advance the bias correction (t = step - skipped steps, as a skipped optimizer.step() under torch's GradScaler);
// otherwise g = (g * grad_scale) * coef, which with coef == 1 is bit for bit the update of flat_adam_kernel.
__global__ __launch_bounds__(256) void flat_adam_clip_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                             float* __restrict__ m, float* __restrict__ v,
                                                             int64_t n4, int64_t n, AdamArgs a,
                                                             const float* __restrict__ state,
                                                             const float* __restrict__ clip_state) {
    if (clip_state[2] == 0.f) return;
    const float gs = a.grad_scale;
    a.grad_scale = clip_state[1];      // adam_elem's own multiply applies the clip coefficient second
    {
        const float t = state[0] - clip_state[3], lr = state[1];
        a.lr = lr;
        a.step_size = lr / -expm1f(t * logf(a.beta1));
        a.inv_sqrt_bc2 = rsqrtf(-expm1f(t * logf(a.beta2)));
    }
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    for (; i < n4; i += stride) {
        float4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i];
        adam_elem(pp.x, gg.x * gs, mm.x, vv.x, a);
        adam_elem(pp.y, gg.y * gs, mm.y, vv.y, a);
        adam_elem(pp.z, gg.z * gs, mm.z, vv.z, a);
        adam_elem(pp.w, gg.w * gs, mm.w, vv.w, a);
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
    }
    for (int64_t j = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
        float pp = p[j], mm = m[j], vv = v[j];
        adam_elem(pp, g[j] * gs, mm, vv, a);
        p[j] = pp; m[j] = mm; v[j] = vv;
    }
}

// The device-state update that also carries an exponential moving average of the weights: per float4 it loads
// p, g, m, v, ema, runs adam_elem exactly as flat_adam_kernel (CLIP = false) or flat_adam_clip_kernel (CLIP = true)
// do -- p, m, v come out bit for bit the same -- then ema = fma(omd_t, p_new - ema, ema) and stores p, m, v, ema
// (36 B/elem instead of 28).  omd is one minus the decay; with warm-up omd_t = max(omd, 9 / (10 + t)), i.e. the decay
// min(decay, (1 + t) / (10 + t)), where t is the Adam step this call performs (the t of the bias corrections, read on
// the device, so a replayed graph advances it).  A skipped step leaves before its first load and writes nothing.
// Lane 0 of workgroup 0 records {omd_t, t, 0, 0} in ema_state with one ordinary vector store.
template <bool CLIP>
__device__ __forceinline__ float pre_scale(float g, float gs) { return CLIP ? g * gs : g; }

template <bool CLIP>
__global__ __launch_bounds__(256) void flat_adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                            float* __restrict__ m, float* __restrict__ v,
                                                            float* __restrict__ ema, int64_t n4, int64_t n, AdamArgs a,
                                                            const float* __restrict__ state,
                                                            const float* __restrict__ clip_state,
                                                            float* __restrict__ ema_state, float omd, int warmup) {
    float gs = 1.f, t = state[0];
    if (CLIP) {
        if (clip_state[2] == 0.f) return;
        gs = a.grad_scale;
        a.grad_scale = clip_state[1];  // adam_elem's own multiply applies the clip coefficient second
        t -= clip_state[3];
    }
    {
        const float lr = state[1];
        a.lr = lr;
        a.step_size = lr / -expm1f(t * logf(a.beta1));
        a.inv_sqrt_bc2 = rsqrtf(-expm1f(t * logf(a.beta2)));
    }
    const float omd_t = warmup ? fmaxf(omd, 9.f / (10.f + t)) : omd;
    if (blockIdx.x == 0 && threadIdx.x == 0) *reinterpret_cast<float4*>(ema_state) = make_float4(omd_t, t, 0.f, 0.f);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    float4* e4 = reinterpret_cast<float4*>(ema);
    for (; i < n4; i += stride) {
        float4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i], ee = e4[i];
        adam_elem(pp.x, pre_scale<CLIP>(gg.x, gs), mm.x, vv.x, a);
        adam_elem(pp.y, pre_scale<CLIP>(gg.y, gs), mm.y, vv.y, a);
        adam_elem(pp.z, pre_scale<CLIP>(gg.z, gs), mm.z, vv.z, a);
        adam_elem(pp.w, pre_scale<CLIP>(gg.w, gs), mm.w, vv.w, a);
        ee.x = fmaf(omd_t, pp.x - ee.x, ee.x);
        ee.y = fmaf(omd_t, pp.y - ee.y, ee.y);
        ee.z = fmaf(omd_t, pp.z - ee.z, ee.z);
        ee.w = fmaf(omd_t, pp.w - ee.w, ee.w);
        p4[i] = pp; m4[i] = mm; v4[i] = vv; e4[i] = ee;
    }
    for (int64_t j = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
        float pp = p[j], mm = m[j], vv = v[j], ee = ema[j];
        adam_elem(pp, pre_scale<CLIP>(g[j], gs), mm, vv, a);
        ee = fmaf(omd_t, pp - ee, ee);
        p[j] = pp; m[j] = mm; v[j] = vv; ema[j] = ee;
    }
}

// Parameter groups: the device-state update of the three kernels above -- plain (CLIP = EMA = false), under clip_state
// (CLIP), with the average (EMA), or both -- with lr and weight_decay PER ELEMENT.  The flat buffer pads every
// parameter to 64 floats, so a 64-float chunk belongs to one parameter and with it to one group: chunk_group[n / 64]
// (uint8, 1/256 B of traffic per element) names the group of each chunk, group_state fp32 [G, 4] = {lr_g, wd_g, 0, 0}
// holds the groups' constants (G <= 16: 256 B, read straight from global memory -- every wave of the grid reads the
// same few lines, which stay in the vector L1 / L2).  A lane's float4 i lies in chunk i >> 4, so the 16 lanes of a
// chunk read one table byte and one float4 of constants.  t, the bias corrections and t - skipped are shared and
// formed exactly as above; per lane a.lr = lr_g, a.weight_decay = wd_g, a.step_size = lr_g / (1 - beta1^t), then the
// same adam_elem with the same operands: the elements of group g come out bit for bit as the ungrouped kernel of the
// same form leaves them when it runs with (lr_g, wd_g).  A table entry >= G is read as G - 1 (never out of bounds).
// n is a multiple of 64: there is no scalar tail.
template <bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void flat_adam_groups_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                               float* __restrict__ m, float* __restrict__ v,
                                                               float* __restrict__ ema, int64_t n4, AdamArgs a,
                                                               const float* __restrict__ state,
                                                               const float4* __restrict__ group_state,
                                                               const uint8_t* __restrict__ chunk_group, int G,
                                                               const float* __restrict__ clip_state,
                                                               float* __restrict__ ema_state, float omd, int warmup) {
    float gs = 1.f, t = state[0];
    if (CLIP) {
        if (clip_state[2] == 0.f) return;
        gs = a.grad_scale;
        a.grad_scale = clip_state[1];  // adam_elem's own multiply applies the clip coefficient second
        t -= clip_state[3];
    }
    const float bc1 = -expm1f(t * logf(a.beta1));
    a.inv_sqrt_bc2 = rsqrtf(-expm1f(t * logf(a.beta2)));
    float omd_t = 0.f;
    if (EMA) {
        omd_t = warmup ? fmaxf(omd, 9.f / (10.f + t)) : omd;
        if (blockIdx.x == 0 && threadIdx.x == 0)
            *reinterpret_cast<float4*>(ema_state) = make_float4(omd_t, t, 0.f, 0.f);
    }
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    float4* e4 = reinterpret_cast<float4*>(ema);
    for (; i < n4; i += stride) {
        const int gi = min((int)chunk_group[i >> 4], G - 1);
        const float4 gc = group_state[gi];
        a.lr = gc.x;
        a.weight_decay = gc.y;
        a.step_size = gc.x / bc1;
        float4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i];
        adam_elem(pp.x, pre_scale<CLIP>(gg.x, gs), mm.x, vv.x, a);
        adam_elem(pp.y, pre_scale<CLIP>(gg.y, gs), mm.y, vv.y, a);
        adam_elem(pp.z, pre_scale<CLIP>(gg.z, gs), mm.z, vv.z, a);
        adam_elem(pp.w, pre_scale<CLIP>(gg.w, gs), mm.w, vv.w, a);
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
        if (EMA) {
            float4 ee = e4[i];
            ee.x = fmaf(omd_t, pp.x - ee.x, ee.x);
            ee.y = fmaf(omd_t, pp.y - ee.y, ee.y);
            ee.z = fmaf(omd_t, pp.z - ee.z, ee.z);
            ee.w = fmaf(omd_t, pp.w - ee.w, ee.w);
            e4[i] = ee;
        }
    }
}

template <bool CLIP, bool EMA>
void launch_groups(unsigned blocks, hipStream_t stream, float* p, const float* g, float* m, float* v, float* ema,
                   int64_t n4, const AdamArgs& a, const float* state, const float* group_state,
                   const uint8_t* chunk_group, int G, const float* clip_state, float* ema_state, float omd,
                   int warmup) {
    hipLaunchKernelGGL((flat_adam_groups_kernel<CLIP, EMA>), dim3(blocks), dim3(256), 0, stream, p, g, m, v, ema, n4, a,
                       state, reinterpret_cast<const float4*>(group_state), chunk_group, G, clip_state, ema_state, omd,
                       warmup);
}

}  // namespace

// ema == nullptr: no average (ema_state unused); clip_state == nullptr: no verdict to obey.  n % 64 == 0, 1 <= G <= 16.
extern "C" int rt1_flat_adam_groups_dev(float* p, const float* g, float* m, float* v, float* ema, int64_t n,
                                        const float* state, const float* group_state, const uint8_t* chunk_group,
                                        int G, const float* clip_state, float* ema_state, float beta1, float beta2,
                                        float eps, float grad_scale, float one_minus_decay, int warmup,
                                        hipStream_t stream) {
    if (state == nullptr || group_state == nullptr || chunk_group == nullptr || n <= 0 || n % 64 != 0 || G < 1 ||
        G > 16 || (ema != nullptr && ema_state == nullptr))
        return (int)hipErrorInvalidValue;
    AdamArgs a{0.f, beta1, beta2, eps, 0.f, 0.f, 1.f, grad_scale};
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    const bool clip = clip_state != nullptr, avg = ema != nullptr;
    auto* fn = clip ? (avg ? launch_groups<true, true> : launch_groups<true, false>)
                    : (avg ? launch_groups<false, true> : launch_groups<false, false>);
    fn((unsigned)blocks, stream, p, g, m, v, ema, n4, a, state, group_state, chunk_group, G, clip_state, ema_state,
       one_minus_decay, warmup);
    return (int)hipGetLastError();
}

extern "C" int rt1_flat_adam_ema_dev(float* p, const float* g, float* m, float* v, float* ema, int64_t n,
                                     const float* state, const float* clip_state, float* ema_state, float beta1,
                                     float beta2, float eps, float weight_decay, float grad_scale,
                                     float one_minus_decay, int warmup, hipStream_t stream) {
    if (state == nullptr || ema == nullptr || ema_state == nullptr) return (int)hipErrorInvalidValue;
    AdamArgs a{0.f, beta1, beta2, eps, weight_decay, 0.f, 1.f, grad_scale};
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    if (clip_state != nullptr)
        hipLaunchKernelGGL(flat_adam_ema_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, p, g, m, v, ema,
                           n4, n, a, state, clip_state, ema_state, one_minus_decay, warmup);
    else
        hipLaunchKernelGGL(flat_adam_ema_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, p, g, m, v, ema,
                           n4, n, a, state, clip_state, ema_state, one_minus_decay, warmup);
    return (int)hipGetLastError();
}

extern "C" int rt1_flat_adam_clip_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* state,
                                      const float* clip_state, float beta1, float beta2, float eps,
                                      float weight_decay, float grad_scale, hipStream_t stream) {
    if (state == nullptr || clip_state == nullptr) return (int)hipErrorInvalidValue;
    AdamArgs a{0.f, beta1, beta2, eps, weight_decay, 0.f, 1.f, grad_scale};
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(flat_adam_clip_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p, g, m, v, n4, n, a,
                       state, clip_state);
    return (int)hipGetLastError();
}

extern "C" int rt1_flat_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, float step_size, float inv_sqrt_bc2,
                             float grad_scale, hipStream_t stream) {
    AdamArgs a{lr, beta1, beta2, eps, weight_decay, step_size, inv_sqrt_bc2, grad_scale};
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(flat_adam_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p, g, m, v, n4, n, a,
                       (const float*)nullptr);
    return (int)hipGetLastError();
}

extern "C" int rt1_flat_adam_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* state,
                                 float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                 hipStream_t stream) {
    AdamArgs a{0.f, beta1, beta2, eps, weight_decay, 0.f, 1.f, grad_scale};
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(flat_adam_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p, g, m, v, n4, n, a, state);
    return (int)hipGetLastError();
}
