// Photometric augmentation (brightness, saturation, hue, contrast) of decoded planar uint8 frames, in place
// (data/photometric.py has the specification; reference: language_table/train/input_pipeline_rlds.py:390-457,
// ``PhotometricDistortions``, one draw of the four numbers per window of T frames).
//
// One workgroup per frame, one launch per batch.  The contrast step needs the frame's per-channel mean after the
// colour steps before any pixel can be finished, so the workgroup makes two passes over its frame: pass 1 runs
// steps 1-3 (u8 / 255, brightness, one fused HSV round trip for saturation + hue) and sums the three channels, pass 2
// recomputes steps 1-3, applies the contrast and writes the bytes.  A 300x300 frame is 270 KB, so pass 2 reads from
// L2.  No atomics; a frame's bytes depend only on its own bytes and its window's four numbers.
//
// Pixel math is fp32.  Two places are exact, because a flat frame (black, white, padding) otherwise puts every one
// of its pixels on the same rounding tie (at the default ranges: white - 0.1 -> 229.5, black + 0.1 -> 25.5) and an
// fp32 error of 1e-7 then moves the whole frame by one:
//  * the channel sums are integers (value * 2^30, exact for values >= 2^-7, truncated by < 2^-30 below), so the sum
//    is exact and order-free, and the mean is that sum rounded once: a flat frame's mean is its value;
//  * step 5 rounds the exact product c * 255 (the product's fp32 rounding error decides what looks like a tie).
//
// Bytes move in words: 4 pixels per thread per plane with 32-bit loads and stores when H*W and the tensor base are
// multiples of 4 (every plane base n*3*H*W + c*H*W is then aligned); otherwise the same 4-pixel groups move byte by
// byte and the last group of a plane may be partial.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int NT = 512;                 // threads per workgroup: 8 waves on one frame
constexpr float FIX = 1073741824.0f;    // 2^30: fixed-point scale of the channel sums

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

// u / 255 as the IEEE division gives it, for the integers 0..255: one correction step on u * (1 / 255)
__device__ __forceinline__ float unit255(float u) {
    const float rc = 1.0f / 255.0f;
    const float q = u * rc;
    return fmaf(fmaf(-q, 255.0f, u), rc, q);
}

__device__ __forceinline__ float hsv_channel(float k, float v, float vs) {
    k = k >= 6.0f ? k - 6.0f : k;
    return clamp01(fmaf(-vs, clamp01(fminf(k, 4.0f - k)), v));
}

// steps 2-3 on one pixel.  max = 0 (s = 0) and max = min (h = 0) select 1 as the divisor: the numerators are 0 there
__device__ __forceinline__ void colour_steps(float& r, float& g, float& b, float db, float fs, float dh) {
    r = clamp01(r + db);
    g = clamp01(g + db);
    b = clamp01(b + db);
    const float mx = fmaxf(fmaxf(r, g), b), mn = fminf(fminf(r, g), b), d = mx - mn;
    const float s = clamp01(d * __builtin_amdgcn_rcpf(mx > 0.0f ? mx : 1.0f) * fs);
    const float rd = __builtin_amdgcn_rcpf(d > 0.0f ? d : 1.0f);
    const float h6 = mx == r ? (g - b) * rd : (mx == g ? fmaf(b - r, rd, 2.0f) : fmaf(r - g, rd, 4.0f));
    float h = fmaf(h6, 1.0f / 6.0f, dh);
    h = (h - floorf(h)) * 6.0f;          // [0, 6]: 6 itself (h a hair below an integer) wraps in hsv_channel
    const float vs = mx * s;
    r = hsv_channel(h + 5.0f, mx, vs);
    g = hsv_channel(h + 3.0f, mx, vs);
    b = hsv_channel(h + 1.0f, mx, vs);
}

// step 5 for c in [0, 1]: round-half-even of the exact c * 255.  The opaque copy keeps the byte packs apart (see
// clip8_opaque in imgproc.hip)
__device__ __forceinline__ uint32_t to_byte(float c) {
#pragma clang fp contract(off)          // p must be the rounded product wherever it is used: p - k fused into
                                        // fma(c, 255, -k) is exact, never 0.5, and the tie test below never fires
    const float p = c * 255.0f;
    const float e = fmaf(c, 255.0f, -p);                    // exact: c * 255 = p + e
    float k = rintf(p);
    if (fabsf(p - k) == 0.5f && e != 0.0f) k = floorf(p) + (e > 0.0f ? 1.0f : 0.0f);
    int r = (int)k;
    asm volatile("" : "+v"(r));
    return (uint32_t)r;
}

template <bool WORDS>
__device__ __forceinline__ uint32_t load4(const uint8_t* p, int cnt) {
    if (WORDS) return *reinterpret_cast<const uint32_t*>(p);
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < cnt) w |= (uint32_t)p[j] << (8 * j);
    return w;
}

template <bool WORDS>
__device__ __forceinline__ void store4(uint8_t* p, uint32_t w, int cnt) {
    if (WORDS) {
        *reinterpret_cast<uint32_t*>(p) = w;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < cnt) p[j] = (uint8_t)(w >> (8 * j));
}

// img: [N, 3, HW] uint8, in place; params: [N / T, 4] fp32 (db, fs, dh, fc); grid = N
template <bool WORDS>
__global__ __launch_bounds__(NT) void photometric_kernel(uint8_t* __restrict__ img, const float* __restrict__ params,
                                                         int T, int HW) {
    __shared__ unsigned long long part[NT / 64][3];
    __shared__ float mean[3];
    const int n = blockIdx.x, t = threadIdx.x;
    const float* p = params + 4 * (int64_t)(n / T);
    const float db = p[0], fs = p[1], dh = p[2], fc = p[3];
    uint8_t* f = img + (int64_t)n * 3 * HW;
    const int G = (HW + 3) >> 2;                            // 4-pixel groups per plane, the last maybe partial
    unsigned long long s0 = 0, s1 = 0, s2 = 0;
#pragma unroll 2
    for (int g = t; g < G; g += NT) {                       // lanes past G add nothing
        const int cnt = WORDS ? 4 : (HW - 4 * g < 4 ? HW - 4 * g : 4);
        const uint32_t w0 = load4<WORDS>(f + 4 * g, cnt), w1 = load4<WORDS>(f + HW + 4 * g, cnt),
                       w2 = load4<WORDS>(f + 2 * (int64_t)HW + 4 * g, cnt);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float r = unit255((float)__builtin_amdgcn_ubfe(w0, 8 * j, 8));
            float gg = unit255((float)__builtin_amdgcn_ubfe(w1, 8 * j, 8));
            float b = unit255((float)__builtin_amdgcn_ubfe(w2, 8 * j, 8));
            colour_steps(r, gg, b, db, fs, dh);
            if (WORDS || j < cnt) {
                s0 += (uint32_t)(r * FIX);
                s1 += (uint32_t)(gg * FIX);
                s2 += (uint32_t)(b * FIX);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s0 += __shfl_down(s0, off);
        s1 += __shfl_down(s1, off);
        s2 += __shfl_down(s2, off);
    }
    if ((t & 63) == 0) {
        part[t >> 6][0] = s0;
        part[t >> 6][1] = s1;
        part[t >> 6][2] = s2;
    }
    __syncthreads();
    if (t < 3) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) s += part[w][t];
        mean[t] = (float)((double)s / ((double)HW * (double)FIX));     // < 2^53: exact until this one rounding
    }
    __syncthreads();          // also: every pass-1 read of the frame is done before pass 2 overwrites it
    const float m0 = mean[0], m1 = mean[1], m2 = mean[2];
    for (int g = t; g < G; g += NT) {
        const int cnt = WORDS ? 4 : (HW - 4 * g < 4 ? HW - 4 * g : 4);
        uint8_t* q = f + 4 * g;
        const uint32_t w0 = load4<WORDS>(q, cnt), w1 = load4<WORDS>(q + HW, cnt),
                       w2 = load4<WORDS>(q + 2 * (int64_t)HW, cnt);
        uint32_t o0 = 0, o1 = 0, o2 = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float r = unit255((float)__builtin_amdgcn_ubfe(w0, 8 * j, 8));
            float gg = unit255((float)__builtin_amdgcn_ubfe(w1, 8 * j, 8));
            float b = unit255((float)__builtin_amdgcn_ubfe(w2, 8 * j, 8));
            colour_steps(r, gg, b, db, fs, dh);
            o0 |= to_byte(clamp01(fmaf(r - m0, fc, m0))) << (8 * j);
            o1 |= to_byte(clamp01(fmaf(gg - m1, fc, m1))) << (8 * j);
            o2 |= to_byte(clamp01(fmaf(b - m2, fc, m2))) << (8 * j);
        }
        store4<WORDS>(q, o0, cnt);
        store4<WORDS>(q + HW, o1, cnt);
        store4<WORDS>(q + 2 * (int64_t)HW, o2, cnt);
    }
}

}  // namespace

extern "C" {

int rt1_photometric_u8(uint8_t* img, const float* params, int N, int T, int HW, hipStream_t st) {
    if (N <= 0 || T <= 0 || HW <= 0 || N % T != 0 || (int64_t)HW * 3 > INT32_MAX) return (int)hipErrorInvalidValue;
    if (HW % 4 == 0 && ((uintptr_t)img & 3) == 0)
        hipLaunchKernelGGL(photometric_kernel<true>, dim3(N), dim3(NT), 0, st, img, params, T, HW);
    else
        hipLaunchKernelGGL(photometric_kernel<false>, dim3(N), dim3(NT), 0, st, img, params, T, HW);
    return (int)hipGetLastError();
}

}  // extern "C"
