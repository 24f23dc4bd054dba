// LAVA image encoder stage as ONE op: y = maxpool2(relu(conv3x3_same(x, W) + b)), VALID pooling (gfx950, wave64).
// Forward, data gradient and weight gradient as implicit GEMMs on v_mfma_f32_16x16x32_bf16; im2col, the
// full-resolution conv output and the full-resolution pre-activation gradient dpre are never in memory.
//
// Shapes served: (Cin, Cout) in {(3 | 6 | 9 | 12, 32), (32, 64), (64, 128), (128, 256)}, any N, any H, W >= 2.
// Activations and their gradients are NHWC bf16, accumulation fp32, dW / db fp32.  The first stage (Cin < 32) reads
// the frames as they arrive, uint8 (/255 fused) or fp32, rounded to bf16 (RNE) while staging.
//
// Work split.  A 256-lane workgroup (4 waves) owns one frame's conv tile of kTh x kTw = 8 x 16 pixels (4 x 8 pooled)
// and BN = 64 (or 32) output columns.  The 128 GEMM rows of the tile are numbered m = 4 * window + position (position
// row-major inside the 2 x 2 pooling window), so the 16x16 accumulator of a lane -- 4 consecutive rows of one column
// -- is exactly the four pooling candidates of one pooled pixel for one channel: bias, ReLU, max and argmax are
// 4-register work, no cross-lane traffic.  (The 32x32x16 instruction groups rows the same way but its 16-register
// accumulator per tile would double the accumulator file for the same tile; 16x16x32 keeps wave = 2 row tiles x 4
// column tiles in 32 accumulator VGPRs and does K = 32 = one Cin chunk per instruction.)
//
// Data movement.  Per Cin chunk of 32 the tile's input window (10 x 18 pixels: the tile plus a 1-pixel halo, zero
// outside the image) is staged NHWC into LDS, pixel stride 40 bf16 (80 B: the 16 rows of an A fragment start 20
// banks apart), together with the chunk's packed weights [9][32][BN] (row stride BN + 8).  One (tap, chunk) is one
// K = 32 step: the A fragment of row m is ONE 16-byte LDS read of 8 consecutive channels at the tap-shifted pixel,
// the B fragment the gfx950 LDS transpose read of the [K][N] slab (as gemm.hip's NN form).  The same staged window
// feeds all 9 taps and all BN columns.  The next chunk's global loads are issued into registers before the current
// chunk's MFMAs and written to LDS after them (gemm.hip's single-buffer scheme: occupancy over a double buffer).
//
// Stage 1 (Cin = 3): the 27 tap-channel products are one K = 32 step (zero padded).  The raw window rows are read
// coalesced over the 3-value pixels (54 consecutive values per window row), and the A rows are built as an explicit
// im2col tile [128][32] in LDS from them.
//
// Data gradient: dx = conv3x3_same(dpre, W flipped and transposed) through the SAME kernel template; only the
// staging (each pooled (dy, idx) element is expanded to its 2 x 2 block while staging: dy at position idx, zeros
// elsewhere, zeros when dead or on a dropped odd row / column), the weight pack and the epilogue (plain bf16 store
// of all 128 rows) differ.
//
// Weight gradient: dW[tap] = x_shifted(tap)^T dpre with K = pixels.  Grid = partials x Cin tiles (32) x Cout tiles
// (64); a workgroup walks a fixed, contiguous range of (frame, tile) items, stages x's window once per tile and reads
// it tap-shifted, both operands pixel-major through the LDS transpose read (as wgrad.hip), and accumulates
// [9][32][64] in registers (72 VGPRs per wave).  db is the column sum of the same staged dpre: one more MFMA against
// a fragment of ones.  Each workgroup writes one fp32 partial; a second launch adds the partials in a fixed order
// (16 interleaved chains per output, combined as a fixed tree) and writes dW in nn.Conv2d's [Cout][Cin][3][3].  No
// atomics: dW, db are bitwise functions of the inputs.
//
// PixelLangMSE's language-conditioned encoder adds two forms (template parameters of the same kernels).  Its first
// stage stacks s = 2 .. 4 frames channel-wise, Cin = 3 s in {6, 9, 12}: the im2col K = 9 Cin <= 108 is padded to 2 .. 4
// chunks of 32 (the "taps" of the stage-1 kernels), the raw window row is 18 Cin consecutive values.  Its later stages
// multiply conv + bias by a per-frame, per-channel gate g fp32 [N, Cout] before the ReLU (GATE): the forward epilogue
// compares v = g * (acc + b); the data gradient rounds bf16(dy * g) while staging (K is the gated channel); the weight
// gradient keeps dy as it is and folds g[frame, column] into a second fp32 accumulator when its item walk changes
// frame; the gate gradient is a reduction of dy * y over the stage's own stored output (lava_conv_dgate_kernel).
//
// Every kernel is built without packed fp32 (common.h NO_PACKED_FP32); the bodies call only __forceinline__ functions.
#include "common.h"

using namespace rt1;

namespace {

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bf16x4 lds_v4;

constexpr int BLOCK = 256;
constexpr int kTh = 8, kTw = 16;                  // conv tile
constexpr int kWh = kTh + 2, kWw = kTw + 2;       // staged window
constexpr int kPix = kWh * kWw;                   // 180
constexpr int kM = kTh * kTw;                     // 128 GEMM rows
constexpr int kXs = 40;                           // LDS pixel stride (bf16): 32 channels + 16 B
constexpr int kRs = 56;                           // raw (Cin = 3) window row stride: 54 values used
constexpr int X_ELEMS = kPix * kXs;               // 7200
constexpr int R_ELEMS = kWh * kRs;                // 560
constexpr int XV = (kPix * 4 + BLOCK - 1) / BLOCK;    // 16-byte window vectors per thread (3)

// first stage, Cin = 3 s stacked frames (s = 1 .. 4): a raw window row is kWw * Cin consecutive values, the im2col
// tile has K = 9 Cin <= 108 zero padded to k_chunks(Cin) chunks of 32
constexpr int r_vals(int cin) { return kWw * cin; }                                   // 54 at Cin = 3
constexpr int r_stride(int cin) { return kWw * cin + 2; }                             // 56 = kRs
constexpr int r_elems(int cin) { return kWh * r_stride(cin); }
constexpr int r_regs(int cin) { return (kWh * r_vals(cin) + BLOCK - 1) / BLOCK; }     // raw values per thread (3 .. 9)
constexpr int k_chunks(int cin) { return (9 * cin + 31) / 32; }
constexpr int a_stride(int cin) { return k_chunks(cin) * 32 + 8; }                    // 40 = kXs
constexpr int a_elems(int cin) { return cin == 3 ? X_ELEMS : kM * a_stride(cin); }
static_assert(r_stride(3) == kRs && r_elems(3) == R_ELEMS && a_stride(3) == kXs, "Cin = 3 keeps its layout");

enum Mode : int { FWD = 0, FWD1 = 1, DGRAD = 2 };

__device__ __forceinline__ void block_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ bf16x8 tr_read8(const bf16_t* base0, const bf16_t* base1) {
    const bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)base0);
    const bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)base1);
    return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

__device__ __forceinline__ bf16_t to_bf(float f) { return (bf16_t)(pack2(f, 0.f) & 0xffffu); }

// GEMM row m = 4 * window + position -> the conv pixel inside the tile
__device__ __forceinline__ void m2pix(int m, int& py, int& px) {
    const int wi = m >> 2, pos = m & 3;
    py = 2 * (wi >> 3) + (pos >> 1);
    px = 2 * (wi & 7) + (pos & 1);
}

// 8 bf16 of dy kept where the window's argmax byte equals pos
__device__ __forceinline__ uint4 mask8(const uint4 v, const uint2 ix, const uint32_t pos) {
    uint4 o;
    o.x = v.x & (((ix.x & 0xffu) == pos ? 0xffffu : 0u) | (((ix.x >> 8) & 0xffu) == pos ? 0xffff0000u : 0u));
    o.y = v.y & ((((ix.x >> 16) & 0xffu) == pos ? 0xffffu : 0u) | ((ix.x >> 24) == pos ? 0xffff0000u : 0u));
    o.z = v.z & (((ix.y & 0xffu) == pos ? 0xffffu : 0u) | (((ix.y >> 8) & 0xffu) == pos ? 0xffff0000u : 0u));
    o.w = v.w & ((((ix.y >> 16) & 0xffu) == pos ? 0xffffu : 0u) | ((ix.y >> 24) == pos ? 0xffff0000u : 0u));
    return o;
}

// ---- staging: global -> registers (issue), registers -> LDS (commit) ----------------------------------------------

// window of an NHWC bf16 tensor [*, H, W, C], channels kc * 32 .. + 32; zero outside the image
struct XRegs {
    uint4 v[XV];
};
__device__ __forceinline__ void x_issue(XRegs& R, const bf16_t* __restrict__ x, int64_t n, int H, int W, int C,
                                        int h0, int w0, int kc, int t) {
#pragma unroll
    for (int i = 0; i < XV; ++i) {
        const int item = t + i * BLOCK, pix = item >> 2, v = item & 3;
        const int r = pix / kWw, c = pix - r * kWw, h = h0 - 1 + r, w = w0 - 1 + c;
        R.v[i] = make_uint4(0, 0, 0, 0);
        if (item < kPix * 4 && h >= 0 && h < H && w >= 0 && w < W)
            R.v[i] = *reinterpret_cast<const uint4*>(x + ((n * H + h) * W + w) * C + kc * 32 + v * 8);
    }
}
__device__ __forceinline__ void x_commit(const XRegs& R, bf16_t* Xl, int t) {
#pragma unroll
    for (int i = 0; i < XV; ++i) {
        const int item = t + i * BLOCK;
        if (item < kPix * 4) *reinterpret_cast<uint4*>(Xl + (item >> 2) * kXs + (item & 3) * 8) = R.v[i];
    }
}

// the same window of dpre, expanded from the pooled (dy, idx) [*, Hp, Wp, C]
// gated stage: the K dimension of the data gradient is the gated channel, so the operand is bf16_rne(dy * g[n, c]);
// a thread's 8 channels are the same for all its window vectors (BLOCK % 4 == 0): one gate load per chunk
struct DRegs {
    uint4 v[XV];
    uint2 ix[XV];
    float4 g[2];
};
template <bool GATE>
__device__ __forceinline__ void d_issue(DRegs& R, const bf16_t* __restrict__ dy, const uint8_t* __restrict__ idx,
                                        const float* __restrict__ gate, int64_t n, int Hp, int Wp, int C, int h0,
                                        int w0, int kc, int t) {
    if constexpr (GATE) {
        const float4* gp = reinterpret_cast<const float4*>(gate + n * C + kc * 32 + (t & 3) * 8);
        R.g[0] = gp[0];
        R.g[1] = gp[1];
    }
#pragma unroll
    for (int i = 0; i < XV; ++i) {
        const int item = t + i * BLOCK, pix = item >> 2, v = item & 3;
        const int r = pix / kWw, c = pix - r * kWw, h = h0 - 1 + r, w = w0 - 1 + c;
        R.v[i] = make_uint4(0, 0, 0, 0);
        R.ix[i] = make_uint2(0x04040404u, 0x04040404u);
        if (item < kPix * 4 && h >= 0 && w >= 0 && (h >> 1) < Hp && (w >> 1) < Wp) {
            const int64_t off = ((n * Hp + (h >> 1)) * Wp + (w >> 1)) * C + kc * 32 + v * 8;
            R.v[i] = *reinterpret_cast<const uint4*>(dy + off);
            R.ix[i] = *reinterpret_cast<const uint2*>(idx + off);
        }
    }
}
template <bool GATE>
__device__ __forceinline__ void d_commit(const DRegs& R, bf16_t* Xl, int h0, int w0, int t) {
#pragma unroll
    for (int i = 0; i < XV; ++i) {
        const int item = t + i * BLOCK, pix = item >> 2;
        const int r = pix / kWw, c = pix - r * kWw, h = h0 - 1 + r, w = w0 - 1 + c;
        uint4 o = mask8(R.v[i], R.ix[i], (uint32_t)(((h & 1) << 1) | (w & 1)));
        if constexpr (GATE) {                     // one fp32 multiply and one rounding (RNE) per element
            float f[8];
            unpack8(o, f);
            o.x = pack2(f[0] * R.g[0].x, f[1] * R.g[0].y);
            o.y = pack2(f[2] * R.g[0].z, f[3] * R.g[0].w);
            o.z = pack2(f[4] * R.g[1].x, f[5] * R.g[1].y);
            o.w = pack2(f[6] * R.g[1].z, f[7] * R.g[1].w);
        }
        if (item < kPix * 4) *reinterpret_cast<uint4*>(Xl + pix * kXs + (item & 3) * 8) = o;
    }
}

// raw window of the frames [*, H, W, CIN] (uint8 / 255 or fp32): 18 * CIN consecutive values per window row
__device__ __forceinline__ float frame_val(const uint8_t* p) { return (float)p[0] / 255.0f; }
__device__ __forceinline__ float frame_val(const float* p) { return p[0]; }

template <int CIN>
struct RRegs {
    float v[r_regs(CIN)];
};
template <int CIN, typename TIn>
__device__ __forceinline__ void r_issue(RRegs<CIN>& R, const TIn* __restrict__ img, int64_t n, int H, int W, int h0,
                                        int w0, int t) {
    constexpr int RW = r_vals(CIN);
#pragma unroll
    for (int i = 0; i < r_regs(CIN); ++i) {
        const int item = t + i * BLOCK, r = item / RW, j = item - r * RW;
        const int h = h0 - 1 + r, w = w0 - 1 + j / CIN;
        R.v[i] = 0.f;
        if (item < kWh * RW && h >= 0 && h < H && w >= 0 && w < W)
            R.v[i] = frame_val(img + ((n * H + h) * W + w) * CIN + (j - (j / CIN) * CIN));
    }
}
// raw values -> LDS, then the im2col tile Al[m][k], k = tap * CIN + channel < 9 CIN, zero up to the chunk boundary
// (both barriers inside).  A tap row of the window is 3 CIN consecutive raw values, but they start px * CIN values
// into the row -- no 16-byte alignment for an A fragment read -- so the tile is built explicitly, value by value.
template <int CIN>
__device__ __forceinline__ void r_commit_im2col(const RRegs<CIN>& R, bf16_t* Rl, bf16_t* Al, int t) {
    constexpr int RW = r_vals(CIN), RS = r_stride(CIN), KP = k_chunks(CIN) * 32, AS = a_stride(CIN);
#pragma unroll
    for (int i = 0; i < r_regs(CIN); ++i) {
        const int item = t + i * BLOCK, r = item / RW, j = item - r * RW;
        if (item < kWh * RW) Rl[r * RS + j] = to_bf(R.v[i]);
    }
    block_sync();
#pragma unroll
    for (int i = 0; i < kM * KP / BLOCK; ++i) {
        const int item = t + i * BLOCK, m = item / KP, k = item - m * KP;
        int py, px;
        m2pix(m, py, px);
        const int dy = k / (3 * CIN);             // k - dy * 3 CIN = dx * CIN + channel: consecutive in the raw row
        Al[m * AS + k] = k < 9 * CIN ? Rl[(py + dy) * RS + px * CIN + (k - dy * 3 * CIN)] : (bf16_t)0;
    }
}

// packed weights B [TAPS][Ktot][Ntot] bf16: rows kc * 32 .. + 32 (zero past Ktot), columns n0 .. n0 + BN
template <int TAPS, int BN>
struct BRegs {
    static constexpr int ITEMS = TAPS * 32 * BN / 8;
    static constexpr int PER = (ITEMS + BLOCK - 1) / BLOCK;
    uint4 v[PER];
};
// FLAT (first stage): B is [Ktot][Ntot] and "tap" counts its chunks of 32 rows
template <int TAPS, int BN, bool FLAT = false>
__device__ __forceinline__ void b_issue(BRegs<TAPS, BN>& R, const bf16_t* __restrict__ B, int Ktot, int Ntot, int kc,
                                        int n0, int t) {
    constexpr int C8 = BN / 8;
#pragma unroll
    for (int i = 0; i < BRegs<TAPS, BN>::PER; ++i) {
        const int item = t + i * BLOCK, tap = item / (32 * C8), rem = item - tap * (32 * C8);
        const int k = rem / C8, c = (rem - k * C8) * 8, kg = FLAT ? tap * 32 + k : kc * 32 + k;
        R.v[i] = make_uint4(0, 0, 0, 0);
        if (item < BRegs<TAPS, BN>::ITEMS && kg < Ktot)
            R.v[i] = *reinterpret_cast<const uint4*>(B + ((int64_t)(FLAT ? 0 : tap) * Ktot + kg) * Ntot + n0 + c);
    }
}
template <int TAPS, int BN>
__device__ __forceinline__ void b_commit(const BRegs<TAPS, BN>& R, bf16_t* Bl, int t) {
    constexpr int C8 = BN / 8;
#pragma unroll
    for (int i = 0; i < BRegs<TAPS, BN>::PER; ++i) {
        const int item = t + i * BLOCK, row = item / C8, c = (item - row * C8) * 8;      // row = tap * 32 + k
        if (item < BRegs<TAPS, BN>::ITEMS) *reinterpret_cast<uint4*>(Bl + row * (BN + 8) + c) = R.v[i];
    }
}

// ---- forward and data gradient: one template ----------------------------------------------------------------------

struct ConvArgs {
    const void* x;            // FWD: bf16 [N, H, W, K]; FWD1: frames [N, H, W, Cin]; DGRAD: dy bf16 [N, Hp, Wp, K]
    const uint8_t* idx_in;    // DGRAD: [N, Hp, Wp, K]
    const bf16_t* B;          // packed weights [9][K][Nc] (FWD1: [9 Cin][Nc])
    const float* bias;        // FWD / FWD1: [Nc]
    bf16_t* y;                // FWD / FWD1: [N, Hp, Wp, Nc]; DGRAD: dx [N, H, W, Nc]
    uint8_t* idx_out;         // FWD / FWD1: [N, Hp, Wp, Nc]
    int H, W, Hp, Wp;         // conv grid and pooled grid
    int K, Nc;                // GEMM K per tap (input channels) and N (output channels)
    int tiles_x, tiles;       // tiles per row, tiles per frame
    const float* gate;        // GATE: fp32 [N, gated channels]: y = pool(relu(g * (conv + b))), dx = conv^T(g * dpre)
};

// GATE: the language-gated stage.  CIN1: the stacked-frame channels of the first stage (FWD1), whose "taps" are the
// k_chunks(CIN1) chunks of the im2col K.
template <int MODE, int NT, typename TIn, bool GATE = false, int CIN1 = 3>
__global__ NO_PACKED_FP32 __launch_bounds__(BLOCK) void lava_conv_kernel(ConvArgs a) {
    constexpr int BN = NT * 16, LDB = BN + 8;
    constexpr int TAPS = MODE == FWD1 ? k_chunks(CIN1) : 9;
    constexpr int AS = MODE == FWD1 ? a_stride(CIN1) : kXs;
    constexpr int A_ELEMS = MODE == FWD1 ? a_elems(CIN1) : X_ELEMS;
    constexpr int B_ELEMS = TAPS * 32 * LDB;
    constexpr int O_ELEMS = MODE == DGRAD ? kM * LDB : 32 * LDB + 32 * (BN + 16) / 2;
    constexpr int S_ELEMS = A_ELEMS + B_ELEMS + (MODE == FWD1 ? r_elems(CIN1) : 0);
    __shared__ __attribute__((aligned(16))) bf16_t smem[S_ELEMS > O_ELEMS ? S_ELEMS : O_ELEMS];
    bf16_t* Xl = smem;
    bf16_t* Bl = smem + A_ELEMS;
    bf16_t* Rl = Bl + B_ELEMS;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 15, lh = lane >> 4;
    const int q4 = lr >> 2, p4 = lr & 3;
    const int64_t n = blockIdx.x / a.tiles;
    const int tile = blockIdx.x - (int)n * a.tiles;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int h0 = ty * kTh, w0 = tx * kTw, n0 = blockIdx.y * BN;
    const int nch = MODE == FWD1 ? 1 : a.K / 32;

    f32x4 acc[2][NT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    int aoff[2];              // the lane's A row: its pixel in the window (or its im2col row), plus its 8 k
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = (wave * 2 + i) * 16 + lr;
        int py, px;
        m2pix(m, py, px);
        aoff[i] = (MODE == FWD1 ? m : py * kWw + px) * AS + lh * 8;
    }

    XRegs xr;
    DRegs dr;
    RRegs<CIN1> rr;
    BRegs<TAPS, BN> br;
    if constexpr (MODE == FWD) x_issue(xr, (const bf16_t*)a.x, n, a.H, a.W, a.K, h0, w0, 0, t);
    if constexpr (MODE == DGRAD)
        d_issue<GATE>(dr, (const bf16_t*)a.x, a.idx_in, a.gate, n, a.Hp, a.Wp, a.K, h0, w0, 0, t);
    if constexpr (MODE == FWD1) r_issue<CIN1>(rr, (const TIn*)a.x, n, a.H, a.W, h0, w0, t);
    b_issue<TAPS, BN, MODE == FWD1>(br, a.B, MODE == FWD1 ? 9 * CIN1 : a.K, a.Nc, 0, n0, t);

    for (int kc = 0; kc < nch; ++kc) {
        block_sync();                              // the previous chunk's fragment reads are done
        if constexpr (MODE == FWD) x_commit(xr, Xl, t);
        if constexpr (MODE == DGRAD) d_commit<GATE>(dr, Xl, h0, w0, t);
        if constexpr (MODE == FWD1) r_commit_im2col<CIN1>(rr, Rl, Xl, t);
        b_commit(br, Bl, t);
        block_sync();
        if (kc + 1 < nch) {                        // in flight during this chunk's MFMAs
            if constexpr (MODE == FWD) x_issue(xr, (const bf16_t*)a.x, n, a.H, a.W, a.K, h0, w0, kc + 1, t);
            if constexpr (MODE == DGRAD)
                d_issue<GATE>(dr, (const bf16_t*)a.x, a.idx_in, a.gate, n, a.Hp, a.Wp, a.K, h0, w0, kc + 1, t);
            b_issue(br, a.B, a.K, a.Nc, kc + 1, n0, t);
        }
#pragma unroll
        for (int tap = 0; tap < TAPS; ++tap) {
            const int toff = MODE == FWD1 ? tap * 32 : ((tap / 3) * kWw + (tap % 3)) * kXs;
            bf16x8 fa[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(Xl + aoff[i] + toff);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const bf16_t* bp = Bl + (tap * 32 + lh * 8 + q4) * LDB + j * 16 + p4 * 4;
                const bf16x8 fb = tr_read8(bp, bp + 4 * LDB);
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb, acc[i][j], 0, 0, 0);
            }
        }
    }

    block_sync();                                  // the last fragment reads are done: smem becomes the output tile
    if constexpr (MODE == DGRAD) {
        // lane holds rows m = (wave * 2 + i) * 16 + lh * 4 + e of column j * 16 + lr
        bf16_t* Ol = smem;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    Ol[((wave * 2 + i) * 16 + lh * 4 + e) * LDB + j * 16 + lr] = to_bf(acc[i][j][e]);
        block_sync();
        constexpr int C8 = BN / 8;
        for (int o = t; o < kM * C8; o += BLOCK) {
            const int m = o / C8, c = (o - m * C8) * 8;
            int py, px;
            m2pix(m, py, px);
            const int h = h0 + py, w = w0 + px;
            if (h < a.H && w < a.W)
                *reinterpret_cast<uint4*>(a.y + ((n * a.H + h) * a.W + w) * a.Nc + n0 + c) =
                    *reinterpret_cast<const uint4*>(Ol + m * LDB + c);
        }
    } else {
        // the lane's 4 accumulator rows are the 4 candidates of window (wave * 2 + i) * 4 + lh, channel j * 16 + lr
        constexpr int LDI = BN + 16;
        bf16_t* Yl = smem;
        uint8_t* Il = reinterpret_cast<uint8_t*>(smem + 32 * LDB);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const float bv = a.bias[n0 + j * 16 + lr];
            float gv = 1.f;
            if constexpr (GATE) gv = a.gate[n * a.Nc + n0 + j * 16 + lr];
            // gated: v = g * (conv + b) in fp32; a negative gate makes the smallest conv value win, a zero gate
            // leaves no v > 0: the whole channel of the frame is dead
            auto cand = [&](int i, int e) __attribute__((always_inline)) {
                return GATE ? gv * (acc[i][j][e] + bv) : acc[i][j][e] + bv;
            };
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float best = cand(i, 0);
                int bi = 0;
#pragma unroll
                for (int e = 1; e < 4; ++e) {
                    const float v = cand(i, e);
                    if (v > best) {                // a tie keeps the lowest position
                        best = v;
                        bi = e;
                    }
                }
                if (!(best > 0.f)) {               // dead window: y is exactly 0 and no gradient flows
                    best = 0.f;
                    bi = 4;
                }
                const int wi = (wave * 2 + i) * 4 + lh;
                Yl[wi * LDB + j * 16 + lr] = to_bf(best);
                Il[wi * LDI + j * 16 + lr] = (uint8_t)bi;
            }
        }
        block_sync();
        constexpr int C8 = BN / 8, C16 = BN / 16;
        const int ph0 = h0 >> 1, pw0 = w0 >> 1;
        for (int o = t; o < 32 * C8; o += BLOCK) {
            const int wi = o / C8, c = (o - wi * C8) * 8, ph = ph0 + (wi >> 3), pw = pw0 + (wi & 7);
            if (ph < a.Hp && pw < a.Wp)
                *reinterpret_cast<uint4*>(a.y + ((n * a.Hp + ph) * a.Wp + pw) * a.Nc + n0 + c) =
                    *reinterpret_cast<const uint4*>(Yl + wi * LDB + c);
        }
        for (int o = t; o < 32 * C16; o += BLOCK) {
            const int wi = o / C16, c = (o - wi * C16) * 16, ph = ph0 + (wi >> 3), pw = pw0 + (wi & 7);
            if (ph < a.Hp && pw < a.Wp)
                *reinterpret_cast<uint4*>(a.idx_out + ((n * a.Hp + ph) * a.Wp + pw) * a.Nc + n0 + c) =
                    *reinterpret_cast<const uint4*>(Il + wi * LDI + c);
        }
    }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------

struct WgradArgs {
    const void* x;            // bf16 [N, H, W, Cin] or the frames [N, H, W, Cin < 32]
    const bf16_t* dy;         // [N, Hp, Wp, Cout]
    const uint8_t* idx;       // [N, Hp, Wp, Cout]
    float* part;              // [P][9 * Cin][Cout]
    float* dbpart;            // [P][Cout]
    int H, W, Hp, Wp, Cin, Cout;
    int tiles_x, tiles;
    int64_t T;                // N * tiles work items, split into P contiguous ranges
    int P;
    const float* gate;        // GATE: fp32 [N, Cout]: dW = sum_n g[n, :] * (patch_n^T dpre_n), db likewise
};

// IM2COL (first stage, CIN1 = 3 s): A^T is the im2col tile [128 pixels][k_chunks x 32], a "tap" is one chunk of 32
// rows, wave = (row tile, column tile) of [32][32] per chunk; otherwise A^T is the staged window read tap-shifted,
// wave = column tile of [9][32][64], both row tiles.
// GATE: the gate is per output column and a lane's accumulator columns are fixed, so dy is not re-rounded: acc is the
// running sum of ONE frame, folded into tot as tot += g[frame, column] * acc (fp32) when the item walk enters
// another frame and at the end.
template <bool IM2COL, typename TIn, bool GATE = false, int CIN1 = 3>
__global__ NO_PACKED_FP32 __launch_bounds__(BLOCK) void lava_conv_wgrad_kernel(WgradArgs a) {
    constexpr int TAPS = IM2COL ? k_chunks(CIN1) : 9, MTW = IM2COL ? 1 : 2, CoT = IM2COL ? 32 : 64, DS = CoT + 8;
    constexpr int AS = IM2COL ? a_stride(CIN1) : kXs, A_ELEMS = IM2COL ? a_elems(CIN1) : X_ELEMS;
    constexpr int D_ELEMS = kM * DS;
    __shared__ __attribute__((aligned(16))) bf16_t smem[A_ELEMS + D_ELEMS + (IM2COL ? r_elems(CIN1) : 0)];
    bf16_t* Xl = smem;
    bf16_t* Dl = smem + A_ELEMS;
    bf16_t* Rl = Dl + D_ELEMS;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 15, lh = lane >> 4;
    const int q4 = lr >> 2, p4 = lr & 3;
    const int rt0 = IM2COL ? wave >> 1 : 0, ct = IM2COL ? wave & 1 : wave;
    const int ci0 = blockIdx.y * 32, co0 = blockIdx.z * CoT;
    const int64_t p = blockIdx.x;
    const int64_t t0 = p * a.T / a.P, t1 = (p + 1) * a.T / a.P;
    const bool do_db = blockIdx.y == 0 && rt0 == 0;

    f32x4 acc[TAPS][MTW], accdb = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 tot[GATE ? TAPS : 1][MTW], totdb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < TAPS; ++i)
#pragma unroll
        for (int j = 0; j < MTW; ++j) {
            acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (GATE) tot[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    const short one = (short)0x3f80;
    const bf16x8 ones = bf16x8{one, one, one, one, one, one, one, one};

    // the thread's pooled element(s) of the tile: window wi, 8 channels
    constexpr int DV = 32 * (CoT / 8);            // 256 or 128 items
    const int dwi = t / (CoT / 8), dv = t - dwi * (CoT / 8);

    XRegs xr;
    RRegs<CIN1> rr;
    uint4 dyv;
    uint2 dix;
    int64_t n;
    int h0, w0;
    auto issue = [&](int64_t item) __attribute__((always_inline)) {
        n = item / a.tiles;
        const int tile = (int)(item - n * a.tiles), ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
        h0 = ty * kTh;
        w0 = tx * kTw;
        if constexpr (IM2COL) r_issue<CIN1>(rr, (const TIn*)a.x, n, a.H, a.W, h0, w0, t);
        else x_issue(xr, (const bf16_t*)a.x, n, a.H, a.W, a.Cin, h0, w0, blockIdx.y, t);
        dyv = make_uint4(0, 0, 0, 0);
        dix = make_uint2(0x04040404u, 0x04040404u);
        const int ph = (h0 >> 1) + (dwi >> 3), pw = (w0 >> 1) + (dwi & 7);
        if (t < DV && ph < a.Hp && pw < a.Wp) {
            const int64_t off = ((n * a.Hp + ph) * a.Wp + pw) * a.Cout + co0 + dv * 8;
            dyv = *reinterpret_cast<const uint4*>(a.dy + off);
            dix = *reinterpret_cast<const uint2*>(a.idx + off);
        }
    };
    auto fold = [&](int64_t frame) __attribute__((always_inline)) {
        const float gv = a.gate[frame * a.Cout + co0 + ct * 16 + lr];
#pragma unroll
        for (int i = 0; i < TAPS; ++i)
#pragma unroll
            for (int j = 0; j < MTW; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    tot[GATE ? i : 0][j][e] += gv * acc[i][j][e];
                    acc[i][j][e] = 0.f;
                }
        totdb[0] += gv * accdb[0];
        accdb = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    issue(t0);
    int64_t nacc = n;                             // the frame acc belongs to
    for (int64_t item = t0; item < t1; ++item) {
        block_sync();
        if constexpr (IM2COL) r_commit_im2col<CIN1>(rr, Rl, Xl, t);
        else x_commit(xr, Xl, t);
        if constexpr (GATE) {                     // n is still this item's frame: the next issue comes below
            if (n != nacc) {
                fold(nacc);
                nacc = n;
            }
        }
        if (t < DV) {
#pragma unroll
            for (int pos = 0; pos < 4; ++pos)
                *reinterpret_cast<uint4*>(Dl + (4 * dwi + pos) * DS + dv * 8) = mask8(dyv, dix, (uint32_t)pos);
        }
        block_sync();
        if (item + 1 < t1) issue(item + 1);
#pragma unroll
        for (int s = 0; s < kM / 32; ++s) {
            const int ma = s * 32 + lh * 8 + q4, mb = ma + 4;      // the lane's two transpose-read rows (pixels)
            const bf16x8 fd = tr_read8(Dl + ma * DS + ct * 16 + p4 * 4, Dl + mb * DS + ct * 16 + p4 * 4);
            if (do_db) accdb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, fd, accdb, 0, 0, 0);
            int pya, pxa, pyb, pxb;
            m2pix(ma, pya, pxa);
            m2pix(mb, pyb, pxb);
            const int xa = (IM2COL ? ma : pya * kWw + pxa) * AS + p4 * 4;
            const int xb = (IM2COL ? mb : pyb * kWw + pxb) * AS + p4 * 4;
#pragma unroll
            for (int tap = 0; tap < TAPS; ++tap) {
                const int toff = IM2COL ? tap * 32 : ((tap / 3) * kWw + (tap % 3)) * kXs;
#pragma unroll
                for (int i = 0; i < MTW; ++i) {
                    const int co = toff + (rt0 + i) * 16;
                    const bf16x8 fa = tr_read8(Xl + xa + co, Xl + xb + co);
                    acc[tap][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fd, acc[tap][i], 0, 0, 0);
                }
            }
        }
    }

    if constexpr (GATE) fold(nacc);

    // lane holds rows (rt0 + i) * 16 + lh * 4 + e (input channel, or chunk * 32 + ... = tap * Cin + channel) of
    // column ct * 16 + lr
    const int rows = IM2COL ? 9 * CIN1 : 9 * a.Cin;
    float* part = a.part + p * rows * a.Cout + co0 + ct * 16 + lr;
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap)
#pragma unroll
        for (int i = 0; i < MTW; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = (rt0 + i) * 16 + lh * 4 + e;
                const int row = IM2COL ? tap * 32 + r : tap * a.Cin + ci0 + r;
                if (row < rows) part[(int64_t)row * a.Cout] = GATE ? tot[GATE ? tap : 0][i][e] : acc[tap][i][e];
            }
    if (do_db && lh == 0) a.dbpart[p * a.Cout + co0 + ct * 16 + lr] = GATE ? totdb[0] : accdb[0];
}

// Gate gradient of a gated stage.  At a live winner y = g * (conv + b) and y is stored (it is the next stage's
// input), so dg[n, c] = (sum_p dy[n, p, c] * y[n, p, c]) / g[n, c], 0 where g == 0; a dead window has y = 0.  No conv
// is recomputed.  Workgroup = (frame, slab of 64 channels): 8 channel vectors x 32 pixel lanes, four 16-byte loads
// of dy and of y in flight per lane, fp32 sums, the 32 lanes combined as a fixed tree: bitwise reproducible.
__global__ NO_PACKED_FP32 __launch_bounds__(BLOCK) void lava_conv_dgate_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ y, const float* __restrict__ gate, int P, int C,
    float* __restrict__ dg) {
    __shared__ float red[32][64 + 1];
    const int t = threadIdx.x, cv = t & 7, pl = t >> 3;
    const int64_t n = blockIdx.x;
    const int c0 = blockIdx.y * 64;
    const int64_t base = n * P * C + c0 + cv * 8;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int p0 = pl; p0 < P; p0 += 128) {
        uint4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = p0 + 32 * u;
            a[u] = b[u] = make_uint4(0, 0, 0, 0);
            if (p < P) {
                a[u] = *reinterpret_cast<const uint4*>(dy + base + (int64_t)p * C);
                b[u] = *reinterpret_cast<const uint4*>(y + base + (int64_t)p * C);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float fa[8], fb[8];
            unpack8(a[u], fa);
            unpack8(b[u], fb);
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += fa[e] * fb[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[pl][cv * 8 + e] = s[e];
    block_sync();
    if (t < 64) {
        float q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float v = 0.f;
#pragma unroll
            for (int r = 0; r < 8; ++r) v += red[u * 8 + r][t];
            q[u] = v;
        }
        const float g = gate[n * C + c0 + t];
        dg[n * C + c0 + t] = g == 0.f ? 0.f : ((q[0] + q[1]) + (q[2] + q[3])) / g;
    }
}

// partials in a fixed order -> dW fp32 [Cout][Cin][3][3] and db fp32 [Cout]
__global__ NO_PACKED_FP32 __launch_bounds__(BLOCK) void lava_conv_wgrad_reduce_kernel(
    const float* __restrict__ part, const float* __restrict__ dbpart, int P, int Cin, int Cout,
    float* __restrict__ dW, float* __restrict__ db) {
    // 64 outputs x 4 slices of the partials per workgroup: slice s adds partials s, s + 4, ... on four independent
    // chains (a serial chain of P dependent loads is latency-bound), and the 16 sums are combined in a fixed order
    __shared__ float s_sum[4][64];
    const int E = 9 * Cin * Cout;
    const int o = threadIdx.x & 63, s = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + o;
    const bool is_w = i < E, live = i < E + Cout;
    const float* src = is_w ? part + i : dbpart + (i - E);
    const int64_t stride = is_w ? E : Cout;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (live) {
        int p = s;
        for (; p + 12 < P; p += 16) {
            a0 += src[p * stride];
            a1 += src[(p + 4) * stride];
            a2 += src[(p + 8) * stride];
            a3 += src[(p + 12) * stride];
        }
        for (; p < P; p += 4) a0 += src[p * stride];
    }
    s_sum[s][o] = (a0 + a1) + (a2 + a3);
    block_sync();
    if (s == 0 && live) {
        const float v = (s_sum[0][o] + s_sum[1][o]) + (s_sum[2][o] + s_sum[3][o]);
        if (is_w) {
            const int tap = i / (Cin * Cout), rem = i - tap * (Cin * Cout), ci = rem / Cout, co = rem - ci * Cout;
            dW[((int64_t)co * Cin + ci) * 9 + tap] = v;
        } else {
            db[i - E] = v;
        }
    }
}

struct Geo {
    int Hp, Wp, tiles_x, tiles_y;
    int64_t blocks;
};

// false when a shape cannot be served (or a launch dimension would overflow)
bool geometry(int64_t N, int64_t H, int64_t W, int cin, int cout, Geo& g) {
    const bool first = (cin == 3 || cin == 6 || cin == 9 || cin == 12) && cout == 32;      // 1 .. 4 stacked frames
    if (!(first || (cin == 32 && cout == 64) || (cin == 64 && cout == 128) || (cin == 128 && cout == 256)))
        return false;
    if (N < 1 || H < 2 || W < 2 || H > (1 << 20) || W > (1 << 20)) return false;
    g.Hp = (int)(H / 2);
    g.Wp = (int)(W / 2);
    g.tiles_x = (int)((W + kTw - 1) / kTw);
    g.tiles_y = (int)((H + kTh - 1) / kTh);
    const int64_t tiles = (int64_t)g.tiles_x * g.tiles_y;
    if (tiles > INT32_MAX) return false;
    g.blocks = N * tiles;
    return g.blocks <= INT32_MAX;
}

template <int MODE, int NT, typename TIn, bool GATE = false, int CIN1 = 3>
void launch_conv(const ConvArgs& a, int64_t blocks, hipStream_t st) {
    hipLaunchKernelGGL((lava_conv_kernel<MODE, NT, TIn, GATE, CIN1>),
                       dim3((unsigned)blocks, (unsigned)(a.Nc / (NT * 16))), dim3(BLOCK), 0, st, a);
}

template <typename TIn>
void launch_fwd1(const ConvArgs& a, int64_t blocks, int cin, hipStream_t st) {
    if (cin == 3) launch_conv<FWD1, 2, TIn, false, 3>(a, blocks, st);
    else if (cin == 6) launch_conv<FWD1, 2, TIn, false, 6>(a, blocks, st);
    else if (cin == 9) launch_conv<FWD1, 2, TIn, false, 9>(a, blocks, st);
    else launch_conv<FWD1, 2, TIn, false, 12>(a, blocks, st);
}

template <typename TIn, int CIN1>
void launch_wgrad1(const WgradArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((lava_conv_wgrad_kernel<true, TIn, false, CIN1>), dim3(a.P, 1, 1), dim3(BLOCK), 0, st, a);
}
template <typename TIn>
void launch_wgrad1(const WgradArgs& a, hipStream_t st) {
    if (a.Cin == 3) launch_wgrad1<TIn, 3>(a, st);
    else if (a.Cin == 6) launch_wgrad1<TIn, 6>(a, st);
    else if (a.Cin == 9) launch_wgrad1<TIn, 9>(a, st);
    else launch_wgrad1<TIn, 12>(a, st);
}

int wgrad_partials(const Geo& g, int cin, int cout) {
    const int ctiles = cin < 32 ? 1 : (cin / 32) * (cout / 64);
    const int64_t cap = 1024 / ctiles;             // about four workgroups per CU over all channel tiles
    return (int)(g.blocks < cap ? g.blocks : cap);
}

// x_kind: 0 = bf16 NHWC activations, 1 = uint8 frames, 2 = fp32 frames (1, 2 only with Cin < 32 and the reverse);
// gate: nullptr for the plain stage, else fp32 [N, cout] (Cin >= 32 only)
bool kind_ok(int cin, int x_kind, const float* gate) {
    return x_kind >= 0 && x_kind <= 2 && (cin < 32) == (x_kind != 0) && (gate == nullptr || cin >= 32);
}

int conv_fwd(const void* x, int x_kind, const uint16_t* wp, const float* bias, const float* gate, int64_t N, int64_t H,
             int64_t W, int cin, int cout, uint16_t* y, uint8_t* idx, hipStream_t stream) {
    Geo g;
    if (x == nullptr || wp == nullptr || bias == nullptr || y == nullptr || idx == nullptr ||
        !geometry(N, H, W, cin, cout, g) || !kind_ok(cin, x_kind, gate))
        return (int)hipErrorInvalidValue;
    ConvArgs a{x, nullptr, wp, bias, y, idx, (int)H, (int)W, g.Hp, g.Wp, cin, cout, g.tiles_x,
               g.tiles_x * g.tiles_y, gate};
    if (x_kind == 1) launch_fwd1<uint8_t>(a, g.blocks, cin, stream);
    else if (x_kind == 2) launch_fwd1<float>(a, g.blocks, cin, stream);
    else if (gate != nullptr) launch_conv<FWD, 4, uint16_t, true>(a, g.blocks, stream);
    else launch_conv<FWD, 4, uint16_t>(a, g.blocks, stream);
    return (int)hipGetLastError();
}

int conv_dgrad(const uint16_t* dy, const uint8_t* idx, const uint16_t* wd, const float* gate, int64_t N, int64_t H,
               int64_t W, int cin, int cout, uint16_t* dx, hipStream_t stream) {
    Geo g;
    if (dy == nullptr || idx == nullptr || wd == nullptr || dx == nullptr || !geometry(N, H, W, cin, cout, g) ||
        cin < 32)
        return (int)hipErrorInvalidValue;
    ConvArgs a{dy, idx, wd, nullptr, dx, nullptr, (int)H, (int)W, g.Hp, g.Wp, cout, cin, g.tiles_x,
               g.tiles_x * g.tiles_y, gate};
    if (gate != nullptr) {
        if (cin == 32) launch_conv<DGRAD, 2, uint16_t, true>(a, g.blocks, stream);
        else launch_conv<DGRAD, 4, uint16_t, true>(a, g.blocks, stream);
    } else {
        if (cin == 32) launch_conv<DGRAD, 2, uint16_t>(a, g.blocks, stream);
        else launch_conv<DGRAD, 4, uint16_t>(a, g.blocks, stream);
    }
    return (int)hipGetLastError();
}

int conv_wgrad(const void* x, int x_kind, const uint16_t* dy, const uint8_t* idx, const float* gate, int64_t N,
               int64_t H, int64_t W, int cin, int cout, float* part, float* dbpart, float* dW, float* db,
               hipStream_t stream) {
    Geo g;
    if (x == nullptr || dy == nullptr || idx == nullptr || part == nullptr || dbpart == nullptr || dW == nullptr ||
        db == nullptr || !geometry(N, H, W, cin, cout, g) || !kind_ok(cin, x_kind, gate))
        return (int)hipErrorInvalidValue;
    const int P = wgrad_partials(g, cin, cout);
    WgradArgs a{x, dy, idx, part, dbpart, (int)H, (int)W, g.Hp, g.Wp, cin, cout, g.tiles_x, g.tiles_x * g.tiles_y,
                g.blocks, P, gate};
    const dim3 grid(P, cin / 32, cout / 64);
    if (x_kind == 1) launch_wgrad1<uint8_t>(a, stream);
    else if (x_kind == 2) launch_wgrad1<float>(a, stream);
    else if (gate != nullptr)
        hipLaunchKernelGGL((lava_conv_wgrad_kernel<false, uint16_t, true>), grid, dim3(BLOCK), 0, stream, a);
    else
        hipLaunchKernelGGL((lava_conv_wgrad_kernel<false, uint16_t>), grid, dim3(BLOCK), 0, stream, a);
    const int E = 9 * cin * cout + cout;
    hipLaunchKernelGGL(lava_conv_wgrad_reduce_kernel, dim3((E + 63) / 64), dim3(BLOCK), 0, stream, part,
                       dbpart, P, cin, cout, dW, db);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int rt1_lava_conv_supported(int cin, int cout) {
    Geo g;
    return geometry(1, 2, 2, cin, cout, g) ? 1 : 0;
}

extern "C" int rt1_lava_conv_tile_h() { return kTh; }
extern "C" int rt1_lava_conv_tile_w() { return kTw; }

extern "C" int rt1_lava_conv_fwd(const void* x, int x_kind, const uint16_t* wp, const float* bias, int64_t N,
                                 int64_t H, int64_t W, int cin, int cout, uint16_t* y, uint8_t* idx,
                                 hipStream_t stream) {
    return conv_fwd(x, x_kind, wp, bias, nullptr, N, H, W, cin, cout, y, idx, stream);
}

// dx [N, H, W, cin] of a stage with cin >= 32; wd = the weights flipped and transposed, [9][cout][cin]
extern "C" int rt1_lava_conv_dgrad(const uint16_t* dy, const uint8_t* idx, const uint16_t* wd, int64_t N, int64_t H,
                                   int64_t W, int cin, int cout, uint16_t* dx, hipStream_t stream) {
    return conv_dgrad(dy, idx, wd, nullptr, N, H, W, cin, cout, dx, stream);
}

// workgroup partials of the weight gradient: a function of the shape alone, 0 for an unserved one
extern "C" int64_t rt1_lava_conv_wgrad_partials(int64_t N, int64_t H, int64_t W, int cin, int cout) {
    Geo g;
    return geometry(N, H, W, cin, cout, g) ? wgrad_partials(g, cin, cout) : 0;
}

// part fp32 [P][9 * cin][cout], dbpart fp32 [P][cout] (workspaces) -> dW fp32 [cout][cin][3][3], db fp32 [cout]
extern "C" int rt1_lava_conv_wgrad(const void* x, int x_kind, const uint16_t* dy, const uint8_t* idx, int64_t N,
                                   int64_t H, int64_t W, int cin, int cout, float* part, float* dbpart, float* dW,
                                   float* db, hipStream_t stream) {
    return conv_wgrad(x, x_kind, dy, idx, nullptr, N, H, W, cin, cout, part, dbpart, dW, db, stream);
}

// the language-gated stage (cin >= 32), gate fp32 [N, cout]: y = maxpool2(relu(gate[n, c] * (conv(x) + b)))
extern "C" int rt1_lava_conv_gated_fwd(const uint16_t* x, const uint16_t* wp, const float* bias, const float* gate,
                                       int64_t N, int64_t H, int64_t W, int cin, int cout, uint16_t* y, uint8_t* idx,
                                       hipStream_t stream) {
    if (gate == nullptr) return (int)hipErrorInvalidValue;
    return conv_fwd(x, 0, wp, bias, gate, N, H, W, cin, cout, y, idx, stream);
}

extern "C" int rt1_lava_conv_gated_dgrad(const uint16_t* dy, const uint8_t* idx, const uint16_t* wd,
                                         const float* gate, int64_t N, int64_t H, int64_t W, int cin, int cout,
                                         uint16_t* dx, hipStream_t stream) {
    if (gate == nullptr) return (int)hipErrorInvalidValue;
    return conv_dgrad(dy, idx, wd, gate, N, H, W, cin, cout, dx, stream);
}

extern "C" int rt1_lava_conv_gated_wgrad(const uint16_t* x, const uint16_t* dy, const uint8_t* idx, const float* gate,
                                         int64_t N, int64_t H, int64_t W, int cin, int cout, float* part,
                                         float* dbpart, float* dW, float* db, hipStream_t stream) {
    if (gate == nullptr) return (int)hipErrorInvalidValue;
    return conv_wgrad(x, 0, dy, idx, gate, N, H, W, cin, cout, part, dbpart, dW, db, stream);
}

// dgate fp32 [N, cout] from the pooled dy and the stage's own stored output y, both bf16 [N, H / 2, W / 2, cout]
extern "C" int rt1_lava_conv_dgate(const uint16_t* dy, const uint16_t* y, const float* gate, int64_t N, int64_t H,
                                   int64_t W, int cin, int cout, float* dgate, hipStream_t stream) {
    Geo g;
    if (dy == nullptr || y == nullptr || gate == nullptr || dgate == nullptr || !geometry(N, H, W, cin, cout, g) ||
        cin < 32 || (int64_t)g.Hp * g.Wp > INT32_MAX)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(lava_conv_dgate_kernel, dim3((unsigned)N, cout / 64), dim3(BLOCK), 0, stream, dy, y, gate,
                       g.Hp * g.Wp, cout, dgate);
    return (int)hipGetLastError();
}
