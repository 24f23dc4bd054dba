// Depthwise k x k convolution (k in {3,5}, stride in {1,2}, pad (k-1)/2) on
// channels-last bf16 activations, with the surrounding BatchNorm work fused
// (26 depthwise convs of the FiLM-EfficientNet-B3; memory-bound,
// vector ALU, not MFMA work).
//
// forward    out = dwconv(act(x*scale + shift))    (BN+SiLU prologue optional)
//            epilogue EPI_STATS: per-workgroup partial (sum, sumsq) of out for the next BN
// bwd data   s=1: the SAME kernel with the kernel flipped (a stride-1 transposed
//            depthwise conv is a correlation with the flipped taps, same padding);
//            s=2: parity-strip kernel (each output strip has one stride-2 phase);
//            epilogue EPI_BNBWD: dz = dx * silu'(y_in*scale+shift), partials of
//            sum dz and sum dz*xhat for the producing BatchNorm's backward
// bwd weight dw[c, tap] = sum dy * act(x*scale+shift), strips of R outputs per thread
//
// Tiling (CDNA4): a 256-thread workgroup owns CV<=8 channel vectors (8 bf16 =
// 16 B, so one pixel's chunk is a 128-B line) x a spatial tile.  The input tile
// + halo is staged ONCE into LDS with the prologue already applied (one exp per
// input element, not k*k), then each thread produces R outputs along W for 8
// channels, streaming the LDS row once per kernel row (weights of that row in
// registers).  Workgroups loop over tiles (grid <= ~8/CU) so the partial rows
// stay few and are reduced by bn_finalize.
//
// This header: what the host-side launch plan (dw_plan.hip) and the kernel units (dw_fwd.hip, dw_bwd_s1.hip,
// dw_bwd_s2.hip) share -- the workgroup size, the kernels' parameter structs and the constants that both a kernel and
// the plan's tile / LDS model depend on.  Plain structs, constants and host declarations, no device code.
#pragma once
#include "../common.h"
#include "dw_plan.h"

namespace rt1 {
namespace dw {

constexpr int BLOCK = 256;
constexpr int EPI_NONE = 0, EPI_STATS = 1, EPI_BNBWD = 2;

struct DwGeo {
    int N, H, W, C, Ho, Wo, k, s, pad;
    int nv;      // C / 8
    int cv;      // channel vectors per workgroup chunk
    int chunks;  // ceil(nv / cv)
};

struct BnBwdEpi {   // producer-BN constants for EPI_BNBWD
    const bf16_t* y;
    const float *scale, *shift, *mean, *rstd;
    int zout;        // unified backward kernels: store dz = dx * silu'(z) instead of dx (pwbwd.hip pw_bwd_z input)
    // unified stride-1 backward without the BN1 epilogue (non-expand residual blocks): dx += res * rmul[n, c], the
    // residual path's gradient (dout * FiLM multiplier) added before the store instead of an add_scaled_ pass
    const bf16_t* res = nullptr;
    const float* rmul = nullptr;
};

// x-mode operand: y1 = x @ we^T is recomputed per staged tile instead of read from HBM (dw_stage.h stage_xmfma)
struct XExp {
    const bf16_t* x;     // [N, H, W, Cin] block input (the depthwise input map's resolution)
    const bf16_t* we;    // [Ce, Cin] bf16 expand weight
    int cin;
};

// Operand of the fused / unified backward kernels: dy is rebuilt from (dA, y2) while staging (dw_stage.h stage_dy)
struct DyBnBwd {   // dy = k1 * (dA * gate + rb) * silu'(y*scale + shift) + k2 * y + k0   (bn_bwd_apply_flat_kernel)
    const bf16_t *dA, *y;
    const float *gate, *rb;                       // [N, C] per-frame
    const float *scale, *shift, *mean, *rstd, *gamma, *mdz, *mdzx;   // [C]
};

// Timing-only builds (tools/bench_dw_phases.py, values wrong): a bit mask of phases removed -- 1 bf16 unpack,
// 2 LDS staging, 4 tap loop, 8 epilogue, 16 backward strip centre, 32 staging loads
#ifndef RT1_DW_TIMING
#define RT1_DW_TIMING 0
#endif

// Occupancy targets (workgroups / CU) the kernels' __launch_bounds__ compile for, each next to the LDS per workgroup
// (KB of the CU's 160) that the plan's tile search keeps to so that this many fit: change a pair together.
// The forward, stride-2 data and weight kernels (DW_LDS_KB) carry their 3 workgroups / CU as a literal.
constexpr int DW_LDS_KB = 52;      // LDS per workgroup the tile search may use (occupancy = 160 KB / this)
constexpr int DWF_OCC = 2;   // workgroups / CU the fused kernel's register budget targets
constexpr int DWF_LDS_KB = 76;     // fused backward: two staged tiles, 2 workgroups / CU
constexpr int DWU_OCC = 2;    // workgroups / CU the unified kernel's register and LDS budgets target
constexpr int DWU_LDS_KB = 76;     // unified backward: one staged dy tile, 2 workgroups / CU
constexpr int DWU2_OCC = 3;   // ... its 2-channel-per-thread k5 form (fewer registers: 3 workgroups / CU)
constexpr int DWU2_LDS_KB = 52;    // ... and its tiles' LDS

// Unified stride-1 backward, y1 in HBM: the tile's strip centres x1 [TH x TW][C8] are copied into LDS by LDS-DMA
// (global_load_lds, no VGPRs, all in flight during the dy staging) instead of global loads at every strip's start that
// each wait a full HBM round trip.  The centre tile's LDS shrinks the dy tile (more halo), so it pays only where the
// tile covers the whole 10 x 10 map anyway: the 2-channel 5-output k5 form, -9 % on blocks 19-23; on the 19 x 19 .. 150 x
// 150 maps the smaller tiles cost 7-27 % (profiles/r6_dw_centre_stage_ab.log).
#ifndef DW_CENTRE_STAGE
#define DW_CENTRE_STAGE 1
#endif
constexpr bool centre_stage_on(int cpt, int r) { return DW_CENTRE_STAGE && cpt == 2 && r == 5; }

// the kernels' view of a plan's geometry
inline DwGeo geo_of(const DwPlan& p) {
    return DwGeo{p.N, p.H, p.W, p.C, p.Ho, p.Wo, p.k, p.s, p.pad, p.nv, p.cv, p.chunks};
}

// The one launch that crosses kernel units: rt1_dw_bwd_fused (dw_bwd_s1.hip) hands a TK_BWD_F plan to the two-pass
// kernel, which lives with the tile-staging kernels it is built from (dw_fwd.hip)
int launch_bwd_twopass(const DwPlan& p, const DyBnBwd& d, const bf16_t* x1, const float* scale1, const float* shift1,
                       int act1, const float* wflip, int grid_x, bf16_t* dx, float* pdz, float* pdzx,
                       const BnBwdEpi& e, bool epi, float* dwp, hipStream_t st);

}  // namespace dw
}  // namespace rt1
