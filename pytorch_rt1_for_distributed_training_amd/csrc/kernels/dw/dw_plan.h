// Launch plan of one depthwise op (host only).  dw_plan() is the single place that turns a request into geometry,
// kernel family, strip shape, tile, LDS bytes and grid: the grid helpers the caller sizes its per-workgroup partial
// buffers from, rt1_dw_tile_info and every launcher read the same struct, so they cannot pick different tiles.
#pragma once

namespace rt1 {
namespace dw {

enum Op : int { OP_FWD = 0, OP_FWD_X, OP_BWD_DATA, OP_BWD_WEIGHT, OP_BWD_FUSED_S1, OP_BWD_FUSED_S2 };

enum TileKind : int {
    TK_FWD = 0, TK_BWD_W = 1, TK_BWD_S2 = 2, TK_BWD_F = 3, TK_BWD_U4 = 4, TK_BWD_U8 = 5, TK_BWD_V4 = 6, TK_BWD_V8 = 7,
    TK_BWD_U2 = 8
};   // U: unified stride-1 backward, V: unified stride-2 backward (2 / 4 / 8 channels per thread)
inline bool is_uni(int kind) { return kind == TK_BWD_U4 || kind == TK_BWD_U8 || kind == TK_BWD_U2; }

constexpr int DW_R1 = 4;      // outputs per thread strip for the stride-1 forward / weight-grad kernels
// unified backward (dw_bwd_uni_kernel): channels per thread and strip length per kernel size
constexpr int DWU_CPT3 = 8;
constexpr int DWU_R3 = 2;
constexpr int DWU_CPT5 = 4;
constexpr int DWU_R5 = 4;
constexpr int DWV_CPT3 = 8;
constexpr int DWV_R3 = 2;
constexpr int DWV_CPT5 = 4;
constexpr int DWV_R5 = 4;

// The x-mode specialisations X(k, xk) per stride (xk = KC * 16 + NG, xk_of): the only (kernel size, key) pairs with
// compiled kernels.  rt1_dw_x_supported, the forward-x dispatch and both unified-backward dispatches expand from
// these lists, so a key accepted by the first cannot be missing from a dispatch.
#define DW_XMODE_S1(X) X(3, 0x14) X(5, 0x26)
#define DW_XMODE_S2(X) X(3, 0x19) X(3, 0x13) X(3, 0x11) X(3, 0x26) X(5, 0x14)

struct DwPlan {
    int err;        // 0, or hipErrorInvalidValue: no kernel for this request (the other fields are still filled)
    int N, H, W, C, Ho, Wo, k, s, pad, nv, cv, chunks;   // geometry (DwGeo)
    int kind;       // TileKind
    int xk;         // x-mode key, 0 = the depthwise input is read from HBM
    int R;          // outputs per thread strip
    int cpt;        // channels per thread
    int ring;       // the staging walks only the in-image rectangle of its window (maps <= DW_RING_PIX pixels)
    int TH, TW;     // tile
    int sb;         // x-mode stride-1 backward: strips per band (0 = all)
    int lds;        // dynamic LDS bytes
    int red_taps;   // unified backward: weight taps per reduction pass
    int grid_x;     // workgroups along x (grid.y = chunks)
};

// pro / epi: the BN(+SiLU) operand prologue and the BN-backward epilogue of the variant that will run; variant: fused
// stride-1 backward only (0 = two-pass kernel, otherwise unified); cin > 0 asks for x-mode (OP_FWD_X and the fused
// backwards).  Pure; the tile search behind it is memoised per thread.
DwPlan dw_plan(int op, int N, int H, int W, int C, int k, int s, int pro, int epi, int variant, int cin,
               int max_blocks_x);

}  // namespace dw
}  // namespace rt1
