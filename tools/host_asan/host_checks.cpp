// Host-side sanitizer harness (SURVEY §5 "race detection / sanitizers"): the kernels' host code -- tile cost
// models, grid sizing, shape validation -- compiled with AddressSanitizer + UBSan (host only: GPU sanitizers are
// not available on this pool) and swept over every encoder / transformer shape family.  No GPU needed: nothing
// here launches; invalid shapes must be rejected before any launch.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../pytorch_rt1_for_distributed_training_amd/csrc/rt1_kernels.h"

static int failures = 0;
#define EXPECT(c)                                                                   \
    do {                                                                            \
        if (!(c)) {                                                                 \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
            ++failures;                                                             \
        }                                                                           \
    } while (0)

// --dw-plans: every host-side launch decision of the depthwise kernels, one line per case (n, h, w, c, k, s), through
// the extern "C" interface only (tests/test_dw_plan.py compares the output with tests/fixtures/dw_plans.txt):
//   n h w c k s : f<flag> uses_uni, then per max_blocks_x ("/ mb:") dw_grid wgrad_grid bwd_grid | fused grids
//   x<cin>=grid_x/fused grid ... ; T<cin> tile_info(which = 0) , tile_info(which = 1), each TH TW lds sb or E<code>
static void dw_plan_case(int n, int h, int w, int c, int k, int s, std::initializer_list<int> mbs) {
    std::printf("%d %d %d %d %d %d :", n, h, w, c, k, s);
    for (int flag = 0; flag < 2; ++flag) {
        std::printf(" f%d %d%d%d", flag, rt1_dw_bwd_uses_uni(1, flag, flag), rt1_dw_bwd_uses_uni(0, flag, flag),
                    rt1_dw_bwd_uses_uni(1, flag, 1 - flag));
        for (int mb : mbs) {
            std::printf(" / %d: %d %d %d |", mb, rt1_dw_grid(n, h, w, c, k, s, mb, flag, 1 - flag),
                        rt1_dw_wgrad_grid(n, h, w, c, k, s, mb, flag), rt1_dw_bwd_grid(n, h, w, c, k, s, mb, flag));
            if (s == 2) std::printf(" %d", rt1_dw_bwd_fused_s2_grid(n, h, w, c, k, mb, flag, 0));
            else std::printf(" %d %d %d %d", rt1_dw_bwd_fused_grid(n, h, w, c, k, mb, flag, flag, 1, 0),
                             rt1_dw_bwd_fused_grid(n, h, w, c, k, mb, flag, flag, 0, 0),
                             rt1_dw_bwd_fused_grid(n, h, w, c, k, mb, flag, 1 - flag, 1, 0),
                             rt1_dw_bwd_fused_grid(n, h, w, c, k, mb, flag, flag, -1, 0));
            for (int cin : {24, 32, 48}) {
                if (!rt1_dw_x_supported(cin, c, k, s)) continue;
                std::printf(" x%d=%d/%d", cin, rt1_dw_grid_x(n, h, w, c, k, s, cin, mb),
                            s == 2 ? rt1_dw_bwd_fused_s2_grid(n, h, w, c, k, mb, 1, cin)
                                   : rt1_dw_bwd_fused_grid(n, h, w, c, k, mb, 1, 1, 1, cin));
            }
        }
    }
    for (int cin : {0, 24, 32, 48}) {
        if (cin && !rt1_dw_x_supported(cin, c, k, s)) continue;
        std::printf(" ; T%d", cin);
        for (int which = 0; which < 2; ++which) {
            int o[4] = {-1, -1, -1, -1};
            const int rc = rt1_dw_tile_info(which, h, w, c, k, s, cin, o);
            if (rc) std::printf(" E%d", rc);
            else std::printf(" %d %d %d %d", o[0], o[1], o[2], o[3]);
            if (!which) std::printf(" ,");
        }
    }
    std::printf("\n");
}

static int dw_plans() {
    const int res[] = {150, 128, 75, 64, 38, 32, 19, 16, 10, 8, 5, 1};
    const int chans[] = {40, 24, 144, 192, 288, 336, 576, 672, 816, 1152, 1392, 2304, 8, 16};
    // the sweep of main(); frames = 768 only (with the frames = 1 rows the fixture passes 256 KB)
    for (int h : res)
        for (int c : chans)
            for (int k = 3; k <= 5; k += 2)
                for (int s = 1; s <= 2; ++s) {
                    const int w = h + 7 * (h % 3);
                    dw_plan_case(768, h, w, c, k, s, {4096, 64});
                }
    // PLAIN, FUSED_S1 and FUSED_S2 of tests/test_dw_oracle_gpu.py: {N, H, W, C, stride, max_blocks, kernel sizes}
    const int shapes[][7] = {
        {2, 21, 22, 40, 1, 64, 35},  {1, 45, 46, 24, 1, 64, 35},  {1, 46, 45, 24, 1, 64, 35},  {3, 13, 25, 48, 1, 64, 35},
        {4, 10, 10, 136, 1, 64, 35}, {3, 19, 19, 152, 1, 64, 35}, {3, 19, 19, 152, 2, 64, 35}, {2, 19, 21, 288, 1, 64, 35},
        {6, 19, 19, 816, 2, 4, 35},  {8, 10, 10, 1392, 1, 8, 5},  {5, 10, 10, 2304, 1, 5, 3},  {2, 17, 33, 144, 2, 64, 35},
        {2, 20, 30, 144, 2, 64, 35}, {1, 91, 92, 16, 2, 64, 35},
        {5, 10, 10, 2304, 1, 5, 3},  {2, 19, 22, 40, 1, 64, 5},   {1, 45, 46, 24, 1, 64, 5},   {2, 20, 20, 48, 1, 64, 5},
        {3, 19, 19, 152, 1, 64, 5},  {4, 19, 19, 816, 1, 16, 5},  {4, 10, 10, 136, 1, 64, 5},  {3, 15, 25, 96, 1, 64, 5},
        {2, 13, 15, 40, 1, 64, 5},   {8, 10, 10, 1392, 1, 8, 5},
        {2, 17, 23, 40, 2, 64, 35},  {2, 20, 30, 144, 2, 64, 35}, {3, 19, 19, 152, 2, 64, 35}, {2, 38, 38, 288, 2, 2048, 35},
        {1, 91, 92, 16, 2, 64, 35}};
    for (const auto& q : shapes)
        for (int k = 3; k <= 5; k += 2) {
            if (q[6] != 35 && q[6] != k) continue;
            dw_plan_case(q[0], q[1], q[2], q[3], k, q[4], {q[5]});
        }
    // the 26 depthwise layers of the B3 backbone at 300 x 300 input: {map, channels, k, stride, block input channels}
    const int layers[][5] = {{150, 40, 3, 1, 0},    {150, 24, 3, 1, 0},    {150, 144, 3, 2, 24},  {75, 192, 3, 1, 32},
                             {75, 192, 3, 1, 32},   {75, 192, 5, 2, 32},   {38, 288, 5, 1, 48},   {38, 288, 5, 1, 48},
                             {38, 288, 3, 2, 48},   {19, 576, 3, 1, 96},   {19, 576, 3, 1, 96},   {19, 576, 3, 1, 96},
                             {19, 576, 3, 1, 96},   {19, 576, 5, 1, 96},   {19, 816, 5, 1, 136},  {19, 816, 5, 1, 136},
                             {19, 816, 5, 1, 136},  {19, 816, 5, 1, 136},  {19, 816, 5, 2, 136},  {10, 1392, 5, 1, 232},
                             {10, 1392, 5, 1, 232}, {10, 1392, 5, 1, 232}, {10, 1392, 5, 1, 232}, {10, 1392, 5, 1, 232},
                             {10, 1392, 3, 1, 232}, {10, 2304, 3, 1, 384}};
    for (const auto& l : layers)
        for (int n : {768, 6}) {
            dw_plan_case(n, l[0], l[0], l[1], l[2], l[3], {4096, 2048});
            const int cin = l[4];
            if (cin && rt1_dw_x_supported(cin, l[1], l[2], l[3])) {
                int o[4] = {-1, -1, -1, -1};
                const int rc = rt1_dw_tile_info(1, l[0], l[0], l[1], l[2], l[3], cin, o);
                std::printf("L %d %d %d %d %d %d : %d %d | %d %d %d %d %d\n", n, l[0], l[1], l[2], l[3], cin,
                            rt1_dw_grid_x(n, l[0], l[0], l[1], l[2], l[3], cin, 4096),
                            l[3] == 2 ? rt1_dw_bwd_fused_s2_grid(n, l[0], l[0], l[1], l[2], 4096, 1, cin)
                                      : rt1_dw_bwd_fused_grid(n, l[0], l[0], l[1], l[2], 4096, 1, 1, 1, cin),
                            rc, o[0], o[1], o[2], o[3]);
            }
        }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--dw-plans") == 0) return dw_plans();
    // depthwise grids: every (resolution, channel, kernel, stride) family of B3 at three input sizes
    const int res[] = {150, 128, 75, 64, 38, 32, 19, 16, 10, 8, 5, 1};
    const int chans[] = {40, 24, 144, 192, 288, 336, 576, 672, 816, 1152, 1392, 2304, 8, 16};
    const int frames[] = {1, 7, 48, 768};
    long checked = 0;
    for (int n : frames)
        for (int h : res)
            for (int c : chans)
                for (int k = 3; k <= 5; k += 2)
                    for (int s = 1; s <= 2; ++s)
                        for (int flag = 0; flag < 2; ++flag) {
                            const int w = h + 7 * (h % 3);
                            const int g1 = rt1_dw_grid(n, h, w, c, k, s, 4096, flag, 1 - flag);
                            const int g2 = rt1_dw_wgrad_grid(n, h, w, c, k, s, 1024, flag);
                            const int g3 = rt1_dw_bwd_grid(n, h, w, c, k, s, 4096, flag);
                            if (s == 2) EXPECT(rt1_dw_bwd_fused_s2_grid(n, h, w, c, k, 4096, flag, 0) >= 1);
                            else EXPECT(rt1_dw_bwd_fused_grid(n, h, w, c, k, 4096, flag, flag, -1, 0) >= 1);
                            // x-mode tile search (y1-free expand blocks) for the shapes that have a specialisation
                            for (int cin : {24, 32, 48}) {
                                if (!rt1_dw_x_supported(cin, c, k, s)) continue;
                                int info[4];
                                EXPECT(rt1_dw_grid_x(n, h, w, c, k, s, cin, 4096) >= 1);
                                EXPECT(rt1_dw_tile_info(1, h, w, c, k, s, cin, info) == 0 && info[0] >= 1 &&
                                       info[1] >= 1 && info[2] <= 160 * 1024);
                                if (s == 2) EXPECT(rt1_dw_bwd_fused_s2_grid(n, h, w, c, k, 4096, 1, cin) >= 1);
                                else EXPECT(rt1_dw_bwd_fused_grid(n, h, w, c, k, 4096, 1, 1, 1, cin) >= 1);
                            }
                            EXPECT(g1 >= 1 && g1 <= 4096);
                            EXPECT(g2 >= 1 && g2 <= 1024);
                            EXPECT(g3 >= 1 && g3 <= 4096);
                            ++checked;
                        }
    // pointwise GEMM dispatch tables
    for (int K = 8; K <= 2560; K += 8)
        for (int N = 8; N <= 2560; N += 8) {
            if (rt1_pw_gemm_supported(K, N)) {
                const int g = rt1_pw_gemm_grid(1 << 20, K, N, 2048);
                EXPECT(g >= 1 && g <= 2048);
            }
            if (rt1_pw_tall_preferred(K, N)) EXPECT(rt1_pw_tall_supported(K, N));
            if (rt1_pw_tall_supported(K, N)) EXPECT(K > N && N <= 384 && K % 8 == 0);
            rt1_pw_wide_supported(K, N);
            ++checked;
        }
    // unsupported shapes are rejected before any launch (no device, no stream needed)
    EXPECT(rt1_pw_tall(nullptr, nullptr, 1000, 96, 576, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr) != 0);
    EXPECT(rt1_pw_tall(nullptr, nullptr, 0, 576, 96, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr) != 0);
    // the operand prologue needs shift + gate and whole frames (M % hw == 0)
    float dummy = 0.f;
    EXPECT(rt1_pw_tall(nullptr, nullptr, 1000, 576, 96, nullptr, &dummy, &dummy, nullptr, 361, nullptr, nullptr) != 0);
    EXPECT(rt1_pw_tall(nullptr, nullptr, 1000, 576, 96, nullptr, &dummy, &dummy, &dummy, 361, nullptr, nullptr) != 0);  // 1000 % 361
    EXPECT(rt1_embed_fwd(nullptr, nullptr, nullptr, nullptr, 100, 510, 512, 66, nullptr, nullptr) != 0);
    EXPECT(rt1_embed_fwd(nullptr, nullptr, nullptr, nullptr, 100, 512, 500, 66, nullptr, nullptr) != 0);
    for (int ce = 8; ce <= 512; ce += 8)
        for (int ci = 8; ci <= 128; ci += 8) rt1_pw_bwd_supported(ce, ci);
    for (int m : {1, 1000, 1 << 22}) EXPECT(rt1_pw_bwd_grid(m, 512) >= 1);
    for (int n : frames)
        for (int hw : {22500, 5700, 1444, 361, 100, 1})
            for (int c : chans) {
                const int s = rt1_frame_splits(n, hw, c);
                EXPECT(s >= 1);
            }
    for (int n : frames)
        for (int h : {300, 256, 456, 128, 16}) EXPECT(rt1_stem_grid(n, h, h + 40, 8192) >= 1);
    for (int t : {1, 66, 165, 8448, 1 << 20}) EXPECT(rt1_tf_grid(t) >= 1);
    for (int p : {1, 64, 100, 120, 225, 256, 257, 1000}) rt1_tl_supported(p, 512, 64, 8);
    EXPECT(!rt1_tl_supported(257, 512, 64, 8));
    for (int v : {2, 128, 256, 512, 1024, 4096}) rt1_head_ce_supported(v, 512);
    // SE MLP: S > 128, C % 4 != 0 and empty shapes are refused before any launch by both entries and the plan; for
    // every admitted S the se_rowmat request fits the 160 KB of a CU, and whatever passes 64 KB (from S = 102 on
    // 32-frame forward tiles, S = 114 on 16-frame ones) is flagged to raise the kernel's limit first
    {
        const int bad = (int)hipErrorInvalidValue;
        int o[10];
        for (int s : {0, 129, 130, 1 << 20}) {
            EXPECT(rt1_se_fwd(nullptr, 1.f, 16, 128, s, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                              nullptr) == bad);
            EXPECT(rt1_se_bwd_frame(nullptr, nullptr, nullptr, 1.f, 16, 128, s, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, nullptr) == bad);
            EXPECT(rt1_se_plan(16, 128, s, o) == bad);
        }
        EXPECT(rt1_se_fwd(nullptr, 1.f, 16, 130, 8, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr) == bad);
        EXPECT(rt1_se_bwd_frame(nullptr, nullptr, nullptr, 1.f, 0, 128, 8, nullptr, nullptr, nullptr, nullptr, nullptr,
                                nullptr) == bad);
        EXPECT(rt1_se_plan(16, 128, 8, nullptr) == bad);
        for (int n : {1, 16, 352, 353, 512, 513, 768, 1536})
            for (int c : {24, 128, 1392, 2304})
                for (int s = 1; s <= 128; ++s) {
                    EXPECT(rt1_se_plan(n, c, s, o) == 0);
                    for (int b = 0; b < 2; ++b) {
                        const int ft = o[2 + b], lds = o[4 + b];
                        EXPECT(ft == 16 || ft == 32);
                        EXPECT(lds == (ft * s + 128 * (b ? s : (s | 1))) * 4 && lds <= 160 * 1024);
                    }
                    EXPECT(o[9] == (o[4] > 64 * 1024 || o[5] > 64 * 1024));
                    if (s <= 101) EXPECT(o[9] == 0);       // the model stops at 96
                    if (s >= 114) EXPECT(o[9] == 1);
                    if (o[2] == 32) EXPECT(o[9] == (s >= 102));
                    EXPECT(o[0] >= 1 && o[0] <= (c + 63) / 64 && o[1] % 64 == 0 && o[0] * o[1] >= c);
                    EXPECT(o[6] >= 1 && o[6] <= 32 && o[6] * o[7] >= n && (o[6] - 1) * o[7] < n);
                    EXPECT(o[8] >= 1 && o[8] <= 1024);
                    EXPECT(rt1_se_part_size(n, c, s) >= o[0] * n * s);
                    ++checked;
                }
        EXPECT(rt1_se_plan(16, 128, 128, o) == 0 && o[4] == 82432 - 16 * 128 * 4 && o[9] == 1);
        EXPECT(rt1_se_plan(768, 2304, 128, o) == 0 && o[2] == 32 && o[4] == 82432);
    }
    // the regularised head refuses label smoothing outside [0, 1), a negative or non-finite z-loss and an unknown
    // vocabulary, and the hit counter a slot count outside [1, 32] or no rows, all before any launch
    {
        const int bad = (int)hipErrorInvalidValue;
        const float nan = std::strtof("nan", nullptr), inf = std::strtof("inf", nullptr);
        const float opts[][2] = {{1.f, 0.f}, {-0.1f, 0.f}, {0.f, -1e-4f}, {nan, 0.f}, {0.f, nan}, {0.f, inf}, {inf, 0.f}};
        for (const auto& o : opts)
            EXPECT(rt1_head_ce_loss_fwd(nullptr, nullptr, nullptr, nullptr, nullptr, 16, 1, 1, 256, o[0], o[1], nullptr,
                                        nullptr, nullptr, nullptr, nullptr, nullptr) == bad);
        EXPECT(rt1_head_ce_loss_fwd(nullptr, nullptr, nullptr, nullptr, nullptr, 16, 1, 1, 128, 0.1f, 0.f, nullptr,
                                    nullptr, nullptr, nullptr, nullptr, nullptr) == bad);
        EXPECT(rt1_head_ce_loss_fwd(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, 1, 256, 0.1f, 0.f, nullptr,
                                    nullptr, nullptr, nullptr, nullptr, nullptr) == bad);
        for (int a : {0, -1, 33}) EXPECT(rt1_head_token_hits(nullptr, nullptr, 16, a, nullptr, nullptr) == bad);
        EXPECT(rt1_head_token_hits(nullptr, nullptr, 0, 3, nullptr, nullptr) == bad);
    }
    // gradient-norm grid: 1 <= P <= cap for every n >= 1 (no overflow in the grid arithmetic), 0 for n <= 0
    {
        const int cap = 2048;
        for (int64_t n : {(int64_t)0, (int64_t)-1, (int64_t)-(1LL << 40), INT64_MIN}) EXPECT(rt1_gradnorm_partials(n) == 0);
        int64_t sizes[48] = {1, 3, 63, 64, 65, 35233152, (1LL << 31) + 5, INT64_MAX};
        int cnt = 8;
        for (int b = 0; b <= 31; ++b) sizes[cnt++] = 1LL << b;
        int prev = 0;
        for (int k = 0; k < cnt; ++k) {
            const int P = rt1_gradnorm_partials(sizes[k]);
            EXPECT(P >= 1 && P <= cap);
            ++checked;
        }
        for (int b = 0; b <= 31; ++b) {     // monotone in n
            const int P = rt1_gradnorm_partials(1LL << b);
            EXPECT(P >= prev);
            prev = P;
        }
        EXPECT(rt1_gradnorm_partials(35233152) == cap);
        // null pointers and empty buffers are rejected before any launch
        EXPECT(rt1_grad_sumsq(nullptr, 64, nullptr, nullptr) != 0);
        EXPECT(rt1_grad_clip_finalize(nullptr, 0, 1.f, 1.f, 1, nullptr, nullptr) != 0);
        EXPECT(rt1_grad_clip_finalize(nullptr, cap + 1, 1.f, 1.f, 1, nullptr, nullptr) != 0);
        EXPECT(rt1_buffer_guard(nullptr, nullptr, 0, nullptr, nullptr) != 0);
        EXPECT(rt1_flat_adam_dev(nullptr, nullptr, nullptr, nullptr, 64, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 nullptr, 0, 0.9f, 0.999f, 1e-8f, 0.f, 1.f, 1.f, 0, nullptr) != 0);
        // with a state: groups given and n % 64 != 0, and an EMA buffer without ema_state (the pointers are compared
        // with null and never read: every case returns before the launch)
        float buf[8] = {0};
        const uint8_t table[2] = {0, 0};
        EXPECT(rt1_flat_adam_dev(buf, buf, buf, buf, 100, buf, nullptr, nullptr, nullptr, buf, table, 2, 0.9f, 0.999f,
                                 1e-8f, 0.f, 1.f, 1.f, 0, nullptr) == (int)hipErrorInvalidValue);
        EXPECT(rt1_flat_adam_dev(buf, buf, buf, buf, 64, buf, nullptr, buf, nullptr, nullptr, nullptr, 0, 0.9f, 0.999f,
                                 1e-8f, 0.f, 1.f, 1.f, 0, nullptr) == (int)hipErrorInvalidValue);
    }
    std::printf("host checks: %ld shape cases, %d failures\n", checked, failures);
    return failures == 0 ? 0 : 1;
}
