// Host-side check of the gate and workspace functions of the resampling-convolution backward (include/mvi_unet_ops.h): a stand-alone
// program for a sanitizer build of the HOST code — no GPU is touched: every call below either is a pure function of the shape or is
// declined with the invalid-argument status before anything is launched.
//
//   cd multiview_inpaint_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -I../../include ../../tools/resample_gates_check.cpp linear_n320.hip conv3x3_wgrad.hip token_rows.hip ff_geglu.hip \
//       groupnorm_silu.hip -o /tmp/resample_gates_check && /tmp/resample_gates_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "mvi_raster.h"      // MVI_OK, MVI_EINVAL
#include "mvi_unet_ops.h"

static int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);       \
            ++failures;                                              \
        }                                                            \
    } while (0)

struct Shape { int64_t N; int32_t H, W, Ci, Co; };

int main() {
    const int32_t BF16 = MVI_DT_BF16, F16 = MVI_DT_F16, F32 = MVI_DT_F32;
    // the shape lists of tests/test_resample_conv_bwd_gpu.py and the training shapes
    const Shape wgrad[] = {{1, 2, 2, 64, 64}, {5, 2, 2, 64, 64}, {2, 6, 10, 128, 64}, {1, 2, 256, 64, 64}, {3, 18, 32, 320, 320}, {1, 40, 34, 192, 320},
                           {14, 72, 128, 320, 320}, {14, 36, 64, 640, 640}, {14, 18, 32, 1280, 1280}, {28, 72, 128, 320, 320}};
    const Shape dgrad[] = {{1, 2, 2, 320, 64}, {2, 6, 10, 320, 128}, {3, 10, 14, 320, 192}, {1, 18, 32, 640, 640}, {2, 4, 6, 960, 320},
                           {14, 72, 128, 320, 320}, {14, 36, 64, 640, 640}, {14, 18, 32, 1280, 1280}};
    int split = 0, unsplit = 0;
    for (const Shape& s : wgrad) {
        for (int32_t dt : {BF16, F16}) CHECK(mvi_conv3x3_s2_wgrad_supported(s.Ci, s.Co, dt) == 1);
        CHECK(mvi_conv3x3_s2_wgrad_supported(s.Ci, s.Co, F32) == 0);
        const size_t ws = mvi_conv3x3_s2_wgrad_workspace_bytes(s.N, s.H, s.W, s.Ci, s.Co);
        CHECK(ws == mvi_conv3x3_s2_wgrad_workspace_bytes(s.N, s.H, s.W, s.Ci, s.Co));          // a pure function of the shape
        CHECK(ws % ((size_t)s.Ci * s.Co * 9 * sizeof(float)) == 0 && ws / ((size_t)s.Ci * s.Co * 9 * sizeof(float)) <= 64);
        (ws ? split : unsplit)++;
        CHECK(mvi_conv3x3_s2_wgrad_workspace_bytes(s.N, s.H + 1, s.W, s.Ci, s.Co) == 0);       // odd H / W: not this kernel's
        CHECK(mvi_conv3x3_s2_wgrad_workspace_bytes(s.N, s.H, s.W + 1, s.Ci, s.Co) == 0);
        CHECK(mvi_conv3x3_s2_wgrad_workspace_bytes(0, s.H, s.W, s.Ci, s.Co) == 0);
    }
    CHECK(split > 0 && unsplit > 0);
    CHECK(mvi_conv3x3_s2_wgrad_workspace_bytes(1, 2, 258, 64, 64) == 0);
    CHECK(mvi_conv3x3_s2_wgrad_supported(72, 64, BF16) == 0 && mvi_conv3x3_s2_wgrad_supported(64, 96, BF16) == 0);
    for (const Shape& s : dgrad) {
        for (int32_t dt : {BF16, F16}) CHECK(mvi_conv3x3_s2_dgrad_supported(s.Ci, s.Co, dt) == 1);
        CHECK(mvi_conv3x3_s2_dgrad_supported(s.Ci, s.Co, F32) == 0);
    }
    CHECK(mvi_conv3x3_s2_dgrad_supported(64, 320, BF16) == 0 && mvi_conv3x3_s2_dgrad_supported(320, 72, BF16) == 0);

    // declined before any launch: the pointers are never dereferenced on the host, but give them real, aligned storage all the same
    void* buf = std::aligned_alloc(64, 1 << 16);
    float* dw = static_cast<float*>(std::aligned_alloc(64, 64 * 64 * 9 * sizeof(float)));
    const int32_t bad[][5] = {{3, 4, 64, 64, BF16}, {4, 5, 64, 64, BF16}, {4, 4, 72, 64, BF16}, {4, 4, 64, 96, BF16}, {4, 4, 64, 64, F32}, {2, 258, 64, 64, BF16}};
    for (const auto& b : bad) CHECK(mvi_conv3x3_s2_wgrad(buf, buf, dw, 1, b[0], b[1], b[2], b[3], b[4], nullptr, 0, nullptr) == MVI_EINVAL);
    CHECK(mvi_conv3x3_s2_wgrad(nullptr, buf, dw, 1, 4, 4, 64, 64, BF16, nullptr, 0, nullptr) == MVI_EINVAL);
    CHECK(mvi_conv3x3_s2_dgrad(buf, buf, buf, 1, 3, 4, 320, 64, 256, 320, BF16, nullptr) == MVI_EINVAL);
    CHECK(mvi_conv3x3_s2_dgrad(buf, buf, buf, 1, 4, 3, 320, 64, 256, 320, BF16, nullptr) == MVI_EINVAL);
    CHECK(mvi_conv3x3_s2_dgrad(buf, buf, buf, 1, 4, 6, 64, 320, 256, 64, BF16, nullptr) == MVI_EINVAL);
    CHECK(mvi_conv3x3_s2_dgrad(buf, buf, buf, 1, 4, 6, 320, 64, 0, 320, BF16, nullptr) == MVI_EINVAL);           // no room for a block
    CHECK(mvi_conv3x3_s2_dgrad(buf, buf, buf, 1, 4, 6, 320, 64, 256, 320, F32, nullptr) == MVI_EINVAL);
    CHECK(mvi_rows_pool2x2_sum(buf, buf, 1, 1, 1, 12, BF16, nullptr) == MVI_EINVAL);
    CHECK(mvi_rows_pool2x2_sum(buf, buf, 1, 1, 1, 8, F32, nullptr) == MVI_EINVAL);
    CHECK(mvi_rows_pool2x2_sum(buf, buf, 1, 0, 1, 8, BF16, nullptr) == MVI_EINVAL);
    CHECK(mvi_rows_pool2x2_sum(nullptr, buf, 1, 1, 1, 8, BF16, nullptr) == MVI_EINVAL);
    CHECK(mvi_rows_pool2x2_sum(buf, buf, 0, 1, 1, 8, BF16, nullptr) == MVI_OK);                                  // nothing to do
    std::free(buf);
    std::free(dw);
    std::printf(failures ? "%d check(s) failed\n" : "resample gates: all checks passed (%d split, %d unsplit wgrad shapes)\n",
                failures ? failures : split, unsplit);
    return failures ? 1 : 0;
}
