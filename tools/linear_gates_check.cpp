// Host-side check of the gate and workspace functions of the projections' weight gradient (include/mvi_unet_ops.h,
// csrc/linear_wgrad.hip): a stand-alone program for a sanitizer build of the HOST code — no GPU is touched: every call below either is
// a pure function of the shape or is declined with the invalid-argument status before anything is launched.
//
//   cd multiview_inpaint_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -I../../include ../../tools/linear_gates_check.cpp linear_wgrad.hip groupnorm_silu.hip -o /tmp/linear_gates_check \
//       && /tmp/linear_gates_check
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

struct Shape { int64_t rows; int32_t K, N; };

int main() {
    const int32_t BF16 = MVI_DT_BF16, F16 = MVI_DT_F16, F32 = MVI_DT_F32;
    // the shape list of tests/test_linear_bwd_gpu.py and the training shapes of tools/bench_linear_bwd.py
    const Shape shapes[] = {{300, 128, 320}, {1, 64, 64}, {64, 64, 64}, {65, 64, 64}, {257, 320, 960}, {513, 1280, 320}, {70001, 64, 128},
                            {14 * 9216, 320, 320}, {28 * 9216, 320, 960}, {28 * 9216, 1280, 320}, {28 * 2304, 640, 640}, {14 * 2304, 640, 1920},
                            {28 * 2304, 2560, 640}, {28 * 576, 1280, 1280}, {14 * 576, 1280, 3840}, {28 * 576, 5120, 1280},
                            {(int64_t)1 << 33, 64, 64}};
    int split = 0, unsplit = 0;
    for (const Shape& s : shapes) {
        for (int32_t dt : {BF16, F16}) CHECK(mvi_linear_wgrad_supported(s.K, s.N, dt) == 1);
        CHECK(mvi_linear_wgrad_supported(s.K, s.N, F32) == 0);
        const size_t ws = mvi_linear_wgrad_workspace_bytes(s.rows, s.K, s.N);
        CHECK(ws == mvi_linear_wgrad_workspace_bytes(s.rows, s.K, s.N));                       // a pure function of the shape
        const size_t slice = ((size_t)s.N * s.K + (size_t)s.N) * sizeof(float);                // S N K 4 + S N 4
        CHECK(ws % slice == 0 && ws / slice != 1 && ws / slice <= 64);
        CHECK(ws / slice <= (size_t)((s.rows + 63) / 64));                                     // never more slices than row chunks
        (ws ? split : unsplit)++;
        CHECK(mvi_linear_wgrad_workspace_bytes(0, s.K, s.N) == 0);
        CHECK(mvi_linear_wgrad_workspace_bytes(-1, s.K, s.N) == 0);
        CHECK(mvi_linear_wgrad_workspace_bytes(s.rows, s.K + 32, s.N) == 0);                   // not this kernel's
        CHECK(mvi_linear_wgrad_workspace_bytes(s.rows, s.K, s.N + 8) == 0);
    }
    CHECK(split > 0 && unsplit > 0);
    CHECK(mvi_linear_wgrad_workspace_bytes(64, 64, 64) == 0 && mvi_linear_wgrad_workspace_bytes(65, 64, 64) > 0);
    CHECK(mvi_linear_wgrad_supported(96, 64, BF16) == 0 && mvi_linear_wgrad_supported(64, 32, BF16) == 0);
    CHECK(mvi_linear_wgrad_supported(0, 64, BF16) == 0 && mvi_linear_wgrad_supported(64, -64, F16) == 0 && mvi_linear_wgrad_supported(64, 64, 7) == 0);

    // declined before any launch: the pointers are never dereferenced on the host, but give them real, aligned storage all the same
    char* buf = static_cast<char*>(std::aligned_alloc(64, 1 << 17));
    float* dw = static_cast<float*>(std::aligned_alloc(64, 64 * 64 * sizeof(float)));
    float* db = static_cast<float*>(std::aligned_alloc(64, 64 * sizeof(float)));
    const int64_t rows = 200;
    const size_t need = mvi_linear_wgrad_workspace_bytes(rows, 64, 64);
    CHECK(need > 0 && need <= (1 << 17));
    CHECK(mvi_linear_wgrad(buf, buf, dw, db, rows, 96, 64, 96, 64, BF16, nullptr, 0, nullptr) == MVI_EINVAL);          // K = 96
    CHECK(mvi_linear_wgrad(buf, buf, dw, db, rows, 64, 32, 64, 32, BF16, nullptr, 0, nullptr) == MVI_EINVAL);          // N = 32
    CHECK(mvi_linear_wgrad(buf, buf, dw, db, rows, 64, 64, 64, 64, F32, nullptr, 0, nullptr) == MVI_EINVAL);           // fp32
    CHECK(mvi_linear_wgrad(buf, buf, dw, db, -1, 64, 64, 64, 64, BF16, nullptr, 0, nullptr) == MVI_EINVAL);
    CHECK(mvi_linear_wgrad(buf + 8, buf, dw, db, rows, 64, 64, 64, 64, BF16, nullptr, 0, nullptr) == MVI_EINVAL);      // misaligned x
    CHECK(mvi_linear_wgrad(buf, buf, dw, db + 1, rows, 64, 64, 64, 64, BF16, nullptr, 0, nullptr) == MVI_EINVAL);      // misaligned dbias
    CHECK(mvi_linear_wgrad(nullptr, buf, dw, db, rows, 64, 64, 64, 64, BF16, nullptr, 0, nullptr) == MVI_EINVAL);
    CHECK(mvi_linear_wgrad(buf, nullptr, dw, db, rows, 64, 64, 64, 64, BF16, nullptr, 0, nullptr) == MVI_EINVAL);
    CHECK(mvi_linear_wgrad(buf, buf, nullptr, db, rows, 64, 64, 64, 64, BF16, nullptr, 0, nullptr) == MVI_EINVAL);
    CHECK(mvi_linear_wgrad(buf, buf, dw, db, rows, 64, 64, 32, 64, BF16, nullptr, 0, nullptr) == MVI_EINVAL);          // stride below the row
    CHECK(mvi_linear_wgrad(buf, buf, dw, db, rows, 64, 64, 64, 68, BF16, nullptr, 0, nullptr) == MVI_EINVAL);          // rows not 16-byte aligned
    CHECK(mvi_linear_wgrad(buf, buf, dw, db, rows, 64, 64, (int64_t)1 << 24, 64, BF16, nullptr, 0, nullptr) == MVI_EINVAL);
    CHECK(mvi_linear_wgrad(buf, buf, dw, db, rows, 64, 64, 64, 64, BF16, buf, need - 4, nullptr) == MVI_EINVAL);       // short workspace
    CHECK(mvi_linear_wgrad(buf, buf, dw, db, rows, 64, 64, 64, 64, BF16, nullptr, need, nullptr) == MVI_EINVAL);       // bytes without a workspace
    CHECK(mvi_linear_wgrad(buf, buf, dw, db, rows, 64, 64, 64, 64, BF16, buf + 4, need, nullptr) == MVI_EINVAL);       // misaligned workspace
    std::free(buf);
    std::free(dw);
    std::free(db);
    std::printf(failures ? "%d check(s) failed\n" : "linear gates: all checks passed (%d split, %d unsplit wgrad shapes)\n",
                failures ? failures : split, unsplit);
    return failures ? 1 : 0;
}
