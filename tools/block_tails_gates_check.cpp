// Host-side check of the gate and workspace functions of the block tails' backward (include/mvi_unet_ops.h,
// csrc/block_tails_bwd.hip): a stand-alone program for a sanitizer build of the HOST code — no GPU is touched: every call below either is
// a pure function of the shape or is declined with the invalid-argument status before anything is launched (the zero-size calls
// return before a launch too).
//
//   cd multiview_inpaint_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -I../../include ../../tools/block_tails_gates_check.cpp block_tails_bwd.hip groupnorm_silu.hip -o /tmp/block_tails_gates_check \
//       && /tmp/block_tails_gates_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

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

struct Planes { int64_t N; int32_t C; int64_t S; };
struct Rows { int64_t G, row_div; int32_t C; };

int main() {
    const int32_t BF16 = MVI_DT_BF16, F16 = MVI_DT_F16, F32 = MVI_DT_F32;
    const int32_t DB = MVI_TAILS_DBIAS, DA = MVI_TAILS_DALPHA;
    // the shape lists of tests/test_block_tails_bwd_gpu.py and the training shapes of tools/bench_block_tails_bwd.py
    const Planes planes[] = {{1, 8, 8}, {3, 64, 72}, {2, 72, 64}, {3, 320, 200}, {6, 128, 64}, {14, 320, 9216}, {28, 320, 9216}, {14, 640, 2304},
                             {28, 640, 2304}, {28, 1280, 576}, {14, 1280, 144}, {(int64_t)1 << 20, 1280, 9216}};
    for (const Planes& p : planes) {
        for (int32_t dt : {BF16, F16}) CHECK(mvi_block_tails_backward_supported(p.C, p.S, dt) == 1);
        CHECK(mvi_block_tails_backward_supported(p.C, p.S, F32) == 0);
        const int32_t walk = mvi_planes_tail_backward_walk(p.S);
        const int64_t p_tiles = (p.S + 63) / 64, pg = (p_tiles + walk - 1) / walk, ct = (p.C + 63) / 64;
        CHECK(walk >= 1 && walk <= 8 && pg >= 1);
        CHECK(mvi_planes_tail_backward_workspace_bytes(p.N, p.C, p.S, 0) == 0);                       // nothing to reduce
        CHECK(mvi_planes_tail_backward_workspace_bytes(p.N, p.C, p.S, MVI_TAILS_DTOK | MVI_TAILS_DBASE) == 0);
        const size_t wb = mvi_planes_tail_backward_workspace_bytes(p.N, p.C, p.S, DB);
        const size_t wa = mvi_planes_tail_backward_workspace_bytes(p.N, p.C, p.S, DB | DA);
        CHECK(wb == (size_t)p.N * pg * p.C * 4);
        CHECK(wa == wb + (size_t)p.N * pg * ct * 4);
        CHECK(wa == mvi_planes_tail_backward_workspace_bytes(p.N, p.C, p.S, DA));                      // dalpha reads the column sums too
        CHECK(wb == mvi_planes_tail_backward_workspace_bytes(p.N, p.C, p.S, DB));                      // a pure function of the shape
        CHECK(mvi_planes_tail_backward_workspace_bytes(0, p.C, p.S, DB | DA) == 0);
        CHECK(mvi_planes_tail_backward_workspace_bytes(p.N, p.C, 0, DB | DA) == 0);
        CHECK(mvi_planes_tail_backward_workspace_bytes(p.N, p.C + 4, p.S, DB) == 0);                   // not this kernel's
        CHECK(mvi_planes_tail_backward_workspace_bytes(p.N, p.C, p.S + 4, DB) == 0);
    }
    CHECK(mvi_planes_tail_backward_walk(64) == 1 && mvi_planes_tail_backward_walk(9216) > 1);
    CHECK(mvi_block_tails_backward_supported(0, 64, BF16) == 0 && mvi_block_tails_backward_supported(12, 64, BF16) == 0
          && mvi_block_tails_backward_supported(64, 12, F16) == 0 && mvi_block_tails_backward_supported(64, 64, 7) == 0);
    mvi_planes_tail_backward_set_walk(3);
    CHECK(mvi_planes_tail_backward_walk(9216) == 3 && mvi_planes_tail_backward_walk(64) == 1);        // never more than the tiles there are
    mvi_planes_tail_backward_set_walk(0);
    CHECK(mvi_planes_tail_backward_walk(9216) == 8);

    const Rows rows[] = {{1, 1, 8}, {3, 37, 64}, {2, 64, 320}, {6, 144, 1280}, {14, 9216, 320}, {28, 9216, 320}, {28, 2304, 640}, {28, 576, 1280},
                         {14, 144, 1280}, {(int64_t)1 << 30, 1, 8}};
    for (const Rows& r : rows) {
        const int64_t bpg = mvi_rows_tail_backward_blocks_per_group(r.row_div, r.C);
        CHECK(bpg == (r.row_div * (r.C / 8) + 1023) / 1024);                                          // a function of (row_div, C) alone
        CHECK(mvi_rows_tail_backward_workspace_bytes(r.G * r.row_div, r.C, r.row_div, DA) == (size_t)r.G * bpg * 4);
        CHECK(mvi_rows_tail_backward_workspace_bytes(r.G * r.row_div, r.C, r.row_div, 0) == 0);
        CHECK(mvi_rows_tail_backward_workspace_bytes(0, r.C, r.row_div, DA) == 0);
        CHECK(mvi_rows_tail_backward_workspace_bytes(r.G * r.row_div, r.C + 4, r.row_div, DA) == 0);
    }
    CHECK(mvi_rows_tail_backward_blocks_per_group(0, 64) == 0 && mvi_rows_tail_backward_blocks_per_group(4, 12) == 0);
    CHECK(mvi_rows_tail_backward_workspace_bytes(10, 64, 3, DA) == 0);                                // row_div does not divide R

    // declined before any launch: the pointers are never dereferenced on the host, but give them real, aligned storage all the same
    char* buf = static_cast<char*>(std::aligned_alloc(64, 1 << 16));
    float* f = static_cast<float*>(std::aligned_alloc(64, 4096));
    std::memset(buf, 0x5A, 1 << 16);
    const int64_t N = 2, S = 72;
    const int32_t C = 64;
    const size_t need = mvi_planes_tail_backward_workspace_bytes(N, C, S, DB | DA);
    CHECK(need > 0 && need <= (1 << 16));
    auto planes_call = [&](const void* dy, const float* al, const void* tok, void* dt_, void* dbs, int32_t sums, void* ws, size_t wsb, int64_t n,
                           int32_t c, int64_t s, int32_t dt) { return mvi_planes_tail_backward(dy, al, tok, dt_, dbs, sums, ws, wsb, n, c, s, dt, nullptr); };
    CHECK(planes_call(buf, f, buf, buf, buf, DB | DA, buf, need, N, 60, S, BF16) == MVI_EINVAL);       // C % 8
    CHECK(planes_call(buf, f, buf, buf, buf, DB | DA, buf, need, N, C, 76, BF16) == MVI_EINVAL);       // S % 8
    CHECK(planes_call(buf, f, buf, buf, buf, DB | DA, buf, need, N, C, S, F32) == MVI_EINVAL);         // fp32
    CHECK(planes_call(buf, f, buf, buf, buf, DB | DA, buf, need, -1, C, S, BF16) == MVI_EINVAL);
    CHECK(planes_call(nullptr, f, buf, buf, buf, DB | DA, buf, need, N, C, S, BF16) == MVI_EINVAL);    // no dy
    CHECK(planes_call(buf, nullptr, buf, buf, buf, 0, nullptr, 0, N, C, S, BF16) == MVI_EINVAL);       // d_base without alpha
    CHECK(planes_call(buf, f, nullptr, buf, buf, DA, buf, need, N, C, S, BF16) == MVI_EINVAL);         // dalpha without tok
    CHECK(planes_call(buf, nullptr, buf, buf, nullptr, DA, buf, need, N, C, S, BF16) == MVI_EINVAL);   // dalpha without alpha
    CHECK(planes_call(buf + 8, f, buf, buf, buf, DB, buf, need, N, C, S, BF16) == MVI_EINVAL);         // misaligned dy
    CHECK(planes_call(buf, f, buf, buf + 2, buf, DB, buf, need, N, C, S, F16) == MVI_EINVAL);          // misaligned d_tok
    CHECK(planes_call(buf, f, buf, buf, buf, DB, buf + 4, need, N, C, S, BF16) == MVI_EINVAL);         // misaligned workspace
    CHECK(planes_call(buf, f, buf, buf, buf, DB | DA, buf, need - 4, N, C, S, BF16) == MVI_EINVAL);    // short workspace
    CHECK(planes_call(buf, f, buf, buf, buf, DB, nullptr, need, N, C, S, BF16) == MVI_EINVAL);         // bytes without a workspace
    CHECK(planes_call(buf, f, buf, buf, buf, 0, nullptr, 0, (int64_t)1 << 40, C, S, BF16) == MVI_EINVAL);   // more than 2^31 - 1 blocks
    CHECK(planes_call(buf, f, buf, buf, buf, DB | DA, nullptr, 0, 0, C, S, BF16) == MVI_OK);           // N = 0: nothing launched
    CHECK(planes_call(buf, f, buf, buf, buf, DB | DA, nullptr, 0, N, C, 0, F16) == MVI_OK);            // S = 0
    CHECK(mvi_planes_tail_reduce(buf, need, f, f, f, f, N, 60, S, nullptr) == MVI_EINVAL);
    CHECK(mvi_planes_tail_reduce(buf, need, f, f, nullptr, nullptr, N, C, S, nullptr) == MVI_EINVAL);  // no output
    CHECK(mvi_planes_tail_reduce(buf, need - 4, f, f, f, f, N, C, S, nullptr) == MVI_EINVAL);
    CHECK(mvi_planes_tail_reduce(nullptr, need, f, f, f, f, N, C, S, nullptr) == MVI_EINVAL);
    CHECK(mvi_planes_tail_reduce(buf + 4, need, f, f, f, f, N, C, S, nullptr) == MVI_EINVAL);
    CHECK(mvi_planes_tail_reduce(buf, need, f, f, (float*)((char*)f + 2), f, N, C, S, nullptr) == MVI_EINVAL);

    const int64_t R = 3 * 37;
    const size_t rneed = mvi_rows_tail_backward_workspace_bytes(R, C, 37, DA);
    CHECK(rneed == 3 * 4);
    auto rows_call = [&](const void* dy, const float* al, const void* x, const void* base, void* dt_, int32_t sums, void* ws, size_t wsb, int64_t r,
                         int32_t c, int64_t rd, int32_t dt) { return mvi_rows_tail_backward(dy, al, x, nullptr, base, dt_, dt_, sums, ws, wsb, r, c, rd, dt, nullptr); };
    CHECK(rows_call(buf, f, buf, buf, buf, DA, buf, rneed, R, 60, 37, BF16) == MVI_EINVAL);            // C % 8
    CHECK(rows_call(buf, f, buf, buf, buf, DA, buf, rneed, R, C, 37, F32) == MVI_EINVAL);              // fp32
    CHECK(rows_call(buf, f, buf, buf, buf, DA, buf, rneed, R, C, 0, BF16) == MVI_EINVAL);              // row_div <= 0
    CHECK(rows_call(buf, f, buf, buf, buf, DA, buf, rneed, R, C, -37, BF16) == MVI_EINVAL);
    CHECK(rows_call(buf, f, buf, buf, buf, DA, buf, rneed, R, C, 36, BF16) == MVI_EINVAL);             // R not a multiple of row_div
    CHECK(rows_call(nullptr, f, buf, buf, buf, DA, buf, rneed, R, C, 37, BF16) == MVI_EINVAL);
    CHECK(rows_call(buf, nullptr, buf, buf, buf, DA, buf, rneed, R, C, 37, BF16) == MVI_EINVAL);       // no alpha
    CHECK(rows_call(buf, f, nullptr, buf, buf, DA, buf, rneed, R, C, 37, BF16) == MVI_EINVAL);         // dalpha without x
    CHECK(rows_call(buf, f, buf, nullptr, buf, DA, buf, rneed, R, C, 37, BF16) == MVI_EINVAL);         // dalpha without base
    CHECK(rows_call(buf, f, buf, buf + 8, buf, DA, buf, rneed, R, C, 37, BF16) == MVI_EINVAL);         // misaligned base
    CHECK(rows_call(buf, f, buf, buf, buf, DA, buf, rneed - 4, R, C, 37, BF16) == MVI_EINVAL);         // short workspace
    CHECK(rows_call(buf, f, buf, buf, buf, DA, nullptr, rneed, R, C, 37, BF16) == MVI_EINVAL);
    CHECK(rows_call(buf, f, buf, buf, buf, 0, nullptr, 0, (int64_t)1 << 42, 8, 1, BF16) == MVI_EINVAL);     // more than 2^31 - 1 blocks
    CHECK(rows_call(buf, f, buf, buf, buf, DA, nullptr, 0, 0, C, 37, F16) == MVI_OK);                  // R = 0
    CHECK(mvi_rows_tail_reduce(buf, rneed, nullptr, R, C, 37, nullptr) == MVI_EINVAL);
    CHECK(mvi_rows_tail_reduce(buf, rneed - 4, f, R, C, 37, nullptr) == MVI_EINVAL);
    CHECK(mvi_rows_tail_reduce(buf, rneed, f, R, C, 36, nullptr) == MVI_EINVAL);
    CHECK(mvi_rows_tail_reduce(buf, rneed, f, 0, C, 37, nullptr) == MVI_OK);
    for (size_t i = 0; i < (1 << 16); ++i)
        if ((unsigned char)buf[i] != 0x5A) { CHECK(!"a declined call wrote to its buffers"); break; }
    std::free(buf);
    std::free(f);
    if (failures) std::printf("%d check(s) failed\n", failures);
    else std::printf("block tails gates: all checks passed\n");
    return failures ? 1 : 0;
}
