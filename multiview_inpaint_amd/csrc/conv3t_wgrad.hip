// Weight gradient of the (3, 1, 1) / padding (1, 0, 0) frame convolution (VideoResBlock.time_stack) on token-major activations for
// gfx950, bf16 / f16:
//     dweight[co][ci][kt] = sum over (b, t, p) of dy[b, t, p, co] * x[b, t + kt - 1, p, ci]                  (frame outside [0, T): 0)
// a GEMM per tap with M = C_out, N = C_in and the (frame, pixel) as contraction index. The frame of csrc/conv3x3_wgrad.hip: both
// operands staged row-major ([pixel][channel]) in LDS with rows 160 bytes apart (40 banks: the 8 rows of a 32-lane half of a transposed
// read cover the 64 banks once), BOTH MFMA operands read transposed with ds_read_b64_tr_b16 (element j of lane (c, g) is pixel row
// (j < 4 ? 4 g + j : 16 + 4 g + j - 4) of the 32-pixel step, the same order in A and B), v_mfma_f32_16x16x32, fp32 accumulators.
//
// What differs: the taps are FRAME offsets, +- S rows of the activation, not neighbouring pixels (the 3x3 kernel with H = T, W = S would
// need a halo of two rows of S <= 3072 pixels). The contraction unit is (video b, chunk of kKc = 64 pixels); for it the block walks the
// frames u = 0 .. T - 1, loads the dy chunk and the x chunk of every frame ONCE, keeps the x chunks of frames u - 1, u, u + 1 in a
// three-slot LDS ring (frame f in slot f % 3), and tap kt multiplies dy[u] with x[u + kt - 1].
// Border rule: a tap whose frame lies outside the video is skipped by a block-uniform branch — no mask, no divergent lane; every
// transposed read runs with EXEC all ones on LDS this unit has written (the slot of a skipped frame is never read). The pixel tail of a
// chunk is zero rows in both operands (pad, don't mask) and the 32-pixel steps past it are not run. A chunk never spans two videos, so
// nothing leaks across a video boundary.
// The frames are pipelined through registers: the global loads of dy[u + 1] and x[u + 2] are issued before the products of frame u and
// stored to LDS behind them (two barriers per frame).
//
// Block = 2 waves, a 64 (C_out) x 64 (C_in) tile of all three taps. A wave owns 32 input channels: three accumulator sets of 4 x 2 tiles
// (24 tiles, 96 registers), so a step is 8 transposed reads for the four A fragments shared by the taps and the two channel halves,
// 12 for the six B fragments, 24 MFMAs: 0.83 reads per MFMA against the 1.17 of a 16-channel wave (csrc/conv3x3_wgrad.hip: 0.72 with
// nine taps). 64-channel tiles because the time-stack widths are 320 k; 40 KiB of LDS, so four blocks (8 waves) share a CU.
//
// Split (wgrad_split.h): the output-tile grid alone is (C_out / 64)(C_in / 64) blocks, 25 at 320 x 320. Unit: (video, chunk), B x ceil(S / 64)
// of them; target 1024 blocks; a partial is 3 C_out C_in floats. Addresses are 64-bit throughout.
//
// -Rpass-analysis=kernel-resource-usage (hipcc 7, -O3, the flags of attn_bwd.hip), per instance:
//   conv3t_wgrad_kernel<bf16> and <f16>: 212 VGPRs, 0 AGPRs, 69 SGPRs, no scratch, occupancy 2 waves per SIMD, 40 960 bytes of
//   static LDS per block (four blocks per CU = the 160 KiB).
#include <cstdint>

#include "mfma_common.h"
#include "unet_host.h"
#include "wgrad_split.h"

namespace mvi {
namespace ctw {

constexpr int kBM = 64;                         // C_out per block
constexpr int kBN = 64;                         // C_in per block
constexpr int kWaves = 2;
constexpr int kNT = kBN / (16 * kWaves);        // 16-channel tiles of C_in per wave
constexpr int kThreads = 64 * kWaves;
constexpr int kKc = 64;                         // pixels per chunk
constexpr int kRow = 160;                       // LDS row stride in bytes: 64 channels + 32 bytes of padding
constexpr int kSlot = kKc * kRow;               // one staged chunk
constexpr int kLds = 4 * kSlot;                 // dy + the ring of three x chunks
constexpr int kPassRows = kThreads / 8;         // rows a pass of the block stages (8 pieces of 16 bytes per 64-channel row)
constexpr int kPasses = kKc / kPassRows;
constexpr int kTargetBlocks = 1024;             // four 2-wave blocks (the 160 KiB of LDS) on each of the 256 CUs

template <typename T> using Mma = MmaBuiltin16<T>;

// rows row0 + kPassRows i of a chunk with `valid` pixels: 16 bytes each from `src` (the thread's piece of row 0), zeros past the tail
template <typename T>
__device__ __forceinline__ void load_chunk(u32x4 (&v)[kPasses], const T* src, int64_t C, int row0, int valid) {
#pragma unroll
    for (int i = 0; i < kPasses; ++i) {
        const int row = row0 + kPassRows * i;
        v[i] = u32x4{0u, 0u, 0u, 0u};
        if (row < valid) v[i] = *reinterpret_cast<const u32x4*>(src + (int64_t)row * C);
    }
}

__device__ __forceinline__ void store_chunk(MVI_AS3 char* dst, const u32x4 (&v)[kPasses]) {
#pragma unroll
    for (int i = 0; i < kPasses; ++i) *reinterpret_cast<MVI_AS3 u32x4*>(dst + kPassRows * i * kRow) = v[i];
}

template <typename T>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2)))
void conv3t_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ out, int frames, int S, int C_in, int C_out,
                         int chunks_per_video, int64_t units, int splits) {
    using M = Mma<T>;
    using frag = typename M::frag;
    __shared__ __attribute__((aligned(16))) char smem[kLds];
    MVI_AS3 char* const ldy = (MVI_AS3 char*)smem;
    MVI_AS3 char* const lx = ldy + kSlot;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, g = lane >> 4;
    const int ci_tiles = C_in / kBN;
    const int co0 = ((int)blockIdx.x / ci_tiles) * kBM, ci0 = ((int)blockIdx.x % ci_tiles) * kBN;
    const int s = blockIdx.y;
    const int64_t un_begin = units * s / splits, un_end = units * (s + 1) / splits;

    // transposed read of a 4-row x 16-column block: lane 4 q + p of a 16-lane group addresses row q, columns 4 p .. 4 p + 3
    const uint32_t tr = (uint32_t)((4 * g + (c16 >> 2)) * kRow + 8 * (c16 & 3));
    const uint32_t tr_b = tr + (uint32_t)(32 * kNT * wave);        // the wave's 16 kNT input channels

    f32x4 acc[3][kNT][4];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int nt = 0; nt < kNT; ++nt)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[t][nt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int piece = tid & 7, row0 = tid >> 3;                    // 16-byte piece of a 64-channel row; kPassRows rows per pass
    const uint32_t st_off = (uint32_t)(row0 * kRow + 16 * piece);
    const int64_t dy_frame = (int64_t)S * C_out, x_frame = (int64_t)S * C_in;
    for (int64_t un = un_begin; un < un_end; ++un) {
        const int64_t b = un / chunks_per_video;
        const int p0 = (int)(un - b * chunks_per_video) * kKc;
        const int valid = S - p0 < kKc ? S - p0 : kKc;
        const int nsteps = (valid + 31) >> 5;
        const T* const dyb = dy + ((b * frames) * (int64_t)S + p0) * C_out + co0 + 8 * piece;      // frame 0 of the unit, the thread's piece
        const T* const xb = x + ((b * frames) * (int64_t)S + p0) * C_in + ci0 + 8 * piece;
        u32x4 vd[kPasses], vx[kPasses];
        __syncthreads();                                           // the previous unit's reads are done
        load_chunk(vx, xb, C_in, row0, valid);
        load_chunk(vd, dyb, C_out, row0, valid);
        store_chunk(lx + st_off, vx);                              // x[0] -> slot 0
        store_chunk(ldy + st_off, vd);
        if (frames > 1) {
            load_chunk(vx, xb + x_frame, C_in, row0, valid);
            store_chunk(lx + kSlot + st_off, vx);                  // x[1] -> slot 1
        }
#pragma unroll 1
        for (int u = 0; u < frames; ++u) {
            const bool more_dy = u + 1 < frames, more_x = u + 2 < frames;
            if (more_dy) load_chunk(vd, dyb + (u + 1) * dy_frame, C_out, row0, valid);
            if (more_x) load_chunk(vx, xb + (u + 2) * x_frame, C_in, row0, valid);
            __syncthreads();                                       // dy[u] and x[u + 1] are staged

#pragma unroll 1
            for (int st = 0; st < nsteps; ++st) {
                const uint32_t so = (uint32_t)(32 * st * kRow);
                frag a[4];
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) a[mt] = read_frag_tr<frag>(ldy + so + tr + 32 * mt, 16 * kRow);
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const int f = u + t - 1;                       // the x frame of tap t
                    if (f < 0 || f >= frames) continue;            // block-uniform: outside the video
                    const uint32_t to = (uint32_t)((f % 3) * kSlot) + so + tr_b;
#pragma unroll
                    for (int nt = 0; nt < kNT; ++nt) {
                        const frag bb = read_frag_tr<frag>(lx + to + 32 * nt, 16 * kRow);
#pragma unroll
                        for (int mt = 0; mt < 4; ++mt) acc[t][nt][mt] = M::mfma(a[mt], bb, acc[t][nt][mt]);
                    }
                }
            }

            if (more_dy) {
                __syncthreads();                                   // frame u's reads are done: dy[u] and slot (u - 1) % 3 are free
                store_chunk(ldy + st_off, vd);
                if (more_x) store_chunk(lx + ((u + 2) % 3) * kSlot + st_off, vx);
            }
        }
    }

    // register i of lane (c, g) of tile (t, nt, mt) = dweight[co0 + 16 mt + 4 g + i][ci0 + 16 (kNT wave + nt) + c][tap t]
    float* const op = out + (int64_t)s * C_out * C_in * 3 + ((int64_t)(co0 + 4 * g) * C_in + ci0 + 16 * kNT * wave + c16) * 3;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int nt = 0; nt < kNT; ++nt)
#pragma unroll
                for (int t = 0; t < 3; ++t) op[((int64_t)(16 * mt + i) * C_in + 16 * nt) * 3 + t] = acc[t][nt][mt][i];
}

static bool shape_ok(int64_t B, int32_t T, int32_t S, int32_t C_in, int32_t C_out) {
    return B >= 0 && T >= 1 && S >= 1 && C_in > 0 && C_out > 0 && C_in % kBN == 0 && C_out % kBM == 0 && B < (1ll << 31) &&
           (int64_t)(C_in / kBN) * (C_out / kBM) <= 0x7FFFFFFFll;
}

// chunks of one video: what the kernel indexes by
static int chunks_per_video(int32_t S) { return (S + kKc - 1) / kKc; }

static int splits_of(int64_t B, int cpv, int32_t C_in, int32_t C_out) {
    return split_count(B * cpv, (int64_t)(C_in / kBN) * (C_out / kBM), kTargetBlocks);
}

template <typename T>
static int launch(const void* x, const void* dy, float* dweight, int64_t B, int frames, int S, int C_in, int C_out, void* ws, size_t ws_bytes,
                  hipStream_t st) {
    const int cpv = chunks_per_video(S);
    int R = splits_of(B, cpv, C_in, C_out);
    const int64_t total = (int64_t)C_out * C_in * 3;
    if (R > 1 && (!ws || ws_bytes < (size_t)R * total * sizeof(float))) R = 1;          // a short workspace: the unsplit launch (linear_wgrad.hip refuses)
    const unsigned tiles = (unsigned)((C_in / kBN) * (C_out / kBM));
    hipLaunchKernelGGL(conv3t_wgrad_kernel<T>, dim3(tiles, (unsigned)R), dim3(kThreads), 0, st, (const T*)x, (const T*)dy,
                       R > 1 ? (float*)ws : dweight, frames, S, C_in, C_out, cpv, B * cpv, R);
    if (hipGetLastError() != hipSuccess) return MVI_EHIP;
    return R > 1 ? wgrad_reduce((const float*)ws, dweight, nullptr, total, 0, R, st) : 0;
}

}  // namespace ctw
}  // namespace mvi

extern "C" int mvi_conv3t_wgrad_supported(int32_t C_in, int32_t C_out, int32_t dtype) {
    return C_in > 0 && C_out > 0 && C_in % mvi::ctw::kBN == 0 && C_out % mvi::ctw::kBM == 0 && (dtype == MVI_DT_BF16 || dtype == MVI_DT_F16);
}

extern "C" size_t mvi_conv3t_wgrad_workspace_bytes(int64_t B, int32_t T, int32_t pixels, int32_t C_in, int32_t C_out) {
    if (!mvi::ctw::shape_ok(B, T, pixels, C_in, C_out) || B == 0) return 0;
    const int R = mvi::ctw::splits_of(B, mvi::ctw::chunks_per_video(pixels), C_in, C_out);
    return R > 1 ? (size_t)R * (size_t)C_out * C_in * 3 * sizeof(float) : 0;
}

extern "C" int mvi_conv3t_wgrad(const void* x, const void* dy, float* dweight, int64_t B, int32_t T, int32_t pixels, int32_t C_in,
                                int32_t C_out, int32_t dtype, void* workspace, size_t workspace_bytes, void* stream) {
    if (!mvi_conv3t_wgrad_supported(C_in, C_out, dtype) || !mvi::ctw::shape_ok(B, T, pixels, C_in, C_out))
        return mvi::unet_fail(MVI_EINVAL, "conv3t wgrad: needs C_in and C_out multiples of 64, bf16 or f16, T >= 1, pixels >= 1");
    if (!dweight || ((!x || !dy) && B > 0)) return mvi::unet_fail(MVI_EINVAL, "conv3t wgrad: NULL pointer");   // (mvi_conv3x3_wgrad rejects these with B == 0 too)
    if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dweight | (uintptr_t)workspace) % 16)
        return mvi::unet_fail(MVI_EINVAL, "conv3t wgrad: x, dy, dweight and workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (B == 0)                                                    // (an empty tensor may have no address)
        return hipMemsetAsync(dweight, 0, (size_t)C_out * C_in * 3 * sizeof(float), st) == hipSuccess ? MVI_OK : MVI_EHIP;
    const int rc = mvi::dispatch_dtype16(dtype, "conv3t wgrad: unknown dtype", [&](auto t) {
        return mvi::ctw::launch<typename decltype(t)::type>(x, dy, dweight, B, T, pixels, C_in, C_out, workspace, workspace_bytes, st);
    });
    return rc == MVI_EHIP ? mvi::unet_fail(rc, "conv3t wgrad: kernel launch failed") : rc;
}
