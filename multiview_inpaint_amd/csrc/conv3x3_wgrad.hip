// Weight gradient of the 3x3 / padding 1 / stride 1 convolution on token-major activations for gfx950, bf16 / f16:
//     dweight[co][ci][ky][kx] = sum over (n, y, x) of dy[n, y, x, co] * x[n, y + ky - 1, x + kx - 1, ci]      (outside the image: 0)
// a GEMM per tap with M = C_out, N = C_in and the PIXEL as contraction index — the slow axis of both operands in memory. Both are
// staged row-major ([pixel][channel]) in LDS and BOTH MFMA operands are read transposed with ds_read_b64_tr_b16 (ff_geglu_bwd.hip
// reads its A operand this way): element j of lane (c, g) is pixel row (j < 4 ? 4 g + j : 16 + 4 g + j - 4) of the 32-pixel step,
// the same order in A and B.
//
// The border rule lives in the LDS images, not in the loop. An image is walked in a PADDED linear pixel space with rows of
// P = W + 2 positions: dy at position q = r P + c is dy[n, r, c] for c < W and 0 for the two pad positions; x at position
// q' = rr P + cc is x[n, rr - 1, cc - 1], 0 outside the image (the forward's tap_ok rule). Then tap (ky, kx) of dy position q reads
// x position q + ky P + kx: the nine taps are nine ROW OFFSETS into one x image, the pad positions of dy annihilate what wraps
// round a row end, and the loop has no mask and no divergence (every transposed read runs with EXEC all ones on addresses inside
// the initialised image; pad, don't mask). Cost: (W + 2) / W more contraction steps (3 % at W = 64, 25 % at W = 8).
//
// Block = 4 waves, a 64 (C_out) x 64 (C_in) tile of all nine taps. Per chunk of kKc = 160 padded positions of one image it loads the
// dy rows once (160 x 64 channels) and the x rows with their halo once (160 + 2 P + 2 rows), then runs 5 steps of 32 pixels. A wave
// owns 16 input channels: NINE ACCUMULATOR SETS (nine taps x four 16 x 16 tiles of C_out = 36 tiles, 144 registers), so a step is
// 8 transposed reads for the four A fragments shared by the taps, 18 for the nine B fragments, 36 MFMAs. Nine passes would have
// needed the accumulators of one tap at a time and so either nine loads of dy or a write of partials per chunk.
// LDS rows are 160 bytes apart (40 banks: the 8 rows of a 32-lane half of a transposed read cover the 64 banks once).
//
// Split (wgrad_split.h): the output-tile grid alone is (C_out / 64)(C_in / 64) blocks, 25 at 320 x 320. Unit: a chunk, N x ceil(H P / 160)
// of them (kS2: N x ceil((H / 2)(W / 2 + 1) / 64)); target 512 blocks; a partial is 9 C_out C_in floats. Addresses are 64-bit throughout.
//
// -Rpass-analysis=kernel-resource-usage (hipcc 7, -O3, the flags of attn_bwd.hip), per instance:
//   conv3x3_wgrad_kernel<bf16> and <f16>: 196 VGPRs, 0 AGPRs, 69 SGPRs, no scratch, occupancy 2 waves per SIMD;
//   LDS dynamic, 160 (2 kKc + 2 P + 2) bytes: 72 640 at W = 64 (two blocks per CU), 56 000 at W = 12; W <= 256 (134 400).
//
// kS2: the weight gradient of the STRIDE-2 convolution (mvi_conv3x3_s2_wgrad; H, W even, dy [N, (H / 2)(W / 2), C_out]):
//     dweight[co][ci][ky][kx] = sum over (n, r, c) of dy[n, r, c, co] * x[n, 2 r + ky - 1, 2 c + kx - 1, ci]      (outside the image: 0)
// (the stride-1 formula with the zero-stuffed dy, the zeros left out). The stride, like the border rule, lives in the LDS images: dy
// is walked in its OWN padded position space with rows of P = W / 2 + 1 positions (position q = r P + c is dy[n, r, c] for c < W / 2
// and 0 at the one pad position), and x is staged as FOUR PARITY PLANES in the same space: plane (pr, pc) at position rr P + cc is
// x[n, 2 rr - pr, 2 cc - pc], 0 outside the image — the odd planes carry the border's zero row / column at rr = 0 / cc = 0, the even-
// column planes a zero at the pad position cc = W / 2. Tap ky reads row 2 r - 1 (odd plane, rr = r), 2 r (even plane, rr = r) or
// 2 r + 1 (odd plane, rr = r + 1), columns likewise: every tap is a (plane, constant offset) pair — offset (ky == 2) P + (kx == 2) —
// and the inner loop is the stride-1 kernel's: no mask, no wasted step, every transposed read with EXEC all ones on initialised LDS.
// The other staging considered — the dy image zero-stuffed in the stride-1 position space, the smallest change — multiplies three
// zeros for every value and measured 0.04 - 0.08 of the matrix peak; this one costs four x images, two of them a row
// longer than the chunk, so its chunk is kKcS2 = 64 positions: 160 (5 kKcS2 + 2 P + 8) bytes = 73 280 at W = 128, two blocks per CU.
//   conv3x3_wgrad_kernel<bf16, true> and <f16, true>: 196 VGPRs, 0 AGPRs, 88 SGPRs, no scratch, occupancy 2 waves per SIMD.
#include <cstdint>

#include "mfma_common.h"
#include "unet_host.h"
#include "wgrad_split.h"

namespace mvi {
namespace cwg {

constexpr int kBM = 64;                         // C_out per block
constexpr int kBN = 64;                         // C_in per block (16 per wave)
constexpr int kWaves = 4;
constexpr int kKc = 160;                        // padded pixel positions per chunk
constexpr int kSteps = kKc / 32;
constexpr int kKcS2 = 64;                       // kS2: dy positions per chunk (the four x planes have to fit beside them)
constexpr int kRow = 160;                       // LDS row stride in bytes: 64 channels + 32 bytes of padding
constexpr int kMaxW = 256;
constexpr int kTargetBlocks = 512;              // two blocks on each of the 256 CUs

template <typename T> using Mma = MmaBuiltin16<T>;

__host__ __device__ constexpr int x_rows(int W) { return kKc + 2 * (W + 2) + 2; }
// kS2: rows of an even-row plane (taps reach one position past the chunk) and of an odd-row plane (one row of P = W / 2 + 1 more)
__host__ __device__ constexpr int s2_even_rows() { return kKcS2 + 2; }
__host__ __device__ constexpr int s2_odd_rows(int W) { return kKcS2 + (W / 2 + 1) + 2; }
__host__ __device__ constexpr int s2_lds_rows(int W) { return kKcS2 + 2 * s2_even_rows() + 2 * s2_odd_rows(W); }

template <typename T, bool kS2 = false>
__global__ __launch_bounds__(64 * kWaves) __attribute__((amdgpu_waves_per_eu(2, 2)))
void conv3x3_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ out, int H, int W, int C_in, int C_out,
                          int chunks_per_image, int64_t chunks, int splits) {
    using M = Mma<T>;
    using frag = typename M::frag;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    MVI_AS3 char* const ldy = (MVI_AS3 char*)smem;
    constexpr int KC = kS2 ? kKcS2 : kKc, STEPS = KC / 32;         // positions per chunk, 32-position steps
    MVI_AS3 char* const lx = ldy + KC * kRow;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, g = lane >> 4;
    const int ci_tiles = C_in / kBN;
    const int co0 = ((int)blockIdx.x / ci_tiles) * kBM, ci0 = ((int)blockIdx.x % ci_tiles) * kBN;
    const int s = blockIdx.y;
    const int64_t ch_begin = chunks * s / splits, ch_end = chunks * (s + 1) / splits;
    const int P = kS2 ? (W >> 1) + 1 : W + 2;
    const int XR = x_rows(W);
    // kS2: first LDS row of plane 2 pr + pc behind lx — (even, even) | (even, odd) | (odd, even) | (odd, odd)
    const int pl_rows[4] = {s2_even_rows(), s2_even_rows(), s2_odd_rows(W), s2_odd_rows(W)};
    const int pl_base[4] = {0, s2_even_rows(), 2 * s2_even_rows(), 2 * s2_even_rows() + s2_odd_rows(W)};

    // transposed read of a 4-row x 16-column block: lane 4 q + p of a 16-lane group addresses row q, columns 4 p .. 4 p + 3
    const uint32_t tr = (uint32_t)((4 * g + (c16 >> 2)) * kRow + 8 * (c16 & 3));
    const uint32_t tr_b = tr + (uint32_t)(32 * wave);              // the wave's 16 input channels

    f32x4 acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int piece = tid & 7, row0 = tid >> 3;                    // 16-byte piece of a 64-channel row; 32 rows per pass of the block
    for (int64_t ch = ch_begin; ch < ch_end; ++ch) {
        const int64_t n = ch / chunks_per_image;
        const int q0 = (int)(ch - n * chunks_per_image) * KC;
        const T* const dyn = (kS2 ? dy + n * (H >> 1) * (W >> 1) * (int64_t)C_out : dy + n * H * W * (int64_t)C_out) + co0 + 8 * piece;
        const T* const xn = x + n * H * W * (int64_t)C_in + ci0 + 8 * piece;
        __syncthreads();                                           // the previous chunk's reads are done
        u32x4 v[STEPS];
#pragma unroll
        for (int i = 0; i < STEPS; ++i) {
            const int q = q0 + row0 + 32 * i;
            const int r = q / P, c = q - r * P;
            v[i] = u32x4{0u, 0u, 0u, 0u};
            if (kS2) {                                             // dy's own (H / 2) x (W / 2) image, one pad position per row
                if (r < (H >> 1) && c < (W >> 1)) v[i] = *reinterpret_cast<const u32x4*>(dyn + (int64_t)(r * (W >> 1) + c) * C_out);
            } else
            if (r < H && c < W) v[i] = *reinterpret_cast<const u32x4*>(dyn + (int64_t)(r * W + c) * C_out);
        }
#pragma unroll
        for (int i = 0; i < STEPS; ++i) *reinterpret_cast<MVI_AS3 u32x4*>(ldy + (row0 + 32 * i) * kRow + 16 * piece) = v[i];
        if (kS2) {
#pragma unroll
            for (int pl = 0; pl < 4; ++pl) {
                const int pr = pl >> 1, pc = pl & 1;
#pragma unroll 2
                for (int row = row0; row < pl_rows[pl]; row += 32) {
                    const int q = q0 + row;
                    const int rr = q / P, cc = q - rr * P;
                    const int y = 2 * rr - pr, xc = 2 * cc - pc;                     // (-1: the border's zero row / column; xc = W: the pad)
                    u32x4 w = u32x4{0u, 0u, 0u, 0u};
                    if (y >= 0 && y < H && xc >= 0 && xc < W) w = *reinterpret_cast<const u32x4*>(xn + (int64_t)(y * W + xc) * C_in);
                    *reinterpret_cast<MVI_AS3 u32x4*>(lx + (pl_base[pl] + row) * kRow + 16 * piece) = w;
                }
            }
        } else
#pragma unroll 4
        for (int row = row0; row < XR; row += 32) {
            const int q = q0 + row;
            const int rr = q / P, cc = q - rr * P;
            u32x4 w = u32x4{0u, 0u, 0u, 0u};
            if (rr >= 1 && rr <= H && cc >= 1 && cc <= W) w = *reinterpret_cast<const u32x4*>(xn + (int64_t)((rr - 1) * W + cc - 1) * C_in);
            *reinterpret_cast<MVI_AS3 u32x4*>(lx + row * kRow + 16 * piece) = w;
        }
        __syncthreads();

#pragma unroll 1
        for (int st = 0; st < STEPS; ++st) {
            const uint32_t so = (uint32_t)(32 * st * kRow);
            frag a[4];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) a[mt] = read_frag_tr<frag>(ldy + so + tr + 32 * mt, 16 * kRow);
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                // kS2: tap (ky, kx) = plane (ky != 1, kx != 1) at offset (ky == 2) P + (kx == 2)
                const uint32_t to = so + tr_b + (kS2 ? (uint32_t)((pl_base[2 * (t / 3 != 1) + (t % 3 != 1)] + (t / 3 == 2 ? P : 0) + (t % 3 == 2)) * kRow)
                                                     : (uint32_t)(((t / 3) * P + t % 3) * kRow));
                const frag b = read_frag_tr<frag>(lx + to, 16 * kRow);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) acc[t][mt] = M::mfma(a[mt], b, acc[t][mt]);
            }
        }
    }

    // register i of lane (c, g) of tile (t, mt) = dweight[co0 + 16 mt + 4 g + i][ci0 + 16 wave + c][tap t]
    float* const op = out + (int64_t)s * C_out * C_in * 9 + ((int64_t)(co0 + 4 * g) * C_in + ci0 + 16 * wave + c16) * 9;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int t = 0; t < 9; ++t) op[(int64_t)(16 * mt + i) * C_in * 9 + t] = acc[t][mt][i];
}

static bool shape_ok(int64_t N, int32_t H, int32_t W, int32_t C_in, int32_t C_out) {
    return N >= 0 && H >= 1 && W >= 1 && W <= kMaxW && C_in > 0 && C_out > 0 && C_in % kBN == 0 && C_out % kBM == 0 &&
           (int64_t)H * (W + 2) < (1ll << 30) && (int64_t)(C_in / kBN) * (C_out / kBM) <= 0x7FFFFFFFll;
}

// chunks of one image: what the kernel indexes by
static int chunks_per_image(int32_t H, int32_t W, bool s2) {
    return s2 ? (int)(((int64_t)(H / 2) * (W / 2 + 1) + kKcS2 - 1) / kKcS2) : (int)(((int64_t)H * (W + 2) + kKc - 1) / kKc);
}

static int splits_of(int64_t N, int cpi, int32_t C_in, int32_t C_out) {
    return split_count(N * cpi, (int64_t)(C_in / kBN) * (C_out / kBM), kTargetBlocks);
}

template <bool kS2> static size_t workspace_bytes(int64_t N, int32_t H, int32_t W, int32_t C_in, int32_t C_out) {
    if (!shape_ok(N, H, W, C_in, C_out) || N == 0 || (kS2 && ((H & 1) || (W & 1)))) return 0;
    const int S = splits_of(N, chunks_per_image(H, W, kS2), C_in, C_out);
    return S > 1 ? (size_t)S * (size_t)C_out * C_in * 9 * sizeof(float) : 0;
}

template <typename T, bool kS2>
static int launch(const void* x, const void* dy, float* dweight, int64_t N, int H, int W, int C_in, int C_out, void* ws, size_t ws_bytes,
                  hipStream_t st) {
    const int cpi = chunks_per_image(H, W, kS2);
    int S = splits_of(N, cpi, C_in, C_out);
    const int64_t total = (int64_t)C_out * C_in * 9;
    if (S > 1 && (!ws || ws_bytes < (size_t)S * total * sizeof(float))) S = 1;          // a short workspace: the unsplit launch (linear_wgrad.hip refuses)
    const int lds_bytes = (kS2 ? s2_lds_rows(W) : kKc + x_rows(W)) * kRow;
    if (allow_large_lds<&conv3x3_wgrad_kernel<T, kS2>>(160 * 1024)) return MVI_EHIP;
    const unsigned tiles = (unsigned)((C_in / kBN) * (C_out / kBM));
    hipLaunchKernelGGL((conv3x3_wgrad_kernel<T, kS2>), dim3(tiles, (unsigned)S), dim3(64 * kWaves), lds_bytes, st, (const T*)x, (const T*)dy,
                       S > 1 ? (float*)ws : dweight, H, W, C_in, C_out, cpi, N * cpi, S);
    if (hipGetLastError() != hipSuccess) return MVI_EHIP;
    return S > 1 ? wgrad_reduce((const float*)ws, dweight, nullptr, total, 0, S, st) : 0;
}

// The body of both entry points. kS2: x [N, H W, C_in], dy [N, (H / 2)(W / 2), C_out], H and W even; gate, split policy (over dy's own
// position space), workspace and determinism as stride 1. Messages are MSG(" text") behind the entry point's own prefix.
template <bool kS2>
static int entry(const void* x, const void* dy, float* dweight, int64_t N, int32_t H, int32_t W, int32_t C_in, int32_t C_out, int32_t dtype,
                 void* workspace, size_t workspace_bytes, void* stream) {
#define MSG(text) (kS2 ? "conv3x3 s2 wgrad:" text : "conv3x3 wgrad:" text)
    if (!mvi_conv3x3_wgrad_supported(C_in, C_out, dtype) || !shape_ok(N, H, W, C_in, C_out) || (kS2 && ((H & 1) || (W & 1))))
        return unet_fail(MVI_EINVAL, kS2 ? "conv3x3 s2 wgrad: needs C_in and C_out multiples of 64, bf16 or f16, even H and W, W <= 256"
                                         : "conv3x3 wgrad: needs C_in and C_out multiples of 64, bf16 or f16, 1 <= W <= 256");
    if (!x || !dy || !dweight) return unet_fail(MVI_EINVAL, MSG(" NULL pointer"));       // also with N == 0 (conv3t and linear accept that)
    if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dweight | (uintptr_t)workspace) % 16)
        return unet_fail(MVI_EINVAL, MSG(" x, dy, dweight and workspace must be 16-byte aligned"));
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) return hipMemsetAsync(dweight, 0, (size_t)C_out * C_in * 9 * sizeof(float), st) == hipSuccess ? MVI_OK : MVI_EHIP;
    const int rc = dispatch_dtype16(dtype, MSG(" unknown dtype"), [&](auto t) {
        return launch<typename decltype(t)::type, kS2>(x, dy, dweight, N, H, W, C_in, C_out, workspace, workspace_bytes, st);
    });
    return rc == MVI_EHIP ? unet_fail(rc, MSG(" kernel launch failed")) : rc;
#undef MSG
}

}  // namespace cwg
}  // namespace mvi

extern "C" int mvi_conv3x3_wgrad_supported(int32_t C_in, int32_t C_out, int32_t dtype) {
    return C_in > 0 && C_out > 0 && C_in % mvi::cwg::kBN == 0 && C_out % mvi::cwg::kBM == 0 && (dtype == MVI_DT_BF16 || dtype == MVI_DT_F16);
}

extern "C" size_t mvi_conv3x3_wgrad_workspace_bytes(int64_t N, int32_t H, int32_t W, int32_t C_in, int32_t C_out) {
    return mvi::cwg::workspace_bytes<false>(N, H, W, C_in, C_out);
}

extern "C" int mvi_conv3x3_wgrad(const void* x, const void* dy, float* dweight, int64_t N, int32_t H, int32_t W, int32_t C_in, int32_t C_out,
                                 int32_t dtype, void* workspace, size_t workspace_bytes, void* stream) {
    return mvi::cwg::entry<false>(x, dy, dweight, N, H, W, C_in, C_out, dtype, workspace, workspace_bytes, stream);
}

// The stride-2 form (kS2 at the kernel).
extern "C" int mvi_conv3x3_s2_wgrad_supported(int32_t C_in, int32_t C_out, int32_t dtype) { return mvi_conv3x3_wgrad_supported(C_in, C_out, dtype); }

extern "C" size_t mvi_conv3x3_s2_wgrad_workspace_bytes(int64_t N, int32_t H, int32_t W, int32_t C_in, int32_t C_out) {
    return mvi::cwg::workspace_bytes<true>(N, H, W, C_in, C_out);
}

extern "C" int mvi_conv3x3_s2_wgrad(const void* x, const void* dy, float* dweight, int64_t N, int32_t H, int32_t W, int32_t C_in,
                                    int32_t C_out, int32_t dtype, void* workspace, size_t workspace_bytes, void* stream) {
    return mvi::cwg::entry<true>(x, dy, dweight, N, H, W, C_in, C_out, dtype, workspace, workspace_bytes, stream);
}
