// Weight and bias gradient of the projections (ops.linear: y = x W^T + b, W [N, K]) for gfx950, bf16 / f16:
//     dweight[n][k] = sum over r of dy[r, n] * x[r, k]          dbias[n] = sum over r of dy[r, n]
// a GEMM with M = N (out_features), N = K and the ROW as contraction index — the slow axis of both operands in memory, the job of
// conv3x3_wgrad.hip with one tap and no border. Both operands are staged row-major ([row][channel]) in LDS and both MFMA operands
// are read transposed (read_frag_tr, mfma_common.h). A one-tap instance of the convolution kernel would stage a 64-channel row of
// each operand per 4 MFMAs of a wave; here a block owns a 128 (out_features) x 128 (K) tile of dweight, a wave a 64 x 64 quarter of
// it (16 accumulator tiles, 64 registers): per 32-row step 4 A and 4 B fragments (16 transposed reads) feed 16 MFMAs.
//
// Staging: rows advance in chunks of kRc = 64. A chunk of an operand is 64 rows x 128 channels = 16 KiB = 16 LDS-DMA pieces of 1 KiB
// (4 rows each); the block's 4 waves issue 4 pieces of x and 4 of dy each. Two buffers of (x | dy) = 64 KiB: chunk c + 1 is issued
// before the MFMAs of chunk c, and the chunk ends with vmcnt(0) and one barrier (the DMA is invisible to the compiler's counters,
// so the wait is written out) — the buffer that is restaged was last read before the previous barrier.
// LDS rows are 256 bytes = all 64 banks, and a DMA piece is lane-linear, so rows cannot be padded: the 32-byte unit u (16 channels:
// what one transposed read takes from a row) of row r sits at unit position u ^ (r & 7), swizzled on the SOURCE address of the DMA
// and again in the read address. The 8 rows of a 32-lane half of a transposed read then cover the 64 banks once.
// K and out_features are multiples of 64, not of 128: the last tile of an axis may be half empty. Its DMA lanes take the tile's
// first half again (addresses inside the tensor), the waves of the empty quarter run no MFMA and store nothing.
// A ragged last chunk: the lanes of rows past the end load the chunk's first row instead (never past the end), and after the wait
// those LDS rows are overwritten with zeros behind a second barrier (that chunk only; the condition is uniform over the block).
//
// dbias: the blocks of the first K tile column hold the dy chunks anyway. Their two waves of the first K half multiply each A
// fragment with a fragment of ONES as well (4 more MFMAs per step): every column of that accumulator tile is the column sum of dy.
// It goes through the same split and reduction; dy is never read a second time.
//
// Split (wgrad_split.h): the tile grid alone is ceil(N / 128) ceil(K / 128) blocks (9 at 320 x 320, 24 at 960 x 320). Unit: a row
// chunk, ceil(rows / 64) of them; target 512 blocks, in whole groups of 8 slices above 8; the partials are [S][N K] floats, then [S][N]
// for dbias. Addresses are 64-bit; the per-lane DMA offset is 32-bit and relative to the chunk's first row (gate: 64 rows of either
// operand span less than 4 GiB).
//
// -Rpass-analysis=kernel-resource-usage (hipcc 7, -O3, the flags of attn_bwd.hip): DESIGN.md section 4, "Projections under autograd".
#include <cstdint>
#include <type_traits>

#include "mfma_common.h"
#include "unet_host.h"
#include "wgrad_split.h"

namespace mvi {
namespace lwg {

constexpr int kBN = 128;                        // out_features per block (A operand: dy)
constexpr int kBK = 128;                        // K per block (B operand: x)
constexpr int kWaves = 4;                       // 2 (out_features halves) x 2 (K halves)
constexpr int kRc = 64;                         // rows per chunk: two 32-row MFMA steps
constexpr int kRowB = 256;                      // LDS row: 128 channels, unpadded
constexpr int kOpBytes = kRc * kRowB;           // one operand's chunk: 16 KiB = 16 DMA pieces
constexpr int kBufBytes = 2 * kOpBytes;         // x | dy
constexpr int kLdsBytes = 2 * kBufBytes;        // double-buffered: 64 KiB, two blocks per CU
constexpr int kPiecesPerWave = kOpBytes / 1024 / kWaves;
constexpr int kXcds = 8;
constexpr int kTargetBlocks = 512;              // two blocks on each of the 256 CUs
constexpr int kVmcnt0 = 0x0F70;                 // s_waitcnt vmcnt(0) alone: expcnt and lgkmcnt fields at their maximum

template <typename T> using Mma = MmaBuiltin16<T>;

template <typename T>
__global__ __launch_bounds__(64 * kWaves) __attribute__((amdgpu_waves_per_eu(2, 2)))
void linear_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ out, float* __restrict__ bias_out,
                         int64_t rows, int K, int N, int64_t x_stride, int64_t dy_stride, int k_tiles, int tiles, int64_t chunks, int splits) {
    using M = Mma<T>;
    using frag = typename M::frag;
    __shared__ __attribute__((aligned(1024))) char smem[kLdsBytes];
    MVI_AS3 char* const lds = (MVI_AS3 char*)smem;
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)lds);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, g = lane >> 4;
    const int wn = wave >> 1, wk = wave & 1;
    // Blocks are dealt round-robin over the 8 XCDs. With 8 or more slices (then a multiple of 8: splits_of) block 8 j + c is tile
    // j % tiles of slice 8 (j / tiles) + c: all tiles of a row slice run on ONE XCD and share its rows through that L2 (speed only:
    // 0.153 -> 0.108 ms at 258048 x 320 -> 320). Fewer slices: tile-fastest order, every XCD busy.
    const int bj = splits >= kXcds ? (int)blockIdx.x >> 3 : (int)blockIdx.x;
    const int tile = bj % tiles, s = splits >= kXcds ? (bj / tiles) * kXcds + ((int)blockIdx.x & (kXcds - 1)) : bj / tiles;
    const int n0 = (tile / k_tiles) * kBN, k0 = (tile % k_tiles) * kBK;
    const int64_t ch_begin = chunks * s / splits, ch_end = chunks * (s + 1) / splits;
    const bool active = n0 + 64 * wn < N && k0 + 64 * wk < K;                 // wave-uniform: the quarter lies inside dweight
    const bool do_bias = bias_out != nullptr && k0 == 0 && wk == 0 && n0 + 64 * wn < N;

    // DMA lane constants. Lane l of a piece writes LDS row (l >> 4) of the piece's 4 rows, 16-byte position l & 15. The wave's pieces
    // are wave + 4 i, so the low three bits of the lane's chunk row are 4 (wave & 1) + (l >> 4) for every piece.
    const int prow = lane >> 4, pos = lane & 15;
    const int unit = (pos >> 1) ^ (4 * (wave & 1) + prow);                    // the 16-channel unit this LDS position holds
    const int ux = k0 + 16 * unit < K ? unit : unit - 4, ud = n0 + 16 * unit < N ? unit : unit - 4;
    const uint32_t cbx = (uint32_t)(32 * ux + 16 * (pos & 1)), cbd = (uint32_t)(32 * ud + 16 * (pos & 1));
    const uint32_t xsb = (uint32_t)(x_stride * 2), dsb = (uint32_t)(dy_stride * 2);      // row strides in bytes

    auto issue = [&](int64_t ch, uint32_t buf) {
        const int64_t r0 = ch * kRc;
        const int left = rows - r0 < kRc ? (int)(rows - r0) : kRc;            // rows of this chunk inside the tensors
        const char* const xb = (const char*)(x + r0 * x_stride + k0);
        const char* const db = (const char*)(dy + r0 * dy_stride + n0);
#pragma unroll
        for (int i = 0; i < kPiecesPerWave; ++i) {
            const int piece = wave + kWaves * i;
            const int rc = 4 * piece + prow;
            const uint32_t r = rc < left ? (uint32_t)rc : 0u;                 // past the end: the chunk's first row, zeroed in LDS later
            dma_piece(xb, r * xsb + cbx, __builtin_amdgcn_readfirstlane(lds0 + buf + 1024u * (uint32_t)piece));
            dma_piece(db, r * dsb + cbd, __builtin_amdgcn_readfirstlane(lds0 + buf + (uint32_t)kOpBytes + 1024u * (uint32_t)piece));
        }
    };
    // every DMA piece of this wave has landed; behind the barrier every wave's has, and the other buffer's reads are done
    auto settle = [&](int64_t ch, uint32_t buf) {
        __builtin_amdgcn_s_waitcnt(kVmcnt0);
        __syncthreads();
        const int64_t r0 = ch * kRc;
        if (rows - r0 < kRc) {                                                // ragged (the last chunk of the last slice only)
            const int left = (int)(rows - r0);
            for (int r = left + (tid >> 4); r < kRc; r += 16) {
                *reinterpret_cast<MVI_AS3 u32x4*>(lds + buf + r * kRowB + 16 * (tid & 15)) = u32x4{0u, 0u, 0u, 0u};
                *reinterpret_cast<MVI_AS3 u32x4*>(lds + buf + kOpBytes + r * kRowB + 16 * (tid & 15)) = u32x4{0u, 0u, 0u, 0u};
            }
            __syncthreads();
        }
    };

    // transposed read of a 4-row x 16-channel block: lane 4 q + p of a 16-lane group addresses row q, channels 4 p .. 4 p + 3 of the
    // unit; the unit's position is XORed with the row's low three bits (rows 16 and 32 further on have the same)
    const int trow = 4 * g + (c16 >> 2);
    const uint32_t tr = (uint32_t)(trow * kRowB + 32 * (trow & 7) + 8 * (c16 & 3));

    f32x4 acc[4][4], accb[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        accb[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    constexpr uint32_t kOne2 = std::is_same<T, __half>::value ? 0x3C003C00u : 0x3F803F80u;       // 1.0 | 1.0
    const frag ones = as_frag<frag>(u32x4{kOne2, kOne2, kOne2, kOne2});

    issue(ch_begin, 0u);
    settle(ch_begin, 0u);
    for (int64_t ch = ch_begin; ch < ch_end; ++ch) {
        const uint32_t buf = ((ch - ch_begin) & 1) ? (uint32_t)kBufBytes : 0u;
        if (ch + 1 < ch_end) issue(ch + 1, buf ^ (uint32_t)kBufBytes);
        if (active) {
#pragma unroll
            for (int st = 0; st < kRc / 32; ++st) {
                const uint32_t so = buf + (uint32_t)(32 * st * kRowB);
                frag a[4];
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
                    a[mt] = read_frag_tr<frag>(lds + kOpBytes + so + (tr ^ (uint32_t)(32 * (4 * wn + mt))), 16 * kRowB);
                if (do_bias) {
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) accb[mt] = M::mfma(a[mt], ones, accb[mt]);
                }
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const frag b = read_frag_tr<frag>(lds + so + (tr ^ (uint32_t)(32 * (4 * wk + nt))), 16 * kRowB);
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = M::mfma(a[mt], b, acc[mt][nt]);
                }
            }
        }
        if (ch + 1 < ch_end) settle(ch + 1, buf ^ (uint32_t)kBufBytes);
    }

    // register i of lane (c, g) of tile (mt, nt) = dweight[n0 + 64 wn + 16 mt + 4 g + i][k0 + 64 wk + 16 nt + c]
    if (active) {
        float* const op = out + (int64_t)s * N * K + (int64_t)(n0 + 64 * wn + 4 * g) * K + k0 + 64 * wk + c16;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) op[(int64_t)(16 * mt + i) * K + 16 * nt] = acc[mt][nt][i];
    }
    // every column of the ones product is the column sum: lane (0, g) writes dbias[n0 + 64 wn + 16 mt + 4 g + i]
    if (do_bias && c16 == 0) {
        float* const bp = bias_out + (int64_t)s * N + n0 + 64 * wn + 4 * g;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) bp[16 * mt + i] = accb[mt][i];
    }
}

static bool shape_ok(int64_t rows, int32_t K, int32_t N) {
    return rows >= 0 && K > 0 && N > 0 && K % 64 == 0 && N % 64 == 0 && rows < (1ll << 40) &&
           (int64_t)((K + kBK - 1) / kBK) * ((N + kBN - 1) / kBN) <= 0x7FFFFFFFll / (kXcds * kMaxSplit);
}

// a row stride (elements): at least the row, rows 16-byte aligned, 64 rows inside the DMA's 32-bit lane offset
static bool stride_ok(int64_t stride, int32_t width) { return stride >= width && stride % 8 == 0 && stride < (1ll << 24); }

// whole groups of 8 slices above 8: the kernel's XCD-aware block order
static int splits_of(int64_t rows, int32_t K, int32_t N) {
    return split_count((rows + kRc - 1) / kRc, (int64_t)((K + kBK - 1) / kBK) * ((N + kBN - 1) / kBN), kTargetBlocks, kXcds);
}

static size_t workspace_of(int S, int32_t K, int32_t N) { return S > 1 ? (size_t)S * ((size_t)N * K + (size_t)N) * sizeof(float) : 0; }

template <typename T>
static int launch(const void* x, const void* dy, float* dweight, float* dbias, int64_t rows, int K, int N, int64_t xs, int64_t dys, int S,
                  void* ws, hipStream_t st) {
    const int64_t chunks = (rows + kRc - 1) / kRc;
    const int k_tiles = (K + kBK - 1) / kBK, n_tiles = (N + kBN - 1) / kBN;
    float* const wpart = S > 1 ? (float*)ws : dweight;
    float* const bpart = !dbias ? nullptr : S > 1 ? (float*)ws + (size_t)S * N * K : dbias;
    const int tiles = k_tiles * n_tiles;
    hipLaunchKernelGGL(linear_wgrad_kernel<T>, dim3((unsigned)tiles * (unsigned)S), dim3(64 * kWaves), 0, st, (const T*)x,
                       (const T*)dy, wpart, bpart, rows, K, N, xs, dys, k_tiles, tiles, chunks, S);
    if (hipGetLastError() != hipSuccess) return MVI_EHIP;
    return S > 1 ? wgrad_reduce((const float*)ws, dweight, dbias, (int64_t)N * K, dbias ? N : 0, S, st) : 0;
}

}  // namespace lwg
}  // namespace mvi

extern "C" int mvi_linear_wgrad_supported(int32_t K, int32_t out_features, int32_t dtype) {
    return K > 0 && out_features > 0 && K % 64 == 0 && out_features % 64 == 0 && (dtype == MVI_DT_BF16 || dtype == MVI_DT_F16);
}

extern "C" size_t mvi_linear_wgrad_workspace_bytes(int64_t rows, int32_t K, int32_t out_features) {
    if (!mvi::lwg::shape_ok(rows, K, out_features) || rows == 0) return 0;
    return mvi::lwg::workspace_of(mvi::lwg::splits_of(rows, K, out_features), K, out_features);
}

// workspace NULL (and workspace_bytes 0): the unsplit launch, one block per tile over all rows. Otherwise it holds at least
// mvi_linear_wgrad_workspace_bytes(rows, K, out_features).
extern "C" int mvi_linear_wgrad(const void* x, const void* dy, float* dweight, float* dbias, int64_t rows, int32_t K, int32_t out_features,
                                int64_t x_row_stride, int64_t dy_row_stride, int32_t dtype, void* workspace, size_t workspace_bytes,
                                void* stream) {
    const int32_t N = out_features;
    if (!mvi_linear_wgrad_supported(K, N, dtype) || !mvi::lwg::shape_ok(rows, K, N))
        return mvi::unet_fail(MVI_EINVAL, "linear wgrad: needs K and out_features multiples of 64, bf16 or f16");
    if (!mvi::lwg::stride_ok(x_row_stride, K) || !mvi::lwg::stride_ok(dy_row_stride, N))
        return mvi::unet_fail(MVI_EINVAL, "linear wgrad: row strides must cover a row, be multiples of 8 elements and below 2^24");
    if (!dweight || (rows > 0 && (!x || !dy))) return mvi::unet_fail(MVI_EINVAL, "linear wgrad: NULL pointer");      // (no rows: nothing is read)
    if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dweight | (uintptr_t)dbias | (uintptr_t)workspace) % 16)
        return mvi::unet_fail(MVI_EINVAL, "linear wgrad: x, dy, dweight, dbias and workspace must be 16-byte aligned");
    int S = mvi::lwg::splits_of(rows, K, N);
    if (!workspace && workspace_bytes == 0) S = 1;
    else if (!workspace || workspace_bytes < mvi::lwg::workspace_of(S, K, N))      // a short workspace is refused (the convolutions run unsplit)
        return mvi::unet_fail(MVI_EINVAL, "linear wgrad: workspace shorter than mvi_linear_wgrad_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    if (rows == 0) {
        if (hipMemsetAsync(dweight, 0, (size_t)N * K * sizeof(float), st) != hipSuccess) return MVI_EHIP;
        if (dbias && hipMemsetAsync(dbias, 0, (size_t)N * sizeof(float), st) != hipSuccess) return MVI_EHIP;
        return MVI_OK;
    }
    const int rc = mvi::dispatch_dtype16(dtype, "linear wgrad: unknown dtype", [&](auto t) {
        return mvi::lwg::launch<typename decltype(t)::type>(x, dy, dweight, dbias, rows, K, N, x_row_stride, dy_row_stride, S, workspace, st);
    });
    return rc == MVI_EHIP ? mvi::unet_fail(rc, "linear wgrad: kernel launch failed") : rc;
}
