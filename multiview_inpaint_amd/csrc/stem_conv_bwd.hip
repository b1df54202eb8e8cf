// Weight and bias gradient of the hint-stem convolutions of csrc/stem_conv.hip (3x3, padding 1; stride 1 with <= 16 -> 16 or <= 32 -> 32
// channels, stride 2 with <= 16 -> 32), NCHW bf16 / f16, for gfx950 — ControlNet.input_hint_block under autograd (ops._StemConvSiluFn):
//     dW[co, ci, ky, kx] = sum over (n, oy, ox) of dz[n, co, oy, ox] * x[n, ci, s oy + ky - 1, s ox + kx - 1], out-of-image pixels 0,
//     db[co] = sum of dz[n, co, oy, ox].
//
// A GEMM on v_mfma_f32_16x16x32 with K = pixels: M = output channels (1 or 2 tiles of 16), N = the (tap, input channel) columns in
// tiles of 16 that share one kx, one k-step = 32 consecutive pixels of an output row (lane group g = 8 of them).
//   * A (dz): both operands are pixel-contiguous in their NCHW planes, so a lane's fragment — 8 pixels of channel lane & 15 — is ONE
//     16-byte global load, issued for all of the wave's k-steps of a tile before the patch is staged;
//   * B (x): the input patch of a tile (8 rows x 64 output pixels; 4 x 64 for stride 2 and for the 32 -> 32 form, whose 38 accumulator
//     tiles leave fewer registers for dz fragments) lies in LDS CHANNEL-major, [channel][row][16-byte
//     piece], brought and stored in 16-byte pieces only (one piece of halo on either side). The kx = 1 fragment is a piece as it lies;
//     kx = 0 and kx = 2 are the same run shifted by one element, built from two neighbouring pieces with v_alignbit. For stride 2 the
//     patch is split by column parity when it is staged (even | odd pieces per row), so the 8 output pixels of a k-step are contiguous
//     again: kx = 1 reads the even piece, kx = 2 the odd one, kx = 0 the odd one shifted;
//   * db: one more MFMA per k-step against a fragment of ones (every column of that accumulator tile is the sum of dz);
//   * a block walks a contiguous range of tiles with its accumulators in registers (each of its 4 waves takes a quarter of a tile's
//     k-steps), adds the four waves' tiles through LDS in wave order and writes ONE fp32 partial. The grid, and so the workspace, is
//     bounded by a few blocks per compute unit, not by the image. A second kernel adds the partials in block order and writes dW / db
//     in the module's order. No atomics: two runs give the same bits.
#include <cstdint>

#include "mfma_common.h"
#include "unet_host.h"

namespace mvi {
namespace scb {

constexpr int kTW = 64;                 // tile width in output pixels: two k-steps per row
constexpr int kCUs = 256;               // the grid bound is a pure function of the shape: the MI355X's compute units, not a device query

template <typename T> using Mma = MmaBuiltin16<T>;

template <int CINP, int COUT, int STRIDE> struct Form {
    static constexpr int TH = STRIDE == 2 || CINP == 32 ? 4 : 8;                   // output rows of a tile
    static constexpr int NTM = COUT / 16;
    static constexpr int CH = CINP >= 16 ? CINP / 16 : 1;            // 16-channel column tiles per tap
    static constexpr int KYB = CINP == 8 ? 2 : 3;                    // CINP 8: a column tile holds ky = 2 kyb and 2 kyb + 1 (ky = 3: padding)
    static constexpr int NTN = KYB * 3 * CH;                         // column tiles; tile NTN is the bias gradient's
    static constexpr int PR = STRIDE * (TH - 1) + 3;                 // patch rows
    static constexpr int PCS = STRIDE == 2 ? 17 : 10;                // 16-byte pieces per patch row: prev | 8 | next, or odd prev | 8 odd | 8 even
    static constexpr int ROWB = PCS * 16;
    static constexpr int CHB = PR * ROWB + ((PR * PCS) % 2 ? 0 : 16);   // an odd number of pieces per channel: the 16 channels of a read spread over the banks
    static constexpr int P = NTM * (NTN + 1) * 256;                  // floats of a block's partial: [M tile][column tile][lane][4]
    static constexpr int LDSB = CINP * CHB > P * 4 ? CINP * CHB : P * 4;
    static constexpr int BPC = COUT == 16 ? 4 : STRIDE == 2 ? 3 : 2; // blocks per compute unit the grid is bounded by
};

__device__ __forceinline__ uint32_t shr16(uint32_t hi, uint32_t lo) { return __builtin_amdgcn_alignbit(hi, lo, 16); }

template <typename T, int CINP, int COUT, int STRIDE>
__global__ __launch_bounds__(256, CINP == 32 ? 2 : 1) void stem_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dz, float* __restrict__ ws,
                                                                             int Cin, int H, int W, int Ho, int Wo, int tiles_x, int tiles_y, int n_tiles,
                                                                             int tiles_per_block) {
    using F = Form<CINP, COUT, STRIDE>;
    using M = Mma<T>;
    using frag = typename M::frag;
    constexpr int TH = F::TH, NTM = F::NTM, NTN = F::NTN, CH = F::CH, PR = F::PR, ROWB = F::ROWB, CHB = F::CHB;
    constexpr int KSW = TH * 2 / 4;                                  // k-steps of a tile per wave
    __shared__ __attribute__((aligned(16))) char s_p[F::LDSB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, g = lane >> 4;
    const uint16_t* xg = reinterpret_cast<const uint16_t*>(x);
    const uint16_t* dg = reinterpret_cast<const uint16_t*>(dz);

    f32x4 acc[NTM][NTN + 1];
#pragma unroll
    for (int mt = 0; mt < NTM; ++mt)
#pragma unroll
        for (int nt = 0; nt <= NTN; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const uint32_t one2 = M::pack2(1.0f, 1.0f);
    const u32x4 ones = {one2, one2, one2, one2};

    const int t0 = blockIdx.x * tiles_per_block, t1 = min(n_tiles, t0 + tiles_per_block);
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        const int tx = t % tiles_x, ty = (t / tiles_x) % tiles_y;
        const int64_t img = t / (tiles_x * tiles_y);
        const int x0 = tx * kTW, y0 = ty * TH;

        // ---- dz fragments of this wave's k-steps (zero outside the image: those pixels then count for nothing, whatever the patch holds)
        u32x4 a[KSW][NTM];
#pragma unroll
        for (int ks = 0; ks < KSW; ++ks) {
            const int kk = wave * KSW + ks, oy = y0 + (kk >> 1), ox = x0 + 32 * (kk & 1) + 8 * g;
            const bool ok = oy < Ho && ox < Wo;
#pragma unroll
            for (int mt = 0; mt < NTM; ++mt) {
                a[ks][mt] = u32x4{0, 0, 0, 0};
                if (ok) a[ks][mt] = *reinterpret_cast<const u32x4*>(dg + ((img * COUT + 16 * mt + n) * Ho + oy) * (int64_t)Wo + ox);
            }
        }

        __syncthreads();                                             // the previous tile's fragment reads are done
        const uint16_t* xin = xg + img * Cin * (int64_t)H * W;
        if constexpr (STRIDE == 1) {
            // piece pc of patch row r: pixels x0 - 8 + 8 pc .. + 7 of input row y0 - 1 + r
            for (int i = tid; i < CINP * PR * 10; i += 256) {
                const int pc = i % 10, r = (i / 10) % PR, c = i / (10 * PR);
                const int gy = y0 - 1 + r, gx = x0 - 8 + 8 * pc;
                u32x4 v = {0, 0, 0, 0};
                if (c < Cin && gy >= 0 && gy < H && gx >= 0 && gx < W) v = *reinterpret_cast<const u32x4*>(xin + ((int64_t)c * H + gy) * W + gx);
                *reinterpret_cast<u32x4*>(s_p + c * CHB + r * ROWB + pc * 16) = v;
            }
        } else {
            // item q of patch row r: the 16 pixels from 2 x0 - 16 + 16 q of input row 2 y0 - 1 + r, split by parity: the odd ones are
            // piece q (piece 0: the halo, whose last element is pixel 2 x0 - 1), the even ones piece 8 + q
            for (int i = tid; i < CINP * PR * 9; i += 256) {
                const int q = i % 9, r = (i / 9) % PR, c = i / (9 * PR);
                const int gy = 2 * y0 - 1 + r, gx = 2 * x0 - 16 + 16 * q;
                u32x4 va = {0, 0, 0, 0}, vb = {0, 0, 0, 0};
                if (c < Cin && gy >= 0 && gy < H && gx >= 0 && gx < W) {
                    const uint16_t* src = xin + ((int64_t)c * H + gy) * W + gx;
                    va = *reinterpret_cast<const u32x4*>(src);
                    vb = *reinterpret_cast<const u32x4*>(src + 8);
                }
                const u32x4 od = {(va[0] >> 16) | (va[1] & 0xFFFF0000u), (va[2] >> 16) | (va[3] & 0xFFFF0000u),
                                  (vb[0] >> 16) | (vb[1] & 0xFFFF0000u), (vb[2] >> 16) | (vb[3] & 0xFFFF0000u)};
                const u32x4 ev = {(va[0] & 0xFFFFu) | (va[1] << 16), (va[2] & 0xFFFFu) | (va[3] << 16),
                                  (vb[0] & 0xFFFFu) | (vb[1] << 16), (vb[2] & 0xFFFFu) | (vb[3] << 16)};
                char* const row = s_p + c * CHB + r * ROWB;
                *reinterpret_cast<u32x4*>(row + q * 16) = od;
                if (q) *reinterpret_cast<u32x4*>(row + (8 + q) * 16) = ev;
            }
        }
        __syncthreads();

        // ---- the wave's k-steps: row kk / 2 of the tile, pixels 32 (kk & 1) + 8 g .. + 7
#pragma unroll
        for (int ks = 0; ks < KSW; ++ks) {
            const int kk = wave * KSW + ks, r = kk >> 1, p = 4 * (kk & 1) + g;
#pragma unroll
            for (int kyb = 0; kyb < F::KYB; ++kyb) {
                const int ky = CINP == 8 ? min(2 * kyb + (n >> 3), 2) : kyb;      // (ky = 3: a padding column, never written out)
#pragma unroll
                for (int chh = 0; chh < CH; ++chh) {
                    const int ci = CINP == 8 ? (n & 7) : 16 * chh + n;
                    const char* const base = s_p + ci * CHB + (STRIDE * r + ky) * ROWB + p * 16;
                    const u32x4 pa = *reinterpret_cast<const u32x4*>(base);          // the piece before the lane's own (stride 2: of the odd ones)
                    const u32x4 pb = *reinterpret_cast<const u32x4*>(base + 16);     // the lane's own
                    const u32x4 pc = *reinterpret_cast<const u32x4*>(base + (STRIDE == 1 ? 32 : 9 * 16));   // the next one; stride 2: the even piece
                    const u32x4 sh = {shr16(pb[0], pa[3]), shr16(pb[1], pb[0]), shr16(pb[2], pb[1]), shr16(pb[3], pb[2])};
                    u32x4 f[3];
                    f[0] = sh;
                    if constexpr (STRIDE == 1) {
                        f[1] = pb;
                        f[2] = u32x4{sh[1], sh[2], sh[3], shr16(pc[0], pb[3])};
                    } else {
                        f[1] = pc;
                        f[2] = pb;
                    }
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                        for (int mt = 0; mt < NTM; ++mt)
                            acc[mt][(kyb * 3 + kx) * CH + chh] = M::mfma(as_frag<frag>(a[ks][mt]), as_frag<frag>(f[kx]), acc[mt][(kyb * 3 + kx) * CH + chh]);
                }
            }
#pragma unroll
            for (int mt = 0; mt < NTM; ++mt) acc[mt][NTN] = M::mfma(as_frag<frag>(a[ks][mt]), as_frag<frag>(ones), acc[mt][NTN]);
        }
    }

    // ---- the four waves' accumulators, added through LDS in wave order; the block's partial goes out in the accumulators' own layout
    f32x4* const s_acc = reinterpret_cast<f32x4*>(s_p);
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int mt = 0; mt < NTM; ++mt)
#pragma unroll
                for (int nt = 0; nt <= NTN; ++nt) {
                    f32x4* const at = s_acc + (mt * (NTN + 1) + nt) * 64 + lane;
                    *at = w ? *at + acc[mt][nt] : acc[mt][nt];
                }
        }
    }
    __syncthreads();
    f32x4* const out = reinterpret_cast<f32x4*>(ws + (int64_t)blockIdx.x * F::P);
    for (int i = tid; i < F::P / 4; i += 256) out[i] = s_acc[i];
}

// dW / db from the blocks' partials, added in block order (four running sums over blocks b % 4, then ((0 + 1) + (2 + 3))). Thread e = one
// accumulator element: tile (mt, nt), lane, register -> output channel 16 mt + 4 (lane >> 4) + reg, column lane & 15 of tile nt
__global__ __launch_bounds__(256) void stem_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, float* __restrict__ db, int blocks,
                                                                int P, int ntn, int cinp, int Cin) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= P) return;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int b = 0;
    for (; b + 4 <= blocks; b += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += ws[(int64_t)(b + k) * P + e];
    }
    for (int k = 0; b + k < blocks; ++k) s[k] += ws[(int64_t)(b + k) * P + e];
    const float sum = (s[0] + s[1]) + (s[2] + s[3]);
    const int reg = e & 3, lane = (e >> 2) & 63, tile = e >> 8;
    const int nt = tile % (ntn + 1), mt = tile / (ntn + 1);
    const int co = 16 * mt + 4 * (lane >> 4) + reg, n = lane & 15;
    if (nt == ntn) {
        if (n == 0 && db) db[co] = sum;
        return;
    }
    const int ch = cinp >= 16 ? cinp / 16 : 1;
    const int chh = nt % ch, kx = (nt / ch) % 3, kyb = nt / (3 * ch);
    const int ky = cinp == 8 ? 2 * kyb + (n >> 3) : kyb, ci = cinp == 8 ? (n & 7) : 16 * chh + n;
    if (ky < 3 && ci < Cin) dw[((co * Cin + ci) * 3 + ky) * 3 + kx] = sum;
}

struct Plan {
    int cinp, ntn, P, th, tiles_x, tiles_y, n_tiles, tiles_per_block, blocks;
};

template <int CINP, int COUT, int STRIDE> static Plan plan_form(int64_t N, int Ho, int Wo) {
    using F = Form<CINP, COUT, STRIDE>;
    Plan p;
    p.cinp = CINP, p.ntn = F::NTN, p.P = F::P, p.th = F::TH;
    p.tiles_x = (Wo + kTW - 1) / kTW, p.tiles_y = (Ho + F::TH - 1) / F::TH;
    const int64_t nt = N * p.tiles_x * p.tiles_y;
    p.n_tiles = nt > 0x7FFFFFFF ? -1 : (int)nt;
    const int cap = kCUs * F::BPC;
    p.tiles_per_block = p.n_tiles > 0 ? (p.n_tiles + cap - 1) / cap : 1;
    p.blocks = p.n_tiles > 0 ? (p.n_tiles + p.tiles_per_block - 1) / p.tiles_per_block : 0;
    return p;
}

// the forms of csrc/stem_conv.hip's dispatcher (stem_cinp)
static Plan plan(int64_t N, int Cin, int Cout, int H, int W, int stride) {
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    if (stride == 2) return plan_form<16, 32, 2>(N, Ho, Wo);
    if (Cout == 32) return plan_form<32, 32, 1>(N, Ho, Wo);
    if (Cin <= 8) return plan_form<8, 16, 1>(N, Ho, Wo);
    return plan_form<16, 16, 1>(N, Ho, Wo);
}

template <typename T, int CINP, int COUT, int STRIDE>
static void launch_form(const Plan& p, const void* x, const void* dz, float* ws, int Cin, int H, int W, hipStream_t st) {
    const int Ho = (H - 1) / STRIDE + 1, Wo = (W - 1) / STRIDE + 1;
    hipLaunchKernelGGL((stem_wgrad_kernel<T, CINP, COUT, STRIDE>), dim3((unsigned)p.blocks), dim3(256), 0, st, (const T*)x, (const T*)dz, ws, Cin, H, W,
                       Ho, Wo, p.tiles_x, p.tiles_y, p.n_tiles, p.tiles_per_block);
}

template <typename T>
static void launch(const Plan& p, const void* x, const void* dz, float* ws, int Cin, int Cout, int H, int W, int stride, hipStream_t st) {
    if (stride == 2) launch_form<T, 16, 32, 2>(p, x, dz, ws, Cin, H, W, st);
    else if (Cout == 32) launch_form<T, 32, 32, 1>(p, x, dz, ws, Cin, H, W, st);
    else if (Cin <= 8) launch_form<T, 8, 16, 1>(p, x, dz, ws, Cin, H, W, st);
    else launch_form<T, 16, 16, 1>(p, x, dz, ws, Cin, H, W, st);
}

}  // namespace scb
}  // namespace mvi

extern "C" size_t mvi_stem_conv3x3_wgrad_workspace_bytes(int64_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t stride) {
    if (N <= 0 || H <= 0 || W <= 0 || !mvi_stem_conv3x3_bwd_supported(Cin, Cout, W, stride, MVI_DT_BF16)) return 0;
    const mvi::scb::Plan p = mvi::scb::plan(N, Cin, Cout, H, W, stride);
    return p.n_tiles < 0 ? 0 : (size_t)p.blocks * p.P * sizeof(float);
}

extern "C" int mvi_stem_conv3x3_wgrad(const void* x, const void* dz, float* dweight, float* dbias, int64_t N, int32_t Cin, int32_t Cout, int32_t H,
                                      int32_t W, int32_t stride, int32_t dtype, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace mvi::scb;
    if (N < 0 || H <= 0 || W <= 0 || !mvi_stem_conv3x3_bwd_supported(Cin, Cout, W, stride, dtype))
        return mvi::unet_fail(MVI_EINVAL, "stem_conv3x3 wgrad: needs stride 1 with (C_out 16, C_in <= 16) or (C_out 32, C_in <= 32) and W % 8 == 0, or stride 2 "
                                          "with C_out 32, C_in <= 16 and W % 16 == 0; bf16 or f16");
    if (!dweight) return mvi::unet_fail(MVI_EINVAL, "stem_conv3x3 wgrad: NULL dweight");
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        if (hipMemsetAsync(dweight, 0, sizeof(float) * Cout * Cin * 9, st) != hipSuccess || (dbias && hipMemsetAsync(dbias, 0, sizeof(float) * Cout, st) != hipSuccess))
            return mvi::unet_fail(MVI_EHIP, "stem_conv3x3 wgrad: memset failed");
        return MVI_OK;
    }
    if (!x || !dz || ((uintptr_t)x | (uintptr_t)dz) % 16) return mvi::unet_fail(MVI_EINVAL, "stem_conv3x3 wgrad: x / dz must be non-NULL and 16-byte aligned");
    const Plan p = plan(N, Cin, Cout, H, W, stride);
    if (p.n_tiles < 0) return mvi::unet_fail(MVI_EINVAL, "stem_conv3x3 wgrad: too many tiles");
    if (!workspace || (uintptr_t)workspace % 16 || workspace_bytes < (size_t)p.blocks * p.P * sizeof(float))
        return mvi::unet_fail(MVI_EINVAL, "stem_conv3x3 wgrad: workspace NULL, unaligned or smaller than mvi_stem_conv3x3_wgrad_workspace_bytes()");
    float* ws = (float*)workspace;
    if (dtype == MVI_DT_BF16) launch<__hip_bfloat16>(p, x, dz, ws, Cin, Cout, H, W, stride, st);
    else launch<__half>(p, x, dz, ws, Cin, Cout, H, W, stride, st);
    hipLaunchKernelGGL(stem_wgrad_reduce_kernel, dim3((unsigned)((p.P + 255) / 256)), dim3(256), 0, st, ws, dweight, dbias, p.blocks, p.P, p.ntn, p.cinp, Cin);
    return hipGetLastError() == hipSuccess ? MVI_OK : mvi::unet_fail(MVI_EHIP, "stem_conv3x3 wgrad: kernel launch failed");
}
