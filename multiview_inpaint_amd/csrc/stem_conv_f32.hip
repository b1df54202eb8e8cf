// conv_in of the first-stage ENCODER (sgm/modules/diffusionmodules/model.py Encoder.conv_in: 3 -> 128 channels, 3x3 / stride 1 /
// padding 1, at the full 576 x 1024 image) for the split-operand walk of svd/vae_split.py: fp32 planes [N, C_in, H, W] in, fp32 TOKEN-MAJOR
// rows [N, H W, C_out] with the bias out — the layout every later layer of that walk reads, so the NCHW -> NHWC pass over the largest
// tensor of the encoder (302 MB per frame) that a library convolution would need never happens.
//
// VALU, not v_mfma_f32_16x16x4_f32: the work is 9 C_in (<= 36) products per output, 57 GFLOP for 14 frames — next to a 4.2 GB store it is
// nothing on either pipe, and the matrix form would buy it with a K = 27 contraction padded to 28, an input gather into fragment order
// and an accumulator layout (a lane holds 4 ROWS of one column) that has to be transposed before a token row can leave as 16-byte pieces.
// On the VALU a lane owns 4 ADJACENT output channels of a pixel: its accumulators are the float4 it stores, consecutive lanes store
// consecutive 16 bytes (a wave writes 1 KiB of whole token rows per instruction, whatever C_out), and the arithmetic is the plain fp32
// FMA chain bias + sum over (c_in, ky, kx) — exact fp32 products, one rounding per term, no operand rounding and no split.
//
// A lane's 4 x 9 C_in weights are 36 C_in CONTIGUOUS floats of the module's [C_out, C_in, 3, 3] tensor (16-byte aligned): it loads them
// once as 9 C_in float4 into registers and keeps them for all its pixels (kPasses of them). No LDS. The lanes of a block that share a
// pixel read the same 9 C_in inputs (one address per load: a broadcast), and the passes walk neighbouring pixels, so the input planes
// (1 / 43 of the output's bytes) come from cache.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "unet_host.h"

namespace mvi {
namespace {

constexpr int kThreads = 256;
constexpr int kPasses = 64;                          // pixels per lane: the weights are loaded once per (block, lane) for all of them
constexpr int kMaxCin = 4, kMaxCout = 1024;          // (C_out / 4 lanes share a pixel: at most one block's worth)

template <int CIN>
__global__ __launch_bounds__(kThreads) void stem_conv_f32_tokens_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                         const float* __restrict__ bias, float* __restrict__ out,
                                                                         int64_t pixels, int H, int W, int cq4, int ppp) {
    // thread t < ppp cq4: channel quad t % cq4 of pixel t / cq4 of the pass; the rest of the block (256 % cq4 threads) idles
    const int t = threadIdx.x;
    if (t >= ppp * cq4) return;
    const int cq = t % cq4, pl = t / cq4;
    float4 wr[9 * CIN];
    const float4* const wv = reinterpret_cast<const float4*>(w) + (int64_t)cq * (9 * CIN);
#pragma unroll
    for (int i = 0; i < 9 * CIN; ++i) wr[i] = wv[i];
    const float* const wf = reinterpret_cast<const float*>(wr);           // [4 channels][CIN][9] (constant indices below: registers)
    const float4 b4 = bias ? reinterpret_cast<const float4*>(bias)[cq] : float4{0.f, 0.f, 0.f, 0.f};
    const int64_t hw = (int64_t)H * W;
    const int64_t p0 = (int64_t)blockIdx.x * ((int64_t)ppp * kPasses) + pl;
    for (int k = 0; k < kPasses; ++k) {
        const int64_t p = p0 + (int64_t)k * ppp;
        if (p >= pixels) return;                                           // (p grows with k)
        const int64_t n = p / hw;
        const int pix = (int)(p - n * hw);
        const int y = pix / W, xx = pix - y * W;
        const float* const xn = x + n * CIN * hw + pix;                    // the centre in plane 0 of image n
        float a0 = b4.x, a1 = b4.y, a2 = b4.z, a3 = b4.w;
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int yy = y + ky - 1, xc = xx + kx - 1;
                    const bool ok = yy >= 0 && yy < H && xc >= 0 && xc < W;
                    const float v = ok ? xn[ci * hw + (int64_t)(ky - 1) * W + (kx - 1)] : 0.f;   // (no address is formed outside the tensor)
                    const int j = ci * 9 + ky * 3 + kx;
                    a0 = __builtin_fmaf(v, wf[0 * 9 * CIN + j], a0);
                    a1 = __builtin_fmaf(v, wf[1 * 9 * CIN + j], a1);
                    a2 = __builtin_fmaf(v, wf[2 * 9 * CIN + j], a2);
                    a3 = __builtin_fmaf(v, wf[3 * 9 * CIN + j], a3);
                }
        reinterpret_cast<float4*>(out)[p * cq4 + cq] = float4{a0, a1, a2, a3};
    }
}

}  // namespace
}  // namespace mvi

extern "C" int mvi_conv3x3_small_cin_f32_tokens_supported(int32_t C_in, int32_t C_out) {
    return C_in >= 1 && C_in <= mvi::kMaxCin && C_out >= 4 && C_out <= mvi::kMaxCout && C_out % 4 == 0;
}

extern "C" int mvi_conv3x3_small_cin_f32_tokens(const float* x, const float* weight, const float* bias, float* out, int64_t N, int32_t C_in,
                                                int32_t H, int32_t W, int32_t C_out, void* stream) {
    using namespace mvi;
    if (N < 0 || H <= 0 || W <= 0 || !mvi_conv3x3_small_cin_f32_tokens_supported(C_in, C_out))
        return unet_fail(MVI_EINVAL, "conv3x3_small_cin_f32_tokens: needs 1 <= C_in <= 4 and C_out a multiple of 4 (<= 1024)");
    if (N == 0) return MVI_OK;
    if (!x || !weight || !out) return unet_fail(MVI_EINVAL, "conv3x3_small_cin_f32_tokens: NULL pointer");
    if (((uintptr_t)weight | (uintptr_t)out | (uintptr_t)bias) % 16 || (uintptr_t)x % 4)
        return unet_fail(MVI_EINVAL, "conv3x3_small_cin_f32_tokens: weight, bias and out must be 16-byte aligned");
    if ((int64_t)H * W > 0x7FFFFFFFll) return unet_fail(MVI_EINVAL, "conv3x3_small_cin_f32_tokens: image too large");
    const int64_t pixels = N * (int64_t)H * W;
    const int cq4 = C_out / 4, ppp = kThreads / cq4;
    const int64_t per_block = (int64_t)ppp * kPasses, blocks = (pixels + per_block - 1) / per_block;
    if (blocks > 0x7FFFFFFFll) return unet_fail(MVI_EINVAL, "conv3x3_small_cin_f32_tokens: too many pixels for one launch");
    hipStream_t st = (hipStream_t)stream;
#define MVI_STEM_F32(CIN) \
    hipLaunchKernelGGL(stem_conv_f32_tokens_kernel<CIN>, dim3((unsigned)blocks), dim3(kThreads), 0, st, x, weight, bias, out, pixels, H, W, cq4, ppp)
    switch (C_in) {
        case 1: MVI_STEM_F32(1); break;
        case 2: MVI_STEM_F32(2); break;
        case 3: MVI_STEM_F32(3); break;
        default: MVI_STEM_F32(4); break;
    }
#undef MVI_STEM_F32
    return hipGetLastError() == hipSuccess ? MVI_OK : unet_fail(MVI_EHIP, "conv3x3_small_cin_f32_tokens: kernel launch failed");
}
