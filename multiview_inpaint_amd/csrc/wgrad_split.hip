// The split count and the second launch of the weight-gradient kernels' deterministic split-K scheme (wgrad_split.h).
// -Rpass-analysis=kernel-resource-usage (hipcc 7, -O3): wgrad_reduce_kernel 14 VGPRs, 22 SGPRs, no LDS, no scratch.
#include "wgrad_split.h"

#include "mfma_common.h"
#include "unet_host.h"

namespace mvi {

int split_count(int64_t units, int64_t tiles, int target_blocks, int group) {
    int64_t S = target_blocks / tiles;
    if (S > kMaxSplit) S = kMaxSplit;
    if (S > units) S = units;
    if (S > group) S -= S % group;
    return S < 2 ? 1 : (int)S;
}

// out[i] = part[0][i] + part[1][i] + ... in that order; the bias partials ([S][n4], behind the [S][nw4] weight partials) likewise
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const f32x4* __restrict__ part, f32x4* __restrict__ dweight,
                                                           f32x4* __restrict__ dbias, int64_t nw4, int64_t n4, int splits) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nw4 + n4) return;
    const bool w = i < nw4;
    const f32x4* const p = w ? part + i : part + (int64_t)splits * nw4 + (i - nw4);
    const int64_t step = w ? nw4 : n4;
    f32x4 a = p[0];
    for (int s = 1; s < splits; ++s) a += p[s * step];
    if (w) dweight[i] = a; else dbias[i - nw4] = a;
}

int wgrad_reduce(const float* ws, float* dweight, float* dbias, int64_t n_w, int64_t n_b, int splits, hipStream_t st) {
    const int64_t nw4 = n_w / 4, n4 = n_b / 4;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((nw4 + n4 + 255) / 256)), dim3(256), 0, st, (const f32x4*)ws, (f32x4*)dweight,
                       (f32x4*)dbias, nw4, n4, splits);
    return hipGetLastError() == hipSuccess ? 0 : MVI_EHIP;
}

}  // namespace mvi
