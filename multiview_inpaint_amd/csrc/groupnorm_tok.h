// Thread layout of the token-row GroupNorm kernels (groupnorm_tokens.hip, and the token-major backward of groupnorm_bwd.hip):
// a block is VPR x RP threads — VPR = C / vec 16-byte vectors per token row, RP rows per pass — and a thread owns the SAME vec
// channels in every row it reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mvi_unet_ops.h"      // MVI_DT_*

namespace mvi {

constexpr int kGtPasses = 8;          // token rows per thread and chunk
constexpr int kGtMaxGroups = 64;

__host__ __device__ inline int gt_rows_per_pass(int vpr) { int rp = 512 / vpr; return rp < 1 ? 1 : (rp > 8 ? 8 : rp); }

inline int gt_geometry_ok(int64_t N, int32_t C, int64_t S, int32_t G, int32_t dtype) {
    const int V = dtype == MVI_DT_F32 ? 4 : 8;
    if (N <= 0 || C <= 0 || S <= 0 || G <= 0 || G > kGtMaxGroups || C % G || C % V) return 0;
    const int vpr = C / V;
    if (vpr > 1024 || N > 65535) return 0;
    const int rp = gt_rows_per_pass(vpr);
    return ((size_t)2 * rp * C + C) * sizeof(float) <= 64 * 1024;
}

}  // namespace mvi
