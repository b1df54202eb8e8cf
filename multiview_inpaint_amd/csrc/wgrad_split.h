// The deterministic split-K scheme the MFMA weight-gradient files share (conv3x3_wgrad.hip, conv3t_wgrad.hip, linear_wgrad.hip;
// DESIGN.md, "Deterministic split-K of the weight gradients"). The output-tile grid alone cannot fill the chip, so the contraction
// units (chunks of pixels or rows: each file's own) are cut into S contiguous ranges, S a pure host function of the shape. S = 1:
// blocks store the gradient. S > 1: block (tile, s) stores its fp32 partial to workspace[s] and a second launch adds the S partials
// in index order. No atomics; run-to-run identical bits. Definitions: wgrad_split.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mvi {

constexpr int kMaxSplit = 64;

// S = min(units, target_blocks / tiles, kMaxSplit), in whole groups of `group` slices above one group; below 2 means 1 (unsplit).
int split_count(int64_t units, int64_t tiles, int target_blocks, int group = 1);

// dweight[i] = ws[0][i] + ws[1][i] + ... in that order over the [splits][n_w] weight partials; with n_b > 0 dbias likewise over the
// [splits][n_b] bias partials behind them. n_w and n_b are multiples of 4, every pointer 16-byte aligned. 0 or MVI_EHIP.
int wgrad_reduce(const float* ws, float* dweight, float* dbias, int64_t n_w, int64_t n_b, int splits, hipStream_t st);

}  // namespace mvi
