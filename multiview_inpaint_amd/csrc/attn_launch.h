// The attention launchers, each defined beside its kernel and called from attn_api.hip (dispatch) and attn_bwd.hip.
// Token strides (q_rs / kv_rs / o_rs, q_ts / ...) are in elements, 0 = contiguous (H * D). Launchers return 0 or an MVI_E* code.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "unet_host.h"      // unet_fail, dispatch_dtype

namespace mvi {

// attn_flash.hip: 4 waves, 128 queries per block. scale_log2e: what a score is multiplied by on its way into exp2
template <typename T>
int attn_flash_launch(const void* q, const void* k, const void* v, void* out, int B, int H, int Sq, int Sk,
                      float scale_log2e, hipStream_t st, int64_t q_rs, int64_t kv_rs, int64_t o_rs, float* lse);

// attn_flash8m16.hip: 8 waves, 256 queries per block. q_log2: q carries scale * log2(e); fold: see attention_folds_scale
template <typename T>
int attn_flash8m16_launch(const void* q, const void* k, const void* v, void* out, int B, int H, int Sq, int Sk,
                          float scale, bool q_log2, bool fold, hipStream_t st, int64_t q_rs, int64_t kv_rs, int64_t o_rs, float* lse);

// attn_rowtile.hip: fp32 math, any dtype, D = 16 / 32 / 64. temporal_inner = S: the batch index is (video, token) and a sequence's
// tokens are S token strides apart (temporal attention without regrouping); 0 otherwise
template <typename T>
int attn_rowtile_launch(const void* q, const void* k, const void* v, void* out, int B, int H, int Sq, int Sk, int D,
                        float scale, hipStream_t st, int temporal_inner, int64_t q_ts, int64_t kv_ts, int64_t o_ts);

// attn_temporal.hip: MFMA temporal attention; _ok says whether it covers a call (pointers may be null: shape and strides only)
bool attn_temporal16_ok(int T, int D, int dtype, int64_t hd, int64_t qkv_ts, int64_t o_ts, const void* q, const void* k, const void* v,
                        const void* out);
template <typename T>
int attn_temporal16_launch(const void* q, const void* k, const void* v, void* out, int Bo, int Tn, int S, int H, float scale, hipStream_t st,
                           int64_t qkv_ts, int64_t o_ts);

// attn_temporal32.hip: the same for 16 < T <= 32 (a second key tile and a second query tile)
bool attn_temporal32_ok(int T, int D, int dtype, int64_t hd, int64_t qkv_ts, int64_t o_ts, const void* q, const void* k, const void* v,
                        const void* out);
template <typename T>
int attn_temporal32_launch(const void* q, const void* k, const void* v, void* out, int Bo, int Tn, int S, int H, float scale, hipStream_t st,
                           int64_t qkv_ts, int64_t o_ts);

// attn_api.hip. Does the forward of this kernel variant (mvi_attention_kernel_variant) and dtype round scale * log2(e) into Q instead
// of multiplying the fp32 scores by it? The forward launches by it and the backward recomputes P by it: L came from those scores.
bool attention_folds_scale(int variant, int dtype);

}  // namespace mvi
