// The C entry points of forward attention (include/mvi_unet_ops.h) and the one place that picks a kernel for a call: spatial
// (attn_flash.hip, attn_flash8m16.hip, attn_rowtile.hip) and temporal (attn_temporal.hip, attn_temporal32.hip, attn_rowtile.hip). The backward's entry
// points are in attn_bwd.hip and ask the same functions.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <cstdlib>

#include "attn_launch.h"

extern "C" int mvi_attention_kernel_kind(int32_t Sq, int32_t Sk, int32_t D, int32_t dtype) {
    return (dtype != MVI_DT_F32 && D == 64 && Sk > 32) ? 1 : 0;
}
// the ONE place that picks the kernel: mvi_attention_forward* and the tests' assertion read the same answer
extern "C" int mvi_attention_kernel_variant(int32_t Sq, int32_t Sk, int32_t D, int32_t dtype) {
    if (mvi_attention_kernel_kind(Sq, Sk, D, dtype) != 1) return 0;
    // 256-row blocks pay off once there are enough of them and the padding of the last block is small
    static const int forced = getenv("MVI_ATTN_VARIANT") ? atoi(getenv("MVI_ATTN_VARIANT")) : 0;   // 4 / 8: force the 4- / 8-wave kernel (A/B runs)
    const bool eight = forced == 8 || (forced != 4 && Sq >= 1024 && Sk >= 256);
    return eight ? 16 : 4;                      // 16: the 8-wave kernel is built on v_mfma_f32_16x16x32 (attn_flash8m16.hip)
}

// The ONE place that decides fold versus exact scale (attn_launch.h); the 4-wave kernel always multiplies the fp32 scores.
// Default: exact for bf16; folded for f16, whose 11-bit mantissa makes the second rounding of Q eight times smaller (below the exact
// bf16 form's own error) — f16 is the reference's precision recipe and the fold is worth 7 % of the kernel. MVI_ATTN_FOLD_SCALE=0|1
// overrides it for both types.
bool mvi::attention_folds_scale(int variant, int dtype) {
    if (variant != 16) return false;
    static const char* const env = getenv("MVI_ATTN_FOLD_SCALE");
    static const int fold_env = env ? atoi(env) : -1;
    return fold_env >= 0 ? fold_env != 0 : dtype == MVI_DT_F16;
}

// q_log2: q carries softmax scale * log2(e) already (mvi_attention_forward_strided_qlog2); `scale` is then ln 2, what the kernels
// that exponentiate with e must apply, and the exp2 kernels take their scores as they are
constexpr float kLn2 = 0.6931471805599453f, kLog2e = 1.4426950408889634f;
static int attention_forward_impl(const void* q, const void* k, const void* v, void* out, int32_t B, int32_t H, int32_t Sq,
                                  int32_t Sk, int32_t D, float scale, int32_t dtype, int64_t q_ts, int64_t kv_ts, int64_t o_ts,
                                  void* stream, bool q_log2 = false, float* lse = nullptr) {
    if (q_log2) scale = kLn2;
    if (B < 0 || H <= 0 || Sq < 0 || Sk <= 0 || D <= 0) return mvi::unet_fail(MVI_EINVAL, "attention: bad shape");
    if (B == 0 || Sq == 0) return MVI_OK;
    if (!q || !k || !v || !out) return mvi::unet_fail(MVI_EINVAL, "attention: NULL pointer");
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) % 16 != 0)
        return mvi::unet_fail(MVI_EINVAL, "attention: pointers must be 16-byte aligned");
    const int64_t hd = (int64_t)H * D;
    const int esz = dtype == MVI_DT_F32 ? 4 : 2;
    if (q_ts < 0 || kv_ts < 0 || o_ts < 0 || (q_ts && q_ts < hd) || (kv_ts && kv_ts < hd) || (o_ts && o_ts < hd) ||
        (q_ts * esz) % 16 || (kv_ts * esz) % 16 || (o_ts * esz) % 16)
        return mvi::unet_fail(MVI_EINVAL, "attention: token strides must be 0 or >= H*D elements and 16-byte multiples");
    hipStream_t st = (hipStream_t)stream;
    const auto launched = [](int rc) { return rc ? mvi::unet_fail(rc, "attention: kernel launch failed") : MVI_OK; };
    const int variant = mvi_attention_kernel_variant(Sq, Sk, D, dtype);
    if (variant == 16) {
        // a q that carries scale * log2(e) runs the folded kernel with nothing left to fold, in both types
        const bool fold = q_log2 || mvi::attention_folds_scale(variant, dtype);
        return mvi::dispatch_dtype16(dtype, "attention: unknown dtype", [&](auto t) {
            return launched(mvi::attn_flash8m16_launch<typename decltype(t)::type>(q, k, v, out, B, H, Sq, Sk, scale, q_log2, fold, st, q_ts, kv_ts, o_ts, lse));
        });
    }
    if (variant != 0) {
        const float sl2 = q_log2 ? 1.0f : scale * kLog2e;
        return mvi::dispatch_dtype16(dtype, "attention: unknown dtype", [&](auto t) {
            return launched(mvi::attn_flash_launch<typename decltype(t)::type>(q, k, v, out, B, H, Sq, Sk, sl2, st, q_ts, kv_ts, o_ts, lse));
        });
    }
    if (D != 16 && D != 32 && D != 64) return mvi::unet_fail(MVI_EINVAL, "attention: head dim must be 16, 32 or 64");
    return mvi::dispatch_dtype(dtype, "attention: unknown dtype", [&](auto t) {
        return launched(mvi::attn_rowtile_launch<typename decltype(t)::type>(q, k, v, out, B, H, Sq, Sk, D, scale, st, 0, q_ts, kv_ts, o_ts));
    });
}

extern "C" int mvi_attention_forward(const void* q, const void* k, const void* v, void* out, int32_t B, int32_t H,
                                     int32_t Sq, int32_t Sk, int32_t D, float scale, int32_t dtype, void* stream) {
    return attention_forward_impl(q, k, v, out, B, H, Sq, Sk, D, scale, dtype, 0, 0, 0, stream);
}

extern "C" int mvi_attention_forward_lse(const void* q, const void* k, const void* v, void* out, void* lse, int32_t B, int32_t H,
                                         int32_t Sq, int32_t Sk, int32_t D, float scale, int32_t dtype, void* stream) {
    if (B < 0 || H <= 0 || Sq < 0 || Sk <= 0 || D <= 0) return mvi::unet_fail(MVI_EINVAL, "attention (lse): bad shape");
    if (mvi_attention_kernel_kind(Sq, Sk, D, dtype) != 1 || (dtype != MVI_DT_BF16 && dtype != MVI_DT_F16))
        return mvi::unet_fail(MVI_EINVAL, "attention (lse): bf16 / f16, head dim 64 and more than 32 keys only");
    if (B == 0 || Sq == 0) return MVI_OK;
    if (!lse || (uintptr_t)lse % 4 != 0) return mvi::unet_fail(MVI_EINVAL, "attention (lse): lse must be a 4-byte aligned pointer");
    return attention_forward_impl(q, k, v, out, B, H, Sq, Sk, D, scale, dtype, 0, 0, 0, stream, false, (float*)lse);
}

extern "C" int mvi_attention_forward_strided(const void* q, const void* k, const void* v, void* out, int32_t B, int32_t H,
                                             int32_t Sq, int32_t Sk, int32_t D, float scale, int32_t dtype,
                                             int64_t q_token_stride, int64_t kv_token_stride, int64_t out_token_stride,
                                             void* stream) {
    return attention_forward_impl(q, k, v, out, B, H, Sq, Sk, D, scale, dtype, q_token_stride, kv_token_stride,
                                  out_token_stride, stream);
}

extern "C" int mvi_attention_forward_strided_qlog2(const void* q, const void* k, const void* v, void* out, int32_t B, int32_t H,
                                                   int32_t Sq, int32_t Sk, int32_t D, int32_t dtype, int64_t q_token_stride,
                                                   int64_t kv_token_stride, int64_t out_token_stride, void* stream) {
    return attention_forward_impl(q, k, v, out, B, H, Sq, Sk, D, kLn2, dtype, q_token_stride, kv_token_stride, out_token_stride, stream, true);
}

// The frame capacity of the MFMA kernel that serves this call: 16 (csrc/attn_temporal.hip), 32 (csrc/attn_temporal32.hip), or 0 for the
// fp32-math kernel of csrc/attn_rowtile.hip. The ONE place that picks the temporal kernel.
extern "C" int mvi_attention_temporal_kernel_kind(int32_t T, int32_t H, int32_t D, int32_t dtype, int64_t qkv_token_stride,
                                                  int64_t out_token_stride) {
    static const bool off = getenv("MVI_ATTN_TEMPORAL_MFMA") && getenv("MVI_ATTN_TEMPORAL_MFMA")[0] == '0';     // same-box A/B runs: both off
    if (off) return 0;
    const int64_t hd = (int64_t)H * D;
    if (mvi::attn_temporal16_ok(T, D, dtype, hd, qkv_token_stride, out_token_stride, nullptr, nullptr, nullptr, nullptr)) return 16;
    if (mvi::attn_temporal32_ok(T, D, dtype, hd, qkv_token_stride, out_token_stride, nullptr, nullptr, nullptr, nullptr)) return 32;
    return 0;
}

// 1 when the 16-frame MFMA kernel of csrc/attn_temporal.hip serves this call, 0 otherwise
extern "C" int mvi_attention_temporal_kernel_variant(int32_t T, int32_t H, int32_t D, int32_t dtype, int64_t qkv_token_stride,
                                                     int64_t out_token_stride) {
    return mvi_attention_temporal_kernel_kind(T, H, D, dtype, qkv_token_stride, out_token_stride) == 16;
}

static int attention_temporal_impl(const void* q, const void* k, const void* v, void* out, int32_t Bo, int32_t T, int32_t S,
                                   int32_t H, int32_t D, float scale, int32_t dtype, int64_t qkv_ts, int64_t o_ts, void* stream) {
    if (Bo < 0 || T <= 0 || S <= 0 || H <= 0 || D <= 0) return mvi::unet_fail(MVI_EINVAL, "temporal attention: bad shape");
    if (Bo == 0) return MVI_OK;
    if (!q || !k || !v || !out) return mvi::unet_fail(MVI_EINVAL, "temporal attention: NULL pointer");
    if (D != 16 && D != 32 && D != 64) return mvi::unet_fail(MVI_EINVAL, "temporal attention: head dim must be 16, 32 or 64");
    if ((int64_t)Bo * S > 0x7FFFFFFFll) return mvi::unet_fail(MVI_EINVAL, "temporal attention: too many problems");
    const int64_t hd = (int64_t)H * D;
    if (qkv_ts < 0 || o_ts < 0 || (qkv_ts && qkv_ts < hd) || (o_ts && o_ts < hd))
        return mvi::unet_fail(MVI_EINVAL, "temporal attention: token strides must be 0 or >= H*D elements");
    hipStream_t st = (hipStream_t)stream;
    const int B = Bo * S;
    const auto launched = [](int rc) { return rc ? mvi::unet_fail(rc, "temporal attention: kernel launch failed") : MVI_OK; };
    const int kind = mvi_attention_temporal_kernel_kind(T, H, D, dtype, qkv_ts, o_ts);
    if (kind == 16 && mvi::attn_temporal16_ok(T, D, dtype, hd, qkv_ts, o_ts, q, k, v, out))
        return mvi::dispatch_dtype16(dtype, "temporal attention: unknown dtype", [&](auto t) {
            return launched(mvi::attn_temporal16_launch<typename decltype(t)::type>(q, k, v, out, Bo, T, S, H, scale, st, qkv_ts, o_ts));
        });
    if (kind == 32 && mvi::attn_temporal32_ok(T, D, dtype, hd, qkv_ts, o_ts, q, k, v, out))
        return mvi::dispatch_dtype16(dtype, "temporal attention: unknown dtype", [&](auto t) {
            return launched(mvi::attn_temporal32_launch<typename decltype(t)::type>(q, k, v, out, Bo, T, S, H, scale, st, qkv_ts, o_ts));
        });
    return mvi::dispatch_dtype(dtype, "temporal attention: unknown dtype", [&](auto t) {
        return launched(mvi::attn_rowtile_launch<typename decltype(t)::type>(q, k, v, out, B, H, T, T, D, scale, st, S, qkv_ts, qkv_ts, o_ts));
    });
}

extern "C" int mvi_attention_temporal(const void* q, const void* k, const void* v, void* out, int32_t Bo, int32_t T,
                                      int32_t S, int32_t H, int32_t D, float scale, int32_t dtype, void* stream) {
    return attention_temporal_impl(q, k, v, out, Bo, T, S, H, D, scale, dtype, 0, 0, stream);
}

extern "C" int mvi_attention_temporal_strided(const void* q, const void* k, const void* v, void* out, int32_t Bo, int32_t T,
                                              int32_t S, int32_t H, int32_t D, float scale, int32_t dtype,
                                              int64_t qkv_token_stride, int64_t out_token_stride, void* stream) {
    return attention_temporal_impl(q, k, v, out, Bo, T, S, H, D, scale, dtype, qkv_token_stride, out_token_stride, stream);
}

// q carries D^-1/2 log2(e): these kernels exponentiate with e, so ln 2 is the factor left to apply
extern "C" int mvi_attention_temporal_strided_qlog2(const void* q, const void* k, const void* v, void* out, int32_t Bo, int32_t T,
                                                    int32_t S, int32_t H, int32_t D, int32_t dtype, int64_t qkv_token_stride,
                                                    int64_t out_token_stride, void* stream) {
    return attention_temporal_impl(q, k, v, out, Bo, T, S, H, D, kLn2, dtype, qkv_token_stride, out_token_stride, stream);
}
