// out[n, c, p] = h[n, c, p] + bias[c] (+ x[n, c, p]) for gfx950 — one pass over NC(T)HW activations.
// PyTorch-ROCm adds a convolution's bias as a separate broadcast kernel after the MIOpen kernel, and the
// ResBlock then adds the skip tensor in yet another pass (svd_inpaint1/sgm/modules/diffusionmodules/
// openaimodel.py:354 `self.skip_connection(x) + h`). The modules call their convolutions without bias and
// fold it here (or into the following GroupNorm's chan_bias). HBM-bound, 16 B per lane.
#include <hip/hip_runtime.h>

#include "unet_host.h"
#include "unet_io.h"

namespace mvi {

// alpha (optional, [N] fp32): out = x + (1 - alpha[n]) * (h + bias) — the AlphaBlender of a VideoResBlock applied to the
// temporal ResBlock's tail, alpha * x + (1 - alpha) * (x + h + bias), without materialising x + h + bias.
template <typename T, bool VEC, bool SILU = false>
__global__ __launch_bounds__(256) void bias_residual_kernel(const T* __restrict__ h, const T* __restrict__ x,
                                                            const float* __restrict__ bias, T* __restrict__ out,
                                                            int64_t total, int C, int64_t S,
                                                            const float* __restrict__ alpha = nullptr) {
    constexpr int N = Io<T>::kVec;
    if (VEC) {
        const int64_t nvec = total / N;
        for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * 256) {
            const int64_t e = v * N;
            const int64_t nc = e / S;                                  // S % N == 0: one channel per vector
            const float b = bias ? bias[nc % C] : 0.0f;
            const float wgt = alpha ? 1.0f - alpha[nc / C] : 1.0f;
            float a[N];
            Io<T>::load(h + e, a);
#pragma unroll
            for (int k = 0; k < N; ++k) a[k] = alpha ? wgt * (a[k] + b) : a[k];
            if (x) {
                float r[N];
                Io<T>::load(x + e, r);
#pragma unroll
                for (int k = 0; k < N; ++k) a[k] += r[k];
            }
#pragma unroll
            for (int k = 0; k < N; ++k) {
                if (!alpha) a[k] += b;
                if (SILU) a[k] = a[k] * __builtin_amdgcn_rcpf(1.0f + __expf(-a[k]));
            }
            Io<T>::store(out + e, a);
        }
    } else {
        for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
            const int64_t nc = e / S;
            float a = Io<T>::ld1(h + e) + (bias ? bias[nc % C] : 0.0f);
            if (alpha) a *= 1.0f - alpha[nc / C];
            if (x) a += Io<T>::ld1(x + e);
            if (SILU) a = a * __builtin_amdgcn_rcpf(1.0f + __expf(-a));
            Io<T>::st1(out + e, a);
        }
    }
}

template <typename T, bool SILU = false>
static int bias_residual_launch(const void* h, const void* x, const float* bias, void* out, int64_t total, int C, int64_t S,
                                hipStream_t st, const float* alpha = nullptr) {
    constexpr int N = Io<T>::kVec;
    const bool vec = (S % N == 0) && (((uintptr_t)h | (uintptr_t)x | (uintptr_t)out) % 16 == 0);
    int64_t work = vec ? total / N : total;
    int64_t blocks = (work + 255) / 256;
    if (blocks > 256 * 64) blocks = 256 * 64;
    if (blocks < 1) blocks = 1;
    if (vec)
        hipLaunchKernelGGL((bias_residual_kernel<T, true, SILU>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)h, (const T*)x, bias, (T*)out, total, C, S, alpha);
    else
        hipLaunchKernelGGL((bias_residual_kernel<T, false, SILU>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)h, (const T*)x, bias, (T*)out, total, C, S, alpha);
    return hipGetLastError() == hipSuccess ? 0 : MVI_EHIP;
}
// out[n] = (h[n] | skip[n] + ctrl[n]) along channels: the decoder's `torch.cat([h, hs.pop() + control.pop()], dim=1)`
// (models/csvd.py:79-91) without materialising the sum. blockIdx.y = sample; lanes walk the output row of that sample.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void concat_add_kernel(const T* __restrict__ h, const T* __restrict__ skip,
                                                         const T* __restrict__ ctrl, T* __restrict__ out,
                                                         int64_t n1, int64_t n2) {      // n1 = C1 * S, n2 = C2 * S
    constexpr int N = VEC ? Io<T>::kVec : 1;
    const int64_t n = blockIdx.y;
    const T* __restrict__ hp = h + n * n1;
    const T* __restrict__ sp = skip + n * n2;
    const T* __restrict__ cp = ctrl ? ctrl + n * n2 : nullptr;
    T* __restrict__ op = out + n * (n1 + n2);
    for (int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * N; e < n1 + n2; e += (int64_t)gridDim.x * 256 * N) {
        if (VEC) {
            float a[Io<T>::kVec];
            if (e < n1) {
                Io<T>::load(hp + e, a);
            } else {
                Io<T>::load(sp + (e - n1), a);
                if (cp) {
                    float r[Io<T>::kVec];
                    Io<T>::load(cp + (e - n1), r);
#pragma unroll
                    for (int k = 0; k < Io<T>::kVec; ++k) a[k] += r[k];
                }
            }
            Io<T>::store(op + e, a);
        } else {
            float a = e < n1 ? Io<T>::ld1(hp + e) : Io<T>::ld1(sp + (e - n1)) + (cp ? Io<T>::ld1(cp + (e - n1)) : 0.0f);
            Io<T>::st1(op + e, a);
        }
    }
}

template <typename T>
static int concat_add_launch(const void* h, const void* skip, const void* ctrl, void* out, int64_t N_, int64_t n1, int64_t n2,
                             hipStream_t st) {
    constexpr int V = Io<T>::kVec;
    const bool vec = n1 % V == 0 && n2 % V == 0 &&
                     (((uintptr_t)h | (uintptr_t)skip | (uintptr_t)ctrl | (uintptr_t)out) % 16 == 0);
    int64_t work = vec ? (n1 + n2) / V : n1 + n2;
    int64_t bx = (work + 255) / 256;
    if (bx > 4096) bx = 4096;
    if (bx < 1) bx = 1;
    const dim3 grid((unsigned)bx, (unsigned)N_);
    if (vec)
        hipLaunchKernelGGL((concat_add_kernel<T, true>), grid, dim3(256), 0, st, (const T*)h, (const T*)skip, (const T*)ctrl, (T*)out, n1, n2);
    else
        hipLaunchKernelGGL((concat_add_kernel<T, false>), grid, dim3(256), 0, st, (const T*)h, (const T*)skip, (const T*)ctrl, (T*)out, n1, n2);
    return hipGetLastError() == hipSuccess ? 0 : MVI_EHIP;
}
}  // namespace mvi

extern "C" int mvi_concat_add(const void* h, const void* skip, const void* ctrl, void* out, int64_t N, int32_t C1, int32_t C2,
                              int64_t spatial, int32_t dtype, void* stream) {
    if (N < 0 || N > 65535 || C1 < 0 || C2 < 0 || spatial < 0) return mvi::unet_fail(MVI_EINVAL, "concat_add: bad shape (N must be below 65536)");
    const int64_t n1 = (int64_t)C1 * spatial, n2 = (int64_t)C2 * spatial;
    if (N == 0 || n1 + n2 == 0) return MVI_OK;
    if ((n1 && !h) || (n2 && !skip) || !out) return mvi::unet_fail(MVI_EINVAL, "concat_add: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    return mvi::dispatch_dtype(dtype, "concat_add: unknown dtype", [&](auto t) {
        return mvi::concat_add_launch<typename decltype(t)::type>(h, skip, ctrl, out, N, n1, n2, st)
                   ? mvi::unet_fail(MVI_EHIP, "concat_add: kernel launch failed") : MVI_OK;
    });
}

extern "C" int mvi_bias_residual_add(const void* h, const void* x, const float* bias, void* out, int64_t N, int32_t C,
                                     int64_t spatial, int32_t dtype, void* stream) {
    if (N < 0 || C <= 0 || spatial < 0) return mvi::unet_fail(MVI_EINVAL, "bias_residual_add: bad shape");
    const int64_t total = N * C * spatial;
    if (total == 0) return MVI_OK;
    if (!h || !out) return mvi::unet_fail(MVI_EINVAL, "bias_residual_add: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    return mvi::dispatch_dtype(dtype, "bias_residual_add: unknown dtype", [&](auto t) {
        return mvi::bias_residual_launch<typename decltype(t)::type>(h, x, bias, out, total, C, spatial, st)
                   ? mvi::unet_fail(MVI_EHIP, "bias_residual_add: kernel launch failed") : MVI_OK;
    });
}

extern "C" int mvi_bias_residual_blend(const void* h, const void* x, const float* bias, const float* alpha, void* out, int64_t N,
                                       int32_t C, int64_t spatial, int32_t dtype, void* stream) {
    if (N < 0 || C <= 0 || spatial < 0) return mvi::unet_fail(MVI_EINVAL, "bias_residual_blend: bad shape");
    const int64_t total = N * C * spatial;
    if (total == 0) return MVI_OK;
    if (!h || !x || !alpha || !out) return mvi::unet_fail(MVI_EINVAL, "bias_residual_blend: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    return mvi::dispatch_dtype(dtype, "bias_residual_blend: unknown dtype", [&](auto t) {
        return mvi::bias_residual_launch<typename decltype(t)::type>(h, x, bias, out, total, C, spatial, st, alpha)
                   ? mvi::unet_fail(MVI_EHIP, "bias_residual_blend: kernel launch failed") : MVI_OK;
    });
}

extern "C" int mvi_bias_silu(const void* h, const float* bias, void* out, int64_t N, int32_t C, int64_t spatial, int32_t dtype,
                             void* stream) {
    if (N < 0 || C <= 0 || spatial < 0) return mvi::unet_fail(MVI_EINVAL, "bias_silu: bad shape");
    const int64_t total = N * C * spatial;
    if (total == 0) return MVI_OK;
    if (!h || !out) return mvi::unet_fail(MVI_EINVAL, "bias_silu: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    return mvi::dispatch_dtype(dtype, "bias_silu: unknown dtype", [&](auto t) {
        return mvi::bias_residual_launch<typename decltype(t)::type, true>(h, nullptr, bias, out, total, C, spatial, st)
                   ? mvi::unet_fail(MVI_EHIP, "bias_silu: kernel launch failed") : MVI_OK;
    });
}
