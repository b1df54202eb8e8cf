// Fused GEGLU for gfx950: out[r, j] = h[r, j] * gelu(h[r, inner + j]) (exact erf GELU), one pass.
// Replaces `x, gate = proj(x).chunk(2, -1); x * F.gelu(gate)`
// (svd_inpaint1/sgm/modules/attention.py:87-95), which PyTorch runs as a GELU over a strided view
// plus a strided multiply (3 full passes). HBM-bound: reads 2*inner, writes inner per row, 16 B/lane.
#include <hip/hip_runtime.h>

#include "geglu_math.h"
#include "unet_host.h"
#include "unet_io.h"

namespace mvi {

template <typename T>
__global__ __launch_bounds__(256) void geglu_kernel(const T* __restrict__ h, T* __restrict__ out, int64_t rows, int inner) {
    constexpr int N = Io<T>::kVec;
    const int vec_per_row = inner / N;
    const int64_t total = rows * vec_per_row;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
        const int64_t r = v / vec_per_row;
        const int j = (int)(v % vec_per_row) * N;
        float a[N], g[N];
        Io<T>::load(h + r * 2 * inner + j, a);
        Io<T>::load(h + r * 2 * inner + inner + j, g);
#pragma unroll
        for (int k = 0; k < N; ++k) a[k] *= gelu_erf(g[k]);
        Io<T>::store(out + r * inner + j, a);
    }
}

// dh[r, j] = dy[r, j] gelu(g), dh[r, inner + j] = dy[r, j] a gelu'(g) with a = h[r, j], g = h[r, inner + j]: fp32 math (geglu_math.h),
// reads 3 inner, writes 2 inner per row
template <typename T>
__global__ __launch_bounds__(256) void geglu_bwd_kernel(const T* __restrict__ h, const T* __restrict__ dy, T* __restrict__ dh, int64_t rows,
                                                        int inner) {
    constexpr int N = Io<T>::kVec;
    const int vec_per_row = inner / N;
    const int64_t total = rows * vec_per_row;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
        const int64_t r = v / vec_per_row;
        const int j = (int)(v % vec_per_row) * N;
        float a[N], g[N], d[N];
        Io<T>::load(h + r * 2 * inner + j, a);
        Io<T>::load(h + r * 2 * inner + inner + j, g);
        Io<T>::load(dy + r * inner + j, d);
#pragma unroll
        for (int k = 0; k < N; ++k) geglu_grad(a[k], g[k], d[k], a[k], g[k]);
        Io<T>::store(dh + r * 2 * inner + j, a);
        Io<T>::store(dh + r * 2 * inner + inner + j, g);
    }
}

template <typename T>
static int geglu_bwd_launch(const void* h, const void* dy, void* dh, int64_t rows, int inner, hipStream_t st) {
    const int64_t total = rows * (inner / Io<T>::kVec);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 256 * 64) blocks = 256 * 64;             // grid-stride the rest
    hipLaunchKernelGGL((geglu_bwd_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)h, (const T*)dy, (T*)dh, rows, inner);
    return hipGetLastError() == hipSuccess ? 0 : MVI_EHIP;
}

template <typename T>
static int geglu_launch(const void* h, void* out, int64_t rows, int inner, hipStream_t st) {
    const int64_t total = rows * (inner / Io<T>::kVec);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 256 * 64) blocks = 256 * 64;             // grid-stride the rest
    hipLaunchKernelGGL((geglu_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)h, (T*)out, rows, inner);
    return hipGetLastError() == hipSuccess ? 0 : MVI_EHIP;
}
}  // namespace mvi

extern "C" int mvi_geglu(const void* h, void* out, int64_t rows, int32_t inner, int32_t dtype, void* stream) {
    if (rows < 0 || inner <= 0) return mvi::unet_fail(MVI_EINVAL, "geglu: bad shape");
    if (rows == 0) return MVI_OK;
    if (!h || !out) return mvi::unet_fail(MVI_EINVAL, "geglu: NULL pointer");
    const int n = dtype == MVI_DT_F32 ? 4 : 8;
    if (inner % n != 0 || ((uintptr_t)h | (uintptr_t)out) % 16 != 0)
        return mvi::unet_fail(MVI_EINVAL, "geglu: inner must be a multiple of the 16-byte vector and pointers 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    return mvi::dispatch_dtype(dtype, "geglu: unknown dtype", [&](auto t) {
        return mvi::geglu_launch<typename decltype(t)::type>(h, out, rows, inner, st)
                   ? mvi::unet_fail(MVI_EHIP, "geglu: kernel launch failed") : MVI_OK;
    });
}

extern "C" int mvi_geglu_backward(const void* h, const void* dy, void* dh, int64_t rows, int32_t inner, int32_t dtype, void* stream) {
    if (rows < 0 || inner <= 0) return mvi::unet_fail(MVI_EINVAL, "geglu backward: bad shape");
    if (rows == 0) return MVI_OK;
    if (!h || !dy || !dh) return mvi::unet_fail(MVI_EINVAL, "geglu backward: NULL pointer");
    const int n = dtype == MVI_DT_F32 ? 4 : 8;
    if (inner % n != 0 || ((uintptr_t)h | (uintptr_t)dy | (uintptr_t)dh) % 16 != 0)
        return mvi::unet_fail(MVI_EINVAL, "geglu backward: inner must be a multiple of the 16-byte vector and pointers 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    return mvi::dispatch_dtype(dtype, "geglu backward: unknown dtype", [&](auto t) {
        return mvi::geglu_bwd_launch<typename decltype(t)::type>(h, dy, dh, rows, inner, st)
                   ? mvi::unet_fail(MVI_EHIP, "geglu backward: kernel launch failed") : MVI_OK;
    });
}
