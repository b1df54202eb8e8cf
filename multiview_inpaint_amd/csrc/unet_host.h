// The host side that the UNet kernel files share: the status codes and dtype tags of the C ABI, the error record, and the
// dtype -> and flag -> template-argument dispatch of the entry points, and the opt-in of a kernel to more than 64 KiB of dynamic LDS.
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

#include "../../include/mvi_raster.h"        // MVI_OK / MVI_E*
#include "../../include/mvi_unet_ops.h"      // MVI_DT_*

namespace mvi {

int unet_fail(int code, const char* msg);       // records msg for mvi_unet_last_error (groupnorm_silu.hip), returns code

// f is a generic lambda that receives the element type as a tag and returns a status:
//     return dispatch_dtype(dtype, "op: unknown dtype", [&](auto t) { return op_launch<typename decltype(t)::type>(...); });
// Returns what f returned, or unet_fail(MVI_EINVAL, what) for a dtype outside the set. For sites that choose nothing but T.
template <typename T> struct DtypeTag { using type = T; };

template <typename F> int dispatch_dtype(int dtype, const char* what, F&& f) {           // fp32, bf16, f16
    switch (dtype) {
        case MVI_DT_F32: return f(DtypeTag<float>{});
        case MVI_DT_BF16: return f(DtypeTag<__hip_bfloat16>{});
        case MVI_DT_F16: return f(DtypeTag<__half>{});
        default: return unet_fail(MVI_EINVAL, what);
    }
}
template <typename F> int dispatch_dtype16(int dtype, const char* what, F&& f) {         // bf16, f16: the MFMA kernels
    switch (dtype) {
        case MVI_DT_BF16: return f(DtypeTag<__hip_bfloat16>{});
        case MVI_DT_F16: return f(DtypeTag<__half>{});
        default: return unet_fail(MVI_EINVAL, what);
    }
}

// The same for a bool template argument: f receives std::true_type or std::false_type and the site spells its launch once,
//     dispatch_flag(stats != nullptr, [&](auto k) { hipLaunchKernelGGL((kernel<T, decltype(k)::value>), ...); });
template <typename F> auto dispatch_flag(bool on, F&& f) { return on ? f(std::true_type{}) : f(std::false_type{}); }

// A launch with more than 64 KiB of dynamic LDS needs hipFuncAttributeMaxDynamicSharedMemorySize set on the kernel, once per device.
// kKern is the kernel's address, so the flag word (one bit per device) is per kernel by construction. Launchers run on any thread
// (autograd's backward has one per device): the bit is published with release and read with acquire; two threads that both find it
// clear both set the attribute, which is harmless. 0 or MVI_EHIP.
template <auto kKern> int allow_large_lds(int bytes) {
    static std::atomic<unsigned long long> attr_set{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return MVI_EHIP;
    if (!(attr_set.load(std::memory_order_acquire) >> dev & 1ull)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kKern), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
            return MVI_EHIP;
        attr_set.fetch_or(1ull << dev, std::memory_order_release);
    }
    return 0;
}

}  // namespace mvi
