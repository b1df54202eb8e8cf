// The host side that the UNet kernel files share: the status codes and dtype tags of the C ABI, the error record, and the
// dtype -> template-argument dispatch of the entry points.
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

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

}  // namespace mvi
