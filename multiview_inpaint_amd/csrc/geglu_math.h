// The gate of the GEGLU backward, shared by the fused kernel (ff_geglu_bwd.hip) and the elementwise one (geglu.hip).
//     y = a gelu(g), gelu(g) = g Phi(g)  =>  da = dy g Phi(g),  dg = dy a (Phi(g) + g phi(g))
// Phi from the forward's erf polynomial (ff_geglu.hip, geglu1: Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7), phi from the SAME
// exp2: with z = |g| / sqrt 2, t = 1 / (1 + p z) and e = exp(-g^2 / 2):  1 - erf z = poly(t) e, so
//     Phi(-|g|) = poly(t) e / 2   (the tail itself, not 1 - something: no cancellation deep in the negative tail)
//     phi(g)    = e / sqrt(2 pi)
#pragma once
#include <hip/hip_runtime.h>

namespace mvi {

// a, g, dy in fp32 -> da, dg in fp32. 20 instructions, branch-free (one select).
__device__ __forceinline__ void geglu_grad(float a, float g, float dy, float& da, float& dg) {
    const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(__builtin_fabsf(g), 0.3275911f * 0.70710678118654752f, 1.0f));
    float p = __builtin_fmaf(1.061405429f, t, -1.453152027f);
    p = __builtin_fmaf(p, t, 1.421413741f);
    p = __builtin_fmaf(p, t, -0.284496736f);
    p = __builtin_fmaf(p, t, 0.254829592f);
    p *= t;
    const float e = __builtin_amdgcn_exp2f(g * g * (-0.5f * 1.4426950408889634f));   // e^(-g^2 / 2)
    const float tail = 0.5f * p * e;                             // Phi(-|g|)
    const float Phi = g < 0.f ? tail : 1.0f - tail;
    const float gphi = g * e * 0.3989422804014327f;              // g phi(g)
    da = dy * (g * Phi);
    dg = dy * a * (Phi + gphi);
}

}  // namespace mvi
