// The gate arithmetic of GEGLU, y = a gelu(g) with gelu(g) = g Phi(g) = g/2 (1 + erf(g / sqrt 2)), once for every kernel that gates.
// Two forms, NOT interchangeable bit for bit:
//   * the polynomial (geglu1, geglu2, geglu_grad): the fused projections ff_geglu.hip and linear_n320.hip, and BOTH backward kernels
//     (ff_geglu_bwd.hip, geglu.hip's geglu_bwd_kernel) — the backward differentiates the function the fused forward computed;
//   * erff (gelu_erf): the elementwise forward geglu.hip's geglu_kernel, behind the library GEMM.
// The polynomial is Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7, below half an ulp of a bf16 / f16 output by four orders of
// magnitude) on v_rcp_f32 / v_exp_f32, branch-free: with z = |g| / sqrt 2, t = 1 / (1 + p z) and e = exp(-z^2) = exp(-g^2 / 2)
//     1 - erf z = poly(t) e,   poly(t) = a1 t + ... + a5 t^5
// Backward:  da = dy g Phi(g),  dg = dy a (Phi(g) + g phi(g)),  with Phi and phi from the SAME poly(t) and e:
//     Phi(-|g|) = poly(t) e / 2   (the tail itself, not 1 - something: no cancellation deep in the negative tail)
//     phi(g)    = e / sqrt(2 pi)
#pragma once
#include <hip/hip_runtime.h>

#include "mfma_common.h"      // f32x2

namespace mvi {

constexpr float kErfP = 0.3275911f, kErfA1 = 0.254829592f, kErfA2 = -0.284496736f, kErfA3 = 1.421413741f, kErfA4 = -1.453152027f,
                kErfA5 = 1.061405429f;
// (prefixed: kernel files that include this header keep constants such as kLog2e of their own)
constexpr float kGateRsqrt2 = 0.70710678118654752f, kGateLog2e = 1.4426950408889634f, kGateRsqrt2Pi = 0.3989422804014327f;

// The shared front of the polynomial forms: t, h = a1 + a2 t + ... + a5 t^4 (poly(t) = h t) and e = exp(-g^2 / 2). The last multiply
// is the caller's, and that is a CODE-GENERATION ACCOMMODATION, not a matter of the arithmetic: geglu1 negates the product, and this
// compiler (ROCm's clang for gfx950 at the time of writing) folds that negation into the multiply one way when it meets both in one
// function and the other way (same value, other device code: v_mul h, -t against v_mul t, -h) when the multiply arrives inside an
// already optimised helper. Keeping it outside left the six fused GEGLU kernels instruction for instruction what they were. To
// revisit on a compiler upgrade: move `* t` in here, return p, and check with tools/kernel_isa_diff.py what the kernels become.
struct ErfcParts { float t, h, e; };
__device__ __forceinline__ ErfcParts erfc_parts(float g) {
    const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(__builtin_fabsf(g), kErfP * kGateRsqrt2, 1.0f));
    float h = __builtin_fmaf(kErfA5, t, kErfA4);
    h = __builtin_fmaf(h, t, kErfA3);
    h = __builtin_fmaf(h, t, kErfA2);
    h = __builtin_fmaf(h, t, kErfA1);
    return {t, h, __builtin_amdgcn_exp2f(g * g * (-0.5f * kGateLog2e))};
}

// v * gelu(g): 14 instructions per output
__device__ __forceinline__ float geglu1(float v, float g) {
    const ErfcParts f = erfc_parts(g);
    const float p = f.h * f.t;
    const float erf_abs = __builtin_fmaf(-p, f.e, 1.0f);
    const float hg = 0.5f * g;                                   // g/2 (1 + sign(g) erf|z|) = g/2 + |g|/2 erf|z|
    return v * __builtin_fmaf(__builtin_fabsf(hg), erf_abs, hg);
}

// geglu1 on a PAIR of outputs with the packed fp32 instructions (v_pk_fma_f32 / v_pk_mul_f32: two lanes' worth per issue slot), for
// an epilogue with nothing on the matrix pipe (linear_n320.hip; beside MFMAs they were an anti-lever, round 5). |g| enters through
// the scalar fma's abs modifier (the packed forms have none).
__device__ __forceinline__ f32x2 geglu2(f32x2 v, f32x2 g) {
    const f32x2 d = {__builtin_fmaf(__builtin_fabsf(g.x), kErfP * kGateRsqrt2, 1.0f), __builtin_fmaf(__builtin_fabsf(g.y), kErfP * kGateRsqrt2, 1.0f)};
    const f32x2 t = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
    f32x2 p = t * kErfA5 + kErfA4;
    p = p * t + kErfA3;
    p = p * t + kErfA2;
    p = p * t + kErfA1;
    p = p * t;
    const f32x2 gg = g * g * (-0.5f * kGateLog2e);
    const f32x2 e = {__builtin_amdgcn_exp2f(gg.x), __builtin_amdgcn_exp2f(gg.y)};
    const f32x2 erf_abs = 1.0f - p * e;
    const f32x2 hg = 0.5f * g;
    const f32x2 s = {__builtin_fmaf(__builtin_fabsf(hg.x), erf_abs.x, hg.x), __builtin_fmaf(__builtin_fabsf(hg.y), erf_abs.y, hg.y)};
    return v * s;
}

// a, g, dy in fp32 -> da, dg in fp32. 20 instructions, branch-free (one select).
__device__ __forceinline__ void geglu_grad(float a, float g, float dy, float& da, float& dg) {
    const ErfcParts f = erfc_parts(g);
    const float p = f.h * f.t;
    const float tail = 0.5f * p * f.e;                           // Phi(-|g|)
    const float Phi = g < 0.f ? tail : 1.0f - tail;
    const float gphi = g * f.e * kGateRsqrt2Pi;                      // g phi(g)
    da = dy * (g * Phi);
    dg = dy * a * (Phi + gphi);
}

// the erff form
__device__ __forceinline__ float gelu_erf(float g) { return 0.5f * g * (1.0f + erff(g * kGateRsqrt2)); }

}  // namespace mvi
