// What the MFMA kernels of this directory share: register vector types, the I/O-type conversions and the LDS-DMA piece. What differs
// from kernel to kernel stays in its file: the matrix instruction itself (`Mma<T>::mfma`: builtin 32x32x16, builtin 16x16x32, or
// tied inline assembly) and the tile constants.
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mvi {

typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
#define MVI_AS3 __attribute__((address_space(3)))

// Per I/O type: the MFMA operand fragment of 8 elements, two floats -> one packed dword (round to nearest even) and back.
// A kernel's Mma<T> derives from this and adds its mfma().
template <typename T> struct MmaType;
template <> struct MmaType<__hip_bfloat16> {
    using frag = bf16x8;
    __device__ static uint32_t pack2(float lo, float hi) {     // one v_cvt_pk_bf16_f32
        f32x2 f = {lo, hi};
        bf16x2 r = __builtin_convertvector(f, bf16x2);
        return *reinterpret_cast<uint32_t*>(&r);
    }
    __device__ static float lo(uint32_t w) { return __uint_as_float(w << 16); }
    __device__ static float hi(uint32_t w) { return __uint_as_float(w & 0xFFFF0000u); }
};
template <> struct MmaType<__half> {
    using frag = f16x8;
    __device__ static uint32_t pack2(float lo, float hi) {
        f32x2 f = {lo, hi};
        f16x2 r = __builtin_convertvector(f, f16x2);
        return *reinterpret_cast<uint32_t*>(&r);
    }
    __device__ static float lo(uint32_t w) { f16x2 h = *reinterpret_cast<f16x2*>(&w); return (float)h[0]; }
    __device__ static float hi(uint32_t w) { f16x2 h = *reinterpret_cast<f16x2*>(&w); return (float)h[1]; }
};

template <typename F> __device__ __forceinline__ F as_frag(u32x4 v) { return *reinterpret_cast<F*>(&v); }

// One LDS-DMA piece: every lane moves 16 bytes from sbase + voff to LDS address (m0 + 16 * lane); sbase is wave-uniform (scalar
// registers). Invisible to the compiler's wait-count bookkeeping on purpose: the kernels count their own vmcnt (a builtin DMA makes
// hipcc put s_waitcnt vmcnt(0) in front of every later LDS read, which serialises a ring of tiles).
__device__ __forceinline__ void dma_piece(const void* sbase, uint32_t voff, uint32_t lds_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %0" ::"s"(sbase), "v"(voff), "s"(lds_addr) : "memory");
}

}  // namespace mvi
