// What the MFMA kernels of this directory share: register vector types, the I/O-type conversions, the three forms of the matrix
// instruction (builtin 16x16x32, builtin 32x32x16, tied inline assembly 16x16x32) and the LDS-DMA piece. A kernel file names the
// form it runs on (`template <typename T> using Mma = MmaBuiltin16<T>;`) and keeps its tile constants.
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
// The Mma forms below derive from this and add mfma().
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

// c + A B through the builtin: the compiler schedules it and keeps the wait states
template <typename T> struct MmaBuiltin16;               // v_mfma_f32_16x16x32
template <> struct MmaBuiltin16<__hip_bfloat16> : MmaType<__hip_bfloat16> {
    __device__ static f32x4 mfma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct MmaBuiltin16<__half> : MmaType<__half> {
    __device__ static f32x4 mfma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <typename T> struct MmaBuiltin32;               // v_mfma_f32_32x32x16
template <> struct MmaBuiltin32<__hip_bfloat16> : MmaType<__hip_bfloat16> {
    __device__ static f32x16 mfma(frag a, frag b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct MmaBuiltin32<__half> : MmaType<__half> {
    __device__ static f32x16 mfma(frag a, frag b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
// c += A B on v_mfma_f32_16x16x32, IN PLACE and in program order. Through the builtin the register allocator took the untied form
// for two MFMAs in three of linear_n320's loop, rotated the forty 4-register accumulators through the W fragments' registers
// (write-after-read stalls on the next ds_read) and spilled; as volatile assembly the loop is issued as written. The compiler does
// not know these are matrix instructions: the KERNEL owns the wait states between the last of them and the first ordinary read or
// write of an accumulator (linear_n320.hip: mfma_settle; ff_geglu.hip writes them out).
template <typename T> struct MmaTied16;
template <> struct MmaTied16<__hip_bfloat16> : MmaType<__hip_bfloat16> {
    __device__ static void mfma(f32x4& c, u32x4 a, u32x4 b) { asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b)); }
};
template <> struct MmaTied16<__half> : MmaType<__half> {
    __device__ static void mfma(f32x4& c, u32x4 a, u32x4 b) { asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b)); }
};

template <typename F> __device__ __forceinline__ F as_frag(u32x4 v) { return *reinterpret_cast<F*>(&v); }

// An MFMA operand fragment read TRANSPOSED from a row-major [contraction row][channel] LDS image (the weight-gradient kernels: both
// operands are contracted along their slow index): two ds_read_b64_tr_b16, each a 16-row x 16-channel block of which lane 4 q + p
// of 16-lane group g addresses row 4 g + q, channels 4 p .. 4 p + 3 (p is the lane's own address); hi_bytes = 16 rows further on.
// Element j of lane (c, g) is row (j < 4 ? 4 g + j : 16 + 4 g + j - 4) of the 32-row step at channel c.
template <typename F> __device__ __forceinline__ F read_frag_tr(MVI_AS3 char* p, uint32_t hi_bytes) {
    s16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MVI_AS3 s16x4*)p);
    s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MVI_AS3 s16x4*)(p + hi_bytes));
    const u32x2 l = *reinterpret_cast<u32x2*>(&lo4), h = *reinterpret_cast<u32x2*>(&hi4);
    return as_frag<F>(u32x4{l[0], l[1], h[0], h[1]});
}

// One LDS-DMA piece: every lane moves 16 bytes from sbase + voff to LDS address (m0 + 16 * lane); sbase is wave-uniform (scalar
// registers). Invisible to the compiler's wait-count bookkeeping on purpose: the kernels count their own vmcnt (a builtin DMA makes
// hipcc put s_waitcnt vmcnt(0) in front of every later LDS read, which serialises a ring of tiles).
__device__ __forceinline__ void dma_piece(const void* sbase, uint32_t voff, uint32_t lds_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %0" ::"s"(sbase), "v"(voff), "s"(lds_addr) : "memory");
}

}  // namespace mvi
