// Prefix-sum primitives of the binning and row-compaction kernels (wave64): the one definition of the wave scan, of the
// block scan over wave totals in LDS, and of the 1024-values-a-round row scan with its carry. Integer sums: exact.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mvi {

// inclusive scan over the 64 lanes of a wave; every lane of the wave must call it
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

// Exclusive scan over the 64 * WAVES threads of a block in thread order; every thread must call it. s_w: WAVES words of LDS.
// *total (may be null) receives the block's sum in every thread. One barrier, between the store of the wave totals and
// their reads: the caller puts a barrier of its own in front of the next write to s_w.
template <int WAVES>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, int tid, uint32_t* s_w, uint32_t* total) {
    const int lane = tid & 63, wave = tid >> 6;
    const uint32_t inc = wave_incl_scan(v, lane);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t off = 0, t = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const uint32_t c = s_w[w];
        if (w < wave) off += c;
        t += c;
    }
    if (total) *total = t;
    return off + inc - v;
}

// A 1024-thread block turns in[0, n) into exclusive offsets out[0, n), 1024 values a round with a running carry, and returns
// the total to every thread. in == out is allowed. s_wave: 16 words of LDS, s_carry: one, both written here only.
// Opens with a barrier: what the caller staged in LDS before the call is visible to the block after it.
__device__ __forceinline__ uint32_t row_excl_scan_1024(const uint32_t* in, uint32_t* out, int n, int tid, uint32_t* s_wave,
                                                       uint32_t* s_carry) {
    const int lane = tid & 63, wave = tid >> 6;
    if (tid == 0) *s_carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        const int i = base + tid;
        const uint32_t v = i < n ? in[i] : 0u;
        const uint32_t inc = wave_incl_scan(v, lane);
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        uint32_t wave_off = 0;
        for (int w = 0; w < wave; ++w) wave_off += s_wave[w];
        const uint32_t carry = *s_carry;
        if (i < n) out[i] = carry + wave_off + inc - v;
        __syncthreads();
        if (tid == 1023) *s_carry = carry + wave_off + inc;
        __syncthreads();
    }
    return *s_carry;
}

}  // namespace mvi
