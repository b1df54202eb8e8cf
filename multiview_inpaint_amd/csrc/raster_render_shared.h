// Device helpers shared by the render kernels (raster_render.hip: colour forward / backward; raster_render_aux.hip: the
// backward of the expected-depth and alpha outputs): the exact box cull, the tile order, the rounding recipe of the Gaussian's
// exponent and the nine-value wave sum. One text, so that every kernel that replays the forward takes its decisions.
#pragma once
#include "raster_common.h"

namespace mvi {

// ballot of a predicate that already lives in a lane mask: no 0/1 materialisation (__ballot(int) costs two VALU issues)
__device__ __forceinline__ unsigned long long ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }


// Per staged entry: t2 = 2 ln(255 o) (+ margin), the largest Mahalanobis distance^2 d^T conic d at which
// alpha = o exp(-d^T conic d / 2) still reaches 1/255; negative = can never be active.
__device__ __forceinline__ float active_t2(float4 co) {
    float t2 = 2.0f * __logf(255.0f * co.w);
    return t2 > 0.0f ? t2 * 1.001f + 0.01f : -1.0f;
}

// Exact conservative test "can any point of the pixel quadrant [qx0,qx0+7] x [qy0,qy0+7] be active?":
// the minimum of the convex form f(d) = A dx^2 + 2 B dx dy + C dy^2 over the box is 0 if the centre
// is inside; otherwise it lies on one of the (at most two) box edges facing the centre, where the
// 1-D minimiser is a clamped closed form. Continuous minimum <= minimum over pixel centres, and t2
// carries a margin that dwarfs the rcp / rounding error, so no active pair is ever dropped.
__device__ __forceinline__ bool quad_overlap(float2 c, float4 co, float t2, float qx0, float qy0, float bw = 7.0f,
                                             float bh = 7.0f) {
    const float dxl = qx0 - c.x, dxr = dxl + bw, dyl = qy0 - c.y, dyr = dyl + bh;
    const float px = fminf(fmaxf(0.0f, dxl), dxr), py = fminf(fmaxf(0.0f, dyl), dyr);   // box point nearest the centre, per axis
    // edge x = px: dy* = clamp(-B px / C); edge y = py: dx* = clamp(-B py / A)
    const float dy1 = fminf(fmaxf(-co.y * px * __builtin_amdgcn_rcpf(co.z), dyl), dyr);
    const float dx2 = fminf(fmaxf(-co.y * py * __builtin_amdgcn_rcpf(co.x), dxl), dxr);
    const float f1 = co.x * px * px + 2.0f * co.y * px * dy1 + co.z * dy1 * dy1;
    const float f2 = co.x * dx2 * dx2 + 2.0f * co.y * dx2 * py + co.z * py * py;
    // px == 0: only the y-facing edge matters (f2); py == 0: only f1; both 0: centre inside, f = 0
    const float f = px == 0.0f ? (py == 0.0f ? 0.0f : f2) : (py == 0.0f ? f1 : fminf(f1, f2));
    return f <= t2;
}

// Workgroups are handed to the 8 XCDs round-robin by linear id, and every XCD has its own L2. Tile t of a launch of
// `tiles` workgroups is chosen so that XCD x works through ONE contiguous band of tiles (rows of the image): the ~11
// tiles a Gaussian touches then gather its 40 bytes through the same L2 (and their gradient atomics meet there)
// instead of through up to 8 of them. (render_backward_kernel may take the tiles of its band in another ORDER, heaviest first:
// heaviest_first_tile in raster_render.hip; the band of a workgroup, bid & 7, is the same there.)
__device__ __forceinline__ int xcd_band_tile(int bid, int tiles) {
    const int q = tiles >> 3, r = tiles & 7, x = bid & 7, i = bid >> 3;
    return x * q + (x < r ? x : r) + i;
}

// ---- tile lists expanded on demand (binning version 2, mvi_raster_list_expansion(1)) -----------------------------------------
// The list of tile (row, column x) is the column segments [col_start[x], col_start[x + 1]) of pass 1 that cover the row
// (first row <= row <= first row + rows - 1), in segment order: pass 1 leaves a column's segments in depth order. A block of
// 256 threads walks its column with a block-uniform cursor and numbers the covering segments as pass 2 would have placed them.
// One step looks at kLazySubs sub-steps of kLazySub segments: a thread reads one aligned 4-byte word (two segments) per
// sub-step, every index clamped to the column's last word so that the four loads travel together; what lies outside
// [c0, c1) is dropped by the compare. Two ballots per sub-step give a thread its place among the wave's covering segments,
// the wave totals go through LDS (one barrier per step) and every thread sums the same totals: cursor and counts stay
// block-uniform without another exchange.
//   cur    first segment of the first sub-step that still holds an entry nobody consumed (even; starts at c0 & ~1)
//   have   covering segments of the column in front of `cur`
// emit(position, segment) is called for every covering segment whose position in the tile's list lies in [lo, hi). A sub-step
// is left behind (cur, have move past it) only when all its entries lie below `hi`; a sub-step that holds entries at or
// beyond `hi` is looked at again by the next call, which emits them when its own [lo, hi) names them: nothing is dropped,
// nothing emitted twice, and no queue can overflow because nothing is kept between calls but the two numbers. Returns the
// number of covering segments in front of the step's end: below `hi` means that all sub-steps were consumed and the caller
// goes on while cur < c1. s_tot: two buffers used in turn (`par`), so that a step's totals are not overwritten by the step
// after the next while a late wave still reads them. Every thread of the block calls it (barrier inside); c1 > c0.
constexpr int kLazySub = 512;
constexpr int kLazySubs = 4;
template <class Emit>
__device__ __forceinline__ uint32_t lazy_list_step(const uint16_t* __restrict__ seg_yh, uint32_t c0, uint32_t c1, uint32_t row,
                                                   uint32_t& cur, uint32_t& have, uint32_t lo, uint32_t hi,
                                                   uint32_t (*s_tot)[kLazySubs * 4], int& par, int tid, Emit emit) {
    const int lane = tid & 63, wave = tid >> 6;
    const uint32_t* yh2 = reinterpret_cast<const uint32_t*>(seg_yh);      // the array starts 256-byte aligned
    const uint32_t dlast = (c1 - 1u) >> 1;                                // word of the column's last segment
    uint32_t w[kLazySubs];
#pragma unroll
    for (int j = 0; j < kLazySubs; ++j) w[j] = yh2[min((cur >> 1) + (uint32_t)(j * (kLazySub / 2) + tid), dlast)];
    unsigned long long m0[kLazySubs], m1[kLazySubs];
    bool k0[kLazySubs], k1[kLazySubs];
    uint32_t* tot = s_tot[par];
    par ^= 1;
#pragma unroll
    for (int j = 0; j < kLazySubs; ++j) {
        const uint32_t s0 = cur + (uint32_t)(j * kLazySub + 2 * tid), s1 = s0 + 1u;
        k0[j] = s0 >= c0 && s0 < c1 && (row - (w[j] & 255u)) <= ((w[j] >> 8) & 255u);
        k1[j] = s1 >= c0 && s1 < c1 && (row - ((w[j] >> 16) & 255u)) <= (w[j] >> 24);
        m0[j] = ballot64(k0[j]);
        m1[j] = ballot64(k1[j]);
        if (lane == 0) tot[j * 4 + wave] = (uint32_t)(__popcll(m0[j]) + __popcll(m1[j]));
    }
    __syncthreads();
    uint32_t base = have, consumed = 0;
    bool open = true;
#pragma unroll
    for (int j = 0; j < kLazySubs; ++j) {
        const uint32_t t0 = tot[j * 4], t1 = tot[j * 4 + 1], t2 = tot[j * 4 + 2], t3 = tot[j * 4 + 3];
        if (base < hi) {                                                  // block-uniform
            const uint32_t off = base + (wave > 0 ? t0 : 0u) + (wave > 1 ? t1 : 0u) + (wave > 2 ? t2 : 0u);
            const uint32_t b0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m0[j] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0[j], 0u));
            const uint32_t b1 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m1[j] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1[j], 0u));
            const uint32_t p0 = off + b0 + b1, p1 = p0 + (k0[j] ? 1u : 0u);
            const uint32_t s0 = cur + (uint32_t)(j * kLazySub + 2 * tid);     // cur: still the step's start
            if (k0[j] && p0 >= lo && p0 < hi) emit(p0, s0);
            if (k1[j] && p1 >= lo && p1 < hi) emit(p1, s0 + 1u);
        }
        base += t0 + t1 + t2 + t3;
        open = open && base <= hi;
        if (open) { have = base; consumed = (uint32_t)(j + 1); }
    }
    cur += consumed * (uint32_t)kLazySub;
    return base;
}

typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 splat(float v) { return f2{v, v}; }
constexpr int kB2 = 128;                // threads per tile in the backward kernel: 2 wave64, two pixels per lane

// power = -0.5 (A dx^2 + C dy^2) - B dx dy for the lane's two pixels (same x, adjacent y), ONE rounding recipe shared by
// the forward and the backward kernel so the backward replays the forward's alpha / threshold decisions exactly:
// products rounded, fma(dx, A dx, (C dy) dy), then fma(., -0.5, -(B dx) dy).
__device__ __forceinline__ f2 gauss_power(float4 co, float dx, f2 dy) {
#pragma clang fp contract(off)
    const float ax = co.x * dx, bx = co.y * dx;
    const f2 cyy = (co.z * dy) * dy;
    const f2 sq = pk_fma(splat(dx), splat(ax), cyy);
    const f2 bxy = bx * dy;
    return pk_fma(sq, splat(-0.5f), -bxy);
}

__device__ __forceinline__ float gauss_power1(float4 co, float dx, float dy) {     // the same recipe, one pixel
#pragma clang fp contract(off)
    const float ax = co.x * dx, bx = co.y * dx;
    const float cyy = (co.z * dy) * dy;
    const float sq = __builtin_fmaf(dx, ax, cyy);
    const float bxy = bx * dy;
    return __builtin_fmaf(sq, -0.5f, -bxy);
}

constexpr int kRow = 16;

// Wave totals of nine values by a halving butterfly: one level per bit of the lane index, and at every level TWO live
// registers are folded into ONE that carries the first value's partial sums in the lanes whose bit is 0 and the second
// value's in the lanes whose bit is 1 (9 -> 5 -> 3 -> 2 -> 1 registers); the odd register of a level takes a plain
// full-width step and carries its partial sums in both halves. Levels, in order:
//   bit 3, bit 2   two v_add_f32_dpp per pair, each writing half of the banks of a row (row_ror:n reads lane (l - n) mod 16
//                  of the own row of 16: ror 8 is the partner l ^ 8 for every lane; ror 12 / ror 4 is l ^ 4 for the lanes with
//                  bit 2 clear / set); one full-width add for the odd register (its partial sums no longer depend on bit 3
//                  when bit 2 is folded, so ror 4 reads a value equal to the partner's in every lane)
//   bit 4, bit 5   v_permlane16_swap / v_permlane32_swap exchange the odd rows (upper half) of the first register with
//                  the even rows (lower half) of the second, then one plain add
//   bit 0, bit 1   two quad_perm adds on the one register that is left
// Lane <-> moment map of the result (a compile-time function of the lane, wave_sum9_moment): lane l < 32 holds the wave
// total of argument (l >> 2), lanes 32..63 hold that of argument 8, every lane of a quad the same number. Lanes 0, 4, ..,
// 32 are the nine owners (wave_sum9_owner). The sum is a balanced tree over the 64 lanes.
// The DPP adds are asm because the compiler lowers update_dpp + add to v_mov_b32_dpp + v_add (two issues each; the
// kernel is VALU-issue-bound). The s_nop in front covers the VALU-write -> DPP-read hazard for whatever precedes a block
// (the assembler does not pad inline asm, and the compiler does not look into it; it does pad the swaps that read a
// block's outputs); inside the first block every register is re-read at least four instructions after it was written.
__device__ __forceinline__ constexpr int wave_sum9_moment(int lane) { return lane < 32 ? lane >> 2 : 8; }
__device__ __forceinline__ constexpr bool wave_sum9_owner(int lane) { return (lane & 3) == 0 && lane <= 32; }
#define MVI_FOLD(a, b, lo, hi, mlo, mhi)                                                                  \
    "v_add_f32_dpp " a ", " a ", " a " row_ror:" lo " row_mask:0xf bank_mask:" mlo "\n\t"                  \
    "v_add_f32_dpp " a ", " b ", " b " row_ror:" hi " row_mask:0xf bank_mask:" mhi "\n\t"
#define MVI_FULL(a, n) "v_add_f32_dpp " a ", " a ", " a " row_ror:" n " row_mask:0xf bank_mask:0xf\n\t"
__device__ __forceinline__ float wave_sum9(float m0, float m1, float m2, float m3, float m4, float m5, float m6, float m7,
                                           float m8) {
    asm("s_nop 1\n\t"
        // bit 3: (m0, m2) -> m0, (m1, m3) -> m1, (m4, m6) -> m4, (m5, m7) -> m5: lanes 0..7 of a row | lanes 8..15
        MVI_FOLD("%0", "%2", "8", "8", "0x3", "0xc") MVI_FOLD("%1", "%3", "8", "8", "0x3", "0xc")
        MVI_FOLD("%4", "%6", "8", "8", "0x3", "0xc") MVI_FOLD("%5", "%7", "8", "8", "0x3", "0xc") MVI_FULL("%8", "8")
        // bit 2: (m0, m1) -> m0, (m4, m5) -> m4: banks 0 and 2 | banks 1 and 3. Lane bits (3, 2) of m0 now name 2 a + b
        MVI_FOLD("%0", "%1", "12", "4", "0x5", "0xa") MVI_FOLD("%4", "%5", "12", "4", "0x5", "0xa") MVI_FULL("%8", "4")
        : "+v"(m0), "+v"(m1), "+v"(m2), "+v"(m3), "+v"(m4), "+v"(m5), "+v"(m6), "+v"(m7), "+v"(m8));
    // bit 4: rows 0, 2 <- m0..m3, rows 1, 3 <- m4..m7; the odd register is folded with itself
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(m0), __float_as_uint(m4), false, false);
    const auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(m8), __float_as_uint(m8), false, false);
    const float lo = __uint_as_float(a[0]) + __uint_as_float(a[1]), hi = __uint_as_float(b[0]) + __uint_as_float(b[1]);
    // bit 5: lanes 0..31 <- m0..m7, lanes 32..63 <- m8
    const auto c = __builtin_amdgcn_permlane32_swap(__float_as_uint(lo), __float_as_uint(hi), false, false);
    float s = __uint_as_float(c[0]) + __uint_as_float(c[1]);
    asm("s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf"
        : "+v"(s));
    return s;
}
#undef MVI_FOLD
#undef MVI_FULL

}  // namespace mvi
