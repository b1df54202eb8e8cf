// Feature splat for gfx950: up to eight per-Gaussian feature channels composited into a finished forward's view,
//     out[c][p] = sum_i alpha_i(p) T_i(p) F[i][c]
// over exactly the (pixel, Gaussian) pairs the forward composited: the entries [0, n_contrib) of a pixel's tile list that pass
// the forward's tests (power <= 0, o G >= 1/255), alpha = min(0.99, o G), taken with the forward's rounding recipe (gauss_power1).
// It is the transpose of the lift (raster_lift.hip): the lift is its backward with respect to F. The list is replayed FRONT TO
// BACK: T starts at 1 and becomes T (1 - alpha) behind every passing entry, the weight is alpha T with the T in front of the
// entry, and a channel takes one fma(F, w, acc) per passing entry in list order: render_forward_kernel's `entry`, so that the
// splat of a forward's own colours is that forward's colour image at zero background bit for bit. Neither final_T nor a colour
// is read (pending deferred colours do not matter) and nothing but `out` is written; no atomics.
//
// Shape: the forward's. One block of 256 threads = 4 wave64 per tile, a wave covers an 8 x 8 quadrant with one pixel per lane
// whose eight sums sit in registers. The loop length is known up front (the forward's is not): a wave replays the list up to the
// largest n_contrib of its pixels, the block stages the positions below the largest of its four waves, 256 entries per round,
// one entry per thread: (x, y, t2), conic + opacity and the entry's `channels` features, which the staging lane gathers with
// dword loads (rows of any stride and any 4-byte alignment: the lift's acc[:, 1 : 1 + C] goes in as it is). Per wave the staged
// entries are culled 64 at a time with the exact box test, and the kept ones are walked in list order by a wave-uniform loop
// over the ballot: every read of an entry is an LDS broadcast.
#include "raster_common.h"
#include "raster_render_shared.h"

namespace mvi {

constexpr int kSplatChannels = 8;

__global__ __launch_bounds__(kBlock) void splat_features_kernel(
    Frame f, const uint32_t* __restrict__ ranges, const uint32_t* __restrict__ point_list, const float2* __restrict__ xy,
    const float4* __restrict__ conic_opacity, const uint32_t* __restrict__ n_contrib, const float* __restrict__ features,
    int channels, int feat_stride, float* __restrict__ out) {
    __shared__ float4 s_a[kBlock];                                    // x, y, t2, -
    __shared__ float4 s_co[kBlock];
    __shared__ float4 s_f[2][kBlock];                                 // channels 0..3 | 4..7; zero past `channels`
    __shared__ uint32_t s_wlast[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tile = xcd_band_tile(blockIdx.x, f.gx * f.gy);
    const int tile_y = tile / f.gx, tile_x = tile - tile_y * f.gx;
    const int qx0 = tile_x * kTile + 8 * (wave & 1), qy0 = tile_y * kTile + 8 * (wave >> 1);
    const int pxi = qx0 + (lane & 7), pyi = qy0 + (lane >> 3);
    const bool inside = pxi < f.W && pyi < f.H;
    const float pfx = (float)pxi, pfy = (float)pyi;
    const uint32_t r0 = ranges[2 * tile], r1 = ranges[2 * tile + 1];
    const size_t pix = (size_t)pyi * f.W + pxi, plane = (size_t)f.W * f.H;
    const uint32_t held = r1 > r0 ? r1 - r0 : 0u;                     // entries of the tile's list
    const uint32_t last = inside ? min(n_contrib[pix], held) : 0u;     // never past the list, whatever the state holds
    const uint32_t wave_last = wave_umax(last);
    if (lane == 0) s_wlast[wave] = wave_last;
    __syncthreads();
    const int total = (int)max(max(s_wlast[0], s_wlast[1]), max(s_wlast[2], s_wlast[3]));
    const int rounds = (total + kBlock - 1) / kBlock;

    float T = 1.0f;
    float acc[kSplatChannels];
#pragma unroll
    for (int c = 0; c < kSplatChannels; ++c) acc[c] = 0.0f;

    // software pipeline: the gathers of round r + 1 are issued before round r is composited
    float2 n_xy = make_float2(0.f, 0.f);
    float4 n_co = make_float4(0.f, 0.f, 0.f, 0.f);                     // opacity 0: t2 < 0, culled
    float n_f[kSplatChannels];
#pragma unroll
    for (int c = 0; c < kSplatChannels; ++c) n_f[c] = 0.0f;
    auto fetch = [&](int r) {
        const int pos = r * kBlock + tid;
        if (pos < total) {
            const uint32_t id = point_list[r0 + (uint32_t)pos];
            if (id < (uint32_t)f.P) {
                n_xy = xy[id]; n_co = conic_opacity[id];
                const float* row = features + (size_t)id * (size_t)feat_stride;
#pragma unroll
                for (int c = 0; c < kSplatChannels; ++c)
                    if (c < channels) n_f[c] = row[c];
            } else {
                n_co = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };
    if (rounds > 0) fetch(0);
    for (int r = 0; r < rounds; ++r) {
        const int base = r * kBlock;
        const int n = total - base < kBlock ? total - base : kBlock;
        __syncthreads();
        s_a[tid] = make_float4(n_xy.x, n_xy.y, active_t2(n_co), 0.f);
        s_co[tid] = n_co;
        s_f[0][tid] = make_float4(n_f[0], n_f[1], n_f[2], n_f[3]);
        s_f[1][tid] = make_float4(n_f[4], n_f[5], n_f[6], n_f[7]);
        __syncthreads();
        if (r + 1 < rounds) fetch(r + 1);
        for (int c = 0; c < n; c += 64) {
            if ((uint32_t)(base + c) >= wave_last) break;               // wave-uniform: this wave's pixels are done
            const int e = c + lane;                                      // < kBlock: n <= kBlock and c is a multiple of 64
            const float4 ce = s_a[e];
            const bool keep = e < n && (uint32_t)(base + e) < wave_last &&
                              quad_overlap(make_float2(ce.x, ce.y), s_co[e], ce.z, (float)qx0, (float)qy0);
            unsigned long long mask = ballot64(keep);
            while (mask != 0ull) {
                const int jc = c + __builtin_ctzll(mask);               // wave-uniform, < n; ascending = list order
                mask &= mask - 1;
                const float4 a = s_a[jc], co = s_co[jc];
                const float dx = a.x - pfx, dy = a.y - pfy;
                const float power = gauss_power1(co, dx, dy);           // the forward's rounding recipe
                float alpha = fminf(kAlphaMax, co.w * __expf(power));
                alpha = power <= 0.0f ? alpha : 0.0f;
                const bool pass = alpha >= kAlphaMin && (uint32_t)(base + jc) < last;
                const float w = pass ? alpha * T : 0.0f;                // T in front of the entry
                T = pass ? T * (1.0f - alpha) : T;
                const float4 f0 = s_f[0][jc];
                acc[0] = __builtin_fmaf(f0.x, w, acc[0]);
                acc[1] = __builtin_fmaf(f0.y, w, acc[1]);
                acc[2] = __builtin_fmaf(f0.z, w, acc[2]);
                acc[3] = __builtin_fmaf(f0.w, w, acc[3]);
                if (channels > 4) {                                      // uniform
                    const float4 f1 = s_f[1][jc];
                    acc[4] = __builtin_fmaf(f1.x, w, acc[4]);
                    acc[5] = __builtin_fmaf(f1.y, w, acc[5]);
                    acc[6] = __builtin_fmaf(f1.z, w, acc[6]);
                    acc[7] = __builtin_fmaf(f1.w, w, acc[7]);
                }
            }
        }
    }
    if (inside) {
#pragma unroll
        for (int c = 0; c < kSplatChannels; ++c)
            if (c < channels) out[c * plane + pix] = acc[c];
    }
}

int launch_splat_features(const Frame& f, GeomView g, BinningView b, ImageView im, int64_t D, const float* features, int channels,
                          int feat_stride, float* out, hipStream_t st) {
    if (f.W <= 0 || f.H <= 0 || D <= 0 || f.P <= 0) return 0;             // nothing composited
    const uint32_t* plist = b.vals[b.passes & 1];
    hipLaunchKernelGGL(splat_features_kernel, dim3(f.gx * f.gy), dim3(kBlock), 0, st, f, im.ranges, plist, g.xy, g.conic_opacity,
                       im.n_contrib, features, channels, feat_stride, out);
    return hipGetLastError() == hipSuccess ? 0 : MVI_EHIP;
}

}  // namespace mvi
