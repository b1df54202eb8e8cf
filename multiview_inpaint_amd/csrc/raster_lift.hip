// Mask lifting for gfx950: the blend weight every Gaussian received in a finished forward, and the same weighted by up to eight
// per-pixel images (2-D masks carried onto the Gaussians by a contribution-weighted vote, summed over views by the caller):
//     total_i = sum_p alpha_i(p) T_i(p)          hit_i,c = sum_p alpha_i(p) T_i(p) w_c(p)
// over exactly the (pixel, Gaussian) pairs the forward composited: the entries [0, n_contrib) of a pixel's tile list that pass
// the forward's tests (power <= 0, o G >= 1/255), alpha = min(0.99, o G), taken with the forward's rounding recipe (gauss_power).
// T_i(p), the transmittance in front of entry i, is rebuilt back to front from final_T by T / (1 - alpha), as the backward
// kernels rebuild it. No colour is read and nothing but the output rows is written.
//
// Shape: render_backward_aux_kernel's (raster_render_aux.hip). One block of 128 threads = 2 wave64 per tile, a wave covers a
// 16 x 8 half tile with two vertically adjacent pixels per lane, whose 2 x channels weights sit in registers; the tile's list is
// staged through LDS back to front, 128 entries per round, culled per wave with the exact box test; per evaluated entry the
// lane's two pixels are added, wave_sum9 sums the total and the eight hits over the wave in registers, 1 + channels lanes add
// the wave totals into the block's per-entry LDS accumulator; once per staged batch the entries somebody evaluated are flushed
// with float atomics into acc[id][0 .. channels] (16 lanes per entry: one request per Gaussian while a row stays inside a
// 64-byte line). Tiles go through xcd_band_tile, so the atomics of a Gaussian meet in one L2.
#include "raster_common.h"
#include "raster_render_shared.h"

namespace mvi {

constexpr int kLiftChannels = 8;        // wave_sum9 sums nine values: the total and eight hits

__global__ __launch_bounds__(kB2) void lift_weights_kernel(
    Frame f, const uint32_t* __restrict__ ranges, const uint32_t* __restrict__ point_list, const float2* __restrict__ xy,
    const float4* __restrict__ conic_opacity, const float* __restrict__ final_T, const uint32_t* __restrict__ n_contrib,
    const float* __restrict__ weights, int channels, float* __restrict__ acc, int acc_stride) {
#pragma clang fp contract(off)
    // a staged entry is one record: [0] (x, y, t2, Gaussian id), [1] conic + opacity
    __shared__ float4 s_ent[2][kB2];
    __shared__ float s_acc[kB2][9];                                   // wave totals per staged entry (wave_sum9's stride)
    __shared__ uint32_t s_blast[2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tile = xcd_band_tile(blockIdx.x, f.gx * f.gy);
    const int tile_y = tile / f.gx, tile_x = tile - tile_y * f.gx;
    const int hx0 = tile_x * kTile, hy0 = tile_y * kTile + 8 * wave;                  // this wave's 16 x 8 half tile
    const int pxi = hx0 + (lane & 15), py0 = hy0 + 2 * (lane >> 4), py1 = py0 + 1;
    const bool in0 = pxi < f.W && py0 < f.H, in1 = pxi < f.W && py1 < f.H;
    const float pfx = (float)pxi;
    const f2 pfy = {(float)py0, (float)py1};
    const uint32_t r0 = ranges[2 * tile];
    const size_t pix0 = (size_t)py0 * f.W + pxi, pix1 = pix0 + f.W;

    f2 T = {in0 ? final_T[pix0] : 0.0f, in1 ? final_T[pix1] : 0.0f};
    const uint32_t last0 = in0 ? n_contrib[pix0] : 0u, last1 = in1 ? n_contrib[pix1] : 0u;
    f2 m[kLiftChannels];                                              // the lane's weights; zero past `channels` and off the image
    const size_t plane = (size_t)f.W * f.H;
#pragma unroll
    for (int c = 0; c < kLiftChannels; ++c) {
        m[c] = f2{0.f, 0.f};
        if (c < channels) {
            if (in0) m[c].x = weights[c * plane + pix0];
            if (in1) m[c].y = weights[c * plane + pix1];
        }
    }
    uint32_t wave_last = max(last0, last1);
    for (int o = 32; o > 0; o >>= 1) wave_last = max(wave_last, (uint32_t)__shfl_xor((int)wave_last, o));
    if (lane == 0) s_blast[wave] = wave_last;
    __syncthreads();
    const int total = (int)max(s_blast[0], s_blast[1]);
    const int rounds = (total + kB2 - 1) / kB2;
    const int moment = wave_sum9_moment(lane);
    const bool owner = wave_sum9_owner(lane) && moment <= channels;

    uint32_t n_id = 0;
    float2 n_xy = make_float2(0.f, 0.f);
    float4 n_co = make_float4(0.f, 0.f, 0.f, 0.f);
    auto fetch = [&](int r) {
        const int hi_ = total - r * kB2;
        if (tid < hi_) {                                        // staged slot tid <-> list position hi_-1-tid
            n_id = point_list[r0 + (uint32_t)(hi_ - 1 - tid)];
            n_xy = xy[n_id]; n_co = conic_opacity[n_id];
        }
    };
    if (rounds > 0) fetch(0);
    for (int r = 0; r < rounds; ++r) {
        const int hi = total - r * kB2;
        const int n = hi < kB2 ? hi : kB2;
        __syncthreads();
        s_ent[0][tid] = make_float4(n_xy.x, n_xy.y, active_t2(n_co), __uint_as_float(n_id));
        s_ent[1][tid] = n_co;
#pragma unroll
        for (int c = 0; c < 9; ++c) s_acc[tid][c] = 0.0f;
        __syncthreads();
        if (r + 1 < rounds) fetch(r + 1);
        for (int c = 0; c < n; c += 64) {
            const int e = c + lane;                              // < kB2: n <= kB2 and c is a multiple of 64
            const float4 ce = s_ent[0][e];
            const bool keep = e < n && (uint32_t)(hi - 1 - e) < wave_last &&
                              quad_overlap(make_float2(ce.x, ce.y), s_ent[1][e], ce.z, (float)hx0, (float)hy0, 15.0f, 7.0f);
            unsigned long long mask = ballot64(keep);
            while (mask != 0ull) {
                const int jc = c + __builtin_ctzll(mask);           // wave-uniform, < n
                mask &= mask - 1;
                const float4 p = s_ent[0][jc], co = s_ent[1][jc];
                const uint32_t pos = (uint32_t)(hi - 1 - jc);
                const float dx = p.x - pfx;
                const f2 dy = splat(p.y) - pfy;
                const f2 power = gauss_power(co, dx, dy);          // the forward's rounding recipe
                const f2 G = {__expf(power.x), __expf(power.y)};
                const f2 oG = co.w * G;
                const bool act0 = pos < last0 && power.x <= 0.0f && oG.x >= kAlphaMin;
                const bool act1 = pos < last1 && power.y <= 0.0f && oG.y >= kAlphaMin;
                const f2 gm = {act0 ? oG.x : 0.0f, act1 ? oG.y : 0.0f};                // o G of the ACTIVE pixels, else 0
                const f2 am = __builtin_elementwise_min(splat(kAlphaMax), gm);         // alpha of the active pixels, else 0
                const unsigned long long any_active = ballot64((__float_as_uint(gm.x) | __float_as_uint(gm.y)) != 0u);
                const f2 om = splat(1.0f) - am;                      // in [0.01, 1]; exactly 1 for an inactive pixel
                const f2 inv = {__builtin_amdgcn_rcpf(om.x), __builtin_amdgcn_rcpf(om.y)};
                T = T * inv;                                         // T in front of the entry (unchanged for an inactive pixel)
                if (any_active != 0ull) {                       // wave-uniform
                    const f2 w = am * T;                             // the blend weight; 0 for an inactive pixel
                    float h[kLiftChannels];
#pragma unroll
                    for (int k = 0; k < kLiftChannels; ++k) h[k] = __builtin_fmaf(w.y, m[k].y, w.x * m[k].x);
                    const float sum = wave_sum9(w.x + w.y, h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]);
                    // both waves add into the same rows; nobody waits for it
                    if (owner) __hip_atomic_fetch_add(&s_acc[jc][moment], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        __syncthreads();
        // flush: 16 lanes per entry; an entry whose sums are all zero was evaluated by neither half tile (or added nothing) and
        // is skipped, so a Gaussian the view does not composite keeps its row bit for bit
        {
            const int comp = lane & 15;                                    // slot of the row
#pragma unroll 4
            for (int it = 0; it < 16; ++it) {
                const int e = wave * 64 + it * 4 + (lane >> 4);            // < kB2
                if (e >= n) continue;
                const float* a = s_acc[e];
                const bool any = (((__float_as_uint(a[0]) | __float_as_uint(a[1]) | __float_as_uint(a[2])) |
                                   (__float_as_uint(a[3]) | __float_as_uint(a[4]) | __float_as_uint(a[5])) |
                                   (__float_as_uint(a[6]) | __float_as_uint(a[7]) | __float_as_uint(a[8]))) &
                                  0x7FFFFFFFu) != 0u;
                if (!any || comp > channels) continue;
                const uint32_t id = __float_as_uint(s_ent[0][e].w);
                atomicAdd(&acc[(size_t)id * (size_t)acc_stride + comp], a[comp]);
            }
        }
    }
}

int launch_lift_weights(const Frame& f, GeomView g, BinningView b, ImageView im, int64_t D, const float* weights, int channels,
                        float* acc, int acc_stride, hipStream_t st) {
    if (f.W <= 0 || f.H <= 0 || D <= 0 || f.P <= 0) return 0;             // nothing composited
    const uint32_t* plist = b.vals[b.passes & 1];
    hipLaunchKernelGGL(lift_weights_kernel, dim3(f.gx * f.gy), dim3(kB2), 0, st, f, im.ranges, plist, g.xy, g.conic_opacity,
                       im.final_T, im.n_contrib, weights, channels, acc, acc_stride);
    return hipGetLastError() == hipSuccess ? 0 : MVI_EHIP;
}

}  // namespace mvi
