// Backward of the rasterizer's two auxiliary per-pixel outputs, for gfx950:
//     expected_depth = sum_i z_i alpha_i T_i        alpha = 1 - T_final
// (the forward is the AUX instantiation of render_forward_kernel, raster_render.hip: one fma per composited entry).
//
// Both outputs are alpha-composited channels with background 0 — "colours" (z_i, 1) — so the replay is the colour backward's
// with two channels and no background term. Per pixel, back to front over the entries [0, n_contrib) from final_T, with
// gD, gA the upstream gradients and c_i = gD z_i + gA:
//     dL/dz_i     = alpha_i T_i gD
//     dL/dalpha_i = T_i (c_i - A_i),   A_i = (sum_{j > i} c_j alpha_j T_j) / T_{i+1}   (A <- alpha c + (1 - alpha) A)
// and dL/dalpha goes through the same six raw moments (W, W dx, W dy, W dx^2, W dx dy, W dy^2; W = o G dL/dalpha, the
// min(0.99, o G) clamp straight-through) into mean2D, conic and opacity as in render_backward_kernel. The kernel ADDS its share
// into the accumulation rows grad_rows [P][16] that the colour backward adds into, before the per-Gaussian chain rule reads
// them (the conversion from raw moments is linear in dL/dalpha, so the two shares just sum), and dL/dz into slot 9:
//   0 mean2D.x  1 mean2D.y  2 conic A  3 conic B  4 conic C  5 opacity  6 r  7 g  8 b  9 dL/dz (view depth)  10..15 unused
// It also sets touched[id]: a Gaussian can receive a depth gradient where its colour gradient is zero, and the
// support-compacted chain rule must see it. depth_to_means_kernel then takes slot 9 to the positions: z = [m, 1] . V[:, 2].
//
// Shape: render_backward_kernel's. One block of 128 threads = 2 wave64 per tile, a wave covers a 16 x 8 half tile with two
// vertically adjacent pixels per lane; the tile's list is staged through LDS back to front, 128 entries per round, culled
// per wave with the exact box test; per evaluated entry the lane's two pixels are added, wave_sum9 sums over the wave in
// registers (seven moments, two zero arguments), seven lanes add the wave totals into the block's per-entry LDS
// accumulator; once per staged batch one lane per entry converts the raw sums and 16 lanes per entry flush the row with
// float atomics (one 64-byte request per Gaussian). Decisions (alpha, active) use the forward's rounding recipe, gauss_power.
#include "raster_common.h"
#include "raster_render_shared.h"

namespace mvi {

constexpr int kAuxMoments = 7;          // W, W dx, W dy, W dx^2, W dx dy, W dy^2, alpha T gD
constexpr int kRowDepthSlot = 9;        // grad_rows[id][9] = dL/dz

__global__ __launch_bounds__(kB2) void render_backward_aux_kernel(
    Frame f, const uint32_t* __restrict__ ranges, const uint32_t* __restrict__ point_list,
    const float2* __restrict__ xy, const float4* __restrict__ rgbd, const float4* __restrict__ conic_opacity,
    const float* __restrict__ final_T, const uint32_t* __restrict__ n_contrib,
    const float* __restrict__ dL_ddepth, const float* __restrict__ dL_dalpha_img, float* __restrict__ grad_rows,
    uint8_t* __restrict__ touched) {
#pragma clang fp contract(off)
    // a staged entry is one record: [0] (x, y, t2, Gaussian id), [1] conic + opacity, [2] colour + depth (only .w is used)
    __shared__ float4 s_ent[3][kB2];
    __shared__ float s_acc[kB2][9];                                   // raw moment sums per staged entry (wave_sum9's stride)
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
    f2 gD = {0.f, 0.f}, gA = {0.f, 0.f};
    if (dL_ddepth) { if (in0) gD.x = dL_ddepth[pix0]; if (in1) gD.y = dL_ddepth[pix1]; }
    if (dL_dalpha_img) { if (in0) gA.x = dL_dalpha_img[pix0]; if (in1) gA.y = dL_dalpha_img[pix1]; }
    f2 A_dot = {0.f, 0.f};             // (sum over the entries behind of c alpha T) / T in front of them; no background term
    uint32_t wave_last = max(last0, last1);
    for (int o = 32; o > 0; o >>= 1) wave_last = max(wave_last, (uint32_t)__shfl_xor((int)wave_last, o));
    if (lane == 0) s_blast[wave] = wave_last;
    __syncthreads();
    const int total = (int)max(s_blast[0], s_blast[1]);
    const int rounds = (total + kB2 - 1) / kB2;
    const bool owner = wave_sum9_owner(lane) && wave_sum9_moment(lane) < kAuxMoments;
    const int moment = wave_sum9_moment(lane);

    uint32_t n_id = 0;
    float2 n_xy = make_float2(0.f, 0.f);
    float4 n_co = make_float4(0.f, 0.f, 0.f, 0.f), n_cd = n_co;
    auto fetch = [&](int r) {
        const int hi_ = total - r * kB2;
        if (tid < hi_) {                                        // staged slot tid <-> list position hi_-1-tid
            n_id = point_list[r0 + (uint32_t)(hi_ - 1 - tid)];
            n_xy = xy[n_id]; n_co = conic_opacity[n_id]; n_cd = rgbd[n_id];
        }
    };
    if (rounds > 0) fetch(0);
    for (int r = 0; r < rounds; ++r) {
        const int hi = total - r * kB2;
        const int n = hi < kB2 ? hi : kB2;
        __syncthreads();
        s_ent[0][tid] = make_float4(n_xy.x, n_xy.y, active_t2(n_co), __uint_as_float(n_id));
        s_ent[1][tid] = n_co;
        s_ent[2][tid] = n_cd;
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
                const float z = s_ent[2][jc].w;
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
                const f2 Tn = T * inv;                               // T in front of the entry (= T for an inactive pixel)
                const f2 c_dot = pk_fma(splat(z), gD, gA);
                const f2 dL_dalpha = (c_dot - A_dot) * Tn;
                const f2 dch = am * Tn, mw = gm * dL_dalpha;
                T = Tn;
                A_dot = pk_fma(am, c_dot, om * A_dot);
                if (any_active != 0ull) {                       // wave-uniform
                    const float wy0 = mw.x * dy.x, wy1 = mw.y * dy.y;
                    const float m_w = mw.x + mw.y;                                         // W
                    const float m_x = m_w * dx;                                            // W dx
                    const float m_y = wy0 + wy1;                                           // W dy
                    const float m_xx = m_x * dx;                                           // W dx^2
                    const float m_xy = m_y * dx;                                           // W dx dy
                    const float m_yy = __builtin_fmaf(wy1, dy.y, wy0 * dy.x);              // W dy^2
                    const float m_z = __builtin_fmaf(dch.y, gD.y, dch.x * gD.x);           // alpha T gD
                    const float sum = wave_sum9(m_w, m_x, m_y, m_xx, m_xy, m_yy, m_z, 0.0f, 0.0f);
                    // both waves add into the same rows; nobody waits for it
                    if (owner) __hip_atomic_fetch_add(&s_acc[jc][moment], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        __syncthreads();
        // flush: (1) one thread per entry turns the raw sums into gradients in place (the conversion render_backward_kernel
        // applies to slots 0..5; the depth sum is final as it stands) and marks entries nobody evaluated; (2) 16 lanes per
        // entry add the row with float atomics, one 64-byte request per Gaussian.
        if (tid < n) {
            float* a = s_acc[tid];
            const float a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6];
            const bool any = (((__float_as_uint(a0) | __float_as_uint(a1) | __float_as_uint(a2)) |
                               (__float_as_uint(a3) | __float_as_uint(a4) | __float_as_uint(a5)) | __float_as_uint(a6)) &
                              0x7FFFFFFFu) != 0u;
            if (any) {
                const float4 co = s_ent[1][tid];
                a[0] = -0.5f * (float)f.W * (co.x * a1 + co.y * a2);       // dL/dmean2D.x (NDC-scaled)
                a[1] = -0.5f * (float)f.H * (co.z * a2 + co.y * a1);       // dL/dmean2D.y
                a[2] = -0.5f * a3;                                         // dL/dA
                a[3] = -a4;                                                // dL/dB
                a[4] = -0.5f * a5;                                         // dL/dC
                a[5] = a0 / co.w;                                          // dL/dopacity = sum G dL/dalpha
            } else {
                s_ent[0][tid].w = __uint_as_float(0xFFFFFFFFu);            // never evaluated by either half tile
            }
        }
        __syncthreads();
        {
            const int comp = lane & 15;                                    // slot of the row
            const int src = comp < 6 ? comp : 6;                           // its place in the accumulator (slot 9 <- sum 6)
            const bool mine = comp < 6 || comp == kRowDepthSlot;
#pragma unroll 4
            for (int it = 0; it < 16; ++it) {
                const int e = wave * 64 + it * 4 + (lane >> 4);            // < kB2
                const uint32_t id = e < n ? __float_as_uint(s_ent[0][e].w) : 0xFFFFFFFFu;
                if (id == 0xFFFFFFFFu || !mine) continue;
                atomicAdd(&grad_rows[(size_t)id * kRow + comp], s_acc[e][src]);
                if (comp == 0) touched[id] = 1;                // gradient support (idempotent store)
            }
        }
    }
}

int launch_render_backward_aux(const Frame& f, GeomView g, BinningView b, ImageView im, int64_t D, const float* dL_dexpected_depth,
                               const float* dL_dalpha, float* grad_rows, hipStream_t st) {
    if ((!dL_dexpected_depth && !dL_dalpha) || f.W <= 0 || f.H <= 0 || D <= 0 || f.P <= 0) return 0;   // nothing to add
    const uint32_t* plist = b.vals[b.passes & 1];
    hipLaunchKernelGGL(render_backward_aux_kernel, dim3(f.gx * f.gy), dim3(kB2), 0, st, f, im.ranges, plist, g.xy, g.rgbd,
                       g.conic_opacity, im.final_T, im.n_contrib, dL_dexpected_depth, dL_dalpha, grad_rows, g.touched);
    return hipGetLastError() == hipSuccess ? 0 : MVI_EHIP;
}

// dL/dmeans3D[i] += grad_rows[i][9] * V[0:3, 2]: the view depth is z = m . V[0:3, 2] + V[3, 2] (row-vector convention, V in
// Camera.world_view_transform memory order). One thread per Gaussian; rows without a depth gradient are left alone.
__global__ __launch_bounds__(256) void depth_to_means_kernel(int P, const float* __restrict__ view,
                                                              const float* __restrict__ grad_rows,
                                                              float* __restrict__ dL_dmeans3D) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const float gz = grad_rows[(size_t)i * kRow + kRowDepthSlot];
    if (gz == 0.0f) return;
    float* o = dL_dmeans3D + 3 * (size_t)i;
    o[0] = __builtin_fmaf(gz, view[2], o[0]);
    o[1] = __builtin_fmaf(gz, view[6], o[1]);
    o[2] = __builtin_fmaf(gz, view[10], o[2]);
}

int launch_depth_to_means(const Frame& f, const float* grad_rows, float* dL_dmeans3D, hipStream_t st) {
    if (f.P <= 0) return 0;
    hipLaunchKernelGGL(depth_to_means_kernel, dim3((f.P + 255) / 256), dim3(256), 0, st, f.P, f.view, grad_rows, dL_dmeans3D);
    return hipGetLastError() == hipSuccess ? 0 : MVI_EHIP;
}

}  // namespace mvi
