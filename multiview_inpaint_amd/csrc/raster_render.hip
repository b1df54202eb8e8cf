// Per-tile alpha compositing with median depth, forward and backward, for gfx950.
// Replaces the plug-in's render stages behind gs-simp/gaussian_renderer/__init__.py:85-93
// (forward: colour [3,H,W] + depth [1,H,W]) and loss.backward() (gs-simp/train.py:93).
//
// One block per 16x16-pixel tile. Forward: 256 threads = 4 wave64, each wave an 8x8-pixel quadrant, one pixel per
// lane. Backward: 128 threads = 2 wave64, each wave a 16x8 half tile, two pixels per lane on packed fp32 math.
// The tile's depth-sorted list is staged through LDS one entry per thread and round by the whole block. Each wave
// then tests 64 staged entries at a time against its own pixel box (one lane per entry): an entry is kept iff its
// "active ellipse" {alpha >= 1/255} = {d^T conic d <= 2 ln(255 o)} can reach the box (exact minimum of the
// quadratic form over the box, quad_overlap). Only kept entries are evaluated per pixel. The test is conservative
// (margin on 2 ln(255 o)), so results are identical to evaluating every entry.
#include <cstdlib>
#include <mutex>

#include "raster_common.h"
#include "raster_render_shared.h"

namespace mvi {

// (ballot64, active_t2, quad_overlap, xcd_band_tile, gauss_power / gauss_power1 and wave_sum9 live in raster_render_shared.h:
// raster_render_aux.hip replays the same decisions with them)

// The CU's scalar unit issues one instruction per cycle for all four SIMDs, so the inner loop must
// stay light on scalar work: the kept entries of a 64-entry chunk are compacted into a per-wave LDS
// strip (lane-parallel copies at popcount positions) and walked by a plain counted loop, and a
// pixel that has saturated is represented by T = 0 (its committed transmittance lives in T_out), so
// the body needs no per-lane "done" mask and no divergent branch.
//
// The strip is walked in groups of G kept entries (G = 1: one entry per iteration, the next entry's address clamped and
// rebuilt every time, the wave's pixels tested at the top of a chunk only). One address register per group and
// compile-time offsets for its 3 G reads, one loop test per group, and in front of every group the wave asks whether any
// of its pixels is still live (T > 0): if none is, nothing behind this point changes any output (test_T = 0: no
// contribution, T stays 0), and the wave leaves the round's chunk loop. The cnt % G entries behind the last full group
// are walked one by one: no padding entry is ever evaluated.
// AUX: the kernel also accumulates the expected depth sum z alpha T over exactly the entries it composites (one fma per entry
// beside the colour's) and writes it and alpha = 1 - T_final; with AUX clear the two pointers are never read and the
// instantiation is the colour-only kernel.
// LAZY (binning version 2 under mvi_raster_list_expansion(1)): nobody has written the tile's list. The block finds a round's
// entries itself, by walking the segments of its tile column (lazy_list_step, raster_render_shared.h), just in time: at the
// top of the round, behind the saturation test, so that no segment is looked at for a round that is never composited. The
// thread that stages an entry takes the Gaussian from the segment and stores it to point_list[r0 + position] (coalesced):
// the prefix of the list that this kernel consumed — all that the backward, the aux backward, the splat and the lift replay —
// lies where pass 2 would have put it, with the same values. What the eager kernel gathers one round ahead is gathered here
// at the top of its own round: the other five blocks of the CU cover the wait, and eleven registers are free while a round
// is composited. With LAZY clear the instantiation is the eager kernel.
struct LazyLists {
    const uint16_t* seg_yh;             // pass 1: first row | rows - 1 << 8 of every column segment
    const uint32_t* seg_idx;            // pass 1: its Gaussian
    const uint32_t* col_start;          // [gx + 1] first segment of every tile column
};
template <int G, bool AUX, bool LAZY>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(G == 1 ? 1 : 6, G == 1 ? 8 : 6))) void render_forward_kernel(
    Frame f, const uint32_t* __restrict__ ranges, uint32_t* __restrict__ point_list,
    const float2* __restrict__ xy, float4* rgbd, const float4* __restrict__ conic_opacity,
    float* __restrict__ final_T, uint32_t* __restrict__ n_contrib, float* __restrict__ out_color,
    float* __restrict__ out_depth, ZeroRegions zero, const ColorSource* __restrict__ color_src, uint8_t* clamped,
    float* __restrict__ out_expected_depth, float* __restrict__ out_alpha, uint32_t* __restrict__ class_count, LazyLists lz) {
    __shared__ uint32_t s_wmax[4];
    __shared__ uint32_t s_q[LAZY ? kBlock : 1];                // segments of the round's entries, by position in the round
    __shared__ uint32_t s_tot[LAZY ? 2 : 1][kLazySubs * 4];
    __shared__ float2 s_xy[kBlock];
    __shared__ float s_t2[kBlock];
    __shared__ float4 s_co[kBlock];
    __shared__ float4 s_cd[kBlock];                 // r, g, b, depth
    // per-wave compacted strip: [0] (x, y, list position, -), [1] conic + opacity, [2] colour + depth — ONE array, so that the
    // three reads of an entry share one address register (constant offsets) instead of costing an address add each
    __shared__ float4 w_s[4][3][64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // the backward's accumulation rows (and the touched flags) are zeroed HERE: this kernel is issue-bound with the memory
    // pipes nearly idle, so the 65 bytes per Gaussian ride along for free instead of costing a 96 MB fill pass in front of
    // the render backward
    zero_share(zero, tid, kBlock);
    const int tile = xcd_band_tile(blockIdx.x, f.gx * f.gy);
    const int tile_y = tile / f.gx, tile_x = tile - tile_y * f.gx;
    const int qx0 = tile_x * kTile + 8 * (wave & 1), qy0 = tile_y * kTile + 8 * (wave >> 1);
    const int pxi = qx0 + (lane & 7), pyi = qy0 + (lane >> 3);
    const bool inside = pxi < f.W && pyi < f.H;
    const float pfx = (float)pxi, pfy = (float)pyi;
    const uint32_t r0 = ranges[2 * tile], r1 = ranges[2 * tile + 1];
    int todo = (int)(r1 - r0);
    const int rounds = (todo + kBlock - 1) / kBlock;

    float T = inside ? 1.0f : 0.0f;                 // 0 = this pixel takes no further contributions
    float T_out = 1.0f, C2 = 0.f, Dp = kDepthSentinel, Tc = 1.0f;
    [[maybe_unused]] float Dexp = 0.f;              // AUX: sum of depth * alpha * T
    f2 C01 = {0.f, 0.f};                            // red, green: one packed fma on the (aligned) first two registers of the colour
    uint32_t last = 0;

    // Deferred SH colours (raster_common.h, ColorSource): rgbd holds (-1, -1, -1, depth) until somebody needs the colour.
    // The lane that stages an entry evaluates it (the same arithmetic as the eager preprocess), writes it back for the other
    // tiles and for the backward, and stages its OWN value: whatever another block wrote meanwhile is either complete
    // (every channel >= 0) or treated as pending.
    const ColorSource cs = *color_src;              // uniform: scalar loads
    // software pipeline: the gathers of batch r+1 are issued before batch r is composited
    float2 n_xy = make_float2(0.f, 0.f);
    float4 n_co = make_float4(0.f, 0.f, 0.f, 0.f), n_cd = n_co;
    uint32_t n_id = 0;
    // LAZY: the walk of the tile column (block-uniform)
    [[maybe_unused]] uint32_t c0 = 0, c1 = 0, cur = 0, have = 0;
    if constexpr (LAZY)
        if (rounds > 0) { c0 = lz.col_start[tile_x]; c1 = lz.col_start[tile_x + 1]; cur = c0 & ~1u; }
    auto fetch = [&](int r) {
        if constexpr (LAZY) {
            const uint32_t lo = (uint32_t)(r * kBlock), hi = min(lo + (uint32_t)kBlock, r1 - r0);
            uint32_t reached = have;
            int par = 0;
            while (cur < c1) {
                reached = lazy_list_step(lz.seg_yh, c0, c1, (uint32_t)tile_y, cur, have, lo, hi, s_tot, par, tid,
                                         [&](uint32_t pos, uint32_t seg) { s_q[pos - lo] = seg; });
                if (reached >= hi) break;
            }
            __syncthreads();
            // the ranges hold the column's count for this row, so the round is complete; a state that says otherwise stages
            // opacity 0 (never kept) for what is missing and reads nothing
            const uint32_t avail = reached > lo ? min(reached, hi) - lo : 0u;
            n_co = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((uint32_t)tid < avail) {
                n_id = lz.seg_idx[s_q[tid]];
                point_list[r0 + lo + (uint32_t)tid] = n_id;
                n_xy = xy[n_id]; n_co = conic_opacity[n_id]; n_cd = rgbd[n_id];
            }
        } else {
            const uint32_t q = r0 + (uint32_t)(r * kBlock + tid);
            if (q < r1) {
                n_id = point_list[q];
                n_xy = xy[n_id]; n_co = conic_opacity[n_id]; n_cd = rgbd[n_id];
            }
        }
    };
    if (!LAZY && rounds > 0) fetch(0);
    for (int r = 0; r < rounds; ++r, todo -= kBlock) {
        if (__syncthreads_count(T <= 0.0f) == kBlock) break;
        if constexpr (LAZY) fetch(r);
        if (cs.deferred && tid < todo && color_pending(n_cd)) n_cd = resolve_color_small(cs, f.campos, n_id, n_cd.w, rgbd, clamped);
        s_xy[tid] = n_xy;
        s_co[tid] = n_co;
        s_t2[tid] = active_t2(n_co);
        s_cd[tid] = n_cd;
        __syncthreads();
        if (!LAZY && r + 1 < rounds) fetch(r + 1);
        const int n = todo < kBlock ? todo : kBlock;
        for (int c = 0; c < n; c += 64) {
            if (ballot64(T > 0.0f) == 0ull) break;
            const int e = c + lane;
            const bool keep = e < n && quad_overlap(s_xy[e], s_co[e], s_t2[e], (float)qx0, (float)qy0);
            const unsigned long long mask = ballot64(keep);
            if (mask == 0ull) continue;
            if (keep) {
                const int pos = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                const float2 q = s_xy[e];
                w_s[wave][0][pos] = make_float4(q.x, q.y, __uint_as_float((uint32_t)(r * kBlock + e + 1)), 0.f);
                w_s[wave][1][pos] = s_co[e];
                w_s[wave][2][pos] = s_cd[e];
            }
            // one kept entry (strip position, conic + opacity, colour + depth) composited onto the lane's pixel
            auto entry = [&](const float4 a, const float4 co, const float4 cd, const float chain) __attribute__((always_inline)) {
                float dx = a.x - pfx, dy = a.y - pfy;
                // No instruction: dx and dy are made to come after the previous entry's exponent (`chain`). The entries of a
                // group are independent up to alpha, and the compiler otherwise pairs their dx / dy / power arithmetic on
                // packed fp32, with register copies to build the pairs (86 VGPRs: five waves); a packed instruction issues
                // at the price of 1.8 plain ones on a busy SIMD.
                if constexpr (G > 1) asm("" : "+v"(dx), "+v"(dy) : "v"(chain));
                float power = gauss_power1(co, dx, dy);
                float alpha = fminf(kAlphaMax, co.w * __expf(power));
                alpha = power <= 0.0f ? alpha : 0.0f;
                const float test_T = T * (1.0f - alpha);                 // 0 for a saturated pixel
                const bool valid = alpha >= kAlphaMin;
                const bool contrib = valid && test_T >= kTEps;
                const float w = contrib ? alpha * T : 0.0f;
                C01 = pk_fma(f2{cd.x, cd.y}, splat(w), C01);
                C2 = __builtin_fmaf(cd.z, w, C2);
                if constexpr (AUX) Dexp = __builtin_fmaf(cd.w, w, Dexp);
                // median depth of the w-depth fork = depth of the entry that takes T from above 0.5 to below it (T > 0.5 and
                // T (1 - alpha) < 0.5, both strict: oracle/raster_oracle.c orc_render_forward). Every contributing entry met
                // while T > 0.5 overwrites the candidate and the T it leaves behind (two selects on one condition): the last
                // of them is the crossing entry iff it left T below 0.5 — checked once, after the loop. An entry that leaves
                // T at exactly 0.5 is not a crossing, and nothing behind it starts from above 0.5: the sentinel stays.
                const bool above = contrib && T > 0.5f;
                Dp = above ? cd.w : Dp;
                Tc = above ? test_T : Tc;
                T_out = contrib ? test_T : T_out;
                last = contrib ? __float_as_uint(a.z) : last;           // 1-based position in the tile's list
                T = contrib ? test_T : (valid ? 0.0f : T);              // valid but below 1e-4: saturated from here on
                return power;
            };
            const int cnt = __popcll(mask);
            if constexpr (G == 1) {
                float4 a = w_s[wave][0][0], co = w_s[wave][1][0], cd = w_s[wave][2][0];
                for (int k = 0; k < cnt; ++k) {
                    const int kn = k + 1 < 64 ? k + 1 : 63;
                    const float4* nx = &w_s[wave][0][kn];
                    const float4 an = nx[0], con = nx[64], cdn = nx[128];   // next entry's reads overlap the math
                    entry(a, co, cd, 0.0f);
                    a = an; co = con; cd = cdn;
                }
            } else {
                // Rotated by hand: every exit of the group loop is at its bottom, behind the group, so the eight carried
                // registers of a pixel leave in the registers they live in. (With the test at the top and a jump out of the
                // chunk loop the compiler kept two copies of them and paid seven v_mov per group.) The chunk-top test above
                // is the first group's test, asked before the cull; the test in front of the remainder also catches a wave
                // that left the group loop saturated with full groups still to go.
                const float4* g = &w_s[wave][0][0];
                int k = 0;
                float chain = 0.0f;
                if (cnt >= G) {
                    do {
                        // The reads of entry j + 1 are issued in front of the arithmetic of entry j, and the scheduling barrier
                        // keeps them there: left alone the compiler issues an entry's conic and colour reads right in front
                        // of their first use and waits for each (207 against 216 us for the kernel).
                        float4 a = g[0], co = g[64], cd = g[128];
#pragma unroll
                        for (int j = 0; j < G; ++j) {
                            const int jn = j + 1 < G ? j + 1 : j;
                            const float4 an = g[jn], con = g[64 + jn], cdn = g[128 + jn];
                            __builtin_amdgcn_sched_barrier(0);
                            chain = entry(a, co, cd, chain);
                            a = an; co = con; cd = cdn;
                        }
                        k += G; g += G;
                    } while ((k + G <= cnt) & (ballot64(T > 0.0f) != 0ull));   // both asked every time: one block, no inner branch
                }
                if (k < cnt && ballot64(T > 0.0f) != 0ull)
                    for (; k < cnt; ++k, ++g) chain = entry(g[0], g[64], g[128], chain);
            }
        }
    }
    // The tile's work class for the backward's dispatch order: the backward replays the list up to the largest n_contrib of
    // the tile, which only this kernel knows. One lane appends the tile to the queue of its class in its XCD band (the band
    // of xcd_band_tile is blockIdx.x & 7, here and in the backward); the counts start at zero (ranges_and_counts_bytes).
    // A pixel outside the image has last = 0. The barrier and the counter's atomic come BEFORE the image stores, the queue
    // store behind them: the barrier then has no stores to drain, and the atomic's round trip runs beside the stores' own.
    const uint32_t wmax = wave_umax(last);          // wave-uniform, on the scalar side
    if (lane == 0) s_wmax[wave] = wmax;
    __syncthreads();
    uint32_t cls = 0, slot = 0;
    if (tid == 0) {
        const uint32_t m = max(max(s_wmax[0], s_wmax[1]), max(s_wmax[2], s_wmax[3]));
        cls = (blockIdx.x & (kTileBands - 1)) * kTileClasses + min((uint32_t)(kTileClasses - 1), m / kTileClassWidth);
        slot = atomicAdd(&class_count[cls], 1u);
    }
    if (inside) {
        size_t pix = (size_t)pyi * f.W + pxi, hw = (size_t)f.H * f.W;
        final_T[pix] = T_out;
        n_contrib[pix] = last;
        out_color[pix] = C01.x + T_out * f.bg[0];
        out_color[hw + pix] = C01.y + T_out * f.bg[1];
        out_color[2 * hw + pix] = C2 + T_out * f.bg[2];
        out_depth[pix] = Tc < 0.5f ? Dp : kDepthSentinel;             // never crossed 0.5: the sentinel (gs-simp/gen_seq.py:50)
        if constexpr (AUX) {
            out_expected_depth[pix] = Dexp;
            out_alpha[pix] = 1.0f - T_out;
        }
    }
    if (tid == 0) {
        const uint32_t stride = (uint32_t)tile_queue_stride(f.gx * f.gy);
        if (slot < stride) tile_class_queues(class_count)[(size_t)cls * stride + slot] = (uint32_t)tile;   // always, from zeroed counts
    }
}

// Deferred SH colours, ahead of the render kernel: the leading `n_front` entries of every tile's list are entries the render
// kernel is going to stage for certain (its first round), and neighbouring tiles share most of them (2.1 M leading entries of
// the bench view are 45 k distinct Gaussians): left to the render kernel, every one of those tiles finds the colour pending at
// the same moment and evaluates it itself (measured: +140 us). Two small kernels instead: mark_front sets a byte per Gaussian
// named by a leading entry (plain idempotent stores: no atomics, no reads), resolve_marked walks the P flags, collects the
// marked Gaussians of 1024 in LDS and evaluates them with full waves. (Claiming with a device-scope compare-and-swap in one
// kernel was measured at 53 us: ~2 M memory-side atomics, the claims invisible through the other XCDs' L2.) What the render
// kernel meets later is either a colour or, beyond the leading entries, the rare Gaussian nobody needed yet.
constexpr int kFrontTiles = 4;
constexpr int kFrontMax = 1024;
__global__ __launch_bounds__(kBlock) void mark_front_kernel(int tiles, const uint32_t* __restrict__ ranges,
                                                            const uint32_t* __restrict__ point_list, uint8_t* __restrict__ front,
                                                            int n_front, const ColorSource* __restrict__ color_src, int gx,
                                                            int every) {
    if (!color_src->deferred) return;                    // precomputed colours: nothing is pending (the host does not know)
    const int tid = threadIdx.x;
    // every == 2: only the tiles of even column AND even row name Gaussians (a Gaussian in the leading entries of a tile
    // covers ~46 tiles of the bench view: it leads a sampled one too; whoever is missed is evaluated by the render kernel)
    const int sx = (gx + every - 1) / every;
#pragma unroll
    for (int t = 0; t < kFrontTiles; ++t) {
        const int j = blockIdx.x * kFrontTiles + t;
        const int tile = every == 1 ? j : (j / sx) * every * gx + (j % sx) * every;
        if (tile >= tiles) break;
        const uint32_t r0 = ranges[2 * tile], r1 = ranges[2 * tile + 1];
        const uint32_t n = min(r1 - r0, (uint32_t)n_front);
        for (uint32_t e = tid; e < n; e += kBlock) front[point_list[r0 + e]] = 1;
    }
}
// The same marks with no list to read (lists expanded on demand): the leading entries of a sampled tile are the first
// min(n_front, length) segments of its column that cover its row, found by the walk the render kernel uses. Nothing is stored
// but the marks.
__global__ __launch_bounds__(kBlock) void mark_front_lazy_kernel(int tiles, const uint32_t* __restrict__ ranges, LazyLists lz,
                                                                 uint8_t* __restrict__ front, int n_front,
                                                                 const ColorSource* __restrict__ color_src, int gx, int every) {
    if (!color_src->deferred) return;
    __shared__ uint32_t s_tot[2][kLazySubs * 4];
    const int tid = threadIdx.x;
    const int sx = (gx + every - 1) / every;
    int par = 0;                                         // carried from tile to tile: see lazy_list_step
    for (int t = 0; t < kFrontTiles; ++t) {
        const int j = blockIdx.x * kFrontTiles + t;
        const int tile = every == 1 ? j : (j / sx) * every * gx + (j % sx) * every;
        if (tile >= tiles) break;
        const uint32_t r0 = ranges[2 * tile], r1 = ranges[2 * tile + 1];
        const uint32_t n = min(r1 - r0, (uint32_t)n_front);
        if (n == 0) continue;                            // block-uniform; an empty column is never walked
        const int tile_y = tile / gx, tile_x = tile - tile_y * gx;
        const uint32_t c0 = lz.col_start[tile_x], c1 = lz.col_start[tile_x + 1];
        uint32_t cur = c0 & ~1u, have = 0;
        while (cur < c1) {
            const uint32_t reached = lazy_list_step(lz.seg_yh, c0, c1, (uint32_t)tile_y, cur, have, 0u, n, s_tot, par, tid,
                                                    [&](uint32_t, uint32_t seg) { front[lz.seg_idx[seg]] = 1; });
            if (reached >= n) break;
        }
    }
}
constexpr int kMarkedPer = 4;                            // flags per thread: one 4-byte load
__global__ __launch_bounds__(kBlock) void resolve_marked_kernel(Frame f, GeomView g) {
    const ColorSource cs = *g.color_src;
    if (!cs.deferred) return;                            // precomputed colours (or an eager forward): the flags were never zeroed
    __shared__ uint32_t s_id[kBlock * kMarkedPer];
    __shared__ uint32_t s_n;
    const int tid = threadIdx.x;
    if (tid == 0) s_n = 0;
    __syncthreads();
    const int i0 = (blockIdx.x * kBlock + tid) * kMarkedPer;
    if (i0 < f.P) {                                      // the 4-byte load may reach into the segment's padding: bytes >= P are ignored
        const uint32_t w = *reinterpret_cast<const uint32_t*>(g.front + i0);
#pragma unroll
        for (int k = 0; k < kMarkedPer; ++k)
            if (((w >> (8 * k)) & 0xFFu) && i0 + k < f.P) s_id[atomicAdd(&s_n, 1u)] = (uint32_t)(i0 + k);
    }
    __syncthreads();
    const uint32_t total = s_n;
    for (uint32_t i = tid; i < total; i += kBlock) {
        const uint32_t id = s_id[i];
        const float4 cd = g.rgbd[id];
        if (color_pending(cd)) resolve_color(cs, f.campos, id, cd.w, g.rgbd, g.clamped);
    }
}

// Strip-walk group size of the forward kernel (the instantiations launch_render_forward dispatches on). Same images bit for
// bit; 1 is the one-entry loop, kept as the partner of the exactness test and of A/B timing. (8 was built and measured: it
// passed the same A/B and came out 3.8 us behind 4, profiles/render_forward_groups_ab.txt.)
constexpr int kForwardGroupDefault = 4;
static bool forward_group_built(int g) { return g == 1 || g == 4; }
static int g_forward_group = [] { const char* e = getenv("MVI_RASTER_FORWARD_GROUP"); const int v = e ? atoi(e) : 0;
                                  return forward_group_built(v) ? v : kForwardGroupDefault; }();
int set_forward_group(int g) {
    const int old = g_forward_group;
    if (g == -1) return old;
    if (g != 0 && !forward_group_built(g)) return MVI_EINVAL;
    g_forward_group = g == 0 ? kForwardGroupDefault : g;
    return old;
}

// Tile order of the render backward (mvi_raster_backward_order): 1 = every XCD band hands out its tiles heaviest class first,
// from the queues the forward filled; 0 = plain tile order inside the band (xcd_band_tile). 1 is the default: on the bench view
// (8160 tiles, 3.2 per resident block slot) it took render_backward_kernel from 364 to 338 us and the step from 0.845 to 0.816 ms,
// every repetition below every one of the parent's, for 3 us more in render_forward (profiles/render_backward_order_ab.txt).
constexpr int kBackwardOrderDefault = 1;
static int g_backward_order = [] { const char* e = getenv("MVI_RASTER_BACKWARD_ORDER");
                                   return e && (e[0] == '0' || e[0] == '1') && e[1] == 0 ? e[0] - '0' : kBackwardOrderDefault; }();
int set_backward_order(int order) {
    const int old = g_backward_order;
    if (order == -1) return old;
    if (order != 0 && order != 1) return MVI_EINVAL;
    g_backward_order = order;
    return old;
}
// Which image scratches hold class queues that a render_forward of this process filled, PER IMAGE SCRATCH and by size (the
// pattern of raster_api.hip's SegmentHint): an entry describes the scratch's contents. Unknown scratch (never rendered into
// here, copied elsewhere, or evicted): the backward takes the plain order, which needs nothing from the forward.
namespace {
struct QueueNote { const void* image; int W, H; uint64_t stamp; };
constexpr int kQueueNotes = 64;
QueueNote g_queue_notes[kQueueNotes] = {};
uint64_t g_queue_clock = 0;
std::mutex g_queue_mutex;
void note_queue_filled(const void* image, int W, int H) {
    std::lock_guard<std::mutex> lock(g_queue_mutex);
    int slot = 0;
    for (int i = 0; i < kQueueNotes; ++i) {
        if (g_queue_notes[i].image == image) { slot = i; break; }
        if (g_queue_notes[i].stamp < g_queue_notes[slot].stamp) slot = i;     // else the least recently written
    }
    g_queue_notes[slot] = {image, W, H, ++g_queue_clock};
}
bool queue_filled(const void* image, int W, int H) {
    std::lock_guard<std::mutex> lock(g_queue_mutex);
    for (int i = 0; i < kQueueNotes; ++i)
        if (g_queue_notes[i].image == image && g_queue_notes[i].stamp) return g_queue_notes[i].W == W && g_queue_notes[i].H == H;
    return false;
}
}  // namespace

int launch_zero_fill(void* p, size_t bytes, hipStream_t st);
int launch_render_forward(const Frame& f, GeomView g, BinningView b, ImageView im, int64_t D,
                          float* out_color, float* out_depth, hipStream_t st, float* zero_rows, float* out_expected_depth,
                          float* out_alpha) {
    if ((out_expected_depth == nullptr) != (out_alpha == nullptr)) return MVI_EINVAL;
    ZeroRegions z;
    if (zero_rows) {
        z.add(zero_rows, (size_t)f.P * kGradRow);
        z.add(g.touched, ((size_t)f.P + 15) / 16 * 4);           // bytes, rounded up to the 16 the compaction reads at once
                                                                  // (inside the scratch segment's 256-byte padding)
    }
    if (f.W <= 0 || f.H <= 0) return launch_zero_regions(z, st);
    uint32_t* plist = b.vals[b.passes & 1];
    const unsigned blocks = (unsigned)(f.gx * f.gy);
    // lists expanded on demand: the binning of this call (launch_binning2, same test) wrote the ranges and no list
    const bool lazy = lazy_lists(f, D);
    LazyLists lz{};
    if (lazy) { lz.seg_yh = (const uint16_t*)b.keys[0]; lz.seg_idx = b.vals[0]; lz.col_start = g.col_start; }
    if (f.defer_colors && D > 0) {
        // MVI_RASTER_FRONT_ENTRIES: leading entries per tile evaluated ahead of the render kernel (0: none, A/B runs)
        static const int n_front = [] { const char* e = getenv("MVI_RASTER_FRONT_ENTRIES"); const int v = e ? atoi(e) : kBlock;
                                        return v < 0 ? 0 : (v > kFrontMax ? kFrontMax : v); }();
        static const int every = [] { const char* e = getenv("MVI_RASTER_FRONT_EVERY"); const int v = e ? atoi(e) : 2; return v < 1 ? 1 : v; }();
        if (n_front > 0) {
            const unsigned sampled = (unsigned)(((f.gx + every - 1) / every) * ((f.gy + every - 1) / every));
            if (lazy)
                hipLaunchKernelGGL(mark_front_lazy_kernel, dim3((sampled + kFrontTiles - 1) / kFrontTiles), dim3(kBlock), 0, st,
                                   (int)blocks, im.ranges, lz, g.front, n_front, g.color_src, f.gx, every);
            else
                hipLaunchKernelGGL(mark_front_kernel, dim3((sampled + kFrontTiles - 1) / kFrontTiles), dim3(kBlock), 0, st, (int)blocks,
                                   im.ranges, plist, g.front, n_front, g.color_src, f.gx, every);
            hipLaunchKernelGGL(resolve_marked_kernel, dim3((f.P + kBlock * kMarkedPer - 1) / (kBlock * kMarkedPer)), dim3(kBlock), 0, st,
                               f, g);
        }
    }
#define MVI_RENDER_FORWARD(G, AUX, LAZY)                                                                                          \
    hipLaunchKernelGGL((render_forward_kernel<G, AUX, LAZY>), dim3(blocks), dim3(kBlock), 0, st, f, im.ranges, plist, g.xy, g.rgbd, \
                       g.conic_opacity, im.final_T, im.n_contrib, out_color, out_depth, z, g.color_src, g.clamped,                  \
                       out_expected_depth, out_alpha, im.class_count, lz)
    switch (g_forward_group * 4 + (out_alpha ? 2 : 0) + (lazy ? 1 : 0)) {
        case 4: MVI_RENDER_FORWARD(1, false, false); break;
        case 5: MVI_RENDER_FORWARD(1, false, true); break;
        case 6: MVI_RENDER_FORWARD(1, true, false); break;
        case 7: MVI_RENDER_FORWARD(1, true, true); break;
        case 16: MVI_RENDER_FORWARD(4, false, false); break;
        case 17: MVI_RENDER_FORWARD(4, false, true); break;
        case 18: MVI_RENDER_FORWARD(4, true, false); break;
        case 19: MVI_RENDER_FORWARD(4, true, true); break;
        default: return MVI_EINVAL;                              // a kernel that is not built is an error, never another kernel
    }
#undef MVI_RENDER_FORWARD
    if (hipGetLastError() != hipSuccess) return MVI_EHIP;
    note_queue_filled(im.ranges, f.W, f.H);                      // `ranges` is the first byte of the image scratch
    return 0;
}

__global__ __launch_bounds__(256) void zero_regions_kernel(ZeroRegions z) { zero_share(z, threadIdx.x, 256); }
int launch_zero_regions(const ZeroRegions& z, hipStream_t st) {
    if (z.n == 0) return 0;
    hipLaunchKernelGGL(zero_regions_kernel, dim3(2048), dim3(256), 0, st, z);
    return hipGetLastError() == hipSuccess ? 0 : MVI_EHIP;
}

// ------------------------------------------------------------------------------------ backward
// Back-to-front replay over the entries [0, max n_contrib of the tile) only.
// Per evaluated (half tile, Gaussian) pair every pixel produces 9 RAW moments
//     W = o G dL/dalpha,  W dx,  W dy,  W dx^2,  W dx dy,  W dy^2,  alpha T dL/dC_{r,g,b}
// (the per-Gaussian factors — conic coefficients, 1/o, the 0.5 W / 0.5 H screen scale — are applied
// once per (tile, Gaussian) after the sums). A lane adds its two pixels, wave_sum9 sums the nine values over the 64 lanes
// in registers, and nine lanes add the wave totals into the block's per-entry accumulator (one LDS float atomic, nothing
// to wait for). Once per staged batch the block turns the raw sums into gradients and flushes
// them with float atomics shaped as whole 64-byte rows (16 lanes per Gaussian): MI355X float atomics
// run at the 64-B-request rate. Row layout of grad_rows [P][16]:
//   0 mean2D.x  1 mean2D.y  2 conic A  3 conic B  4 conic C  5 opacity  6 r  7 g  8 b  9 dL/dz (raster_render_aux.hip)  10..15 unused

// Diagnostics (mvi_raster_dev_wave_sum9): one wave per block runs in[w][m][lane] through wave_sum9, the owners write out[w][m]
__global__ __launch_bounds__(64) void wave_sum9_probe_kernel(const float* __restrict__ in, float* __restrict__ out) {
    const int lane = threadIdx.x;
    const float* x = in + (size_t)blockIdx.x * 9 * 64 + lane;
    const float s = wave_sum9(x[0], x[64], x[128], x[192], x[256], x[320], x[384], x[448], x[512]);
    if (wave_sum9_owner(lane)) out[blockIdx.x * 9 + wave_sum9_moment(lane)] = s;
}
int launch_wave_sum9_probe(const float* in, float* out, int n_waves, hipStream_t st) {
    if (n_waves <= 0) return 0;
    hipLaunchKernelGGL(wave_sum9_probe_kernel, dim3(n_waves), dim3(64), 0, st, in, out);
    return hipGetLastError() == hipSuccess ? 0 : MVI_EHIP;
}

// ---- backward, two pixels per lane --------------------------------------------------------------------------------
// Back-to-front replay of the tile's list (positions < max n_contrib of the tile only) with the same exact box
// culling as the forward. Every pixel produces 9 raw moments per evaluated Gaussian (W, W dx, W dy, W dx^2, W dx dy,
// W dy^2, alpha T dL/dC); wave totals in registers (wave_sum9), added into the block's per-entry accumulator by nine
// lanes; per (tile, Gaussian) the block converts raw sums into gradients once and flushes them with float atomics
// shaped as whole 64-byte rows (grad_rows [P][16]).
// The kernel's time is its vector instructions at their issue prices (about 0.65 of that roof: DESIGN.md §8 item 3). With one
// pixel per lane it needed ~90 vector
// instructions per (wave, Gaussian), about a third of them (the cross-lane sums) independent of how many pixels the wave
// covers. Here a wave covers a 16x8 half tile, lane l owning the vertically adjacent pixels (x = l & 15, y = 2 (l >> 4) + {0, 1}):
// the per-pixel math runs on packed fp32 (v_pk_mul/add/fma_f32: two pixels per instruction at full rate), the two
// pixels are summed in the lane before the wave reduction, and the reduction cost is paid once per 128 pixels. The moments
// are factored: the two pixels are added before they meet dx, which they share (14 vector instructions, one of them packed, where
// the products per pixel took 18, eight of them packed, and a v_mov for the (dx, dx) pair). On a SIMD that has other waves to issue
// from, a packed fp32 instruction costs 4.1 cycles against 2.3 for a plain one (tools/experiments/valu_issue_probe.cpp): packed
// pays only where both halves do work that cannot be shared.
// Block = 128 threads = one tile; 128 list entries are staged per round. Decisions (alpha, active) use the same
// operation order as the forward kernel (products rounded, one fma per sum), element-wise.
// Registers decide the occupancy (LDS: 10.5 KB per block, 12 blocks per CU fit). The entry loop keeps ONE entry in registers,
// read from LDS at the top of its iteration: 67 VGPRs and no scratch at five waves per SIMD (76 before the moments were factored,
// at five AND at six). MVI_RB_WAVES is the register allocator's target; the kernel now takes 67 VGPRs and no scratch at 5 and at 6.
// Five is the default. The work recorded as "six waves per SIMD"
// measured six and kept five (the same kernel time, the keep rule not passed: profiles/render_backward_six_waves_ab.txt), and
// six measured again on top of the heaviest-first tile order overlaps five in the step and in the kernel
// (profiles/render_backward_order_ab.txt).
#ifndef MVI_RB_WAVES
#define MVI_RB_WAVES 5             // waves per SIMD the register allocation aims at (A/B builds: -DMVI_RB_WAVES=6)
#endif
// Tile of workgroup `bid` when the band's tiles are handed out heaviest first: the hardware starts workgroups in id order, a
// block's work is its tile's largest n_contrib, and in plain tile order the heavy tiles that happen to start in the last of
// the launch's ~3 rounds run on alone over an emptying GPU. Band x = bid & 7 (the XCD, as in xcd_band_tile: band membership
// and the L2 a Gaussian's row atomics meet in are unchanged); its i-th workgroup takes the i-th tile of the band's queues read
// from the heaviest class down. The 16 counts are wave-uniform (scalar loads), and they sum to the band's size, so the map is
// a bijection; queue position and tile are clamped all the same, so that no scratch content sends a block outside the image.
__device__ __forceinline__ int heaviest_first_tile(int bid, int tiles, const uint32_t* __restrict__ class_count) {
    const int queue_stride = tile_queue_stride(tiles);
    const int x = bid & (kTileBands - 1);
    uint32_t rel = (uint32_t)bid >> 3;
    const uint32_t* cc = class_count + x * kTileClasses;
    int c = kTileClasses - 1;
#pragma unroll
    for (int k = kTileClasses - 1; k > 0; --k) {
        const uint32_t n = cc[k];
        if (c == k && rel >= n) { rel -= n; c = k - 1; }     // c == k: no heavier class holds position `rel`
    }
    rel = min(rel, (uint32_t)(queue_stride - 1));
    const uint32_t t = tile_class_queues(class_count)[(size_t)(x * kTileClasses + c) * queue_stride + rel];
    return (int)min(t, (uint32_t)(tiles - 1));
}
template <bool QUEUE>
__global__ __launch_bounds__(kB2) __attribute__((amdgpu_waves_per_eu(MVI_RB_WAVES, MVI_RB_WAVES))) void render_backward_kernel(
    Frame f, const uint32_t* __restrict__ ranges, const uint32_t* __restrict__ point_list,
    const float2* __restrict__ xy, const float4* __restrict__ rgbd, const float4* __restrict__ conic_opacity,
    const float* __restrict__ final_T, const uint32_t* __restrict__ n_contrib,
    const float* __restrict__ dL_dpix, float* __restrict__ grad_rows, uint8_t* __restrict__ touched, ZeroRegions zero,
    const uint32_t* __restrict__ class_count) {
#pragma clang fp contract(off)
    // the dense gradient outputs of the per-Gaussian chain rule are zeroed HERE (this kernel is bound by vector issue, its
    // memory pipes are idle): preprocess_backward then only writes the few per cent of rows that received a gradient
    zero_share(zero, threadIdx.x, kB2);
    // a staged entry is ONE record in one array: [0] (x, y, t2, Gaussian id), [1] conic + opacity, [2] colour — the reads of an
    // entry share one address register with constant offsets (the forward's w_s layout)
    __shared__ float4 s_ent[3][kB2];
    __shared__ float s_acc[kB2][9];                                   // raw moment sums per staged entry
    __shared__ uint32_t s_blast[2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tile = QUEUE ? heaviest_first_tile(blockIdx.x, f.gx * f.gy, class_count)
                           : xcd_band_tile(blockIdx.x, f.gx * f.gy);
    const int tile_y = tile / f.gx, tile_x = tile - tile_y * f.gx;
    const int hx0 = tile_x * kTile, hy0 = tile_y * kTile + 8 * wave;                  // this wave's 16 x 8 half tile
    const int pxi = hx0 + (lane & 15), py0 = hy0 + 2 * (lane >> 4), py1 = py0 + 1;
    const bool in0 = pxi < f.W && py0 < f.H, in1 = pxi < f.W && py1 < f.H;
    const float pfx = (float)pxi;
    const f2 pfy = {(float)py0, (float)py1};
    const uint32_t r0 = ranges[2 * tile];
    const size_t hw = (size_t)f.H * f.W, pix0 = (size_t)py0 * f.W + pxi, pix1 = pix0 + f.W;

    const f2 T_final = {in0 ? final_T[pix0] : 0.0f, in1 ? final_T[pix1] : 0.0f};
    f2 T = T_final;
    const uint32_t last0 = in0 ? n_contrib[pix0] : 0u, last1 = in1 ? n_contrib[pix1] : 0u;
    // The reference's recurrence carries (accum_rec, last_color, last_alpha) per pixel and forms
    //     a_dot = last_alpha * last_color + (1 - last_alpha) * accum_rec
    // when the next contributing entry arrives. Here ONE value per pixel is carried: that a_dot for the next entry, updated by
    // the entry that changes it — A <- alpha * c_dot + (1 - alpha) * A, the same expression with the same operands, evaluated
    // one entry earlier (same bits). An entry that is not active for a pixel enters with alpha = 0 and o G = 0: A, T and every
    // moment are then unchanged by plain arithmetic (1 - 0 = 1, rcp(1) = 1, 0 * x = 0), so the eight selects that used to keep
    // six state values apart for the two pixels are two selects on alpha and two on o G.
    f2 A_dot = {0.f, 0.f};
    f2 dp0 = {0.f, 0.f}, dp1 = {0.f, 0.f}, dp2 = {0.f, 0.f};
    if (in0) { dp0.x = dL_dpix[pix0]; dp1.x = dL_dpix[hw + pix0]; dp2.x = dL_dpix[2 * hw + pix0]; }
    if (in1) { dp0.y = dL_dpix[pix1]; dp1.y = dL_dpix[hw + pix1]; dp2.y = dL_dpix[2 * hw + pix1]; }
    const f2 bg_dot = f.bg[0] * dp0 + f.bg[1] * dp1 + f.bg[2] * dp2;
    const f2 bg_term = -T_final * bg_dot;                   // dL/dalpha's background part is bg_term / (1 - alpha)
    uint32_t wave_last = max(last0, last1);
    for (int o = 32; o > 0; o >>= 1) wave_last = max(wave_last, (uint32_t)__shfl_xor((int)wave_last, o));
    if (lane == 0) s_blast[wave] = wave_last;
    __syncthreads();
    const int total = (int)max(s_blast[0], s_blast[1]);
    const int rounds = (total + kB2 - 1) / kB2;
    const bool owner = wave_sum9_owner(lane);
    // LDS byte address of this lane's moment in accumulator row 0; the row of entry j lies 36 j further, and j is wave-uniform:
    // one scalar multiply and one 32-bit vector add per entry (a generic pointer cost a 64-bit multiply-add on the vector unit)
    typedef __attribute__((address_space(3))) float lds_float;
    const uint32_t acc_lane = (uint32_t)(uintptr_t)(lds_float*)&s_acc[0][wave_sum9_moment(lane)];

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
            const int e = c + lane;
            const float4 ce = s_ent[0][e];
            const bool keep = e < n && (uint32_t)(hi - 1 - e) < wave_last &&
                              quad_overlap(make_float2(ce.x, ce.y), s_ent[1][e], ce.z, (float)hx0, (float)hy0, 15.0f, 7.0f);
            unsigned long long mask = ballot64(keep);
            // The entry is read at the top of its iteration, as in the forward kernel: the other waves of the SIMD cover the LDS
            // latency, and a second entry held in registers (18 of them, the loop body emitted twice) bought nothing measurable.
            while (mask != 0ull) {
                const int jc = c + __builtin_ctzll(mask);           // wave-uniform
                mask &= mask - 1;
                const float4* rec = &s_ent[0][jc];
                const float2 p = *reinterpret_cast<const float2*>(rec);
                const float4 co = rec[kB2], col = rec[2 * kB2];
                const uint32_t pos = (uint32_t)(hi - 1 - jc);
                const float dx = p.x - pfx;
                const f2 dy = splat(p.y) - pfy;
                const f2 power = gauss_power(co, dx, dy);          // the forward's rounding recipe
                const f2 G = {__expf(power.x), __expf(power.y)};    // power > 0 (inf, NaN) is never active: selected away
                const f2 oG = co.w * G;
                // alpha = min(0.99, o G) >= 1/255 iff o G >= 1/255, and min(0.99, 0) = 0: one select per pixel instead of two
                const bool act0 = pos < last0 && power.x <= 0.0f && oG.x >= kAlphaMin;
                const bool act1 = pos < last1 && power.y <= 0.0f && oG.y >= kAlphaMin;
                const f2 gm = {act0 ? oG.x : 0.0f, act1 ? oG.y : 0.0f};                // o G of the ACTIVE pixels, else 0
                const f2 am = __builtin_elementwise_min(splat(kAlphaMax), gm);         // alpha of the active pixels, else 0
                // (an active alpha is >= 1/255: nonzero bits. Asking the two lane predicates themselves made the compiler
                // materialise them as 0 / 1 and compare again: four vector instructions per entry)
                const unsigned long long any_active = ballot64((__float_as_uint(gm.x) | __float_as_uint(gm.y)) != 0u);
                const f2 om = splat(1.0f) - am;                      // in [0.01, 1]; exactly 1 for an inactive pixel
                const f2 inv = {__builtin_amdgcn_rcpf(om.x), __builtin_amdgcn_rcpf(om.y)};
                const f2 Tn = T * inv;                               // (= T for an inactive pixel)
                const f2 c_dot = pk_fma(splat(col.z), dp2, pk_fma(splat(col.y), dp1, col.x * dp0));
                const f2 dL_dalpha = pk_fma(c_dot - A_dot, Tn, bg_term * inv);
                const f2 dch = am * Tn, mw = gm * dL_dalpha;
                T = Tn;
                A_dot = pk_fma(am, c_dot, om * A_dot);
                if (any_active != 0ull) {                       // wave-uniform
                    // the lane's two pixels share dx: they are added FIRST and what they share is multiplied once (dx never
                    // meets a pixel's own weight); a sum over the two pixels is one product and one fma (contraction is off:
                    // the fma is written out). No packed operand but W dy, no (dx, dx) register pair
                    const float wy0 = mw.x * dy.x, wy1 = mw.y * dy.y;
                    float m_w = mw.x + mw.y;                                         // W
                    float m_x = m_w * dx;                                            // W dx
                    float m_y = wy0 + wy1;                                           // W dy
                    float m_xx = m_x * dx;                                           // W dx^2
                    float m_xy = m_y * dx;                                           // W dx dy
                    float m_yy = __builtin_fmaf(wy1, dy.y, wy0 * dy.x);              // W dy^2
                    float m_r = __builtin_fmaf(dch.y, dp0.y, dch.x * dp0.x);         // alpha T dL/dC
                    float m_g = __builtin_fmaf(dch.y, dp1.y, dch.x * dp1.x);
                    float m_b = __builtin_fmaf(dch.y, dp2.y, dch.x * dp2.x);
                    const float sum = wave_sum9(m_w, m_x, m_y, m_xx, m_xy, m_yy, m_r, m_g, m_b);
                    // both waves add into the same rows; nobody waits for it
                    uint32_t row = 36u * (uint32_t)jc;
                    asm("" : "+s"(row));                     // the product stays on the scalar unit
                    if (owner) __hip_atomic_fetch_add((lds_float*)(uintptr_t)(acc_lane + row), sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        __syncthreads();
        // flush, in two steps per wave (a wave handles the 64 staged entries with its own index range, so only the wave has to
        // agree on LDS): (1) ONE lane per entry turns the raw sums into the nine gradients in place and marks entries that
        // nobody evaluated; (2) 16 lanes per entry add the row with float atomics, one 64-byte request per Gaussian.
        // (Before: every one of the 16 lanes of an entry read all nine sums, tested them and ran a switch over its component.)
        {
            const int e1 = wave * 64 + lane;
            if (e1 < n) {
                float* a = s_acc[e1];
                const float a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6], a7 = a[7], a8 = a[8];
                // any sum != 0 (as floats: +0 and -0 both count as zero), on the bit patterns: nine compares and their 0 / 1
                // bookkeeping became five bitwise instructions and one compare
                const bool any = (((__float_as_uint(a0) | __float_as_uint(a1) | __float_as_uint(a2)) |
                                   (__float_as_uint(a3) | __float_as_uint(a4) | __float_as_uint(a5)) |
                                   (__float_as_uint(a6) | __float_as_uint(a7) | __float_as_uint(a8))) & 0x7FFFFFFFu) != 0u;
                if (any) {
                    const float4 co = s_ent[1][e1];
                    a[0] = -0.5f * (float)f.W * (co.x * a1 + co.y * a2);       // dL/dmean2D.x (NDC-scaled)
                    a[1] = -0.5f * (float)f.H * (co.z * a2 + co.y * a1);       // dL/dmean2D.y
                    a[2] = -0.5f * a3;                                         // dL/dA
                    a[3] = -a4;                                                // dL/dB
                    a[4] = -0.5f * a5;                                         // dL/dC
                    a[5] = a0 / co.w;                                          // dL/dopacity = sum G dL/dalpha
                } else {
                    s_ent[0][e1].w = __uint_as_float(0xFFFFFFFFu);                                   // never evaluated by either half tile
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            const int comp = lane & 15;
#pragma unroll 4
            for (int it = 0; it < 16; ++it) {
                const int e = wave * 64 + it * 4 + (lane >> 4);
                const uint32_t id = e < n ? __float_as_uint(s_ent[0][e].w) : 0xFFFFFFFFu;
                if (id == 0xFFFFFFFFu || comp >= 9) continue;
                atomicAdd(&grad_rows[(size_t)id * kRow + comp], s_acc[e][comp]);
                if (comp == 0) touched[id] = 1;                // gradient support (idempotent store)
            }
        }
    }
}

int launch_render_backward(const Frame& f, GeomView g, BinningView b, ImageView im, int64_t D,
                           const float* dL_dpix, float* grad_rows, hipStream_t st, const ZeroRegions* zero) {
    ZeroRegions z;
    if (zero) z = *zero;
    if (f.W <= 0 || f.H <= 0 || D <= 0) return launch_zero_regions(z, st);
    const uint32_t* plist = b.vals[b.passes & 1];
    // heaviest first only from queues that a forward of this process left in THIS scratch; otherwise the plain order
    if (g_backward_order == 1 && queue_filled(im.ranges, f.W, f.H))
        hipLaunchKernelGGL(render_backward_kernel<true>, dim3(f.gx * f.gy), dim3(kB2), 0, st, f, im.ranges, plist, g.xy, g.rgbd,
                           g.conic_opacity, im.final_T, im.n_contrib, dL_dpix, grad_rows, g.touched, z, im.class_count);
    else
        hipLaunchKernelGGL(render_backward_kernel<false>, dim3(f.gx * f.gy), dim3(kB2), 0, st, f, im.ranges, plist, g.xy, g.rgbd,
                           g.conic_opacity, im.final_T, im.n_contrib, dL_dpix, grad_rows, g.touched, z, (const uint32_t*)nullptr);
    return hipGetLastError() == hipSuccess ? 0 : MVI_EHIP;
}

}  // namespace mvi
