// Backward of the fused GroupNorm(+SiLU) of groupnorm_silu.hip for gfx950 — HBM-bound, deterministic (no atomics).
// Differentiates GroupNorm32 -> SiLU of the reference UNet under training
// (svd_inpaint1/sgm/modules/diffusionmodules/openaimodel.py:341-353 with the embedding bias in front, video_model.py:71-75 for the
// temporal form, attention.py:125-128 for the eps = 1e-6, no-SiLU stem norm).
//
//   u = x + chan_bias, xh = (u - mean) rstd per (video, group), z = w_c xh + b_c, y = silu(z) or z
//   g = dy silu'(z)                      silu'(z) = s (1 + z (1 - s)), s = sigmoid(z)
//   dweight_c = sum g xh, dbias_c = sum g;  A = sum_group w_c g, B = sum_group w_c g xh, m = elements of the group
//   dx = rstd (w_c g - A / m - xh B / m);   dchan_bias[row, c] = sum_positions dx
//
// x [rows = videos * T, C, S] as the forward takes it; (mean, rstd) [videos * G, 2] fp32 from the forward (mvi_groupnorm_forward's stats).
// Four launches, the two that touch the tensor on 64-channel x 128-position tiles (64 positions on the scalar path):
//   reduce   : per tile and channel sum g, sum g xh, sum xh over the tile's positions -> part [row, s_tile, C, 3]  (reads x, dy)
//   finalize : one block per (video, group): the tiles summed in a fixed order -> sums [row, C, 3]; A, B -> coef [videos * G, 2]
//              = rstd (A, B) / m; dchan_bias from the sums (no further pass over the tensor)
//   params   : dweight, dbias = sums over the rows (launched only when asked for)
//   apply    : dx = rstd w_c g - coef_A - xh coef_B                                         (reads x, dy again, writes dx)
// dy is read in place in one of three layouts: planes [rows, C, S]; stack3 [rows, 3 C, S] (the gradient of frame t is block 1 of
// row t + block 0 of row t + 1 + block 2 of row t - 1: the mirror of the forward's three writes); token-major [rows, S, C], which
// crosses LDS once (XOR-swizzled 16-byte chunks, so that the transposed reads of a wave spread over the banks).
//
// Token-major x, dy AND dx [rows, S, C] (mvi_groupnorm_tok2tok_backward: the norm between the two convolutions of a ResBlock,
// mvi_groupnorm_tok2tok_forward) have kernels of their own for the two passes over the tensor, gn_bwd_tok_reduce_kernel and
// gn_bwd_tok_apply_kernel: channels are contiguous in all three tensors, so nothing is transposed; finalize and params are the same
// launches on the same `part` layout.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "groupnorm_tok.h"
#include "unet_host.h"
#include "unet_io.h"

namespace mvi {

constexpr int kGbC = 64;                                  // channels per tile
constexpr int kGbBlock = 256;

struct GbGeom {
    int64_t S;                                            // positions per channel plane
    int C, Cg, G, T;                                      // T frames share one group's statistics
    int s_tiles, c_tiles, silu;
    const float *weight, *bias, *chan_bias, *stats;       // chan_bias nullable [rows, C]; stats [videos * G, 2] = (mean, rstd)
};

template <typename T, bool VEC> struct GbTile {
    static constexpr int W = VEC ? Io<T>::kVec : 1;      // elements per item (one 16-byte vector, or one scalar)
    static constexpr int TS = VEC ? 128 : 64;             // positions per tile
    static constexpr int IPR = TS / W;                    // items per channel row: 16 (bf16 / f16), 32 (fp32), 64 (scalar) lanes share a channel
    static constexpr int kItems = kGbC * IPR / kGbBlock;  // items per thread: 4, 8, 16
};

__device__ __forceinline__ float silu_grad(float z) {
    const float s = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(z * -1.4426950408889634f));
    return s * (1.0f + z * (1.0f - s));
}

// APPLY = false: the reduce launch; APPLY = true: the apply launch (coef = rstd (A, B) / m per (video, group)).
template <typename T, int LAYOUT, bool VEC, bool APPLY>
__global__ __launch_bounds__(kGbBlock) void gn_bwd_tile_kernel(const T* __restrict__ x, const T* __restrict__ dy, GbGeom q,
                                                              float* __restrict__ part, const float* __restrict__ coef,
                                                              T* __restrict__ dx) {
    using G_ = GbTile<T, VEC>;
    constexpr int W = G_::W, TS = G_::TS, IPR = G_::IPR, kItems = G_::kItems;
    constexpr bool kTok = LAYOUT == MVI_GN_DY_TOKENS, kSt3 = LAYOUT == MVI_GN_DY_STACK3;
    static_assert(!kTok || VEC, "the token-major layout exists on the vector path only");
    constexpr int NCH = kGbC / W;                         // 16-byte chunks per token row of the LDS image
    __shared__ __attribute__((aligned(16))) T s_d[kTok ? TS * kGbC : 8];
    // xh = (x + s_b) s_a with s_b = chan_bias - mean: centred FIRST, as the forward's apply passes are. Folded into one fma,
    // x rstd + (chan_bias - mean) rstd, the shift is rounded at the size of |mean| rstd instead of the spread: a constant group
    // then has an xh of a few 1e-6 instead of 0, a dweight that is not 0, and every dx of the group is off
    __shared__ float s_a[kGbC], s_b[kGbC], s_w[kGbC], s_bias[kGbC], s_k2[kGbC], s_k3[kGbC];
    int bid = blockIdx.x;
    const int stile = bid % q.s_tiles; bid /= q.s_tiles;
    const int ctile = bid % q.c_tiles;
    const int64_t row = bid / q.c_tiles;
    const int C = q.C, c0 = ctile * kGbC;
    const int64_t S = q.S, s0 = (int64_t)stile * TS;
    const int slice = (int)(row % q.T);
    if (threadIdx.x < kGbC) {
        const int c = c0 + (int)threadIdx.x < C ? c0 + (int)threadIdx.x : C - 1;
        const int64_t vg = (row / q.T) * q.G + c / q.Cg;
        const float mean = q.stats[2 * vg], rstd = q.stats[2 * vg + 1];
        const float add = q.chan_bias ? q.chan_bias[row * C + c] : 0.f;
        s_a[threadIdx.x] = rstd;
        s_b[threadIdx.x] = add - mean;
        s_w[threadIdx.x] = q.weight[c];
        s_bias[threadIdx.x] = q.bias[c];
        if constexpr (APPLY) { s_k2[threadIdx.x] = coef[2 * vg]; s_k3[threadIdx.x] = coef[2 * vg + 1]; }
    }
    const bool has_next = kSt3 && slice + 1 < q.T, has_prev = kSt3 && slice > 0;
    auto item_pos = [&](int j, int& cr, int& sv, int& c, int64_t& s) {
        const int i = threadIdx.x + kGbBlock * j;
        cr = i / IPR; sv = i % IPR;
        c = c0 + cr; s = s0 + (int64_t)sv * W;
        return c < C && s < S;
    };
    // element offset of (row r, channel c of channel block blk, position s) in a tensor of `nblk` C-blocks per row
    auto plane_off = [&](int64_t r, int nblk, int blk, int c, int64_t s) { return ((r * nblk + blk) * C + c) * S + s; };
    // every vector load is issued unconditionally at a clamped address (all of a thread's loads in flight together); items outside the
    // tensor are masked when they are used
    uint4 rx[VEC ? kItems : 1], rd[VEC ? kItems : 1], rd0[(VEC && kSt3) ? kItems : 1], rd2[(VEC && kSt3) ? kItems : 1];
    if constexpr (VEC) {
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            int cr, sv, c; int64_t s;
            item_pos(j, cr, sv, c, s);
            c = c < C ? c : C - 1; s = s < S ? s : S - W;
            rx[j] = *reinterpret_cast<const uint4*>(x + plane_off(row, 1, 0, c, s));
            if constexpr (LAYOUT == MVI_GN_DY_PLANES) rd[j] = *reinterpret_cast<const uint4*>(dy + plane_off(row, 1, 0, c, s));
            if constexpr (kSt3) rd[j] = *reinterpret_cast<const uint4*>(dy + plane_off(row, 3, 1, c, s));
        }
        if constexpr (kSt3) {
            // (a missing neighbour reads the frame's own block again: a valid address, the value is not used)
#pragma unroll
            for (int j = 0; j < kItems; ++j) {
                int cr, sv, c; int64_t s;
                item_pos(j, cr, sv, c, s);
                c = c < C ? c : C - 1; s = s < S ? s : S - W;
                rd0[j] = *reinterpret_cast<const uint4*>(dy + plane_off(has_next ? row + 1 : row, 3, has_next ? 0 : 1, c, s));
                rd2[j] = *reinterpret_cast<const uint4*>(dy + plane_off(has_prev ? row - 1 : row, 3, has_prev ? 2 : 1, c, s));
            }
        }
        if constexpr (kTok) {
            // dy tile [TS tokens][64 channels], 16 bytes (W channels) per load; chunk cv of token sr goes to chunk cv ^ (sr / W) of its row
            constexpr int kTokLoads = TS * NCH / kGbBlock;
            uint4 rt[kTokLoads];
#pragma unroll
            for (int j = 0; j < kTokLoads; ++j) {
                const int i = threadIdx.x + kGbBlock * j;
                const int sr = i / NCH, cv = i % NCH;
                const int64_t s = s0 + sr < S ? s0 + sr : S - 1;
                const int c = c0 + cv * W < C ? c0 + cv * W : C - W;
                rt[j] = *reinterpret_cast<const uint4*>(dy + (row * S + s) * C + c);
            }
#pragma unroll
            for (int j = 0; j < kTokLoads; ++j) {
                const int i = threadIdx.x + kGbBlock * j;
                const int sr = i / NCH, cv = i % NCH;
                *reinterpret_cast<uint4*>(&s_d[sr * kGbC + ((cv ^ ((sr / W) & (NCH - 1))) * W)]) = rt[j];
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        int cr, sv, c; int64_t s;
        const bool ok = item_pos(j, cr, sv, c, s);
        float xv[W], gv[W];
        if constexpr (VEC) {
            Io<T>::load(reinterpret_cast<const T*>(&rx[j]), xv);
            if constexpr (kTok) {
#pragma unroll
                for (int k = 0; k < W; ++k)
                    gv[k] = Io<T>::ld1(&s_d[(sv * W + k) * kGbC + (((cr / W) ^ (sv & (NCH - 1))) * W) + (cr % W)]);
            } else {
                Io<T>::load(reinterpret_cast<const T*>(&rd[j]), gv);
                if constexpr (kSt3) {
                    float t0[W], t2[W];
                    Io<T>::load(reinterpret_cast<const T*>(&rd0[j]), t0);
                    Io<T>::load(reinterpret_cast<const T*>(&rd2[j]), t2);
#pragma unroll
                    for (int k = 0; k < W; ++k) gv[k] += (has_next ? t0[k] : 0.f) + (has_prev ? t2[k] : 0.f);
                }
            }
        } else {
            xv[0] = 0.f; gv[0] = 0.f;
            if (ok) {
                xv[0] = Io<T>::ld1(x + plane_off(row, 1, 0, c, s));
                if constexpr (LAYOUT == MVI_GN_DY_PLANES) gv[0] = Io<T>::ld1(dy + plane_off(row, 1, 0, c, s));
                if constexpr (kSt3) {
                    gv[0] = Io<T>::ld1(dy + plane_off(row, 3, 1, c, s));
                    if (has_next) gv[0] += Io<T>::ld1(dy + plane_off(row + 1, 3, 0, c, s));
                    if (has_prev) gv[0] += Io<T>::ld1(dy + plane_off(row - 1, 3, 2, c, s));
                }
            }
        }
        const float a = s_a[cr], b = s_b[cr], w = s_w[cr], bi = s_bias[cr];
        float p0 = 0.f, p1 = 0.f, p2 = 0.f;
        float ov[W];
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const float xh = (xv[k] + b) * a;
            const float gg = q.silu ? gv[k] * silu_grad(w * xh + bi) : gv[k];
            if constexpr (APPLY) {
                ov[k] = (a * w) * gg - s_k2[cr] - xh * s_k3[cr];
            } else {
                ov[k] = 0.f;
                p0 += gg; p1 += gg * xh; p2 += xh;
            }
        }
        if constexpr (APPLY) {
            if (ok) {
                if constexpr (VEC) Io<T>::store(dx + plane_off(row, 1, 0, c, s), ov);
                else Io<T>::st1(dx + plane_off(row, 1, 0, c, s), ov[0]);
            }
        } else {
            if (!ok) { p0 = 0.f; p1 = 0.f; p2 = 0.f; }
            // the IPR lanes of a channel row are consecutive lanes of one wave: butterfly, the same order in every run
#pragma unroll
            for (int o = IPR / 2; o > 0; o >>= 1) { p0 += __shfl_xor(p0, o); p1 += __shfl_xor(p1, o); p2 += __shfl_xor(p2, o); }
            if (sv == 0 && c < C) {
                float* p = part + ((row * q.s_tiles + stile) * C + c) * 3;
                p[0] = p0; p[1] = p1; p[2] = p2;
            }
        }
    }
}

// One block per (video, group). Lane l of every wave owns entry e = e0 + l = (frame, channel of the group); wave w sums the tiles
// st = w, w + 4, ...; the four waves' sums are added in wave order. Wave 0 then accumulates A and B and writes the outputs.
__global__ __launch_bounds__(kGbBlock) void gn_bwd_finalize_kernel(const float* __restrict__ part, GbGeom q, float* sums,
                                                                  float* __restrict__ coef, float* __restrict__ dchan_bias) {
    __shared__ float s_p[4][64][3];
    const int64_t vg = blockIdx.x, video = vg / q.G;
    const int g = (int)(vg % q.G), lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int entries = q.T * q.Cg, C = q.C;
    float accA = 0.f, accB = 0.f;
    for (int e0 = 0; e0 < entries; e0 += 64) {
        const int e = e0 + lane;
        const bool ok = e < entries;
        const int64_t row = video * q.T + (ok ? e / q.Cg : 0);
        const int c = g * q.Cg + (ok ? e % q.Cg : 0);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        if (ok) {
            for (int st = wv; st < q.s_tiles; st += 4) {
                const float* p = part + ((row * q.s_tiles + st) * C + c) * 3;
                a0 += p[0]; a1 += p[1]; a2 += p[2];
            }
        }
        s_p[wv][lane][0] = a0; s_p[wv][lane][1] = a1; s_p[wv][lane][2] = a2;
        __syncthreads();
        if (wv == 0 && ok) {
            float t[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = ((s_p[0][lane][k] + s_p[1][lane][k]) + s_p[2][lane][k]) + s_p[3][lane][k];
            float* o = sums + (row * C + c) * 3;
            o[0] = t[0]; o[1] = t[1]; o[2] = t[2];
            const float w = q.weight[c];
            accA += w * t[0]; accB += w * t[1];
        }
        __syncthreads();
    }
    if (wv != 0) return;
    for (int o = 32; o > 0; o >>= 1) { accA += __shfl_xor(accA, o); accB += __shfl_xor(accB, o); }
    const float inv_m = 1.0f / ((float)entries * (float)q.S);
    const float rstd = q.stats[2 * vg + 1];
    const float Am = accA * inv_m, Bm = accB * inv_m;
    if (lane == 0) { coef[2 * vg] = rstd * Am; coef[2 * vg + 1] = rstd * Bm; }
    if (!dchan_bias) return;
    // sum over positions of dx = rstd (w sum g - S A / m - sum xh B / m): each lane re-reads the sums it wrote itself
    for (int e = lane; e < entries; e += 64) {
        const int64_t row = video * q.T + e / q.Cg;
        const int c = g * q.Cg + e % q.Cg;
        const float* o = sums + (row * C + c) * 3;
        dchan_bias[row * C + c] = rstd * (q.weight[c] * o[0] - (float)q.S * Am - o[2] * Bm);
    }
}

// dweight_c = sum over rows of sum g xh, dbias_c = sum over rows of sum g: one thread per channel, rows in order (C threads on the
// whole chip walking `rows` = 14 ... 28 triples each: a few microseconds, bound by its launch; a batch of thousands of rows would want
// the rows split over lanes)
__global__ __launch_bounds__(kGbBlock) void gn_bwd_params_kernel(const float* __restrict__ sums, int64_t rows, int C,
                                                                float* __restrict__ dweight, float* __restrict__ dbias) {
    const int c = blockIdx.x * kGbBlock + threadIdx.x;
    if (c >= C) return;
    float dw = 0.f, db = 0.f;
    for (int64_t r = 0; r < rows; ++r) {
        const float* o = sums + (r * C + c) * 3;
        db += o[0]; dw += o[1];
    }
    if (dweight) dweight[c] = dw;
    if (dbias) dbias[c] = db;
}

struct GbPlan {
    bool vec;
    int s_tiles, c_tiles;
    int64_t blocks;
    size_t part_floats, sums_floats, coef_floats;
};

static int gb_elems_per_vec(int dtype) { return dtype == MVI_DT_F32 ? 4 : 8; }

// vec: the 16-byte path (S % W == 0, aligned bases); the workspace is sized for the scalar tiling, which has more tiles
static bool gb_plan(int64_t videos, int T, int C, int64_t S, int G, int dtype, bool vec, GbPlan* p) {
    if (videos <= 0 || T <= 0 || C <= 0 || S <= 0 || G <= 0 || C % G != 0 || dtype < 0 || dtype > 2) return false;
    const int ts = vec ? 128 : 64;
    const int64_t st = (S + ts - 1) / ts, ct = (C + kGbC - 1) / kGbC, rows = videos * T;
    const int64_t blocks = rows * st * ct;
    if (blocks > 0x7FFFFFFFll || st > 0x7FFFFFll || videos * G > 0x7FFFFFFFll) return false;
    p->vec = vec; p->s_tiles = (int)st; p->c_tiles = (int)ct; p->blocks = blocks;
    p->part_floats = (size_t)(rows * st) * C * 3;
    p->sums_floats = (size_t)rows * C * 3;
    p->coef_floats = (size_t)(videos * G) * 2;
    return true;
}

template <typename T, int LAYOUT, bool VEC>
static void gb_launch_tiles(const void* x, const void* dy, const GbGeom& q, const GbPlan& p, float* part, const float* coef, void* dx,
                            bool apply, hipStream_t st) {
    dispatch_flag(apply, [&](auto k) {
        hipLaunchKernelGGL((gn_bwd_tile_kernel<T, LAYOUT, VEC, decltype(k)::value>), dim3((unsigned)p.blocks), dim3(kGbBlock), 0, st,
                           (const T*)x, (const T*)dy, q, part, coef, (T*)dx);
    });
}

template <typename T>
static int gb_run(const void* x, const void* dy, const GbGeom& q, const GbPlan& p, int layout, int64_t videos, float* ws, float* dweight,
                  float* dbias, float* dchan_bias, void* dx, hipStream_t st) {
    float* part = ws;
    float* sums = part + p.part_floats;
    float* coef = sums + p.sums_floats;
    for (int apply = 0; apply < 2; ++apply) {
        if (apply && !dx) break;
        if (layout == MVI_GN_DY_TOKENS) gb_launch_tiles<T, MVI_GN_DY_TOKENS, true>(x, dy, q, p, part, coef, dx, apply, st);
        else if (layout == MVI_GN_DY_STACK3 && p.vec) gb_launch_tiles<T, MVI_GN_DY_STACK3, true>(x, dy, q, p, part, coef, dx, apply, st);
        else if (layout == MVI_GN_DY_STACK3) gb_launch_tiles<T, MVI_GN_DY_STACK3, false>(x, dy, q, p, part, coef, dx, apply, st);
        else if (p.vec) gb_launch_tiles<T, MVI_GN_DY_PLANES, true>(x, dy, q, p, part, coef, dx, apply, st);
        else gb_launch_tiles<T, MVI_GN_DY_PLANES, false>(x, dy, q, p, part, coef, dx, apply, st);
        if (!apply) {
            hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3((unsigned)(videos * q.G)), dim3(kGbBlock), 0, st, part, q, sums, coef,
                               dchan_bias);
            if (dweight || dbias)
                hipLaunchKernelGGL(gn_bwd_params_kernel, dim3((unsigned)((q.C + kGbBlock - 1) / kGbBlock)), dim3(kGbBlock), 0, st, sums,
                                   videos * q.T, q.C, dweight, dbias);
        }
    }
    return hipGetLastError() == hipSuccess ? MVI_OK : MVI_EHIP;
}

// ---- token-major x, dy, dx [N, S, C] ------------------------------------------------------------------------------------------------
// The thread layout of groupnorm_tokens.hip: a block is vpr x rp threads (vpr = C / vec vectors per token row, rp rows per pass) on a
// tile of kGtPasses rp tokens, and a thread owns the SAME vec channels in every row — its per-channel constants (rstd, chan_bias - mean
// (xh = (x + that) rstd: centred first, see gn_bwd_tile_kernel), weight, bias, coef: looked up per CHANNEL, a vector may span groups)
// live in registers. kGkRows rows of x and of dy are in flight per thread and step (the step loop stays rolled: unrolled, the
// compiler hoists every step's loads and spills); every load is issued at a clamped row, rows past the end are masked where they
// are used.
constexpr int kGkRows = 4;

template <int V> struct GkChan { float a[V], b[V], w[V], bi[V]; };

template <int V> __device__ __forceinline__ void gk_channel_constants(const GbGeom& q, int64_t n, int c0, GkChan<V>& k, const float* coef,
                                                                      float* k2, float* k3) {
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int c = c0 + i;
        const int64_t vg = (n / q.T) * q.G + c / q.Cg;
        const float mean = q.stats[2 * vg], rstd = q.stats[2 * vg + 1];
        const float add = q.chan_bias ? q.chan_bias[n * q.C + c] : 0.f;
        k.a[i] = rstd;
        k.b[i] = add - mean;
        k.w[i] = q.weight[c];
        k.bi[i] = q.bias[c];
        if (coef) { k2[i] = coef[2 * vg]; k3[i] = coef[2 * vg + 1]; }
    }
}

// reduce: per tile and channel sum g, sum g xh, sum xh over the tile's tokens -> part [row, s_tile, C, 3]. A thread sums its rows in
// pass order; the rp threads that share a channel are added through LDS in row order.
template <typename T>
__global__ __launch_bounds__(1024) void gn_bwd_tok_reduce_kernel(const T* __restrict__ x, const T* __restrict__ dy, GbGeom q,
                                                                 float* __restrict__ part, int vpr, int rp) {
    constexpr int V = Io<T>::kVec;
    // 8 channels' constants and sums are 56 registers: two rows of x and dy per step keep the kernel inside the 128 a 1024-thread
    // block may use (four rows: 68 bytes of scratch)
    constexpr int kGkRows = V == 8 ? 2 : 4;
    extern __shared__ float s_red[];                       // [3][rp][C]
    const int tid = threadIdx.x, v = tid % vpr, r0 = tid / vpr;
    const int64_t n = blockIdx.y, S = q.S;
    const int st = blockIdx.x, C = q.C;
    const int64_t row0 = (int64_t)st * (kGtPasses * rp);
    GkChan<V> k;
    gk_channel_constants<V>(q, n, v * V, k, nullptr, nullptr, nullptr);
    const T* xb = x + (n * S) * C + (int64_t)v * V;
    const T* db = dy + (n * S) * C + (int64_t)v * V;
    float p0[V], p1[V], p2[V];
#pragma unroll
    for (int i = 0; i < V; ++i) p0[i] = p1[i] = p2[i] = 0.f;
#pragma unroll 1
    for (int h = 0; h < kGtPasses / kGkRows; ++h) {
        uint4 rx[kGkRows], rd[kGkRows];
#pragma unroll
        for (int p = 0; p < kGkRows; ++p) {
            const int64_t row = row0 + (h * kGkRows + p) * rp + r0;
            const int64_t rc = row < S ? row : S - 1;
            rx[p] = *reinterpret_cast<const uint4*>(xb + rc * C);
            rd[p] = *reinterpret_cast<const uint4*>(db + rc * C);
        }
#pragma unroll
        for (int p = 0; p < kGkRows; ++p) {
            const int64_t row = row0 + (h * kGkRows + p) * rp + r0;
            float xv[V], gv[V];
            Io<T>::load(reinterpret_cast<const T*>(&rx[p]), xv);
            Io<T>::load(reinterpret_cast<const T*>(&rd[p]), gv);
            const float m = row < S ? 1.f : 0.f;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const float xh = (xv[i] + k.b[i]) * k.a[i];
                const float gg = m * (q.silu ? gv[i] * silu_grad(k.w[i] * xh + k.bi[i]) : gv[i]);
                p0[i] += gg; p1[i] += gg * xh; p2[i] += m * xh;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < V; ++i) {
        s_red[((size_t)0 * rp + r0) * C + v * V + i] = p0[i];
        s_red[((size_t)1 * rp + r0) * C + v * V + i] = p1[i];
        s_red[((size_t)2 * rp + r0) * C + v * V + i] = p2[i];
    }
    __syncthreads();
    for (int c = tid; c < C; c += blockDim.x) {
        float* o = part + ((n * q.s_tiles + st) * C + c) * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float t = 0.f;
            for (int r = 0; r < rp; ++r) t += s_red[((size_t)j * rp + r) * C + c];
            o[j] = t;
        }
    }
}

// apply: dx = rstd w_c g - coef_A - xh coef_B, a straight 16-byte load / store pass
template <typename T>
__global__ __launch_bounds__(1024) void gn_bwd_tok_apply_kernel(const T* __restrict__ x, const T* __restrict__ dy, GbGeom q,
                                                                const float* __restrict__ coef, T* __restrict__ dx, int vpr, int rp) {
    constexpr int V = Io<T>::kVec;
    const int tid = threadIdx.x, v = tid % vpr, r0 = tid / vpr;
    const int64_t n = blockIdx.y, S = q.S;
    const int C = q.C;
    const int64_t row0 = (int64_t)blockIdx.x * (kGtPasses * rp);
    GkChan<V> k;
    float k2[V], k3[V];
    gk_channel_constants<V>(q, n, v * V, k, coef, k2, k3);
    const int64_t off = (n * S) * C + (int64_t)v * V;
#pragma unroll 1
    for (int h = 0; h < kGtPasses / kGkRows; ++h) {
        uint4 rx[kGkRows], rd[kGkRows];
#pragma unroll
        for (int p = 0; p < kGkRows; ++p) {
            const int64_t row = row0 + (h * kGkRows + p) * rp + r0;
            const int64_t rc = row < S ? row : S - 1;
            rx[p] = *reinterpret_cast<const uint4*>(x + off + rc * C);
            rd[p] = *reinterpret_cast<const uint4*>(dy + off + rc * C);
        }
#pragma unroll
        for (int p = 0; p < kGkRows; ++p) {
            const int64_t row = row0 + (h * kGkRows + p) * rp + r0;
            float xv[V], gv[V], ov[V];
            Io<T>::load(reinterpret_cast<const T*>(&rx[p]), xv);
            Io<T>::load(reinterpret_cast<const T*>(&rd[p]), gv);
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const float xh = (xv[i] + k.b[i]) * k.a[i];
                const float gg = q.silu ? gv[i] * silu_grad(k.w[i] * xh + k.bi[i]) : gv[i];
                ov[i] = (k.a[i] * k.w[i]) * gg - k2[i] - xh * k3[i];
            }
            if (row < S) Io<T>::store(dx + off + row * C, ov);
        }
    }
}

struct GkPlan {
    int vpr, rp, s_tiles;
    size_t lds, part_floats, sums_floats, coef_floats;
};

// the forward's geometry (gt_geometry_ok: C a multiple of the groups (<= 64) and of the vector, at most 65535 samples), whole videos,
// the reduce pass's LDS image within 64 KB, and grids / tables within 32 bits
static bool gk_plan(int64_t N, int T, int C, int64_t S, int G, int dtype, GkPlan* p) {
    if (dtype < 0 || dtype > 2 || T < 1 || !gt_geometry_ok(N, C, S, G, dtype) || N % T != 0) return false;
    const int V = gb_elems_per_vec(dtype);
    p->vpr = C / V; p->rp = gt_rows_per_pass(p->vpr);
    const int64_t tile = (int64_t)kGtPasses * p->rp, st = (S + tile - 1) / tile;
    p->lds = (size_t)3 * p->rp * C * sizeof(float);
    if (p->lds > 64 * 1024 || st > 0x7FFFFFll || N * st > 0x7FFFFFFFll || N / T * G > 0x7FFFFFFFll) return false;
    p->s_tiles = (int)st;
    p->part_floats = (size_t)(N * st) * C * 3;
    p->sums_floats = (size_t)N * C * 3;
    p->coef_floats = (size_t)(N / T * G) * 2;
    return true;
}

template <typename T>
static int gk_run(const void* x, const void* dy, const GbGeom& q, const GkPlan& p, int64_t N, float* ws, float* dweight, float* dbias,
                  float* dchan_bias, void* dx, hipStream_t st) {
    float* part = ws;
    float* sums = part + p.part_floats;
    float* coef = sums + p.sums_floats;
    const dim3 grid((unsigned)p.s_tiles, (unsigned)N), block((unsigned)(p.vpr * p.rp));
    hipLaunchKernelGGL((gn_bwd_tok_reduce_kernel<T>), grid, block, p.lds, st, (const T*)x, (const T*)dy, q, part, p.vpr, p.rp);
    hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3((unsigned)(N / q.T * q.G)), dim3(kGbBlock), 0, st, part, q, sums, coef, dchan_bias);
    if (dweight || dbias)
        hipLaunchKernelGGL(gn_bwd_params_kernel, dim3((unsigned)((q.C + kGbBlock - 1) / kGbBlock)), dim3(kGbBlock), 0, st, sums, N, q.C,
                           dweight, dbias);
    if (dx) hipLaunchKernelGGL((gn_bwd_tok_apply_kernel<T>), grid, block, 0, st, (const T*)x, (const T*)dy, q, coef, (T*)dx, p.vpr, p.rp);
    return hipGetLastError() == hipSuccess ? MVI_OK : MVI_EHIP;
}

}  // namespace mvi

extern "C" int mvi_groupnorm_tok2tok_backward_supported(int64_t N, int32_t frames, int32_t C, int64_t spatial, int32_t groups,
                                                        int32_t dtype) {
    mvi::GkPlan p;
    return mvi::gk_plan(N, frames, C, spatial, groups, dtype, &p) ? 1 : 0;
}

extern "C" size_t mvi_groupnorm_tok2tok_backward_workspace_bytes(int64_t N, int32_t frames, int32_t C, int64_t spatial, int32_t groups,
                                                                 int32_t dtype) {
    mvi::GkPlan p;
    if (!mvi::gk_plan(N, frames, C, spatial, groups, dtype, &p)) return 0;
    return (p.part_floats + p.sums_floats + p.coef_floats) * sizeof(float);
}

extern "C" int mvi_groupnorm_tok2tok_backward(const void* x, const void* dy, const float* stats, const float* weight, const float* bias,
                                              const float* chan_bias, void* dx, float* dweight, float* dbias, float* dchan_bias, int64_t N,
                                              int32_t frames, int32_t C, int64_t spatial, int32_t groups, int32_t fuse_silu, int32_t dtype,
                                              void* workspace, size_t workspace_bytes, void* stream) {
    if (N == 0 || spatial == 0) return MVI_OK;
    mvi::GkPlan p;
    if (!mvi::gk_plan(N, frames, C, spatial, groups, dtype, &p))
        return mvi::unet_fail(MVI_EINVAL, "groupnorm_tok2tok backward: unsupported shape or dtype");
    if (!x || !dy || !stats || !weight || !bias || !workspace) return mvi::unet_fail(MVI_EINVAL, "groupnorm_tok2tok backward: NULL pointer");
    if (dchan_bias && !chan_bias) return mvi::unet_fail(MVI_EINVAL, "groupnorm_tok2tok backward: dchan_bias without chan_bias");
    if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) % 16)
        return mvi::unet_fail(MVI_EINVAL, "groupnorm_tok2tok backward: x / dy / dx must be 16-byte aligned");
    if (workspace_bytes < (p.part_floats + p.sums_floats + p.coef_floats) * sizeof(float) || (uintptr_t)workspace % 4 != 0)
        return mvi::unet_fail(MVI_ENOMEM, "groupnorm_tok2tok backward: workspace too small or misaligned");
    mvi::GbGeom q;
    q.S = spatial; q.C = C; q.Cg = C / groups; q.G = groups; q.T = frames;
    q.s_tiles = p.s_tiles; q.c_tiles = 0; q.silu = fuse_silu ? 1 : 0;
    q.weight = weight; q.bias = bias; q.chan_bias = chan_bias; q.stats = stats;
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    return mvi::dispatch_dtype(dtype, "groupnorm_tok2tok backward: unknown dtype", [&](auto t) {
        return mvi::gk_run<typename decltype(t)::type>(x, dy, q, p, N, ws, dweight, dbias, dchan_bias, dx, st)
                   ? mvi::unet_fail(MVI_EHIP, "groupnorm_tok2tok backward: kernel launch failed") : MVI_OK;
    });
}

extern "C" int mvi_groupnorm_backward_supported(int64_t videos, int32_t T, int32_t C, int64_t spatial, int32_t groups, int32_t dy_layout,
                                                int32_t dtype) {
    mvi::GbPlan p;
    if (dy_layout < MVI_GN_DY_PLANES || dy_layout > MVI_GN_DY_TOKENS) return 0;
    if (!mvi::gb_plan(videos, T, C, spatial, groups, dtype, false, &p)) return 0;
    if (videos * groups > 65535) return 0;                 // the forward's grid.y
    if (dy_layout == MVI_GN_DY_TOKENS) {
        const int w = mvi::gb_elems_per_vec(dtype);
        if (T != 1 || C % w != 0 || spatial % w != 0) return 0;
    }
    return 1;
}

extern "C" size_t mvi_groupnorm_backward_workspace_bytes(int64_t videos, int32_t T, int32_t C, int64_t spatial, int32_t groups) {
    mvi::GbPlan p;
    if (!mvi::gb_plan(videos, T, C, spatial, groups, MVI_DT_F32, false, &p)) return 0;
    return (p.part_floats + p.sums_floats + p.coef_floats) * sizeof(float);
}

extern "C" int mvi_groupnorm_backward(const void* x, const void* dy, const float* stats, const float* weight, const float* bias,
                                      const float* chan_bias, void* dx, float* dweight, float* dbias, float* dchan_bias, int64_t videos,
                                      int32_t T, int32_t C, int64_t spatial, int32_t groups, int32_t fuse_silu, int32_t dy_layout,
                                      int32_t dtype, void* workspace, size_t workspace_bytes, void* stream) {
    if (videos == 0 || spatial == 0) return MVI_OK;
    if (!mvi_groupnorm_backward_supported(videos, T, C, spatial, groups, dy_layout, dtype))
        return mvi::unet_fail(MVI_EINVAL, "groupnorm backward: unsupported shape, layout or dtype");
    if (!x || !dy || !stats || !weight || !bias || !workspace) return mvi::unet_fail(MVI_EINVAL, "groupnorm backward: NULL pointer");
    if (dchan_bias && !chan_bias) return mvi::unet_fail(MVI_EINVAL, "groupnorm backward: dchan_bias without chan_bias");
    if (workspace_bytes < mvi_groupnorm_backward_workspace_bytes(videos, T, C, spatial, groups) || (uintptr_t)workspace % 4 != 0)
        return mvi::unet_fail(MVI_ENOMEM, "groupnorm backward: workspace too small or misaligned");
    const int w = mvi::gb_elems_per_vec(dtype);
    const bool aligned = (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) % 16) == 0;
    const bool vec = aligned && spatial % w == 0 && (dy_layout != MVI_GN_DY_TOKENS || C % w == 0);
    if (dy_layout == MVI_GN_DY_TOKENS && !vec)
        return mvi::unet_fail(MVI_EINVAL, "groupnorm backward (token-major dy): C and spatial must be multiples of the 16-byte vector, 16-B aligned");
    mvi::GbPlan p;
    if (!mvi::gb_plan(videos, T, C, spatial, groups, dtype, vec, &p)) return mvi::unet_fail(MVI_EINVAL, "groupnorm backward: shape too large");
    mvi::GbGeom q;
    q.S = spatial; q.C = C; q.Cg = C / groups; q.G = groups; q.T = T;
    q.s_tiles = p.s_tiles; q.c_tiles = p.c_tiles; q.silu = fuse_silu ? 1 : 0;
    q.weight = weight; q.bias = bias; q.chan_bias = chan_bias; q.stats = stats;
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    return mvi::dispatch_dtype(dtype, "groupnorm backward: unknown dtype", [&](auto t) {          // (gb_plan has turned an unknown dtype down)
        return mvi::gb_run<typename decltype(t)::type>(x, dy, q, p, dy_layout, videos, ws, dweight, dbias, dchan_bias, dx, st)
                   ? mvi::unet_fail(MVI_EHIP, "groupnorm backward: kernel launch failed") : MVI_OK;
    });
}
