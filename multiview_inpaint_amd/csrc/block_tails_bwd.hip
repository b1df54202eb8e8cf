// Backward of the block tails for gfx950 (training): the adjoints of token_rows.hip's tokens_to_planes_add / tokens_blend_to_planes
// (the passes that end a ResBlock, a temporal ResBlock, a SpatialTransformer) and of add_lerp (the AlphaBlender of the video
// transformer). All HBM-bound, one pass each, bf16 / f16, no atomics: every sum is formed in a fixed order, so two calls give the
// same bits.
//
//   planes_tail_backward : dy [N, C, S] planes -> d_tok[n, p, c] = (1 - alpha[n]) dy[n, c, p]  (mode A, alpha NULL: the transposition)
//                          d_base[n, p, c] = dy[n, c, p]                                        (mode B only)
//                          colsum[n, pg, c] = sum over the block's pixels of dy[n, c, p]         (fp32 partials, for dbias and dalpha)
//                          dot[n, pg, ct]   = sum over the block's tile(s) of dy[n, c, p] tok[n, p, c]    (for dalpha)
//                          through the 64 x 64 LDS tile of tokens_to_planes_add_kernel, 16-byte accesses on both sides
//   rows_tail_backward   : dy [R, C] rows -> d_t = (1 - alpha[g]) dy, d_base = alpha[g] dy, g = r / row_div, and one fp32 partial per
//                          block of sum dy (base - round(x + h)); a block covers rows of ONE group
//   tails_reduce         : adds the partials in an order fixed by the shape: dbias[c] = sum_n w_n sum_pg colsum, dalpha_n = -(sum dot + sum_c bias[c]
//                          sum_pg colsum[n, pg, c]), dalpha_g = sum of the group's partials. One kernel, the block index picks the job.
#include <hip/hip_runtime.h>

#include "unet_host.h"
#include "unet_io.h"

namespace mvi {
namespace tails {

constexpr int kTile = 64;                 // pixels x channels of an LDS tile (token_rows.hip's kTpTile)
constexpr int kRowsVec = 4;               // 16-byte vectors of each tensor per thread of the row pass
constexpr int kRowsBlockVec = 256 * kRowsVec;

static int g_walk_override = 0;           // mvi_planes_tail_backward_set_walk: > 0 replaces the rule below (measurement only)

// Pixel tiles a block walks: large images cut the partial count (and the finishing kernel's serial length) by up to 8; from 16 tiles
// per walked run on, so that a sample still has 16 blocks per channel tile.
static int walk_of(int64_t S) {
    const int64_t p_tiles = (S + kTile - 1) / kTile;
    if (g_walk_override > 0) return (int)(g_walk_override < p_tiles ? g_walk_override : (p_tiles > 0 ? p_tiles : 1));
    const int64_t w = p_tiles / 16;
    return (int)(w < 1 ? 1 : (w > 8 ? 8 : w));
}

struct PlanesGeom { int p_tiles, c_tiles, walk, p_groups; };

static PlanesGeom planes_geom(int32_t C, int64_t S) {
    PlanesGeom g;
    g.p_tiles = (int)((S + kTile - 1) / kTile);
    g.c_tiles = (C + kTile - 1) / kTile;
    g.walk = walk_of(S);
    g.p_groups = (g.p_tiles + g.walk - 1) / g.walk;
    return g;
}

__device__ __forceinline__ float wave_sum(float v) {            // all 64 lanes end with the same, order-fixed sum
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sum over the block in a fixed order (waves 0..3); valid in thread 0. s_red: 4 floats; callers separate reuses by a barrier.
__device__ __forceinline__ float block_sum(float v, float* s_red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

struct PlanesArgs {
    const void *dy, *tok;
    const float* alpha;
    void *d_tok, *d_base;
    float *colsum, *dot;           // workspace partials (NULL: not formed)
    int64_t S;
    int C, p_tiles, c_tiles, walk, p_groups;
};

template <typename T>
__global__ __launch_bounds__(256) void planes_tail_backward_kernel(PlanesArgs a) {
    constexpr int V = 8, VPR = kTile / V, kIt = kTile * VPR / 256;      // 8 vectors per tile row, 2 pieces per thread and phase
    __shared__ float s_t[kTile][kTile + 1];                              // [c][p], zero outside the tensor
    __shared__ float s_red[4];
    const T* __restrict__ dy = (const T*)a.dy;
    const T* __restrict__ tok = (const T*)a.tok;
    T* __restrict__ d_tok = (T*)a.d_tok;
    T* __restrict__ d_base = (T*)a.d_base;
    int bid = blockIdx.x;
    const int pg = bid % a.p_groups; bid /= a.p_groups;
    const int ct = bid % a.c_tiles;
    const int64_t n = bid / a.c_tiles;
    const int c0 = ct * kTile;
    const int C = a.C;
    const int64_t S = a.S;
    const float wgt = a.alpha ? 1.0f - a.alpha[n] : 1.0f;
    const bool want_dot = a.dot != nullptr;
    float col[kIt] = {0.f, 0.f};                 // the column sums of this thread's two channels, over the walked tiles
    float dot = 0.f;
    const int pt_end = min((pg + 1) * a.walk, a.p_tiles);
    for (int pt = pg * a.walk; pt < pt_end; ++pt) {
        const int64_t p0 = (int64_t)pt * kTile;
        // every load of the tile is issued before the first use, from an address clamped into the tensor (token_rows.hip)
        uint4 ry[kIt], rk[kIt];
#pragma unroll
        for (int it = 0; it < kIt; ++it) {
            const int i = threadIdx.x + 256 * it, cr = i / VPR, pv = i % VPR;
            const bool ok = c0 + cr < C && p0 + pv * V < S;
            ry[it] = *reinterpret_cast<const uint4*>(dy + (ok ? (n * C + c0 + cr) * S + p0 + pv * V : n * C * S));
        }
        if (want_dot) {
#pragma unroll
            for (int it = 0; it < kIt; ++it) {
                const int i = threadIdx.x + 256 * it, pr = i / VPR, cv = i % VPR;
                const bool ok = p0 + pr < S && c0 + cv * V < C;
                rk[it] = *reinterpret_cast<const uint4*>(tok + (ok ? (n * S + p0 + pr) * C + c0 + cv * V : n * S * C));
            }
        }
        if (pt != pg * a.walk) __syncthreads();                          // the previous tile's reads of s_t are done
#pragma unroll
        for (int it = 0; it < kIt; ++it) {
            const int i = threadIdx.x + 256 * it, cr = i / VPR, pv = i % VPR;
            const bool ok = c0 + cr < C && p0 + pv * V < S;
            float t[V];
            Io<T>::load(reinterpret_cast<const T*>(&ry[it]), t);
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                t[k] = ok ? t[k] : 0.f;
                s_t[cr][pv * V + k] = t[k];
                s += t[k];
            }
            // the eight lanes that share channel cr (consecutive lanes of one wave) add their pieces
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            s += __shfl_xor(s, 4);
            col[it] += s;
        }
        __syncthreads();
        float part = 0.f;
#pragma unroll
        for (int it = 0; it < kIt; ++it) {
            const int i = threadIdx.x + 256 * it, pr = i / VPR, cv = i % VPR;
            const int64_t p = p0 + pr;
            const bool ok = p < S && c0 + cv * V < C;
            float t[V];
#pragma unroll
            for (int k = 0; k < V; ++k) t[k] = s_t[cv * V + k][pr];
            if (want_dot) {
                float kk[V];
                Io<T>::load(reinterpret_cast<const T*>(&rk[it]), kk);
#pragma unroll
                for (int k = 0; k < V; ++k) part += ok ? t[k] * kk[k] : 0.f;
            }
            if (ok) {
                const int64_t o = (n * S + p) * C + c0 + cv * V;
                if (d_base) Io<T>::store(d_base + o, t);                 // dy itself: the conversion back is exact
                if (d_tok) {
#pragma unroll
                    for (int k = 0; k < V; ++k) t[k] = wgt * t[k];       // one fp32 multiply, rounded once by the store
                    Io<T>::store(d_tok + o, t);
                }
            }
        }
        if (want_dot) {
            const float tile = block_sum(part, s_red);                   // (its barrier also orders s_red against the next tile's)
            dot += tile;
        }
    }
    if (a.colsum) {
#pragma unroll
        for (int it = 0; it < kIt; ++it) {
            const int i = threadIdx.x + 256 * it, cr = i / VPR, pv = i % VPR;
            if (pv == 0 && c0 + cr < C) a.colsum[(n * a.p_groups + pg) * C + c0 + cr] = col[it];
        }
    }
    if (want_dot && threadIdx.x == 0) a.dot[(n * a.p_groups + pg) * a.c_tiles + ct] = dot;
}

struct RowsArgs {
    const void *dy, *x, *h, *base;
    const float* alpha;
    void *d_t, *d_base;
    float* part;                   // [G * blocks_per_group] or NULL
    int64_t group_vec;             // 16-byte vectors of a group: row_div * C / 8
    int blocks_per_group;
};

template <typename T>
__global__ __launch_bounds__(256) void rows_tail_backward_kernel(RowsArgs a) {
    constexpr int V = 8, U = kRowsVec;
    __shared__ float s_red[4];
    const T* __restrict__ dy = (const T*)a.dy;
    const T* __restrict__ x = (const T*)a.x;
    const T* __restrict__ h = (const T*)a.h;
    const T* __restrict__ base = (const T*)a.base;
    T* __restrict__ d_t = (T*)a.d_t;
    T* __restrict__ d_base = (T*)a.d_base;
    const int64_t g = blockIdx.x / a.blocks_per_group;
    const int b = blockIdx.x % a.blocks_per_group;
    const float al = a.alpha[g], om = 1.0f - al;
    const int64_t g0 = g * a.group_vec;                                  // first vector of the group
    const bool want_part = a.part != nullptr;
    // all loads first, from an address clamped into the group
    uint4 ry[U], rx[U], rh[U], rb[U];
    int64_t idx[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t i = ((int64_t)b * U + u) * 256 + threadIdx.x;
        idx[u] = i < a.group_vec ? g0 + i : -1;
        const int64_t o = (i < a.group_vec ? g0 + i : g0) * V;
        ry[u] = *reinterpret_cast<const uint4*>(dy + o);
        if (want_part) {
            rx[u] = *reinterpret_cast<const uint4*>(x + o);
            rb[u] = *reinterpret_cast<const uint4*>(base + o);
            if (h) rh[u] = *reinterpret_cast<const uint4*>(h + o);
        }
    }
    float part = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const bool ok = idx[u] >= 0;
        float d[V];
        Io<T>::load(reinterpret_cast<const T*>(&ry[u]), d);
        if (want_part) {
            float xv[V], bv[V];
            Io<T>::load(reinterpret_cast<const T*>(&rx[u]), xv);
            Io<T>::load(reinterpret_cast<const T*>(&rb[u]), bv);
            if (h) {
                float hv[V];
                Io<T>::load(reinterpret_cast<const T*>(&rh[u]), hv);
#pragma unroll
                for (int k = 0; k < V; ++k) xv[k] = round_to<T>(xv[k] + hv[k]);       // the forward's own t
            }
#pragma unroll
            for (int k = 0; k < V; ++k) part += ok ? d[k] * (bv[k] - xv[k]) : 0.f;
        }
        if (ok) {
            float o[V];
            if (d_t) {
#pragma unroll
                for (int k = 0; k < V; ++k) o[k] = om * d[k];
                Io<T>::store(d_t + idx[u] * V, o);
            }
            if (d_base) {
#pragma unroll
                for (int k = 0; k < V; ++k) o[k] = al * d[k];
                Io<T>::store(d_base + idx[u] * V, o);
            }
        }
    }
    if (want_part) {
        const float s = block_sum(part, s_red);
        if (threadIdx.x == 0) a.part[blockIdx.x] = s;
    }
}

// Blocks [0, bias_blocks): dbias of kRedCh channels each. The samples are dealt to kRedSeg segments (n = seg, seg + kRedSeg, ...): a
// segment adds w_n sum_pg colsum[n, pg, c] over its samples in index order, the segments are then added in order — a thread per
// channel alone is a chain of N p_groups dependent loads (measured: 62 - 126 us at the training shapes, twice the pass itself).
// Blocks behind: one per sample (planes) or group (rows), the threads take the terms in strides of 256 and block_sum adds them.
// Every order is fixed by the shape.
constexpr int kRedCh = 32, kRedSeg = 8;

struct ReduceArgs {
    const float *colsum, *dot, *alpha, *bias, *part;
    float *dbias, *dalpha;
    int64_t N;                    // samples, or groups of the row pass
    int C, p_groups, c_tiles, bias_blocks, blocks_per_group;
};

__global__ __launch_bounds__(256) void tails_reduce_kernel(ReduceArgs a) {
    __shared__ float s_red[4];
    __shared__ float s_seg[kRedSeg][kRedCh];
    if ((int)blockIdx.x < a.bias_blocks) {
        const int cl = threadIdx.x % kRedCh, seg = threadIdx.x / kRedCh;
        const int c = blockIdx.x * kRedCh + cl;
        float acc = 0.f;
        if (c < a.C) {
            for (int64_t n = seg; n < a.N; n += kRedSeg) {
                float s = 0.f;
                const float* p = a.colsum + n * a.p_groups * a.C + c;
                for (int pg = 0; pg < a.p_groups; ++pg) s += p[(int64_t)pg * a.C];
                acc += a.alpha ? (1.0f - a.alpha[n]) * s : s;
            }
        }
        s_seg[seg][cl] = acc;
        __syncthreads();
        if (seg == 0 && c < a.C) {
            float t = s_seg[0][cl];
#pragma unroll
            for (int k = 1; k < kRedSeg; ++k) t += s_seg[k][cl];
            a.dbias[c] = t;
        }
        return;
    }
    const int64_t n = blockIdx.x - a.bias_blocks;
    float v = 0.f;
    if (a.part) {                                                        // rows: the group's partials
        const float* p = a.part + n * a.blocks_per_group;
        for (int i = threadIdx.x; i < a.blocks_per_group; i += 256) v += p[i];
        const float s = block_sum(v, s_red);
        if (threadIdx.x == 0) a.dalpha[n] = s;
        return;
    }
    const int n_dot = a.p_groups * a.c_tiles;
    const float* d = a.dot + n * n_dot;
    for (int i = threadIdx.x; i < n_dot; i += 256) v += d[i];
    if (a.bias) {
        for (int c = threadIdx.x; c < a.C; c += 256) {
            float s = 0.f;
            const float* p = a.colsum + n * a.p_groups * a.C + c;
            for (int pg = 0; pg < a.p_groups; ++pg) s += p[(int64_t)pg * a.C];
            v += a.bias[c] * s;
        }
    }
    const float s = block_sum(v, s_red);
    if (threadIdx.x == 0) a.dalpha[n] = -s;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

static bool planes_shape_ok(int64_t N, int32_t C, int64_t S) { return N >= 0 && C > 0 && S >= 0 && C % 8 == 0 && S % 8 == 0; }

static size_t planes_ws_bytes(int64_t N, int32_t C, int64_t S, int32_t flags) {
    if (!planes_shape_ok(N, C, S) || N == 0 || S == 0) return 0;
    const PlanesGeom g = planes_geom(C, S);
    size_t n = 0;
    if (flags & (MVI_TAILS_DBIAS | MVI_TAILS_DALPHA)) n += (size_t)N * g.p_groups * C * sizeof(float);
    if (flags & MVI_TAILS_DALPHA) n += (size_t)N * g.p_groups * g.c_tiles * sizeof(float);
    return n;
}

static int64_t rows_blocks_per_group(int64_t row_div, int32_t C) {
    const int64_t gv = row_div * (C / 8);
    return (gv + kRowsBlockVec - 1) / kRowsBlockVec;
}

}  // namespace tails
}  // namespace mvi

using namespace mvi;
using namespace mvi::tails;

extern "C" int mvi_block_tails_backward_supported(int32_t C, int64_t S, int32_t dtype) {
    return (dtype == MVI_DT_BF16 || dtype == MVI_DT_F16) && C > 0 && S >= 0 && C % 8 == 0 && S % 8 == 0;
}

extern "C" void mvi_planes_tail_backward_set_walk(int32_t walk) { g_walk_override = walk > 0 ? walk : 0; }

extern "C" int32_t mvi_planes_tail_backward_walk(int64_t S) { return S > 0 ? walk_of(S) : 1; }

extern "C" size_t mvi_planes_tail_backward_workspace_bytes(int64_t N, int32_t C, int64_t S, int32_t flags) {
    return planes_ws_bytes(N, C, S, flags);
}

extern "C" int mvi_planes_tail_backward(const void* dy, const float* alpha, const void* tok, void* d_tok, void* d_base, int32_t sums,
                                        void* workspace, size_t workspace_bytes, int64_t N, int32_t C, int64_t S, int32_t dtype,
                                        void* stream) {
    if (dtype != MVI_DT_BF16 && dtype != MVI_DT_F16) return unet_fail(MVI_EINVAL, "planes_tail_backward: bf16 or f16 expected");
    if (!planes_shape_ok(N, C, S)) return unet_fail(MVI_EINVAL, "planes_tail_backward: C and S must be multiples of 8 (C positive)");
    const bool want_da = (sums & MVI_TAILS_DALPHA) != 0;
    if (!dy || (d_base && !alpha) || (want_da && (!alpha || !tok)))
        return unet_fail(MVI_EINVAL, "planes_tail_backward: NULL pointer (dy; alpha for d_base; alpha and tok for dalpha)");
    if (!aligned16(dy) || !aligned16(tok) || !aligned16(d_tok) || !aligned16(d_base) || !aligned16(workspace) || !aligned4(alpha))
        return unet_fail(MVI_EINVAL, "planes_tail_backward: tensors and workspace must be 16-byte aligned, alpha 4-byte");
    const size_t need = planes_ws_bytes(N, C, S, sums);
    if (need && (!workspace || workspace_bytes < need))
        return unet_fail(MVI_EINVAL, "planes_tail_backward: workspace shorter than mvi_planes_tail_backward_workspace_bytes");
    const PlanesGeom g = planes_geom(C, S);
    const int64_t blocks = N * g.c_tiles * g.p_groups;
    if (blocks > 0x7FFFFFFFll) return unet_fail(MVI_EINVAL, "planes_tail_backward: too many blocks for one launch");
    if (N == 0 || S == 0 || !(d_tok || d_base || need)) return MVI_OK;
    float* colsum = need ? (float*)workspace : nullptr;
    float* dot = want_da ? colsum + (size_t)N * g.p_groups * C : nullptr;
    PlanesArgs a{dy, want_da ? tok : nullptr, alpha, d_tok, d_base, colsum, dot, S, C, g.p_tiles, g.c_tiles, g.walk, g.p_groups};
    return dispatch_dtype16(dtype, "planes_tail_backward: unknown dtype", [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((planes_tail_backward_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
        return hipGetLastError() == hipSuccess ? MVI_OK : unet_fail(MVI_EHIP, "planes_tail_backward: kernel launch failed");
    });
}

extern "C" int mvi_planes_tail_reduce(const void* workspace, size_t workspace_bytes, const float* alpha, const float* bias, float* dbias,
                                      float* dalpha, int64_t N, int32_t C, int64_t S, void* stream) {
    if (!planes_shape_ok(N, C, S)) return unet_fail(MVI_EINVAL, "planes_tail_reduce: C and S must be multiples of 8 (C positive)");
    if (!dbias && !dalpha) return unet_fail(MVI_EINVAL, "planes_tail_reduce: NULL pointer (dbias or dalpha)");
    if (!aligned16(workspace) || !aligned4(alpha) || !aligned4(bias) || !aligned4(dbias) || !aligned4(dalpha))
        return unet_fail(MVI_EINVAL, "planes_tail_reduce: workspace must be 16-byte aligned, fp32 vectors 4-byte");
    const size_t need = planes_ws_bytes(N, C, S, (dbias ? MVI_TAILS_DBIAS : 0) | (dalpha ? MVI_TAILS_DALPHA : 0));
    if (need && (!workspace || workspace_bytes < need))
        return unet_fail(MVI_EINVAL, "planes_tail_reduce: workspace shorter than mvi_planes_tail_backward_workspace_bytes");
    const int64_t bias_blocks = dbias ? (C + kRedCh - 1) / kRedCh : 0;
    if (bias_blocks + N > 0x7FFFFFFFll) return unet_fail(MVI_EINVAL, "planes_tail_reduce: too many blocks for one launch");
    hipStream_t st = (hipStream_t)stream;
    if (N == 0 || S == 0) {                                              // the sums are empty
        if (dbias && hipMemsetAsync(dbias, 0, (size_t)C * sizeof(float), st) != hipSuccess) return unet_fail(MVI_EHIP, "planes_tail_reduce: memset failed");
        if (dalpha && N && hipMemsetAsync(dalpha, 0, (size_t)N * sizeof(float), st) != hipSuccess) return unet_fail(MVI_EHIP, "planes_tail_reduce: memset failed");
        return MVI_OK;
    }
    const PlanesGeom g = planes_geom(C, S);
    const float* colsum = (const float*)workspace;
    ReduceArgs r{colsum, dalpha ? colsum + (size_t)N * g.p_groups * C : nullptr, alpha, bias, nullptr, dbias, dalpha, N, C, g.p_groups, g.c_tiles,
                 (int)bias_blocks, 0};
    hipLaunchKernelGGL(tails_reduce_kernel, dim3((unsigned)(bias_blocks + (dalpha ? N : 0))), dim3(256), 0, st, r);
    return hipGetLastError() == hipSuccess ? MVI_OK : unet_fail(MVI_EHIP, "planes_tail_reduce: kernel launch failed");
}

extern "C" int64_t mvi_rows_tail_backward_blocks_per_group(int64_t row_div, int32_t C) {
    return row_div > 0 && C > 0 && C % 8 == 0 ? rows_blocks_per_group(row_div, C) : 0;
}

extern "C" size_t mvi_rows_tail_backward_workspace_bytes(int64_t R, int32_t C, int64_t row_div, int32_t flags) {
    if (R <= 0 || C <= 0 || C % 8 || row_div <= 0 || R % row_div || !(flags & MVI_TAILS_DALPHA)) return 0;
    return (size_t)(R / row_div) * (size_t)rows_blocks_per_group(row_div, C) * sizeof(float);
}

extern "C" int mvi_rows_tail_backward(const void* dy, const float* alpha, const void* x, const void* h, const void* base, void* d_t,
                                      void* d_base, int32_t sums, void* workspace, size_t workspace_bytes, int64_t R, int32_t C,
                                      int64_t row_div, int32_t dtype, void* stream) {
    if (dtype != MVI_DT_BF16 && dtype != MVI_DT_F16) return unet_fail(MVI_EINVAL, "rows_tail_backward: bf16 or f16 expected");
    if (R < 0 || C <= 0 || C % 8) return unet_fail(MVI_EINVAL, "rows_tail_backward: C must be a positive multiple of 8");
    if (row_div <= 0 || R % row_div) return unet_fail(MVI_EINVAL, "rows_tail_backward: the rows must split into runs of row_div");
    const bool want_da = (sums & MVI_TAILS_DALPHA) != 0;
    if (!dy || !alpha || (want_da && (!x || !base))) return unet_fail(MVI_EINVAL, "rows_tail_backward: NULL pointer (dy, alpha; x and base for dalpha)");
    if (!aligned16(dy) || !aligned16(x) || !aligned16(h) || !aligned16(base) || !aligned16(d_t) || !aligned16(d_base) || !aligned16(workspace)
            || !aligned4(alpha))
        return unet_fail(MVI_EINVAL, "rows_tail_backward: tensors and workspace must be 16-byte aligned, alpha 4-byte");
    const size_t need = mvi_rows_tail_backward_workspace_bytes(R, C, row_div, sums);
    if (need && (!workspace || workspace_bytes < need))
        return unet_fail(MVI_EINVAL, "rows_tail_backward: workspace shorter than mvi_rows_tail_backward_workspace_bytes");
    const int64_t G = R / row_div, bpg = rows_blocks_per_group(row_div, C);
    if (bpg > 0x7FFFFFFFll || G * bpg > 0x7FFFFFFFll) return unet_fail(MVI_EINVAL, "rows_tail_backward: too many blocks for one launch");
    if (R == 0 || !(d_t || d_base || want_da)) return MVI_OK;
    RowsArgs a{dy, want_da ? x : nullptr, want_da ? h : nullptr, want_da ? base : nullptr, alpha, d_t, d_base, want_da ? (float*)workspace : nullptr,
               row_div * (C / 8), (int)bpg};
    return dispatch_dtype16(dtype, "rows_tail_backward: unknown dtype", [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((rows_tail_backward_kernel<T>), dim3((unsigned)(G * bpg)), dim3(256), 0, (hipStream_t)stream, a);
        return hipGetLastError() == hipSuccess ? MVI_OK : unet_fail(MVI_EHIP, "rows_tail_backward: kernel launch failed");
    });
}

extern "C" int mvi_rows_tail_reduce(const void* workspace, size_t workspace_bytes, float* dalpha, int64_t R, int32_t C, int64_t row_div,
                                    void* stream) {
    if (R < 0 || C <= 0 || C % 8) return unet_fail(MVI_EINVAL, "rows_tail_reduce: C must be a positive multiple of 8");
    if (row_div <= 0 || R % row_div) return unet_fail(MVI_EINVAL, "rows_tail_reduce: the rows must split into runs of row_div");
    if (!dalpha) return unet_fail(MVI_EINVAL, "rows_tail_reduce: NULL pointer (dalpha)");
    if (!aligned16(workspace) || !aligned4(dalpha)) return unet_fail(MVI_EINVAL, "rows_tail_reduce: workspace must be 16-byte aligned, dalpha 4-byte");
    const size_t need = mvi_rows_tail_backward_workspace_bytes(R, C, row_div, MVI_TAILS_DALPHA);
    if (need && (!workspace || workspace_bytes < need))
        return unet_fail(MVI_EINVAL, "rows_tail_reduce: workspace shorter than mvi_rows_tail_backward_workspace_bytes");
    const int64_t G = R / row_div, bpg = rows_blocks_per_group(row_div, C);
    if (bpg > 0x7FFFFFFFll || G > 0x7FFFFFFFll) return unet_fail(MVI_EINVAL, "rows_tail_reduce: too many blocks for one launch");
    if (R == 0) return MVI_OK;                                           // no group, so no sum to write
    ReduceArgs r{nullptr, nullptr, nullptr, nullptr, (const float*)workspace, nullptr, dalpha, G, C, 0, 0, 0, (int)bpg};
    hipLaunchKernelGGL(tails_reduce_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, r);
    return hipGetLastError() == hipSuccess ? MVI_OK : unet_fail(MVI_EHIP, "rows_tail_reduce: kernel launch failed");
}
