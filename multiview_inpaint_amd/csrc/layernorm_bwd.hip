// Backward of add_layernorm (token_rows.hip) for gfx950 — HBM-bound, deterministic (no atomics), one pass over the tensors.
// Differentiates the residual add(s) + LayerNorm chains of the reference's transformer blocks under training
// (svd_inpaint1/sgm/modules/attention.py:544-572, video_attention.py:110-141, :278-296):
//
//   forward : s_pre = x + h,  s = s_pre + row[r / row_div],  y = LayerNorm(s) * w + b        outputs y, s, s_pre
//   given   : s (the forward's rounded sum; x itself when there is neither h nor row), w, and the gradients gy, gs, gs_pre of the
//             three outputs (each may be absent)
//   per row : mean, rstd recomputed from s exactly as add_layernorm_kernel computes them (the forward's bits, no table stored)
//             xh = (s - mean) rstd,  t = gy w,  c1 = mean_c(t xh),  c2 = mean_c(t)
//             gS = rstd (t - c2 - xh c1) + gs            the whole gradient of s
//             gP = gS + gs_pre                           the whole gradient of s_pre: dx = dh = gP, ONE tensor, rounded once
//   columns : drow[g] = sum of the UNROUNDED gS over the rows of run g;  dweight = sum_r gy xh;  dbias = sum_r gy     (fp32)
//
// Row layout and L / K search of add_layernorm: a row is L = 2^k lanes x K <= 8 16-byte vectors, a block holds 256 / L rows per
// pass. A block owns a slab of consecutive rows INSIDE one run of `row` (blocks are dealt per run, the tail rows of a slab are
// masked), walks it pass by pass and keeps the column partials of its lanes in registers; at the end the 256 / L row groups are
// added through LDS in group order and the block writes one fp32 partial row per sum into the workspace [sum][block][C]. The
// finalize launch adds the partial rows in a fixed order: all blocks for dweight / dbias, the blocks of run g for drow[g]. Every
// output element is therefore a fixed sequence of additions. row_div = 1 (one row per run) needs no sum: the kernel stores gS.
// The kernels are instantiated per set of requested outputs (gP store, parameter sums, drow sums), so a gradient nobody needs
// costs neither arithmetic nor registers nor traffic.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "unet_host.h"
#include "unet_io.h"

namespace mvi {

constexpr int kLnbTargetBlocks = 512;       // two 256-thread blocks per CU: what the register budget of the K = 5 kernels allows
constexpr int kLnbFinCols = 32;             // finalize: 32 columns x 8 segments of the partial rows per block
constexpr int kLnbFinSegs = 8;

struct LnbArgs {
    const void *gy, *s, *gs, *gsp;
    const float* w;
    void* g_out;
    float* drow_direct;                      // row_div == 1: gS itself, fp32 [R, C]
    float* part;                             // [sums][blocks][C]
    int64_t R, run_len, slab_rows, blocks;
    int nb;                                  // blocks per run
    int C, L, log2L;
    float eps;
};

// Two waves per SIMD (256 registers) are asked of the compiler while the column partials take at most 40 of them: at K = 5 in bf16 /
// f16 (every width of the networks) that is the frozen norm (no parameter sums). With parameter sums (80 partials, 120 with drow)
// the compiler needs 260 - 340 registers and the instance runs one wave per SIMD, without scratch.
template <typename T, int K, bool GP, bool PAR, bool DROW>
__global__ __launch_bounds__(256, (K * Io<T>::kVec * ((PAR ? 2 : 0) + (DROW ? 1 : 0)) <= 40 ? 2 : 1))
void add_layernorm_bwd_kernel(LnbArgs a) {
    constexpr int V = Io<T>::kVec;
    constexpr bool kInputGrad = GP || DROW;                  // c1, c2 and gS are needed
    // the image of the end reduction [256 / L groups][C]; until then its first C floats hold the norm's weight
    __shared__ __attribute__((aligned(16))) float s_red[(PAR || DROW) ? 256 * K * V : 64 * K * V];
    const int L = a.L, C = a.C;
    const int li = threadIdx.x & (L - 1), grp = threadIdx.x >> a.log2L, P = 256 >> a.log2L;
    const int64_t run = blockIdx.x / a.nb;
    const int64_t run_end = (run + 1) * a.run_len;
    const int64_t r0 = run * a.run_len + (int64_t)(blockIdx.x % a.nb) * a.slab_rows;
    const int64_t r1 = r0 + a.slab_rows < run_end ? r0 + a.slab_rows : run_end;
    const float inv_c = 1.0f / (float)C;
    float acc_w[PAR ? K : 1][V], acc_b[PAR ? K : 1][V], acc_r[DROW ? K : 1][V];
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if constexpr (PAR) { acc_w[j][k] = 0.f; acc_b[j][k] = 0.f; }
            if constexpr (DROW) acc_r[j][k] = 0.f;
        }
    if constexpr (kInputGrad) {
        for (int c = threadIdx.x; c < C; c += 256) s_red[c] = a.w[c];
        __syncthreads();
    }
    for (int64_t rb = r0; rb < r1; rb += P) {                // the same trip count for every thread of the block
        const int64_t r = rb + grp;
        if (r >= r1) continue;                               // rows are L-lane aligned: an L-group skips together
        const int64_t base = r * C;
        const T* ps = (const T*)a.s + base;
        const T* pgy = a.gy ? (const T*)a.gy + base : nullptr;
        const T* pgs = (kInputGrad && a.gs) ? (const T*)a.gs + base : nullptr;
        const T* pgp = (GP && a.gsp) ? (const T*)a.gsp + base : nullptr;
        // every load of the row is issued before anything is used (one memory latency per row, not one per piece: token_rows.hip);
        // the 16-byte pieces stay packed until they are used, and gy w is formed twice from the packed gy rather than kept
        uint4 rs[K], rg[K], rgs[K], rgp[K];
#pragma unroll
        for (int j = 0; j < K; ++j) rs[j] = *reinterpret_cast<const uint4*>(ps + (j * L + li) * V);
        // (an absent gradient is a row of zero bits: the arithmetic below has no branches, x + 0 is x)
#pragma unroll
        for (int j = 0; j < K; ++j) rg[j] = pgy ? *reinterpret_cast<const uint4*>(pgy + (j * L + li) * V) : make_uint4(0, 0, 0, 0);
        if constexpr (kInputGrad) {
#pragma unroll
            for (int j = 0; j < K; ++j) rgs[j] = pgs ? *reinterpret_cast<const uint4*>(pgs + (j * L + li) * V) : make_uint4(0, 0, 0, 0);
        }
        if constexpr (GP) {
#pragma unroll
            for (int j = 0; j < K; ++j) rgp[j] = pgp ? *reinterpret_cast<const uint4*>(pgp + (j * L + li) * V) : make_uint4(0, 0, 0, 0);
        }
        // The row stays in its packed 16-byte pieces; each phase below expands a piece again where it needs it (a shift or a convert
        // per element) instead of holding the row in fp32, which together with the column partials would cost the second wave per
        // SIMD. The empty asm keeps the compiler from merging the expansions of two phases back into one long-lived copy (and, on
        // the LDS offset of the weight, from keeping the weight in registers across phases and passes).
        auto expand = [&](uint4& r, float* o) {
            if constexpr (sizeof(T) == 2) asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(r.z), "+v"(r.w));
            Io<T>::load(reinterpret_cast<const T*>(&r), o);
        };
        auto gy_times_w = [&](int j, int woff, float* g, float* t) {     // g <- gy, t <- gy w of vector j
            expand(rg[j], g);
#pragma unroll
            for (int k = 0; k < V; k += 4) {
                const float4 w = *reinterpret_cast<const float4*>(&s_red[j * L * V + woff + k]);
                t[k] = g[k] * w.x; t[k + 1] = g[k + 1] * w.y; t[k + 2] = g[k + 2] * w.z; t[k + 3] = g[k + 3] * w.w;
            }
        };
        // statistics: the forward's order of operations (sum, then the centred sum of squares, xor shuffles over the L lanes)
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            float x[V];
            expand(rs[j], x);
#pragma unroll
            for (int k = 0; k < V; ++k) sum += x[k];
        }
        for (int o = 1; o < L; o <<= 1) sum += __shfl_xor(sum, o);
        const float mean = sum / (float)C;
        float m2 = 0.f;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            float x[V];
            expand(rs[j], x);
#pragma unroll
            for (int k = 0; k < V; ++k) { const float d = x[k] - mean; m2 += d * d; }
        }
        for (int o = 1; o < L; o <<= 1) m2 += __shfl_xor(m2, o);
        const float rstd = rsqrtf(m2 / (float)C + a.eps);
        // the parameter sums; the two row means of t = gy w
        float c1 = 0.f, c2 = 0.f;
        int woff = li * V;
        asm volatile("" : "+v"(woff));
#pragma unroll
        for (int j = 0; j < K; ++j) {
            float x[V], g[V], t[V];
            expand(rs[j], x);
            if constexpr (kInputGrad) gy_times_w(j, woff, g, t);
            else expand(rg[j], g);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float xh = (x[k] - mean) * rstd;
                if constexpr (PAR) { acc_w[j][k] += g[k] * xh; acc_b[j][k] += g[k]; }
                if constexpr (kInputGrad) { c1 += t[k] * xh; c2 += t[k]; }
            }
        }
        if constexpr (kInputGrad) {
            for (int o = 1; o < L; o <<= 1) { c1 += __shfl_xor(c1, o); c2 += __shfl_xor(c2, o); }
            c1 *= inv_c; c2 *= inv_c;
            asm volatile("" : "+v"(woff));
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const int e = (j * L + li) * V;
                float x[V], g[V], gS[V];
                expand(rs[j], x);
                float u[V];
                gy_times_w(j, woff, g, gS);
                expand(rgs[j], u);
#pragma unroll
                for (int k = 0; k < V; ++k) gS[k] = rstd * (gS[k] - c2 - (x[k] - mean) * rstd * c1) + u[k];
                if constexpr (DROW) {
                    if (a.drow_direct) {
#pragma unroll
                        for (int k = 0; k < V; k += 4)
                            *reinterpret_cast<float4*>(a.drow_direct + base + e + k) = make_float4(gS[k], gS[k + 1], gS[k + 2], gS[k + 3]);
                    } else {
#pragma unroll
                        for (int k = 0; k < V; ++k) acc_r[j][k] += gS[k];
                    }
                }
                if constexpr (GP) {
                    expand(rgp[j], u);
#pragma unroll
                    for (int k = 0; k < V; ++k) gS[k] += u[k];
                    Io<T>::store((T*)a.g_out + base + e, gS);
                }
            }
        }
    }
    // the block's 256 / L row groups, added in group order: thread c sums column c down the LDS image [group][C]
    auto reduce = [&](float (&acc)[K][V], int plane) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int k = 0; k < V; k += 4)
                *reinterpret_cast<float4*>(&s_red[grp * C + (j * L + li) * V + k]) =
                    make_float4(acc[j][k], acc[j][k + 1], acc[j][k + 2], acc[j][k + 3]);
        __syncthreads();
        float* out = a.part + ((int64_t)plane * a.blocks + blockIdx.x) * C;
        for (int c = threadIdx.x; c < C; c += 256) {
            float x = 0.f;
            for (int g = 0; g < P; ++g) x += s_red[g * C + c];
            out[c] = x;
        }
    };
    if constexpr (PAR) { reduce(acc_w, 0); reduce(acc_b, 1); }
    if constexpr (DROW) {
        if (!a.drow_direct) reduce(acc_r, PAR ? 2 : 0);
    }
}

// One block per (sum, 32 columns): sum 0 / 1 = dweight / dbias over all blocks (when `par`), then one sum per run over its nb blocks.
// The partial rows of a sum are cut into 8 consecutive segments, one per 32-lane half wave; a thread adds its segment in block order,
// the 8 segment sums are added in segment order.
__global__ __launch_bounds__(256) void add_layernorm_bwd_finalize_kernel(const float* __restrict__ part, int64_t blocks, int nb, int C,
                                                                         int cblocks, int par, float* __restrict__ dweight,
                                                                         float* __restrict__ dbias, float* __restrict__ drow) {
    __shared__ float s_seg[kLnbFinSegs][kLnbFinCols];
    int64_t sum_id = blockIdx.x / cblocks;
    const int c = (int)(blockIdx.x % cblocks) * kLnbFinCols + (threadIdx.x & (kLnbFinCols - 1));
    const int seg = threadIdx.x / kLnbFinCols;
    const float* p;
    float* out;
    int64_t n;
    if (par && sum_id < 2) {
        p = part + sum_id * blocks * C; n = blocks; out = sum_id == 0 ? dweight : dbias;
    } else {
        if (par) sum_id -= 2;
        p = part + ((par ? 2 : 0) * blocks + sum_id * nb) * C; n = nb; out = drow + sum_id * C;
    }
    if (!out) return;                                        // the whole block: only one of dweight / dbias was asked for
    const int64_t chunk = (n + kLnbFinSegs - 1) / kLnbFinSegs;
    const int64_t lo = seg * chunk, hi = lo + chunk < n ? lo + chunk : n;
    float x = 0.f;
    if (c < C)
        for (int64_t b = lo; b < hi; ++b) x += p[b * C + c];
    s_seg[seg][threadIdx.x & (kLnbFinCols - 1)] = x;
    __syncthreads();
    if (seg == 0 && c < C) {
        float y = s_seg[0][threadIdx.x];
#pragma unroll
        for (int q = 1; q < kLnbFinSegs; ++q) y += s_seg[q][threadIdx.x];
        out[c] = y;
    }
}

struct LnbPlan {
    int L, log2L, K;
    int64_t run_len, runs, slab_rows, nb, blocks;
    int sums;                                                // partial planes in the workspace: 2 with PAR, + 1 with summed drow
    bool direct;                                             // drow is gS itself
};

// flags: MVI_LNB_*; row_div <= 0 or no MVI_LNB_DROW: one run of R rows
static bool lnb_plan(int64_t R, int C, int64_t row_div, int flags, int V, LnbPlan* p) {
    if (R <= 0 || C <= 0 || C % V != 0) return false;
    const int vecs = C / V;
    int L = 1, log2L = 0;
    while (L <= 64 && (vecs % L != 0 || vecs / L > 8)) { L <<= 1; ++log2L; }
    if (L > 64) return false;
    p->L = L; p->log2L = log2L; p->K = vecs / L;
    const bool drow = (flags & MVI_LNB_DROW) != 0, par = (flags & MVI_LNB_PARAMS) != 0;
    p->direct = drow && row_div == 1;
    const bool runs = drow && !p->direct;
    if (runs && (row_div <= 0 || R % row_div != 0)) return false;
    p->run_len = runs ? row_div : R;
    p->runs = R / p->run_len;
    const int64_t P = 256 / L;
    const int64_t passes = (p->run_len + P - 1) / P;         // per run
    int64_t nb = (kLnbTargetBlocks + p->runs - 1) / p->runs;
    nb = nb < passes ? nb : passes;
    const int64_t slab_passes = (passes + nb - 1) / nb;
    p->slab_rows = slab_passes * P;
    p->nb = (p->run_len + p->slab_rows - 1) / p->slab_rows;
    p->blocks = p->runs * p->nb;
    p->sums = (par ? 2 : 0) + (runs ? 1 : 0);
    // grid limits of the two launches (the finalize launch has 2 + runs sums of ceil(C / 32) blocks)
    return p->blocks <= 0x7FFFFFFFll && (p->runs + 2) * ((C + kLnbFinCols - 1) / kLnbFinCols) <= 0x7FFFFFFFll;
}

template <typename T, int K>
static void lnb_launch_k(const LnbArgs& a, const LnbPlan& p, bool gp, bool par, bool drow, hipStream_t st) {
    const dim3 grid((unsigned)p.blocks), block(256);
#define MVI_LNB(G_, P_, D_) hipLaunchKernelGGL((add_layernorm_bwd_kernel<T, K, G_, P_, D_>), grid, block, 0, st, a)
    if (gp) {
        if (par) { if (drow) MVI_LNB(true, true, true); else MVI_LNB(true, true, false); }
        else { if (drow) MVI_LNB(true, false, true); else MVI_LNB(true, false, false); }
    } else {
        if (par) { if (drow) MVI_LNB(false, true, true); else MVI_LNB(false, true, false); }
        else if (drow) MVI_LNB(false, false, true);
    }
#undef MVI_LNB
}

template <typename T>
static int lnb_run(LnbArgs a, const LnbPlan& p, bool gp, bool par, bool drow, float* dweight, float* dbias, float* drow_out,
                   hipStream_t st) {
    switch (p.K) {
        case 1: lnb_launch_k<T, 1>(a, p, gp, par, drow, st); break;
        case 2: lnb_launch_k<T, 2>(a, p, gp, par, drow, st); break;
        case 3: lnb_launch_k<T, 3>(a, p, gp, par, drow, st); break;
        case 4: lnb_launch_k<T, 4>(a, p, gp, par, drow, st); break;
        case 5: lnb_launch_k<T, 5>(a, p, gp, par, drow, st); break;
        case 6: lnb_launch_k<T, 6>(a, p, gp, par, drow, st); break;
        case 7: lnb_launch_k<T, 7>(a, p, gp, par, drow, st); break;
        default: lnb_launch_k<T, 8>(a, p, gp, par, drow, st); break;
    }
    if (p.sums > 0) {
        const int cblocks = (a.C + kLnbFinCols - 1) / kLnbFinCols;
        const int64_t nsums = (par ? 2 : 0) + ((drow && !p.direct) ? p.runs : 0);
        hipLaunchKernelGGL(add_layernorm_bwd_finalize_kernel, dim3((unsigned)(nsums * cblocks)), dim3(256), 0, st, a.part, p.blocks,
                           (int)p.nb, a.C, cblocks, par ? 1 : 0, dweight, dbias, drow_out);
    }
    return hipGetLastError() == hipSuccess ? MVI_OK : MVI_EHIP;
}

}  // namespace mvi

extern "C" int mvi_add_layernorm_backward_supported(int32_t C, int32_t dtype) {
    return dtype >= MVI_DT_F32 && dtype <= MVI_DT_F16 && mvi_layernorm_supported(C, dtype);
}

extern "C" size_t mvi_add_layernorm_backward_workspace_bytes(int64_t R, int32_t C, int64_t row_div, int32_t flags) {
    mvi::LnbPlan p;
    // no dtype here: the larger of the plans of the two vector widths (4 fp32, 8 bf16 / f16 elements) serves every type
    size_t need = 0;
    for (int V = 4; V <= 8; V += 4) {
        if (!mvi::lnb_plan(R, C, row_div, flags, V, &p)) continue;
        const size_t n = (size_t)p.sums * (size_t)p.blocks * (size_t)C * sizeof(float);
        need = n > need ? n : need;
    }
    return need;
}

extern "C" int mvi_add_layernorm_backward(const void* gy, const void* s, const void* gs, const void* gs_pre, const float* weight,
                                          int64_t row_div, float eps, void* g_out, float* dweight, float* dbias, float* drow,
                                          void* workspace, size_t workspace_bytes, int64_t R, int32_t C, int32_t dtype, void* stream) {
    using namespace mvi;
    if (R < 0 || C <= 0) return unet_fail(MVI_EINVAL, "add_layernorm backward: bad shape");
    if (R == 0) return MVI_OK;
    if (!mvi_add_layernorm_backward_supported(C, dtype))
        return unet_fail(MVI_EINVAL, "add_layernorm backward: C must split into 2^k lanes x <= 8 16-byte vectors of fp32 / bf16 / f16");
    const bool gp = g_out != nullptr, par = dweight || dbias, dr = drow != nullptr;
    if (!gp && !par && !dr) return MVI_OK;
    if (!s || !weight) return unet_fail(MVI_EINVAL, "add_layernorm backward: NULL pointer");
    if (dr && (row_div <= 0 || R % row_div != 0)) return unet_fail(MVI_EINVAL, "add_layernorm backward: row_div must divide R");
    const int flags = (gp ? MVI_LNB_GRAD : 0) | (par ? MVI_LNB_PARAMS : 0) | (dr ? MVI_LNB_DROW : 0);
    LnbPlan p;
    if (!lnb_plan(R, C, row_div, flags, dtype == MVI_DT_F32 ? 4 : 8, &p)) return unet_fail(MVI_EINVAL, "add_layernorm backward: shape too large");
    const size_t need = (size_t)p.sums * (size_t)p.blocks * (size_t)C * sizeof(float);
    if (need && (!workspace || workspace_bytes < need || (uintptr_t)workspace % 16 != 0))
        return unet_fail(MVI_ENOMEM, "add_layernorm backward: workspace too small or misaligned");
    if ((((uintptr_t)gy | (uintptr_t)s | (uintptr_t)gs | (uintptr_t)gs_pre | (uintptr_t)g_out | (uintptr_t)weight | (uintptr_t)drow) % 16) != 0)
        return unet_fail(MVI_EINVAL, "add_layernorm backward: tensors must be 16-byte aligned");
    LnbArgs a{gy, s, gs, gs_pre, weight, g_out, p.direct ? drow : nullptr, (float*)workspace, R, p.run_len, p.slab_rows, p.blocks,
              (int)p.nb, C, p.L, p.log2L, eps};
    return dispatch_dtype(dtype, "add_layernorm backward: unknown dtype", [&](auto t) {     // (turned down above already)
        return lnb_run<typename decltype(t)::type>(a, p, gp, par, dr, dweight, dbias, drow, (hipStream_t)stream)
                   ? unet_fail(MVI_EHIP, "add_layernorm backward: kernel launch failed") : MVI_OK;
    });
}
