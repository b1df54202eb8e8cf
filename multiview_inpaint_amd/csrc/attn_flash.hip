// bf16/f16 MFMA flash attention (forward) for gfx950, head dim 64 — the only dense contraction of
// the SVD denoise loop that is hand-written (BASELINE.json north_star). Replaces
// xformers.ops.memory_efficient_attention / F.scaled_dot_product_attention
// (svd_inpaint1/sgm/modules/attention.py:427-439, :332-336) for the spatial self-attention calls:
// (B*H, S) = (140, 9216), (280, 2304), (560, 576), (560, 144) at 14 x 576x1024.
//
// Layout: q/out [B, Sq, H, 64], k/v [B, Sk, H, 64] token-major, contiguous.
// Block = 4 wave64 = 128 query rows of one (batch, head); each wave owns 32 rows. KV tile = 64 keys.
// Per wave and KV tile (v_mfma_f32_32x32x16, fp32 accumulate):
//   S^T[key][query] = K Q^T    : 2 key blocks x 4 d-steps  = 8 MFMA   (A = K rows from LDS, B = Q in regs)
//   online softmax in registers: the query sits on the lane (col = lane & 31), its 64 scores are 2 x 16
//                                registers in this lane and in lane ^ 32 -> one cross-lane max, no LDS
//   O^T[d][query]  += V^T P^T  : 2 d blocks x 4 key-steps   = 8 MFMA   (A = V^T from LDS, B = P from the
//                                S^T accumulators, converted in place: MFMA C/D layout == next B layout
//                                up to the fixed key permutation the V^T fragment read follows)
// K tile rows are padded to 72 elements (b128 reads conflict-free), V is stored transposed with a
// row of 68 elements (b64 reads conflict-free).
#include <type_traits>

#include "attn_launch.h"
#include "mfma_common.h"

namespace mvi {

constexpr int kFD = 64;          // head dim
constexpr int kFQ = 128;         // query rows per block
constexpr int kFK = 64;          // keys per tile
constexpr int kKStride = 72;     // elements per K row in LDS
constexpr int kVStride = 68;     // elements per V^T row in LDS

template <typename T> using Mma = MmaBuiltin32<T>;

// Forms measured in round 1 (micro-benchmark B28 H5 S9216 / B28 H10 S2304, bf16, TFLOP/s); only the first is built:
//   pipelined, 3 waves per SIMD (this file)         781 / 761     QK^T of tile t+1 issued under the softmax of tile t
//   not pipelined, 3 waves per SIMD                 768 / 738     one score accumulator, overlap left to the SIMD's other waves
//   not pipelined, 4 waves per SIMD                 783 / 744     ... with 128 VGPRs, 7 spilled
//   not pipelined, 3 waves, row sums on MFMAs       699 / 690     row sums as 4 extra MFMAs per tile instead of 33 v_add_f32
// The last line shows the matrix pipe is NOT idle enough to take 25 % more work: the loop is balanced between the two
// pipes at ~780 TFLOP/s, which is why removing VALU instructions alone (the first three lines) does not move it.
constexpr float kRescaleThreshold = 8.0f;   // log2 units: O and l are rescaled only when the row max grows by > 2^8

// Software pipeline: one wave keeps BOTH pipes busy. While the VALU runs the softmax of tile t (scores
// computed in the previous iteration), the matrix pipe runs S^T = K Q^T of tile t+1; the PV MFMAs of
// tile t follow as their P fragments come out of the converts (the compiler's own schedule of that
// single basic block spaces the 16 MFMAs ~8 VALU issues apart; sched_group_barrier hints made it worse).
// Measured and rejected: a 2x unrolled loop whose two score accumulators swap roles (removes the 16 v_mov_b64 of the
// loop latch) — 168 VGPRs + 43 spilled at 3 waves/SIMD: 597 TFLOP/s, 746 at 2 waves/SIMD, against 778 for this form.
// Costs a second score accumulator; 163 VGPRs, pinned to 3 waves/SIMD. The issue port, not the matrix
// pipe, bounds the loop at D = 64: 32 exp (8 cyc) + 32 fma + 32 add + 16 max3 + 16 cvt + 16 MFMA issue
// slots ~ 900 cycles per wave-tile against 512 matrix-pipe cycles. LDS holds K_{t+1} / K_{t+2} and V_t / V_{t+1}: two buffers each, one
// barrier per tile (K_{t+2} overwrites K_t, whose last reader finished before the previous barrier;
// V_{t+1} overwrites V_{t-1} likewise).
// kLse (the forward under autograd, mvi_attention_forward_lse): also writes the row's log-sum-exp of the scaled scores, fp32
// [B, H, Sq], for csrc/attn_bwd.hip; `out` is computed by the same instructions in the same order either way.
template <typename T, bool kLse>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void attn_flash_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                   const T* __restrict__ v, T* __restrict__ out, int H,
                                                                   int Sq, int Sk, float scale_log2e, int q_blocks,
                                                                   int total_blocks, int64_t q_rs, int64_t kv_rs,
                                                                   int64_t o_rs, float* __restrict__ lse) {
    using M = Mma<T>;
    using frag = typename M::frag;
    __shared__ __attribute__((aligned(16))) uint16_t s_k[2][kFK * kKStride];
    __shared__ __attribute__((aligned(16))) uint16_t s_vt[2][kFD * kVStride];

    int bid = blockIdx.x;
    if ((total_blocks & 7) == 0) bid = (bid & 7) * (total_blocks >> 3) + (bid >> 3);
    const int qb = bid % q_blocks;
    const int bh = bid / q_blocks;
    const int h = bh % H;
    const int64_t b = bh / H;
    // q_rs / kv_rs / o_rs: elements between consecutive tokens of q, of k and v, of out (H * 64 when contiguous;
    // 3 * H * 64 for q, k, v taken out of one packed projection)

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int qcol = lane & 31, hh = lane >> 5;
    const int q0 = qb * kFQ + wave * 32;
    const int qrow = q0 + qcol;

    frag qf[4];
    {
        const T* qp = q + ((b * Sq + (qrow < Sq ? qrow : 0)) * q_rs + (int64_t)h * kFD + 8 * hh);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            u32x4 raw = qrow < Sq ? *reinterpret_cast<const u32x4*>(qp + 16 * s) : u32x4{0, 0, 0, 0};
            qf[s] = as_frag<frag>(raw);
        }
    }
    f32x16 o[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) { o[0][i] = 0.f; o[1][i] = 0.f; }
    float m = -INFINITY, l = 0.f;

    const int kr = tid >> 2, ks = tid & 3;
    const int vp = tid >> 3, vs = tid & 7;
    const T* kbase = k + (b * Sk * kv_rs + (int64_t)h * kFD);
    const T* vbase = v + (b * Sk * kv_rs + (int64_t)h * kFD);
    u32x4 rk0, rk1, rv0, rv1;
    const u32x4 z4 = {0, 0, 0, 0};
    auto load_k = [&](int k0) {
        int r = k0 + kr;
        const T* p = kbase + (int64_t)r * kv_rs + 16 * ks;
        rk0 = r < Sk ? *reinterpret_cast<const u32x4*>(p) : z4;
        rk1 = r < Sk ? *reinterpret_cast<const u32x4*>(p + 8) : z4;
    };
    auto load_v = [&](int k0) {
        int r0 = k0 + 2 * vp;
        const T* pv = vbase + (int64_t)r0 * kv_rs + 8 * vs;
        rv0 = r0 < Sk ? *reinterpret_cast<const u32x4*>(pv) : z4;
        rv1 = r0 + 1 < Sk ? *reinterpret_cast<const u32x4*>(pv + kv_rs) : z4;
    };
    auto store_k = [&](int buf) {
        uint16_t* sk = s_k[buf];
        *reinterpret_cast<u32x4*>(&sk[kr * kKStride + 16 * ks]) = rk0;
        *reinterpret_cast<u32x4*>(&sk[kr * kKStride + 16 * ks + 8]) = rk1;
    };
    auto store_v = [&](int buf) {
        uint16_t* sv = s_vt[buf];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t a = rv0[i], c = rv1[i];
            uint32_t lo = (a & 0xFFFFu) | (c << 16), hi = (a >> 16) | (c & 0xFFFF0000u);
            *reinterpret_cast<uint32_t*>(&sv[(8 * vs + 2 * i) * kVStride + 2 * vp]) = lo;
            *reinterpret_cast<uint32_t*>(&sv[(8 * vs + 2 * i + 1) * kVStride + 2 * vp]) = hi;
        }
    };
    auto qk = [&](const uint16_t* sk, f32x16* st) {
        u32x4 kf[2][4];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int s = 0; s < 4; ++s)
                kf[kb][s] = *reinterpret_cast<const u32x4*>(&sk[(kb * 32 + qcol) * kKStride + 16 * s + 8 * hh]);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) st[kb][i] = 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) st[kb] = M::mfma(as_frag<frag>(kf[kb][s]), qf[s], st[kb]);
        }
    };

    const int n_tiles = (Sk + kFK - 1) / kFK;
    // prologue: K_0, V_0 -> buffers 0; K_1 -> buffer 1; scores of tile 0
    load_k(0); load_v(0);
    store_k(0); store_v(0);
    if (n_tiles > 1) { load_k(kFK); store_k(1); }
    __syncthreads();
    f32x16 st[2], sn[2];
    qk(s_k[0], st);

    auto tile = [&](int t, auto has_next_c) {
        constexpr bool kHasNext = decltype(has_next_c)::value;
        const int k0 = t * kFK;
        if (t + 2 < n_tiles) load_k((t + 2) * kFK);             // lands while this tile is processed
        if (kHasNext) load_v((t + 1) * kFK);
        // ---- row max of tile t, reference exponent (VALU only; rarely rescales)
        if (!kHasNext && k0 + kFK > Sk) {                       // only the last tile can be ragged
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if ((k0 + 32 * kb + (r & 3) + 8 * (r >> 2) + 4 * hh) >= Sk) st[kb][r] = -INFINITY;
        }
        float rmax = fmaxf(st[0][0], st[1][0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) rmax = fmaxf(rmax, fmaxf(st[0][r], st[1][r]));
        rmax = fmaxf(rmax, __shfl_xor(rmax, 32)) * scale_log2e;
        const bool grow = rmax > m + kRescaleThreshold;
        if (__ballot(grow) != 0ull) {
            const float m_new = grow ? rmax : m;
            const float alpha = __builtin_amdgcn_exp2f(m - m_new);
            l *= alpha;
#pragma unroll
            for (int i = 0; i < 16; ++i) { o[0][i] *= alpha; o[1][i] *= alpha; }
            m = m_new;
        }
        // ---- one scheduling region: QK^T of tile t+1 (matrix pipe) under exp/convert of tile t (VALU),
        //      then PV of tile t as its P fragments become available
        if (kHasNext) qk(s_k[(t + 1) & 1], sn);
        const uint16_t* sv = s_vt[t & 1];
        float rsum = 0.f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                u32x4 pr;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(st[kb][8 * s2 + 2 * i], scale_log2e, -m));
                    float p1 = __builtin_amdgcn_exp2f(__builtin_fmaf(st[kb][8 * s2 + 2 * i + 1], scale_log2e, -m));
                    rsum += p0 + p1;
                    pr[i] = M::pack2(p0, p1);
                }
                const frag pf = as_frag<frag>(pr);
                const int koff = 32 * kb + 16 * s2 + 4 * hh;
#pragma unroll
                for (int db = 0; db < 2; ++db) {
                    const uint16_t* row = &sv[(32 * db + qcol) * kVStride + koff];
                    u32x2 a0 = *reinterpret_cast<const u32x2*>(row);
                    u32x2 a1 = *reinterpret_cast<const u32x2*>(row + 8);
                    u32x4 av = {a0[0], a0[1], a1[0], a1[1]};
                    o[db] = M::mfma(as_frag<frag>(av), pf, o[db]);
                }
            }
        l += rsum;
        if (t + 2 < n_tiles) store_k(t & 1);                     // K_t is dead: its scores exist since the last iteration
        if (kHasNext) store_v((t + 1) & 1);                      // V_{t-1} is dead
        if (kHasNext) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 16; ++i) { st[0][i] = sn[0][i]; st[1][i] = sn[1][i]; }
        }
    };
    for (int t = 0; t + 1 < n_tiles; ++t) tile(t, std::true_type{});
    tile(n_tiles - 1, std::false_type{});
    l += __shfl_xor(l, 32);                                  // the two lane halves hold disjoint keys of every k-step
    if (kLse && qrow < Sq && hh == 0) lse[(b * H + h) * Sq + qrow] = (m + __builtin_amdgcn_logf(l)) * 0.6931471805599453f;   // m is in log2 units
    if (qrow < Sq) {
        const float inv = 1.0f / l;
        T* op = out + ((b * Sq + qrow) * o_rs + (int64_t)h * kFD);
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                u32x2 w = {M::pack2(o[db][4 * g] * inv, o[db][4 * g + 1] * inv),
                           M::pack2(o[db][4 * g + 2] * inv, o[db][4 * g + 3] * inv)};
                *reinterpret_cast<u32x2*>(op + 32 * db + 8 * g + 4 * hh) = w;
            }
    }
}

// scale_log2e: softmax scale * log2 e; 1 for a q that carries it already
template <typename T>
int attn_flash_launch(const void* q, const void* k, const void* v, void* out, int B, int H, int Sq, int Sk,
                      float scale_log2e, hipStream_t st, int64_t q_rs, int64_t kv_rs, int64_t o_rs, float* lse) {
    const int64_t hd = (int64_t)H * kFD;
    if (q_rs == 0) q_rs = hd;
    if (kv_rs == 0) kv_rs = hd;
    if (o_rs == 0) o_rs = hd;
    const int q_blocks = (Sq + kFQ - 1) / kFQ;
    const int64_t total = (int64_t)B * H * q_blocks;
    if (total > 0x7FFFFFFFll) return MVI_EINVAL;
    if (lse)
        hipLaunchKernelGGL((attn_flash_kernel<T, true>), dim3((unsigned)total), dim3(256), 0, st, (const T*)q, (const T*)k,
                           (const T*)v, (T*)out, H, Sq, Sk, scale_log2e, q_blocks, (int)total, q_rs, kv_rs, o_rs, lse);
    else
        hipLaunchKernelGGL((attn_flash_kernel<T, false>), dim3((unsigned)total), dim3(256), 0, st, (const T*)q, (const T*)k,
                           (const T*)v, (T*)out, H, Sq, Sk, scale_log2e, q_blocks, (int)total, q_rs, kv_rs, o_rs, (float*)nullptr);
    return hipGetLastError() == hipSuccess ? 0 : MVI_EHIP;
}
template int attn_flash_launch<__hip_bfloat16>(const void*, const void*, const void*, void*, int, int, int, int, float, hipStream_t, int64_t, int64_t, int64_t, float*);
template int attn_flash_launch<__half>(const void*, const void*, const void*, void*, int, int, int, int, float, hipStream_t, int64_t, int64_t, int64_t, float*);

}  // namespace mvi
