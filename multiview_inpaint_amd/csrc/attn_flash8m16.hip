// bf16/f16 MFMA flash attention (forward), head dim 64, 8-wave workgroups, on v_mfma_f32_16x16x32 — the kernel behind the large
// spatial self-attentions of the SVD denoise step: (B*H, S) = (140, 9216) and (280, 2304) at 14 x 576x1024, 99.7 % of the attention
// FLOPs. Replaces xformers.ops.memory_efficient_attention / SDPA (svd_inpaint1/sgm/modules/attention.py:427-439,
// :332-336). attn_flash.hip keeps the 4-wave kernel for short sequences; mvi_attention_kernel_variant reports 16 where this one runs.
//
// Why a second kernel: at D = 64 the 4-wave kernel is bound by the SIMD's ISSUE port, not by the matrix pipe
// (profiles/r01u_pmc_attention.txt: 13.8 VALU per MFMA, pipe 39.7 % busy). This one removes issue slots:
//   * the running reference exponent m never touches the VALU: -m enters the scores as the C operand of the first MFMA of every
//     QK^T chain (a register block holding -m). The softmax SCALE has two forms (template kExact, below): applied to the fp32
//     scores (one v_mul per score; the form a caller's own q gets in bf16), or absent from the loop because Q carries
//     scale * log2(e) — either rounded into Q in the prologue (f16's default: a second rounding of q) or already inside q from its
//     projection's weights (mvi_attention_forward_strided_qlog2: no second rounding, both types; what the self-attentions of the
//     SVD modules run) — so P = exp2(S') directly. Which form a call gets is decided in attn_api.hip (attention_folds_scale);
//   * the softmax row sums come out of the matrix pipe: a fifth "d tile" whose V^T fragment is a row of ones (two more MFMAs per
//     32-key block, +1/8 of the matrix work) replaces 32 v_add_f32 per wave and tile; the sums are then those of the ROUNDED
//     probabilities, i.e. of exactly the numerators the P V products use;
//   * K and V tiles go HBM/L2 -> LDS by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave-instruction) instead of through VGPRs
//     (8 loads + 12 LDS stores + 16 pack ops per wave and tile in the 4-wave kernel);
//   * V stays row-major in LDS and is read transposed by ds_read_b64_tr_b16 (no hand transposition);
//   * the loop is unrolled over a 4-deep ring with two score accumulators in FIXED roles, so neither ring offsets nor an
//     accumulator hand-over cost instructions (16 v_mov_b64 per tile in the 4-wave kernel);
//   * 256 query rows share one K/V tile (8 waves x 32 rows): half the LDS fill traffic per row.
// Measured and not kept (profiles/round6_attention_mfma16_ab.txt, same box, alternating; commit 7903115 is the last that holds them):
// the same kernel on v_mfma_f32_32x32x16 (a file of its own there) and this one with the row sums on the VALU. Per 64-key tile and
// block 1638 shader cycles on 32x32x16, 1841 here with VALU row sums, 1868 as shipped — at in-kernel clocks of 1.83, 2.07 and
// 2.11 GHz: the chip is power-bound under this kernel and pays the cheaper instruction back as clock, 12 % more cycles become
// 2.7 - 3.0 % LESS time (S = 9216: 2.742 -> 2.668 ms; S = 2304: 0.402 -> 0.390 ms). On all-zero operands (2.39 GHz for all three) the
// order is the cycle order.
//
// Layout: q/out [B, Sq, H, 64], k/v [B, Sk, H, 64] token-major with element strides q_rs / kv_rs / o_rs between tokens (H*64 when
// contiguous, 3*H*64 inside a packed projection).
// A wave owns 32 queries = two 16-query tiles (qt). Lane = (c = lane & 15, g = lane >> 4).
// Per wave and 32-key block (two 16-key tiles kt), v_mfma_f32_16x16x32, fp32 accumulate:
//   S'^T[key][query] (16 x 16) = K (16 keys x 32 d) Q'^T (32 d x 16 queries) - m : 2 kt x 2 qt x 2 d-steps = 8 MFMA
//        A = K rows from LDS: lane (c, g) holds K[16 kt + c][32 ks + 8 g .. + 7]  (one ds_read_b128, shared by both qt)
//        B = Q' in registers: lane (c, g) holds Q[16 qt + c][32 ks + 8 g .. + 7]
//        C/D: lane (c, g) holds S'^T[key 16 kt + 4 g + r][query 16 qt + c], r = 0..3; the first MFMA of a chain takes -m as C
//   P = exp2(S'): the query sits on the lane, everything lane-local; row sums reduced over g at the very end
//   O^T[d][query] (16 x 16) += V^T (16 d x 32 keys) P^T (32 keys x 16 queries): 4 d tiles x 2 qt = 8 MFMA
//        B = P from the S' accumulators: element j of lane (c, g) is k-index 8 g + j  <->  key (j < 4 ? 4 g + j : 16 + 4 g + j - 4)
//        A = V^T by two ds_read_b64_tr_b16 per d tile (keys 4 g .. 4 g + 3 of key tile 0, then of key tile 1): the same permutation
// LDS images (128-byte rows, 16-byte chunks XOR-swizzled; the DMA's destination is lane-linear, so the swizzle is applied to the
// SOURCE address): K chunk c of row r in slot c ^ ((r >> 1) & 7) (ds_read_b128 of 16 rows x one chunk: conflict-free); V chunk c of
// row r in slot c ^ (((r >> 1) & 3) << 1) (a transposed read touches 8 rows x 32 bytes per half wave: conflict-free).
// Ring: 4 slots each for K and V; tile t (between two barriers) issues K_{t+3}, V_{t+3}; before the closing barrier every wave waits
// for its own pieces of tile t + 2 with a COUNTED vmcnt (the pieces of tile t + 3 stay in flight across the barrier).
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "attn_launch.h"
#include "mfma_common.h"

namespace mvi {
namespace f8m {

constexpr int kD = 64;            // head dim
constexpr int kKT = 64;           // keys per tile
constexpr int kRing = 4;
constexpr int kTileBytes = kKT * kD * 2;          // 8 KiB
constexpr int kLdsBytes = 2 * kRing * kTileBytes; // K ring | V ring = 64 KiB (+ 16 bytes: the block's "repeat safely" flag)
constexpr float kRescaleThreshold = 8.0f;         // log2 units: O, l rescaled only when the row max grows by > 2^8
// kWaves = 8: one 512-thread block per CU (2 waves per SIMD, 256 query rows share a K/V tile). kLoaders = 4: waves 0 .. 3 move the
// LDS-DMA pieces, at the END of a tile (see issue_tile). The timing ablations, in-kernel stamps and block timeline that led here (other
// kWaves / kLoaders, static wave priority, DMA pieces spread over the quarters — all measured and not kept) are in profiles/HISTORY.md
// rounds 2 - 5; the diagnostic build that exists today is generated from this file (tools/attn_dev/build_stamped.sh), not kept beside it.
constexpr int kWaves = 8;
constexpr int kLoaders = 4;

template <typename T> using Mma = MmaBuiltin16<T>;

template <int N> __device__ __forceinline__ void wait_vm_then_barrier() {
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}
// reduction over the four 16-lane groups of a wave (the keys of a query are spread over g)
__device__ __forceinline__ float group_sum(float x) {
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
__device__ __forceinline__ float group_max(float x) {
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = __builtin_fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __builtin_fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

// scores of one 32-key block: [key tile kt][query tile qt], each the C/D tile of one accumulation chain
struct Scores { f32x4 t[2][2]; };

// kExact: the softmax scale is applied to the fp32 scores (one v_mul per score) instead of being rounded into Q. Folding
// scale * log2(e) into Q saves those 32 multiplies per wave and tile but rounds Q a second time to bf16: an error of
// |logit| * 2^-9 in the exponent, i.e. a few per cent on P where two keys with logits of ~60 compete (2.7e-2 of the
// output scale on the adversarial rows of tests/test_unet_ops_gpu.py, against 5e-3 with the exact form).
// kLse: as in attn_flash.hip — the row's log-sum-exp beside an `out` computed by the same instructions
template <typename T, bool kExact, bool kLse = false>
__global__ __launch_bounds__(64 * kWaves) __attribute__((amdgpu_waves_per_eu(2, 2)))
void attn_flash8m16_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, T* __restrict__ out,
                           int H, int Sq, int Sk, float scale_log2e, int q_blocks, int total_blocks, int64_t q_rs,
                           int64_t kv_rs, int64_t o_rs, float* __restrict__ lse) {
    using M = Mma<T>;
    using frag = typename M::frag;
    constexpr int kQB = 32 * kWaves;             // query rows per block
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    MVI_AS3 char* const lds = (MVI_AS3 char*)smem;
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)lds);

    int bid = blockIdx.x;
    if ((total_blocks & 7) == 0) bid = (bid & 7) * (total_blocks >> 3) + (bid >> 3);    // consecutive q blocks of a head share an XCD's L2
    const int qb = bid % q_blocks;
    const int bh = bid / q_blocks;
    const int h = bh % H;
    const int64_t b = bh / H;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, g = lane >> 4;
    const int qrow0 = qb * kQB + wave * 32 + c16;     // query of tile qt: qrow0 + 16 qt

    const float sc_mul = kExact ? scale_log2e : 1.0f;
    // ---- Q': B operand of S'^T = K Q'^T, element j of lane (c, g), query tile qt, d-step ks: Q[qrow0 + 16 qt][32 ks + 8 g + j]
    frag qf[2][2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int qrow = qrow0 + 16 * qt;
        const T* qp = q + ((b * Sq + (qrow < Sq ? qrow : 0)) * q_rs + (int64_t)h * kD + 8 * g);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            u32x4 raw = qrow < Sq ? *reinterpret_cast<const u32x4*>(qp + 32 * ks) : u32x4{0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (!kExact) raw[i] = M::pack2(M::lo(raw[i]) * scale_log2e, M::hi(raw[i]) * scale_log2e);
            qf[qt][ks] = as_frag<frag>(raw);
        }
    }

    // ---- LDS-DMA source addressing. A tile is 16 pieces of 1 KiB: pieces 0..7 = K rows 8 p .. 8 p + 7, pieces 8..15 = the same for
    // V. Lane i of piece p fills LDS slot (row 8 (p & 7) + (i >> 3), 16-byte slot i & 7) with the chunk the image's swizzle assigns
    // to that slot. Only waves 0 .. kLoaders - 1 move pieces (wave w: pieces w, w + kLoaders, ...), and they do it at the END of a
    // tile: issuing a piece costs its wave ~150 cycles, and the first-dispatched half of the workgroup wins the SIMD's arbitration
    // and waits ~500 cycles per tile at the barrier for the other half: that wait is where the loaders issue.
    const char* const kbase = reinterpret_cast<const char*>(k + (b * Sk * kv_rs + (int64_t)h * kD));
    const char* const vbase = reinterpret_cast<const char*>(v + (b * Sk * kv_rs + (int64_t)h * kD));
    constexpr int kMaxPieces = (16 + kLoaders - 1) / kLoaders;
    const int n_pieces = wave < kLoaders ? (16 - wave + kLoaders - 1) / kLoaders : 0;
    const uint32_t row_bytes = (uint32_t)(kv_rs * 2);
    const int pslot = lane & 7;
    int p_row[kMaxPieces], p_chunk[kMaxPieces];
    uint32_t p_voff[kMaxPieces], p_dst[kMaxPieces];
    bool p_is_v[kMaxPieces];
#pragma unroll
    for (int i = 0; i < kMaxPieces; ++i) {
        const int pc = wave + i * kLoaders;
        p_is_v[i] = pc >= 8;
        p_row[i] = 8 * (pc & 7) + (lane >> 3);
        p_chunk[i] = p_is_v[i] ? pslot ^ (((p_row[i] >> 1) & 3) << 1) : pslot ^ ((p_row[i] >> 1) & 7);
        p_voff[i] = (uint32_t)p_row[i] * row_bytes + 16u * p_chunk[i];
        p_dst[i] = lds0 + (p_is_v[i] ? kRing * kTileBytes : 0) + 1024u * (pc & 7);
    }
    const int n_tiles = (Sk + kKT - 1) / kKT;
    const int n_full = Sk / kKT;                 // tiles whose 64 rows all exist
    // tiles past the end are still "loaded" (rows clamped to Sk - 1) so that every iteration issues the same number of pieces and
    // the counted vmcnt stays valid; their ring slots are never read
    auto issue_tile = [&](int tt) __attribute__((always_inline)) {
        const uint32_t ring_off = (uint32_t)((tt & (kRing - 1)) * kTileBytes);
        const bool full = tt < n_full;
        const int64_t off = (int64_t)tt * kKT * row_bytes;
#pragma unroll
        for (int i = 0; i < kMaxPieces; ++i) {
            if (i >= n_pieces) break;
            const char* const base = p_is_v[i] ? vbase : kbase;
            if (full) {
                dma_piece(base + off, p_voff[i], p_dst[i] + ring_off);
            } else {
                int r = tt * kKT + p_row[i];
                r = r < Sk ? r : Sk - 1;
                dma_piece(base, (uint32_t)r * row_bytes + 16u * p_chunk[i], p_dst[i] + ring_off);
            }
        }
    };
    // counted waits: "at most `tiles_c` tiles' worth of this wave's own pieces still outstanding", then the barrier
    auto wait_tiles_then_barrier = [&](auto tiles_c) __attribute__((always_inline)) {
        constexpr int kT = decltype(tiles_c)::value;
        static_assert(16 % kLoaders == 0, "every loader moves 16 / kLoaders pieces");
        if (n_pieces == 0) wait_vm_then_barrier<0>();
        else wait_vm_then_barrier<kMaxPieces * kT>();
    };

    // ---- LDS read addressing (per lane; ring slot / block / key tile enter as immediates)
    // K, A operand: row 32 kb + 16 kt + c, chunk 4 ks + g  ->  slot (4 ks + g) ^ ((c >> 1) & 7)   (16 kt and 32 kb leave (row >> 1) & 7 alone)
    uint32_t ka[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) ka[ks] = (uint32_t)(c16 * 128 + (((4 * ks + g) ^ ((c16 >> 1) & 7)) << 4));
    // V^T, A operand of d tile dt: the 16-lane group g reads the 4-key x 16-d block (keys 4 g .. 4 g + 3 of a key tile, d0 = 16 dt);
    // lane 4 qq + p of the group supplies row qq, columns 4 p .. 4 p + 3 and receives column c. Row 4 g + qq holds chunk ch in slot
    // ch ^ (x << 1), x = ((4 g + qq) >> 1) & 3: byte 32 (dt ^ x) + 8 p of the row.
    uint32_t va[4];
    {
        const int qq = c16 >> 2, p = c16 & 3, x = (2 * (g & 1) + (qq >> 1)) & 3;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) va[dt] = kRing * kTileBytes + (uint32_t)((4 * g + qq) * 128 + ((dt ^ x) << 5) + 8 * p);
    }

    f32x4 o[4][2], negm[2];                  // o[d tile][query tile]
    f32x4 lacc[2];                           // row 0 of the "ones" tile = the row sums (lanes g == 0, register 0; zeros elsewhere)
    const uint32_t one2 = std::is_same<T, __half>::value ? 0x3C003C00u : 0x3F803F80u;
    const u32x4 ones = c16 == 0 ? u32x4{one2, one2, one2, one2} : u32x4{0, 0, 0, 0};     // A operand: V^T row 0 = 1 for every key
    Scores s0, s1;                           // scores of key block 0 / 1 of a tile: FIXED roles
    float l[2], rsum[2];                     // l: row sum up to the last rescale; rsum (kLse only): what the VALU added since
    float l_exact[2] = {0.f, 0.f};           // kLse only

    // all of S' of one 32-key block (prologue only)
    auto qk_block = [&](int slot, int kb, Scores& sc) __attribute__((always_inline)) {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const u32x4 kf = *reinterpret_cast<MVI_AS3 const u32x4*>(lds + ka[ks] + slot * kTileBytes + kb * 4096 + kt * 2048);
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) sc.t[kt][qt] = M::mfma(as_frag<frag>(kf), qf[qt][ks], ks == 0 ? negm[qt] : sc.t[kt][qt]);
            }
    };
    // keys >= Sk of the block that starts at key kbase0 never win
    auto mask_block = [&](Scores& sc, int kbase0) __attribute__((always_inline)) {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (kbase0 + 16 * kt + 4 * g + r >= Sk) { sc.t[kt][0][r] = -INFINITY; sc.t[kt][1][r] = -INFINITY; }
    };
    // Row max of a block whose scores already carry -m, for query tile qt
    auto block_max = [&](const Scores& sc, int qt) __attribute__((always_inline)) {
        const f32x4 a = sc.t[0][qt], bb = sc.t[1][qt];
        const float ra = __builtin_fmaxf(__builtin_fmaxf(a[0], a[1]), __builtin_fmaxf(a[2], a[3]));
        const float rb = __builtin_fmaxf(__builtin_fmaxf(bb[0], bb[1]), __builtin_fmaxf(bb[2], bb[3]));
        return group_max(__builtin_fmaxf(ra, rb));
    };
    // Moves the reference exponent of the lanes in `grow` up by their block's excess over it: O, l, the block's scores and the -m
    // operand all follow (first: O = l = 0, nothing to scale — and 0 * 2^big would be NaN)
    auto rescale = [&](Scores& sc, const bool (&grow)[2], const float (&rmax)[2], bool first) __attribute__((always_inline)) {
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            const float delta = grow[qt] ? rmax[qt] : 0.f;
            const float alpha = first ? 1.0f : __builtin_amdgcn_exp2f(-delta * sc_mul);
            l[qt] = (l[qt] + rsum[qt]) * alpha;
            rsum[qt] = 0.f;
            lacc[qt] *= alpha;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[dt][qt] *= alpha;
            sc.t[0][qt] -= delta;
            sc.t[1][qt] -= delta;
            negm[qt] -= delta;
        }
    };
    // K fragments of one key tile (both d-steps): two ds_read_b128
    struct KFrags { u32x4 k[2]; };
    auto load_k = [&](int slot, int kb, int kt, bool on) __attribute__((always_inline)) {
        KFrags f;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            f.k[ks] = on ? *reinterpret_cast<MVI_AS3 const u32x4*>(lds + ka[ks] + slot * kTileBytes + kb * 4096 + kt * 2048) : u32x4{0, 0, 0, 0};
        return f;
    };
    // V^T fragments of d tiles dt0, dt0 + 1 of block kb: four transposed reads into vs[dt0], vs[dt0 + 1]
    auto load_v = [&](u32x4 (&vs)[4], int slot, int kb, int dt0) __attribute__((always_inline)) {
#pragma unroll
        for (int dt = dt0; dt < dt0 + 2; ++dt) {
            const int off = slot * kTileBytes + kb * 4096;
            vs[dt] = read_frag_tr<u32x4>(lds + va[dt] + off, 2048);
        }
    };
    // exp / pack / row sum of query tile qt of a block: the P fragment (B operand of the P V MFMAs of that query tile)
    auto probs = [&](const Scores& sc, int qt) __attribute__((always_inline)) {
        u32x4 pr;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float x0 = kExact ? sc.t[kt][qt][2 * i] * sc_mul : sc.t[kt][qt][2 * i];
                const float x1 = kExact ? sc.t[kt][qt][2 * i + 1] * sc_mul : sc.t[kt][qt][2 * i + 1];
                const float p0 = __builtin_amdgcn_exp2f(x0);
                const float p1 = __builtin_amdgcn_exp2f(x1);
                if (kLse) rsum[qt] += p0 + p1;
                pr[2 * kt + i] = M::pack2(p0, p1);
            }
        // the sum is complete HERE: without this, the fast form (which reads rsum only after the loop) sinks four tiles' adds — and
        // 128 live P values — to the loop's end
        if (kLse) asm volatile("" : "+v"(rsum[qt]));
        return pr;
    };
    // The matrix work beside one quarter: the S' MFMAs of key tile kt of the OTHER block (into acc.t[kt][*]) and the four P V MFMAs
    // of query tile pqt with fragment pf and the V^T set vs. Dependent S' links sit two apart; two P V MFMAs trail the last link.
    auto matrix_part = [&](const KFrags& f, bool with_k, Scores& acc, int kt, u32x4 pf_raw, const u32x4 (&vs)[4], int pqt, bool with_pv) __attribute__((always_inline)) {
        const frag pf = as_frag<frag>(pf_raw);
        if (with_k) acc.t[kt][0] = M::mfma(as_frag<frag>(f.k[0]), qf[0][0], negm[0]);
        if (with_k) acc.t[kt][1] = M::mfma(as_frag<frag>(f.k[0]), qf[1][0], negm[1]);
        if (with_pv) o[0][pqt] = M::mfma(as_frag<frag>(vs[0]), pf, o[0][pqt]);
        if (with_k) acc.t[kt][0] = M::mfma(as_frag<frag>(f.k[1]), qf[0][1], acc.t[kt][0]);
        if (with_pv) o[1][pqt] = M::mfma(as_frag<frag>(vs[1]), pf, o[1][pqt]);
        if (with_k) acc.t[kt][1] = M::mfma(as_frag<frag>(f.k[1]), qf[1][1], acc.t[kt][1]);
        if (with_pv) o[2][pqt] = M::mfma(as_frag<frag>(vs[2]), pf, o[2][pqt]);
        if (with_pv) o[3][pqt] = M::mfma(as_frag<frag>(vs[3]), pf, o[3][pqt]);
        if (with_pv) lacc[pqt] = M::mfma(as_frag<frag>(ones), pf, lacc[pqt]);
    };

    // The whole key loop for this block's 256 queries. Two forms of the SAME arithmetic:
    //   kSafe = false (tried first): the reference exponent m is the row max of the FIRST 32 keys and never moves. Nothing about
    //     softmax needs the true maximum: P = 2^(s - m) / sum is exact for any m as long as nothing over- or underflows, fp32 / bf16
    //     keep their relative precision at any magnitude, and keys far below m are as negligible against the first block's own
    //     maximum (P = 1) as against the true one. Dropping the per-block max takes the v_max3 chain, the lane swaps and a
    //     compare-and-branch per tile off the issue port that bounds this kernel.
    //   kSafe = true: the usual online softmax (max per 32-key block, rescale when it grows by more than 2^8). Run only if the fast
    //     form's row sum left [0, 2^100] ([0, 2^15] in f16, where P must fit the type; or became NaN) for any query of the block —
    //     i.e. some score exceeded the first block's maximum by ~100 / log2(e) = 69 — everything is then recomputed from scratch.
    auto run = [&](auto safe_c) __attribute__((always_inline)) {
        constexpr bool kSafe = decltype(safe_c)::value;
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[dt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
            negm[qt] = f32x4{0.f, 0.f, 0.f, 0.f};
            lacc[qt] = f32x4{0.f, 0.f, 0.f, 0.f};
            l[qt] = 0.f;
            rsum[qt] = 0.f;
        }
        issue_tile(0);
        issue_tile(1);
        issue_tile(2);
        wait_tiles_then_barrier(std::integral_constant<int, 2>{});   // tile 0 landed everywhere
        qk_block(0, 0, s0);
        if (Sk < 32) mask_block(s0, 0);
        {
            const float rm[2] = {block_max(s0, 0), block_max(s0, 1)};
            const bool gr[2] = {true, true};
            rescale(s0, gr, rm, true);
        }
        wait_tiles_then_barrier(std::integral_constant<int, 1>{});   // tile 1
        u32x4 vb0[4], vb1[4];                                        // V^T sets of key block 0 / 1 of the current tile
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) { vb0[dt] = u32x4{0, 0, 0, 0}; vb1[dt] = u32x4{0, 0, 0, 0}; }
        KFrags fq0 = load_k(0, 1, 0, true), fq1 = load_k(0, 1, 1, true);   // S' of tile 0, block 1
        load_v(vb0, 0, 0, 0);                                        // (d tiles 2, 3 follow in the first quarter)

        auto decide = [&](Scores& sc) __attribute__((always_inline)) {
            if (!kSafe) return;
            const float rm[2] = {block_max(sc, 0), block_max(sc, 1)};
            const bool gr[2] = {rm[0] * sc_mul > kRescaleThreshold, rm[1] * sc_mul > kRescaleThreshold};
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(gr[0] || gr[1]) != 0ull, 0)) rescale(sc, gr, rm, false);   // wave-uniform, rare
        };
        // Fragments are requested TWO quarters before their use (measured: an MFMA that waits on its K fragment costs 19 % of the
        // kernel), also across the tile boundary: while tile t runs, tiles t and t + 1 are complete in LDS (the closing wait of tile
        // t - 1 covered tile t + 1), so its last two quarters request the first two of tile t + 1. The scheduling fences keep the
        // quarters apart (left alone, the scheduler hoists every LDS read of a tile and the allocator runs out of registers).
        // Fast form, software-pipelined: the MFMAs of a quarter are the S' MFMAs and the P V MFMAs of the PREVIOUS quarter (`pend`),
        // the VALU work is the P of THIS quarter — independent of each other, so an in-order wave never waits for its own pack
        // before a matrix instruction. Safe form: a quarter multiplies its own P (a rescale must find nothing pending).
        u32x4 pend = u32x4{0, 0, 0, 0};                              // fast form: the P fragment whose P V is still to be issued
        // One 64-key tile = four quarters; a quarter = one query tile of one 32-key block on the VALU (8 exp, 8 adds, 4 packs)
        // beside 8 MFMAs: the S' of one key tile of the other block and the P V of the PREVIOUS quarter's P (fast form) or of its
        // own (safe form).
        //            VALU                 S' MFMAs                      P V MFMAs (fast form)            LDS reads issued
        //   Q1   P(s0, qt 0)     s1 key tile 0 of tile t       P(prev s1, qt 1) x vb1(t - 1)     K(t+1, b0, kt0), vb0 d tiles 2, 3
        //   Q2   P(s0, qt 1)     s1 key tile 1                 P(s0, qt 0)     x vb0             K(t+1, b0, kt1), vb1 d tiles 0, 1
        //   Q3   P(s1, qt 0)     s0 key tile 0 of tile t + 1   P(s0, qt 1)     x vb0             K(t+1, b1, kt0), vb1 d tiles 2, 3
        //   Q4   P(s1, qt 1)     s0 key tile 1 of tile t + 1   P(s1, qt 0)     x vb1             K(t+1, b1, kt1), vb0(t+1) d tiles 0, 1
        constexpr bool kPipe = !kSafe;
        auto quarter = [&](const KFrags& f, bool with_k, Scores& acc, int kt, const Scores& sc, int qt, const u32x4 (&v_pipe)[4],
                           const u32x4 (&v_own)[4], bool pend_valid) __attribute__((always_inline)) {
            if (kPipe) {
                matrix_part(f, with_k, acc, kt, pend, v_pipe, qt ^ 1, pend_valid);
                pend = probs(sc, qt);
            } else {
                const u32x4 now = probs(sc, qt);
                matrix_part(f, with_k, acc, kt, now, v_own, qt, true);
            }
        };
        auto tile = [&](int t, auto slot_c, auto has_next_c) __attribute__((always_inline)) {
            const int slot = slot_c, next = (slot + 1) & (kRing - 1);
            const bool has_next = has_next_c;
            const int k0 = t * kKT;
            const bool ragged = !has_next && k0 + kKT > Sk;          // only the last tile can be ragged
            if (ragged && t > 0) mask_block(s0, k0);                 // (tile 0's first block was masked before it set m)
            decide(s0);
            KFrags f2 = load_k(next, 0, 0, has_next);
            load_v(vb0, slot, 0, 2);
            quarter(fq0, true, s1, 0, s0, 0, vb1, vb0, t > 0);       // (before tile 0 nothing is pending)
            __builtin_amdgcn_sched_barrier(0);
            KFrags f3 = load_k(next, 0, 1, has_next);
            load_v(vb1, slot, 1, 0);
            quarter(fq1, true, s1, 1, s0, 1, vb0, vb0, true);
            __builtin_amdgcn_sched_barrier(0);
            if (ragged) mask_block(s1, k0 + 32);
            decide(s1);
            if (has_next) fq0 = load_k(next, 1, 0, true);
            load_v(vb1, slot, 1, 2);
            quarter(f2, has_next, s0, 0, s1, 0, vb0, vb1, true);
            __builtin_amdgcn_sched_barrier(0);
            if (has_next) fq1 = load_k(next, 1, 1, true);
            if (has_next) load_v(vb0, next, 0, 0);
            quarter(f3, has_next, s0, 1, s1, 1, vb1, vb1, true);
            __builtin_amdgcn_sched_barrier(0);
            if (has_next) {
                // slot (t + 3) % 4 held tile t - 1: nobody reads it after the barrier that opened this tile
                issue_tile(t + 3);
                wait_tiles_then_barrier(std::integral_constant<int, 1>{});   // own pieces of tile t + 2 (and everything older) landed
            }
        };
        using std::integral_constant;
        using std::true_type;
        int t = 0;
        for (; t + 4 < n_tiles; t += 4) {
            tile(t, integral_constant<int, 0>{}, true_type{});
            tile(t + 1, integral_constant<int, 1>{}, true_type{});
            tile(t + 2, integral_constant<int, 2>{}, true_type{});
            tile(t + 3, integral_constant<int, 3>{}, true_type{});
        }
        for (; t < n_tiles; ++t) tile(t, t & (kRing - 1), t + 1 < n_tiles);
        if (kPipe) {                                                 // the last quarter's P V: P(s1, qt 1) x vb1
            KFrags none;
            none.k[0] = none.k[1] = u32x4{0, 0, 0, 0};
            matrix_part(none, false, s0, 0, pend, vb1, 1, true);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // trailing (unused) pieces must land before the ring is reused / released
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            // kLse: `out` is normalised by the sum of the ROUNDED probabilities as always; the row statistic handed to the
            // backward is the sum of the unrounded ones (the backward recomputes P in fp32), kept on the VALU beside it
            if (kLse) l_exact[qt] = group_sum(l[qt] + rsum[qt]);     // the four lane groups hold disjoint keys
            l[qt] = group_sum(lacc[qt][0]);                          // (the sum sits in group 0, zeros elsewhere)
        }
    };

    MVI_AS3 uint32_t* const redo_flag = (MVI_AS3 uint32_t*)(lds + kLdsBytes);
    if (tid == 0) *redo_flag = 0u;                               // ordered before any read by the barriers of run()
    run(std::false_type{});
    // block-wide vote (the waves share the K / V ring and its barriers, so they repeat together or not at all)
    // (f16: P itself is packed to f16, which ends at 65504 — a row sum of at most 2^15 proves that no P of the row was larger)
    const float l_limit = std::is_same<T, __half>::value ? 0x1p15f : 0x1p100f;
    // Compared as BIT PATTERNS: with the row sums from the matrix pipe a probability that overflowed the type (f16: > 65504)
    // gives 0 x inf = NaN in the rows of the ones tile that hold zeros, i.e. a NaN sum — and this file is compiled with
    // -fno-honor-nans, under which `!(l <= limit)` may be folded to `l > limit` (false for NaN). Sums are >= 0: |bits| orders them,
    // and every inf / NaN pattern is above every finite limit.
    const uint32_t lim = __float_as_uint(l_limit);
    const bool out_of_range = (__float_as_uint(l[0]) & 0x7FFFFFFFu) > lim || (__float_as_uint(l[1]) & 0x7FFFFFFFu) > lim;
    if (__builtin_amdgcn_ballot_w64(out_of_range) != 0ull && lane == 0) *redo_flag = 1u;
    __syncthreads();
    if (*redo_flag != 0u) {
        __syncthreads();
        run(std::true_type{});
    }

#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int qrow = qrow0 + 16 * qt;
        // negm holds minus the reference exponent in the units of the accumulators (sc_mul apart from log2 units)
        if (kLse && qrow < Sq && g == 0) lse[(b * H + h) * Sq + qrow] = (__builtin_amdgcn_logf(l_exact[qt]) - negm[qt][0] * sc_mul) * 0.6931471805599453f;
        if (qrow < Sq) {
            const float inv = 1.0f / l[qt];
            T* op = out + ((b * Sq + qrow) * o_rs + (int64_t)h * kD + 4 * g);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                u32x2 w = {M::pack2(o[dt][qt][0] * inv, o[dt][qt][1] * inv), M::pack2(o[dt][qt][2] * inv, o[dt][qt][3] * inv)};
                *reinterpret_cast<u32x2*>(op + 16 * dt) = w;
            }
        }
    }
}

}  // namespace f8m

// fold: the kernel without the per-score multiply (!kExact) — q carries scale * log2(e) already (q_log2: the prologue then multiplies
// Q by exactly 1) or gets it rounded in; the caller decides (attention_folds_scale, attn_api.hip) and the backward is told the same
template <typename T>
int attn_flash8m16_launch(const void* q, const void* k, const void* v, void* out, int B, int H, int Sq, int Sk,
                          float scale, bool q_log2, bool fold, hipStream_t st, int64_t q_rs, int64_t kv_rs, int64_t o_rs, float* lse) {
    using namespace f8m;
    const int64_t hd = (int64_t)H * kD;
    if (q_rs == 0) q_rs = hd;
    if (kv_rs == 0) kv_rs = hd;
    if (o_rs == 0) o_rs = hd;
    constexpr int kQB = 32 * kWaves;
    const int q_blocks = (Sq + kQB - 1) / kQB;
    const int64_t total = (int64_t)B * H * q_blocks;
    if (total > 0x7FFFFFFFll) return MVI_EINVAL;
    if ((int64_t)Sk * kv_rs * 2 > 0xFFFFFFFFll) return MVI_EINVAL;       // 32-bit byte offsets inside one batch entry
    // all four forms before the first launch of any
    if (allow_large_lds<&attn_flash8m16_kernel<T, true>>(kLdsBytes + 16) || allow_large_lds<&attn_flash8m16_kernel<T, false>>(kLdsBytes + 16) ||
        allow_large_lds<&attn_flash8m16_kernel<T, true, true>>(kLdsBytes + 16) || allow_large_lds<&attn_flash8m16_kernel<T, false, true>>(kLdsBytes + 16))
        return MVI_EHIP;
    auto kern =lse ? (fold ? &attn_flash8m16_kernel<T, false, true> : &attn_flash8m16_kernel<T, true, true>)
                    : (fold ? &attn_flash8m16_kernel<T, false> : &attn_flash8m16_kernel<T, true>);
    hipLaunchKernelGGL(kern, dim3((unsigned)total), dim3(64 * kWaves), kLdsBytes + 16, st, (const T*)q, (const T*)k, (const T*)v,
                       (T*)out, H, Sq, Sk, q_log2 ? 1.0f : scale * 1.4426950408889634f, q_blocks, (int)total, q_rs, kv_rs, o_rs, lse);
    return hipGetLastError() == hipSuccess ? 0 : MVI_EHIP;
}
template int attn_flash8m16_launch<__hip_bfloat16>(const void*, const void*, const void*, void*, int, int, int, int, float, bool, bool, hipStream_t, int64_t, int64_t, int64_t, float*);
template int attn_flash8m16_launch<__half>(const void*, const void*, const void*, void*, int, int, int, int, float, bool, bool, hipStream_t, int64_t, int64_t, int64_t, float*);

}  // namespace mvi
