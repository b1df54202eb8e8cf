// Temporal self-attention for 17 .. 32 frames in bf16 / f16, head dim 64: the 25-frame checkpoint of the reference's stock sampler
// (svd_xt: svd_inpaint1/scripts/sampling/simple_video_sample.py:46-55) — 92 160 problems of 25 x 25 x 64 at
// level 0 of a 576x1024 step at CFG batch 2. csrc/attn_temporal.hip (T <= 16) extended by a second key tile and a second query tile,
// same index maps; a problem reads 3 T rows of 128 bytes and writes T (12.5 KiB at T = 25), one wave per problem:
//   S^T[key][query] = K Q^T      two key tiles x two query tiles x two d-steps: 8 v_mfma_f32_16x16x32. Lane (r16 = l & 15, g = l >> 4)
//                                loads K and Q rows r16 and 16 + r16, 16 bytes at d = 32 step + 8 g — no LDS.
//                                C layout of tile (kt, qt): lane (query 16 qt + r16, g) holds keys 16 kt + 4 g + r, r < 4.
//   softmax over keys            per query tile: over the lane's 2 x 4 registers and the 4 lane groups (two xor-shuffles).
//   O^T[d][query] = V^T P^T      B = P^T: contraction index k = 8 g + j stands for key 4 g + j (j < 4) and key 16 + 4 g + j - 4 (j >= 4):
//                                the lane's eight probabilities ARE its B fragment — what is half zeros at T <= 16 is the second key
//                                tile here. A = V^T under the same map: two ds_read_b64_tr_b16 per 16-channel tile from the row-major
//                                32-row V image (mfma_common.h: read_frag_tr; EXEC is all ones wherever they run). Rows T .. 31 of
//                                the image are zeroed once. 4 channel tiles x 2 query tiles: 8 MFMAs.
//                                C layout: lane (query 16 qt + r16, g) holds channels 16 tile + 4 g + r: one 8-byte store per tile.
// V image rows are 160 bytes (40 dwords): the 8 rows a 32-lane half reads at once (two 4-row blocks, 32 bytes of each row) start at
// banks 0, 40, 16, 56, 32, 8, 48, 24 of 64 — disjoint — and a piece is stored as one aligned 16 bytes.
// A wave walks problems grid-stride and loads the next problem's fragments before it computes the current one.
#include <cstdint>

#include "attn_launch.h"
#include "mfma_common.h"

namespace mvi {
namespace at32 {


constexpr int kD = 64;
constexpr int kWaves = 4;                            // waves per block, one problem each at a time
constexpr int kTCap = 32;
constexpr int kVRow = 160;                           // bytes per V row in LDS
constexpr int kVTile = kTCap * kVRow;
constexpr int kBlocksPerCU = 3;                      // (the register count leaves 3 waves per SIMD)

template <typename T> using Mma = MmaBuiltin16<T>;

struct Operands {                                    // one problem's global loads, in flight while the previous problem computes
    u32x4 k[2][2], q[2][2];                          // [row tile][d step] (frame T - 1 again for the rows >= T)
    u32x4 v[4];                                      // V pieces lane + 64 i of the T x 8 pieces of 16 bytes
};

template <typename T>
__global__ __launch_bounds__(64 * kWaves) void attn_temporal32_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
                                                                      T* __restrict__ out, int Tn, int S, int H, float scale,
                                                                      int64_t n_problems, int64_t qkv_ts, int64_t o_ts) {
    using M = Mma<T>;
    using frag = typename M::frag;
    __shared__ __attribute__((aligned(16))) char s_v[kWaves * kVTile];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r16 = lane & 15, g = lane >> 4;
    char* const vt = s_v + wave * kVTile;
    MVI_AS3 char* const vt3 = (MVI_AS3 char*)s_v + wave * kVTile;
    const int64_t n_waves = (int64_t)gridDim.x * kWaves;
    const bool frame_ok[2] = {r16 < Tn, 16 + r16 < Tn};              // this lane's K / Q rows (and output rows) exist
    const int64_t q_frame = (int64_t)S * qkv_ts, o_frame = (int64_t)S * o_ts;      // elements between frames of one token
    const int rclamp[2] = {min(r16, Tn - 1), min(16 + r16, Tn - 1)};
    int vclamp[4];                                                   // frame of V piece lane + 64 i (piece lane % 8 of its row)
#pragma unroll
    for (int i = 0; i < 4; ++i) vclamp[i] = min((lane + 64 * i) >> 3, Tn - 1);

    // problem p = (bo S + s) H + h: element offset of (frame 0, token s, head h) in q / k / v and in out
    auto load = [&](int64_t p, Operands& o) __attribute__((always_inline)) {
        const int64_t bs = p / H;
        const int h = (int)(p - bs * H);
        const int64_t bo = bs / S, s = bs - bo * S;
        const int64_t base = (bo * Tn * S + s) * qkv_ts + (int64_t)h * kD;
        // no load sits in a branch (attn_temporal.hip: the compiler counts vmcnt only through straight-line code). Lanes whose frame
        // does not exist read frame T - 1 instead: as K rows they end in masked scores, as Q rows in columns that are never stored.
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            const int64_t row = base + rclamp[rt] * q_frame + 8 * g;
            o.k[rt][0] = *reinterpret_cast<const u32x4*>(k + row);
            o.k[rt][1] = *reinterpret_cast<const u32x4*>(k + row + 32);
            o.q[rt][0] = *reinterpret_cast<const u32x4*>(q + row);
            o.q[rt][1] = *reinterpret_cast<const u32x4*>(q + row + 32);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) o.v[i] = *reinterpret_cast<const u32x4*>(v + base + vclamp[i] * q_frame + 8 * (lane & 7));
    };

    int64_t p = (int64_t)blockIdx.x * kWaves + wave;
    if (p >= n_problems) return;                     // (whole wave)
    Operands cur, nxt;
    load(p, cur);
    // rows T .. 31 of the V image are read (times probability 0) by the lanes whose keys do not exist: keep them finite
    for (int e = lane; e < (kTCap - Tn) * (kVRow / 8); e += 64) *reinterpret_cast<u32x2*>(vt + Tn * kVRow + 8 * e) = u32x2{0u, 0u};
    // transposed read: the 16-lane group g reads the 4-row x 16-channel block (rows 4 g .. 4 g + 3); lane 4 qq + pp of the group
    // supplies row qq, channels 4 pp .. 4 pp + 3 and receives channel r16
    const uint32_t tr_a = (uint32_t)((4 * g + (r16 >> 2)) * kVRow + 8 * (r16 & 3));

    for (; p < n_problems; p += n_waves) {
        const int64_t pn = p + n_waves;
        load(pn < n_problems ? pn : n_problems - 1, nxt);            // (unconditional, like the loads inside: the last round's is unused)

        // ---- V -> LDS, row-major
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = lane + 64 * i, t = e >> 3;
            if (t < Tn) *reinterpret_cast<u32x4*>(vt + t * kVRow + 16 * (e & 7)) = cur.v[i];
        }
        __builtin_amdgcn_wave_barrier();

        // ---- scores, transposed: lane (query 16 qt + r16, g) gets keys 16 kt + 4 g + r
        f32x4 sc[2][2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                sc[kt][qt] = M::mfma(as_frag<frag>(cur.k[kt][0]), as_frag<frag>(cur.q[qt][0]), f32x4{0.f, 0.f, 0.f, 0.f});
                sc[kt][qt] = M::mfma(as_frag<frag>(cur.k[kt][1]), as_frag<frag>(cur.q[qt][1]), sc[kt][qt]);
            }
        u32x4 pb[2];
        float inv[2];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            float m = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    sc[kt][qt][r] = 16 * kt + 4 * g + r < Tn ? sc[kt][qt][r] * scale : -INFINITY;
                    m = fmaxf(m, sc[kt][qt][r]);
                }
            m = fmaxf(m, __shfl_xor(m, 16));
            m = fmaxf(m, __shfl_xor(m, 32));         // (key 0 exists: finite for every query row, clamped ones included)
            float pr[2][4], l = 0.f;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pr[kt][r] = __expf(sc[kt][qt][r] - m);
                    l += pr[kt][r];
                }
            l += __shfl_xor(l, 16);
            l += __shfl_xor(l, 32);
            pb[qt] = u32x4{M::pack2(pr[0][0], pr[0][1]), M::pack2(pr[0][2], pr[0][3]), M::pack2(pr[1][0], pr[1][1]), M::pack2(pr[1][2], pr[1][3])};
            inv[qt] = 1.0f / l;
        }

        // ---- O^T tile by tile: A = V^T[d = 16 tile + r16][keys 4 g .. 4 g + 3, 16 + 4 g .. 16 + 4 g + 3] from LDS
        const int64_t bs = p / H;
        const int h = (int)(p - bs * H);
        const int64_t bo = bs / S, s = bs - bo * S;
        T* const orow = out + (bo * Tn * S + s) * o_ts + (int64_t)h * kD + r16 * o_frame + 4 * g;
#pragma unroll
        for (int tile = 0; tile < 4; ++tile) {
            const frag va = read_frag_tr<frag>(vt3 + tr_a + 32 * tile, 16 * kVRow);
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                const f32x4 o = M::mfma(va, as_frag<frag>(pb[qt]), f32x4{0.f, 0.f, 0.f, 0.f});
                if (frame_ok[qt]) {
                    const u32x2 w = {M::pack2(o[0] * inv[qt], o[1] * inv[qt]), M::pack2(o[2] * inv[qt], o[3] * inv[qt])};
                    *reinterpret_cast<u32x2*>(orow + 16 * qt * o_frame + 16 * tile) = w;
                }
            }
        }
        cur = nxt;
    }
}

}  // namespace at32

// Covered: bf16 / f16, D = 64, 16 < T <= 32, strides that keep every row 16-byte aligned (q, k, v) / 8-byte aligned (out).
bool attn_temporal32_ok(int T, int D, int dtype, int64_t hd, int64_t qkv_ts, int64_t o_ts, const void* q, const void* k, const void* v,
                        const void* out) {
    if (!(dtype == MVI_DT_BF16 || dtype == MVI_DT_F16) || D != at32::kD || T <= 16 || T > at32::kTCap) return false;
    const int64_t qs = qkv_ts ? qkv_ts : hd, os = o_ts ? o_ts : hd;
    return qs % 8 == 0 && os % 4 == 0 && ((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 == 0 && (uintptr_t)out % 8 == 0;
}

template <typename T>
int attn_temporal32_launch(const void* q, const void* k, const void* v, void* out, int Bo, int Tn, int S, int H, float scale, hipStream_t st,
                           int64_t qkv_ts, int64_t o_ts) {
    using namespace at32;
    const int64_t hd = (int64_t)H * kD;
    if (qkv_ts == 0) qkv_ts = hd;
    if (o_ts == 0) o_ts = hd;
    const int64_t n = (int64_t)Bo * S * H;
    if (n == 0) return 0;
    if (Tn <= 0 || Tn > kTCap) return MVI_EINVAL;
    // as many waves as fit (kBlocksPerCU blocks of 4 waves on 256 CUs), each walking ~n / waves problems with one problem in flight
    int64_t blocks = (n + kWaves - 1) / kWaves;
    if (blocks > 256 * kBlocksPerCU) blocks = 256 * kBlocksPerCU;
    hipLaunchKernelGGL((attn_temporal32_kernel<T>), dim3((unsigned)blocks), dim3(64 * kWaves), 0, st, (const T*)q, (const T*)k, (const T*)v,
                       (T*)out, Tn, S, H, scale, n, qkv_ts, o_ts);
    return hipGetLastError() == hipSuccess ? 0 : MVI_EHIP;
}

template int attn_temporal32_launch<__hip_bfloat16>(const void*, const void*, const void*, void*, int, int, int, int, float, hipStream_t, int64_t, int64_t);
template int attn_temporal32_launch<__half>(const void*, const void*, const void*, void*, int, int, int, int, float, hipStream_t, int64_t, int64_t);

}  // namespace mvi
