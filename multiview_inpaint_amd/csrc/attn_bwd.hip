// Backward of softmax(scale Q K^T) V for the shapes the MFMA forward kernels serve (bf16 / f16, D = 64, Sk > 32), deterministic:
// every output element is written by exactly one block, in a fixed order — no float atomics. Three launches:
//   delta   delta_i = sum_d dout_id out_id, fp32 [B, H, Sq] in the caller's workspace
//   dQ      one block per (batch, head, 128 queries): Q and dO resident, the keys (K, V) stream; 3 products: S^T = K Q^T,
//           dP^T = V dO^T, dQ^T += K^T dS^T; also writes sum_j P_ij dP_ij, the same delta free of out's rounding, for the next kernel
//   dK/dV   one block per (batch, head, 128 keys): K and V resident in registers, the queries (Q, dO, L, delta) stream through LDS;
//           per 64-query tile 4 products: S = Q K^T, dP = dO V^T, dV^T += dO^T P, dK^T += Q^T dS
// 7 tile products against the 5 of a single pass with atomic dQ: the price of run-to-run identical bits.
// Both kernels are ONE template (kDQ): a "resident" operand pair sits in registers as the B operands of the two score products and a
// "streamed" pair passes through a double-buffered LDS image, read row-wise (ds_read_b128) as the A operand of the score products
// and transposed (ds_read_b64_tr_b16) as the A operand of the output products, as attn_flash8m16.hip reads K and V^T.
//
// v_mfma_f32_16x16x32, lane = (c = lane & 15, g = lane >> 4), a wave owns 32 resident rows (two 16-row tiles rt):
//   scores[streamed][resident] (16 x 16) = A (streamed rows x 32 d) B (32 d x resident rows), 2 d-steps
//        A: lane (c, g) holds streamed[16 st + c][32 ks + 8 g .. + 7];  B: lane (c, g) holds resident[16 rt + c][32 ks + 8 g .. + 7]
//        C/D: lane (c, g) register i holds [streamed 16 st + 4 g + i][resident 16 rt + c]
//   P = exp2(s - L log2 e), dS = P (dP - delta) in fp32, rounded to the I/O type only as MFMA operands
//   out^T[d][resident] (16 x 16) += A (16 d x 32 streamed) B (32 streamed x 16 resident)
//        B = P or dS from the score accumulators: element j of lane (c, g) is streamed row (j < 4 ? 4 g + j : 16 + 4 g + j - 4)
//        A = two transposed 4-row x 16-d LDS reads (rows 4 g .. 4 g + 3 of streamed tile 0, then of tile 1): the same permutation
//        C/D: lane (c, g) register i holds out[resident 16 rt + c][d = 16 dt + 4 g + i]: one 8-byte store per d tile
// The softmax scale: the forward either multiplies the fp32 scores by scale log2 e (bf16) or rounds scale log2 e into Q (f16 default,
// attn_flash8m16.hip `kExact`; attention_folds_scale in attn_api.hip decides for both directions). L was computed from those scores,
// so the recomputation here takes the same form (kFold) — P then sums to one over a row; dK uses the unscaled Q (a second LDS
// image), dQ and dK get `scale` in the epilogue. (Measured: exact scores against a folded forward's L are WORSE — f16, S = 1300
// with a peaked row: dk rms 2.7 x the reference's own error against 1.8 x, dv 2.0 x against 0.4 x.)
// Rows past the end of a ragged last tile: resident rows are loaded as zeros and not stored; streamed rows are loaded as zeros and
// their P and dS are set to zero. No lane is ever masked around a transposed LDS read (it needs EXEC all ones).
//
// Temporal backward (softmax over the T <= 32 frames of each (video, token, head), [(Bo T), S, H, D], nothing regrouped): seven tensors
// against T x T scores, so one block per problem (64 threads for T <= 16, 256 above) recomputes the softmax in fp32 from an LDS copy.
#include <cstdlib>
#include <type_traits>

#include "attn_launch.h"
#include "mfma_common.h"

namespace mvi {
namespace bwd {


constexpr int kD = 64;
constexpr int kST = 64;                 // streamed rows per tile
constexpr int kWaves = 4;
constexpr int kRB = 32 * kWaves;        // resident rows per block
constexpr int kStride = 72;             // LDS row stride in elements (144 bytes: 16-byte aligned rows, 36 banks apart)
constexpr int kImg = kST * kStride * 2; // bytes of one tile image
constexpr float kLog2e = 1.4426950408889634f;

template <typename T> using Mma = MmaBuiltin16<T>;

// delta[b, h, i] = sum_d dout[b, i, h, d] out[b, i, h, d]: 8 lanes per row, 16 bytes per lane and tensor
template <typename T>
__global__ __launch_bounds__(256) void attn_bwd_delta_kernel(const T* __restrict__ out, const T* __restrict__ dout, float* __restrict__ delta,
                                                             int H, int Sq, int64_t rows) {
    using M = Mma<T>;
    const int64_t row = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);      // row = (b Sq + i) H + h
    const int part = threadIdx.x & 7;
    float acc = 0.f;
    if (row < rows) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(out + row * kD + 8 * part);
        const u32x4 d = *reinterpret_cast<const u32x4*>(dout + row * kD + 8 * part);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc += M::lo(a[i]) * M::lo(d[i]) + M::hi(a[i]) * M::hi(d[i]);
    }
    acc += __shfl_xor(acc, 1);
    acc += __shfl_xor(acc, 2);
    acc += __shfl_xor(acc, 4);
    if (row < rows && part == 0) {
        const int h = (int)(row % H);
        const int64_t bi = row / H;
        const int64_t b = bi / Sq, i = bi % Sq;
        delta[(b * H + h) * Sq + i] = acc;
    }
}

// kDQ: resident = (Q, dO), streamed = (K, V), output dQ.  !kDQ: resident = (K, V), streamed = (Q, dO), outputs dK and dV.
// n_res / n_str: rows of the resident / streamed side (Sq / Sk or Sk / Sq). lse, delta: [B, H, Sq] fp32.
template <typename T, bool kDQ, bool kFold>
__global__ __launch_bounds__(64 * kWaves) __attribute__((amdgpu_waves_per_eu(2, 2)))
void attn_bwd_kernel(const T* __restrict__ res1, const T* __restrict__ res2, const T* __restrict__ str1, const T* __restrict__ str2,
                     const float* __restrict__ lse, const float* __restrict__ delta, T* __restrict__ out1, T* __restrict__ out2,
                     float* __restrict__ delta_out, int H, int n_res, int n_str, float scale, int res_blocks) {
    using M = Mma<T>;
    using frag = typename M::frag;
    constexpr bool kImg3 = !kDQ && kFold;                        // a third image: Q carrying scale log2 e, for the S product only
    constexpr int kImages = kImg3 ? 3 : 2;
    __shared__ __attribute__((aligned(16))) char smem[2 * kImages * kImg];
    __shared__ __attribute__((aligned(16))) float s_stat[2][2][kST];     // [buffer][L log2 e | delta][streamed row] (dK/dV only)
    MVI_AS3 char* const lds = (MVI_AS3 char*)smem;

    const int rb = blockIdx.x % res_blocks;
    const int bh = blockIdx.x / res_blocks;
    const int h = bh % H;
    const int64_t b = bh / H;
    const int64_t hd = (int64_t)H * kD;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, g = lane >> 4;
    const int rrow0 = rb * kRB + wave * 32 + c16;                // resident row of tile rt: rrow0 + 16 rt
    const float scale_log2e = scale * kLog2e;
    const float sc_mul = kFold ? 1.0f : scale_log2e;

    // ---- resident operands: element j of lane (c, g), tile rt, d-step ks: X[rrow0 + 16 rt][32 ks + 8 g + j]
    frag xf[2][2], yf[2][2];
    float rL[2], rDelta[2];                                      // kDQ: the lane's query statistics
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const int rrow = rrow0 + 16 * rt;
        const bool ok = rrow < n_res;
        const int64_t off = (b * n_res + (ok ? rrow : 0)) * hd + (int64_t)h * kD + 8 * g;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            u32x4 x = ok ? *reinterpret_cast<const u32x4*>(res1 + off + 32 * ks) : u32x4{0, 0, 0, 0};
            const u32x4 y = ok ? *reinterpret_cast<const u32x4*>(res2 + off + 32 * ks) : u32x4{0, 0, 0, 0};
            if (kDQ && kFold) {
#pragma unroll
                for (int i = 0; i < 4; ++i) x[i] = M::pack2(M::lo(x[i]) * scale_log2e, M::hi(x[i]) * scale_log2e);
            }
            xf[rt][ks] = as_frag<frag>(x);
            yf[rt][ks] = as_frag<frag>(y);
        }
        if (kDQ) {
            const int64_t so = (b * H + h) * (int64_t)n_res + (ok ? rrow : 0);
            rL[rt] = lse[so] * kLog2e;
            rDelta[rt] = delta[so];
        } else {
            rL[rt] = 0.f;
            rDelta[rt] = 0.f;
        }
    }

    // ---- streamed tiles: global -> registers -> LDS; thread (row tid >> 2, 32-byte piece tid & 3) per tensor
    const int lr = tid >> 2, lp = tid & 3;
    const T* const s1base = str1 + (b * n_str * hd + (int64_t)h * kD + 16 * lp);
    const T* const s2base = str2 + (b * n_str * hd + (int64_t)h * kD + 16 * lp);
    const float* const lbase = lse + (b * H + h) * (int64_t)n_str;       // (dK/dV: the streamed side is the query side)
    const float* const dbase = delta + (b * H + h) * (int64_t)n_str;
    u32x4 pa0, pa1, pb0, pb1;
    float pl = 0.f, pd = 0.f;
    auto load_tile = [&](int s0) __attribute__((always_inline)) {
        const int r = s0 + lr;
        const bool ok = r < n_str;
        const int64_t o = (int64_t)(ok ? r : 0) * hd;
        const u32x4 z = {0, 0, 0, 0};
        pa0 = ok ? *reinterpret_cast<const u32x4*>(s1base + o) : z;
        pa1 = ok ? *reinterpret_cast<const u32x4*>(s1base + o + 8) : z;
        pb0 = ok ? *reinterpret_cast<const u32x4*>(s2base + o) : z;
        pb1 = ok ? *reinterpret_cast<const u32x4*>(s2base + o + 8) : z;
        if (!kDQ && tid < kST) {
            const int rr = s0 + tid;
            pl = rr < n_str ? lbase[rr] * kLog2e : 0.f;
            pd = rr < n_str ? dbase[rr] : 0.f;
        }
    };
    auto store_tile = [&](int buf) __attribute__((always_inline)) {
        char* const base = smem + buf * kImages * kImg + (lr * kStride + 16 * lp) * 2;
        *reinterpret_cast<u32x4*>(base) = pa0;
        *reinterpret_cast<u32x4*>(base + 16) = pa1;
        *reinterpret_cast<u32x4*>(base + kImg) = pb0;
        *reinterpret_cast<u32x4*>(base + kImg + 16) = pb1;
        if (kImg3) {
            u32x4 f0, f1;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f0[i] = M::pack2(M::lo(pa0[i]) * scale_log2e, M::hi(pa0[i]) * scale_log2e);
                f1[i] = M::pack2(M::lo(pa1[i]) * scale_log2e, M::hi(pa1[i]) * scale_log2e);
            }
            *reinterpret_cast<u32x4*>(base + 2 * kImg) = f0;
            *reinterpret_cast<u32x4*>(base + 2 * kImg + 16) = f1;
        }
        if (!kDQ && tid < kST) {
            s_stat[buf][0][tid] = pl;
            s_stat[buf][1][tid] = pd;
        }
    };

    // ---- LDS read addressing (byte offsets inside one image)
    // rows: streamed row 32 sb + 16 st + c, elements 32 ks + 8 g .. + 7
    const uint32_t row_a = (uint32_t)((c16 * kStride + 8 * g) * 2);
    // transposed: the 16-lane group g reads the 4-row x 16-d block (rows 4 g .. 4 g + 3, d0 = 16 dt); lane 4 qq + p of the group
    // supplies row qq, columns 4 p .. 4 p + 3 and receives column c
    const uint32_t tr_a = (uint32_t)(((4 * g + (c16 >> 2)) * kStride + 4 * (c16 & 3)) * 2);

    f32x4 acc1[4][2], acc2[4][2];             // [d tile][resident tile]: dQ^T | (dK^T, dV^T)
    float pdp[2] = {0.f, 0.f};                // kDQ: the lane's part of sum_j P_ij dP_ij, the delta the dK/dV kernel uses (see bwd_launch)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            acc1[dt][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
            acc2[dt][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }

    auto compute = [&](int buf, int s0) __attribute__((always_inline)) {
        MVI_AS3 char* const img1 = lds + buf * kImages * kImg;           // streamed 1: K (dQ) / Q (dK, dV)
        MVI_AS3 char* const img2 = img1 + kImg;                          // streamed 2: V / dO
        MVI_AS3 char* const imgs = kImg3 ? img1 + 2 * kImg : img1;       // what the S product reads
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) {
            f32x4 s[2][2], dp[2][2];                                     // [streamed tile st][resident tile rt]
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const uint32_t ro = row_a + (uint32_t)((32 * sb + 16 * st) * kStride * 2);
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const u32x4 a1 = *reinterpret_cast<MVI_AS3 const u32x4*>(imgs + ro + 64 * ks);
                    const u32x4 a2 = *reinterpret_cast<MVI_AS3 const u32x4*>(img2 + ro + 64 * ks);
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt) {
                        s[st][rt] = M::mfma(as_frag<frag>(a1), xf[rt][ks], ks == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : s[st][rt]);
                        dp[st][rt] = M::mfma(as_frag<frag>(a2), yf[rt][ks], ks == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : dp[st][rt]);
                    }
                }
            }
            // P and dS as B operands of the output products
            u32x4 pf[2], dsf[2];
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                f32x4 sl, sd;                                            // dK/dV: statistics of streamed rows 4 g .. 4 g + 3
                if (!kDQ) {
                    sl = *reinterpret_cast<const f32x4*>(&s_stat[buf][0][32 * sb + 16 * st + 4 * g]);
                    sd = *reinterpret_cast<const f32x4*>(&s_stat[buf][1][32 * sb + 16 * st + 4 * g]);
                }
                const int srow = s0 + 32 * sb + 16 * st + 4 * g;
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    float p[4], ds[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float l2 = kDQ ? rL[rt] : sl[i];
                        const float dl = kDQ ? rDelta[rt] : sd[i];
                        const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(s[st][rt][i], sc_mul, -l2));
                        p[i] = srow + i < n_str ? e : 0.f;
                        ds[i] = p[i] * (dp[st][rt][i] - dl);
                        if (kDQ) pdp[rt] = __builtin_fmaf(p[i], dp[st][rt][i], pdp[rt]);
                    }
                    pf[rt][2 * st] = M::pack2(p[0], p[1]);
                    pf[rt][2 * st + 1] = M::pack2(p[2], p[3]);
                    dsf[rt][2 * st] = M::pack2(ds[0], ds[1]);
                    dsf[rt][2 * st + 1] = M::pack2(ds[2], ds[3]);
                }
            }
            // output products: A = transposed streamed image
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const uint32_t to = tr_a + (uint32_t)(32 * sb * kStride * 2 + 32 * dt);
                const frag t1 = read_frag_tr<frag>(img1 + to, 16 * kStride * 2);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) acc1[dt][rt] = M::mfma(t1, as_frag<frag>(dsf[rt]), acc1[dt][rt]);       // dQ^T += K^T dS^T | dK^T += Q^T dS
                if (!kDQ) {
                    const frag t2 = read_frag_tr<frag>(img2 + to, 16 * kStride * 2);
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt) acc2[dt][rt] = M::mfma(t2, as_frag<frag>(pf[rt]), acc2[dt][rt]);    // dV^T += dO^T P
                }
            }
        }
    };

    const int n_tiles = (n_str + kST - 1) / kST;
    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (int t = 0; t < n_tiles; ++t) {
        const bool has_next = t + 1 < n_tiles;
        if (has_next) load_tile((t + 1) * kST);                  // in flight under this tile's products
        compute(t & 1, t * kST);
        if (has_next) store_tile((t + 1) & 1);                   // that buffer was last read in tile t - 1, before the previous barrier
        __syncthreads();
    }

#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const int rrow = rrow0 + 16 * rt;
        if (kDQ) {                                               // the four lane groups hold disjoint keys of the query
            float t = pdp[rt];
            t += __shfl_xor(t, 16);
            t += __shfl_xor(t, 32);
            if (g == 0 && rrow < n_res) delta_out[(b * H + h) * (int64_t)n_res + rrow] = t;
        }
        if (rrow < n_res && (!kDQ || out1 != nullptr)) {
            const int64_t off = (b * n_res + rrow) * hd + (int64_t)h * kD + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const f32x4 a = acc1[dt][rt] * scale;
                const u32x2 w = {M::pack2(a[0], a[1]), M::pack2(a[2], a[3])};
                *reinterpret_cast<u32x2*>(out1 + off + 16 * dt) = w;
                if (!kDQ) {
                    const f32x4 v = acc2[dt][rt];
                    const u32x2 w2 = {M::pack2(v[0], v[1]), M::pack2(v[2], v[3])};
                    *reinterpret_cast<u32x2*>(out2 + off + 16 * dt) = w2;
                }
            }
        }
    }
}

// ---- temporal: one block per (video, token, head); fp32 math on an LDS copy of q, k, v, dout [T][D]
template <typename T> __device__ __forceinline__ float ld_f(const T* p) { return (float)*p; }
template <> __device__ __forceinline__ float ld_f<__hip_bfloat16>(const __hip_bfloat16* p) { return __bfloat162float(*p); }
template <> __device__ __forceinline__ float ld_f<__half>(const __half* p) { return __half2float(*p); }
template <typename T> __device__ __forceinline__ void st_f(T* p, float x) { *p = (T)x; }
template <> __device__ __forceinline__ void st_f<__hip_bfloat16>(__hip_bfloat16* p, float x) { *p = __float2bfloat16(x); }
template <> __device__ __forceinline__ void st_f<__half>(__half* p, float x) { *p = __float2half(x); }
// global -> the LDS copy: to fp32, or as it is where the copy keeps the I/O type
template <typename L, typename T> __device__ __forceinline__ L to_lds(const T* p) {
    if constexpr (std::is_same<L, T>::value) return *p;
    else return ld_f(p);
}

constexpr int kTMax = 32;

// kCap = 16 (T <= 16): 64 threads and an fp32 copy, 18.4 KB at D = 64. kCap = 32 (16 < T <= 32): the fp32 copy would be 41 KB per block
// — three blocks per CU — so a block has 256 threads and a 16-bit input stays 16-bit in LDS (25 KB: six blocks, 24 waves per CU). A
// 16-bit number is an fp32 number: the same formulas on the same values in the same fixed summation order, whatever the thread count.
// Measured at (Bo, T, S, H) = (2, 25, 9216, 5) bf16: 1.92 ms; an fp32 copy with 256 threads 2.41, the 16-bit copy with 128 / 64
// threads 2.04 / 2.82 ('Attention under autograd').
template <typename T, int D, int kCap>
__global__ __launch_bounds__(kCap == 16 ? 64 : 256) void attn_temporal_bwd_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                                 const T* __restrict__ v, const T* __restrict__ dout,
                                                                                 T* __restrict__ dq, T* __restrict__ dk, T* __restrict__ dv,
                                                                                 int Tn, int S, int H, float scale) {
    constexpr int kThreads = kCap == 16 ? 64 : 256;
    using L = typename std::conditional<kCap == 16, float, T>::type;     // element type of the LDS copy
    constexpr int kRow = D + (sizeof(L) == 4 ? 1 : 2);           // rows one bank apart
    __shared__ L s_q[kCap * kRow], s_k[kCap * kRow], s_v[kCap * kRow], s_do[kCap * kRow];
    __shared__ float s_p[kCap * (kCap + 1)], s_ds[kCap * (kCap + 1)];
    const int tid = threadIdx.x;
    const int64_t prob = blockIdx.x;                             // (bo S + s) H + h
    const int h = (int)(prob % H);
    const int64_t bs = prob / H;
    const int64_t s = bs % S, bo = bs / S;
    const int64_t hd = (int64_t)H * D;
    const int64_t base = ((bo * Tn) * S + s) * hd + (int64_t)h * D;      // frame t: + t S hd
    const int64_t fstride = (int64_t)S * hd;
    for (int e = tid; e < Tn * D; e += kThreads) {
        const int t = e / D, d = e % D;
        const int64_t o = base + t * fstride + d;
        s_q[t * kRow + d] = to_lds<L>(q + o);
        s_k[t * kRow + d] = to_lds<L>(k + o);
        s_v[t * kRow + d] = to_lds<L>(v + o);
        s_do[t * kRow + d] = to_lds<L>(dout + o);
    }
    __syncthreads();
    // scores and dP: entry (i, j) per thread, scaled scores into s_p, dP into s_ds
    for (int e = tid; e < Tn * Tn; e += kThreads) {
        const int i = e / Tn, j = e % Tn;
        float a = 0.f, c = 0.f;
#pragma unroll 8
        for (int d = 0; d < D; ++d) {
            a = __builtin_fmaf(ld_f(s_q + i * kRow + d), ld_f(s_k + j * kRow + d), a);
            c = __builtin_fmaf(ld_f(s_do + i * kRow + d), ld_f(s_v + j * kRow + d), c);
        }
        s_p[i * (kCap + 1) + j] = a * scale;
        s_ds[i * (kCap + 1) + j] = c;
    }
    __syncthreads();
    if (tid < Tn) {                                              // one softmax row per thread
        float* const pr = s_p + tid * (kCap + 1);
        float* const dr = s_ds + tid * (kCap + 1);
        float m = pr[0];
        for (int j = 1; j < Tn; ++j) m = fmaxf(m, pr[j]);
        float l = 0.f;
        for (int j = 0; j < Tn; ++j) { const float e = __expf(pr[j] - m); pr[j] = e; l += e; }
        const float inv = 1.0f / l;
        float dl = 0.f;
        for (int j = 0; j < Tn; ++j) { pr[j] *= inv; dl = __builtin_fmaf(pr[j], dr[j], dl); }
        for (int j = 0; j < Tn; ++j) dr[j] = pr[j] * (dr[j] - dl);
    }
    __syncthreads();
    for (int e = tid; e < Tn * D; e += kThreads) {
        const int t = e / D, d = e % D;
        float aq = 0.f, ak = 0.f, av = 0.f;
        for (int j = 0; j < Tn; ++j) {
            aq = __builtin_fmaf(s_ds[t * (kCap + 1) + j], ld_f(s_k + j * kRow + d), aq);      // dQ_t = scale sum_j dS_tj k_j
            ak = __builtin_fmaf(s_ds[j * (kCap + 1) + t], ld_f(s_q + j * kRow + d), ak);      // dK_t = scale sum_i dS_it q_i
            av = __builtin_fmaf(s_p[j * (kCap + 1) + t], ld_f(s_do + j * kRow + d), av);      // dV_t = sum_i P_it dout_i
        }
        const int64_t o = base + t * fstride + d;
        st_f(dq + o, aq * scale);
        st_f(dk + o, ak * scale);
        st_f(dv + o, av);
    }
}

template <typename T>
static int temporal_bwd_launch(const void* q, const void* k, const void* v, const void* dout, void* dq, void* dk, void* dv, int Bo, int Tn,
                               int S, int H, int D, float scale, hipStream_t st) {
    const unsigned grid = (unsigned)((int64_t)Bo * S * H);
#define MVI_TB(DD, CAP)                                                                                                                   \
    hipLaunchKernelGGL((attn_temporal_bwd_kernel<T, DD, CAP>), dim3(grid), dim3(CAP == 16 ? 64 : 256), 0, st, (const T*)q, (const T*)k,  \
                       (const T*)v, (const T*)dout, (T*)dq, (T*)dk, (T*)dv, Tn, S, H, scale)
    if (Tn <= 16) {
        if (D == 16) MVI_TB(16, 16);
        else if (D == 32) MVI_TB(32, 16);
        else MVI_TB(64, 16);
    } else {
        if (D == 16) MVI_TB(16, 32);
        else if (D == 32) MVI_TB(32, 32);
        else MVI_TB(64, 32);
    }
#undef MVI_TB
    return hipGetLastError() == hipSuccess ? 0 : MVI_EHIP;
}

template <typename T>
static int bwd_launch(const void* q, const void* k, const void* v, const void* out, const void* dout, const float* lse, void* dq, void* dk,
                      void* dv, int B, int H, int Sq, int Sk, float scale, bool fold, float* delta, hipStream_t st) {
    // Two deltas. The dQ kernel needs one before it starts: rowsum(dout * out), from the ROUNDED out. On its way it sums P dP in fp32
    // — the same quantity without out's rounding, which on a row whose softmax is one key is all that is left of dP - delta — and
    // the dK/dV kernel, which runs after it, takes that one. (bf16, 33 queries with one peaked row: dk max-norm error 1.65e-2 with the
    // first delta, of which 1.45e-2 are out's rounding.) So the dQ kernel runs whenever dk / dv are asked for, storing dq or not.
    float* const delta_exact = delta + (int64_t)B * H * Sq;
    const int64_t rows = (int64_t)B * Sq * H;
    const int64_t qb = (Sq + kRB - 1) / kRB, kb = (Sk + kRB - 1) / kRB;
    if ((rows + 31) / 32 > 0x7FFFFFFFll || (int64_t)B * H * qb > 0x7FFFFFFFll || (int64_t)B * H * kb > 0x7FFFFFFFll) return MVI_EINVAL;
    hipLaunchKernelGGL((attn_bwd_delta_kernel<T>), dim3((unsigned)((rows + 31) / 32)), dim3(256), 0, st, (const T*)out, (const T*)dout, delta,
                       H, Sq, rows);
    {
        auto kern = fold ? &attn_bwd_kernel<T, true, true> : &attn_bwd_kernel<T, true, false>;
        hipLaunchKernelGGL(kern, dim3((unsigned)(B * H * qb)), dim3(64 * kWaves), 0, st, (const T*)q, (const T*)dout, (const T*)k, (const T*)v,
                           lse, (const float*)delta, (T*)dq, (T*)nullptr, delta_exact, H, Sq, Sk, scale, (int)qb);
    }
    if (dk || dv) {
        auto kern = fold ? &attn_bwd_kernel<T, false, true> : &attn_bwd_kernel<T, false, false>;
        hipLaunchKernelGGL(kern, dim3((unsigned)(B * H * kb)), dim3(64 * kWaves), 0, st, (const T*)k, (const T*)v, (const T*)q, (const T*)dout,
                           lse, (const float*)delta_exact, (T*)dk, (T*)dv, (float*)nullptr, H, Sk, Sq, scale, (int)kb);
    }
    return hipGetLastError() == hipSuccess ? 0 : MVI_EHIP;
}

}  // namespace bwd
}  // namespace mvi

extern "C" int mvi_attention_backward_supported(int32_t Sq, int32_t Sk, int32_t D, int32_t dtype) {
    return (Sq > 0 && (dtype == MVI_DT_BF16 || dtype == MVI_DT_F16) && mvi_attention_kernel_kind(Sq, Sk, D, dtype) == 1) ? 1 : 0;
}

extern "C" size_t mvi_attention_backward_workspace_bytes(int32_t B, int32_t H, int32_t Sq, int32_t Sk, int32_t D, int32_t dtype) {
    if (B <= 0 || H <= 0 || !mvi_attention_backward_supported(Sq, Sk, D, dtype)) return 0;
    return 2 * (size_t)B * H * Sq * sizeof(float);               // delta from the rounded out | delta = rowsum(P dP) (bwd_launch)
}

extern "C" int mvi_attention_backward(const void* q, const void* k, const void* v, const void* out, const void* dout, const void* lse,
                                      void* dq, void* dk, void* dv, int32_t B, int32_t H, int32_t Sq, int32_t Sk, int32_t D, float scale,
                                      int32_t dtype, void* workspace, size_t workspace_bytes, void* stream) {
    if (B < 0 || H <= 0 || Sq < 0 || Sk <= 0 || D <= 0) return mvi::unet_fail(MVI_EINVAL, "attention backward: bad shape");
    if (B == 0 || Sq == 0) return MVI_OK;
    if (!mvi_attention_backward_supported(Sq, Sk, D, dtype))
        return mvi::unet_fail(MVI_EINVAL, "attention backward: bf16 / f16, head dim 64 and more than 32 keys only");
    if (!q || !k || !v || !out || !dout || !lse) return mvi::unet_fail(MVI_EINVAL, "attention backward: NULL pointer");
    if ((dk == nullptr) != (dv == nullptr)) return mvi::unet_fail(MVI_EINVAL, "attention backward: dk and dv come from one kernel, pass both or neither");
    if (!dq && !dk) return MVI_OK;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)dout | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) % 16 != 0 ||
        ((uintptr_t)lse | (uintptr_t)workspace) % 4 != 0)
        return mvi::unet_fail(MVI_EINVAL, "attention backward: tensors must be 16-byte aligned");
    if (!workspace || workspace_bytes < mvi_attention_backward_workspace_bytes(B, H, Sq, Sk, D, dtype))
        return mvi::unet_fail(MVI_EINVAL, "attention backward: workspace too small");
    const bool fold = mvi::attention_folds_scale(mvi_attention_kernel_variant(Sq, Sk, D, dtype), dtype);   // as the forward that wrote lse
    hipStream_t st = (hipStream_t)stream;
    return mvi::dispatch_dtype16(dtype, "attention backward: unknown dtype", [&](auto t) {
        const int rc = mvi::bwd::bwd_launch<typename decltype(t)::type>(q, k, v, out, dout, (const float*)lse, dq, dk, dv, B, H, Sq, Sk, scale, fold, (float*)workspace, st);
        return rc ? mvi::unet_fail(rc, "attention backward: kernel launch failed") : MVI_OK;
    });
}

extern "C" int mvi_attention_temporal_backward(const void* q, const void* k, const void* v, const void* dout, void* dq, void* dk, void* dv,
                                               int32_t Bo, int32_t T, int32_t S, int32_t H, int32_t D, float scale, int32_t dtype, void* stream) {
    if (Bo < 0 || T <= 0 || S <= 0 || H <= 0 || D <= 0) return mvi::unet_fail(MVI_EINVAL, "temporal attention backward: bad shape");
    if (Bo == 0) return MVI_OK;
    if (T > mvi::bwd::kTMax) return mvi::unet_fail(MVI_EINVAL, "temporal attention backward: at most 32 frames");
    if (D != 16 && D != 32 && D != 64) return mvi::unet_fail(MVI_EINVAL, "temporal attention backward: head dim must be 16, 32 or 64");
    if (!q || !k || !v || !dout || !dq || !dk || !dv) return mvi::unet_fail(MVI_EINVAL, "temporal attention backward: NULL pointer");
    if ((int64_t)Bo * S * H > 0x7FFFFFFFll) return mvi::unet_fail(MVI_EINVAL, "temporal attention backward: too many problems");
    hipStream_t st = (hipStream_t)stream;
    return mvi::dispatch_dtype(dtype, "temporal attention backward: unknown dtype", [&](auto t) {
        const int rc = mvi::bwd::temporal_bwd_launch<typename decltype(t)::type>(q, k, v, dout, dq, dk, dv, Bo, T, S, H, D, scale, st);
        return rc ? mvi::unet_fail(rc, "temporal attention backward: kernel launch failed") : MVI_OK;
    });
}
