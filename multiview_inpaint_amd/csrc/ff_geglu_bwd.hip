// Backward of the fused GEGLU feed-forward projection (ff_geglu.hip) for gfx950, contraction length 320, bf16 / f16:
//     h = x W^T + b,  a = h[:, :inner],  g = h[:, inner:],  y = a gelu(g)
//     da = dy g Phi(g),  dg = dy a (Phi(g) + g phi(g)),  dh = [da | dg],  dx = dh W
// As in the forward the [rows, 2 inner] projection never exists: only x, W and b are held between forward and backward, and a block
// recomputes its tile of h on the matrix pipe, gates it in registers and contracts it straight into dx. dx is written once, by one
// block per row, in a fixed order: no atomics, run-to-run identical bits.
//
// Structure — the dQ kernel of attn_bwd.hip with W as the streamed rows and a "head dim" of 320:
//   * block = 8 waves x 16 rows of x, resident in registers as B operands for the whole block (10 k-steps of 32: 40 registers);
//     dx^T of those rows in 20 accumulator tiles (80 registers);
//   * W streams in the forward's tiles of 64 rows — the 32 value rows and the 32 gate rows of the same 32 outputs — through a
//     double-buffered LDS image (global -> registers -> LDS, the next tile in flight under this one's products), rows 656 bytes
//     apart (36 banks, as attn_bwd.hip's 144);
//   * per tile: h^T = W_tile x^T (40 MFMAs, bias as the accumulators' start), the gate in fp32 from the unrounded a, g and dy
//     (geglu_math.h), one rounding of da / dg to the I/O type as MFMA operands, dx^T += W_tile^T dh^T (40 MFMAs; dh^T leaves the
//     accumulators as the B operand without a shuffle, the A operand is the same LDS image read transposed, ds_read_b64_tr_b16).
// v_mfma_f32_16x16x32, lane = (c = lane & 15, g = lane >> 4):
//   h^T tile st (W rows 16 st .. + 15 of the image; st 0, 1 value, st 2, 3 gate): C/D register i of lane (c, g) = [W row 16 st + 4 g + i][x row c]
//   B operand of the contraction over 32 W rows (value rows, then gate rows): element j of lane (c, g) is row (j < 4 ? 4 g + j : 16 + 4 g + j - 4)
//   dx^T tile dt: register i of lane (c, g) = dx[x row c][16 dt + 4 g + i]: one 8-byte store per tile.
// kStoreDh: also writes dh [rows, 2 inner] in the I/O type (the SAME rounded values the contraction used) for the caller's
// dweight = dh^T x and dbias = colsum(dh); without it nothing tensor-sized is written besides dx. kDx = false (dx NULL: x does not
// require grad, the parameters do): recomputation, gate and the dh store only, no contraction.
// Ragged last block: rows past the end load the last valid row (x, dy) and store nothing. No lane is masked around a transposed read.
#include <cstdint>
#include <type_traits>

#include "geglu_math.h"
#include "mfma_common.h"
#include "unet_host.h"

namespace mvi {
namespace ffb {

constexpr int kK = 320;
constexpr int kKS = kK / 32;                    // k-steps of the recomputation
constexpr int kDT = kK / 16;                    // dx^T tiles
constexpr int kWaves = 8;
constexpr int kRB = 16 * kWaves;                // x rows per block
constexpr int kStep = 32;                       // outputs per tile
constexpr int kTR = 2 * kStep;                  // W rows per tile
constexpr int kStride = 328;                    // LDS row stride in elements (656 bytes)
constexpr int kImg = kTR * kStride * 2;         // 41984 bytes
constexpr int kPieces = kTR * (kK / 8) / (64 * kWaves);     // 16-byte pieces of a tile per thread: 5

template <typename T> using Mma = MmaBuiltin16<T>;

template <typename T, bool kStoreDh, bool kDx>
__global__ __launch_bounds__(64 * kWaves) __attribute__((amdgpu_waves_per_eu(2, 2)))
void ff_geglu_bwd_kernel(const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ bias, const T* __restrict__ dy,
                         T* __restrict__ dx, T* __restrict__ dh, int64_t rows, int inner, int64_t x_rs, int64_t dy_rs, int64_t dx_rs,
                         int64_t dh_rs) {
    using M = Mma<T>;
    using frag = typename M::frag;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    MVI_AS3 char* const lds = (MVI_AS3 char*)smem;
    MVI_AS3 float* const lbias = (MVI_AS3 float*)(lds + 2 * kImg);      // [2 inner]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, g = lane >> 4;
    const int64_t row = (int64_t)blockIdx.x * kRB + wave * 16 + c16;
    const bool ok = row < rows;
    const int64_t rowc = ok ? row : rows - 1;

    for (int i = tid; i < 2 * inner; i += 64 * kWaves) lbias[i] = bias ? bias[i] : 0.f;

    // ---- resident x: element j of lane (c, g), k-step ks: x[row][32 ks + 8 g + j]
    frag xf[kKS];
    {
        const T* const xp = x + rowc * x_rs + 8 * g;
#pragma unroll
        for (int ks = 0; ks < kKS; ++ks) xf[ks] = as_frag<frag>(*reinterpret_cast<const u32x4*>(xp + 32 * ks));
    }

    // ---- W tiles: global -> registers -> LDS; piece p = tid + 512 i is (image row p / 40, 16-byte chunk p % 40)
    int64_t w_off[kPieces];
    uint32_t l_off[kPieces];
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
        const int p = tid + 64 * kWaves * i;
        const int r = p / (kK / 8), ch = p - r * (kK / 8);
        w_off[i] = (int64_t)(r < kStep ? r : inner + r - kStep) * kK + 8 * ch;
        l_off[i] = (uint32_t)((r * kStride + 8 * ch) * 2);
    }
    const T* const dyp = dy + rowc * dy_rs + 4 * g;              // + 32 t + 16 st: the lane's four outputs of h^T tile st
    u32x4 pw[kPieces];
    u32x2 dyn[2], dyc[2];
    auto load_tile = [&](int t) __attribute__((always_inline)) {
        const T* const wt = w + (int64_t)t * (kStep * kK);
#pragma unroll
        for (int i = 0; i < kPieces; ++i) pw[i] = *reinterpret_cast<const u32x4*>(wt + w_off[i]);
#pragma unroll
        for (int st = 0; st < 2; ++st) dyn[st] = *reinterpret_cast<const u32x2*>(dyp + kStep * t + 16 * st);
    };
    auto store_tile = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kPieces; ++i) *reinterpret_cast<u32x4*>(smem + buf * kImg + l_off[i]) = pw[i];
    };

    // ---- LDS read addressing (byte offsets inside one image), as attn_bwd.hip
    const uint32_t row_a = (uint32_t)((c16 * kStride + 8 * g) * 2);                                  // image row 16 st + c, elements 32 ks + 8 g ..
    const uint32_t tr_a = (uint32_t)(((4 * g + (c16 >> 2)) * kStride + 4 * (c16 & 3)) * 2);          // 4-row x 16-column block, transposed

    f32x4 acc[kDT];
#pragma unroll
    for (int dt = 0; dt < kDT; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    char* const dhp = kStoreDh ? reinterpret_cast<char*>(dh + rowc * dh_rs + 4 * g) : nullptr;

    auto compute = [&](int buf, int t) __attribute__((always_inline)) {
        MVI_AS3 char* const img = lds + buf * kImg;
        // recompute: h^T = W_tile x^T + b
        f32x4 h[4];
#pragma unroll
        for (int st = 0; st < 4; ++st)
            h[st] = *reinterpret_cast<MVI_AS3 const f32x4*>(lbias + (st < 2 ? 0 : inner) + kStep * t + 16 * (st & 1) + 4 * g);
#pragma unroll
        for (int ks = 0; ks < kKS; ++ks)
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const u32x4 a = *reinterpret_cast<MVI_AS3 const u32x4*>(img + row_a + (uint32_t)(16 * st * kStride * 2) + 64 * ks);
                h[st] = M::mfma(as_frag<frag>(a), xf[ks], h[st]);
            }
        // gate: da, dg in fp32, rounded once, as B operands
        u32x4 daf, dgf;
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const float d4[4] = {M::lo(dyc[st][0]), M::hi(dyc[st][0]), M::lo(dyc[st][1]), M::hi(dyc[st][1])};
            float da[4], dg[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) geglu_grad(h[st][i], h[2 + st][i], d4[i], da[i], dg[i]);
            daf[2 * st] = M::pack2(da[0], da[1]);
            daf[2 * st + 1] = M::pack2(da[2], da[3]);
            dgf[2 * st] = M::pack2(dg[0], dg[1]);
            dgf[2 * st + 1] = M::pack2(dg[2], dg[3]);
        }
        if (kStoreDh && ok) {
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                char* const p = dhp + (kStep * t + 16 * st) * 2;
                *reinterpret_cast<u32x2*>(p) = u32x2{daf[2 * st], daf[2 * st + 1]};
                *reinterpret_cast<u32x2*>(p + (int64_t)inner * 2) = u32x2{dgf[2 * st], dgf[2 * st + 1]};
            }
        }
        // contract: dx^T += W_tile^T dh^T (value rows with da, gate rows with dg)
#pragma unroll
        for (int dt = 0; dt < (kDx ? kDT : 0); ++dt) {
#pragma unroll
            for (int sb = 0; sb < 2; ++sb) {
                const uint32_t to = tr_a + (uint32_t)(32 * sb * kStride * 2 + 32 * dt);
                const frag wt = read_frag_tr<frag>(img + to, 16 * kStride * 2);
                acc[dt] = M::mfma(wt, as_frag<frag>(sb ? dgf : daf), acc[dt]);
            }
        }
    };

    const int n_tiles = inner / kStep;
    load_tile(0);
    store_tile(0);
    __syncthreads();                                             // tile 0 and the bias vector are in LDS
    for (int t = 0; t < n_tiles; ++t) {
        const bool has_next = t + 1 < n_tiles;
        dyc[0] = dyn[0];
        dyc[1] = dyn[1];
        if (has_next) load_tile(t + 1);                          // in flight under this tile's products
        compute(t & 1, t);
        if (has_next) store_tile((t + 1) & 1);                   // that buffer was last read in tile t - 1, before the previous barrier
        __syncthreads();
    }

    if (kDx && ok) {
        T* const op = dx + row * dx_rs + 4 * g;
#pragma unroll
        for (int dt = 0; dt < kDT; ++dt) {
            const f32x4 a = acc[dt];
            *reinterpret_cast<u32x2*>(op + 16 * dt) = u32x2{M::pack2(a[0], a[1]), M::pack2(a[2], a[3])};
        }
    }
}

template <typename T, bool kStoreDh, bool kDx>
static int launch(const void* x, const void* w, const float* bias, const void* dy, void* dx, void* dh, int64_t rows, int inner, int64_t x_rs,
                  int64_t dy_rs, int64_t dx_rs, int64_t dh_rs, hipStream_t st) {
    const int64_t n_blocks = (rows + kRB - 1) / kRB;
    if (n_blocks > 0x7FFFFFFFll) return MVI_EINVAL;
    const int lds_bytes = 2 * kImg + 2 * inner * (int)sizeof(float);
    constexpr auto kern = &ff_geglu_bwd_kernel<T, kStoreDh, kDx>;
    if (allow_large_lds<kern>(160 * 1024)) return MVI_EHIP;
    hipLaunchKernelGGL(kern,dim3((unsigned)n_blocks), dim3(64 * kWaves), lds_bytes, st, (const T*)x, (const T*)w, bias, (const T*)dy, (T*)dx,
                       (T*)dh, rows, inner, x_rs, dy_rs, dx_rs, dh_rs);
    return hipGetLastError() == hipSuccess ? 0 : MVI_EHIP;
}

}  // namespace ffb
}  // namespace mvi

extern "C" int mvi_ff_geglu_backward_supported(int32_t K, int32_t inner, int32_t dtype) {
    return mvi_ff_geglu_supported(K, inner, dtype) && 2 * mvi::ffb::kImg + 2 * (int64_t)inner * 4 <= 160 * 1024;
}

extern "C" int mvi_ff_geglu_backward(const void* x, const void* weight, const float* bias, const void* dy, void* dx, void* dh, int64_t rows,
                                     int32_t K, int32_t inner, int64_t x_row_stride, int64_t dy_row_stride, int64_t dx_row_stride,
                                     int64_t dh_row_stride, int32_t dtype, void* stream) {
    if (rows < 0 || !mvi_ff_geglu_backward_supported(K, inner, dtype))
        return mvi::unet_fail(MVI_EINVAL, "ff_geglu backward: needs K = 320, inner a multiple of 32 (64 ... 4864), bf16 or f16");
    if (rows == 0) return MVI_OK;
    if (!x || !weight || !dy || (!dx && !dh)) return mvi::unet_fail(MVI_EINVAL, "ff_geglu backward: NULL pointer");
    if (x_row_stride < K || dy_row_stride < inner || x_row_stride % 8 || dy_row_stride % 4 ||
        (dx && (dx_row_stride < K || dx_row_stride % 4)) || ((uintptr_t)x | (uintptr_t)weight) % 16 || ((uintptr_t)dy | (uintptr_t)dx) % 8)
        return mvi::unet_fail(MVI_EINVAL, "ff_geglu backward: rows must be 16-byte aligned (x, weight) / 8-byte aligned (dy, dx)");
    if (dh && (dh_row_stride < 2 * (int64_t)inner || dh_row_stride % 4 || (uintptr_t)dh % 8))
        return mvi::unet_fail(MVI_EINVAL, "ff_geglu backward: dh needs rows of at least 2 inner elements, 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    using namespace mvi::ffb;
    int rc;
#define MVI_FFB_LAUNCH(T, DH, DX) \
    launch<T, DH, DX>(x, weight, bias, dy, dx, dh, rows, inner, x_row_stride, dy_row_stride, dx_row_stride, dh_row_stride, st)
    if (dtype == MVI_DT_BF16)
        rc = !dx ? MVI_FFB_LAUNCH(__hip_bfloat16, true, false) : dh ? MVI_FFB_LAUNCH(__hip_bfloat16, true, true) : MVI_FFB_LAUNCH(__hip_bfloat16, false, true);
    else
        rc = !dx ? MVI_FFB_LAUNCH(__half, true, false) : dh ? MVI_FFB_LAUNCH(__half, true, true) : MVI_FFB_LAUNCH(__half, false, true);
#undef MVI_FFB_LAUNCH
    return rc ? mvi::unet_fail(rc, "ff_geglu backward: kernel launch failed") : MVI_OK;
}
