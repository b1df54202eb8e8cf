// What does one vector instruction cost to ISSUE on an MI355X SIMD? (DESIGN.md §8 item 3 counted every vector instruction of
// render_backward_kernel as 4 cycles.) Every wave runs a long unrolled stream of INDEPENDENT instructions of one kind (16
// destination registers in turn: a register is re-read 16 instructions after it was written) and records the shader clock
// (s_memtime) around it and the ABSOLUTE 100 MHz clock (s_memrealtime) at its start and end. Streams: v_fma_f32, v_pk_fma_f32,
// v_pk_mul_f32, v_exp_f32, v_rcp_f32, v_add_f32_dpp, and s_nop 1 + v_add_f32_dpp (the form of the quad steps of wave_sum9).
// Each at ONE and at FIVE waves per SIMD on every CU: a block is 256 threads (one wave per SIMD) and asks for so much LDS that
// one or five blocks fit a CU; the grid is exactly what is resident at once, and the blocks wait for each other at the start
// (a counter in memory, given up after 200 us: never a hang) so that the waves of a SIMD run their streams together.
// What a SIMD pays is NOT one wave's cycles divided by five unless the five ran together: it is measured per SIMD (HW_ID) from
// the waves' absolute times, over the SIMDs that hold exactly the intended number of waves: instructions of all its waves over
// the span from the first start to the last end, with the share of that span in which all of them ran beside it.
// Build: hipcc -O2 --offload-arch=gfx950 tools/experiments/valu_issue_probe.cpp -o tools/experiments/valu_issue_probe
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

typedef float f2v __attribute__((ext_vector_type(2)));
constexpr int kPerIter = 128;             // instructions of the stream per loop iteration (8 x 16)
constexpr int kIters = 2048;              // 262144 instructions per wave

#define R16(OP) OP("%0") OP("%1") OP("%2") OP("%3") OP("%4") OP("%5") OP("%6") OP("%7") OP("%8") OP("%9") OP("%10") OP("%11") \
    OP("%12") OP("%13") OP("%14") OP("%15")
#define R128(OP) R16(OP) R16(OP) R16(OP) R16(OP) R16(OP) R16(OP) R16(OP) R16(OP)
#define ACC(a) "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), "+v"(a[8]), \
    "+v"(a[9]), "+v"(a[10]), "+v"(a[11]), "+v"(a[12]), "+v"(a[13]), "+v"(a[14]), "+v"(a[15])
#define OP_FMA(r) "v_fma_f32 " r ", " r ", %16, %17\n\t"
#define OP_PKFMA(r) "v_pk_fma_f32 " r ", " r ", %16, %17\n\t"
#define OP_PKMUL(r) "v_pk_mul_f32 " r ", " r ", %16\n\t"
#define OP_EXP(r) "v_exp_f32 " r ", %16\n\t"
#define OP_RCP(r) "v_rcp_f32 " r ", %16\n\t"
#define OP_DPP(r) "v_add_f32_dpp " r ", " r ", " r " row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
#define OP_NOPDPP(r) "s_nop 1\n\t" OP_DPP(r)

enum { kFma, kPkFma, kPkMul, kExp, kRcp, kDpp, kNopDpp, kModes };
static const char* kName[kModes] = {"v_fma_f32", "v_pk_fma_f32", "v_pk_mul_f32", "v_exp_f32", "v_rcp_f32", "v_add_f32_dpp",
                                    "s_nop 1 + v_add_f32_dpp"};

template <int MODE>
__global__ __launch_bounds__(256) void stream_kernel(uint64_t* __restrict__ rec, float* __restrict__ sink, unsigned* arrived) {
    extern __shared__ float lds[];        // only its size matters: it sets how many blocks share a CU
    float a[16];
    f2v p[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { a[i] = 0.0f; p[i] = f2v{1.0f, 1.0f}; }
    const float c0 = 0.5f, c1 = 1.0f;     // x <- 0.5 x + 1 stays finite; exp / rcp read a constant; the DPP sums stay 0
    const f2v q0 = {0.5f, 0.5f}, q1 = {1.0f, 1.0f};
    if (threadIdx.x == 0) {                // start together: every block of the grid is resident, or the wait ends after 200 us
        __hip_atomic_fetch_add(arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint64_t w0 = __builtin_amdgcn_s_memrealtime();
        while (__hip_atomic_load(arrived, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < gridDim.x &&
               __builtin_amdgcn_s_memrealtime() - w0 < 20000) __builtin_amdgcn_s_sleep(8);
    }
    __syncthreads();
    const uint64_t t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < kIters; ++it) {
        if (MODE == kFma) asm volatile(R128(OP_FMA) : ACC(a) : "v"(c0), "v"(c1));
        if (MODE == kPkFma) asm volatile(R128(OP_PKFMA) : ACC(p) : "v"(q0), "v"(q1));
        if (MODE == kPkMul) asm volatile(R128(OP_PKMUL) : ACC(p) : "v"(q1));
        if (MODE == kExp) asm volatile(R128(OP_EXP) : ACC(a) : "v"(c0));
        if (MODE == kRcp) asm volatile(R128(OP_RCP) : ACC(a) : "v"(c0));
        if (MODE == kDpp) asm volatile(R128(OP_DPP) : ACC(a));
        if (MODE == kNopDpp) asm volatile(R128(OP_NOPDPP) : ACC(a));
    }
    const uint64_t t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += a[i] + p[i].x + p[i].y;
    if (s == 12345.678f) { lds[threadIdx.x] = s; sink[threadIdx.x] = lds[threadIdx.x ^ 1]; }
    if ((threadIdx.x & 63) == 0) {
        uint64_t* r = rec + 5 * ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6));
        r[0] = t1 - t0;
        r[1] = r0;
        r[2] = r1;
        r[3] = __builtin_amdgcn_s_getreg((31 << 11) | 4);     // HW_ID
        r[4] = __builtin_amdgcn_s_getreg((31 << 11) | 20);    // XCC_ID
    }
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <int MODE>
int run(int n_cu, int per_simd, uint64_t* d, float* sink, unsigned* arrived) {
    // LDS per block so that exactly per_simd blocks fit the CU's 160 KB (one: 96 KB; five: 30 KB. With 32 KB only four of the five
    // were resident at once: the fifth ran alone afterwards, which the shares of the span showed)
    const size_t lds = per_simd == 1 ? 96 * 1024 : (160 * 1024) / per_simd - 2048;
    CHECK(hipFuncSetAttribute((const void*)stream_kernel<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int blocks = n_cu * per_simd;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    float ms = 0.f;
    for (int rep = 0; rep < 2; ++rep) {                          // the first launch loads the code object
        CHECK(hipMemsetAsync(arrived, 0, sizeof(unsigned), 0));
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(stream_kernel<MODE>, dim3(blocks), dim3(256), lds, 0, d, sink, arrived);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&ms, e0, e1));
    }
    CHECK(hipGetLastError());
    std::vector<uint64_t> r((size_t)blocks * 4 * 5);
    CHECK(hipMemcpy(r.data(), d, r.size() * 8, hipMemcpyDeviceToHost));
    const double n_inst = (double)kPerIter * kIters;
    std::vector<double> cyc, ghz;
    struct Simd { int n = 0; uint64_t first = ~0ull, last_start = 0, first_end = ~0ull, last = 0; };
    std::map<uint32_t, Simd> per;                                // waves per (XCD, SE, SH, CU, SIMD)
    for (int w = 0; w < blocks * 4; ++w) {
        const uint64_t* q = &r[5 * (size_t)w];
        cyc.push_back((double)q[0]);
        ghz.push_back((double)q[0] / ((double)(q[2] - q[1]) * 10.0));
        Simd& s = per[((uint32_t)(q[4] & 15) << 16) | ((uint32_t)q[3] & 0xfff0u)];
        s.n++; s.first = std::min(s.first, q[1]); s.last_start = std::max(s.last_start, q[1]);
        s.first_end = std::min(s.first_end, q[2]); s.last = std::max(s.last, q[2]);
    }
    std::sort(cyc.begin(), cyc.end()); std::sort(ghz.begin(), ghz.end());
    const double clk = ghz[ghz.size() / 2];
    std::vector<double> span_cyc, together;
    int mx = 0;
    for (auto& kv : per) {
        const Simd& s = kv.second;
        mx = std::max(mx, s.n);
        if (s.n != per_simd) continue;
        const double span = (double)(s.last - s.first) * 10.0;                   // ns
        span_cyc.push_back(span * clk / (n_inst * s.n));
        together.push_back(s.first_end > s.last_start ? (double)(s.first_end - s.last_start) * 10.0 / span : 0.0);
    }
    if (span_cyc.empty()) { printf("%-24s %d wave(s)/SIMD: no SIMD holds exactly %d waves\n", kName[MODE], per_simd, per_simd); return 0; }
    std::sort(span_cyc.begin(), span_cyc.end()); std::sort(together.begin(), together.end());
    printf("%-24s %d wave(s)/SIMD: per SIMD %6.3f cyc/inst (min %6.3f max %6.3f over %zu SIMDs with exactly %d waves; all of them "
           "running for %.3f of the span, median, min %.3f); per wave %7.3f cyc/inst (min %7.3f max %7.3f); %.2f GHz; wall %8.1f us "
           "= %6.3f ns/inst per SIMD; %zu SIMDs hold waves, at most %d on one\n",
           kName[MODE], per_simd, span_cyc[span_cyc.size() / 2], span_cyc.front(), span_cyc.back(), span_cyc.size(), per_simd,
           together[together.size() / 2], together.front(), cyc[cyc.size() / 2] / n_inst, cyc.front() / n_inst, cyc.back() / n_inst,
           clk, ms * 1e3, ms * 1e6 / n_inst / per_simd, per.size(), mx);
    return 0;
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int n_cu = prop.multiProcessorCount;
    printf("%s, %d CUs; %d instructions per wave and stream\n", prop.name, n_cu, kPerIter * kIters);
    uint64_t* d; float* sink; unsigned* arrived;
    CHECK(hipMalloc(&d, (size_t)n_cu * 5 * 4 * 5 * sizeof(uint64_t))); CHECK(hipMalloc(&sink, 4096)); CHECK(hipMalloc(&arrived, sizeof(unsigned)));
    for (int per_simd : {1, 5}) {
        if (run<kFma>(n_cu, per_simd, d, sink, arrived) || run<kPkFma>(n_cu, per_simd, d, sink, arrived) || run<kPkMul>(n_cu, per_simd, d, sink, arrived) ||
            run<kExp>(n_cu, per_simd, d, sink, arrived) || run<kRcp>(n_cu, per_simd, d, sink, arrived) || run<kDpp>(n_cu, per_simd, d, sink, arrived) ||
            run<kNopDpp>(n_cu, per_simd, d, sink, arrived)) return 1;
    }
    return 0;
}
