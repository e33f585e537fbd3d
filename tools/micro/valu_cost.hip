// Micro-benchmark: what one wave64 VALU instruction costs the SIMD's pipe, per opcode, on gfx950.
// (Prices the path kernel's loop: tools/pmc_summary.py's valu_busy takes every VALU instruction at the
// cost of an fma, which its docstring calls a lower bound.)
//
// One register-only kernel per instruction: four independent chains per lane, 16 x 4 instructions per
// unrolled run, one-wave groups.  The launch is sized to 1, 2, 4 and 8 resident waves per SIMD: 4 W groups
// per CU, held there (below 8) by a dynamic LDS allocation of 1 / (4 W) of the CU's 160 KiB each.  Every wave
// stamps s_memtime (shader cycles) around the middle half of its run, when every wave of the launch is
// resident; the report is the median over waves of
//   wave   = elapsed / instructions           what one wave sees per instruction (latency-bound at W = 1)
// A SIMD serves its oldest waves first, so with the pipe full the younger ones wait and "wave" stops
// growing with W; the pipe's price is taken from the whole launch instead:
//   simd   = the launch's span in cycles / instructions issued per SIMD
// with the span from the waves' own s_memrealtime stamps (first start to last end) and the clock from
// their s_memtime / s_memrealtime ratio; as a cross-check, the same from the kernel's HIP-event time
// and the device's clock attribute.
//   hipcc --offload-arch=gfx950 -O2 tools/micro/valu_cost.hip -o tools/micro/valu_cost && tools/micro/valu_cost
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

constexpr uint32_t kUnroll = 16, kChains = 4;
constexpr uint32_t kOut = 4;  // words a wave writes

// the chains' registers: four 32-bit values, four 64-bit values, and constant operands
struct Regs {
    uint32_t a0, a1, a2, a3, b, c;
    uint64_t w0, w1, w2, w3, bw;
    uint32_t s0, s1, s2, s3;  // scalar results (v_readfirstlane)
    uint64_t m;               // a lane mask in a scalar pair
};

// one instruction on each of the four chains
#define OP32(NAME, TEXT)                                                               \
    struct NAME {                                                                      \
        static constexpr const char* name = #NAME;                                     \
        static __device__ __forceinline__ void step(Regs& r) {                         \
            asm volatile(TEXT : "+v"(r.a0) : "v"(r.b), "v"(r.c) : "vcc");              \
            asm volatile(TEXT : "+v"(r.a1) : "v"(r.b), "v"(r.c) : "vcc");              \
            asm volatile(TEXT : "+v"(r.a2) : "v"(r.b), "v"(r.c) : "vcc");              \
            asm volatile(TEXT : "+v"(r.a3) : "v"(r.b), "v"(r.c) : "vcc");              \
        }                                                                              \
    }
// ... on the 64-bit chains, with the 32-bit constants and the 64-bit one as %1, %2, %3
#define OP64(NAME, TEXT)                                                               \
    struct NAME {                                                                      \
        static constexpr const char* name = #NAME;                                     \
        static __device__ __forceinline__ void step(Regs& r) {                         \
            asm volatile(TEXT : "+v"(r.w0) : "v"(r.b), "v"(r.c), "v"(r.bw) : "vcc");   \
            asm volatile(TEXT : "+v"(r.w1) : "v"(r.b), "v"(r.c), "v"(r.bw) : "vcc");   \
            asm volatile(TEXT : "+v"(r.w2) : "v"(r.b), "v"(r.c), "v"(r.bw) : "vcc");   \
            asm volatile(TEXT : "+v"(r.w3) : "v"(r.b), "v"(r.c), "v"(r.bw) : "vcc");   \
        }                                                                              \
    }
// ... a 32-bit result (%0) from a 64-bit chain value (%1) and the reverse: no chain through the result,
// the four instructions are independent of each other and of the run before
#define OP_NARROW(NAME, TEXT)                                                          \
    struct NAME {                                                                      \
        static constexpr const char* name = #NAME;                                     \
        static __device__ __forceinline__ void step(Regs& r) {                         \
            asm volatile(TEXT : "=v"(r.a0) : "v"(r.w0), "v"(r.bw) : "vcc");            \
            asm volatile(TEXT : "=v"(r.a1) : "v"(r.w1), "v"(r.bw) : "vcc");            \
            asm volatile(TEXT : "=v"(r.a2) : "v"(r.w2), "v"(r.bw) : "vcc");            \
            asm volatile(TEXT : "=v"(r.a3) : "v"(r.w3), "v"(r.bw) : "vcc");            \
        }                                                                              \
    }
#define OP_WIDEN(NAME, TEXT)                                                           \
    struct NAME {                                                                      \
        static constexpr const char* name = #NAME;                                     \
        static __device__ __forceinline__ void step(Regs& r) {                         \
            asm volatile(TEXT : "=v"(r.w0) : "v"(r.a0));                               \
            asm volatile(TEXT : "=v"(r.w1) : "v"(r.a1));                               \
            asm volatile(TEXT : "=v"(r.w2) : "v"(r.a2));                               \
            asm volatile(TEXT : "=v"(r.w3) : "v"(r.a3));                               \
        }                                                                              \
    }
#define OP_SCALAR(NAME, TEXT)                                                          \
    struct NAME {                                                                      \
        static constexpr const char* name = #NAME;                                     \
        static __device__ __forceinline__ void step(Regs& r) {                         \
            asm volatile(TEXT : "=s"(r.s0) : "v"(r.a0));                               \
            asm volatile(TEXT : "=s"(r.s1) : "v"(r.a1));                               \
            asm volatile(TEXT : "=s"(r.s2) : "v"(r.a2));                               \
            asm volatile(TEXT : "=s"(r.s3) : "v"(r.a3));                               \
        }                                                                              \
    }

OP32(v_fma_f32, "v_fma_f32 %0, %0, %1, %2");
OP32(v_mul_f32, "v_mul_f32 %0, %0, %1");
OP32(v_add_f32, "v_add_f32 %0, %0, %1");
OP32(v_add_u32, "v_add_u32 %0, %0, %1");
OP32(v_mov_b32, "v_mov_b32 %0, %1");
OP32(v_mul_lo_u32, "v_mul_lo_u32 %0, %0, %1");
OP32(v_mul_hi_u32, "v_mul_hi_u32 %0, %0, %1");
OP64(v_mad_u64_u32, "v_mad_u64_u32 %0, vcc, %1, %2, %0");
OP32(v_mad_u32_u24, "v_mad_u32_u24 %0, %0, %1, %2");
OP32(v_lshl_add_u32, "v_lshl_add_u32 %0, %0, 1, %1");
OP64(v_lshl_add_u64, "v_lshl_add_u64 %0, %0, 1, %3");
OP32(v_add3_u32, "v_add3_u32 %0, %0, %1, %2");
OP32(v_alignbit_b32, "v_alignbit_b32 %0, %0, %1, 7");
OP32(v_rcp_f32, "v_rcp_f32 %0, %0");
OP32(v_rsq_f32, "v_rsq_f32 %0, %0");
OP32(v_sqrt_f32, "v_sqrt_f32 %0, %0");
OP32(v_sin_f32, "v_sin_f32 %0, %0");
OP32(v_cos_f32, "v_cos_f32 %0, %0");
OP_WIDEN(v_cvt_f64_u32, "v_cvt_f64_u32 %0, %1");
OP64(v_mul_f64, "v_mul_f64 %0, %0, %3");
OP_NARROW(v_cvt_u32_f64, "v_cvt_u32_f64 %0, %1");
OP_NARROW(v_cmp_lt_u64, "v_cmp_lt_u64 vcc, %1, %2");
// (the mask from a scalar pair; vcc is left to the compiler, which declares nothing about it here)
struct v_cndmask_b32 {
    static constexpr const char* name = "v_cndmask_b32";
    static __device__ __forceinline__ void step(Regs& r) {
        asm volatile("v_cndmask_b32 %0, %0, %1, %2" : "+v"(r.a0) : "v"(r.b), "s"(r.m));
        asm volatile("v_cndmask_b32 %0, %0, %1, %2" : "+v"(r.a1) : "v"(r.b), "s"(r.m));
        asm volatile("v_cndmask_b32 %0, %0, %1, %2" : "+v"(r.a2) : "v"(r.b), "s"(r.m));
        asm volatile("v_cndmask_b32 %0, %0, %1, %2" : "+v"(r.a3) : "v"(r.b), "s"(r.m));
    }
};
OP_SCALAR(v_readfirstlane_b32, "v_readfirstlane_b32 %0, %1");

template <class Op>
__global__ void __launch_bounds__(64) k(uint64_t* out, uint32_t iters, float seed) {
    extern __shared__ uint32_t hold[];  // never touched: its size sets how many groups a CU takes
    const uint32_t lane = threadIdx.x;
    Regs r;
    r.a0 = __float_as_uint(seed + lane * 0.001f);
    r.a1 = __float_as_uint(seed + lane * 0.002f);
    r.a2 = __float_as_uint(seed + lane * 0.003f);
    r.a3 = __float_as_uint(seed + lane * 0.004f);
    r.b = __float_as_uint(0.9990234375f);
    r.c = __float_as_uint(0.0009765625f);
    r.w0 = (uint64_t)__double_as_longlong(1.0 + lane * 0.001);
    r.w1 = (uint64_t)__double_as_longlong(1.0 + lane * 0.002);
    r.w2 = (uint64_t)__double_as_longlong(1.0 + lane * 0.003);
    r.w3 = (uint64_t)__double_as_longlong(1.0 + lane * 0.004);
    r.bw = (uint64_t)__double_as_longlong(0.9990234375);
    r.s0 = r.s1 = r.s2 = r.s3 = 0;
    r.m = 0x5555aaaa0f0f3333ull ^ (uint64_t)iters;
    // the stamps bracket the middle half of the run: the launch's first waves run beside empty slots
    // until the dispatcher has placed the last ones, and the last ones beside slots already drained
    uint64_t t0 = 0, t1 = 0;
    const uint64_t ta = __builtin_amdgcn_s_memtime(), ra = __builtin_amdgcn_s_memrealtime();
    for (uint32_t i = 0; i < iters; i++) {
        if (i == iters / 4) t0 = __builtin_amdgcn_s_memtime();
        if (i == iters - iters / 4) t1 = __builtin_amdgcn_s_memtime();
#pragma unroll
        for (uint32_t u = 0; u < kUnroll; u++) Op::step(r);
    }
    const uint64_t tb = __builtin_amdgcn_s_memtime(), rb = __builtin_amdgcn_s_memrealtime();
    // (the results are read, so no chain is dead; nothing is stored unless they hit one bit pattern)
    const uint64_t x = r.a0 ^ r.a1 ^ r.a2 ^ r.a3 ^ r.w0 ^ r.w1 ^ r.w2 ^ r.w3 ^ r.s0 ^ r.s1 ^ r.s2 ^ r.s3;
    if (lane == 0) {
        uint64_t* o = out + (size_t)blockIdx.x * kOut;
        o[0] = t1 - t0;  // the middle half
        o[1] = tb - ta;  // the whole run
        o[2] = ra;       // ... and on the 100 MHz counter that every wave reads alike
        o[3] = rb;
    }
    if (x == 0x123456789abcdef0ull) out[(size_t)blockIdx.x * kOut] = x;
}

constexpr int kW = 4;
static const uint32_t kWaves[kW] = {1, 2, 4, 8};
struct Row { const char* name; double wave[kW], simd[kW], ev, mhz; };

template <class Op>
static int run(uint64_t* d_out, uint32_t n_cu, double mhz, std::vector<Row>& rows) {
    const uint32_t iters = 8192;
    const double n_inst = (double)(iters / 2) * kUnroll * kChains;  // between the stamps
    Row row{Op::name, {}, {}, 0.0, 0.0};
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int wi = 0; wi < kW; wi++) {
        const uint32_t W = kWaves[wi], groups = n_cu * 4 * W;
        // 4 W groups fill the CU's LDS, one more does not fit; at 8 the CU's 32 wave slots are the limit
        const uint32_t lds = W < 8 ? 160u * 1024u / (4 * W) : 0u;
        std::vector<uint64_t> h((size_t)groups * kOut);
        float ms = 0;
        for (int rep = 0; rep < 2; rep++) {  // the first launch loads the code
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL(k<Op>, dim3(groups), dim3(64), lds, 0, d_out, iters, 1.0f);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            CK(hipEventElapsedTime(&ms, e0, e1));
        }
        CK(hipMemcpy(h.data(), d_out, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        std::vector<uint64_t> mid(groups);
        uint64_t first = ~0ull, last = 0;
        double ticks = 0, real = 0;
        for (uint32_t g = 0; g < groups; g++) {
            const uint64_t* o = &h[(size_t)g * kOut];
            mid[g] = o[0];
            first = std::min(first, o[2]);
            last = std::max(last, o[3]);
            ticks += (double)o[1];
            real += (double)(o[3] - o[2]);
        }
        std::sort(mid.begin(), mid.end());
        row.wave[wi] = (double)mid[groups / 2] / n_inst;
        // the launch's span, first wave's start to last wave's end, in shader cycles at the clock the
        // waves saw, over the instructions one SIMD issued
        const double clk = ticks / real * 100.0;  // MHz
        row.simd[wi] = (double)(last - first) * 1e-8 * clk * 1e6 / (2.0 * n_inst * W);
        if (W == 8) {
            row.mhz = clk;
            row.ev = ms * 1e-3 * mhz * 1e6 / (2.0 * n_inst * W);
        }
    }
    rows.push_back(row);
    return 0;
}

int main() {
    int cu = 0, khz = 0;
    CK(hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, 0));
    CK(hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, 0));
    const double mhz = khz / 1000.0;
    uint64_t* d_out = nullptr;
    CK(hipMalloc(&d_out, (size_t)cu * 4 * 8 * kOut * sizeof(uint64_t)));
    std::vector<Row> rows;
    int rc = 0;
    rc |= run<v_fma_f32>(d_out, cu, mhz, rows);
    rc |= run<v_mul_f32>(d_out, cu, mhz, rows);
    rc |= run<v_add_f32>(d_out, cu, mhz, rows);
    rc |= run<v_add_u32>(d_out, cu, mhz, rows);
    rc |= run<v_mov_b32>(d_out, cu, mhz, rows);
    rc |= run<v_mul_lo_u32>(d_out, cu, mhz, rows);
    rc |= run<v_mul_hi_u32>(d_out, cu, mhz, rows);
    rc |= run<v_mad_u64_u32>(d_out, cu, mhz, rows);
    rc |= run<v_mad_u32_u24>(d_out, cu, mhz, rows);
    rc |= run<v_lshl_add_u32>(d_out, cu, mhz, rows);
    rc |= run<v_lshl_add_u64>(d_out, cu, mhz, rows);
    rc |= run<v_add3_u32>(d_out, cu, mhz, rows);
    rc |= run<v_alignbit_b32>(d_out, cu, mhz, rows);
    rc |= run<v_rcp_f32>(d_out, cu, mhz, rows);
    rc |= run<v_rsq_f32>(d_out, cu, mhz, rows);
    rc |= run<v_sqrt_f32>(d_out, cu, mhz, rows);
    rc |= run<v_sin_f32>(d_out, cu, mhz, rows);
    rc |= run<v_cos_f32>(d_out, cu, mhz, rows);
    rc |= run<v_cvt_f64_u32>(d_out, cu, mhz, rows);
    rc |= run<v_mul_f64>(d_out, cu, mhz, rows);
    rc |= run<v_cvt_u32_f64>(d_out, cu, mhz, rows);
    rc |= run<v_cmp_lt_u64>(d_out, cu, mhz, rows);
    rc |= run<v_cndmask_b32>(d_out, cu, mhz, rows);
    rc |= run<v_readfirstlane_b32>(d_out, cu, mhz, rows);
    if (rc) return 1;
    printf("# %d CUs, clock attribute %.0f MHz; %u instructions per wave, the stamped middle half %u\n", cu, mhz,
           8192u * kUnroll * kChains, 4096u * kUnroll * kChains);
    printf("# wave:  s_memtime ticks per instruction as one wave sees it in its middle half, median over waves, W waves per SIMD launched\n");
    printf("# simd:  SIMD cycles per wave-instruction: the launch's span (s_memrealtime, first start to last end) at the measured clock\n");
    printf("#        over the instructions a SIMD issued; the pipe's price where W waves keep it busy\n");
    printf("# event: the W = 8 figure from the HIP-event time and the clock attribute;  MHz: s_memtime ticks per 10 ns of s_memrealtime, W = 8\n");
    printf("%-20s %7s %7s %7s %7s | %7s %7s %7s %7s | %6s %6s | %5s\n", "instruction", "wave 1", "2", "4", "8", "simd 1", "2", "4", "8",
           "event", "x fma", "MHz");
    for (const Row& r : rows)
        printf("%-20s %7.2f %7.2f %7.2f %7.2f | %7.2f %7.2f %7.2f %7.2f | %6.2f %6.2f | %5.0f\n", r.name, r.wave[0], r.wave[1], r.wave[2],
               r.wave[3], r.simd[0], r.simd[1], r.simd[2], r.simd[3], r.ev, r.simd[3] / rows[0].simd[3], r.mhz);
    return 0;
}
