// lds_atomic_calib.hip -- what one CU's LDS charges for the instructions the backward's accumulate is made of, so that a
// design that trades sparse ds_add_f32 for staged stores and dense adds is priced from MEASURED costs
// (DESIGN.md "LDS accumulate"; MI355X_MICROARCH.md's LDS table has loads and stores, no atomics).
//
//   hipcc --offload-arch=gfx950 -O3 -o lds_atomic_calib lds_atomic_calib.hip && ./lds_atomic_calib > lds_atomic_calibration.jsonl
//
// Every kernel runs ITER x UNROLL instructions of one kind per wave, drained with s_waitcnt lgkmcnt(0) after every UNROLL
// (the backward drains its 29 adds at a barrier).  Blocks of four waves (one per SIMD), 32 KB of LDS each, grid = CUs x
// blocks per CU (1, 2, 4 -> 4, 8, 16 waves per CU).  With the LDS the only busy unit, elapsed cycles / (instructions per
// wave x waves per CU) is what ONE wave-instruction holds the CU's LDS for once enough waves are there to keep it busy.
// Two clocks: s_memtime inside the kernel (lds_cycles_per_instr) and hipEvent time x the nominal shader clock
// (lds_cycles_per_instr_wall).  They agree at 4 waves per CU; at 16 the s_memtime figure falls to ~0.62 of the other for
// every kind, ds_read_b32 (2 cycles by the table) included: read the WALL figure at 16 waves per CU.
//   ds_add_f32 (no return)   active lanes 1, 4, 10, 32, 58, 64 (spread over the wave as emit lanes are)
//                            x lanes per address 1, 2, 4 (neighbouring active lanes share one)
//                            x addresses in distinct banks (pitch 33 dwords, the accumulator rows') / all in one bank
//   ds_write_b128            active lanes 1, 4, 10, 32, 64, one 16-byte slot each (pitch 36 dwords)
//   ds_read_b32              active lanes 16, 32, 64, consecutive dwords
//   ds_write_b32             active lanes 1, 4, 10, 32, 64, the addresses of ds_add_f32 (what an emit costs where no other wave shares its row)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)

constexpr int ITER = 1024;
constexpr int UNROLL = 16;
constexpr int LDS_DWORDS = 8192;                          // 32 KB per block: four blocks per CU fit

enum Kind { K_ADD = 0, K_WRITE128 = 1, K_READ32 = 2, K_WRITE32 = 3 };
static const char* kind_name[4] = {"ds_add_f32", "ds_write_b128", "ds_read_b32", "ds_write_b32"};
typedef float v4f __attribute__((ext_vector_type(4)));

// dword index a lane works on; -1: the lane is idle.  n active lanes spread evenly over the wave, rank r among them,
// `mult` neighbouring ranks per address
__device__ __forceinline__ int lane_dword(int kind, int lane, int n, int mult, int one_bank) {
    const int r = (lane * n) >> 6;
    if ((((lane + 1) * n) >> 6) == r) return -1;
    if (kind == K_READ32) return r;
    if (kind == K_WRITE128) return r * 36;
    return (r / mult) * (one_bank ? 128 : 33);
}

template <int KIND>
__global__ void __launch_bounds__(256) k_calib(float* out, unsigned long long* cyc, int n, int mult, int one_bank) {
    __shared__ __attribute__((aligned(16))) float lds[LDS_DWORDS];
    for (int i = threadIdx.x; i < LDS_DWORDS; i += 256) lds[i] = 0.f;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int dw = lane_dword(KIND, lane, n, mult, one_bank);
    float got = 0.f;
    unsigned long long t0 = 0, t1 = 0;
    if (dw >= 0 && dw + 4 <= LDS_DWORDS) {                // (the idle lanes sit the loop out: EXEC holds the active ones only)
        const unsigned addr = (unsigned)(size_t)(__attribute__((address_space(3))) float*)(lds + dw);
        const float val = 1.0f;
        const v4f val4 = {1.f, 2.f, 3.f, 4.f};
        t0 = __builtin_readcyclecounter();
        for (int it = 0; it < ITER; it++) {
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
                if (KIND == K_ADD) asm volatile("ds_add_f32 %0, %1" :: "v"(addr), "v"(val) : "memory");
                else if (KIND == K_WRITE128) asm volatile("ds_write_b128 %0, %1" :: "v"(addr), "v"(val4) : "memory");
                else if (KIND == K_WRITE32) asm volatile("ds_write_b32 %0, %1" :: "v"(addr), "v"(val) : "memory");
                else asm volatile("ds_read_b32 %0, %1" : "=v"(got) : "v"(addr) : "memory");
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        t1 = __builtin_readcyclecounter();
    }
    __syncthreads();
    if (got == 123.456f) out[0] = got + lds[threadIdx.x];  // keeps the loads alive; never true
    // (which lanes were active depends on the layout: the wave reports the largest of its lanes' figures, idle lanes hold 0)
    unsigned long long dt = t1 - t0;
    for (int o = 32; o >= 1; o >>= 1) { const unsigned long long other = __shfl_xor(dt, o); dt = other > dt ? other : dt; }
    if (lane == 0) cyc[blockIdx.x * 4 + (threadIdx.x >> 6)] = dt;
}

template <int KIND>
static void run(int n, int mult, int one_bank, int blocks_per_cu, float* d_out, unsigned long long* d_cyc, int ncu, double khz) {
    const int blocks = ncu * blocks_per_cu, waves = blocks * 4;
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    hipLaunchKernelGGL((k_calib<KIND>), dim3(blocks), dim3(256), 0, 0, d_out, d_cyc, n, mult, one_bank);   // warm-up
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL((k_calib<KIND>), dim3(blocks), dim3(256), 0, 0, d_out, d_cyc, n, mult, one_bank);
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<unsigned long long> cyc(waves);
    CK(hipMemcpy(cyc.data(), d_cyc, waves * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    double mean = 0; for (auto c : cyc) mean += (double)c; mean /= waves;
    const double instr = (double)ITER * UNROLL;           // per wave
    const int wpc = 4 * blocks_per_cu;
    printf("{\"kind\": \"%s\", \"active_lanes\": %d, \"lanes_per_address\": %d, \"banks\": \"%s\", \"waves_per_cu\": %d, "
           "\"cycles_per_instr_seen_by_wave\": %.2f, \"lds_cycles_per_instr\": %.2f, \"wall_ms\": %.4f, \"lds_cycles_per_instr_wall\": %.2f}\n",
           kind_name[KIND], n, mult, one_bank ? "one" : "distinct", wpc, mean / instr, mean / instr / wpc, ms,
           ms * khz / (instr * wpc));
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
}

int main() {
    hipDeviceProp_t p; CK(hipGetDeviceProperties(&p, 0));
    const int ncu = p.multiProcessorCount;
    printf("{\"device\": \"%s\", \"cus\": %d, \"clock_khz\": %d}\n", p.gcnArchName, ncu, p.clockRate);
    float* d_out; unsigned long long* d_cyc;
    CK(hipMalloc(&d_out, 4096)); CK(hipMalloc(&d_cyc, sizeof(unsigned long long) * ncu * 4 * 4));
    const double khz = (double)p.clockRate;
    for (int bpc : {1, 2, 4}) {
        for (int one_bank : {0, 1})
            for (int mult : {1, 2, 4})
                for (int n : {1, 4, 10, 32, 58, 64})
                    if (mult <= n) run<K_ADD>(n, mult, one_bank, bpc, d_out, d_cyc, ncu, khz);
        for (int n : {1, 4, 10, 32, 64}) run<K_WRITE128>(n, 1, 0, bpc, d_out, d_cyc, ncu, khz);
        for (int n : {16, 32, 64}) run<K_READ32>(n, 1, 0, bpc, d_out, d_cyc, ncu, khz);
        for (int n : {1, 4, 10, 32, 64}) run<K_WRITE32>(n, 1, 0, bpc, d_out, d_cyc, ncu, khz);
    }
    return 0;
}
