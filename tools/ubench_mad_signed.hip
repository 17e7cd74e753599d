// Micro-benchmark: issue rate of the signed wide multiply-add (v_mad_i64_i32) and of the arithmetic 64-bit shift (v_ashrrev_i64)
// beside their unsigned twins (v_mad_u64_u32, v_lshrrev_b64) on gfx950, in the shape of the mad_u64_u32 rows of
// profiles/r01_ubench_int_rates.txt: 4 and 8 waves per SIMD, one dependent chain and eight independent chains per lane.
// Standalone (no torch): hipcc --offload-arch=gfx950 -O3 ubench_mad_signed.hip -o ubench_mad_signed
// Every timing is taken five times; the line gives the median and the range.  profiles/accumulate_signed_differences.txt holds a run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
typedef uint32_t u32;
typedef uint64_t u64;
#define CHECK(x) do{hipError_t e=(x); if(e!=hipSuccess){printf("HIP error %s at %s:%d\n",hipGetErrorString(e),__FILE__,__LINE__); return 1;}}while(0)
#define ITERS 4096
#define CH 8

#define MAD_U(acc, x, y) asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc) : "v"(x), "v"(y) : "vcc")
#define MAD_I(acc, x, y) asm volatile("v_mad_i64_i32 %0, vcc, %1, %2, %0" : "+v"(acc) : "v"(x), "v"(y) : "vcc")
#define SHR_U(acc) asm volatile("v_lshrrev_b64 %0, 1, %0" : "+v"(acc))
#define SHR_I(acc) asm volatile("v_ashrrev_i64 %0, 1, %0" : "+v"(acc))

// SIGNED picks the instruction; CHAINS = 1: every multiply-add waits for the one before it; CHAINS = 8: eight accumulators in turn
template <bool SIGNED, int CHAINS>
__global__ void k_mad(u64 *out, u32 a, u32 b)
{
    u64 acc[CHAINS];
    u32 x = a + threadIdx.x, y[CHAINS];
    for (int c = 0; c < CHAINS; c++) {
        acc[c] = c + threadIdx.x;
        y[c] = b * (c + 3) + blockIdx.x + (threadIdx.x << c);
    }
    for (int it = 0; it < ITERS * CH / CHAINS; it++) {
#pragma unroll
        for (int c = 0; c < CHAINS; c++) {
            if constexpr (SIGNED)
                MAD_I(acc[c], x, y[c]);
            else
                MAD_U(acc[c], x, y[c]);
        }
    }
    u64 s = 0;
    for (int c = 0; c < CHAINS; c++) s += acc[c];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <bool SIGNED, int CHAINS>
__global__ void k_shift(u64 *out, u32 a, u32 b)
{
    u64 acc[CHAINS];
    for (int c = 0; c < CHAINS; c++) acc[c] = ((u64)(a + c + threadIdx.x) << 33) ^ ((u64)b << 63) ^ blockIdx.x;
    for (int it = 0; it < ITERS * CH / CHAINS; it++) {
#pragma unroll
        for (int c = 0; c < CHAINS; c++) {
            if constexpr (SIGNED)
                SHR_I(acc[c]);
            else
                SHR_U(acc[c]);
        }
    }
    u64 s = 0;
    for (int c = 0; c < CHAINS; c++) s += acc[c];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <typename K>
static void timeit(const char *name, int cus, int blocks, int threads, K kern, u64 *out)
{
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    kern<<<blocks, threads>>>(out, 3u, 5u);
    hipDeviceSynchronize();
    float ms[5];
    for (int s = 0; s < 5; s++) {
        hipEventRecord(e0);
        for (int r = 0; r < 3; r++) kern<<<blocks, threads>>>(out, 3u, 5u);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        hipEventElapsedTime(&ms[s], e0, e1);
        ms[s] /= 3;
    }
    std::sort(ms, ms + 5);
    const double total = (double)ITERS * CH * blocks * threads;
    const double rate = total / (ms[2] * 1e-3);
    printf("%-22s blocks=%5d thr=%4d  %8.4f ms (%8.4f ... %8.4f)  %10.2f Gop/s  %7.2f lane-ops/clk/CU(@2.4GHz, %dCU)\n", name, blocks, threads, ms[2], ms[0], ms[4], rate * 1e-9,
           rate / (2.4e9 * cus), cus);
    hipEventDestroy(e0);
    hipEventDestroy(e1);
}

int main()
{
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    printf("device: %s  CUs=%d clock=%d kHz\n", prop.gcnArchName, cus, prop.clockRate);
    u64 *out;
    CHECK(hipMalloc(&out, sizeof(u64) * (size_t)cus * 8 * 256));
    for (int wps : {4, 8}) {
        const int blocks = cus * wps, threads = 256; // wps waves on each of a CU's four SIMDs
        printf("--- %d wave(s) per SIMD ---\n", wps);
        timeit("mad_u64_u32 dependent", cus, blocks, threads, k_mad<false, 1>, out);
        timeit("mad_i64_i32 dependent", cus, blocks, threads, k_mad<true, 1>, out);
        timeit("mad_u64_u32 8 chains", cus, blocks, threads, k_mad<false, 8>, out);
        timeit("mad_i64_i32 8 chains", cus, blocks, threads, k_mad<true, 8>, out);
        timeit("lshrrev_b64 dependent", cus, blocks, threads, k_shift<false, 1>, out);
        timeit("ashrrev_i64 dependent", cus, blocks, threads, k_shift<true, 1>, out);
        timeit("lshrrev_b64 8 chains", cus, blocks, threads, k_shift<false, 8>, out);
        timeit("ashrrev_i64 8 chains", cus, blocks, threads, k_shift<true, 8>, out);
    }
    CHECK(hipDeviceSynchronize());
    CHECK(hipFree(out));
    return 0;
}
