// tools/ubench_mfma_i8.hip -- the issue rate of v_mfma_i32_32x32x32_i8 on gfx950, which the guides do not give: the bound of the matrix-core road of exact
// k-NN on 8-bit sets (csrc/lsq_knnu.hip, knnu_scan_kernel: nq n ceil(d / 32) / 1024 MFMAs).  A dependent-free stream: four accumulators of 32 x 32 i32
// per wave, as in the kernel, so an accumulator is touched again only four instructions later.  One block per CU (96 KiB of LDS held), 1 / 2 / 4 waves
// per SIMD; measured on ONE CU (one block) and on the CHIP (256 blocks).  s_memtime counts shader clocks, s_memrealtime (100 MHz) gives the clock the
// part really ran at.  One JSON line.
//   hipcc --offload-arch=gfx950 -O3 tools/ubench_mfma_i8.hip -o tools/bin/ubench_mfma_i8 && tools/bin/ubench_mfma_i8
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int NACC = 4, UNROLL = 8;       // MFMAs per loop iteration: NACC * UNROLL

__global__ void k(int *out, const int *in, int iters, unsigned long long *clk) {
    extern __shared__ int hold[];                     // never read: 96 KiB of the CU's 160, so that every block has a CU to itself
    if (iters < 0) hold[threadIdx.x] = 0;
    const int v = in[threadIdx.x & 63];               // not known at compile time
    const i32x4 a = {v, v + 1, v + 2, v + 3}, b = {v ^ 5, v ^ 6, v ^ 7, v ^ 8};
    i32x16 acc[NACC];
#pragma unroll
    for (int j = 0; j < NACC; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = v + j + r;
    __syncthreads();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
#pragma unroll
            for (int j = 0; j < NACC; ++j) acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc[j], 0, 0, 0);
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    int r = 0;
#pragma unroll
    for (int j = 0; j < NACC; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) r ^= acc[j][e];
    if ((threadIdx.x & 63) == 0) {
        const size_t w = (size_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
        clk[2 * w] = t1 - t0;
        clk[2 * w + 1] = r1 - r0;
    }
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = r;
}

struct Rate { double clk_per_mfma, mhz; };

// waves_per_simd waves on each SIMD of `blocks` CUs -> shader clocks per MFMA per SIMD (median of 5 launches after a warm-up)
static Rate run(int blocks, int waves_per_simd, int iters, const int *in) {
    const int threads = 256 * waves_per_simd, waves = blocks * threads / 64;
    int *out; unsigned long long *clk;
    CK(hipMalloc(&out, sizeof(int) * (size_t)blocks * threads)); CK(hipMalloc(&clk, sizeof(unsigned long long) * 2 * waves));
    constexpr size_t lds = 96 * 1024;
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    k<<<blocks, threads, lds>>>(out, in, iters, clk);      // warm-up
    CK(hipDeviceSynchronize());
    std::vector<double> per;
    double mhz = 0;
    for (int rep = 0; rep < 5; ++rep) {
        k<<<blocks, threads, lds>>>(out, in, iters, clk);
        CK(hipDeviceSynchronize());
        std::vector<unsigned long long> h(2 * (size_t)waves);
        CK(hipMemcpy(h.data(), clk, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
        double cyc = 0, real = 0;
        for (int i = 0; i < waves; ++i) { cyc += (double)h[2 * i]; real += (double)h[2 * i + 1]; }
        cyc /= waves; real /= waves;
        per.push_back(cyc / ((double)iters * NACC * UNROLL * waves_per_simd));
        mhz = cyc / (real / 100.0);
    }
    std::sort(per.begin(), per.end());
    CK(hipFree(out)); CK(hipFree(clk));
    return {per[per.size() / 2], mhz};
}

int main() {
    std::vector<int> h(64);
    for (int i = 0; i < 64; ++i) h[i] = 0x01020304 * (i + 1);
    int *in;
    CK(hipMalloc(&in, sizeof(int) * 64));
    CK(hipMemcpy(in, h.data(), sizeof(int) * 64, hipMemcpyHostToDevice));
    const int iters = 20000;
    printf("{\"ubench\": \"mfma_i8\", \"mfmas_per_wave\": %d", iters * NACC * UNROLL);
    double best[2] = {1e30, 1e30}, mhz[2] = {0, 0};
    const int blocks[2] = {1, 256};
    for (int c = 0; c < 2; ++c)
        for (int w : {1, 2, 4}) {
            const Rate r = run(blocks[c], w, iters, in);
            printf(", \"%s_waves_per_simd_%d\": {\"clk_per_mfma\": %.3f, \"shader_mhz\": %.0f}", c ? "chip" : "one_cu", w, r.clk_per_mfma, r.mhz);
            if (r.clk_per_mfma < best[c]) { best[c] = r.clk_per_mfma; mhz[c] = r.mhz; }
        }
    // one MFMA is 32 x 32 x 32 multiply-adds; 4 SIMDs per CU, 256 CUs
    const double macs = 32.0 * 32.0 * 32.0;
    printf(", \"one_cu_clk_per_mfma\": %.3f, \"chip_clk_per_mfma\": %.3f, \"one_cu_mfma_per_s\": %.4g, \"chip_mfma_per_s\": %.4g, \"chip_tera_ops_per_s\": %.1f}\n",
           best[0], best[1], 4.0 / best[0] * mhz[0] * 1e6, 4.0 * 256 / best[1] * mhz[1] * 1e6, 2.0 * macs * 4.0 * 256 / best[1] * mhz[1] * 1e6 / 1e12);
    CK(hipFree(in));
    return 0;
}
