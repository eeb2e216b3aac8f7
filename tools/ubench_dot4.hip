// tools/ubench_dot4.hip -- the issue rate of v_dot4_u32_u8 per SIMD on gfx950, which the guides do not give: the bound of the integer road of exact
// k-NN (csrc/lsq_knn.hip, knn_scan_u8_kernel: nq n d / 4 dot4 lane-ops).  A dependent-free stream from a few waves: 32 accumulators per lane, as in
// the kernel, so an accumulator is touched again only 32 instructions later.  Next to it the same stream of v_pk_add_f32 (the f32 kernel's
// instruction, 16 float2 accumulators x 2) as the yardstick of "full rate".  Plain C++ and builtins; s_memtime counts shader clocks, s_memrealtime
// (100 MHz) gives the clock the part really ran at.  One JSON line.
//   hipcc --offload-arch=gfx950 -O3 tools/ubench_dot4.hip -o tools/bin/ubench_dot4 && tools/bin/ubench_dot4
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int NACC = 32, UNROLL = 4;      // instructions per loop iteration: NACC * UNROLL

// OP 0: v_dot4_u32_u8, OP 1: v_pk_add_f32
template <int OP>
__global__ void k(unsigned *out, const unsigned *in, int iters, unsigned long long *clk) {
    extern __shared__ unsigned hold[];                // never read: 96 KiB of the CU's 160, so that every block has a CU to itself
    if (iters < 0) hold[threadIdx.x] = 0;
    const unsigned a = in[threadIdx.x & 63], b = in[64 + (threadIdx.x & 63)];      // not known at compile time
    unsigned acc[NACC];
    f32x2 facc[NACC];
#pragma unroll
    for (int j = 0; j < NACC; ++j) { acc[j] = a + j; facc[j] = (f32x2){(float)(a + j), (float)(b + j)}; }
    const f32x2 inc = (f32x2){(float)a * 1e-3f, (float)b * 1e-3f};
    __syncthreads();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
#pragma unroll
            for (int j = 0; j < NACC; ++j) {
                if (OP == 0) acc[j] = __builtin_amdgcn_udot4(a + u, b, acc[j], false);
                else facc[j] = facc[j] + inc;
            }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    unsigned r = 0;
#pragma unroll
    for (int j = 0; j < NACC; ++j) r ^= OP == 0 ? acc[j] : (__float_as_uint(facc[j].x) ^ __float_as_uint(facc[j].y));
    if ((threadIdx.x & 63) == 0) {
        const size_t w = (size_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
        clk[2 * w] = t1 - t0;
        clk[2 * w + 1] = r1 - r0;
    }
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = r;
}

struct Rate { double clk_per_instr, mhz; };

// waves_per_simd waves on each SIMD of every CU (one block of 4 * waves_per_simd waves per CU, 256 blocks) -> shader clocks per wave-instruction per SIMD
template <int OP>
static Rate run(int waves_per_simd, int iters, const unsigned *in) {
    const int threads = 256 * waves_per_simd, blocks = 256, waves = blocks * threads / 64;
    unsigned *out; unsigned long long *clk;
    CK(hipMalloc(&out, sizeof(unsigned) * (size_t)blocks * threads)); CK(hipMalloc(&clk, sizeof(unsigned long long) * 2 * waves));
    constexpr size_t lds = 96 * 1024;
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k<OP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    k<OP><<<blocks, threads, lds>>>(out, in, iters, clk);      // warm-up
    CK(hipDeviceSynchronize());
    std::vector<double> per;
    double mhz = 0;
    for (int rep = 0; rep < 5; ++rep) {
        k<OP><<<blocks, threads, lds>>>(out, in, iters, clk);
        CK(hipDeviceSynchronize());
        std::vector<unsigned long long> h(2 * (size_t)waves);
        CK(hipMemcpy(h.data(), clk, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
        double cyc = 0, real = 0;
        for (int i = 0; i < waves; ++i) { cyc += (double)h[2 * i]; real += (double)h[2 * i + 1]; }
        cyc /= waves; real /= waves;
        // a wave ran iters * NACC * UNROLL instructions in cyc clocks while waves_per_simd waves shared its SIMD
        per.push_back(cyc / ((double)iters * NACC * UNROLL * waves_per_simd));
        mhz = cyc / (real / 100.0);
    }
    std::sort(per.begin(), per.end());
    CK(hipFree(out)); CK(hipFree(clk));
    return {per[per.size() / 2], mhz};
}

int main() {
    std::vector<unsigned> h(128);
    for (int i = 0; i < 128; ++i) h[i] = 0x01020304u * (unsigned)(i + 1);
    unsigned *in;
    CK(hipMalloc(&in, sizeof(unsigned) * 128));
    CK(hipMemcpy(in, h.data(), sizeof(unsigned) * 128, hipMemcpyHostToDevice));
    const int iters = 20000;
    printf("{\"ubench\": \"dot4\", \"instructions_per_wave\": %d", iters * NACC * UNROLL);
    double best_dot = 1e30, best_pk = 1e30, mhz = 0;
    for (int w : {1, 2, 4}) {
        const Rate d = run<0>(w, iters, in), p = run<1>(w, iters, in);
        printf(", \"waves_per_simd_%d\": {\"v_dot4_u32_u8_clk_per_instr\": %.3f, \"v_pk_add_f32_clk_per_instr\": %.3f, \"shader_mhz\": %.0f}", w,
               d.clk_per_instr, p.clk_per_instr, d.mhz);
        if (d.clk_per_instr < best_dot) best_dot = d.clk_per_instr;
        if (p.clk_per_instr < best_pk) best_pk = p.clk_per_instr;
        mhz = d.mhz;
    }
    // lane-ops per second chip-wide: 64 lanes per instruction, 4 SIMDs x 256 CUs
    printf(", \"dot4_clk_per_instr\": %.3f, \"pk_add_clk_per_instr\": %.3f, \"dot4_over_pk_add\": %.3f, \"dot4_lane_ops_per_s\": %.4g}\n", best_dot, best_pk,
           best_dot / best_pk, 64.0 / best_dot * 4 * 256 * mhz * 1e6);
    CK(hipFree(in));
    return 0;
}
