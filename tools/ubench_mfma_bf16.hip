// tools/ubench_mfma_bf16.hip -- v_mfma_f32_32x32x16_bf16 on gfx950: (1) its issue rate, the bound of the half-precision pre-filter of exact k-NN
// (csrc/lsq_knnh.hip, knnh_scan_kernel: P nq n ceil(d / 16) / 1024 MFMAs, P = 2 pairs for bf16 rows and 3 for f16 rows), measured as
// tools/ubench_mfma_i8.hip measures the i8 instruction; (2) its ARITHMETIC, which no document at hand states: single instructions against a float64
// evaluation on the host, on inputs chosen to expose truncation, a narrow internal accumulator or a fixed-point alignment of the sixteen products --
//   gauss    Gaussian a, b, c                       cancel   c = -fl(SUM a b): the result is what the unit lost
//   bigacc   |c| = 2^20 .. 2^24 against products of order 1
//   spread   products spanning 2^-60 .. 2^60 in one instruction (c = 0, and c = -SUM |a b| / 4)
//   samesign all sixteen products and c positive (a truncating unit drifts one way)
//   denorm   bf16 denormal inputs, f32 denormal c and results below 2^-126 -- reported APART: a flushing unit loses them whole, which the window's absolute
//            term eta covers, not its relative term
// The figure the bound of DESIGN 4.31 adopts: worst |result - exact| / (|c| + SUM |a_k b_k|) over every element of every case but denorm.  One JSON line.
//   hipcc --offload-arch=gfx950 -O3 tools/ubench_mfma_bf16.hip -o tools/bin/ubench_mfma_bf16 && tools/bin/ubench_mfma_bf16
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NACC = 4, UNROLL = 8;       // MFMAs per loop iteration: NACC * UNROLL

__global__ void rate_kernel(float *out, const short *in, int iters, unsigned long long *clk) {
    extern __shared__ int hold[];                     // never read: 96 KiB of the CU's 160, so that every block has a CU to itself
    if (iters < 0) hold[threadIdx.x] = 0;
    const short v = in[threadIdx.x & 63];             // not known at compile time
    s16x8 as, bs;
#pragma unroll
    for (int e = 0; e < 8; ++e) { as[e] = (short)(v + e); bs[e] = (short)(v ^ (e + 5)); }
    const bf16x8 a = __builtin_bit_cast(bf16x8, as), b = __builtin_bit_cast(bf16x8, bs);
    f32x16 acc[NACC];
#pragma unroll
    for (int j = 0; j < NACC; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = (float)(v + j + r);
    __syncthreads();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
#pragma unroll
            for (int j = 0; j < NACC; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[j], 0, 0, 0);
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    float r = 0.0f;
#pragma unroll
    for (int j = 0; j < NACC; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) r += acc[j][e];
    if ((threadIdx.x & 63) == 0) {
        const size_t w = (size_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
        clk[2 * w] = t1 - t0;
        clk[2 * w + 1] = r1 - r0;
    }
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = r;
}

// one instruction per block (one wave): A [32 rows][16], B [32 columns][16] bf16 bits, C and D [32][32] f32.  Lane l holds row / column l & 31, k = 8 (l >> 5)
// .. + 7, and accumulator element r = row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
__global__ void one_kernel(const uint16_t *A, const uint16_t *B, const float *C, float *D) {
    const int l = threadIdx.x, c = blockIdx.x;
    const uint16_t *ap = A + ((size_t)c * 32 + (l & 31)) * 16 + 8 * (l >> 5), *bp = B + ((size_t)c * 32 + (l & 31)) * 16 + 8 * (l >> 5);
    s16x8 as, bs;
#pragma unroll
    for (int e = 0; e < 8; ++e) { as[e] = (short)ap[e]; bs[e] = (short)bp[e]; }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = C[((size_t)c * 32 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5)) * 32 + (l & 31)];
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, as), __builtin_bit_cast(bf16x8, bs), acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) D[((size_t)c * 32 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5)) * 32 + (l & 31)] = acc[r];
}

struct Rate { double clk_per_mfma, mhz; };

static Rate run(int blocks, int waves_per_simd, int iters, const short *in) {
    const int threads = 256 * waves_per_simd, waves = blocks * threads / 64;
    float *out; unsigned long long *clk;
    CK(hipMalloc(&out, sizeof(float) * (size_t)blocks * threads)); CK(hipMalloc(&clk, sizeof(unsigned long long) * 2 * waves));
    constexpr size_t lds = 96 * 1024;
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(&rate_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    rate_kernel<<<blocks, threads, lds>>>(out, in, iters, clk);      // warm-up
    CK(hipDeviceSynchronize());
    std::vector<double> per;
    double mhz = 0;
    for (int rep = 0; rep < 5; ++rep) {
        rate_kernel<<<blocks, threads, lds>>>(out, in, iters, clk);
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

static uint16_t to_bf16(float x) {                    // round to nearest even (the integer rule of csrc/lsq_half_check.h)
    uint32_t u; memcpy(&u, &x, 4);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
static double from_bf16(uint16_t h) { const uint32_t u = (uint32_t)h << 16; float x; memcpy(&x, &u, 4); return (double)x; }

enum { GAUSS, CANCEL, BIGACC, SPREAD, SAMESIGN, DENORM, KINDS };
static const char *KIND_NAME[KINDS] = {"gauss", "cancel", "bigacc", "spread", "samesign", "denorm"};

int main() {
    // ---- the arithmetic ----
    constexpr int PER = 64, CASES = PER * KINDS;      // instructions: 1024 elements each
    std::mt19937_64 rng(20260);
    std::normal_distribution<float> g(0.0f, 1.0f);
    std::uniform_int_distribution<int> ex(-30, 30), big(20, 24), coin(0, 1), dm(1, 127);
    std::vector<uint16_t> A((size_t)CASES * 32 * 16), B(A.size());
    std::vector<float> C((size_t)CASES * 32 * 32), D(C.size());
    auto dot = [&](int c, int i, int j, long double *mag) {
        long double s = 0, m = 0;
        for (int k = 0; k < 16; ++k) {
            const long double p = (long double)from_bf16(A[((size_t)c * 32 + i) * 16 + k]) * (long double)from_bf16(B[((size_t)c * 32 + j) * 16 + k]);
            s += p; m += fabsl(p);
        }
        *mag = m;
        return s;
    };
    for (int c = 0; c < CASES; ++c) {
        const int kind = c / PER;
        for (int i = 0; i < 32; ++i)
            for (int k = 0; k < 16; ++k) {
                float a = g(rng), b = g(rng);
                if (kind == SPREAD) { a = ldexpf(1.0f + 0.5f * fabsf(a), ex(rng)) * (coin(rng) ? 1 : -1); b = ldexpf(1.0f + 0.5f * fabsf(b), ex(rng)) * (coin(rng) ? 1 : -1); }
                if (kind == SAMESIGN) { a = fabsf(a) + 0.5f; b = fabsf(b) + 0.5f; }
                uint16_t ab = to_bf16(a), bb = to_bf16(b);
                if (kind == DENORM) {                 // half the instructions: bf16 denormals against ordinary values; the others: tiny normals whose products are denormal
                    if ((c & 1) == 0) ab = (uint16_t)((ab & 0x8000u) | (uint16_t)dm(rng));
                    else { ab = to_bf16(ldexpf(a, -70)); bb = to_bf16(ldexpf(b, -68)); }
                }
                A[((size_t)c * 32 + i) * 16 + k] = ab;
                B[((size_t)c * 32 + i) * 16 + k] = bb;
            }
        for (int i = 0; i < 32; ++i)
            for (int j = 0; j < 32; ++j) {
                long double m;
                const long double s = dot(c, i, j, &m);
                float cv = g(rng);
                if (kind == CANCEL) cv = -(float)s;
                if (kind == BIGACC) cv = ldexpf(1.0f + 0.5f * fabsf(cv), big(rng)) * (coin(rng) ? 1 : -1);
                if (kind == SPREAD) cv = (c & 1) ? 0.0f : -(float)(m / 4);
                if (kind == SAMESIGN) cv = fabsf(cv) * 16.0f;
                if (kind == DENORM) cv = (c & 2) ? 0.0f : ldexpf(cv, -140);
                C[((size_t)c * 32 + i) * 32 + j] = cv;
            }
    }
    uint16_t *dA, *dB; float *dC, *dD;
    CK(hipMalloc(&dA, A.size() * 2)); CK(hipMalloc(&dB, B.size() * 2)); CK(hipMalloc(&dC, C.size() * 4)); CK(hipMalloc(&dD, D.size() * 4));
    CK(hipMemcpy(dA, A.data(), A.size() * 2, hipMemcpyHostToDevice)); CK(hipMemcpy(dB, B.data(), B.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(dC, C.data(), C.size() * 4, hipMemcpyHostToDevice));
    one_kernel<<<CASES, 64>>>(dA, dB, dC, dD);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(D.data(), dD, D.size() * 4, hipMemcpyDeviceToHost));
    double worst[KINDS] = {0}, worst_abs[KINDS] = {0};
    long nonfinite = 0;
    for (int c = 0; c < CASES; ++c)
        for (int i = 0; i < 32; ++i)
            for (int j = 0; j < 32; ++j) {
                long double m;
                const size_t at = ((size_t)c * 32 + i) * 32 + j;
                const long double exact = dot(c, i, j, &m) + (long double)C[at];
                if (!std::isfinite(D[at])) { ++nonfinite; continue; }
                const double err = (double)fabsl((long double)D[at] - exact), den = (double)(m + fabsl((long double)C[at]));
                const int kind = c / PER;
                if (den > 0) worst[kind] = std::max(worst[kind], err / den);
                worst_abs[kind] = std::max(worst_abs[kind], err);
            }
    double measured = 0;
    for (int kd = 0; kd < KINDS; ++kd) if (kd != DENORM) measured = std::max(measured, worst[kd]);
    double adopted = ldexp(1.0, -21);                 // 8 x the worst ratio, up to a power of two, not below 2^-21
    while (adopted < 8.0 * measured) adopted *= 2.0;
    printf("{\"ubench\": \"mfma_bf16\", \"instructions\": %d, \"elements\": %ld, \"nonfinite_results\": %ld", CASES, (long)CASES * 1024, nonfinite);
    for (int kd = 0; kd < KINDS; ++kd) printf(", \"worst_ratio_%s\": %.6g, \"log2_%s\": %.2f", KIND_NAME[kd], worst[kd], KIND_NAME[kd], worst[kd] > 0 ? log2(worst[kd]) : -999.0);
    printf(", \"denorm_worst_abs_error\": %.6g, \"log2_denorm_worst_abs_error\": %.2f", worst_abs[DENORM], worst_abs[DENORM] > 0 ? log2(worst_abs[DENORM]) : -999.0);
    printf(", \"eps_hw_measured\": %.6g, \"log2_eps_hw_measured\": %.2f, \"eps_hw_adopted\": %.6g, \"log2_eps_hw_adopted\": %d", measured,
           measured > 0 ? log2(measured) : -999.0, adopted, (int)lround(log2(adopted)));
    CK(hipFree(dA)); CK(hipFree(dB)); CK(hipFree(dC)); CK(hipFree(dD));
    // ---- the issue rate ----
    std::vector<short> h(64);
    for (int i = 0; i < 64; ++i) h[i] = (short)(0x3f80 + i);
    short *in;
    CK(hipMalloc(&in, sizeof(short) * 64));
    CK(hipMemcpy(in, h.data(), sizeof(short) * 64, hipMemcpyHostToDevice));
    const int iters = 20000;
    double best[2] = {1e30, 1e30}, mhz[2] = {0, 0};
    const int blocks[2] = {1, 256};
    for (int c = 0; c < 2; ++c)
        for (int w : {1, 2, 4}) {
            const Rate r = run(blocks[c], w, iters, in);
            printf(", \"%s_waves_per_simd_%d\": {\"clk_per_mfma\": %.3f, \"shader_mhz\": %.0f}", c ? "chip" : "one_cu", w, r.clk_per_mfma, r.mhz);
            if (r.clk_per_mfma < best[c]) { best[c] = r.clk_per_mfma; mhz[c] = r.mhz; }
        }
    const double macs = 32.0 * 32.0 * 16.0;           // one MFMA; 4 SIMDs per CU, 256 CUs
    printf(", \"one_cu_clk_per_mfma\": %.3f, \"chip_clk_per_mfma\": %.3f, \"chip_mfma_per_s\": %.4g, \"chip_tera_flops_per_s\": %.1f}\n", best[0], best[1],
           4.0 * 256 / best[1] * mhz[1] * 1e6, 2.0 * macs * 4.0 * 256 / best[1] * mhz[1] * 1e6 / 1e12);
    CK(hipFree(in));
    return 0;
}
