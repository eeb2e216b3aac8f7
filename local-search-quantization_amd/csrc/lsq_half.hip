// lsq_half.hip -- half-precision base rows ON THE DEVICE (gfx950): the two streaming converts behind lsq_index_narrow_base and
// lsq_index_get_base, and the host narrowing lsq_narrow_rows_cpu.  The reference has no counterpart: it keeps no base rows.
//
// The kernels that READ half rows are the ones that read f32 and uint8 rows -- rerank_kernel<T, ALIGN> (lsq_rerank.hip) and knn_scan_kernel<MODE, TX, TQ,
// FILT> (lsq_knn.hip), instantiated on lsq_f16 / lsq_bf16 (lsq_xload.h) -- and widening is exact, so they return the bits of the f32 instantiation on the
// widened matrix (Identity W).  What is new here only moves bytes:
//
//   narrow_rows_kernel<T>   f32 rows at any pitch -> DENSE rows of T (pitch d).  Round to nearest even (Identity N): (_Float16)x for binary16 -- v_cvt_f16_f32,
//                           never the packed convert that rounds toward zero -- and the integer rule of lsq_half_check.h for bfloat16.  A lane takes EIGHT
//                           components: two 16-byte loads where the source pointer and pitch allow (16-byte aligned, lds % 4 == 0), dword loads otherwise, and
//                           ONE 16-byte store; dword / 2-byte stores cover a row's tail and, when d % 8 != 0, a destination row that does not start on 16
//                           bytes.  Nothing at or past a source row's d-th component is loaded.  4 + 2 bytes per component: bounded by HBM like a copy.
//                           It counts what narrowing destroyed -- finite -> +-inf, non-zero -> +-0 -- and the NaNs: per lane, summed over the wave, one
//                           partial per wave in LDS, one non-returning integer add per block and counter (lsq_range.hip's count pass).
//   widen_rows_kernel<T>    the other direction, for lsq_index_get_base: rows of T (uint8 as well) at any pitch -> f32 rows at any pitch; eight components per
//                           lane, one 16-byte (8-byte for uint8) load and two 16-byte stores where pointers and pitches allow, element loads / dword stores
//                           otherwise.
#include <string.h>

#include <type_traits>

#include "lsq_internal.h"
#include "lsq_xload.h"

namespace {

constexpr int HF_THREADS = 256;
constexpr int HF_LANE = 8;                   // components per lane and step

typedef uint32_t hf_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t hf_u32x2 __attribute__((ext_vector_type(2)));

// src rows lds floats apart -> dst rows d halves apart; vec: src is 16-byte aligned and lds % 4 == 0 (then every group of eight starts on 16 bytes)
template <typename T>
__global__ __launch_bounds__(HF_THREADS) void narrow_rows_kernel(const float *__restrict__ src, int64_t lds, uint16_t *__restrict__ dst, int64_t n, int d,
                                                                 int groups, int vec, unsigned long long *__restrict__ counts) {
    __shared__ unsigned wcnt[3][HF_THREADS / 64];
    constexpr uint32_t inf = std::is_same<T, lsq_f16>::value ? 0x7c00u : 0x7f80u;      // the bits of +inf in T
    unsigned c_inf = 0, c_zero = 0, c_nan = 0;
    const int64_t items = n * groups;
    for (int64_t it = (int64_t)blockIdx.x * HF_THREADS + threadIdx.x; it < items; it += (int64_t)gridDim.x * HF_THREADS) {
        const int64_t row = it / groups;
        const int k0 = (int)(it - row * groups) * HF_LANE;
        const int valid = d - k0 < HF_LANE ? d - k0 : HF_LANE;       // 1 .. 8 components of this row from k0 on
        const float *p = src + row * lds + k0;
        float x[HF_LANE];
        if (vec && valid == HF_LANE) {
            const lsq_f32x4 a = lsq_ld4_nt(p), b = lsq_ld4_nt(p + 4);
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
        } else {
#pragma unroll
            for (int e = 0; e < HF_LANE; ++e) x[e] = e < valid ? __builtin_nontemporal_load(p + e) : 0.0f;
        }
        uint32_t h[HF_LANE];
#pragma unroll
        for (int e = 0; e < HF_LANE; ++e) {
            h[e] = lsq_narrow1<T>(x[e]);
            const uint32_t a = __float_as_uint(x[e]) & 0x7fffffffu, m = h[e] & 0x7fffu;
            const bool live = e < valid;
            c_nan += (live && a > 0x7f800000u) ? 1u : 0u;
            c_inf += (live && a < 0x7f800000u && m == inf) ? 1u : 0u;
            c_zero += (live && a != 0u && a <= 0x7f800000u && m == 0u) ? 1u : 0u;
        }
        const int64_t e0 = row * d + k0;                             // the destination element: dense rows
        uint16_t *o = dst + e0;
        if (valid == HF_LANE && (e0 & 7) == 0) {
            hf_u32x4 w;
            w.x = h[0] | (h[1] << 16); w.y = h[2] | (h[3] << 16); w.z = h[4] | (h[5] << 16); w.w = h[6] | (h[7] << 16);
            *reinterpret_cast<hf_u32x4 *>(o) = w;
        } else if ((e0 & 1) == 0) {                                  // dwords, and the last odd component as two bytes
#pragma unroll
            for (int e = 0; e < HF_LANE; e += 2) {
                if (e + 1 < valid) *reinterpret_cast<uint32_t *>(o + e) = h[e] | (h[e + 1] << 16);
                else if (e < valid) o[e] = (uint16_t)h[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < HF_LANE; ++e)
                if (e < valid) o[e] = (uint16_t)h[e];
        }
    }
    // the counts: a sum per wave, a partial per wave, one add per block (the values are not used: no round trip)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        c_inf += __shfl_xor(c_inf, off, 64);
        c_zero += __shfl_xor(c_zero, off, 64);
        c_nan += __shfl_xor(c_nan, off, 64);
    }
    const int t = threadIdx.x;
    if ((t & 63) == 0) { wcnt[0][t >> 6] = c_inf; wcnt[1][t >> 6] = c_zero; wcnt[2][t >> 6] = c_nan; }
    __syncthreads();
    if (t < 3) {
        unsigned long long sum = 0;
#pragma unroll
        for (int w = 0; w < HF_THREADS / 64; ++w) sum += wcnt[t][w];
        if (sum) atomicAdd(&counts[t], sum);
    }
}

template <typename T> __device__ inline float hf_widen1(T v) { return (float)v; }

// src rows lds elements of T apart -> dst rows ldo floats apart.  vin: src and its pitch in bytes are multiples of 8 sizeof(T); vout: dst is 16-byte aligned
// and ldo % 4 == 0
template <typename T>
__global__ __launch_bounds__(HF_THREADS) void widen_rows_kernel(const T *__restrict__ src, int64_t lds, float *__restrict__ dst, int64_t ldo, int64_t count,
                                                                int d, int groups, int vin, int vout) {
    const int64_t items = count * groups;
    for (int64_t it = (int64_t)blockIdx.x * HF_THREADS + threadIdx.x; it < items; it += (int64_t)gridDim.x * HF_THREADS) {
        const int64_t row = it / groups;
        const int k0 = (int)(it - row * groups) * HF_LANE;
        const int valid = d - k0 < HF_LANE ? d - k0 : HF_LANE;
        const T *p = src + row * lds + k0;
        float x[HF_LANE];
        if (vin && valid == HF_LANE) {
            if constexpr (sizeof(T) == 2) {
                const hf_u32x4 w = __builtin_nontemporal_load(reinterpret_cast<const hf_u32x4 *>(p));
                const uint32_t wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const lsq_f32x2 f = lsq_widen2<T>(wv[j]);
                    x[2 * j] = f.x; x[2 * j + 1] = f.y;
                }
            } else {
                const hf_u32x2 w = __builtin_nontemporal_load(reinterpret_cast<const hf_u32x2 *>(p));
                const lsq_f32x4 a = lsq_widen4(w.x), b = lsq_widen4(w.y);
                x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < HF_LANE; ++e) x[e] = e < valid ? hf_widen1(p[e]) : 0.0f;
        }
        float *o = dst + row * ldo + k0;
        if (vout && valid == HF_LANE) {
            lsq_f32x4 a, b;
            a.x = x[0]; a.y = x[1]; a.z = x[2]; a.w = x[3]; b.x = x[4]; b.y = x[5]; b.z = x[6]; b.w = x[7];
            *reinterpret_cast<lsq_f32x4 *>(o) = a;
            *reinterpret_cast<lsq_f32x4 *>(o + 4) = b;
        } else {
#pragma unroll
            for (int e = 0; e < HF_LANE; ++e)
                if (e < valid) o[e] = x[e];
        }
    }
}

inline unsigned hf_grid(int64_t items) {
    int64_t blocks = (items + HF_THREADS - 1) / HF_THREADS;
    if (blocks > 256 * 16) blocks = 256 * 16;                        // grid-stride from here on: a few blocks per CU
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

template <typename T>
int widen_launch(hipStream_t s, const void *src, int64_t lds, float *dst, int64_t ldo, int64_t count, int d) {
    const int groups = (d + HF_LANE - 1) / HF_LANE;
    const uintptr_t ain = (uintptr_t)src | (uintptr_t)(lds * (int64_t)sizeof(T)), aout = (uintptr_t)dst | (uintptr_t)(ldo * 4);
    const int vin = (ain & (HF_LANE * sizeof(T) - 1)) == 0, vout = (aout & 15) == 0;
    hipLaunchKernelGGL((widen_rows_kernel<T>), dim3(hf_grid(count * groups)), dim3(HF_THREADS), 0, s, static_cast<const T *>(src), lds, dst, ldo, count, d,
                       groups, vin, vout);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

}  // namespace

int lsq_half_launch_narrow(hipStream_t s, const float *src, int64_t lds, void *dst, int64_t n, int d, int format, unsigned long long *counts) {
    if (n <= 0) return LSQ_OK;
    const int groups = (d + HF_LANE - 1) / HF_LANE;
    const int vec = (((uintptr_t)src | (uintptr_t)(lds * 4)) & 15) == 0;
    const dim3 grid(hf_grid(n * groups)), block(HF_THREADS);
    if (format == LSQ_BASE_F16)
        hipLaunchKernelGGL((narrow_rows_kernel<lsq_f16>), grid, block, 0, s, src, lds, static_cast<uint16_t *>(dst), n, d, groups, vec, counts);
    else
        hipLaunchKernelGGL((narrow_rows_kernel<lsq_bf16>), grid, block, 0, s, src, lds, static_cast<uint16_t *>(dst), n, d, groups, vec, counts);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

int lsq_half_launch_widen(hipStream_t s, const void *src, int format, int64_t lds, float *dst, int64_t ldo, int64_t count, int d) {
    if (count <= 0) return LSQ_OK;
    if (format == LSQ_BASE_F16) return widen_launch<lsq_f16>(s, src, lds, dst, ldo, count, d);
    if (format == LSQ_BASE_BF16) return widen_launch<lsq_bf16>(s, src, lds, dst, ldo, count, d);
    return widen_launch<uint8_t>(s, src, lds, dst, ldo, count, d);
}

// ---- the host narrowing: the checker of narrow_rows_kernel and the road the host binding uses (body: lsq_half_check.h) -----------------------------------
extern "C" int lsq_narrow_rows_cpu(void *dst, const float *src, int64_t n, int d, int64_t lds, int64_t ldd, int format, int nthreads) {
    if (const char *why = lsq_narrow_rows_host(dst, src, n, d, lds, ldd, format, nthreads)) {
        lsq_set_error("lsq_narrow_rows_cpu: %s (n=%lld d=%d lds=%lld ldd=%lld format=%d)", why, (long long)n, d, (long long)lds, (long long)ldd, format);
        return LSQ_EINVAL;
    }
    return LSQ_OK;
}
