// lsq_recon.hip -- decode on the device: the vectors a quantiser's codes stand for.
//
// Reference: reconstruct(B, C) (src/utils.jl:203-223): CB = zeros; CB += C[i][:, B[i, :]], i ascending.  Per row b (m bytes, 0-based) and codebooks K [m h][d]
//   x^[t] = (((+0.0f + K[(0 h + b_0) d + t]) + K[(1 h + b_1) d + t]) + ...) + K[((m - 1) h + b_(m-1)) d + t]
// in f32, every add rounded, codebooks ascending, STARTING FROM +0.0 (so m codewords of -0.0 give +0.0; quantize_norms_kernel starts from row[0], which is fine
// for a norm and wrong here); with the coarse add one more rounded add of the centroid of the row's list.  These are reference_api.reconstruct's bits.
//
// The work per row is m gathers of a d-float codeword and one d-float store: nothing is reused inside a row, the table (m h d floats: 1 MiB at m = 8,
// d = 128) is reused across rows out of L2.  Lanes run along the dimension, four components each; a group of min(64, next_pow2(ceil(d / 4))) lanes owns a
// row, a wave holds 64 / group rows per step.  The m codeword loads of a lane are independent and go out together, the chain is added in registers in
// codebook order, one store per lane follows.  No LDS, no atomics in the decode, plain vector stores.
#include "lsq_internal.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RECON_BLOCK = 256;
constexpr int RECON_MAX_BLOCKS = 2048;        // grid-stride beyond: 8 blocks of 4 waves for each of 256 CUs
constexpr uint32_t RECON_NAN = 0x7FC00000u;

struct ReconArgs {
    const uint8_t *codes; int64_t ldc;        // rows ldc bytes apart
    const float *K; int d, m;
    int64_t n;                                // rows addressable
    const int32_t *ids; int id_base;          // IDS: ids [count] in id_base; else rows start .. start + count - 1
    int64_t start, count;
    float *out; int64_t ldo;                  // elements
    const float *cent; const int32_t *lor;    // COARSE: centroids [nlist][d], the list of every row
    int nlist;
    int gshift;                               // log2 of the lane group
};

// VEC: 16-byte loads of K (and the centroids) and 16-byte stores -- d % 4 == 0, K / out 16-byte aligned, ldo % 4 == 0 (the launcher decides); else dwords.
// CW: the code row is read as ceil(m / 4) dwords (ldc % 4 == 0, codes 4-byte aligned: they lie inside the row's pitch); else m bytes.
// MQ = ceil(m / 4): the codeword loads are unrolled to 4 MQ with the m-tail guarded.  IDS / COARSE / PAD: the id form, the coarse add, the NaN pad
template <int MQ, bool VEC, bool CW, bool IDS, bool COARSE, bool PAD>
__global__ __launch_bounds__(RECON_BLOCK) void recon_kernel(const ReconArgs a) {
    const int group = 1 << a.gshift;
    const int lane = (int)threadIdx.x & (group - 1);
    const int rows_per_block = RECON_BLOCK >> a.gshift;
    const int64_t stride = (int64_t)gridDim.x * rows_per_block;
    const int d = a.d, m = a.m;
    for (int64_t r = (int64_t)blockIdx.x * rows_per_block + ((int)threadIdx.x >> a.gshift); r < a.count; r += stride) {
        int64_t row = a.start + r;
        if (IDS) row = (int64_t)a.ids[r] - a.id_base;
        float *o = a.out + r * a.ldo;
        const bool valid = row >= 0 && row < a.n;     // range form: always (the caller checked); id form without PAD: an id that slipped past the check writes nothing
        if (!valid) {
            if (PAD) {
                const float nanv = __uint_as_float(RECON_NAN);
                for (int t = lane * 4; t < d; t += group * 4) {
                    if (VEC) *reinterpret_cast<f32x4 *>(o + t) = f32x4{nanv, nanv, nanv, nanv};
                    else
                        for (int e = 0; e < 4; ++e)
                            if (t + e < d) o[t + e] = nanv;
                }
            }
            continue;
        }
        // the code row: m bytes -> the m codeword rows
        const uint8_t *b = a.codes + row * a.ldc;
        uint32_t w[MQ];
        if (CW) {
#pragma unroll
            for (int q = 0; q < MQ; ++q) w[q] = reinterpret_cast<const uint32_t *>(b)[q];
        } else {
#pragma unroll
            for (int q = 0; q < MQ; ++q) {
                w[q] = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * q + e < m) w[q] |= (uint32_t)b[4 * q + e] << (8 * e);
            }
        }
        const float *cw[4 * MQ];
#pragma unroll
        for (int j = 0; j < 4 * MQ; ++j) cw[j] = a.K + ((int64_t)j * LSQ_H + ((w[j >> 2] >> (8 * (j & 3))) & 255u)) * d;
        const float *cc = nullptr;
        if (COARSE) cc = a.cent + (int64_t)min(max(a.lor[row], 0), a.nlist - 1) * d;      // (the map holds lists; the clamp keeps a stale word inside the table)
        for (int t = lane * 4; t < d; t += group * 4) {
            if (VEC) {
                f32x4 v[4 * MQ], c4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int j = 0; j < 4 * MQ; ++j)
                    if (j < m) v[j] = *reinterpret_cast<const f32x4 *>(cw[j] + t);      // independent: all in flight before the first add
                if (COARSE) c4 = *reinterpret_cast<const f32x4 *>(cc + t);
                f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};                                   // from +0.0
#pragma unroll
                for (int j = 0; j < 4 * MQ; ++j)
                    if (j < m) acc = acc + v[j];                                         // codebooks ascending
                if (COARSE) acc = acc + c4;
                *reinterpret_cast<f32x4 *>(o + t) = acc;
            } else {
                float v[4 * MQ][4], c4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int j = 0; j < 4 * MQ; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[j][e] = (j < m && t + e < d) ? cw[j][t + e] : 0.0f;
                if (COARSE) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (t + e < d) c4[e] = cc[t + e];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float acc = 0.0f;
#pragma unroll
                    for (int j = 0; j < 4 * MQ; ++j)
                        if (j < m) acc = acc + v[j][e];
                    if (COARSE) acc = acc + c4[e];
                    if (t + e < d) o[t + e] = acc;
                }
            }
        }
    }
}

// ids outside [id_base, id_base + n): counted -- one add per wave that saw one.  The one kernel that reads the ids before a decode without PAD
__global__ __launch_bounds__(256) void recon_check_ids_kernel(const int32_t *__restrict__ ids, int64_t count, int id_base, int64_t n, unsigned *__restrict__ bad) {
    unsigned mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        const int64_t r = (int64_t)ids[i] - id_base;
        mine += (r < 0 || r >= n) ? 1u : 0u;
    }
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(bad, mine);
}

// the row -> list map from the inverted layout: position p holds original row ids[p] and lies in the list l with off[l] <= p < off[l + 1].  The original
// ids are distinct, so every lor entry is written once: plain stores, no atomics
__global__ __launch_bounds__(256) void recon_lor_kernel(const int *__restrict__ ids, const int *__restrict__ off, int64_t n, int nlist, int32_t *__restrict__ lor) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        int lo = 0, hi = nlist;                       // the last l with off[l] <= p (empty lists share an offset: the last of them is followed by a greater one)
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if ((int64_t)off[mid] <= p) lo = mid; else hi = mid;
        }
        const int64_t row = ids[p];
        if (row >= 0 && row < n) lor[row] = lo;
    }
}

template <int MQ, bool VEC, bool CW>
void recon_pick(const ReconArgs &a, bool coarse, bool pad, dim3 grid, hipStream_t s) {
    const bool ids = a.ids != nullptr;
#define RECON_GO(I, C, P) hipLaunchKernelGGL((recon_kernel<MQ, VEC, CW, I, C, P>), grid, dim3(RECON_BLOCK), 0, s, a)
    if (!ids) { if (coarse) RECON_GO(false, true, false); else RECON_GO(false, false, false); }
    else if (!pad) { if (coarse) RECON_GO(true, true, false); else RECON_GO(true, false, false); }
    else { if (coarse) RECON_GO(true, true, true); else RECON_GO(true, false, true); }
#undef RECON_GO
}

template <int MQ>
void recon_pick_road(const ReconArgs &a, bool vec, bool cw, bool coarse, bool pad, dim3 grid, hipStream_t s) {
    if (vec) { if (cw) recon_pick<MQ, true, true>(a, coarse, pad, grid, s); else recon_pick<MQ, true, false>(a, coarse, pad, grid, s); }
    else { if (cw) recon_pick<MQ, false, true>(a, coarse, pad, grid, s); else recon_pick<MQ, false, false>(a, coarse, pad, grid, s); }
}

}  // namespace

int lsq_recon_launch(hipStream_t s, const lsq_recon_call &c, int *road) {
    if (road) *road = 0;
    if (c.count <= 0) return LSQ_OK;
    ReconArgs a{};
    a.codes = c.codes; a.ldc = c.ldc; a.K = c.K; a.d = c.d; a.m = c.m; a.n = c.n;
    a.ids = c.ids; a.id_base = c.id_base; a.start = c.start; a.count = c.count;
    a.out = c.out; a.ldo = c.ldo; a.cent = c.cent; a.lor = c.lor; a.nlist = c.nlist;
    const bool coarse = c.cent != nullptr;
    // the roads: 16-byte loads and stores where every address they form is 16-byte aligned; dword code rows where the pitch keeps them inside the row
    const bool vec = (c.d & 3) == 0 && (c.ldo & 3) == 0 && ((uintptr_t)c.K & 15) == 0 && ((uintptr_t)c.out & 15) == 0 && (!coarse || ((uintptr_t)c.cent & 15) == 0);
    const bool cw = (c.ldc & 3) == 0 && ((uintptr_t)c.codes & 3) == 0;
    const int quads = (c.d + 3) / 4;
    int gshift = 0;
    while ((1 << gshift) < quads && gshift < 6) ++gshift;
    a.gshift = gshift;
    const int rows_per_block = RECON_BLOCK >> gshift;
    const int64_t blocks = std::min<int64_t>((c.count + rows_per_block - 1) / rows_per_block, RECON_MAX_BLOCKS);
    const dim3 grid((unsigned)blocks);
    switch ((c.m + 3) / 4) {
        case 1: recon_pick_road<1>(a, vec, cw, coarse, c.pad_nan != 0, grid, s); break;
        case 2: recon_pick_road<2>(a, vec, cw, coarse, c.pad_nan != 0, grid, s); break;
        case 3: recon_pick_road<3>(a, vec, cw, coarse, c.pad_nan != 0, grid, s); break;
        default: recon_pick_road<4>(a, vec, cw, coarse, c.pad_nan != 0, grid, s); break;
    }
    LSQ_HIP(hipGetLastError());
    if (road) *road = (vec ? LSQ_RECON_ROAD_VEC16 : LSQ_RECON_ROAD_DWORD) | (cw ? LSQ_RECON_ROAD_CODE_DWORDS : 0);
    return LSQ_OK;
}

int lsq_recon_launch_check_ids(hipStream_t s, const int32_t *ids, int64_t count, int id_base, int64_t n, unsigned *bad) {
    if (count <= 0) return LSQ_OK;
    const int64_t blocks = std::min<int64_t>((count + 255) / 256, 1024);
    hipLaunchKernelGGL(recon_check_ids_kernel, dim3((unsigned)blocks), dim3(256), 0, s, ids, count, id_base, n, bad);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

int lsq_recon_launch_lor(hipStream_t s, const int *ids, const int *off, int64_t n, int nlist, int32_t *lor) {
    if (n <= 0 || nlist <= 0) return LSQ_OK;
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(recon_lor_kernel, dim3((unsigned)blocks), dim3(256), 0, s, ids, off, n, nlist, lor);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

// the host checker and the engine-less road (lsq_recon_check.h holds the body: a stand-alone program runs it under sanitizers)
extern "C" int lsq_reconstruct_cpu(float *out, int64_t ldo, const uint8_t *codes, int64_t ldc, const float *K, const int32_t *ids, int64_t count, int id_base,
                                   int64_t n, int m, int h, int d, const float *centroids, const int32_t *list_of_row, int flags, int nthreads) {
    const lsq_recon_cpu_args a{out, ldo, codes, ldc, K, ids, count, id_base, n, m, h, d, centroids, list_of_row, flags};
    if (const char *why = lsq_recon_cpu(a, nthreads)) {
        lsq_set_error("lsq_reconstruct_cpu: %s (n=%lld count=%lld m=%d h=%d d=%d ldc=%lld ldo=%lld id_base=%d flags=%d)", why, (long long)n, (long long)count, m, h,
                      d, (long long)ldc, (long long)ldo, id_base, flags);
        return LSQ_EINVAL;
    }
    return LSQ_OK;
}
