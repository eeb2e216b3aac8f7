// lsq_knnh.hip -- the pre-filter of exact k-NN on HALF-PRECISION base rows, on the 16-bit matrix cores (gfx950; option "knn_prefilter_half").
//
// lsq_knnm.hip's MFMA pass widens f16 / bf16 rows to f32 and runs v_mfma_f32_32x32x2_f32.  A pre-filter only has to be CONSERVATIVE -- the recheck makes the
// result -- so the f32 queries need not be represented exactly: each component q becomes two bf16 pieces q1 = bf16(q), q2 = bf16(q - q1) (both round to nearest
// even, lsq_half_check.h's integer rule), |q - q1 - q2| <= 2^-17 |q|, and the dot product runs on v_mfma_f32_32x32x16_bf16, eight times the K per instruction:
//
//   split    knnh_split_kernel      the batch's queries -> a scratch panel [piece][query][d padded to 16] of bf16, zero past d (once per batch)
//   scan     knnh_scan_kernel<TX>   a = (Nx + Nq) - 2 dot,  dot = SUM over the PRODUCT PAIRS of the tile's K dimension:
//                                     bf16 rows  (x, q1) (x, q2)                          -- the row operand is the stored bytes, no conversion
//                                     f16 rows   (x_hi, q1) (x_hi, q2) (x_lo, q1)         -- x_hi = bf16(x), x_lo = x - x_hi, BOTH EXACT (x_lo has at most 4
//                                                                                            significant bits); (x_lo, q2) is dropped and sits in the bound
//                                   the pair is DROPPED iff  a > tau_q + kappa^h_d (Nx + Nq) + eta^h_d,  otherwise its row id joins the query's pending list
//
// Norms, pending lists and their capacity, the recheck, the overflow mark and the redo are lsq_knnm.hip's, unchanged: this unit only replaces the scan.  The
// window (lsq_knn_prefilter_half_bound; proof: DESIGN 4.31) adds to 4.29's the representation term rho (2^-16 for bf16 rows, 2^-15 for f16 rows) and the accumulation term (3 ceil(d / 16) + 3) eps_hw,
// where eps_hw = 2^-19 is a MEASURED property of the instruction with a margin of 8 (tools/ubench_mfma_bf16.hip), not a documented one.
//
// knnh_scan_kernel: 256 threads = 2 x 2 waves, block tile 128 rows x 128 queries, each wave 2 x 2 accumulators of 32 x 32; M carries the rows, N the queries
// (4.29's epilogue, verbatim).  K is staged BK dimensions at a time into double-buffered LDS panels [128][BK] of bf16, pitch BK + 8 halves: an operand of
// one MFMA (eight bf16: row / query l & 31, halves 8 (l >> 5) .. + 7 of the K step) is ONE ds_read_b128, and the pitch in 16-byte quads (5 at BK = 32, 3 at
// BK = 16) is odd, so sixteen consecutive lanes fall on sixteen distinct bank quads.  bf16 rows: BK = 32, three panels per buffer (x, q1, q2), 61 440 B; f16
// rows: BK = 16, four panels (x_hi, x_lo, q1, q2), 49 152 B -- two blocks per CU either way.  Staging is by 16-byte PIECES (eight halves): one global load
// where the base pointer is 16-byte aligned, the pitch a multiple of eight halves and the piece lies whole inside the row's d elements; every other piece --
// a view at an odd element, an odd pitch, the tail of a row -- by single elements, nothing at or past the d-th element of a row is loaded.  The next chunk's
// global loads are in flight under the MFMAs of the current one, one barrier per chunk.  Rows >= n, slots >= nqb and dimensions >= d are zeros and never emit.
// The query pieces are staged PER CHUNK at every d (DESIGN 4.31 says what keeping them resident would take).
#include <math.h>

#include "lsq_internal.h"
#include "lsq_xload.h"

#pragma clang fp contract(off)

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int KH_THREADS = 256;
constexpr int KH_T = 128;                    // rows per block step = queries per block

template <typename TX> struct KhFmt;
template <> struct KhFmt<lsq_bf16> { static constexpr int BK = 32, XP = 1; };      // dimensions per chunk, row panels
template <> struct KhFmt<lsq_f16> { static constexpr int BK = 16, XP = 2; };

// q -> q1 = bf16(q), q2 = bf16(q - q1), round to nearest even both (lsq_narrow1<lsq_bf16>: NaN stays NaN, inf stays inf in q1 -- and makes q2 NaN, which
// keeps every pair of the query).  q - q1 is exact in f32.  One thread per (slot, k < dpad)
__global__ __launch_bounds__(KH_THREADS) void knnh_split_kernel(const float *__restrict__ Q, int64_t ldq, int q0, int nqb, int d, int dpad,
                                                                uint16_t *__restrict__ out) {
    const int64_t at = (int64_t)blockIdx.x * KH_THREADS + threadIdx.x;
    if (at >= (int64_t)nqb * dpad) return;
    const int slot = (int)(at / dpad), k = (int)(at % dpad);
    uint32_t p1 = 0u, p2 = 0u;
    if (k < d) {
        const float q = Q[(int64_t)(q0 + slot) * ldq + k];
        p1 = lsq_narrow1<lsq_bf16>(q);
        p2 = lsq_narrow1<lsq_bf16>(q - __uint_as_float(p1 << 16));
    }
    out[at] = (uint16_t)p1;
    out[(int64_t)nqb * dpad + at] = (uint16_t)p2;
}

// eight halves of row `row` from element k on, as four dwords (element e in bits 16 (e & 1) .. of dword e >> 1), zero from the d-th element of the row on.
// vec (block-uniform): rows start 16-byte aligned and k is a multiple of 8 -- a piece that lies whole inside the row is one 16-byte load
__device__ inline u32x4 kh_load_piece(const uint16_t *__restrict__ row, int k, int d, bool vec) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (k >= d) return v;
    if (vec && k + 8 <= d) return *reinterpret_cast<const u32x4 *>(row + k);
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (k + e < d) v[e >> 1] |= (uint32_t)row[k + e] << (16 * (e & 1));
    return v;
}

// two f16 of one dword -> their bf16 parts: hi = bf16(x) (nearest even), lo = x - hi, which needs at most 4 significant bits and no exponent below 2^-24:
// its upper 16 bits are the whole of it.  inf -> (inf, NaN), NaN -> (NaN, NaN): the pair is kept
__device__ inline void kh_split_f16(uint32_t w, uint32_t *hi, uint32_t *lo) {
    const lsq_f32x2 x = lsq_widen2<lsq_f16>(w);
    const uint32_t h0 = lsq_narrow1<lsq_bf16>(x.x), h1 = lsq_narrow1<lsq_bf16>(x.y);
    const float l0 = x.x - __uint_as_float(h0 << 16), l1 = x.y - __uint_as_float(h1 << 16);
    *hi = h0 | (h1 << 16);
    *lo = (__float_as_uint(l0) >> 16) | (__float_as_uint(l1) & 0xffff0000u);
}

template <typename TX>
__global__ __launch_bounds__(KH_THREADS, 2) void knnh_scan_kernel(const uint16_t *__restrict__ X, int64_t ldb, int xvec, const uint16_t *__restrict__ QP,
                                                                 int q0, int nqb, int d, int dpad, int n, int per_block, const float *__restrict__ nx,
                                                                 const float *__restrict__ nqv, const uint32_t *__restrict__ tau, float kappa, float eta,
                                                                 unsigned *pcount, int pcap, uint32_t *__restrict__ pend) {
    constexpr int BK = KhFmt<TX>::BK, XP = KhFmt<TX>::XP;
    constexpr int LD = BK + 8;                        // panel pitch (halves): 16-byte aligned rows, LD / 8 odd
    constexpr int PPR = BK / 8;                       // 16-byte pieces of a row per chunk
    constexpr int NP = KH_T * PPR / KH_THREADS;       // pieces per thread, chunk and panel (2 at BK = 32, 1 at BK = 16)
    constexpr int KS = BK / 16;                       // MFMA K steps per chunk and product pair
    constexpr int PANEL = KH_T * LD;                  // halves
    __shared__ __attribute__((aligned(16))) uint16_t xs[2][XP][PANEL];
    __shared__ __attribute__((aligned(16))) uint16_t qs[2][2][PANEL];
    __shared__ float nxs[2][KH_T];
    const int t = threadIdx.x, tile = blockIdx.x;
    const int64_t first = (int64_t)blockIdx.y * per_block;
    const int64_t last = first + per_block < n ? first + per_block : (int64_t)n;
    if (first >= last) return;
    // staging roles: piece j of this thread is (row / query (t + 256 j) / PPR, halves 8 ((t + 256 j) % PPR) .. + 7 of the chunk)
    u32x4 xreg[NP], qreg[2][NP];
    auto fetch = [&](int64_t r0, int k0) {            // global -> registers: chunk k0 of rows r0 .. r0 + 127 and of both query pieces
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int pi = t + KH_THREADS * j, sr = pi / PPR, k = k0 + 8 * (pi % PPR);
            const int64_t row = r0 + sr;
            const u32x4 zero = {0u, 0u, 0u, 0u};
            xreg[j] = row < last ? kh_load_piece(X + row * ldb, k, d, xvec != 0) : zero;
            const int slot = tile * KH_T + sr;
            const bool qok = slot < nqb && k < dpad;  // the scratch panel: 16-byte aligned rows of dpad halves, zero past d
#pragma unroll
            for (int pc = 0; pc < 2; ++pc)
                qreg[pc][j] = qok ? *reinterpret_cast<const u32x4 *>(QP + ((int64_t)pc * nqb + slot) * dpad + k) : zero;
        }
    };
    auto stage = [&](int buf) {                       // registers -> LDS; f16 rows are split here, exactly
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int pi = t + KH_THREADS * j, at = (pi / PPR) * LD + 8 * (pi % PPR);
            if constexpr (XP == 1) {
                *reinterpret_cast<u32x4 *>(&xs[buf][0][at]) = xreg[j];
            } else {
                u32x4 hi, lo;
#pragma unroll
                for (int w = 0; w < 4; ++w) { uint32_t h, l; kh_split_f16(xreg[j][w], &h, &l); hi[w] = h; lo[w] = l; }
                *reinterpret_cast<u32x4 *>(&xs[buf][0][at]) = hi;
                *reinterpret_cast<u32x4 *>(&xs[buf][XP - 1][at]) = lo;
            }
            *reinterpret_cast<u32x4 *>(&qs[buf][0][at]) = qreg[0][j];
            *reinterpret_cast<u32x4 *>(&qs[buf][1][at]) = qreg[1][j];
        }
    };
    // compute roles (lsq_knnm.hip's)
    const int lane = t & 63, wave = t >> 6;
    const int wy = wave >> 1, wx = wave & 1, l31 = lane & 31, lhi = lane >> 5;
    int slot2[2];
    bool live[2];
    float tq[2], nq2[2];
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
        slot2[tj] = tile * KH_T + wx * 64 + tj * 32 + l31;
        live[tj] = slot2[tj] < nqb;
        tq[tj] = live[tj] ? lsq_adc_unkey(tau[slot2[tj]]) : 0.0f;
        nq2[tj] = live[tj] ? nqv[q0 + slot2[tj]] : 0.0f;
    }
    const int nk = (d + BK - 1) / BK;
    fetch(first, 0);
    stage(0);
    int cur = 0, par = 0;
    for (int64_t r0 = first; r0 < last; r0 += KH_T, par ^= 1) {
        if (t < KH_T) nxs[par][t] = r0 + t < last ? nx[r0 + t] : 0.0f;
        // a query whose pending list has already overflowed is redone by the direct scan whatever else it collects: stop its atomics
        bool open[2];
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
            open[tj] = live[tj] && __hip_atomic_load(&pcount[slot2[tj]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= (unsigned)pcap;
        f32x16 acc[2][2];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[ti][tj][r] = 0.0f;
        __syncthreads();                                            // the staged chunk (and nxs) is visible
        for (int kc = 0; kc < nk; ++kc) {
            const bool more_k = kc + 1 < nk, more = more_k || r0 + KH_T < last;
            if (more_k) fetch(r0, (kc + 1) * BK);
            else if (more) fetch(r0 + KH_T, 0);
            const int xo = (wy * 64 + l31) * LD + 8 * lhi, qo = (wx * 64 + l31) * LD + 8 * lhi;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {                       // K step ks: halves 16 ks + 8 lhi .. + 7 of the chunk, the same for both operands
                bf16x8 a[XP][2], b[2][2];
#pragma unroll
                for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
                    for (int xp = 0; xp < XP; ++xp) a[xp][ti] = *reinterpret_cast<const bf16x8 *>(&xs[cur][xp][xo + ti * 32 * LD + 16 * ks]);
#pragma unroll
                    for (int pc = 0; pc < 2; ++pc) b[pc][ti] = *reinterpret_cast<const bf16x8 *>(&qs[cur][pc][qo + ti * 32 * LD + 16 * ks]);
                }
#pragma unroll
                for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                    for (int tj = 0; tj < 2; ++tj) {
                        acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][ti], b[0][tj], acc[ti][tj], 0, 0, 0);       // (x | x_hi, q1)
                        acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][ti], b[1][tj], acc[ti][tj], 0, 0, 0);       // (x | x_hi, q2)
                        if constexpr (XP == 2)
                            acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][ti], b[0][tj], acc[ti][tj], 0, 0, 0);   // (x_lo, q1)
                    }
            }
            if (more) stage(cur ^ 1);                               // the other buffer was last read one chunk ago (barrier below)
            __syncthreads();
            cur ^= 1;
        }
        // epilogue (4.29's): accumulator (ti, tj)[r] is row r0 + wy 64 + ti 32 + (r & 3) + 8 (r >> 2) + 4 lhi, query slot2[tj].  A branch-free pass that leaves
        // one bit per pair, then the rare appends bit by bit
        const float *nxl = nxs[par] + wy * 64 + 4 * lhi;
        uint32_t keep[2] = {0u, 0u};
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float nxr = nxl[ti * 32 + (r & 3) + 8 * (r >> 2)];
#pragma unroll
                for (int tj = 0; tj < 2; ++tj) {
                    const float nsum = nxr + nq2[tj];
                    const float a = fmaf(-2.0f, acc[ti][tj][r], nsum);      // (Nx + Nq) - 2 dot: 2 dot is exact, one rounding
                    const float thr = fmaf(kappa, nsum, tq[tj]) + eta;
                    keep[tj] |= (a > thr) ? 0u : (1u << (16 * ti + r));     // the negated form: NaN or inf anywhere keeps the pair
                }
            }
        }
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
            uint32_t w = open[tj] ? keep[tj] : 0u;
            while (w) {
                const int b = __builtin_ctz(w);
                w &= w - 1u;
                const int64_t row = r0 + wy * 64 + 4 * lhi + (b >> 4) * 32 + (b & 3) + 8 * ((b & 15) >> 2);
                if (row >= last) continue;                          // a zero row past the range never emits
                const unsigned at = atomicAdd(&pcount[slot2[tj]], 1u);
                if (at < (unsigned)pcap) pend[(int64_t)slot2[tj] * pcap + at] = (uint32_t)row;
            }
        }
    }
}

}  // namespace

// eps_hw: per instruction and element, |result - (c + SUM_16 a_k b_k)| <= eps_hw (|c| + SUM |a_k b_k|).  Measured worst ratio 2^-22.36
// (tools/ubench_mfma_bf16.hip, profiles/knn_prefilter_half.jsonl); adopted: 8 x that, up to a power of two
static constexpr int KH_EPS_HW_LOG2 = -19;

// kappa^h_d = ((4 d + 32) 2^-24 + rho + (3 ceil(d / 16) + 3) eps_hw) 1.01 (in double, rounded UP to float), rho = 2^-16 (bf16 rows: the query split alone) or
// 2^-15 (f16 rows: the dropped pair (x_lo, q2) as well); eta^h_d = (8 d + 64) 2^-120 (exact)
extern "C" int lsq_knn_prefilter_half_bound(int d, int base_format, float *kappa, float *eta) {
    if (d < 1 || d > LSQ_KNN_PREFILTER_MAX_D || !lsq_base_is_half(base_format) || !kappa || !eta) {
        lsq_set_error("lsq_knn_prefilter_half_bound: needs 1 <= d <= %d, base_format LSQ_BASE_F16 or LSQ_BASE_BF16 and two pointers (got d=%d format=%d)",
                      LSQ_KNN_PREFILTER_MAX_D, d, base_format);
        return LSQ_EINVAL;
    }
    const double steps = 3.0 * ((d + 15) / 16) + 3.0;
    const double k = ((4.0 * d + 32.0) * ldexp(1.0, -24) + ldexp(1.0, base_format == LSQ_BASE_F16 ? -15 : -16) + steps * ldexp(1.0, KH_EPS_HW_LOG2)) * 1.01;
    float kf = (float)k;
    if ((double)kf < k) kf = nextafterf(kf, INFINITY);
    *kappa = kf;
    *eta = (float)ldexp(8.0 * d + 64.0, -120);
    return LSQ_OK;
}

int64_t lsq_knnh_scratch_bytes(int nqb, int d) { return (int64_t)2 * nqb * ((d + 15) / 16 * 16) * (int64_t)sizeof(uint16_t); }

// the batch's query pieces into `scratch` (lsq_knnh_scratch_bytes, 16-byte aligned)
int lsq_knnh_launch_split(hipStream_t s, const lsq_search_input &in, int q0, int nqb, uint16_t *scratch) {
    const int dpad = (in.d + 15) / 16 * 16;
    const int64_t items = (int64_t)nqb * dpad;
    hipLaunchKernelGGL(knnh_split_kernel, dim3((unsigned)((items + KH_THREADS - 1) / KH_THREADS)), dim3(KH_THREADS), 0, s, static_cast<const float *>(in.Q),
                       (int64_t)in.qstride, q0, nqb, in.d, dpad, scratch);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

// the scan of one batch in lsq_knnm.hip's launch_road: pending lists from the 16-bit tile (pcount zeroed by the caller)
int lsq_knnh_launch_scan(hipStream_t s, const lsq_search_input &in, int q0, int nqb, const uint32_t *tau, const lsq_knnm_work &w) {
    const int fmt = lsq_base_format(in.base_u8);
    if (!lsq_base_is_half(fmt) || !w.qpieces) { lsq_set_error("lsq_knnh_launch_scan: needs half-precision rows and the query pieces"); return LSQ_EINVAL; }
    const uint16_t *X = static_cast<const uint16_t *>(in.base);
    const int n = in.n, d = in.d, dpad = (d + 15) / 16 * 16;
    const int tiles = (nqb + KH_T - 1) / KH_T;
    // lsq_knnm.hip's grid rule: ~2048 blocks, ranges of at least 8 row steps
    int ranges = (2048 + tiles - 1) / tiles;
    const int max_ranges = (int)(((int64_t)n + 8 * KH_T - 1) / (8 * KH_T));
    if (ranges > max_ranges) ranges = max_ranges;
    if (ranges < 1) ranges = 1;
    if (ranges > 65535) ranges = 65535;
    int64_t per_block = ((int64_t)n + ranges - 1) / ranges;
    per_block = (per_block + KH_T - 1) / KH_T * KH_T;
    ranges = (int)(((int64_t)n + per_block - 1) / per_block);
    const int xvec = ((uintptr_t)X & 15) == 0 && in.bstride % 8 == 0;
    const dim3 grid((unsigned)tiles, (unsigned)ranges), block(KH_THREADS);
    if (fmt == LSQ_BASE_F16)
        hipLaunchKernelGGL((knnh_scan_kernel<lsq_f16>), grid, block, 0, s, X, (int64_t)in.bstride, xvec, w.qpieces, q0, nqb, d, dpad, n, (int)per_block, w.nx,
                           w.nq, tau, w.kappa, w.eta, w.pcount, w.pcap, w.pend);
    else
        hipLaunchKernelGGL((knnh_scan_kernel<lsq_bf16>), grid, block, 0, s, X, (int64_t)in.bstride, xvec, w.qpieces, q0, nqb, d, dpad, n, (int)per_block, w.nx,
                           w.nq, tau, w.kappa, w.eta, w.pcount, w.pcap, w.pend);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}
