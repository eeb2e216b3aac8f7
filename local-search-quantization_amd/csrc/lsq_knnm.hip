// lsq_knnm.hip -- the MFMA PRE-FILTER of exact k-NN (gfx950; option "knn_prefilter").
//
// lsq_knn.hip computes every distance of the thresholded road by the direct chain  ((0 + e_0 e_0) + e_1 e_1) + ...,  e_s = x[s] - q[s]: three VALU
// element-ops per (query, row, dimension), of which all but a few per million pairs end in "dist > tau: nothing to append".  This unit decides that
// question on the f32 matrix cores instead and leaves the chain to the pairs it cannot decide:
//
//   norms    knnm_norms_kernel      Nx[i] = SUM_s x_i[s]^2,  Nq[q] = SUM_s q[s]^2     (f32 fma chains, elements widened exactly first)
//   MFMA     knnm_scan_kernel<TX>   a = (Nx + Nq) - 2 <x, q>  with <x, q> by v_mfma_f32_32x32x2_f32;  the pair is DROPPED iff
//                                   a > tau_q + kappa_d (Nx + Nq) + eta_d,   otherwise its row id joins the query's PENDING list
//   recheck  knnm_recheck_kernel<TX> the direct chain of every pending pair (the contract's bits), knn_scan_kernel's own test !(dist > tau) and its
//                                   own append: the candidate lists receive the SAME set of records as MODE 0 of knn_scan_kernel.
//
// The window kappa_d N + eta_d bounds |a - dist| over every rounding of both computations (lsq_knn_prefilter_bound; the proof is DESIGN 4.29), so no pair
// with dist <= tau is dropped; NaN or inf anywhere makes the comparison false and the pair pending.  What the window cannot bound is how MANY pairs it
// lets through: a pending list holds pcap ids, a query whose list overflows is marked (knnm_mark_kernel: fail = 2) and redone by the direct scan.
//
// knnm_scan_kernel: 256 threads = 2 x 2 waves, block tile 128 base rows x 128 queries, each wave 64 x 64 = 2 x 2 accumulators of 32 x 32 (64 registers).
// The MFMA M dimension carries the ROWS and N the QUERIES: a lane's 64 accumulator values belong to TWO queries (its column of either N tile), whose
// tau, Nq and liveness it keeps in registers, and to 32 rows whose Nx it reads from LDS.  K is staged 16 dimensions at a time into double-buffered LDS
// panels [row][16] of pitch 20 floats; the next chunk's global loads are in flight while the MFMAs of the current one run, one barrier per chunk.
// The pre-filter's bound holds for ANY order of the d products, so the chain need not be k-ascending (lsq_gemm.hip's contract): MFMA step s of a chunk
// multiplies dimensions s (lanes 0-31) and 8 + s (lanes 32-63), and a lane fetches its eight operands of a row as TWO ds_read_b128 instead of eight
// ds_read_b32 -- 8 LDS reads per 32 MFMAs.  Pitch 20: sixteen consecutive lanes' 16-byte reads fall on sixteen distinct bank quads.
// Rows >= n, query slots >= nqb and dimensions >= d are staged as zeros (0 * 0 adds +0) and never emit; nothing at or past a row's d-th element is loaded.
// Staging is by single elements (16 consecutive lanes read 16 consecutive elements of one row): any d, any pitch, any element alignment, one loader for
// f32, f16, bf16 and uint8 rows.  16 loads and 16 LDS writes per thread stand against 2048 MFMA cycles per chunk.
#include <math.h>

#include "lsq_internal.h"
#include "lsq_xload.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int KM_THREADS = 256;
constexpr int KM_T = 128;                    // rows per block step = queries per block
constexpr int KM_BK = 16;                    // dimensions staged per chunk
constexpr int KM_LD = KM_BK + 4;             // LDS row pitch (floats): 16-byte aligned rows, LD / 4 odd
constexpr int KM_SL = KM_T * KM_BK / KM_THREADS;      // staged elements per thread, chunk and operand (8)

// out[i] = SUM_s X[i][s]^2: 16 lanes per row, each an fma chain over its elements s = lane, lane + 16, ..., then the tree over the 16 partial sums.
// Every product enters through one rounding and the terms are non-negative: |out - N| <= gamma_d N whatever the order
template <typename T>
__global__ __launch_bounds__(KM_THREADS) void knnm_norms_kernel(const T *__restrict__ X, int64_t ld, int n, int d, float *__restrict__ out) {
    const int kk = threadIdx.x & 15;
    for (int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); i < n; i += (int64_t)gridDim.x * 16) {      // (a 16-lane group shares i: it leaves together)
        const T *row = X + i * ld;
        float acc = 0.0f;
        for (int s = kk; s < d; s += 16) {
            const float v = (float)row[s];
            acc = fmaf(v, v, acc);
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) acc = acc + __shfl_xor(acc, off, 16);
        if (kk == 0) out[i] = acc;
    }
}

template <typename TX>
__global__ __launch_bounds__(KM_THREADS, 2) void knnm_scan_kernel(const TX *__restrict__ X, int64_t ldb, const float *__restrict__ Q, int64_t ldq, int q0,
                                                               int nqb, int d, int n, int per_block, const float *__restrict__ nx,
                                                               const float *__restrict__ nqv, const uint32_t *__restrict__ tau, float kappa, float eta,
                                                               unsigned *pcount, int pcap, uint32_t *__restrict__ pend) {
    __shared__ __attribute__((aligned(16))) float xs[2][KM_T * KM_LD];
    __shared__ __attribute__((aligned(16))) float qs[2][KM_T * KM_LD];
    __shared__ float nxs[2][KM_T];
    const int t = threadIdx.x, tile = blockIdx.x;
    const int64_t first = (int64_t)blockIdx.y * per_block;
    const int64_t last = first + per_block < n ? first + per_block : (int64_t)n;
    if (first >= last) return;
    // staging roles: element j of this thread is (row / query (t >> 4) + 16 j, dimension t & 15 of the chunk)
    const int kk = t & (KM_BK - 1), sr = t >> 4;
    const int qslot0 = tile * KM_T + sr;                            // the thread's first query slot; the others 16 j further
    const float *qbase = Q + (int64_t)(q0 + qslot0) * ldq;          // (never dereferenced past the batch)
    float qreg[KM_SL];
    TX xreg[KM_SL];
    auto fetch = [&](int64_t r0, int k0) {                          // global -> registers: chunk k0 of the queries and of rows r0 .. r0 + 127
        const int k = k0 + kk;
#pragma unroll
        for (int j = 0; j < KM_SL; ++j) qreg[j] = (qslot0 + 16 * j < nqb && k < d) ? qbase[(int64_t)(16 * j) * ldq + k] : 0.0f;
#pragma unroll
        for (int j = 0; j < KM_SL; ++j) {
            const int64_t row = r0 + sr + 16 * j;
            xreg[j] = (row < last && k < d) ? X[row * ldb + k] : (TX)0;
        }
    };
    auto stage = [&](int buf) {                                     // registers -> LDS, widened (exact)
#pragma unroll
        for (int j = 0; j < KM_SL; ++j) {
            qs[buf][(sr + 16 * j) * KM_LD + kk] = qreg[j];
            xs[buf][(sr + 16 * j) * KM_LD + kk] = (float)xreg[j];
        }
    };
    // compute roles
    const int lane = t & 63, wave = t >> 6;
    const int wy = wave >> 1, wx = wave & 1, l31 = lane & 31, lhi = lane >> 5;
    // the lane's two queries: column l31 of N tile tj.  A slot past the batch never emits (tq = -inf would not do: NaN norms pass every test)
    int slot2[2];
    bool live[2];
    float tq[2], nq2[2];
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
        slot2[tj] = tile * KM_T + wx * 64 + tj * 32 + l31;
        live[tj] = slot2[tj] < nqb;
        tq[tj] = live[tj] ? lsq_adc_unkey(tau[slot2[tj]]) : 0.0f;
        nq2[tj] = live[tj] ? nqv[q0 + slot2[tj]] : 0.0f;
    }
    const int nk = (d + KM_BK - 1) / KM_BK;
    fetch(first, 0);
    stage(0);
    int cur = 0, par = 0;
    for (int64_t r0 = first; r0 < last; r0 += KM_T, par ^= 1) {
        // Nx of this step's rows: read after at least one barrier of the chunk loop, overwritten two steps later (after the next step's barriers)
        if (t < KM_T) nxs[par][t] = r0 + t < last ? nx[r0 + t] : 0.0f;
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
            const bool more_k = kc + 1 < nk, more = more_k || r0 + KM_T < last;
            if (more_k) fetch(r0, (kc + 1) * KM_BK);
            else if (more) fetch(r0 + KM_T, 0);
            const f32x4 *ap = reinterpret_cast<const f32x4 *>(xs[cur] + (wy * 64 + l31) * KM_LD + 8 * lhi);
            const f32x4 *bp = reinterpret_cast<const f32x4 *>(qs[cur] + (wx * 64 + l31) * KM_LD + 8 * lhi);
            const f32x4 a0[2] = {ap[0], ap[1]}, a1[2] = {ap[32 * KM_LD / 4], ap[32 * KM_LD / 4 + 1]};
            const f32x4 b0[2] = {bp[0], bp[1]}, b1[2] = {bp[32 * KM_LD / 4], bp[32 * KM_LD / 4 + 1]};
#pragma unroll
            for (int s = 0; s < 8; ++s) {                           // step s: dimensions s (lanes 0-31) and 8 + s (lanes 32-63) of the chunk
                const float av0 = a0[s >> 2][s & 3], av1 = a1[s >> 2][s & 3];
                const float bv0 = b0[s >> 2][s & 3], bv1 = b1[s >> 2][s & 3];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, bv0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, bv1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, bv0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, bv1, acc[1][1], 0, 0, 0);
            }
            if (more) stage(cur ^ 1);                               // the other buffer was last read one chunk ago (barrier below)
            __syncthreads();
            cur ^= 1;
        }
        // epilogue: accumulator (ti, tj)[r] is row r0 + wy 64 + ti 32 + (r & 3) + 8 (r >> 2) + 4 lhi, query slot2[tj]
        // Two stages: a branch-free pass that leaves one bit per pair (bit 16 ti + r of the query's word), then the rare appends bit by bit -- the
        // accumulators are dead before the first atomic is issued
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

constexpr int KR_KC = 32;                    // dimensions staged per chunk
constexpr int KR_RP = KM_THREADS + 1;        // padded LDS pitch (floats)

// One block: query slot blockIdx.y, pending entries tile * 256 .. of its list; lane t owns ONE (query, row) pair from its first dimension to its last.
// Staging: 32 consecutive lanes read 32 consecutive elements of one row (a 128-byte line of an f32 row), widened into LDS transposed [dimension][pair];
// the owner walks them back with conflict-free reads against the block's query (block-uniform addresses).  A list that overflowed is not rechecked:
// its query keeps count = 0, fails the selection and is redone.
template <typename TX>
__global__ __launch_bounds__(KM_THREADS) void knnm_recheck_kernel(const TX *__restrict__ X, int64_t ldb, const float *__restrict__ Q, int64_t ldq, int q0,
                                                                  int d, const unsigned *__restrict__ pcount, int pcap,
                                                                  const uint32_t *__restrict__ pend, const uint32_t *__restrict__ tau,
                                                                  unsigned *__restrict__ count, int cap, uint64_t *__restrict__ out, int idbits) {
    __shared__ float xs[KR_KC * KR_RP];
    __shared__ uint32_t ids[KM_THREADS];
    const int t = threadIdx.x, slot = blockIdx.y;
    const unsigned have = pcount[slot];
    if (have > (unsigned)pcap) return;
    const int left = (int)have - (int)blockIdx.x * KM_THREADS;      // pairs of this tile
    if (left <= 0) return;
    ids[t] = t < left ? pend[(int64_t)slot * pcap + (int64_t)blockIdx.x * KM_THREADS + t] : 0u;
    __syncthreads();
    const float *__restrict__ q = Q + (int64_t)(q0 + slot) * ldq;   // block-uniform
    const int kk = t & (KR_KC - 1), sr = t >> 5;                    // staging roles: dimension kk of the chunk, pairs sr + 8 j
    float acc = 0.0f;
    for (int k0 = 0; k0 < d; k0 += KR_KC) {
        const int kc = d - k0 < KR_KC ? d - k0 : KR_KC;             // uniform
        __syncthreads();                                            // the previous chunk has been walked
#pragma unroll 8
        for (int j = 0; j < KM_THREADS / 8; ++j) {
            const int p = sr + 8 * j;
            if (p < left && kk < kc) xs[kk * KR_RP + p] = (float)X[(int64_t)ids[p] * ldb + k0 + kk];
        }
        __syncthreads();
        if (t < left) {
            for (int s = 0; s < kc; ++s) {
                const float e = xs[s * KR_RP + t] - q[k0 + s];      // x - q, rounded; the square, rounded; then the add (no FMA)
                acc = acc + e * e;
            }
        }
    }
    if (t >= left) return;
    if (acc > lsq_adc_unkey(tau[slot])) return;                     // knn_scan_kernel's test: emit unless dist > tau
    const uint64_t rec = ((uint64_t)lsq_adc_key(acc) << idbits) | (uint64_t)((int64_t)ids[t] + 1);
    const unsigned at = atomicAdd(&count[slot], 1u);
    if (at < (unsigned)cap) out[(int64_t)slot * cap + at] = rec;
}

// fail[slot] = 2 for a query whose pending list overflowed (its candidate list was left empty: the selection has set 1)
__global__ void knnm_mark_kernel(const unsigned *__restrict__ pcount, int pcap, int *__restrict__ fail, int nqb) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot < nqb && pcount[slot] > (unsigned)pcap) fail[slot] = LSQ_KNNM_FAIL_OVERFLOW;
}

template <typename T>
int launch_norms(hipStream_t s, const T *X, int64_t ld, int n, int d, float *out) {
    if (n <= 0) return LSQ_OK;
    const int64_t blocks = ((int64_t)n + 15) / 16;
    hipLaunchKernelGGL((knnm_norms_kernel<T>), dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(KM_THREADS), 0, s, X, ld, n, d, out);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

template <typename TX>
int launch_road(hipStream_t s, const lsq_search_input &in, int q0, int nqb, const uint32_t *tau, unsigned *count, int cap, uint64_t *out, int idbits,
                const lsq_knnm_work &w) {
    const TX *X = static_cast<const TX *>(in.base);
    const float *Q = static_cast<const float *>(in.Q);
    const int n = in.n, d = in.d;
    const int tiles = (nqb + KM_T - 1) / KM_T;
    // lsq_knn_launch_scan's grid rule: ~2048 blocks, ranges of at least 8 row steps
    int ranges = (2048 + tiles - 1) / tiles;
    const int max_ranges = (int)(((int64_t)n + 8 * KM_T - 1) / (8 * KM_T));
    if (ranges > max_ranges) ranges = max_ranges;
    if (ranges < 1) ranges = 1;
    if (ranges > 65535) ranges = 65535;
    int64_t per_block = ((int64_t)n + ranges - 1) / ranges;
    per_block = (per_block + KM_T - 1) / KM_T * KM_T;
    ranges = (int)(((int64_t)n + per_block - 1) / per_block);
    LSQ_HIP(hipMemsetAsync(w.pcount, 0, sizeof(unsigned) * (size_t)nqb, s));
    if (w.qpieces) {                                  // half-precision rows on the 16-bit tile (lsq_knnh.hip): split the queries, then its scan
        if (w.clock) LSQ_TRY(w.clock->mark(s));
        LSQ_TRY(lsq_knnh_launch_split(s, in, q0, nqb, w.qpieces));
        if (w.clock) LSQ_TRY(w.clock->mark(s));
        LSQ_TRY(lsq_knnh_launch_scan(s, in, q0, nqb, tau, w));
    } else {
        if (w.clock) LSQ_TRY(w.clock->mark(s));
        hipLaunchKernelGGL((knnm_scan_kernel<TX>), dim3((unsigned)tiles, (unsigned)ranges), dim3(KM_THREADS), 0, s, X, (int64_t)in.bstride, Q,
                           (int64_t)in.qstride, q0, nqb, d, n, (int)per_block, w.nx, w.nq, tau, w.kappa, w.eta, w.pcount, w.pcap, w.pend);
        LSQ_HIP(hipGetLastError());
    }
    if (w.clock) LSQ_TRY(w.clock->mark(s));
    const int rtiles = (w.pcap + KM_THREADS - 1) / KM_THREADS;
    hipLaunchKernelGGL((knnm_recheck_kernel<TX>), dim3((unsigned)rtiles, (unsigned)nqb), dim3(KM_THREADS), 0, s, X, (int64_t)in.bstride, Q,
                       (int64_t)in.qstride, q0, d, w.pcount, w.pcap, w.pend, tau, count, cap, out, idbits);
    LSQ_HIP(hipGetLastError());
    if (w.clock) LSQ_TRY(w.clock->mark(s));
    return LSQ_OK;
}

}  // namespace

// kappa_d = (4 d + 32) 2^-24 1.01 (computed in double, rounded UP to float), eta_d = (4 d + 32) 2^-120 (exact): |a - dist| <= kappa_d (Nx + Nq) + eta_d
extern "C" int lsq_knn_prefilter_bound(int d, float *kappa, float *eta) {
    if (d < 1 || d > LSQ_KNN_PREFILTER_MAX_D || !kappa || !eta) {
        lsq_set_error("lsq_knn_prefilter_bound: needs 1 <= d <= %d and two pointers (got d=%d)", LSQ_KNN_PREFILTER_MAX_D, d);
        return LSQ_EINVAL;
    }
    const double c = 4.0 * d + 32.0, k = c * ldexp(1.0, -24) * 1.01;
    float kf = (float)k;
    if ((double)kf < k) kf = nextafterf(kf, INFINITY);
    *kappa = kf;
    *eta = (float)ldexp(c, -120);
    return LSQ_OK;
}

// the norms of the call: nx [n] of the base rows (in's element type), nqv [nq] of the f32 queries.  Nothing is kept between calls: a borrowed base may change
int lsq_knnm_launch_norms(hipStream_t s, const lsq_search_input &in, int nq, float *nx, float *nqv) {
    LSQ_TRY(launch_norms(s, static_cast<const float *>(in.Q), (int64_t)in.qstride, nq, in.d, nqv));
    const int fmt = lsq_base_format(in.base_u8);
    if (fmt == LSQ_BASE_F16) return launch_norms(s, static_cast<const lsq_f16 *>(in.base), (int64_t)in.bstride, in.n, in.d, nx);
    if (fmt == LSQ_BASE_BF16) return launch_norms(s, static_cast<const lsq_bf16 *>(in.base), (int64_t)in.bstride, in.n, in.d, nx);
    if (fmt) return launch_norms(s, static_cast<const uint8_t *>(in.base), (int64_t)in.bstride, in.n, in.d, nx);
    return launch_norms(s, static_cast<const float *>(in.base), (int64_t)in.bstride, in.n, in.d, nx);
}

int lsq_knnm_launch_row_norms(hipStream_t s, const void *X, int x_u8, int64_t ld, int n, int d, float *out) {
    if (x_u8) return launch_norms(s, static_cast<const uint8_t *>(X), ld, n, d, out);
    return launch_norms(s, static_cast<const float *>(X), ld, n, d, out);
}

// MODE 0 of one batch on the pre-filtered road: pending lists, then the recheck into the candidate lists (count zeroed by the caller, as for the direct scan)
int lsq_knnm_launch(hipStream_t s, const lsq_search_input &in, int q0, int nqb, const uint32_t *tau, unsigned *count, int cap, uint64_t *out, int idbits,
                    const lsq_knnm_work &w) {
    if (nqb <= 0 || in.n <= 0) return LSQ_OK;
    const int fmt = lsq_base_format(in.base_u8);
    if (fmt == LSQ_BASE_F16) return launch_road<lsq_f16>(s, in, q0, nqb, tau, count, cap, out, idbits, w);
    if (fmt == LSQ_BASE_BF16) return launch_road<lsq_bf16>(s, in, q0, nqb, tau, count, cap, out, idbits, w);
    if (fmt) return launch_road<uint8_t>(s, in, q0, nqb, tau, count, cap, out, idbits, w);
    return launch_road<float>(s, in, q0, nqb, tau, count, cap, out, idbits, w);
}

int lsq_knnm_launch_mark(hipStream_t s, const unsigned *pcount, int pcap, int *fail, int nqb) {
    hipLaunchKernelGGL(knnm_mark_kernel, dim3((unsigned)((nqb + 255) / 256)), dim3(256), 0, s, pcount, pcap, fail, nqb);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}
