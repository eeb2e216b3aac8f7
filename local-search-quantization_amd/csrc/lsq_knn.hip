// lsq_knn.hip -- exact brute-force k-NN ON THE DEVICE (gfx950): the ground truth every recall figure depends on.
//
// The reference reads its ground truth from sift_groundtruth.ivecs, which only describes the full SIFT1M base.  This computes it for any float base:
//
//   dist(q, i) = ((0 + e_0 e_0) + e_1 e_1) + ... + e_{d-1} e_{d-1},   e_s = x_i[s] - q[s]     f32, s ascending, every op rounded (no FMA)
//   result     = the nn smallest (dist, id) pairs in lexicographic order, ids 0-BASED; NaN sorts last
//
// -- the sub-space table rule of the PQ scan (linscan_aqd.cpp:66-74) with one sub-space of width d, so the PQ host drop-in with the base rows as
// centres computes the same bits.  The direct form, not |x|^2 + |q|^2 - 2<q, x> on MFMA: the expanded form cancels on near-ties, so it cannot be
// ground truth.
//
// This file is the distance PRODUCER of the ADC scan's selection (lsq_adc.hip): it writes the same records (order-preserving distance key << idbits
// | id + 1) in the same three modes as adc_scan_kernel, so that make_plan, the threshold rank select, the segmented sort, the gather and the
// exhaustive fallback serve it unchanged.  adc_search routes its "exact" input kind here (lsq_knn_launch_scan) and skips the table build.
//
// Kernel: a block of 256 threads holds a tile of QT = 128 queries and RT = 64 base rows in LDS, both transposed ([s][row]) and staged KD = 16
// dimensions at a time (zero-padded past d: 0 - 0 = +0 adds +0, which leaves every partial sum -- never -0 -- unchanged, so any d runs the same
// unrolled loop).  A lane owns 8 queries x 4 rows: per dimension three ds_read_b128 and 16 v_pk_add_f32 (the subtract) + 16 v_pk_mul_f32 + 16
// v_pk_add_f32 on float2 pairs of queries.  The next chunk's global loads are in flight while the current chunk is walked.
#include "lsq_internal.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int KNN_THREADS = 256;
constexpr int KNN_QT = 128;                  // queries per block: 16 query groups x 8
constexpr int KNN_RT = 64;                   // base rows per block step: 16 row groups x 4
constexpr int KNN_KD = 16;                   // dimensions staged per pass
constexpr int KNN_QP = KNN_QT + 4;           // padded LDS row pitches (floats): the transposed stores hit 16 distinct banks per wave
constexpr int KNN_RP = KNN_RT + 4;
constexpr int KNN_QL = KNN_QT * KNN_KD / KNN_THREADS;      // staged query floats per thread (8)
constexpr int KNN_RL = KNN_RT * KNN_KD / KNN_THREADS;      // staged row floats per thread (4)

// MODE 0: append (key << idbits | i + 1) of every distance <= tau to the query's candidate list;  MODE 1: write every record of the strided subset
// i = s * stride, s < ns, to out[slot * ns + s];  MODE 2: the same subset, keys only (u32).  Query of slot: qsel[slot] (fallback) or q0 + slot.
template <int MODE>
__global__ __launch_bounds__(KNN_THREADS) void knn_scan_kernel(const float *__restrict__ X, int ldb, const float *__restrict__ Q, int ldq,
                                                               const int *__restrict__ qsel, int q0, int nqb, int d, int stride, int total,
                                                               int per_block, const uint32_t *__restrict__ tau, unsigned *__restrict__ count,
                                                               int cap, uint64_t *__restrict__ out, int idbits) {
    __shared__ __attribute__((aligned(16))) float qs[KNN_KD * KNN_QP];
    __shared__ __attribute__((aligned(16))) float xs[KNN_KD * KNN_RP];
    const int t = threadIdx.x, tile = blockIdx.x;
    const int first = blockIdx.y * per_block;
    const int last = first + per_block < total ? first + per_block : total;
    if (first >= last) return;
    // staging roles: element j of this thread is (query / row (t >> 4) + 16 j, dimension t & 15): 16 consecutive threads read one row's chunk
    const int kk = t & (KNN_KD - 1), sr = t >> 4;
    const float *qrow[KNN_QL];
#pragma unroll
    for (int j = 0; j < KNN_QL; ++j) {
        const int slot = tile * KNN_QT + sr + 16 * j;
        qrow[j] = slot < nqb ? Q + (int64_t)(qsel ? qsel[slot] : q0 + slot) * ldq : nullptr;
    }
    float qreg[KNN_QL], xreg[KNN_RL];
    auto fetch = [&](int r0, int k0) {                              // global -> registers: chunk k0 of queries and of rows r0 .. r0 + RT - 1
        const int k = k0 + kk;
#pragma unroll
        for (int j = 0; j < KNN_QL; ++j) qreg[j] = (qrow[j] && k < d) ? qrow[j][k] : 0.0f;
#pragma unroll
        for (int j = 0; j < KNN_RL; ++j) {
            const int s = r0 + sr + 16 * j;
            xreg[j] = (s < last && k < d) ? X[(int64_t)s * stride * ldb + k] : 0.0f;
        }
    };
    // compute roles: query group qg owns queries 4 qg .. 4 qg + 3 and 64 + 4 qg .. 64 + 4 qg + 3, row group rg rows 4 rg .. 4 rg + 3
    const int qg = t & 15, rg = t >> 4;
    float tf[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int slot = tile * KNN_QT + (c < 4 ? 4 * qg + c : 64 + 4 * qg + c - 4);
        tf[c] = (MODE == 0 && slot < nqb) ? lsq_adc_unkey(tau[slot]) : -__builtin_inff();
    }
    const int nk = (d + KNN_KD - 1) / KNN_KD;
    fetch(first, 0);
    for (int r0 = first; r0 < last; r0 += KNN_RT) {
        f32x2 acc[4][4];                                            // [row j][query pair p]: pairs (4 qg + 2p, + 1) for p < 2, (64 + 4 qg + 2(p - 2), + 1)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int p = 0; p < 4; ++p) acc[j][p] = (f32x2){0.0f, 0.0f};
        for (int kc = 0; kc < nk; ++kc) {
            __syncthreads();                                        // the previous chunk has been walked
#pragma unroll
            for (int j = 0; j < KNN_QL; ++j) qs[kk * KNN_QP + sr + 16 * j] = qreg[j];
#pragma unroll
            for (int j = 0; j < KNN_RL; ++j) xs[kk * KNN_RP + sr + 16 * j] = xreg[j];
            __syncthreads();
            if (kc + 1 < nk) fetch(r0, (kc + 1) * KNN_KD);
            else if (r0 + KNN_RT < last) fetch(r0 + KNN_RT, 0);
#pragma unroll
            for (int s = 0; s < KNN_KD; ++s) {
                const f32x4 qa = *reinterpret_cast<const f32x4 *>(qs + s * KNN_QP + 4 * qg);
                const f32x4 qb = *reinterpret_cast<const f32x4 *>(qs + s * KNN_QP + 64 + 4 * qg);
                const f32x4 xv = *reinterpret_cast<const f32x4 *>(xs + s * KNN_RP + 4 * rg);
                const f32x2 qp[4] = {qa.xy, qa.zw, qb.xy, qb.zw};
                const float xr[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const f32x2 e = (f32x2){xr[j], xr[j]} - qp[p];      // x - q, rounded; the square, rounded; then the add (no FMA)
                        acc[j][p] = acc[j][p] + e * e;
                    }
            }
        }
        // emission: row r0 + 4 rg + j, query slot of pair p, half h
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int s = r0 + 4 * rg + j;
            if (s >= last) continue;
            const int64_t i = (int64_t)s * stride;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int p = c >> 1;
                const float dv = (c & 1) ? acc[j][p].y : acc[j][p].x;
                const int slot = tile * KNN_QT + (c < 4 ? 4 * qg + c : 64 + 4 * qg + c - 4);
                if (slot >= nqb) continue;
                if (MODE == 0 && dv > tf[c]) continue;              // emit unless dist > tau (a NaN on either side emits)
                const uint32_t key = lsq_adc_key(dv);
                const uint64_t rec = ((uint64_t)key << idbits) | (uint64_t)(i + 1);      // 1-based in the record; the gather hands out 0-based ids
                if (MODE == 1) {
                    out[(int64_t)slot * total + s] = rec;
                } else if (MODE == 2) {
                    reinterpret_cast<uint32_t *>(out)[(int64_t)slot * total + s] = key;
                } else {
                    const unsigned at = atomicAdd(&count[slot], 1u);
                    if (at < (unsigned)cap) out[(int64_t)slot * cap + at] = rec;
                }
            }
        }
    }
}

}  // namespace

// The scan of one batch for adc_search's "exact" input kind.  MODE 0: rows 0 .. n-1 against tau; MODE 1 / 2: rows s * stride, s < ns.
int lsq_knn_launch_scan(hipStream_t s, int mode, const float *X, int ldb, const float *Q, int ldq, const int *qsel, int q0, int nqb, int n, int d,
                        int stride, int ns, const uint32_t *tau, unsigned *count, int cap, uint64_t *out, int idbits) {
    const int tiles = (nqb + KNN_QT - 1) / KNN_QT;
    const int total = mode == 0 ? n : ns;
    if (tiles == 0 || total == 0) return LSQ_OK;
    // ~2048 blocks (a few per CU), ranges of at least 8 row steps
    int ranges = (2048 + tiles - 1) / tiles;
    const int max_ranges = (total + 8 * KNN_RT - 1) / (8 * KNN_RT);
    if (ranges > max_ranges) ranges = max_ranges;
    if (ranges < 1) ranges = 1;
    if (ranges > 65535) ranges = 65535;
    int per_block = (total + ranges - 1) / ranges;
    per_block = (per_block + KNN_RT - 1) / KNN_RT * KNN_RT;
    ranges = (total + per_block - 1) / per_block;
    const dim3 grid((unsigned)tiles, (unsigned)ranges), block(KNN_THREADS);
    const int st = mode == 0 ? 1 : stride;
    if (mode == 0)
        hipLaunchKernelGGL(knn_scan_kernel<0>, grid, block, 0, s, X, ldb, Q, ldq, qsel, q0, nqb, d, st, total, per_block, tau, count, cap, out, idbits);
    else if (mode == 1)
        hipLaunchKernelGGL(knn_scan_kernel<1>, grid, block, 0, s, X, ldb, Q, ldq, qsel, q0, nqb, d, st, total, per_block, tau, count, cap, out, idbits);
    else
        hipLaunchKernelGGL(knn_scan_kernel<2>, grid, block, 0, s, X, ldb, Q, ldq, qsel, q0, nqb, d, st, total, per_block, tau, count, cap, out, idbits);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}
