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
//
// 8-bit rows and queries (the un-widened bytes of a .bvecs set: lsq_index_knn) take one of two roads to the SAME bits:
//   widened   knn_scan_kernel<MODE, TX, TQ> with uint8_t for either element type: byte loads, widened (exact) at the staging store; the hot loop is the
//             shared source above, so the result is that of the f32 instantiation on the widened matrices.
//   integer   knn_scan_u8_kernel<MODE>, uint8 x uint8 with d <= 258 only.  Every e_s^2 is an integer <= 255^2 and the chain's partial sums are
//             non-decreasing integers, so whenever the final D <= 2^24 each of them is representable and the chain returns (float)D; d 255^2 <= 2^24
//             holds up to d = 258.  D = N_x + N_q - 2 <x, q> in uint32 -- no rounding, no cancellation -- with <x, q> by v_dot4_u32_u8 on packed
//             dwords: the same tile, eight instructions per dimension instead of 48, a quarter of the bytes.
#include "lsq_internal.h"
#include "lsq_xload.h"

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
// TX / TQ: the element types of the rows and of the queries, float or uint8_t (widened where the staged registers are stored to LDS); TX also lsq_f16 /
// lsq_bf16 (lsq_xload.h), widened at the same place.
// FILT (a row filter, lsq_filter.hip; adc_scan_kernel's rule): frows == nullptr -- dense: walk position p IS the row and its bit of fbits decides whether it
// leaves a record; frows != nullptr -- compact: position p < nlive is row frows[p], positions past nlive (MODE 1's padding up to nn) are staged as zeros.
// A row that is filtered or padding does not pass (MODE 0), or leaves as the record of an id outside the base (MODE 1) / the key 0xffffffff (MODE 2).
// FILT = false: the kernel as it was, the three arguments unread.
template <bool FILT>
__device__ inline int64_t knn_filter_row(int64_t p, const uint32_t *__restrict__ fbits, const int *__restrict__ frows, int nlive, bool &allowed) {
    if constexpr (!FILT) { allowed = true; return p; }
    if (frows) {
        allowed = p < nlive;
        return allowed ? (int64_t)frows[p] : 0;                      // (row 0 exists; a padding position never dereferences it)
    }
    allowed = ((fbits[p >> 5] >> (p & 31)) & 1u) != 0;
    return p;
}
// the record of an id outside the base (lsq_rerank.hip): the bit above the key, the key of +inf, id field 0
__device__ inline uint64_t knn_outside_record(int idbits) {
    return (1ull << (32 + idbits)) | ((uint64_t)lsq_adc_key(__builtin_inff()) << idbits);
}

template <int MODE, typename TX, typename TQ, bool FILT = false>
__global__ __launch_bounds__(KNN_THREADS) void knn_scan_kernel(const TX *__restrict__ X, int ldb, const TQ *__restrict__ Q, int ldq,
                                                               const int *__restrict__ qsel, int q0, int nqb, int d, int stride, int total,
                                                               int per_block, const uint32_t *__restrict__ tau, unsigned *__restrict__ count,
                                                               int cap, uint64_t *__restrict__ out, int idbits,
                                                               const uint32_t *__restrict__ fbits, const int *__restrict__ frows, int nlive) {
    __shared__ __attribute__((aligned(16))) float qs[KNN_KD * KNN_QP];
    __shared__ __attribute__((aligned(16))) float xs[KNN_KD * KNN_RP];
    const int t = threadIdx.x, tile = blockIdx.x;
    const int first = blockIdx.y * per_block;
    const int last = first + per_block < total ? first + per_block : total;
    if (first >= last) return;
    // staging roles: element j of this thread is (query / row (t >> 4) + 16 j, dimension t & 15): 16 consecutive threads read one row's chunk
    const int kk = t & (KNN_KD - 1), sr = t >> 4;
    const TQ *qrow[KNN_QL];
#pragma unroll
    for (int j = 0; j < KNN_QL; ++j) {
        const int slot = tile * KNN_QT + sr + 16 * j;
        qrow[j] = slot < nqb ? Q + (int64_t)(qsel ? qsel[slot] : q0 + slot) * ldq : nullptr;
    }
    TQ qreg[KNN_QL];
    TX xreg[KNN_RL];
    auto fetch = [&](int r0, int k0) {                              // global -> registers: chunk k0 of queries and of rows r0 .. r0 + RT - 1
        const int k = k0 + kk;
#pragma unroll
        for (int j = 0; j < KNN_QL; ++j) qreg[j] = (qrow[j] && k < d) ? qrow[j][k] : (TQ)0;
#pragma unroll
        for (int j = 0; j < KNN_RL; ++j) {
            const int s = r0 + sr + 16 * j;
            if constexpr (FILT) {
                bool have = false;
                const int64_t row = s < last ? knn_filter_row<FILT>((int64_t)s * stride, fbits, frows, nlive, have) : 0;
                xreg[j] = (s < last && (have || !frows) && k < d) ? X[row * ldb + k] : (TX)0;
            } else {
                xreg[j] = (s < last && k < d) ? X[(int64_t)s * stride * ldb + k] : (TX)0;
            }
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
            for (int j = 0; j < KNN_QL; ++j) qs[kk * KNN_QP + sr + 16 * j] = (float)qreg[j];
#pragma unroll
            for (int j = 0; j < KNN_RL; ++j) xs[kk * KNN_RP + sr + 16 * j] = (float)xreg[j];
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
            bool allowed = true;
            const int64_t i = knn_filter_row<FILT>((int64_t)s * stride, fbits, frows, nlive, allowed);
            if (FILT && MODE == 0 && !allowed) continue;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int p = c >> 1;
                const float dv = (c & 1) ? acc[j][p].y : acc[j][p].x;
                const int slot = tile * KNN_QT + (c < 4 ? 4 * qg + c : 64 + 4 * qg + c - 4);
                if (slot >= nqb) continue;
                if (MODE == 0 && dv > tf[c]) continue;              // emit unless dist > tau (a NaN on either side emits)
                uint32_t key = lsq_adc_key(dv);
                uint64_t rec = ((uint64_t)key << idbits) | (uint64_t)(i + 1);      // 1-based in the record; the gather hands out 0-based ids
                if (FILT && !allowed) { key = 0xffffffffu; rec = knn_outside_record(idbits); }
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

// ---- the integer road ------------------------------------------------------------------------------------------------------------------------------
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Dword w (components 4 w .. 4 w + 3) of a row of d bytes, component e in byte e, zero from the d-th component on.  vec (lsq_xload.h's rule: the
// matrix pointer and its row pitch in bytes are multiples of 4): one dword load where all four components exist.  Everything else -- a matrix at any
// byte offset, an odd pitch, and the LAST, partial dword of any row -- travels as single bytes: nothing at or past the d-th byte of a row is loaded,
// so nothing outside [base, base + (n - 1) ldb + d) is, and there is no padding to mask.
__device__ inline uint32_t knn_ld_packed(const uint8_t *__restrict__ row, int w, int d, bool vec) {
    const int b0 = 4 * w, valid = d - b0;
    if (valid <= 0) return 0u;
    if (vec && valid >= 4) return lsq_ld4_packed(row + b0);
    uint32_t v = 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (e < valid) v |= (uint32_t)row[b0 + e] << (8 * e);
    return v;
}

// out[i] = SUM_s x_i[s]^2 (uint32: <= 258 * 255^2 < 2^24), 16 lanes per row, dot4 of each packed dword with itself
__global__ __launch_bounds__(KNN_THREADS) void knn_norms_u8_kernel(const uint8_t *__restrict__ X, int64_t ld, int n, int d, int vec,
                                                                   uint32_t *__restrict__ out) {
    const int kk = threadIdx.x & 15, nw = (d + 3) / 4;
    for (int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); i < n; i += (int64_t)gridDim.x * 16) {      // (a 16-lane group shares i: it leaves together)
        const uint8_t *row = X + i * ld;
        uint32_t acc = 0u;
        for (int w = kk; w < nw; w += 16) {
            const uint32_t v = knn_ld_packed(row, w, d, vec != 0);
            acc = __builtin_amdgcn_udot4(v, v, acc, false);
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 16);
        if (kk == 0) out[i] = acc;
    }
}

// knn_scan_kernel's tile, modes, records, grid and per_block rule on PACKED dwords: LDS holds [dword][row] with the same padded pitches, KNN_KD dwords
// (64 dimensions) staged per pass; per dword step a lane issues three ds_read_b128 and 32 v_dot4_u32_u8.  xn [n] / qn [queries]: the squared norms
// (knn_norms_u8_kernel).  D = xn + qn - 2 acc is exact and (float)D is the chain's result (d <= 258: the top of this file).
template <int MODE, bool FILT = false>
__global__ __launch_bounds__(KNN_THREADS) void knn_scan_u8_kernel(const uint8_t *__restrict__ X, int ldb, int vecx, const uint8_t *__restrict__ Q, int ldq,
                                                                  int vecq, const uint32_t *__restrict__ xn, const uint32_t *__restrict__ qn,
                                                                  const int *__restrict__ qsel, int q0, int nqb, int d, int stride, int total,
                                                                  int per_block, const uint32_t *__restrict__ tau, unsigned *__restrict__ count,
                                                                  int cap, uint64_t *__restrict__ out, int idbits,
                                                                  const uint32_t *__restrict__ fbits, const int *__restrict__ frows, int nlive) {
    __shared__ __attribute__((aligned(16))) uint32_t qs[KNN_KD * KNN_QP];
    __shared__ __attribute__((aligned(16))) uint32_t xs[KNN_KD * KNN_RP];
    const int t = threadIdx.x, tile = blockIdx.x;
    const int first = blockIdx.y * per_block;
    const int last = first + per_block < total ? first + per_block : total;
    if (first >= last) return;
    // staging roles: element j of this thread is (query / row (t >> 4) + 16 j, dword t & 15): 16 consecutive threads read 64 bytes of one row
    const int kk = t & (KNN_KD - 1), sr = t >> 4;
    const uint8_t *qrow[KNN_QL];
#pragma unroll
    for (int j = 0; j < KNN_QL; ++j) {
        const int slot = tile * KNN_QT + sr + 16 * j;
        qrow[j] = slot < nqb ? Q + (int64_t)(qsel ? qsel[slot] : q0 + slot) * ldq : nullptr;
    }
    uint32_t qreg[KNN_QL], xreg[KNN_RL];
    auto fetch = [&](int r0, int w0) {                              // global -> registers: dwords w0 .. w0 + KD - 1 of the queries and of rows r0 .. r0 + RT - 1
        const int w = w0 + kk;
#pragma unroll
        for (int j = 0; j < KNN_QL; ++j) qreg[j] = qrow[j] ? knn_ld_packed(qrow[j], w, d, vecq != 0) : 0u;      // slots >= nqb: zero
#pragma unroll
        for (int j = 0; j < KNN_RL; ++j) {
            const int s = r0 + sr + 16 * j;
            if constexpr (FILT) {
                bool have = false;
                const int64_t row = s < last ? knn_filter_row<FILT>((int64_t)s * stride, fbits, frows, nlive, have) : 0;
                xreg[j] = (s < last && (have || !frows)) ? knn_ld_packed(X + row * ldb, w, d, vecx != 0) : 0u;
            } else {
                xreg[j] = s < last ? knn_ld_packed(X + (int64_t)s * stride * ldb, w, d, vecx != 0) : 0u;              // rows >= last: zero
            }
        }
    };
    // compute roles: those of knn_scan_kernel
    const int qg = t & 15, rg = t >> 4;
    float tf[8];
    uint32_t nq8[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int slot = tile * KNN_QT + (c < 4 ? 4 * qg + c : 64 + 4 * qg + c - 4);
        tf[c] = (MODE == 0 && slot < nqb) ? lsq_adc_unkey(tau[slot]) : -__builtin_inff();
        nq8[c] = slot < nqb ? qn[qsel ? qsel[slot] : q0 + slot] : 0u;
    }
    const int nk = ((d + 3) / 4 + KNN_KD - 1) / KNN_KD;
    fetch(first, 0);
    for (int r0 = first; r0 < last; r0 += KNN_RT) {
        uint32_t acc[4][8];                                         // [row j][query c]: query 4 qg + c for c < 4, 64 + 4 qg + c - 4 above
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[j][c] = 0u;
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
                const u32x4 qa = *reinterpret_cast<const u32x4 *>(qs + s * KNN_QP + 4 * qg);
                const u32x4 qb = *reinterpret_cast<const u32x4 *>(qs + s * KNN_QP + 64 + 4 * qg);
                const u32x4 xv = *reinterpret_cast<const u32x4 *>(xs + s * KNN_RP + 4 * rg);
                const uint32_t qv[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
                const uint32_t xr[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int c = 0; c < 8; ++c) acc[j][c] = __builtin_amdgcn_udot4(xr[j], qv[c], acc[j][c], false);
            }
        }
        // emission: that of knn_scan_kernel, on dv = (float)(N_x + N_q - 2 <x, q>)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int s = r0 + 4 * rg + j;
            if (s >= last) continue;
            bool allowed = true;
            const int64_t i = knn_filter_row<FILT>((int64_t)s * stride, fbits, frows, nlive, allowed);
            if (FILT && MODE == 0 && !allowed) continue;
            const uint32_t nx = xn[i];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float dv = (float)(nx + nq8[c] - 2u * acc[j][c]);      // exact in uint32 (never negative), exact as a float (<= 2^24)
                const int slot = tile * KNN_QT + (c < 4 ? 4 * qg + c : 64 + 4 * qg + c - 4);
                if (slot >= nqb) continue;
                if (MODE == 0 && dv > tf[c]) continue;
                uint32_t key = lsq_adc_key(dv);
                uint64_t rec = ((uint64_t)key << idbits) | (uint64_t)(i + 1);
                if (FILT && !allowed) { key = 0xffffffffu; rec = knn_outside_record(idbits); }
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

// the three modes of one producer; K(MODE) names the instantiation
#define KNN_LAUNCH_FILT(K, F, ...)                                                                  \
    do {                                                                                            \
        if (mode == 0) hipLaunchKernelGGL((K(0, F)), grid, block, 0, s, __VA_ARGS__);                \
        else if (mode == 1) hipLaunchKernelGGL((K(1, F)), grid, block, 0, s, __VA_ARGS__);           \
        else hipLaunchKernelGGL((K(2, F)), grid, block, 0, s, __VA_ARGS__);                          \
    } while (0)
#define KNN_LAUNCH_MODES(K, ...)                                                                    \
    do {                                                                                            \
        if (in.filtered()) KNN_LAUNCH_FILT(K, true, __VA_ARGS__, in.filter_bits, in.filter_rows, in.filter_count);   \
        else KNN_LAUNCH_FILT(K, false, __VA_ARGS__, nullptr, nullptr, 0);                            \
    } while (0)
#define KNN_INT(M, F) knn_scan_u8_kernel<M, F>
#define KNN_FF(M, F) knn_scan_kernel<M, float, float, F>
#define KNN_BF(M, F) knn_scan_kernel<M, uint8_t, float, F>
#define KNN_FB(M, F) knn_scan_kernel<M, float, uint8_t, F>
#define KNN_BB(M, F) knn_scan_kernel<M, uint8_t, uint8_t, F>
// half rows (lsq_xload.h): 2-byte loads, widened (exact) at the staging store like the bytes -- f32 or uint8 queries, no road of their own
#define KNN_HF(M, F) knn_scan_kernel<M, lsq_f16, float, F>
#define KNN_HB(M, F) knn_scan_kernel<M, lsq_f16, uint8_t, F>
#define KNN_GF(M, F) knn_scan_kernel<M, lsq_bf16, float, F>
#define KNN_GB(M, F) knn_scan_kernel<M, lsq_bf16, uint8_t, F>

}  // namespace

// out[i] = |row i|^2 of an 8-bit matrix (rows ld bytes apart, d components read): the norms of the integer road
int lsq_knn_launch_norms_u8(hipStream_t s, const uint8_t *X, int64_t ld, int n, int d, uint32_t *out) {
    if (n <= 0) return LSQ_OK;
    const int vec = lsq_x_vec_ok(X) && (ld & 3) == 0;
    const int64_t blocks = ((int64_t)n + 15) / 16;
    hipLaunchKernelGGL(knn_norms_u8_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(KNN_THREADS), 0, s, X, ld, n, d, vec, out);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

// The scan of one batch for adc_search's "exact" input kind.  MODE 0: rows 0 .. n-1 against tau; MODE 1 / 2: rows s * stride, s < ns.  The producer is
// chosen by what `in` says its rows and queries are made of: the integer road when it carries norms, a widened instantiation otherwise.
int lsq_knn_launch_scan(hipStream_t s, int mode, const lsq_search_input &in, const int *qsel, int q0, int nqb, int stride, int ns, const uint32_t *tau,
                        unsigned *count, int cap, uint64_t *out, int idbits) {
    const int n = in.rows_walked(), d = in.d, ldb = in.bstride, ldq = in.qstride;      // compact road of a filter: the allowed rows
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
    const float *Xf = static_cast<const float *>(in.base), *Qf = static_cast<const float *>(in.Q);
    const uint8_t *Xb = static_cast<const uint8_t *>(in.base), *Qb = static_cast<const uint8_t *>(in.Q);
    if (in.xnorms) {                                                // (set by the caller for uint8 x uint8 with d <= 258 only)
        const int vecx = lsq_x_vec_ok(Xb) && (ldb & 3) == 0, vecq = lsq_x_vec_ok(Qb) && (ldq & 3) == 0;
        KNN_LAUNCH_MODES(KNN_INT, Xb, ldb, vecx, Qb, ldq, vecq, in.xnorms, in.qnorms, qsel, q0, nqb, d, st, total, per_block, tau, count, cap,
                         out, idbits);
    } else if (in.base_u8 == LSQ_BASE_F16 || in.base_u8 == LSQ_BASE_BF16) {
        const lsq_f16 *Xh = static_cast<const lsq_f16 *>(in.base);
        const lsq_bf16 *Xg = static_cast<const lsq_bf16 *>(in.base);
        if (in.base_u8 == LSQ_BASE_F16 && in.q_u8) KNN_LAUNCH_MODES(KNN_HB, Xh, ldb, Qb, ldq, qsel, q0, nqb, d, st, total, per_block, tau, count, cap, out, idbits);
        else if (in.base_u8 == LSQ_BASE_F16) KNN_LAUNCH_MODES(KNN_HF, Xh, ldb, Qf, ldq, qsel, q0, nqb, d, st, total, per_block, tau, count, cap, out, idbits);
        else if (in.q_u8) KNN_LAUNCH_MODES(KNN_GB, Xg, ldb, Qb, ldq, qsel, q0, nqb, d, st, total, per_block, tau, count, cap, out, idbits);
        else KNN_LAUNCH_MODES(KNN_GF, Xg, ldb, Qf, ldq, qsel, q0, nqb, d, st, total, per_block, tau, count, cap, out, idbits);
    } else if (in.base_u8 && in.q_u8) {
        KNN_LAUNCH_MODES(KNN_BB, Xb, ldb, Qb, ldq, qsel, q0, nqb, d, st, total, per_block, tau, count, cap, out, idbits);
    } else if (in.base_u8) {
        KNN_LAUNCH_MODES(KNN_BF, Xb, ldb, Qf, ldq, qsel, q0, nqb, d, st, total, per_block, tau, count, cap, out, idbits);
    } else if (in.q_u8) {
        KNN_LAUNCH_MODES(KNN_FB, Xf, ldb, Qb, ldq, qsel, q0, nqb, d, st, total, per_block, tau, count, cap, out, idbits);
    } else {
        KNN_LAUNCH_MODES(KNN_FF, Xf, ldb, Qf, ldq, qsel, q0, nqb, d, st, total, per_block, tau, count, cap, out, idbits);
    }
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}
