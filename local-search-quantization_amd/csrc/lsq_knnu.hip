// lsq_knnu.hip -- exact k-NN of 8-bit sets ON THE i8 MATRIX CORES (gfx950; option "knn_u8_mfma").
//
// The integer road of lsq_knn.hip (uint8 rows x uint8 queries, d <= 258) computes D = N_x + N_q - 2 <x, q> by v_dot4_u32_u8: exact, but eight VALU
// instructions per dimension.  v_mfma_i32_32x32x32_i8 computes the same inner product exactly in i32, so MODE 0 of the thresholded road -- "append the
// record of every pair with dist <= tau" -- is decided and finished by the matrix-core tile itself: no error window, no pending list, no recheck.
//
// The signed trick.  The i8 MFMA multiplies SIGNED bytes.  Squared distance is translation-invariant: with x' = x - 128, q' = q - 128 (byte XOR 0x80, read
// as int8)   D = N'_x + N'_q - 2 <x', q'>,  N' the squared norm of the shifted vector.  |<x', q'>| <= 258 * 2^14, N' <= 258 * 2^14, D <= 258 * 255^2 < 2^24:
// everything stays in i32 and (float)D is the contract's distance (the proof at the top of lsq_knn.hip).  Padding must be zero IN THE SIGNED DOMAIN: the
// XOR is applied to real bytes alone (knnu_flip); bytes at or past d, rows past the block's range and query slots past the batch are staged as 0x00.
//
//   norms   knnu_norms_kernel   N' = N - 256 S + 16384 d,  N = udot4(v, v), S = udot4(v, 0x01010101) over the packed dwords of a row (i32)
//   tile    knnu_scan_kernel    256 threads = 2 x 2 waves, block tile 128 rows x 128 queries, each wave 64 x 64 = 2 x 2 accumulators of 32 x 32 i32.
//
// M carries the ROWS and N the QUERIES: a lane's 64 accumulator values belong to two queries (column lane & 31 of either N tile), whose folded threshold
// and N'_q it keeps in registers, and to 32 rows whose N'_x it reads from LDS.
//
// LDS.  A panel is [row][64 bytes] at a pitch of 80 bytes (20 dwords: sixteen consecutive lanes' 16-byte reads fall on distinct bank quads, as in
// lsq_knnm.hip).  The QUERIES of the block are staged ONCE, every chunk of them (at most 5 chunks x 128 x 80 B = 50 KiB at d = 258), and stay; only the
// ROWS stream, one 64-dimension chunk at a time through two panels of 10 KiB, the next chunk's global loads in flight under the MFMAs of the current one,
// one barrier per chunk.  71 KiB in all: two blocks per CU.  At d = 128 a tile step is 16 MFMAs per wave -- staging the queries again for every step
// would double the staging work of the kernel's shortest loop.
//
// The operand rule this kernel relies on: one A or B operand of 32x32x32_i8 is 16 bytes per lane; lane l's byte j is element (l & 31, kappa(l >> 5, j)) of
// its matrix, with the SAME map kappa onto the K step's 32 indices for A and for B.  An integer sum has no order, so which 16 of a K step's 32 dimensions
// a half-wave holds is immaterial as long as both operands are fetched by one rule: half-wave h reads bytes 16 h .. 16 h + 15 of the step's 32, of its row
// (A) and of its query (B), one ds_read_b128 each.  A 64-dimension chunk is two K steps.
//
// Staging follows knn_scan_u8_kernel: 16 consecutive threads read 64 consecutive bytes of one row through knn_ld_packed (lsq_xload.h) -- one dword load
// where the matrix is 4-byte aligned with a pitch that is a multiple of 4, single bytes otherwise and for a row's last partial dword; nothing at or past
// a row's d-th byte is loaded.
//
// Epilogue: per accumulator value E = N'_x - 2 acc and the test E <= c_q, c_q = floor(tau_q) - N'_q folded once per query (knnu_floor_tau: it agrees
// with !((float)D > tau) for NaN, +-inf and negative tau).  A lane first marks its passing values in one word per query, reserves that many places of
// the query's list by ONE atomicAdd, and then writes knn_scan_u8_kernel's record (lsq_adc_key((float)D) << idbits | i + 1) into the places below cap.
// count[slot] ends as the number of passing pairs, as on the dot4 road; a list that does not overflow holds the same set of records, one that does is
// refused by the selection on either road.
#include "lsq_internal.h"
#include "lsq_xload.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int KU_THREADS = 256;
constexpr int KU_T = 128;                    // rows per block step = queries per block
constexpr int KU_LD = 20;                    // LDS row pitch (dwords): 64 bytes of a chunk + 16, 16-byte aligned rows, LD / 4 odd
constexpr int KU_MAXK = 5;                   // 64-dimension chunks at d = 258
constexpr int KU_SL = KU_T * 16 / KU_THREADS;      // staged dwords per thread, chunk and operand (8)
constexpr int KU_PAST = 1 << 30;             // N'_x of a row past the block's range: above every c_q, and 2 acc = 0 there

// the bytes of dword w of a row of d bytes that exist: 0x80 in each of them (x ^ 0x80 = x - 128 as int8), 0x00 in the padding
__device__ inline uint32_t knnu_flip(int d, int w) {
    const int valid = d - 4 * w;
    return valid >= 4 ? 0x80808080u : valid <= 0 ? 0u : 0x80808080u >> (8 * (4 - valid));
}

// the largest integer D with !((float)D > tau), for 0 <= D < 2^24: 2^24 when every D passes (NaN, +inf, tau >= 2^24), -1 when none does (tau < 0 -- not
// -0.0, which D = 0 passes), floor(tau) otherwise
__device__ inline int knnu_floor_tau(float tau) {
    if (!(tau < 16777216.0f)) return 1 << 24;
    if (tau < 0.0f) return -1;
    return (int)tau;
}

// out[i] = SUM_s (x_i[s] - 128)^2 = N - 256 S + 16384 d (i32: <= 258 * 2^14), 16 lanes per row as in knn_norms_u8_kernel
__global__ __launch_bounds__(KU_THREADS) void knnu_norms_kernel(const uint8_t *__restrict__ X, int64_t ld, int n, int d, int vec, int32_t *__restrict__ out) {
    const int kk = threadIdx.x & 15, nw = (d + 3) / 4;
    for (int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); i < n; i += (int64_t)gridDim.x * 16) {      // (a 16-lane group shares i: it leaves together)
        const uint8_t *row = X + i * ld;
        uint32_t nn = 0u, ss = 0u;
        for (int w = kk; w < nw; w += 16) {
            const uint32_t v = knn_ld_packed(row, w, d, vec != 0);
            nn = __builtin_amdgcn_udot4(v, v, nn, false);
            ss = __builtin_amdgcn_udot4(v, 0x01010101u, ss, false);
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {
            nn += __shfl_xor(nn, off, 16);
            ss += __shfl_xor(ss, off, 16);
        }
        if (kk == 0) out[i] = (int32_t)nn - 256 * (int32_t)ss + 16384 * d;
    }
}

__global__ __launch_bounds__(KU_THREADS, 2) void knnu_scan_kernel(const uint8_t *__restrict__ X, int64_t ldb, int vecx, const uint8_t *__restrict__ Q,
                                                                  int64_t ldq, int vecq, const int32_t *__restrict__ xn, const int32_t *__restrict__ qn,
                                                                  int q0, int nqb, int d, int n, int per_block, const uint32_t *__restrict__ tau,
                                                                  unsigned *__restrict__ count, int cap, uint64_t *__restrict__ out, int idbits) {
    __shared__ __attribute__((aligned(16))) uint32_t qs[KU_MAXK][KU_T * KU_LD];
    __shared__ __attribute__((aligned(16))) uint32_t xs[2][KU_T * KU_LD];
    __shared__ int32_t nxs[2][KU_T];
    const int t = threadIdx.x, tile = blockIdx.x;
    const int64_t first = (int64_t)blockIdx.y * per_block;
    const int64_t last = first + per_block < n ? first + per_block : (int64_t)n;
    if (first >= last) return;
    // staging roles: dword j of this thread is (row / query (t >> 4) + 16 j, dword t & 15 of the chunk): 16 consecutive threads read 64 bytes of one row
    const int kk = t & 15, sr = t >> 4;
    const int nk = (d + 63) / 64;
    // the block's queries, every chunk, once (visible after the first barrier below)
    for (int kc = 0; kc < nk; ++kc) {
        const int w = 16 * kc + kk;
        const uint32_t flip = knnu_flip(d, w);
#pragma unroll
        for (int j = 0; j < KU_SL; ++j) {
            const int slot = tile * KU_T + sr + 16 * j;
            qs[kc][(sr + 16 * j) * KU_LD + kk] = slot < nqb ? knn_ld_packed(Q + (int64_t)(q0 + slot) * ldq, w, d, vecq != 0) ^ flip : 0u;
        }
    }
    uint32_t xreg[KU_SL];
    auto fetch = [&](int64_t r0, int kc) {                          // global -> registers: chunk kc of rows r0 .. r0 + 127, shifted; rows >= last: zero
        const int w = 16 * kc + kk;
        const uint32_t flip = knnu_flip(d, w);
#pragma unroll
        for (int j = 0; j < KU_SL; ++j) {
            const int64_t row = r0 + sr + 16 * j;
            xreg[j] = row < last ? knn_ld_packed(X + row * ldb, w, d, vecx != 0) ^ flip : 0u;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int j = 0; j < KU_SL; ++j) xs[buf][(sr + 16 * j) * KU_LD + kk] = xreg[j];
    };
    // compute roles
    const int lane = t & 63, wave = t >> 6;
    const int wy = wave >> 1, wx = wave & 1, l31 = lane & 31, lhi = lane >> 5;
    // the lane's two queries: column l31 of N tile tj.  c_q = floor(tau) - N'_q; a slot past the batch never passes (E >= -2^23 > INT32_MIN)
    int slot2[2], cq[2], nq2[2];
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
        slot2[tj] = tile * KU_T + wx * 64 + tj * 32 + l31;
        const bool live = slot2[tj] < nqb;
        nq2[tj] = live ? qn[q0 + slot2[tj]] : 0;
        cq[tj] = live ? knnu_floor_tau(lsq_adc_unkey(tau[slot2[tj]])) - nq2[tj] : INT32_MIN;
    }
    fetch(first, 0);
    stage(0);
    int cur = 0, par = 0;
    for (int64_t r0 = first; r0 < last; r0 += KU_T, par ^= 1) {
        // N'_x of this step's rows: read after at least one barrier of the chunk loop, overwritten two steps later (after the next step's barriers)
        if (t < KU_T) nxs[par][t] = r0 + t < last ? xn[r0 + t] : KU_PAST;
        i32x16 acc[2][2];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[ti][tj][r] = 0;
        __syncthreads();                                            // the staged chunk (and nxs, and at first the queries) is visible
        for (int kc = 0; kc < nk; ++kc) {
            const bool more_k = kc + 1 < nk, more = more_k || r0 + KU_T < last;
            if (more_k) fetch(r0, kc + 1);
            else if (more) fetch(r0 + KU_T, 0);
            const i32x4 *ap = reinterpret_cast<const i32x4 *>(xs[cur] + (wy * 64 + l31) * KU_LD + 4 * lhi);
            const i32x4 *bp = reinterpret_cast<const i32x4 *>(qs[kc] + (wx * 64 + l31) * KU_LD + 4 * lhi);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {                        // K step ks: bytes 32 ks + 16 lhi .. + 15 of the chunk, rows and queries alike
                const i32x4 a0 = ap[2 * ks], a1 = ap[32 * KU_LD / 4 + 2 * ks];
                const i32x4 b0 = bp[2 * ks], b1 = bp[32 * KU_LD / 4 + 2 * ks];
                acc[0][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, acc[1][1], 0, 0, 0);
            }
            if (more) stage(cur ^ 1);                               // the other panel was last read one chunk ago (barrier below)
            __syncthreads();
            cur ^= 1;
        }
        // epilogue: accumulator (ti, tj)[r] is row r0 + wy 64 + ti 32 + (r & 3) + 8 (r >> 2) + 4 lhi, query slot2[tj]
        // pass one: E = N'_x - 2 acc in place of the accumulator, bit 16 ti + r of the query's word for a pair that passes
        const int32_t *nxl = nxs[par] + wy * 64 + 4 * lhi;
        uint32_t keep[2] = {0u, 0u};
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int nxr = nxl[ti * 32 + (r & 3) + 8 * (r >> 2)];
#pragma unroll
                for (int tj = 0; tj < 2; ++tj) {
                    const int e = nxr - 2 * acc[ti][tj][r];
                    acc[ti][tj][r] = e;
                    keep[tj] |= e <= cq[tj] ? 1u << (16 * ti + r) : 0u;
                }
            }
        }
        // pass two: one reservation per lane and query, then the records
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
            if (!keep[tj]) continue;
            unsigned at = atomicAdd(&count[slot2[tj]], (unsigned)__builtin_popcount(keep[tj]));
            uint64_t *list = out + (int64_t)slot2[tj] * cap;
#pragma unroll
            for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (!((keep[tj] >> (16 * ti + r)) & 1u)) continue;
                    const int64_t i = r0 + wy * 64 + ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                    const float dv = (float)(acc[ti][tj][r] + nq2[tj]);      // D: exact in i32, exact as a float (< 2^24)
                    if (at < (unsigned)cap) list[at] = ((uint64_t)lsq_adc_key(dv) << idbits) | (uint64_t)(i + 1);
                    ++at;
                }
            }
        }
    }
}

}  // namespace

// out[i] = |row i - 128|^2 of an 8-bit matrix (rows ld bytes apart, d components read): the shifted norms of the matrix-core road
int lsq_knnu_launch_norms(hipStream_t s, const uint8_t *X, int64_t ld, int n, int d, int32_t *out) {
    if (n <= 0) return LSQ_OK;
    const int vec = lsq_x_vec_ok(X) && (ld & 3) == 0;
    const int64_t blocks = ((int64_t)n + 15) / 16;
    hipLaunchKernelGGL(knnu_norms_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(KU_THREADS), 0, s, X, ld, n, d, vec, out);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

// MODE 0 of one batch, unfiltered, queries q0 .. q0 + nqb - 1: the records of every pair with dist <= tau into the candidate lists (count zeroed by the
// caller, as for the dot4 scan).  in carries the shifted norms (xnorms_s / qnorms_s) and d <= 258.  No allocation and no wait
int lsq_knnu_launch(hipStream_t s, const lsq_search_input &in, int q0, int nqb, const uint32_t *tau, unsigned *count, int cap, uint64_t *out, int idbits) {
    const int n = in.n, d = in.d;
    if (nqb <= 0 || n <= 0) return LSQ_OK;
    if (d < 1 || d > 64 * KU_MAXK || !in.xnorms_s || !in.qnorms_s) { lsq_set_error("lsq_knnu_launch: needs shifted norms and 1 <= d <= %d", 64 * KU_MAXK); return LSQ_EINVAL; }
    const uint8_t *X = static_cast<const uint8_t *>(in.base), *Q = static_cast<const uint8_t *>(in.Q);
    const int tiles = (nqb + KU_T - 1) / KU_T;
    // lsq_knn_launch_scan's grid rule: ~2048 blocks, ranges of at least 8 row steps, per_block in multiples of the row step
    int ranges = (2048 + tiles - 1) / tiles;
    const int max_ranges = (int)(((int64_t)n + 8 * KU_T - 1) / (8 * KU_T));
    if (ranges > max_ranges) ranges = max_ranges;
    if (ranges < 1) ranges = 1;
    if (ranges > 65535) ranges = 65535;
    int64_t per_block = ((int64_t)n + ranges - 1) / ranges;
    per_block = (per_block + KU_T - 1) / KU_T * KU_T;
    ranges = (int)(((int64_t)n + per_block - 1) / per_block);
    const int vecx = lsq_x_vec_ok(X) && (in.bstride & 3) == 0, vecq = lsq_x_vec_ok(Q) && (in.qstride & 3) == 0;
    hipLaunchKernelGGL(knnu_scan_kernel, dim3((unsigned)tiles, (unsigned)ranges), dim3(KU_THREADS), 0, s, X, (int64_t)in.bstride, vecx, Q,
                       (int64_t)in.qstride, vecq, in.xnorms_s, in.qnorms_s, q0, nqb, d, n, (int)per_block, tau, count, cap, out, idbits);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}
