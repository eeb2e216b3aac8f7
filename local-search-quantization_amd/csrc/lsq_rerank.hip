// lsq_rerank.hip -- stage two of a two-stage search ON THE DEVICE (gfx950): the exact distances of every query to the rows of its own shortlist.
//
// Stage one is the ADC scan of src/linscan/Linscan.jl:46-73 (lsq_adc.hip).  Stage two has no counterpart in the reference: its users re-order a shortlist
// on the host.  For query q and candidate row x the distance is lsq_knn.hip's, bit for bit:
//
//   dist = ((0 + e_0 e_0) + e_1 e_1) + ... + e_{d-1} e_{d-1},   e_s = x[s] - q[s]     f32, s ascending, every op rounded (no FMA)
//
// This is a GATHER kernel, not a VALU kernel: nq L independent (query, row) pairs, 3 flops per component against 4 bytes (f32 rows) or 1 byte (uint8 rows,
// widened in registers by lsq_xload.h: exact, so the 8-bit instantiation returns the bits of the f32 one on the widened matrix).  What bounds it is the
// rate at which random rows of 4 d or d bytes arrive, so the work of a block is laid out around the loads:
//
//   block    256 threads = one query and a tile of 256 of its candidates.  The chain is sequential in s, so a lane owns ONE (query, candidate) pair from
//            its first component to its last: no distance is ever reduced across lanes.
//   staging  64 lanes of one load must not hit 64 rows 16 bytes at a time.  Eight consecutive lanes fetch one whole 128-byte line of a row (16 bytes
//            each), a wave-instruction eight lines, a thread eight rows per chunk of 128 bytes.  The pieces go through LDS transposed, [dword][row] with
//            the padded pitch of lsq_knn.hip's tiles, and the owner of a row walks them back with conflict-free 4-byte reads.  The next chunk's loads are in
//            flight while the current one is walked (lsq_knn.hip's pattern).  8-bit quads stay packed -- in the registers, in LDS -- until they are consumed.
//   query    one per block, read at block-uniform addresses: it lives in scalar registers, not in LDS and not in 64 copies.
//   padding  the last chunk is zero-filled past the row's d components and the query reads as 0 there: 0 - 0 = +0 adds +0, which leaves every partial sum
//            -- never -0 -- unchanged (the reason given at the top of lsq_knn.hip).  Nothing past the d-th component of a row is ever loaded.
//
// Alignment (the rule of lsq_xload.h, per 16-byte piece): one 16-byte load when the row pitch in bytes and the base are multiples of 16; dword loads
// when they are multiples of 4 (every f32 matrix; a uint8 matrix with ldb % 4 == 0 on a 4-byte-aligned base); byte loads otherwise.  Half rows (lsq_f16 /
// lsq_bf16, lsq_xload.h): 2 components per dword, 64 per line; dword loads when pitch and base are multiples of 4, the last, partial dword of an
// odd-d row as one 2-byte load; 2-byte loads otherwise (an odd ldb, a base at an odd element).  A half base is 2-byte aligned (checked where it is taken).
//
// The kernel is a distance PRODUCER for the scans' selection (lsq_adc.hip): it writes records (lsq_adc_key(dist) << idbits | id + 1) to
// out[slot * L + s], the layout of the scans' MODE 1, and the exhaustive road's segments / segmented sort / gather serve it unchanged.  A candidate id
// outside [id_base, id_base + n) is never dereferenced: its record carries the key of +inf, the id field 0 (which no row uses) and ONE bit above the
// key, so that it sorts after every number and after NaN, and the gather -- which drops that bit -- hands out (+inf, id_base - 1).
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "lsq_internal.h"
#include "lsq_xload.h"

#pragma clang fp contract(off)

namespace {

constexpr int RR_THREADS = 256;              // = candidates per block: lane t owns candidate t of the tile
constexpr int RR_LINE = 128;                 // bytes of a row per chunk: one line
constexpr int RR_DW = RR_LINE / 4;           // dwords per chunk and row (32)
constexpr int RR_PIECES = RR_LINE / 16;      // 16-byte pieces per line = lanes that share a row (8)
constexpr int RR_ROWS = RR_THREADS / RR_PIECES;      // rows per load instruction of the block (32)
constexpr int RR_RL = RR_THREADS / RR_ROWS;  // rows staged per thread and chunk (8)
constexpr int RR_RP = RR_THREADS + 1;        // padded LDS pitch (dwords): a half-wave's transposed store (8 pieces x 4 rows, dwords 4 RP apart) falls on 32 distinct banks

struct u32x4 { uint32_t v[4]; };

// bytes [0, 16) of p as four dwords, `valid` (1 .. 16, a multiple of sizeof(T)) of them read, the rest zero.  ALIGN: what p is known to be a multiple of
template <typename T, int ALIGN>
__device__ inline u32x4 rr_load16(const uint8_t *p, int valid) {
    u32x4 w = {{0u, 0u, 0u, 0u}};
    if (ALIGN == 16 && valid == 16) {
        const uint4 q = *reinterpret_cast<const uint4 *>(p);
        w.v[0] = q.x; w.v[1] = q.y; w.v[2] = q.z; w.v[3] = q.w;
    } else if (ALIGN >= 4 && (sizeof(T) == 4 || valid == 16)) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * j < valid) w.v[j] = reinterpret_cast<const uint32_t *>(p)[j];
    } else if (sizeof(T) == 2) {                                    // half rows below the 16-byte road, and the tail of a half row
        if (ALIGN >= 4) {                                           // whole dwords; the last, partial dword of an odd-d row as one 2-byte load
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (4 * j + 4 <= valid) w.v[j] = reinterpret_cast<const uint32_t *>(p)[j];
                else if (4 * j + 2 <= valid) w.v[j] = reinterpret_cast<const uint16_t *>(p)[2 * j];
            }
        } else {                                                    // an odd pitch or a base at an odd element: 2-byte loads
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (2 * j < valid) w.v[j >> 1] |= (uint32_t)reinterpret_cast<const uint16_t *>(p)[j] << (16 * (j & 1));
        }
    } else {                                                        // 8-bit rows at any byte offset, and the tail of an 8-bit row
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < valid) w.v[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
    }
    return w;
}

// acc after the components of dword w (component k0 onwards of the row), against the block's query: q[k] read at uniform addresses, 0 past d
template <typename T, bool TAIL>
__device__ inline float rr_consume(float acc, uint32_t w, const float *__restrict__ q, int k0, int d) {
    if (sizeof(T) == 4) {
        const float e = __uint_as_float(w) - ((!TAIL || k0 < d) ? q[k0] : 0.0f);      // x - q, rounded; the square, rounded; then the add (no FMA)
        return acc + e * e;
    }
    if constexpr (sizeof(T) == 2) {                                 // two halves of the dword, widened here (exact): the same chain
        const lsq_f32x2 h = lsq_widen2<T>(w);
        const float hv[2] = {h.x, h.y};
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float e = hv[c] - ((!TAIL || k0 + c < d) ? q[k0 + c] : 0.0f);
            acc = acc + e * e;
        }
        return acc;
    }
    const lsq_f32x4 x = lsq_widen4(w);
    const float xv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float e = xv[c] - ((!TAIL || k0 + c < d) ? q[k0 + c] : 0.0f);
        acc = acc + e * e;
    }
    return acc;
}

// One block: query slot blockIdx.x / tiles of the batch (query q0 + slot), candidates tile * 256 .. of its list.  cand [nq][L] (ids in the caller's
// id_base), out [nqb][L] records, invalid: += candidates outside the base.
template <typename T, int ALIGN>
__global__ __launch_bounds__(RR_THREADS) void rerank_kernel(const T *__restrict__ X, int64_t ldb, int64_t n, const float *__restrict__ Q, int64_t ldq,
                                                            const int *__restrict__ cand, int q0, int L, int tiles, int d, int id_base,
                                                            uint64_t *__restrict__ out, int idbits, unsigned long long *__restrict__ invalid) {
    __shared__ uint32_t xs[RR_DW * RR_RP];
    constexpr int CPD = 4 / (int)sizeof(T);                         // components per dword
    constexpr int KC = RR_DW * CPD;                                 // components per chunk
    const int t = threadIdx.x;
    const int slot = blockIdx.x / tiles, tile = blockIdx.x - slot * tiles;
    const int64_t qid = (int64_t)q0 + slot;
    const float *__restrict__ q = Q + qid * ldq;                    // block-uniform
    const int *__restrict__ cl = cand + qid * L + (int64_t)tile * RR_THREADS;
    const int left = L - tile * RR_THREADS;                         // candidates of this tile (>= 1), RR_THREADS of them at most
    // staging roles: piece kp of row sr + 32 j, j < 8: eight consecutive lanes read one line
    const int kp = t & (RR_PIECES - 1), sr = t >> 3;
    const uint8_t *rowp[RR_RL];
#pragma unroll
    for (int j = 0; j < RR_RL; ++j) {
        const int r = sr + RR_ROWS * j;
        rowp[j] = nullptr;
        if (r < left) {
            const int64_t i = (int64_t)cl[r] - id_base;
            if (i >= 0 && i < n) rowp[j] = reinterpret_cast<const uint8_t *>(X + i * ldb);      // an id outside the base is never dereferenced
        }
    }
    const int rowbytes = d * (int)sizeof(T);
    u32x4 reg[RR_RL];
    auto fetch = [&](int c) {                                       // global -> registers: chunk c (bytes 128 c ..) of the thread's eight rows
        const int off = c * RR_LINE + 16 * kp;
        if ((c + 1) * RR_LINE <= rowbytes) {                        // (uniform) a whole line of every row: one load per piece
#pragma unroll
            for (int j = 0; j < RR_RL; ++j) {
                if (rowp[j]) reg[j] = rr_load16<T, ALIGN>(rowp[j] + off, 16);
                else reg[j] = u32x4{{0u, 0u, 0u, 0u}};
            }
        } else {                                                    // the row's last, partial line: nothing past its d-th component is read
            const int valid = rowbytes - off < 16 ? rowbytes - off : 16;
#pragma unroll
            for (int j = 0; j < RR_RL; ++j) {
                if (rowp[j] && valid > 0) reg[j] = rr_load16<T, ALIGN>(rowp[j] + off, valid);
                else reg[j] = u32x4{{0u, 0u, 0u, 0u}};
            }
        }
    };
    const int nk = (rowbytes + RR_LINE - 1) / RR_LINE;
    float acc = 0.0f;
    fetch(0);
    for (int c = 0; c < nk; ++c) {
        __syncthreads();                                            // the previous chunk has been walked
#pragma unroll
        for (int j = 0; j < RR_RL; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) xs[(4 * kp + e) * RR_RP + sr + RR_ROWS * j] = reg[j].v[e];
        __syncthreads();
        if (c + 1 < nk) fetch(c + 1);
        const int k0 = c * KC;
        if (k0 + KC <= d) {
#pragma unroll
            for (int s = 0; s < RR_DW; ++s) acc = rr_consume<T, false>(acc, xs[s * RR_RP + t], q, k0 + s * CPD, d);
        } else {
            const int nd = (d - k0 + CPD - 1) / CPD;                // uniform
            for (int s = 0; s < nd; ++s) acc = rr_consume<T, true>(acc, xs[s * RR_RP + t], q, k0 + s * CPD, d);
        }
    }
    bool bad = false;
    if (t < left) {
        const int64_t i = (int64_t)cl[t] - id_base;
        bad = i < 0 || i >= n;
        const uint64_t rec = bad ? ((1ull << (32 + idbits)) | ((uint64_t)lsq_adc_key(__builtin_inff()) << idbits))
                                 : (((uint64_t)lsq_adc_key(acc) << idbits) | (uint64_t)(i + 1));
        out[(int64_t)slot * L + (int64_t)tile * RR_THREADS + t] = rec;
    }
    const unsigned long long nb = __popcll(__ballot(bad));
    if ((t & 63) == 0 && nb) atomicAdd(invalid, nb);
}

template <typename T>
int launch(hipStream_t s, const T *X, int64_t ldb, int64_t n, const float *Q, int64_t ldq, const int *cand, int q0, int nqb, int L, int d, int id_base,
           uint64_t *out, int idbits, unsigned long long *invalid) {
    const int tiles = (L + RR_THREADS - 1) / RR_THREADS;
    const dim3 grid((unsigned)((int64_t)nqb * tiles)), block(RR_THREADS);
    const uintptr_t a = (uintptr_t)X | (uintptr_t)(ldb * (int64_t)sizeof(T));
#define RR_LAUNCH(AL) \
    hipLaunchKernelGGL((rerank_kernel<T, AL>), grid, block, 0, s, X, ldb, n, Q, ldq, cand, q0, L, tiles, d, id_base, out, idbits, invalid)
    if ((a & 15) == 0) RR_LAUNCH(16);
    else if ((a & 3) == 0) RR_LAUNCH(4);
    else if constexpr (sizeof(T) == 1) RR_LAUNCH(1);
    else if constexpr (sizeof(T) == 2) {
        if ((a & 1) != 0) { lsq_set_error("re-rank: the half-precision base is not 2-byte aligned"); return LSQ_EINVAL; }
        RR_LAUNCH(2);
    }
    else { lsq_set_error("re-rank: the f32 base is not 4-byte aligned"); return LSQ_EINVAL; }
#undef RR_LAUNCH
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

}  // namespace

int lsq_rerank_launch(hipStream_t s, const void *base, int base_u8, int64_t ldb, int64_t n, const float *Q, int64_t ldq, const int *cand, int q0, int nqb,
                      int L, int d, int id_base, uint64_t *out, int idbits, unsigned long long *invalid) {
    if (nqb <= 0 || L <= 0) return LSQ_OK;
    const int fmt = lsq_base_format(base_u8);
    if (fmt == LSQ_BASE_F16) return launch(s, static_cast<const lsq_f16 *>(base), ldb, n, Q, ldq, cand, q0, nqb, L, d, id_base, out, idbits, invalid);
    if (fmt == LSQ_BASE_BF16) return launch(s, static_cast<const lsq_bf16 *>(base), ldb, n, Q, ldq, cand, q0, nqb, L, d, id_base, out, idbits, invalid);
    if (fmt) return launch(s, static_cast<const uint8_t *>(base), ldb, n, Q, ldq, cand, q0, nqb, L, d, id_base, out, idbits, invalid);
    return launch(s, static_cast<const float *>(base), ldb, n, Q, ldq, cand, q0, nqb, L, d, id_base, out, idbits, invalid);
}

// ---- the host drop-in: the checker of the kernel above and the engine-less road -----------------------------------------------------------------
namespace {

inline uint32_t host_key(float v) {
    if (v != v) return 0xffffffffu;
    uint32_t b;
    memcpy(&b, &v, 4);
    return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}

template <typename T>
void rerank_queries(float *dists, int *ids, const T *base, const float *queries, const int *cand, int64_t n, int q0, int q1, int d, int64_t ldb,
                    int64_t ldq, int L, int nn, int id_base) {
    struct Rec { uint64_t hi; uint32_t id; float dist; };       // hi = (invalid, key): the order is (hi, id)
    std::vector<Rec> recs((size_t)L);
    for (int qi = q0; qi < q1; ++qi) {
        const float *q = queries + (int64_t)qi * ldq;
        for (int s = 0; s < L; ++s) {
            const int64_t i = (int64_t)cand[(int64_t)qi * L + s] - id_base;
            if (i < 0 || i >= n) { recs[(size_t)s] = Rec{1ull << 32, 0u, __builtin_inff()}; continue; }
            const T *x = base + i * ldb;
            float acc = 0.0f;
            for (int k = 0; k < d; ++k) {
                const float e = (float)x[k] - q[k];
                acc += e * e;                                           // product rounded, then the add (-ffp-contract=off)
            }
            recs[(size_t)s] = Rec{(uint64_t)host_key(acc), (uint32_t)(i + 1), acc};
        }
        const auto less = [](const Rec &a, const Rec &b) { return a.hi != b.hi ? a.hi < b.hi : a.id < b.id; };
        std::partial_sort(recs.begin(), recs.begin() + nn, recs.end(), less);
        for (int j = 0; j < nn; ++j) {
            const Rec &r = recs[(size_t)j];
            float dv = r.dist;
            if (dv != dv) { const uint32_t nanbits = 0x7fc00000u; memcpy(&dv, &nanbits, 4); }      // one NaN, whatever the payload
            dists[(int64_t)qi * nn + j] = dv;
            ids[(int64_t)qi * nn + j] = (int)r.id - 1 + id_base;      // id field 0 (outside the base) -> id_base - 1
        }
    }
}

}  // namespace

// Argument checks shared by the host drop-in and the index (lsq_api.hip): 0 or LSQ_EINVAL with the message set.
int lsq_rerank_check(const char *fn, const void *dists, const void *ids, const void *base, const void *queries, const void *cand, int64_t n, int nq, int d,
                     int64_t ldb, int64_t ldq, int L, int nn, int id_base) {
    if (d < 1 || ldb < d || ldq < d) {
        lsq_set_error("%s: needs d >= 1, ldb >= d, ldq >= d (got d=%d ldb=%lld ldq=%lld)", fn, d, (long long)ldb, (long long)ldq);
        return LSQ_EINVAL;
    }
    if (n < 1 || n > (int64_t)INT32_MAX - 1) { lsq_set_error("%s: needs 1 <= n <= 2^31 - 2 (got %lld)", fn, (long long)n); return LSQ_EINVAL; }
    if (nq < 0) { lsq_set_error("%s: needs nq >= 0 (got %d)", fn, nq); return LSQ_EINVAL; }
    if (nn < 1 || nn > L) { lsq_set_error("%s: needs 1 <= nn <= L (got nn=%d L=%d)", fn, nn, L); return LSQ_EINVAL; }
    if (id_base != 0 && id_base != 1) { lsq_set_error("%s: id_base must be 0 or 1 (got %d)", fn, id_base); return LSQ_EINVAL; }
    if (!dists || !ids || !base || !queries || !cand) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    return LSQ_OK;
}

extern "C" int lsq_rerank_cpu(float *dists, int *ids, const void *base, int base_u8, const float *queries, const int *cand, int n, int nq, int d,
                              int ldb, int ldq, int L, int nn, int id_base, int nthreads) {
    LSQ_TRY(lsq_rerank_check("lsq_rerank_cpu", dists, ids, base, queries, cand, n, nq, d, ldb, ldq, L, nn, id_base));
    const int fmt = lsq_base_format(base_u8);
    if (const char *why = lsq_base_align_refusal(lsq_base_is_half(fmt) ? fmt : 1, base)) { lsq_set_error("lsq_rerank_cpu: %s", why); return LSQ_EINVAL; }
    if (nq == 0) return LSQ_OK;
    int nt = nthreads > 0 ? nthreads : (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if (nt > nq) nt = nq;
    std::vector<std::thread> pool;
    pool.reserve((size_t)nt);
    for (int t = 0; t < nt; ++t) {
        const int q0 = (int)((int64_t)nq * t / nt), q1 = (int)((int64_t)nq * (t + 1) / nt);
        if (fmt == LSQ_BASE_F16)
            pool.emplace_back(rerank_queries<lsq_f16>, dists, ids, static_cast<const lsq_f16 *>(base), queries, cand, n, q0, q1, d, (int64_t)ldb,
                              (int64_t)ldq, L, nn, id_base);
        else if (fmt == LSQ_BASE_BF16)
            pool.emplace_back(rerank_queries<lsq_bf16>, dists, ids, static_cast<const lsq_bf16 *>(base), queries, cand, n, q0, q1, d, (int64_t)ldb,
                              (int64_t)ldq, L, nn, id_base);
        else if (fmt)
            pool.emplace_back(rerank_queries<uint8_t>, dists, ids, static_cast<const uint8_t *>(base), queries, cand, n, q0, q1, d, (int64_t)ldb,
                              (int64_t)ldq, L, nn, id_base);
        else
            pool.emplace_back(rerank_queries<float>, dists, ids, static_cast<const float *>(base), queries, cand, n, q0, q1, d, (int64_t)ldb,
                              (int64_t)ldq, L, nn, id_base);
    }
    for (auto &th : pool) th.join();
    return LSQ_OK;
}
