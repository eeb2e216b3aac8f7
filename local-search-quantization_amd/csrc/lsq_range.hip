// lsq_range.hip -- range search on a resident index ON THE DEVICE (gfx950): every candidate row within a radius of the query, a result of variable length.
//
// The reference has no counterpart; the arithmetic is the scans' own, so that the result of a query is a prefix of the ranking they return:
//
//   table[e]  = adc_lut_kernel's, from q_scan                                                                             (lsq_adc.hip, unchanged)
//   dist(i)   = (((0 + table[0 h + b_i0]) + table[1 h + b_i1]) + ...) + dbnorms[i]   [ + coarse(q, l) with LSQ_IVF_ADD_COARSE ]
//   result    = every (dist, original id + 1) over the candidate rows with dist <= r_q (IEEE: a NaN on either side is out), in lexicographic order
//
// The scans of lsq_adc.hip and lsq_ivf.hip answer "the nn nearest" and bet on a threshold of their own; here the threshold is the caller's and the list
// must be exactly as long as the answer.  So the candidate rows are walked TWICE by the same walk:
//   COUNT   per (query tile, row range) block, the rows with dist <= r_q are counted per query in registers, reduced over the wave (shuffles) and the block
//           (LDS), and ONE integer per (block, query) is added to count[q].  Integer sums commute: the counts are the same on every call.  No returning
//           atomic anywhere in the pass.
//   PLAN    count -> lims (the exclusive prefix in int64, on the host: the counts come back anyway); the host cuts the queries into fill batches of at
//           most 2^28 records (lsq_range_check.h); a query larger than the budget is a batch of its own.
//   FILL    the same walk appends (lsq_adc_key(dist) << idbits | id) to the query's exact-size segment: staged per wave in LDS, one run of slots claimed
//           per query and flush (adc_scan_kernel's MODE 0).  Every store is guarded against the segment's end although the count is exact.  The order
//           inside a segment varies from run to run; the records are distinct, so the sorted segment does not.
//   SORT    hipcub's segmented radix sort over 32 + idbits bits makes it (dist, id); one hand-out kernel writes dists / ids at lims[q] in the HELD buffers,
//           which the index owns until the next range search or the next call that changes what a search would see.
// Two walks:
//   every row (nprobe == 0)   adc_scan_kernel's geometry, restated: the tables of QT = 16 (m <= 8) or 8 queries in LDS, a lane owns one row and four
//                             queries, the next batch of rows is prefetched, the table reads of a group of steps are in flight together; the dword loader
//                             for rows of 4 / 8 / 12 / 16 bytes and the byte loader; plain rows with dbnorms[i] or packed rows with the norm table in LDS;
//                             a filter's dense road (the bitmap word fetched with the row) and compact road (the walk is over filter_rows).
//   probed lists (nprobe >= 1) ivf_scan_kernel's geometry: one query's table per block, the block walks every gridDim.y-th of that query's probed lists;
//                             plain and packed rows, both loaders, the layout-order filter bits, LSQ_IVF_ADD_COARSE as one more rounded add.
#include <hipcub/hipcub.hpp>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "lsq_internal.h"
#include "lsq_range_check.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RG_THREADS = 1024;             // every-row walk: threads per block (16 waves: one block per CU beside 128 KiB of tables)
constexpr int RG_STAGE = 64;                 // staged records per wave
constexpr int RG_NORM_TABLE = 256;           // floats of the staged norm table of a packed index
constexpr int RG_IVF_THREADS = 256;
constexpr int RG_CHUNK = 16384;              // queries whose tables are resident together (m KiB each)
enum { RG_COUNT = 0, RG_FILL = 1 };
enum { RG_NORM_F32 = 1, RG_NORM_BYTE = 2 };

struct RangeStage {
    uint64_t rec[RG_STAGE];
    unsigned slot[RG_STAGE];                 // query of the tile (0 .. QT-1)
    unsigned hist[16], base[16];
    unsigned n, pad[3];
};

// what both passes of the every-row walk are launched with.  Slots count the queries of the resident chunk; the launch covers tiles tile0 .. and only the
// slots qa <= slot < qb take part (the others' radius is NaN: nothing passes)
struct RangeScan {
    const float *LUT;                        // adc_lut_kernel's tiles of the chunk
    const uint8_t *codes; const float *dbnorms;
    const uint32_t *fbits; const int *frows;
    const float *radius;                     // [slot]
    unsigned *count;                         // COUNT: count[slot] += the block's hits; FILL: cursor[slot], the slots of the segment handed out so far
    const int64_t *lims;                     // FILL: [slot], [slot + 1]: the query's segment in the result
    uint64_t *out; int64_t out_base;         // FILL: record r of the segment goes to out[lims[slot] - out_base + r]
    int n, m, cstride, qa, qb, tile0, per_block, idbits;
};

// PASS = RG_COUNT / RG_FILL.  MW > 0: rows of 4 MW = cstride bytes, read as dwords; MW = 0: any m, byte reads of rows cstride bytes apart.  NORM: RG_NORM_F32 --
// dbnorms[i]; RG_NORM_BYTE -- a packed row (m code bytes, then the norm byte; m = 4 MW - 1 on the dword loader) and dbnorms = the norm table of 256 floats,
// staged behind the query tables.  FILT: frows == nullptr -- the dense road, the word of fbits that holds row i's bit is fetched with its code; frows != nullptr
// -- the compact road, position s of the walk is row frows[s], s < n = the allowed rows.  The distance of a row is computed by adc_scan_kernel's instructions
// on the same operands in the same order on every road and in both passes.
template <int QT, int PASS, int MW, int NORM, bool FILT>
__global__ __launch_bounds__(RG_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void range_scan_kernel(const RangeScan a) {
    extern __shared__ __attribute__((aligned(16))) float lut[];      // [m * 256][QT], the norm table (RG_NORM_BYTE), then the block's counts (COUNT) or the waves' staging (FILL)
    constexpr int NQ = QT / 4, CPW = 64 / NQ;                        // query quads, rows per wave step
    constexpr int U = MW == 0 ? 1 : (MW <= 2 ? 4 : 2);               // steps per batch
    // steps whose table reads are in flight together (<= 64 registers of them).  The filtered fill at 8-byte rows keeps one: with the rows' ids and bits and the
    // staging's addresses beside two steps of reads it would spill past the 128 registers of four waves per SIMD
    constexpr int G = (MW == 1 || (MW == 2 && !(FILT && PASS == RG_FILL))) ? 2 : 1;
    constexpr int CW = MW > 0 ? MW : 1;
    constexpr int NT = NORM == RG_NORM_BYTE ? 4 * CW - 1 : 4 * CW;   // bytes of a dword-loaded row that index tables
    constexpr int NTAB = NORM == RG_NORM_BYTE ? RG_NORM_TABLE : 0;
    constexpr int NW = RG_THREADS / 64;
    const int tile = a.tile0 + (int)blockIdx.x;
    const int m = a.m, n = a.n, entries = m * LSQ_H;
    {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(a.LUT + (int64_t)tile * entries * QT);
        f32x4 *dst = reinterpret_cast<f32x4 *>(lut);
        for (int t = threadIdx.x; t < entries * QT / 4; t += RG_THREADS) dst[t] = src[t];
    }
    const float *ntab = lut + (size_t)entries * QT;
    if constexpr (NORM == RG_NORM_BYTE) {
        if (threadIdx.x < RG_NORM_TABLE) lut[(size_t)entries * QT + threadIdx.x] = a.dbnorms[threadIdx.x];
    }
    unsigned *blockcnt = reinterpret_cast<unsigned *>(lut + (size_t)entries * QT + NTAB);      // COUNT: [QT]
    if (PASS == RG_COUNT && threadIdx.x < QT) blockcnt[threadIdx.x] = 0u;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    RangeStage *stage = reinterpret_cast<RangeStage *>(lut + (size_t)entries * QT + NTAB) + wave;      // FILL
    if (PASS == RG_FILL && lane == 0) stage->n = 0;
    __syncthreads();
    const int qq = lane % NQ, cs = lane / NQ;
    const int slot0 = tile * QT + 4 * qq;                            // the lane's four queries
    float rf[4];                                                     // radii: a row passes iff dist <= r (a NaN on either side does not)
#pragma unroll
    for (int c = 0; c < 4; ++c) rf[c] = (slot0 + c >= a.qa && slot0 + c < a.qb) ? a.radius[slot0 + c] : __uint_as_float(0x7fc00000u);
    unsigned cnt[4] = {0u, 0u, 0u, 0u};
    const int first = blockIdx.y * a.per_block;
    const int last = first + a.per_block < n ? first + a.per_block : n;
    const f32x4 *lut4 = reinterpret_cast<const f32x4 *>(lut);
    // FILL: a record is parked in the wave's staging list; a flush claims ONE run of slots per query of the tile (16 lanes, one wait) instead of one returning
    // atomic -- a round trip to L2 that stalls the wave -- per record
    auto store = [&](unsigned q, unsigned at, uint64_t rec) {        // slot `at` of query q's segment, guarded against the segment's end
        const int slot = tile * QT + (int)q;
        const int64_t seg = a.lims[slot], len = a.lims[slot + 1] - seg;
        if ((int64_t)at < len) a.out[seg - a.out_base + (int64_t)at] = rec;
    };
    auto flush = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const unsigned have_n = stage->n < (unsigned)RG_STAGE ? stage->n : (unsigned)RG_STAGE;
        if (lane < QT) stage->hist[lane] = 0;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const bool have = (unsigned)lane < have_n;
        const uint64_t rec = have ? stage->rec[lane] : 0ull;
        const unsigned q = have ? stage->slot[lane] : 0u;
        const unsigned rank = have ? atomicAdd(&stage->hist[q], 1u) : 0u;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (lane < QT) {
            const unsigned c = stage->hist[lane];
            stage->base[lane] = c ? atomicAdd(&a.count[tile * QT + lane], c) : 0u;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (have) store(q, stage->base[q] + rank, rec);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (lane == 0) stage->n = 0;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    };

    struct Batch { uint32_t w[U][CW]; float nrm[U]; int row[FILT ? U : 1]; uint32_t ok[FILT ? U : 1]; };
    const bool compact = FILT && a.frows != nullptr;                 // (block-uniform)
    // FILT: the row of walk position s and whether it is allowed; a dead position (s >= last) reads the block's first position, which exists
    auto row_of = [&](int s, uint32_t &ok) -> int64_t {
        const int64_t at = s < last ? s : first;
        if (compact) { ok = 1u; return (int64_t)a.frows[at]; }
        ok = (a.fbits[at >> 5] >> (at & 31)) & 1u;
        return at;
    };
    auto fetch = [&](Batch &bt, int s0) {                            // rows s0 + u * CPW + cs, u < U (dead ones read the block's first row)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int s = s0 + u * CPW + cs;
            int64_t i;
            if constexpr (FILT) {
                i = row_of(s, bt.ok[u]);
                bt.row[u] = (int)i;
            } else {
                i = s < last ? s : first;
            }
            if (MW > 0) {
                const uint32_t *cp = reinterpret_cast<const uint32_t *>(a.codes + i * (4 * CW));
#pragma unroll
                for (int t = 0; t < CW; ++t) bt.w[u][t] = cp[t];
            }
            if (NORM == RG_NORM_F32) bt.nrm[u] = a.dbnorms[i];
        }
    };
    Batch cur, nxt;
    int s0 = first + wave * (U * CPW);
    if (s0 < last) fetch(cur, s0);
    for (; s0 < last; s0 += NW * U * CPW) {
        const int sn = s0 + NW * U * CPW;
        if (sn < last) fetch(nxt, sn);
#pragma unroll
        for (int u0 = 0; u0 < U; u0 += G) {
            // all table reads of G steps are requested before the first is consumed
            f32x4 v[G][MW > 0 ? 4 * CW : 1];
            f32x4 dist[G];
            float nb[G];                                             // RG_NORM_BYTE: cbnorms[c_i], requested with the table reads
            if (MW > 0) {
#pragma unroll
                for (int g = 0; g < G; ++g) {
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const uint32_t b = (cur.w[u0 + g][j >> 2] >> (8 * (j & 3))) & 0xffu;
                        v[g][j] = lut4[(j * LSQ_H + (int)b) * NQ + qq];
                    }
                    if constexpr (NORM == RG_NORM_BYTE) nb[g] = ntab[cur.w[u0 + g][CW - 1] >> 24];
                }
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int s = s0 + (u0 + g) * CPW + cs;
                f32x4 acc = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                if (MW > 0) {
#pragma unroll
                    for (int j = 0; j < NT; ++j) acc = acc + v[g][j];
                } else {
                    const int64_t i = FILT ? (int64_t)cur.row[u0 + g] : (int64_t)(s < last ? s : first);
                    const uint8_t *cp = a.codes + i * a.cstride;
                    for (int j = 0; j < m; ++j) acc = acc + lut4[(j * LSQ_H + (int)cp[j]) * NQ + qq];
                    if constexpr (NORM == RG_NORM_BYTE) nb[g] = ntab[cp[m]];
                }
                if constexpr (NORM == RG_NORM_F32) {
                    const float nrm = cur.nrm[u0 + g];
                    dist[g] = acc + (f32x4){nrm, nrm, nrm, nrm};
                } else {
                    dist[g] = acc + (f32x4){nb[g], nb[g], nb[g], nb[g]};
                }
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int s = s0 + (u0 + g) * CPW + cs;
                const bool live = s < last;
                const int64_t i = FILT ? (int64_t)cur.row[u0 + g] : (int64_t)(live ? s : first);
                const bool allowed = FILT ? cur.ok[u0 + g] != 0u : true;
                const float dv[4] = {dist[g].x, dist[g].y, dist[g].z, dist[g].w};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const bool hit = live && allowed && dv[c] <= rf[c];
                    if (PASS == RG_COUNT) {
                        cnt[c] += hit ? 1u : 0u;
                    } else {
                        if (!hit) continue;
                        const uint64_t rec = ((uint64_t)lsq_adc_key(dv[c]) << a.idbits) | (uint64_t)(i + 1);      // ids are 1-BASED
                        const unsigned pos = atomicAdd(&stage->n, 1u);
                        if (pos < (unsigned)RG_STAGE) {
                            stage->rec[pos] = rec;
                            stage->slot[pos] = (unsigned)(4 * qq + c);
                        } else {                                     // more than a list's worth in one group: the direct road
                            store((unsigned)(4 * qq + c), atomicAdd(&a.count[slot0 + c], 1u), rec);
                        }
                    }
                }
            }
            if (PASS == RG_FILL) {
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                if (__builtin_amdgcn_readfirstlane((int)stage->n) >= RG_STAGE / 2) flush();      // wave-uniform
            }
        }
        if (sn < last) cur = nxt;
    }
    if (PASS == RG_FILL) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (__builtin_amdgcn_readfirstlane((int)stage->n) > 0) flush();
    } else {
        // the lanes of a wave that share a query quad differ in lane / NQ: butterfly over those bits, then one LDS add per (wave, query), one global add
        // per (block, query)
#pragma unroll
        for (int off = NQ; off < 64; off <<= 1) {
#pragma unroll
            for (int c = 0; c < 4; ++c) cnt[c] += __shfl_xor(cnt[c], off, 64);
        }
        if (lane < NQ) {
#pragma unroll
            for (int c = 0; c < 4; ++c) if (cnt[c]) atomicAdd(&blockcnt[4 * qq + c], cnt[c]);
        }
        __syncthreads();
        if (threadIdx.x < QT) {
            const unsigned c = blockcnt[threadIdx.x];
            if (c) atomicAdd(&a.count[tile * QT + threadIdx.x], c);  // (the value is not used: no round trip)
        }
    }
}

// ---- the probed lists ------------------------------------------------------------------------------------------------------------------------------
struct RangeIvf {
    const float *LUT; int QT;                                        // adc_lut_kernel's tiles of the chunk
    const uint8_t *codes; const float *norms; const int *ids; const int *off;      // the inverted layout
    const int *probe; const float *coarse;                           // [slot][nprobe]: the probed lists in rank order and their coarse distances
    const uint32_t *lbits;                                           // FILT: the filter's bitmap in layout order
    const float *radius;                                             // [slot]
    unsigned *count;                                                 // COUNT: count[slot] +=; FILL: cursor[slot]
    unsigned long long *rows;                                        // COUNT: += the rows walked
    const int64_t *lims; uint64_t *out; int64_t out_base;            // FILL, as in RangeScan
    int nprobe, m, idbits, add, sa;                                  // sa: the slot of block 0
};

// A block owns ONE query and every gridDim.y-th of its probed lists; a lane owns a row of the list.  The distance is ivf_scan_kernel's: m LDS gathers and m adds
// in order, the norm, then (add) the coarse distance of the row's list.  PACKED / MW / FILT as there
template <int MW, int PASS, bool PACKED, bool FILT>
__global__ __launch_bounds__(RG_IVF_THREADS) void range_ivf_kernel(const RangeIvf a) {
    __shared__ float lut[LSQ_MAX_M * LSQ_H + (PACKED ? 256 : 0)];    // the query's table: m KiB used; PACKED: the norm table behind all 16 KiB
    __shared__ unsigned wcnt[RG_IVF_THREADS / 64];
    constexpr int NT = PACKED ? 4 * MW - 1 : 4 * MW;                 // bytes of a dword-loaded row that index tables
    const int t = threadIdx.x, slot = a.sa + (int)blockIdx.x, lane = t & 63;
    const int entries = a.m * LSQ_H;
    {
        const float *__restrict__ src = a.LUT + (int64_t)(slot / a.QT) * entries * a.QT + slot % a.QT;
        for (int e = t; e < entries; e += RG_IVF_THREADS) lut[e] = src[(int64_t)e * a.QT];
        if constexpr (PACKED) lut[LSQ_MAX_M * LSQ_H + t] = a.norms[t];      // (RG_IVF_THREADS == 256 entries)
    }
    __syncthreads();
    const int *__restrict__ probe = a.probe + (int64_t)slot * a.nprobe;
    const float rad = a.radius[slot];
    const int64_t seg = PASS == RG_FILL ? a.lims[slot] : 0, seglen = PASS == RG_FILL ? a.lims[slot + 1] - seg : 0;
    unsigned cnt = 0;
    unsigned long long walked = 0;
    for (int r = (int)blockIdx.y; r < a.nprobe; r += (int)gridDim.y) {
        const int l = probe[r];
        const int b = a.off[l], len = a.off[l + 1] - b;
        const float cq = a.add ? a.coarse[(int64_t)slot * a.nprobe + r] : 0.0f;
        walked += (unsigned long long)len;
        for (int i0 = 0; i0 < len; i0 += RG_IVF_THREADS) {           // (block-uniform trip count; len >= 1 inside: row b exists)
            const int i = i0 + t;
            const bool live = i < len;
            const int64_t row = (int64_t)b + (live ? i : 0);
            float acc = 0.0f;
            float nrm;
            if constexpr (MW > 0) {
                const uint32_t *cp = reinterpret_cast<const uint32_t *>(a.codes + row * (4 * MW));
                uint32_t w[MW > 0 ? MW : 1];
#pragma unroll
                for (int k = 0; k < MW; ++k) w[k] = cp[k];
#pragma unroll
                for (int j = 0; j < NT; ++j) acc = acc + lut[j * LSQ_H + (int)((w[j >> 2] >> (8 * (j & 3))) & 0xffu)];
                if constexpr (PACKED) nrm = lut[LSQ_MAX_M * LSQ_H + (int)(w[MW > 0 ? MW - 1 : 0] >> 24)];
            } else {
                const uint8_t *cp = a.codes + row * (PACKED ? a.m + 1 : a.m);
                for (int j = 0; j < a.m; ++j) acc = acc + lut[j * LSQ_H + (int)cp[j]];
                if constexpr (PACKED) nrm = lut[LSQ_MAX_M * LSQ_H + (int)cp[a.m]];
            }
            if constexpr (!PACKED) nrm = a.norms[row];
            float dist = acc + nrm;
            if (a.add) dist = dist + cq;                             // one more rounded add
            bool allowed = true;
            if constexpr (FILT) allowed = ((a.lbits[row >> 5] >> (row & 31)) & 1u) != 0;
            const bool hit = live && allowed && dist <= rad;
            if (PASS == RG_COUNT) {
                cnt += hit ? 1u : 0u;
            } else {
                const unsigned long long mask = __ballot(hit);
                if (mask) {                                          // (wave-uniform) one atomic for the wave's records of this step
                    const int leader = __ffsll((long long)mask) - 1;
                    unsigned base = 0;
                    if (lane == leader) base = atomicAdd(&a.count[slot], (unsigned)__popcll(mask));
                    base = __shfl(base, leader, 64);
                    const int64_t at = (int64_t)base + __popcll(mask & ((1ull << lane) - 1ull));
                    const uint64_t rec = ((uint64_t)lsq_adc_key(dist) << a.idbits) | (uint64_t)(uint32_t)(a.ids[row] + 1);      // the ORIGINAL id, 1-based
                    if (hit && at < seglen) a.out[seg - a.out_base + at] = rec;
                }
            }
        }
    }
    if (PASS == RG_COUNT) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
        if (lane == 0) wcnt[t >> 6] = cnt;
        __syncthreads();
        if (t == 0) {
            unsigned c = 0;
            for (int w = 0; w < RG_IVF_THREADS / 64; ++w) c += wcnt[w];
            if (c) atomicAdd(&a.count[slot], c);
            if (walked) atomicAdd(a.rows, walked);
        }
    }
}

// ---- the selection's small kernels -------------------------------------------------------------------------------------------------------------------
// the segments of queries qa .. qa + segs - 1 inside the batch's record buffer
__global__ void range_segments_kernel(const int64_t *__restrict__ lims, int qa, int segs, int64_t out_base, int *__restrict__ begin, int *__restrict__ end) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= segs) return;
    begin[j] = (int)(lims[qa + j] - out_base);
    end[j] = (int)(lims[qa + j + 1] - out_base);
}

// sorted record r of the batch -> entry out_base + r of the held result (dists / ids point at out_base)
__global__ void range_handout_kernel(const uint64_t *__restrict__ sorted, int64_t records, int idbits, float *__restrict__ dists, int *__restrict__ ids) {
    const uint64_t mask = (1ull << idbits) - 1ull;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < records; r += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t rec = sorted[r];
        dists[r] = lsq_adc_unkey((uint32_t)(rec >> idbits));
        ids[r] = (int)(uint32_t)(rec & mask);
    }
}

template <int QT, int PASS>
int launch_scan(hipStream_t s, RangeScan a, const lsq_search_input &in) {
    const int tiles = (a.qb + QT - 1) / QT - a.qa / QT;
    const int n = in.rows_walked(), m = in.m;                        // compact road: the allowed rows
    if (tiles <= 0 || n == 0) return LSQ_OK;
    a.tile0 = a.qa / QT;
    a.n = n;
    // adc_scan_kernel's grid: enough blocks to fill the chip a few times over, ranges long enough that the table load is amortised
    int ranges = (2048 + tiles - 1) / tiles;
    const int max_ranges = (n + 4095) / 4096;
    if (ranges > max_ranges) ranges = max_ranges;
    if (ranges < 1) ranges = 1;
    if (ranges > 65535) ranges = 65535;
    int per_block = (n + ranges - 1) / ranges;
    per_block = (per_block + 255) & ~255;
    ranges = (n + per_block - 1) / per_block;
    a.per_block = per_block;
    const bool packed = in.packed != 0;
    const int rowb = packed ? m + 1 : m;
    const size_t lds = sizeof(float) * ((size_t)m * LSQ_H * QT + (packed ? RG_NORM_TABLE : 0)) +
                       (PASS == RG_FILL ? sizeof(RangeStage) * (RG_THREADS / 64) : sizeof(unsigned) * QT);
    const bool words = (rowb % 4 == 0) && in.cstride == rowb && (((uintptr_t)in.codes & 3) == 0);
    const dim3 grid((unsigned)tiles, (unsigned)ranges), block(RG_THREADS);
#define RG_LAUNCH_F(MWV, NORMV, FILTV)                                                                                       \
    do {                                                                                                                     \
        LSQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&range_scan_kernel<QT, PASS, MWV, NORMV, FILTV>),          \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                                   \
        hipLaunchKernelGGL((range_scan_kernel<QT, PASS, MWV, NORMV, FILTV>), grid, block, lds, s, a);                        \
    } while (0)
#define RG_LAUNCH(MWV, NORMV)                               \
    do {                                                    \
        if (in.filtered()) RG_LAUNCH_F(MWV, NORMV, true);   \
        else RG_LAUNCH_F(MWV, NORMV, false);                \
    } while (0)
#define RG_LAUNCH_MW(NORMV)                                 \
    do {                                                    \
        if (words && rowb == 4) RG_LAUNCH(1, NORMV);        \
        else if (words && rowb == 8) RG_LAUNCH(2, NORMV);   \
        else if (words && rowb == 12) RG_LAUNCH(3, NORMV);  \
        else if (words && rowb == 16) RG_LAUNCH(4, NORMV);  \
        else RG_LAUNCH(0, NORMV);                           \
    } while (0)
    if (packed) RG_LAUNCH_MW(RG_NORM_BYTE);
    else RG_LAUNCH_MW(RG_NORM_F32);
#undef RG_LAUNCH_MW
#undef RG_LAUNCH
#undef RG_LAUNCH_F
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

template <int PASS>
int launch_ivf(hipStream_t s, const RangeIvf &a, int slots, bool packed) {
    if (slots <= 0) return LSQ_OK;
    const int rowb = packed ? a.m + 1 : a.m;                         // bytes of a row: the dword loader takes whole words
    int splits = (2048 + slots - 1) / slots;                         // ivf_scan_kernel's grid
    if (splits > a.nprobe) splits = a.nprobe;
    if (splits > 65535) splits = 65535;
    if (splits < 1) splits = 1;
    const dim3 grid((unsigned)slots, (unsigned)splits), block(RG_IVF_THREADS);
#define RG_IVF_LAUNCH(MWV)                                                                              \
    do {                                                                                                \
        if (a.lbits) {                                                                                  \
            if (packed) hipLaunchKernelGGL((range_ivf_kernel<MWV, PASS, true, true>), grid, block, 0, s, a);    \
            else hipLaunchKernelGGL((range_ivf_kernel<MWV, PASS, false, true>), grid, block, 0, s, a);          \
        } else if (packed) hipLaunchKernelGGL((range_ivf_kernel<MWV, PASS, true, false>), grid, block, 0, s, a); \
        else hipLaunchKernelGGL((range_ivf_kernel<MWV, PASS, false, false>), grid, block, 0, s, a);     \
    } while (0)
    if (rowb == 4) RG_IVF_LAUNCH(1);
    else if (rowb == 8) RG_IVF_LAUNCH(2);
    else if (rowb == 12) RG_IVF_LAUNCH(3);
    else if (rowb == 16) RG_IVF_LAUNCH(4);
    else RG_IVF_LAUNCH(0);
#undef RG_IVF_LAUNCH
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

}  // namespace

struct lsq_range_state {
    DevBuf held_d, held_i;                           // the held result: dists / ids [results]
    bool held = false;
    int64_t held_total = 0;
    DevBuf lut, count, cursor, lims, rows, rec_a, rec_b, seg, tmp;      // a call's scratch
    PhaseClock<2> clock;
    lsq_range_info info{};
};

void lsq_range_drop(lsq_range_state *st) {
    if (!st) return;
    st->held_d.release(); st->held_i.release();
    st->held = false; st->held_total = 0;
}

void lsq_range_free(lsq_range_state *st) {
    if (!st) return;
    lsq_range_drop(st);
    DevBuf *all[] = {&st->lut, &st->count, &st->cursor, &st->lims, &st->rows, &st->rec_a, &st->rec_b, &st->seg, &st->tmp};
    for (DevBuf *b : all) b->release();
    st->clock.release();
    delete st;
}

void lsq_range_get_info(const lsq_range_state *st, lsq_range_info *out) { *out = st ? st->info : lsq_range_info{}; }

namespace {

// one phase of a profiled call: the time between two marks, added to *ms (a wait; nothing without option "profile")
struct Lap {
    lsq_range_state *st; hipStream_t s; bool timed;
    int begin() { LSQ_TRY(st->clock.begin(timed)); return st->clock.mark(s); }
    int end(double *ms) {
        LSQ_TRY(st->clock.mark(s));
        float t[1];
        LSQ_TRY(st->clock.read(t));
        *ms += t[0];
        return LSQ_OK;
    }
};

// the sort of a batch's segments and the hand-out into the held buffers
int select_batch(lsq_range_state *st, hipStream_t s, int qa, int qb, int64_t out_base, int64_t records, int idbits) {
    const int segs = qb - qa, end_bit = 32 + idbits;
    const uint64_t *in = st->rec_a.as<uint64_t>();
    uint64_t *out = st->rec_b.as<uint64_t>();
    size_t bytes = 0;
    if (segs == 1) {                                 // one query (perhaps larger than the budget): the whole-array sort
        LSQ_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, in, out, (int)records, 0, end_bit, s));
        LSQ_TRY(st->tmp.ensure(bytes > 0 ? bytes : 16));
        LSQ_HIP(hipcub::DeviceRadixSort::SortKeys(st->tmp.p, bytes, in, out, (int)records, 0, end_bit, s));
    } else {
        LSQ_TRY(st->seg.ensure(sizeof(int) * 2 * (size_t)segs));
        int *begin = st->seg.as<int>(), *end = begin + segs;
        hipLaunchKernelGGL(range_segments_kernel, dim3((unsigned)((segs + 255) / 256)), dim3(256), 0, s, st->lims.as<int64_t>(), qa, segs, out_base, begin, end);
        LSQ_HIP(hipGetLastError());
        LSQ_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, bytes, in, out, (int)records, segs, begin, end, 0, end_bit, s));
        LSQ_TRY(st->tmp.ensure(bytes > 0 ? bytes : 16));
        LSQ_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(st->tmp.p, bytes, in, out, (int)records, segs, begin, end, 0, end_bit, s));
    }
    const int64_t blocks = std::min<int64_t>((records + 255) / 256, 4096);
    hipLaunchKernelGGL(range_handout_kernel, dim3((unsigned)blocks), dim3(256), 0, s, out, records, idbits, st->held_d.as<float>() + out_base,
                       st->held_i.as<int>() + out_base);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

}  // namespace

int lsq_range_search(hipStream_t s, lsq_range_state **pst, const lsq_range_call &call, int64_t *h_lims) {
    if (!*pst) *pst = new lsq_range_state();
    lsq_range_state *st = *pst;
    lsq_range_drop(st);                              // the former result leaves whatever becomes of this call
    st->info = lsq_range_info{};
    st->info.road = call.road;
    const int nq = call.nq;
    h_lims[0] = 0;
    const bool ivf = call.nprobe >= 1;
    const lsq_search_input &in = call.in;
    const int m = in.m, d = in.d, QT = lsq_adc_lut_qt(m);
    const bool timed = call.timed != 0;
    Lap lap{st, s, timed};
    if (nq > 0) {
        // chunks of queries whose tables are resident together and, on the list road, whose per-(query, probe) words stay below 2^28 (lsq_ivf_search's rule);
        // whole tiles, so that a chunk's slots start a tile
        int64_t qc = RG_CHUNK;
        if (ivf) qc = std::min<int64_t>(qc, std::max<int64_t>(QT, ((int64_t)(1u << 28) / ((int64_t)call.nprobe + 1)) / QT * QT));
        const int nchunks = (int)((nq + qc - 1) / qc);
        const size_t slots_max = (size_t)((std::min<int64_t>(qc, nq) + QT - 1) / QT) * QT;
        LSQ_TRY(st->lut.ensure(sizeof(float) * slots_max * m * LSQ_H));
        LSQ_TRY(st->count.ensure(sizeof(unsigned) * ((size_t)nq + QT)));
        LSQ_TRY(st->cursor.ensure(sizeof(unsigned) * slots_max));
        LSQ_TRY(st->lims.ensure(sizeof(int64_t) * ((size_t)nq + 1)));
        LSQ_TRY(st->rows.ensure(sizeof(unsigned long long)));
        LSQ_HIP(hipMemsetAsync(st->count.p, 0, sizeof(unsigned) * ((size_t)nq + QT), s));
        LSQ_HIP(hipMemsetAsync(st->rows.p, 0, sizeof(unsigned long long), s));
        lsq_ivf_probes pv{};
        const int idbits = lsq_adc_idbits(in.n);
        // a chunk's set-up: the probed lists (list road) and the tables
        auto prepare = [&](int64_t c0, int nqc) -> int {
            if (ivf) {
                double ms = 0.0;
                LSQ_TRY(lsq_ivf_coarse(s, call.ivf, call.adc, call.q_coarse + c0 * call.ldc, call.ldc, nqc, call.nprobe, call.coarse, call.timed, &pv, &ms));
                st->info.coarse_ms += ms;
            }
            lsq_search_input li = in;
            li.Q = static_cast<const float *>(in.Q) + c0 * d;
            LSQ_TRY(lap.begin());
            LSQ_TRY(lsq_adc_launch_lut(s, li, nullptr, 0, nqc, st->lut.as<float>()));
            return lap.end(&st->info.lut_ms);
        };
        auto scan_args = [&](int64_t c0) {
            RangeScan a{};
            a.LUT = st->lut.as<float>(); a.codes = in.codes; a.dbnorms = in.dbnorms; a.fbits = in.filter_bits; a.frows = in.filter_rows;
            a.radius = call.radius + c0; a.m = m; a.cstride = in.cstride; a.idbits = idbits;
            return a;
        };
        auto ivf_args = [&](int64_t c0) {
            RangeIvf a{};
            a.LUT = st->lut.as<float>(); a.QT = QT; a.codes = pv.codes; a.norms = pv.norms; a.ids = pv.ids; a.off = pv.off;
            a.probe = pv.probe; a.coarse = pv.coarse; a.lbits = call.lbits; a.radius = call.radius + c0; a.rows = st->rows.as<unsigned long long>();
            a.nprobe = call.nprobe; a.m = m; a.idbits = idbits; a.add = (call.flags & LSQ_IVF_ADD_COARSE) ? 1 : 0;
            return a;
        };
        // ---- COUNT
        for (int ch = 0; ch < nchunks; ++ch) {
            const int64_t c0 = (int64_t)ch * qc;
            const int nqc = (int)std::min<int64_t>(qc, nq - c0);
            LSQ_TRY(prepare(c0, nqc));
            LSQ_TRY(lap.begin());
            if (ivf) {
                RangeIvf a = ivf_args(c0);
                a.count = st->count.as<unsigned>() + c0; a.sa = 0;
                LSQ_TRY(launch_ivf<RG_COUNT>(s, a, nqc, pv.packed != 0));
            } else {
                RangeScan a = scan_args(c0);
                a.count = st->count.as<unsigned>() + c0; a.qa = 0; a.qb = nqc;
                if (QT == 16) LSQ_TRY((launch_scan<16, RG_COUNT>(s, a, in)));
                else LSQ_TRY((launch_scan<8, RG_COUNT>(s, a, in)));
            }
            LSQ_TRY(lap.end(&st->info.count_ms));
        }
        // ---- PLAN: the counts come back, lims goes out
        std::vector<uint32_t> h_count((size_t)nq);
        unsigned long long h_rows = 0;
        LSQ_HIP(hipMemcpyAsync(h_count.data(), st->count.p, sizeof(uint32_t) * (size_t)nq, hipMemcpyDeviceToHost, s));
        LSQ_HIP(hipMemcpyAsync(&h_rows, st->rows.p, sizeof(h_rows), hipMemcpyDeviceToHost, s));
        LSQ_HIP(hipStreamSynchronize(s));
        st->info.max_per_query = lsq_range_prefix(h_count.data(), nq, h_lims);
        st->info.rows_walked = ivf ? (int64_t)h_rows : (int64_t)nq * in.rows_walked();
        const int64_t total = h_lims[nq];
        LSQ_HIP(hipMemcpyAsync(st->lims.p, h_lims, sizeof(int64_t) * ((size_t)nq + 1), hipMemcpyHostToDevice, s));
        if (total > 0) {
            LSQ_TRY(st->held_d.ensure(sizeof(float) * (size_t)total));
            LSQ_TRY(st->held_i.ensure(sizeof(int) * (size_t)total));
        }
        // ---- FILL, SORT, hand-out: batch by batch
        std::vector<int64_t> cuts;
        for (int ch = 0; ch < nchunks && total > 0; ++ch) {
            const int64_t c0 = (int64_t)ch * qc;
            const int nqc = (int)std::min<int64_t>(qc, nq - c0);
            if (h_lims[c0 + nqc] == h_lims[c0]) continue;            // nothing within the radius of any query of the chunk
            if (nchunks > 1) LSQ_TRY(prepare(c0, nqc));              // (one chunk: its tables and probed lists are still there)
            LSQ_HIP(hipMemsetAsync(st->cursor.p, 0, sizeof(unsigned) * (size_t)((nqc + QT - 1) / QT) * QT, s));
            lsq_range_cut(h_lims, c0, c0 + nqc, call.budget, &cuts);
            for (size_t b = 0; b + 1 < cuts.size(); ++b) {
                const int64_t qa = cuts[b], qb = cuts[b + 1], out_base = h_lims[qa], records = h_lims[qb] - out_base;
                if (records == 0) continue;
                if (records > (int64_t)INT32_MAX) { lsq_set_error("lsq_index_range_search: a batch of %lld records exceeds 2^31 - 1", (long long)records); return LSQ_EINVAL; }
                LSQ_TRY(st->rec_a.ensure(sizeof(uint64_t) * (size_t)records));
                LSQ_TRY(st->rec_b.ensure(sizeof(uint64_t) * (size_t)records));
                LSQ_TRY(lap.begin());
                if (ivf) {
                    RangeIvf a = ivf_args(c0);
                    a.count = st->cursor.as<unsigned>(); a.lims = st->lims.as<int64_t>() + c0; a.out = st->rec_a.as<uint64_t>(); a.out_base = out_base;
                    a.sa = (int)(qa - c0);
                    LSQ_TRY(launch_ivf<RG_FILL>(s, a, (int)(qb - qa), pv.packed != 0));
                } else {
                    RangeScan a = scan_args(c0);
                    a.count = st->cursor.as<unsigned>(); a.lims = st->lims.as<int64_t>() + c0; a.out = st->rec_a.as<uint64_t>(); a.out_base = out_base;
                    a.qa = (int)(qa - c0); a.qb = (int)(qb - c0);
                    if (QT == 16) LSQ_TRY((launch_scan<16, RG_FILL>(s, a, in)));
                    else LSQ_TRY((launch_scan<8, RG_FILL>(s, a, in)));
                }
                LSQ_TRY(lap.end(&st->info.fill_ms));
                LSQ_TRY(lap.begin());
                LSQ_TRY(select_batch(st, s, (int)qa, (int)qb, out_base, records, idbits));
                LSQ_TRY(lap.end(&st->info.sort_ms));
                st->info.batches += 1;
            }
        }
        if (call.lims_dev) LSQ_HIP(hipMemcpyAsync(call.lims_dev, st->lims.p, sizeof(int64_t) * ((size_t)nq + 1), hipMemcpyDeviceToDevice, s));
    } else if (call.lims_dev) {
        LSQ_HIP(hipMemcpyAsync(call.lims_dev, h_lims, sizeof(int64_t), hipMemcpyHostToDevice, s));
    }
    LSQ_HIP(hipStreamSynchronize(s));
    st->held = true;
    st->held_total = h_lims[nq];
    st->info.queries = nq;
    st->info.results = st->held_total;
    st->info.held_bytes = (int64_t)(st->held_d.cap + st->held_i.cap);
    return LSQ_OK;
}

int lsq_range_fetch(hipStream_t s, lsq_range_state *st, float *dists, int *ids, int64_t capacity, int on_device) {
    if (!st || !st->held) { lsq_set_error("lsq_index_range_fetch: the index holds no range result (none made yet, or dropped by a call that changed the index)"); return LSQ_EINVAL; }
    if (capacity < st->held_total) {
        lsq_set_error("lsq_index_range_fetch: capacity %lld is less than the %lld held results", (long long)capacity, (long long)st->held_total);
        return LSQ_EINVAL;
    }
    if (st->held_total == 0) return LSQ_OK;
    if (!dists || !ids) { lsq_set_error("lsq_index_range_fetch: null pointer"); return LSQ_EINVAL; }
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    LSQ_HIP(hipMemcpyAsync(dists, st->held_d.p, sizeof(float) * (size_t)st->held_total, kind, s));
    LSQ_HIP(hipMemcpyAsync(ids, st->held_i.p, sizeof(int) * (size_t)st->held_total, kind, s));
    LSQ_HIP(hipStreamSynchronize(s));
    return LSQ_OK;
}

// ---- the host drop-in and engine-less road: the contract on plain arrays ------------------------------------------------------------------------------
namespace {

inline uint32_t host_key(float v) {
    if (v != v) return 0xffffffffu;
    uint32_t b;
    memcpy(&b, &v, 4);
    return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
inline float host_unkey(uint32_t k) {
    const uint32_t b = k == 0xffffffffu ? 0x7fc00000u : ((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
    float v;
    memcpy(&v, &b, 4);
    return v;
}

struct RangeCpu {
    const uint8_t *codes; const float *K, *dbnorms, *cent; const int32_t *lor; const uint8_t *allowed; const float *q_scan, *q_coarse, *radius;
    int n, m, h, d, nlist, ldq, nprobe, add;
    std::vector<uint64_t> *found;                    // [nq]: the records (key << 32 | id) of every query, sorted
};

void range_queries(const RangeCpu a, int q0, int q1) {
    const int total = a.m * a.h;
    const bool lists = a.nprobe >= 1;
    std::vector<float> table((size_t)total), coarse((size_t)(lists ? a.nlist : 0));
    std::vector<uint64_t> ckeys((size_t)(lists ? a.nlist : 0));
    std::vector<char> probed((size_t)(lists ? a.nlist : 0));
    for (int q = q0; q < q1; ++q) {
        const float *qs = a.q_scan + (size_t)q * a.ldq;
        if (lists) {                                                 // lsq_ivf_search_cpu's probed lists
            const float *qc = a.q_coarse + (size_t)q * a.ldq;
            for (int l = 0; l < a.nlist; ++l) {
                const float *c = a.cent + (size_t)l * a.d;
                float acc = 0.0f;
                for (int s = 0; s < a.d; ++s) {
                    const float e = c[s] - qc[s];
                    acc += e * e;
                }
                coarse[(size_t)l] = acc;
                ckeys[(size_t)l] = ((uint64_t)host_key(acc) << 32) | (uint32_t)l;
            }
            std::partial_sort(ckeys.begin(), ckeys.begin() + a.nprobe, ckeys.end());
            std::fill(probed.begin(), probed.end(), 0);
            for (int r = 0; r < a.nprobe; ++r) probed[(size_t)(uint32_t)ckeys[(size_t)r]] = 1;
        }
        for (int j = 0; j < total; ++j) {                            // lsq_linscan_aqd_query_extra_byte's table
            const float *c = a.K + (size_t)j * a.d;
            float t = 0.0f;
            for (int k = 0; k < a.d; ++k) t -= 2 * qs[k] * c[k];
            table[(size_t)j] = t;
        }
        const float rad = a.radius[q];
        std::vector<uint64_t> &out = a.found[q];
        for (int i = 0; i < a.n; ++i) {
            if (a.allowed && !a.allowed[i]) continue;
            const int l = lists ? a.lor[i] : 0;
            if (lists && !probed[(size_t)l]) continue;
            const uint8_t *code = a.codes + (size_t)i * a.m;
            float acc = 0.0f;
            for (int k = 0; k < a.m; ++k) acc += table[(size_t)a.h * k + code[k]];
            acc += a.dbnorms[i];
            if (a.add) acc += coarse[(size_t)l];
            if (acc <= rad) out.push_back(((uint64_t)host_key(acc) << 32) | (uint32_t)(i + 1));      // ids are 1-based
        }
        std::sort(out.begin(), out.end());
    }
}

}  // namespace

extern "C" int lsq_range_search_cpu(int64_t *lims, float *dists, int *ids, int64_t capacity, const uint8_t *codes, const float *codebooks,
                                    const float *dbnorms, const float *centroids, const int32_t *list_of_row, int nlist, int nprobe, int flags,
                                    const uint8_t *allowed, const float *q_scan, const float *q_coarse, const float *radius, int n, int m, int h, int d,
                                    int nq, int ldq, int nthreads) {
    const char *fn = "lsq_range_search_cpu";
    if (n < 1 || m < 1 || h < 1 || h > 256 || d < 1 || nq < 0 || ldq < d || capacity < 0) {
        lsq_set_error("%s: bad shape n=%d m=%d h=%d d=%d nq=%d ldq=%d capacity=%lld", fn, n, m, h, d, nq, ldq, (long long)capacity);
        return LSQ_EINVAL;
    }
    if (!lims || !codes || !codebooks || !dbnorms || !q_scan || !radius) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    if (nprobe < 0) { lsq_set_error("%s: nprobe < 0", fn); return LSQ_EINVAL; }
    if (flags & ~LSQ_IVF_ADD_COARSE) { lsq_set_error("%s: unknown flags %d", fn, flags); return LSQ_EINVAL; }
    if (nprobe == 0 && flags) { lsq_set_error("%s: LSQ_IVF_ADD_COARSE needs nprobe >= 1", fn); return LSQ_EINVAL; }
    if (nprobe >= 1) {
        if (!centroids || !list_of_row) { lsq_set_error("%s: nprobe >= 1 without centroids or list_of_row", fn); return LSQ_EINVAL; }
        if (nlist < 1 || nlist > (1 << 24)) { lsq_set_error("%s: needs 1 <= nlist <= 2^24 (got %d)", fn, nlist); return LSQ_EINVAL; }
        if (nprobe > nlist) { lsq_set_error("%s: needs nprobe <= nlist (got nprobe=%d nlist=%d)", fn, nprobe, nlist); return LSQ_EINVAL; }
        for (int i = 0; i < n; ++i)
            if (list_of_row[i] < 0 || list_of_row[i] >= nlist) {
                lsq_set_error("%s: list_of_row[%d] = %d lies outside [0, %d)", fn, i, list_of_row[i], nlist);
                return LSQ_EINVAL;
            }
    }
    lims[0] = 0;
    if (nq == 0) return LSQ_OK;
    std::vector<std::vector<uint64_t>> found((size_t)nq);
    const RangeCpu a{codes, codebooks, dbnorms, centroids, list_of_row, allowed, q_scan, q_coarse ? q_coarse : q_scan, radius,
                     n, m, h, d, nlist, ldq, nprobe, (flags & LSQ_IVF_ADD_COARSE) ? 1 : 0, found.data()};
    int nt = nthreads > 0 ? nthreads : (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if (nt > nq) nt = nq;
    std::vector<std::thread> pool;
    pool.reserve((size_t)nt);
    for (int t = 0; t < nt; ++t) pool.emplace_back(range_queries, a, (int)((int64_t)nq * t / nt), (int)((int64_t)nq * (t + 1) / nt));
    for (auto &th : pool) th.join();
    for (int q = 0; q < nq; ++q) lims[q + 1] = lims[q] + (int64_t)found[(size_t)q].size();
    if (!dists || !ids || lims[nq] > capacity) return LSQ_OK;        // the count-only call, or the first of two
    for (int q = 0; q < nq; ++q) {
        const std::vector<uint64_t> &f = found[(size_t)q];
        for (size_t r = 0; r < f.size(); ++r) {
            dists[lims[q] + (int64_t)r] = host_unkey((uint32_t)(f[r] >> 32));
            ids[lims[q] + (int64_t)r] = (int)(uint32_t)f[r];
        }
    }
    return LSQ_OK;
}
