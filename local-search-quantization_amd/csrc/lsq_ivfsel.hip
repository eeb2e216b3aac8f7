// lsq_ivfsel.hip -- the inverted-list search with the selection INSIDE the list scan (gfx950; option "ivf_select").
//
// lsq_ivf.hip writes a record per probed row (or per row within the head's bound) to a segment in memory and has hipcub sort the segments; its own profile
// says the sorts are 58 - 87 % of a call.  ivf_scan_kernel already gives one block to one query, and that is the shape in which the nn best records can live
// in the block's LDS.  Here they do: nothing of a query leaves its block but its answer.
//
//   WALK    ivf_scan_kernel's, restated (as lsq_range.hip restated it): one query per blockIdx.x, every gridDim.y-th probed list in rank order, the query's
//           table staged once from adc_lut_kernel's tile column (m KiB, dynamic LDS; PACKED: the norm table of 256 floats behind it), a lane owns a row,
//           the dword loader (MW > 0) or the byte loader, adc_scan_kernel's accumulation order, then the norm, then the one rounded coarse add.  FILT: the
//           filter's bit in layout order is read where the code is read; a row that is not allowed is not offered.
//   RECORD  (lsq_adc_key(dist) << idbits | original id + 1): distinct per row, so the nn smallest are a SET that no arrival order changes.
//   POOL    P = 2 pow2ceil(max(nn, 256)) records of dynamic LDS behind the table (4 KiB at nn <= 256, 32 KiB at nn = 2048: sized from nn, so that a small nn
//           keeps many blocks on a CU).  The block holds `bound` -- all ones until the pool has been compacted to nn records, then the nn-th of them -- and
//           the fill, both as block-uniform registers.  A step of the walk: a lane whose record is < bound takes a slot; slots are handed out per wave by
//           __ballot, ONE integer LDS add by the wave's first hitting lane, and prefix popcounts.  The add goes to one of three step counters used in
//           rotation, so that ONE barrier per step is enough: after it every thread reads the step's count and adds it to its copy of the fill (a wave that
//           runs ahead adds to the next counter, never to the one a slower wave has yet to read; thread 0 clears the counter of the step after next).
//           Which slot a record gets depends on the order of the waves' adds; how many records a step adds does not, so the fill, and with it every
//           decision to compact, is a function of the data and the shapes alone.
//   COMPACT when fewer than 256 slots are free after a step (block-uniform): the slots past the fill up to the next power of two are set to all ones, a
//           bitonic sort in LDS puts the records in order, bound = the nn-th, fill = nn.  Lists are walked nearest first, so the first compaction already
//           leaves a tight bound and most later steps offer nothing.
//   FINISH  gridDim.y == 1: the block sorts what it holds and writes the caller's dists / ids row: lsq_adc_unkey of the key and the id field -- the bits
//           adc_gather_kernel writes, -0 and NaN included -- and (+inf, 0) past the records it has.  gridDim.y > 1: the block writes its <= nn sorted records
//           and their count as a run, and ivf_merge_kernel, one block per query, streams the query's runs through THE SAME pool routine (pool_offer),
//           leaving a run at its first record >= bound, and finishes in the same way.
// No head, no tail, no overflow, no redo: every query is answered in one pass.  Atomics: integer adds in LDS, and one non-returning integer add per block and
// statistic (sums of integers: the same on every call).
#include <algorithm>

#include "lsq_internal.h"
#include "lsq_pool.h"

#pragma clang fp contract(off)

namespace {

// (the pool -- Pool, pool_sort, pool_compact, pool_offer, pool_hand_out -- is lsq_pool.h: one selection, every feeder)
struct IvfSel {
    const float *LUT; int QT;                        // adc_lut_kernel's tiles of this batch
    const uint8_t *codes; const float *norms; const int *ids; const int *off;      // the inverted layout
    const int *probe; const float *coarse;           // [.][nprobe]: the probed lists in rank order and their coarse distances
    const uint32_t *lbits;                           // FILT: the filter's bits in layout order
    int q0, nprobe, m, nn, P, idbits, add;           // the query of a slot is q0 + slot
    float *dists; int *out_ids;                      // [.][nn]: the caller's rows
    uint64_t *part; unsigned *pcount;                // gridDim.y > 1: the runs [slot][y][nn] and their lengths [slot][y]
    unsigned long long *stat;                        // [0] += records offered to pools, [1] += compactions
};

template <int MW, bool PACKED, bool FILT>
__global__ __launch_bounds__(SEL_THREADS) void ivf_topk_kernel(const IvfSel a) {
    extern __shared__ __align__(16) unsigned char sel_lds[];
    __shared__ unsigned tick[4];                                     // the pool's three step counters; [3]: the records this block offered
    constexpr int NT = PACKED ? 4 * MW - 1 : 4 * MW;                 // bytes of a dword-loaded row that index tables
    const int t = threadIdx.x, lane = t & 63, slot = blockIdx.x;
    const int q = a.q0 + slot;
    const int entries = a.m * LSQ_H;
    float *lut = reinterpret_cast<float *>(sel_lds);                 // the query's table; PACKED: the norm table behind it
    Pool p;
    p.rec = reinterpret_cast<uint64_t *>(lut + entries + (PACKED ? 256 : 0));
    p.tick = tick; p.bound = ~0ull; p.fill = 0; p.P = a.P; p.nn = a.nn; p.step = 0u; p.compactions = 0u;
    {
        const float *__restrict__ src = a.LUT + (int64_t)(slot / a.QT) * entries * a.QT + slot % a.QT;
        for (int e = t; e < entries; e += SEL_THREADS) lut[e] = src[(int64_t)e * a.QT];
        if constexpr (PACKED) lut[entries + t] = a.norms[t];         // (SEL_THREADS == 256 entries)
        if (t < 4) tick[t] = 0u;
    }
    __syncthreads();
    const int *__restrict__ probe = a.probe + (int64_t)q * a.nprobe;
    unsigned offered = 0;                                            // (wave-uniform)
    for (int r = (int)blockIdx.y; r < a.nprobe; r += (int)gridDim.y) {
        const int l = probe[r];
        const int b = a.off[l], len = a.off[l + 1] - b;
        const float cq = a.add ? a.coarse[(int64_t)q * a.nprobe + r] : 0.0f;
        for (int i0 = 0; i0 < len; i0 += SEL_THREADS) {              // (block-uniform trip count; len >= 1 inside: row b exists)
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
                if constexpr (PACKED) nrm = lut[entries + (int)(w[MW > 0 ? MW - 1 : 0] >> 24)];
            } else {
                const uint8_t *cp = a.codes + row * (PACKED ? a.m + 1 : a.m);
                for (int j = 0; j < a.m; ++j) acc = acc + lut[j * LSQ_H + (int)cp[j]];
                if constexpr (PACKED) nrm = lut[entries + (int)cp[a.m]];
            }
            if constexpr (!PACKED) nrm = a.norms[row];
            float dist = acc + nrm;
            if (a.add) dist = dist + cq;                             // one more rounded add
            const uint64_t rec = ((uint64_t)lsq_adc_key(dist) << a.idbits) | (uint64_t)(uint32_t)(a.ids[row] + 1);      // the ORIGINAL id, 1-based
            bool offer = live;
            if constexpr (FILT) offer = live && ((a.lbits[row >> 5] >> (row & 31)) & 1u) != 0;
            offered += (unsigned)__popcll(__ballot(offer));
            pool_offer(p, rec, offer && rec < p.bound);
        }
    }
    if (lane == 0 && offered) atomicAdd(&tick[3], offered);          // (read behind the barriers of the sort below)
    if (gridDim.y == 1) {
        pool_hand_out(p, q, a.dists, a.out_ids, a.idbits);
    } else {
        pool_sort(p);
        const int have = p.fill < p.nn ? p.fill : p.nn;
        const int64_t run = (int64_t)slot * gridDim.y + blockIdx.y;
        for (int r = t; r < have; r += SEL_THREADS) a.part[run * a.nn + r] = p.rec[r];
        if (t == 0) a.pcount[run] = (unsigned)have;
    }
    if (t == 0) {
        if (tick[3]) atomicAdd(&a.stat[0], (unsigned long long)tick[3]);
        if (p.compactions) atomicAdd(&a.stat[1], (unsigned long long)p.compactions);
    }
}

// the runs of a query, nearest lists first, through the pool.  A run is sorted: it is left at its first record >= bound
__global__ __launch_bounds__(SEL_THREADS) void ivf_merge_kernel(const IvfSel a, int runs) {
    extern __shared__ __align__(16) unsigned char sel_lds[];
    __shared__ unsigned tick[4];
    const int t = threadIdx.x, slot = blockIdx.x;
    Pool p;
    p.rec = reinterpret_cast<uint64_t *>(sel_lds);
    p.tick = tick; p.bound = ~0ull; p.fill = 0; p.P = a.P; p.nn = a.nn; p.step = 0u; p.compactions = 0u;
    if (t < 4) tick[t] = 0u;
    __syncthreads();
    for (int y = 0; y < runs; ++y) {
        const int64_t run = (int64_t)slot * runs + y;
        const uint64_t *__restrict__ src = a.part + run * a.nn;
        const int len = (int)a.pcount[run];                          // <= nn
        for (int i0 = 0; i0 < len; i0 += SEL_THREADS) {
            if (src[i0] >= p.bound) break;                           // (block-uniform: one address, a uniform bound)
            const int i = i0 + t;
            const bool live = i < len;
            const uint64_t rec = live ? src[i] : 0ull;
            pool_offer(p, rec, live && rec < p.bound);
        }
    }
    pool_hand_out(p, a.q0 + slot, a.dists, a.out_ids, a.idbits);
    if (t == 0 && p.compactions) atomicAdd(&a.stat[1], (unsigned long long)p.compactions);
}

}  // namespace

int lsq_ivfsel_pool_records(int nn) {
    int p = 256;
    while (p < nn) p <<= 1;
    return 2 * p;
}

int lsq_ivfsel_splits(int nqb, int nprobe) {
    // ivf_scan_kernel's rule: enough blocks to fill the chip a few times over when the queries are few
    const int splits = (2048 + nqb - 1) / nqb;
    return std::max(1, std::min(splits, nprobe));
}

size_t lsq_ivfsel_lds_bytes(int m, int packed, int nn) {
    return sizeof(float) * ((size_t)m * LSQ_H + (packed ? 256 : 0)) + sizeof(uint64_t) * (size_t)lsq_ivfsel_pool_records(nn);
}

int lsq_ivfsel_launch(hipStream_t s, const lsq_ivfsel_call &c, int q0, int nqb, int splits) {
    if (c.nn < 1 || c.nn > LSQ_IVF_SELECT_MAX_NN || c.m < 1 || c.m > LSQ_MAX_M || splits < 1 || splits > c.nprobe) {
        lsq_set_error("lsq_ivfsel_launch: nn=%d m=%d splits=%d nprobe=%d outside what the pool serves", c.nn, c.m, splits, c.nprobe);
        return LSQ_EINVAL;
    }
    IvfSel a{};
    a.LUT = c.LUT; a.QT = c.QT; a.codes = c.codes; a.norms = c.norms; a.ids = c.ids; a.off = c.off; a.probe = c.probe; a.coarse = c.coarse; a.lbits = c.lbits;
    a.q0 = q0; a.nprobe = c.nprobe; a.m = c.m; a.nn = c.nn; a.P = lsq_ivfsel_pool_records(c.nn); a.idbits = c.idbits; a.add = c.add;
    a.dists = c.dists; a.out_ids = c.out_ids; a.part = c.part; a.pcount = c.pcount; a.stat = c.stat;
    const bool packed = c.packed != 0;
    const int rowb = packed ? c.m + 1 : c.m;                         // bytes of a row: the dword loader takes whole words
    const size_t lds = lsq_ivfsel_lds_bytes(c.m, c.packed, c.nn);
    const dim3 grid((unsigned)nqb, (unsigned)splits), block(SEL_THREADS);
#define SEL_LAUNCH(MWV)                                                                                           \
    do {                                                                                                          \
        if (c.lbits) {                                                                                            \
            if (packed) hipLaunchKernelGGL((ivf_topk_kernel<MWV, true, true>), grid, block, lds, s, a);           \
            else hipLaunchKernelGGL((ivf_topk_kernel<MWV, false, true>), grid, block, lds, s, a);                 \
        } else if (packed) hipLaunchKernelGGL((ivf_topk_kernel<MWV, true, false>), grid, block, lds, s, a);       \
        else hipLaunchKernelGGL((ivf_topk_kernel<MWV, false, false>), grid, block, lds, s, a);                    \
    } while (0)
    if (rowb == 4) SEL_LAUNCH(1);
    else if (rowb == 8) SEL_LAUNCH(2);
    else if (rowb == 12) SEL_LAUNCH(3);
    else if (rowb == 16) SEL_LAUNCH(4);
    else SEL_LAUNCH(0);
#undef SEL_LAUNCH
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

int lsq_ivfsel_launch_merge(hipStream_t s, const lsq_ivfsel_call &c, int q0, int nqb, int splits) {
    IvfSel a{};
    a.q0 = q0; a.nn = c.nn; a.P = lsq_ivfsel_pool_records(c.nn); a.idbits = c.idbits;
    a.dists = c.dists; a.out_ids = c.out_ids; a.part = c.part; a.pcount = c.pcount; a.stat = c.stat;
    hipLaunchKernelGGL(ivf_merge_kernel, dim3((unsigned)nqb), dim3(SEL_THREADS), sizeof(uint64_t) * (size_t)a.P, s, a, splits);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}
