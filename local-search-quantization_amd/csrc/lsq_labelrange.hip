// lsq_labelrange.hip -- labelled range search on the resident index: every row within a radius, a row predicate PER QUERY (gfx950).
//
// CONTRACT (Identity LR).  Row r is a candidate of query q iff (label[r] & mask[q]) == want[q] -- or, with LSQ_LABEL_ANY, iff (label[r] & mask[q]) != 0 -- AND
// the filter in force (tombstones are one) allows r.  For every query lims, distances and ids equal, bit for bit, what lsq_index_range_search returns for that
// single query after lsq_index_set_filter(its candidates): lsq_range.hip's arithmetic (adc_scan_kernel's adds in its order, the norm last, the optional coarse
// add), dist <= r in IEEE, (dist, id) order, a CSR of exactly the answer's length.
//
// lsq_range.hip counts per QUERY and fills through one global cursor per query: its second walk reads every row again whatever the first one found.  Here the
// counts are kept per CELL, and one block owns a cell:
//   GEOMETRY, every row (IVF = false): 256 threads, a lane owns a ROW, the block owns QB QUERIES (4 at m <= 8, 2 above: the tables of a block stay within
//           32 KiB) and one range of LR_CELL rows: blockIdx.x the range, blockIdx.y the group of QB queries.  A step: a lane loads its row's code words, its
//           norm (or norm byte), its label and its filter bit ONCE -- the dword loader (MW > 0) or the byte loader -- and then, for each of the block's
//           queries: the predicate; where any lane of the wave passes (wave-uniform: a wave without a candidate issues no table gather) the query's table is
//           summed in adc_scan_kernel's order, the norm added last, and the distance compared with the query's radius.  No pool, no barrier inside the walk.
//   GEOMETRY, lists (IVF = true, QB = 1): label_topk_kernel's list walk -- one query per blockIdx.x, every gridDim.y-th probed list in rank order, the optional
//           one rounded coarse add -- with the label in LAYOUT order (lsq_label_layout).  Cell = (query, blockIdx.y).
//   COUNT   hits per query in registers, reduced over the wave by shuffles and over the block in LDS; the block STORES cnt[q][y] (it owns the cell: no global
//           atomic).  The pairs that passed predicate and filter go by one non-returning integer add per block.
//   PLAN    three small kernels: the sum of a query's cells, the exclusive scan of those sums (lims, int64), and per query the exclusive scan of its cells
//           on top of lims[q] (off[q][y], int64).  Only lims comes back to the host, which cuts the fill batches by lsq_range_check.h's rule.
//   FILL    a block whose cells are all empty (or whose queries lie outside the batch) returns before it stages a table.  Otherwise the same walk parks
//           records (lsq_adc_key(dist) << idbits | id) in the wave's staging list of the query (LDS; its length is wave-uniform and lives in a register) and a
//           flush claims a run of slots on the (block, query) cursor in LDS and writes out[off[q][y] - out_base + slot], every store guarded by the cell's count.
//   SORT    lsq_range.hip's segmented sort and hand-out, into the index's held result: lsq_index_range_fetch and the drop rules serve it unchanged.
// Atomics: integer adds in LDS, and one non-returning integer add per block and statistic.  No inline assembly.
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "lsq_internal.h"
#include "lsq_range_check.h"

#pragma clang fp contract(off)

namespace {

constexpr int LR_THREADS = 256, LR_WAVES = LR_THREADS / 64;
constexpr int LR_STAGE = 64;                         // staged records per (wave, query): a step adds at most 64
constexpr int LR_CELL = 4096;                        // rows of a cell of the every-row walk: a multiple of 256 (DESIGN 4.36 has the measurements)
constexpr int LR_CHUNK = 16384;                      // queries whose tables are resident together (m KiB each)
enum { LR_COUNT = 0, LR_FILL = 1 };
enum { LR_STAT_PAIRS = 0, LR_STAT_SKIPPED = 1, LR_STAT_NONEMPTY = 2, LR_STATS = 3 };
static_assert(LR_CELL % LR_THREADS == 0 && LR_CELL <= 8192, "a cell is whole steps of the block and at most 8192 rows");

// what both passes are launched with.  Slots count the queries of the resident chunk: radius, qmask, qwant, cnt and offs point at the chunk's first query
struct LabelRange {
    const float *LUT; int QT;                        // adc_lut_kernel's tiles of the chunk
    const uint8_t *codes; const float *norms;        // the rows of the walk: the index's flat arrays, or the inverted layout (norms: per row, or (packed) the table)
    const int *ids; const int *off;                  // IVF: the layout's original ids and list offsets
    const int *probe; const float *coarse;           // IVF: [slot][nprobe] the probed lists in rank order and their coarse distances
    const uint32_t *labels;                          // the label of the row at a position of the walk (original order; IVF: layout order)
    const uint32_t *bits;                            // FILT: the filter's bits by position of the walk
    const uint32_t *qmask; const uint32_t *qwant;    // [slot]
    const float *radius;                             // [slot]
    unsigned *cnt;                                   // [slot][cells]: COUNT writes, FILL reads
    const int64_t *offs;                             // FILL: [slot][cells] the cell's first entry in the result
    uint64_t *out; int64_t out_base;                 // FILL: record r of a cell goes to out[offs[slot][y] - out_base + r]
    unsigned long long *stat;                        // [LR_STATS]
    int qa, qb, s0;                                  // the slots that take part: qa <= slot < qb (COUNT: the whole chunk; FILL: the batch); s0: the first block's first slot
    int n, nprobe, m, idbits, add, any;
    int64_t cells;                                   // cells per query
    int per;                                         // every row: rows of a cell
};

template <int MW, bool PACKED, bool FILT, int QB, bool IVF, int PASS>
__global__ __launch_bounds__(LR_THREADS) void label_range_kernel(const LabelRange a) {
    extern __shared__ __align__(16) unsigned char lr_lds[];          // [QB][entries] tables; PACKED: the norm table; FILL: [waves][QB][LR_STAGE] records
    __shared__ unsigned cell[QB];                                    // COUNT: the block's hits per query; FILL: the slots of the cell handed out so far
    __shared__ unsigned long long bpairs;
    constexpr int NT = PACKED ? 4 * MW - 1 : 4 * MW;                 // bytes of a dword-loaded row that index tables
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int slot0 = a.s0 + (IVF ? (int)blockIdx.x : (int)blockIdx.y * QB);
    const int64_t y = IVF ? (int64_t)blockIdx.y : (int64_t)blockIdx.x;
    const int entries = a.m * LSQ_H;
    float *lut = reinterpret_cast<float *>(lr_lds);
    float *ntab = lut + QB * entries;
    uint64_t *stage = reinterpret_cast<uint64_t *>(ntab + (PACKED ? 256 : 0)) + (size_t)wave * QB * LR_STAGE;
    // a query takes part iff its slot lies in the launch's window and (FILL) its cell holds a result.  One that does not gets a predicate no label passes
    // and a NaN radius
    bool on[QB];
    uint32_t qm[QB], qw[QB];
    float rad[QB];
    unsigned have[QB];                                               // FILL: the cell's count
    int64_t base[QB];                                                // FILL: the cell's first record in out
    bool any_on = false;
#pragma unroll
    for (int i = 0; i < QB; ++i) {
        const int slot = slot0 + i;
        on[i] = slot >= a.qa && slot < a.qb;
        have[i] = 0u; base[i] = 0;
        if (PASS == LR_FILL && on[i]) {
            have[i] = a.cnt[(int64_t)slot * a.cells + y];
            base[i] = a.offs[(int64_t)slot * a.cells + y] - a.out_base;
            on[i] = have[i] != 0u;
        }
        qm[i] = on[i] ? a.qmask[slot] : 0u;
        qw[i] = on[i] ? a.qwant[slot] : 1u;
        rad[i] = on[i] ? a.radius[slot] : __uint_as_float(0x7fc00000u);
        any_on = any_on || on[i];
    }
    if (PASS == LR_FILL && !any_on) {                                // (block-uniform) nothing to write: no table is staged
        if (t == 0) atomicAdd(&a.stat[LR_STAT_SKIPPED], 1ull);
        return;
    }
    if constexpr (QB > 1) {
        // the block's QB slots are neighbours in one tile (QB divides QT, slot0 is a multiple of QB): an entry of all of them is ONE aligned vector load
        typedef float fvec __attribute__((ext_vector_type(QB)));
        const fvec *__restrict__ src = reinterpret_cast<const fvec *>(a.LUT + (int64_t)(slot0 / a.QT) * entries * a.QT + slot0 % a.QT);
        const int pitch = a.QT / QB;
        for (int e = t; e < entries; e += LR_THREADS) {
            const fvec v = src[(int64_t)e * pitch];
#pragma unroll
            for (int i = 0; i < QB; ++i)
                if (on[i]) lut[i * entries + e] = v[i];              // (block-uniform)
        }
    } else {
        if (on[0]) {                                                 // (block-uniform)
            const float *__restrict__ src = a.LUT + (int64_t)(slot0 / a.QT) * entries * a.QT + slot0 % a.QT;
            for (int e = t; e < entries; e += LR_THREADS) lut[e] = src[(int64_t)e * a.QT];
        }
    }
    if constexpr (PACKED) ntab[t] = a.norms[t];                      // (LR_THREADS == 256 entries)
    if (t < QB) cell[t] = 0u;
    if (t == 0) bpairs = 0ull;
    __syncthreads();
    unsigned cnt[QB], pairs = 0;                                     // COUNT: this lane's hits per query, and its pairs that passed predicate and filter
    int sn[QB];                                                      // FILL: records parked in the wave's list of query i (wave-uniform)
#pragma unroll
    for (int i = 0; i < QB; ++i) { cnt[i] = 0u; sn[i] = 0; }
    // FILL: the wave's parked records of query i leave: one run of slots on the cell's cursor (an LDS add), then the stores, each guarded by the cell's count
    auto flush = [&](int i) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        unsigned b = 0u;
        if (lane == 0) b = atomicAdd(&cell[i], (unsigned)sn[i]);
        b = __shfl(b, 0, 64);
        const unsigned at = b + (unsigned)lane;
        if (lane < sn[i] && at < have[i]) a.out[base[i] + (int64_t)at] = stage[i * LR_STAGE + lane];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        sn[i] = 0;
    };
    // one step of the walk: this lane's row (a dead lane reads a row that exists and offers nothing); cq: the list's coarse distance
    auto step = [&](int64_t row, bool live, float cq) {
        uint32_t w[MW > 0 ? MW : 1];
        (void)w;
        const uint8_t *cp = a.codes + row * (MW > 0 ? 4 * MW : (PACKED ? a.m + 1 : a.m));
        if constexpr (MW > 0) {
#pragma unroll
            for (int k = 0; k < MW; ++k) w[k] = reinterpret_cast<const uint32_t *>(cp)[k];
        }
        float nrm = 0.0f;
        if constexpr (!PACKED) nrm = a.norms[row];
        const uint32_t lab = a.labels[row];
        bool ok = live;
        if constexpr (FILT) ok = live && ((a.bits[row >> 5] >> (row & 31)) & 1u) != 0;
        int id = (int)row;                                           // the ORIGINAL id, 1-based below
        if constexpr (IVF) id = a.ids[row];
#pragma unroll
        for (int i = 0; i < QB; ++i) {
            if (!on[i]) continue;                                    // (block-uniform)
            const uint32_t v = lab & qm[i];
            const bool pass = ok && (a.any ? v != 0u : v == qw[i]);
            if (!__ballot(pass)) continue;                           // (wave-uniform) a wave without a candidate gathers nothing
            const float *tab = lut + i * entries;
            float acc = 0.0f;
            if constexpr (MW > 0) {
#pragma unroll
                for (int j = 0; j < NT; ++j) acc = acc + tab[j * LSQ_H + (int)((w[j >> 2] >> (8 * (j & 3))) & 0xffu)];
                if constexpr (PACKED) nrm = ntab[(int)(w[MW > 0 ? MW - 1 : 0] >> 24)];
            } else {
                for (int j = 0; j < a.m; ++j) acc = acc + tab[j * LSQ_H + (int)cp[j]];
                if constexpr (PACKED) nrm = ntab[(int)cp[a.m]];
            }
            float dist = acc + nrm;
            if constexpr (IVF) { if (a.add) dist = dist + cq; }      // one more rounded add
            const bool hit = pass && dist <= rad[i];                 // IEEE: a NaN on either side is out
            if constexpr (PASS == LR_COUNT) {
                cnt[i] += hit ? 1u : 0u;
                pairs += pass ? 1u : 0u;
            } else {
                const unsigned long long hm = __ballot(hit);
                if (!hm) continue;                                   // (wave-uniform)
                const int k = __popcll(hm);
                if (sn[i] + k > LR_STAGE) flush(i);
                if (hit) {
                    const int pos = sn[i] + __popcll(hm & ((1ull << lane) - 1ull));
                    stage[i * LR_STAGE + pos] = ((uint64_t)lsq_adc_key(dist) << a.idbits) | (uint64_t)(uint32_t)(id + 1);
                }
                sn[i] += k;
            }
        }
    };
    if constexpr (!IVF) {
        const int64_t first = y * a.per;                             // (< n: the grid has ceil(n / per) ranges)
        const int64_t last = first + a.per < (int64_t)a.n ? first + a.per : (int64_t)a.n;
        for (int64_t r0 = first; r0 < last; r0 += LR_THREADS) {
            const bool live = r0 + t < last;
            step(live ? r0 + t : first, live, 0.0f);
        }
    } else {
        const int *__restrict__ probe = a.probe + (int64_t)slot0 * a.nprobe;
        for (int r = (int)blockIdx.y; r < a.nprobe; r += (int)gridDim.y) {
            const int l = probe[r];
            const int b = a.off[l], len = a.off[l + 1] - b;
            const float cq = a.add ? a.coarse[(int64_t)slot0 * a.nprobe + r] : 0.0f;
            for (int i0 = 0; i0 < len; i0 += LR_THREADS) {           // (len >= 1 inside: row b exists)
                const bool live = i0 + t < len;
                step((int64_t)b + (live ? i0 + t : 0), live, cq);
            }
        }
    }
    if constexpr (PASS == LR_FILL) {
#pragma unroll
        for (int i = 0; i < QB; ++i)
            if (sn[i] > 0) flush(i);                                 // (wave-uniform)
    } else {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int i = 0; i < QB; ++i) cnt[i] += __shfl_xor(cnt[i], off, 64);
            pairs += __shfl_xor(pairs, off, 64);
        }
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < QB; ++i)
                if (cnt[i]) atomicAdd(&cell[i], cnt[i]);
            if (pairs) atomicAdd(&bpairs, (unsigned long long)pairs);
        }
        __syncthreads();
        if (t < QB && slot0 + t >= a.qa && slot0 + t < a.qb) a.cnt[(int64_t)(slot0 + t) * a.cells + y] = cell[t];      // the block owns the cell: a plain store
        if (t == 0 && bpairs) atomicAdd(&a.stat[LR_STAT_PAIRS], bpairs);      // (the value is not used: no round trip)
    }
}

// ---- PLAN: the cells' counts -> lims and every cell's offset, on the device ---------------------------------------------------------------------------------
// the exclusive prefix of one value per thread of a block of 256 (*total: the block's sum); wsum: LR_WAVES + 1 words of LDS.  Two barriers
__device__ inline int64_t block_exclusive(int64_t v, int64_t *wsum, int64_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t up = __shfl_up(inc, off, 64);
        if (lane >= off) inc += up;
    }
    __syncthreads();                                                 // (the former round's reads of wsum are over)
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int64_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < LR_WAVES; ++k) {
        if (k < wave) before += wsum[k];
        all += wsum[k];
    }
    *total = all;
    return before + inc - v;
}

// tot[q] = the sum of query q's cells; *nonempty += its cells that hold a result.  One block per query
__global__ __launch_bounds__(LR_THREADS) void label_range_sum_kernel(const unsigned *__restrict__ cnt, int64_t cells, int64_t *__restrict__ tot,
                                                                      unsigned long long *nonempty) {
    __shared__ int64_t wsum[2 * LR_WAVES];
    const unsigned *__restrict__ row = cnt + (int64_t)blockIdx.x * cells;
    int64_t sum = 0, full = 0;
    for (int64_t c = threadIdx.x; c < cells; c += LR_THREADS) { sum += (int64_t)row[c]; full += row[c] ? 1 : 0; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { sum += __shfl_xor(sum, off, 64); full += __shfl_xor(full, off, 64); }
    if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6] = sum; wsum[LR_WAVES + (threadIdx.x >> 6)] = full; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t s = 0, f = 0;
        for (int k = 0; k < LR_WAVES; ++k) { s += wsum[k]; f += wsum[LR_WAVES + k]; }
        tot[blockIdx.x] = s;
        if (f) atomicAdd(nonempty, (unsigned long long)f);
    }
}

// lims[0] = 0, lims[q + 1] = lims[q] + tot[q]: one block walks the queries 256 at a time and carries the sum
__global__ __launch_bounds__(LR_THREADS) void label_range_lims_kernel(const int64_t *__restrict__ tot, int nq, int64_t *__restrict__ lims) {
    __shared__ int64_t wsum[LR_WAVES];
    int64_t carry = 0;
    for (int q0 = 0; q0 < nq; q0 += LR_THREADS) {                    // (block-uniform trip count)
        const int q = q0 + (int)threadIdx.x;
        int64_t total;
        const int64_t before = block_exclusive(q < nq ? tot[q] : 0, wsum, &total);
        if (q < nq) lims[q] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) lims[nq] = carry;
}

// offs[q][y] = lims[q] + the cells of q before y.  One block per query
__global__ __launch_bounds__(LR_THREADS) void label_range_offsets_kernel(const unsigned *__restrict__ cnt, int64_t cells, const int64_t *__restrict__ lims,
                                                                          int64_t *__restrict__ offs) {
    __shared__ int64_t wsum[LR_WAVES];
    const unsigned *__restrict__ row = cnt + (int64_t)blockIdx.x * cells;
    int64_t *__restrict__ dst = offs + (int64_t)blockIdx.x * cells;
    int64_t carry = lims[blockIdx.x];
    for (int64_t c0 = 0; c0 < cells; c0 += LR_THREADS) {             // (block-uniform trip count)
        const int64_t c = c0 + threadIdx.x;
        int64_t total;
        const int64_t before = block_exclusive(c < cells ? (int64_t)row[c] : 0, wsum, &total);
        if (c < cells) dst[c] = carry + before;
        carry += total;
    }
}

// the statistics' words are cleared by a kernel (a memset node has no place in a captured stream)
__global__ void label_range_clear_kernel(unsigned long long *stat) {
    if (threadIdx.x < LR_STATS) stat[threadIdx.x] = 0ull;
}

// ---- the launch ------------------------------------------------------------------------------------------------------------------------------------------
inline int labelrange_qb(int m) { return m <= 8 ? 4 : 2; }           // the block's tables stay within 32 KiB

inline size_t labelrange_lds(int m, bool packed, int qb, int pass) {
    return sizeof(float) * ((size_t)qb * m * LSQ_H + (packed ? 256 : 0)) + (pass == LR_FILL ? sizeof(uint64_t) * (size_t)LR_WAVES * qb * LR_STAGE : 0);
}

template <int MW, bool PACKED, bool FILT, int PASS>
int launch_geometry(hipStream_t s, const LabelRange &a, bool ivf, int qb, dim3 grid) {
    const size_t lds = labelrange_lds(a.m, PACKED, ivf ? 1 : qb, PASS);
#define LR_GO(QBV, IVFV)                                                                                                                 \
    do {                                                                                                                                \
        LSQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&label_range_kernel<MW, PACKED, FILT, QBV, IVFV, PASS>),             \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                                             \
        hipLaunchKernelGGL((label_range_kernel<MW, PACKED, FILT, QBV, IVFV, PASS>), grid, dim3(LR_THREADS), lds, s, a);                 \
    } while (0)
    if (ivf) LR_GO(1, true);
    else if (qb == 4) LR_GO(4, false);
    else LR_GO(2, false);
#undef LR_GO
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

template <int MW, int PASS>
int launch_rows(hipStream_t s, const LabelRange &a, bool packed, bool ivf, int qb, dim3 grid) {
    if (a.bits) return packed ? launch_geometry<MW, true, true, PASS>(s, a, ivf, qb, grid) : launch_geometry<MW, false, true, PASS>(s, a, ivf, qb, grid);
    return packed ? launch_geometry<MW, true, false, PASS>(s, a, ivf, qb, grid) : launch_geometry<MW, false, false, PASS>(s, a, ivf, qb, grid);
}

// one pass over the slots qa .. qb - 1 of the resident chunk; *blocks += the blocks launched
template <int PASS>
int launch_pass(hipStream_t s, LabelRange a, bool packed, bool ivf, int qa, int qb, int64_t *blocks) {
    if (qb <= qa) return LSQ_OK;
    const int QB = ivf ? 1 : labelrange_qb(a.m);
    const int rowb = packed ? a.m + 1 : a.m;                         // bytes of a row: the dword loader takes whole, aligned words
    const bool words = rowb % 4 == 0 && ((uintptr_t)a.codes & 3) == 0;
    a.qa = qa; a.qb = qb;
    a.s0 = qa / QB * QB;                                             // the grid's first group is the one that holds slot qa
    const int groups = (qb - a.s0 + QB - 1) / QB;
    const dim3 grid = ivf ? dim3((unsigned)groups, (unsigned)a.cells) : dim3((unsigned)a.cells, (unsigned)groups);
    *blocks += (int64_t)groups * a.cells;
    if (words && rowb == 4) return launch_rows<1, PASS>(s, a, packed, ivf, QB, grid);
    if (words && rowb == 8) return launch_rows<2, PASS>(s, a, packed, ivf, QB, grid);
    if (words && rowb == 12) return launch_rows<3, PASS>(s, a, packed, ivf, QB, grid);
    if (words && rowb == 16) return launch_rows<4, PASS>(s, a, packed, ivf, QB, grid);
    return launch_rows<0, PASS>(s, a, packed, ivf, QB, grid);
}

}  // namespace

struct lsq_labelrange_state {
    DevBuf qmask, qwant, lut, cnt, offs, tot, stat;
    PhaseClock<2> clock;
    lsq_label_range_info info{};
};

void lsq_labelrange_free(lsq_labelrange_state *st) {
    if (!st) return;
    DevBuf *all[] = {&st->qmask, &st->qwant, &st->lut, &st->cnt, &st->offs, &st->tot, &st->stat};
    for (DevBuf *b : all) b->release();
    st->clock.release();
    delete st;
}

void lsq_labelrange_get_info(const lsq_labelrange_state *st, lsq_label_range_info *out) { *out = st ? st->info : lsq_label_range_info{}; }

// rows of a cell of the every-row walk
static int labelrange_cell() {
#ifdef LSQ_TUNING
    // the tuning library's knob: LSQ_LABELRANGE_CELL = a multiple of 256 in 256 .. 8192 (read at every call, so that one process can alternate the lengths): the
    // constant was chosen against it (tools/label_range_bench.py n nq cells)
    if (const char *e = getenv("LSQ_LABELRANGE_CELL")) return std::max(256, std::min(8192, atoi(e) / 256 * 256));
#endif
    return LR_CELL;
}

// cells per query: the ranges of LR_CELL rows, or (lists) the blocks that share a query's probed lists (lsq_ivfsel_splits over the first chunk's queries)
int64_t lsq_labelrange_cells(int64_t n, int nq, int nprobe) {
    if (nprobe >= 1) return lsq_ivfsel_splits(std::max(1, std::min(nq, LR_CHUNK)), nprobe);
    return std::max<int64_t>(1, (n + labelrange_cell() - 1) / labelrange_cell());
}

int lsq_labelrange_search(hipStream_t s, lsq_range_state **prange, lsq_labelrange_state **pst, const lsq_labelrange_call &call, int64_t *h_lims) {
    if (!*prange) *prange = new lsq_range_state();
    if (!*pst) *pst = new lsq_labelrange_state();
    lsq_range_state *rs = *prange;
    lsq_labelrange_state *st = *pst;
    const lsq_range_call &rc = call.rc;
    lsq_range_drop(rs);                              // the former result leaves whatever becomes of this call
    rs->info = lsq_range_info{};
    rs->info.road = rc.road;
    st->info = lsq_label_range_info{};
    const int nq = rc.nq;
    const bool ivf = rc.nprobe >= 1, timed = rc.timed != 0;
    const lsq_search_input &in = rc.in;
    const int m = in.m, d = in.d, QT = lsq_adc_lut_qt(m), QB = ivf ? 1 : labelrange_qb(m);
    const int64_t cells = lsq_labelrange_cells(in.n, nq, rc.nprobe);
    h_lims[0] = 0;
    st->info.queries = nq; st->info.queries_per_block = QB; st->info.cells_per_query = cells; st->info.rows_per_cell = ivf ? 0 : labelrange_cell();
    st->info.cells = (int64_t)nq * cells;
    // one phase of a profiled call: the time between two marks, added to *ms (a wait; nothing without option "profile")
    auto lap_begin = [&]() -> int { LSQ_TRY(st->clock.begin(timed)); return st->clock.mark(s); };
    auto lap_end = [&](double *ms) -> int {
        LSQ_TRY(st->clock.mark(s));
        float t[1];
        LSQ_TRY(st->clock.read(t));
        *ms += t[0];
        return LSQ_OK;
    };
    if (nq > 0) {
        // chunks of queries whose tables are resident together and, on the list road, whose per-(query, probe) words stay below 2^28 (lsq_range_search's rule);
        // whole tiles, so that a chunk's slots start a tile
        int64_t qc = LR_CHUNK;
        if (ivf) qc = std::min<int64_t>(qc, std::max<int64_t>(QT, ((int64_t)(1u << 28) / ((int64_t)rc.nprobe + 1)) / QT * QT));
        const int nchunks = (int)((nq + qc - 1) / qc);
        const size_t slots_max = (size_t)((std::min<int64_t>(qc, nq) + QT - 1) / QT) * QT;
        const size_t ncells = (size_t)nq * (size_t)cells;
        LSQ_TRY(st->lut.ensure(sizeof(float) * slots_max * m * LSQ_H));
        LSQ_TRY(st->qmask.ensure(sizeof(uint32_t) * (size_t)nq));
        LSQ_TRY(st->qwant.ensure(sizeof(uint32_t) * (size_t)nq));
        LSQ_TRY(st->cnt.ensure(sizeof(unsigned) * ncells));
        LSQ_TRY(st->offs.ensure(sizeof(int64_t) * ncells));
        LSQ_TRY(st->tot.ensure(sizeof(int64_t) * (size_t)nq));
        LSQ_TRY(st->stat.ensure(sizeof(unsigned long long) * LR_STATS));
        LSQ_TRY(rs->lims.ensure(sizeof(int64_t) * ((size_t)nq + 1)));
        LSQ_HIP(hipMemcpyAsync(st->qmask.p, call.q_mask, sizeof(uint32_t) * (size_t)nq, hipMemcpyDefault, s));
        LSQ_HIP(hipMemcpyAsync(st->qwant.p, call.q_want, sizeof(uint32_t) * (size_t)nq, hipMemcpyDefault, s));
        hipLaunchKernelGGL(label_range_clear_kernel, dim3(1), dim3(64), 0, s, st->stat.as<unsigned long long>());
        LSQ_HIP(hipGetLastError());
        lsq_ivf_probes pv{};
        const int idbits = lsq_adc_idbits(in.n);
        bool packed = in.packed != 0;
        const uint32_t *labels = call.labels;
        // a chunk's set-up: the probed lists (list road) and the tables
        auto prepare = [&](int64_t c0, int nqc) -> int {
            if (ivf) {
                double ms = 0.0;
                LSQ_TRY(lsq_ivf_coarse(s, rc.ivf, rc.adc, rc.q_coarse + c0 * rc.ldc, rc.ldc, nqc, rc.nprobe, rc.coarse, rc.timed, &pv, &ms));
                st->info.coarse_ms += ms;
                packed = pv.packed != 0;
                LSQ_TRY(lsq_label_layout(s, call.lab, pv.ids, pv.n, &labels));      // the labels where the list walk reads the codes
            }
            lsq_search_input li = in;
            li.Q = static_cast<const float *>(in.Q) + c0 * d;
            LSQ_TRY(lap_begin());
            LSQ_TRY(lsq_adc_launch_lut(s, li, nullptr, 0, nqc, st->lut.as<float>()));
            return lap_end(&st->info.lut_ms);
        };
        auto args = [&](int64_t c0) {
            LabelRange a{};
            a.LUT = st->lut.as<float>(); a.QT = QT; a.labels = labels; a.bits = call.bits;
            if (ivf) {
                a.codes = pv.codes; a.norms = pv.norms; a.ids = pv.ids; a.off = pv.off; a.probe = pv.probe; a.coarse = pv.coarse;
            } else {
                a.codes = in.codes; a.norms = in.dbnorms;
            }
            a.qmask = st->qmask.as<uint32_t>() + c0; a.qwant = st->qwant.as<uint32_t>() + c0; a.radius = rc.radius + c0;
            a.cnt = st->cnt.as<unsigned>() + c0 * cells; a.offs = st->offs.as<int64_t>() + c0 * cells;
            a.stat = st->stat.as<unsigned long long>();
            a.n = in.n; a.nprobe = rc.nprobe; a.m = m; a.idbits = idbits; a.add = (rc.flags & LSQ_IVF_ADD_COARSE) ? 1 : 0; a.any = call.any;
            a.cells = cells; a.per = labelrange_cell();
            return a;
        };
        // ---- COUNT
        int64_t count_blocks = 0;
        for (int ch = 0; ch < nchunks; ++ch) {
            const int64_t c0 = (int64_t)ch * qc;
            const int nqc = (int)std::min<int64_t>(qc, nq - c0);
            LSQ_TRY(prepare(c0, nqc));
            LSQ_TRY(lap_begin());
            LSQ_TRY(launch_pass<LR_COUNT>(s, args(c0), packed, ivf, 0, nqc, &count_blocks));
            LSQ_TRY(lap_end(&st->info.count_ms));
        }
        // ---- PLAN: on the device; lims alone comes back
        LSQ_TRY(lap_begin());
        hipLaunchKernelGGL(label_range_sum_kernel, dim3((unsigned)nq), dim3(LR_THREADS), 0, s, st->cnt.as<unsigned>(), cells, st->tot.as<int64_t>(),
                           st->stat.as<unsigned long long>() + LR_STAT_NONEMPTY);
        hipLaunchKernelGGL(label_range_lims_kernel, dim3(1), dim3(LR_THREADS), 0, s, st->tot.as<int64_t>(), nq, rs->lims.as<int64_t>());
        hipLaunchKernelGGL(label_range_offsets_kernel, dim3((unsigned)nq), dim3(LR_THREADS), 0, s, st->cnt.as<unsigned>(), cells, rs->lims.as<int64_t>(),
                           st->offs.as<int64_t>());
        LSQ_HIP(hipGetLastError());
        LSQ_TRY(lap_end(&st->info.plan_ms));
        LSQ_HIP(hipMemcpyAsync(h_lims, rs->lims.p, sizeof(int64_t) * ((size_t)nq + 1), hipMemcpyDeviceToHost, s));
        LSQ_HIP(hipStreamSynchronize(s));
        const int64_t total = h_lims[nq];
        for (int q = 0; q < nq; ++q) rs->info.max_per_query = std::max(rs->info.max_per_query, h_lims[q + 1] - h_lims[q]);
        if (total > 0) {
            LSQ_TRY(rs->held_d.ensure(sizeof(float) * (size_t)total));
            LSQ_TRY(rs->held_i.ensure(sizeof(int) * (size_t)total));
        }
        // ---- FILL, SORT, hand-out: batch by batch
        std::vector<int64_t> cuts;
        for (int ch = 0; ch < nchunks && total > 0; ++ch) {
            const int64_t c0 = (int64_t)ch * qc;
            const int nqc = (int)std::min<int64_t>(qc, nq - c0);
            if (h_lims[c0 + nqc] == h_lims[c0]) continue;            // nothing within the radius of any query of the chunk
            if (nchunks > 1) LSQ_TRY(prepare(c0, nqc));              // (one chunk: its tables and probed lists are still there)
            lsq_range_cut(h_lims, c0, c0 + nqc, rc.budget, &cuts);
            for (size_t b = 0; b + 1 < cuts.size(); ++b) {
                const int64_t qa = cuts[b], qb = cuts[b + 1], out_base = h_lims[qa], records = h_lims[qb] - out_base;
                if (records == 0) continue;
                if (records > (int64_t)INT32_MAX) { lsq_set_error("lsq_index_range_search_labelled: a batch of %lld records exceeds 2^31 - 1", (long long)records); return LSQ_EINVAL; }
                LSQ_TRY(rs->rec_a.ensure(sizeof(uint64_t) * (size_t)records));
                LSQ_TRY(rs->rec_b.ensure(sizeof(uint64_t) * (size_t)records));
                LSQ_TRY(lap_begin());
                LabelRange a = args(c0);
                a.out = rs->rec_a.as<uint64_t>(); a.out_base = out_base;
                LSQ_TRY(launch_pass<LR_FILL>(s, a, packed, ivf, (int)(qa - c0), (int)(qb - c0), &st->info.fill_blocks_launched));
                LSQ_TRY(lap_end(&st->info.fill_ms));
                LSQ_TRY(lap_begin());
                LSQ_TRY(lsq_range_select_batch(rs, s, (int)qa, (int)qb, out_base, records, idbits));
                LSQ_TRY(lap_end(&st->info.sort_ms));
                st->info.batches += 1;
            }
        }
        unsigned long long stat[LR_STATS] = {0, 0, 0};
        LSQ_HIP(hipMemcpyAsync(stat, st->stat.p, sizeof(stat), hipMemcpyDeviceToHost, s));
        if (rc.lims_dev) LSQ_HIP(hipMemcpyAsync(rc.lims_dev, rs->lims.p, sizeof(int64_t) * ((size_t)nq + 1), hipMemcpyDeviceToDevice, s));
        LSQ_HIP(hipStreamSynchronize(s));
        st->info.allowed_pairs = (int64_t)stat[LR_STAT_PAIRS]; st->info.fill_blocks_skipped = (int64_t)stat[LR_STAT_SKIPPED];
        st->info.cells_nonempty = (int64_t)stat[LR_STAT_NONEMPTY];
    } else if (rc.lims_dev) {
        LSQ_HIP(hipMemcpyAsync(rc.lims_dev, h_lims, sizeof(int64_t), hipMemcpyHostToDevice, s));
        LSQ_HIP(hipStreamSynchronize(s));
    }
    rs->held = true;
    rs->held_total = h_lims[nq];
    st->info.results = rs->held_total;
    rs->info.queries = nq; rs->info.results = rs->held_total; rs->info.batches = st->info.batches; rs->info.rows_walked = st->info.allowed_pairs;
    rs->info.held_bytes = (int64_t)(rs->held_d.cap + rs->held_i.cap);
    rs->info.coarse_ms = st->info.coarse_ms; rs->info.lut_ms = st->info.lut_ms; rs->info.count_ms = st->info.count_ms; rs->info.fill_ms = st->info.fill_ms;
    rs->info.sort_ms = st->info.sort_ms;
    return LSQ_OK;
}
