// lsq_label.hip -- labelled search on the resident index: a row predicate PER QUERY, tested inside a scan that selects in LDS (gfx950).
//
// CONTRACT (Identity L).  The index holds one 32-bit label per row.  Query q carries (mask, want); row r is a candidate iff (label[r] & mask) == want -- or,
// with LSQ_LABEL_ANY, iff (label[r] & mask) != 0 -- AND the index's filter in force (lsq_filter.hip; tombstones are one) allows r.  The result row of q is, bit
// for bit, what lsq_index_search / _search_ivf returns for that single query after lsq_index_set_filter(that candidate set): the full ranking with the other
// rows removed, cut to nn, (+inf, 0) behind it.
//
// lsq_adc.hip's selection estimates ONE threshold per query from a sample of the rows and redoes the queries whose list overflows: with a different number of
// allowed rows per query there is no sample to estimate from.  The pool of lsq_pool.h needs none: records (lsq_adc_key(dist) << idbits | id + 1) are distinct
// per row, the nn smallest are a set, every query is answered in one pass.
//
//   GEOMETRY, exhaustive (IVF = false): 256 threads, a lane owns a ROW, the block owns QB QUERIES: QB in {4, 2, 1}, the largest with
//           QB (m KiB of table + 8 P bytes of pool [+ 1 KiB of norm table, packed]) <= 64 KiB (lsq_label_qb: 4 at m = 8 and nn <= 512 -- packed: nn <= 256 --, 2 at m = 16,
//           1 from nn = 1025 on).  blockIdx.x: the group of QB queries (the last group of a batch may hold fewer), blockIdx.y: one of `splits` contiguous row ranges cut
//           at multiples of 256 rows (lsq_label_split).  A step: a lane loads its row's code words, its norm (or norm byte), its label and its filter bit ONCE
//           -- the dword loader (MW > 0) or the byte loader -- and then, for each of the block's queries: the predicate; where any lane of the wave passes
//           (wave-uniform: a wave without a candidate issues no table gather) the query's table is summed in adc_scan_kernel's order, the norm added last, the
//           record formed; a lane that passes and whose record is < the pool's bound takes a slot (pool_place).  ONE barrier serves the QB pools of the step;
//           behind it each pool takes up its count and is compacted when fewer than 256 slots are free (pool_settle: block-uniform per pool).  What QB buys:
//           the rows are read once per QB queries.
//   GEOMETRY, lists (IVF = true, QB = 1): ivf_topk_kernel's walk -- one query per blockIdx.x, every gridDim.y-th probed list in rank order, the optional one
//           rounded coarse add -- with the label in LAYOUT order (label_layout_kernel: lab[p] = labels[ids[p]]) read where the code is read.
//   FINISH  gridDim.y == 1: pool_hand_out per query.  gridDim.y > 1: every block writes its <= nn sorted records per query as a run and ivf_merge_kernel
//           (lsq_ivfsel.hip: its argument struct fits) streams a query's runs through pool_offer.
// Atomics: integer adds in LDS, and one non-returning integer add per block and statistic (sums of integers: the same on every call).  No inline assembly.
#include <algorithm>
#include <vector>

#include "lsq_internal.h"
#include "lsq_pool.h"

#pragma clang fp contract(off)

namespace {

struct LabelScan {
    const float *LUT; int QT;                        // adc_lut_kernel's tiles of this batch
    const uint8_t *codes; const float *norms;        // the rows of the walk: the index's flat arrays, or the inverted layout (norms: per row, or (packed) the table)
    const int *ids; const int *off;                  // IVF: the layout's original ids and list offsets
    const int *probe; const float *coarse;           // IVF: [.][nprobe] the probed lists in rank order and their coarse distances
    const uint32_t *labels;                          // the label of the row at a position of the walk (original order; IVF: layout order)
    const uint32_t *bits;                            // FILT: the filter's bits by position of the walk
    const uint32_t *qmask; const uint32_t *qwant;    // [.] by query of the chunk
    int q0, nqb, n, nprobe, m, nn, P, idbits, add, any;           // the query of a slot is q0 + slot
    int64_t per;                                     // exhaustive: rows of a range
    float *dists; int *out_ids;                      // [.][nn]: the caller's rows
    uint64_t *part; unsigned *pcount;                // gridDim.y > 1: the runs [slot][y][nn] and their lengths [slot][y]
    unsigned long long *stat;                        // [0] += records that entered pools, [1] += compactions, [2] += (row, query) pairs that passed both tests
};

template <int MW, bool PACKED, bool FILT, int QB, bool IVF>
__global__ __launch_bounds__(SEL_THREADS) void label_topk_kernel(const LabelScan a) {
    extern __shared__ __align__(16) unsigned char lab_lds[];
    __shared__ unsigned tick[3 * QB];                                // pool i's three step counters at [3 i ..]
    __shared__ unsigned long long bstat[2];                          // the block's records placed and pairs passed (64-bit: one range of 2^31 rows x QB queries fits)
    constexpr int NT = PACKED ? 4 * MW - 1 : 4 * MW;                 // bytes of a dword-loaded row that index tables
    const int t = threadIdx.x, lane = t & 63;
    const int slot0 = (int)blockIdx.x * QB;
    const int nqg = a.nqb - slot0 < QB ? a.nqb - slot0 : QB;         // queries of this group (block-uniform, >= 1)
    const int entries = a.m * LSQ_H;
    float *lut = reinterpret_cast<float *>(lab_lds);                 // [QB][entries]; PACKED: the norm table behind them; then the QB pools
    float *ntab = lut + QB * entries;
    uint64_t *recs = reinterpret_cast<uint64_t *>(ntab + (PACKED ? 256 : 0));
    Pool p[QB];
    uint32_t qm[QB], qw[QB];
#pragma unroll
    for (int i = 0; i < QB; ++i) {
        p[i].rec = recs + (size_t)i * a.P; p[i].tick = tick + 3 * i;
        p[i].bound = ~0ull; p[i].fill = 0; p[i].P = a.P; p[i].nn = a.nn; p[i].step = 0u; p[i].compactions = 0u;
        qm[i] = qw[i] = 0u;
        if (i < nqg) {
            const int slot = slot0 + i;
            qm[i] = a.qmask[a.q0 + slot]; qw[i] = a.qwant[a.q0 + slot];
            const float *__restrict__ src = a.LUT + (int64_t)(slot / a.QT) * entries * a.QT + slot % a.QT;
            for (int e = t; e < entries; e += SEL_THREADS) lut[i * entries + e] = src[(int64_t)e * a.QT];
        }
    }
    if constexpr (PACKED) ntab[t] = a.norms[t];                      // (SEL_THREADS == 256 entries)
    if (t < 3 * QB) tick[t] = 0u;
    if (t < 2) bstat[t] = 0ull;
    __syncthreads();
    unsigned placed = 0, pairs = 0;                                  // (wave-uniform; a wave sees a quarter of its range: at most 2^29 rows x QB <= 2^31)
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
            if (i >= nqg) continue;                                  // (block-uniform)
            const uint32_t v = lab & qm[i];
            const bool pass = ok && (a.any ? v != 0u : v == qw[i]);
            const unsigned long long pm = __ballot(pass);
            uint64_t rec = 0ull;
            bool hit = false;
            if (pm) {                                                // (wave-uniform) a wave without a candidate gathers nothing
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
                if constexpr (IVF) { if (a.add) dist = dist + cq; }  // one more rounded add
                rec = ((uint64_t)lsq_adc_key(dist) << a.idbits) | (uint64_t)(uint32_t)(id + 1);
                hit = pass && rec < p[i].bound;
                pairs += (unsigned)__popcll(pm);
                placed += (unsigned)__popcll(__ballot(hit));
            }
            pool_place(p[i], rec, hit);
        }
        __syncthreads();                                             // the step's one barrier
#pragma unroll
        for (int i = 0; i < QB; ++i)
            if (i < nqg) pool_settle(p[i]);
    };
    if constexpr (!IVF) {
        const int64_t first = (int64_t)blockIdx.y * a.per;
        const int64_t last = first + a.per < (int64_t)a.n ? first + a.per : (int64_t)a.n;
        for (int64_t r0 = first; r0 < last; r0 += SEL_THREADS) {     // (block-uniform trip count; row `first` exists inside)
            const bool live = r0 + t < last;
            step(live ? r0 + t : first, live, 0.0f);
        }
    } else {
        const int q = a.q0 + slot0;
        const int *__restrict__ probe = a.probe + (int64_t)q * a.nprobe;
        for (int r = (int)blockIdx.y; r < a.nprobe; r += (int)gridDim.y) {
            const int l = probe[r];
            const int b = a.off[l], len = a.off[l + 1] - b;
            const float cq = a.add ? a.coarse[(int64_t)q * a.nprobe + r] : 0.0f;
            for (int i0 = 0; i0 < len; i0 += SEL_THREADS) {          // (block-uniform trip count; len >= 1 inside: row b exists)
                const bool live = i0 + t < len;
                step((int64_t)b + (live ? i0 + t : 0), live, cq);
            }
        }
    }
    if (lane == 0) {                                                 // (read behind the barrier below)
        if (placed) atomicAdd(&bstat[0], (unsigned long long)placed);
        if (pairs) atomicAdd(&bstat[1], (unsigned long long)pairs);
    }
    unsigned compactions = 0;
#pragma unroll
    for (int i = 0; i < QB; ++i) {
        if (i >= nqg) continue;
        const int slot = slot0 + i;
        if (gridDim.y == 1) {
            pool_hand_out(p[i], a.q0 + slot, a.dists, a.out_ids, a.idbits);
        } else {
            pool_sort(p[i]);
            const int have = p[i].fill < p[i].nn ? p[i].fill : p[i].nn;
            const int64_t run = (int64_t)slot * gridDim.y + blockIdx.y;
            for (int r = t; r < have; r += SEL_THREADS) a.part[run * a.nn + r] = p[i].rec[r];
            if (t == 0) a.pcount[run] = (unsigned)have;
        }
        compactions += p[i].compactions;
    }
    __syncthreads();
    if (t == 0) {
        if (bstat[0]) atomicAdd(&a.stat[0], bstat[0]);
        if (compactions) atomicAdd(&a.stat[1], (unsigned long long)compactions);
        if (bstat[1]) atomicAdd(&a.stat[2], bstat[1]);
    }
}

// lab[p] = labels[ids[p]]: the labels in the order of the inverted layout, so that the list walk reads a row's label where it reads its code
__global__ void label_layout_kernel(const uint32_t *__restrict__ labels, const int *__restrict__ ids, int64_t n, uint32_t *__restrict__ lab) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) lab[p] = labels[ids[p]];
}

// the statistics' words are cleared by a kernel (a memset node has no place in a captured stream)
__global__ void label_clear_kernel(unsigned long long *stat) {
    if (threadIdx.x < 3) stat[threadIdx.x] = 0ull;
}

template <int MW, bool PACKED, bool FILT>
int launch_geometry(hipStream_t s, const LabelScan &a, bool ivf, int qb, dim3 grid, size_t lds) {
#define LABEL_GO(QBV, IVFV)                                                                                                             \
    do {                                                                                                                                \
        LSQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&label_topk_kernel<MW, PACKED, FILT, QBV, IVFV>),                    \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                                             \
        hipLaunchKernelGGL((label_topk_kernel<MW, PACKED, FILT, QBV, IVFV>), grid, dim3(SEL_THREADS), lds, s, a);                       \
    } while (0)
    if (ivf) LABEL_GO(1, true);
    else if (qb == 4) LABEL_GO(4, false);
    else if (qb == 2) LABEL_GO(2, false);
    else LABEL_GO(1, false);
#undef LABEL_GO
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

template <int MW>
int launch_rows(hipStream_t s, const LabelScan &a, bool packed, bool ivf, int qb, dim3 grid, size_t lds) {
    if (a.bits) return packed ? launch_geometry<MW, true, true>(s, a, ivf, qb, grid, lds) : launch_geometry<MW, false, true>(s, a, ivf, qb, grid, lds);
    return packed ? launch_geometry<MW, true, false>(s, a, ivf, qb, grid, lds) : launch_geometry<MW, false, false>(s, a, ivf, qb, grid, lds);
}

}  // namespace

// ---- the geometry, as host functions -----------------------------------------------------------------------------------------------------------------------
int lsq_label_qb(int m, int packed, int nn) {
    const size_t per_query = sizeof(float) * ((size_t)m * LSQ_H + (packed ? 256 : 0)) + sizeof(uint64_t) * (size_t)lsq_ivfsel_pool_records(nn);
    int cap = 4;
#ifdef LSQ_TUNING
    // the tuning library's knob: LSQ_LABEL_QB = 1 or 2 caps the queries per block (read at every call, so that one process can alternate the geometries):
    // what QB buys is measured against it (tools/label_bench.py --qb)
    if (const char *e = getenv("LSQ_LABEL_QB")) cap = std::max(1, std::min(4, atoi(e)));
#endif
    for (int qb = 4; qb > 1; qb >>= 1)
        if (qb <= cap && (size_t)qb * per_query <= 65536) return qb;
    return 1;
}

// what a block allocates: qb tables, ONE norm table (packed), qb pools
size_t lsq_label_lds_bytes(int m, int packed, int nn, int qb) {
    return sizeof(float) * ((size_t)qb * m * LSQ_H + (packed ? 256 : 0)) + sizeof(uint64_t) * (size_t)qb * lsq_ivfsel_pool_records(nn);
}

// the row ranges of the exhaustive walk: range y = rows [y per, min(n, (y + 1) per)), per a multiple of 256, every range non-empty.  Enough blocks to fill the
// chip a few times over when the query groups are few (ivf_scan_kernel's rule); never more than 2^28 rows to a range unless one range is asked for
void lsq_label_split(int64_t n, int groups, int one_split, int *splits, int64_t *per) {
    const int64_t steps = (n + 255) / 256;
    int64_t want = one_split ? 1 : (2048 + (int64_t)groups - 1) / std::max(groups, 1);
    if (!one_split) want = std::max<int64_t>(want, (n + (1 << 28) - 1) >> 28);
    want = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, steps), 65535));
    const int64_t rows = (steps + want - 1) / want * 256;
    *per = rows;
    *splits = (int)std::max<int64_t>(1, (n + rows - 1) / rows);
}

extern "C" int lsq_label_geometry(int64_t n, int m, int packed, int nn, int nq, int flags, lsq_label_geometry_info *out) {
    if (!out || n < 1 || m < 1 || m > LSQ_MAX_M || nn < 1 || nn > LSQ_IVF_SELECT_MAX_NN || nq < 1 || (flags & ~(LSQ_LABEL_ANY | LSQ_LABEL_TEST_ONE_SPLIT))) {
        lsq_set_error("lsq_label_geometry: needs n >= 1, 1 <= m <= %d, 1 <= nn <= %d, nq >= 1, known flags and an output (got n=%lld m=%d nn=%d nq=%d flags=%d)",
                      LSQ_MAX_M, LSQ_IVF_SELECT_MAX_NN, (long long)n, m, nn, nq, flags);
        return LSQ_EINVAL;
    }
    const int qb = lsq_label_qb(m, packed, nn);
    int splits = 0;
    int64_t per = 0;
    lsq_label_split(n, (nq + qb - 1) / qb, (flags & LSQ_LABEL_TEST_ONE_SPLIT) != 0, &splits, &per);
    out->queries_per_block = qb; out->pool_records = lsq_ivfsel_pool_records(nn); out->lds_bytes = (int64_t)lsq_label_lds_bytes(m, packed, nn, qb);
    out->query_groups = (nq + qb - 1) / qb; out->blocks_per_query = splits; out->rows_per_block = per;
    return LSQ_OK;
}

// ---- the index's labels and the scratch of its labelled searches ---------------------------------------------------------------------------------------------
struct lsq_label_state {
    int64_t n = 0;
    bool set = false, layout_valid = false;
    DevBuf labels, layout;                           // [n] in original order (a copy: the index owns it); [n] in the order of the inverted layout, built lazily
    DevBuf qmask, qwant, lut, part, pcount, stat;
    PhaseClock<4> clock;                             // one batch: tables, scan, merge
    lsq_label_info info{};
};

void lsq_label_free(lsq_label_state *st) {
    if (!st) return;
    DevBuf *all[] = {&st->labels, &st->layout, &st->qmask, &st->qwant, &st->lut, &st->part, &st->pcount, &st->stat};
    for (DevBuf *b : all) b->release();
    st->clock.release();
    delete st;
}

bool lsq_label_active(const lsq_label_state *st) { return st && st->set; }
void lsq_label_drop(lsq_label_state *st) { if (st) st->set = st->layout_valid = false; }
void lsq_label_drop_layout(lsq_label_state *st) { if (st) st->layout_valid = false; }
const uint32_t *lsq_label_device(const lsq_label_state *st, int64_t *n) {
    if (!lsq_label_active(st)) return nullptr;
    *n = st->n;
    return st->labels.as<uint32_t>();
}

void lsq_label_get_info(const lsq_label_state *st, lsq_label_info *out) {
    *out = st ? st->info : lsq_label_info{};
    out->labels_set = lsq_label_active(st) ? 1 : 0;
    out->rows = lsq_label_active(st) ? st->n : 0;
}

int lsq_label_set(hipStream_t s, lsq_label_state **pst, const uint32_t *labels, int64_t n, int on_device) {
    if (!*pst) *pst = new lsq_label_state();
    lsq_label_state *st = *pst;
    st->set = st->layout_valid = false;
    LSQ_TRY(st->labels.ensure(sizeof(uint32_t) * (size_t)n));
    LSQ_HIP(hipMemcpyAsync(st->labels.p, labels, sizeof(uint32_t) * (size_t)n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    LSQ_HIP(hipStreamSynchronize(s));                                // the caller's array is free when the call returns
    st->n = n; st->set = true;
    return LSQ_OK;
}

// the labels in layout order, once per (labels, lists)
int lsq_label_layout(hipStream_t s, lsq_label_state *st, const int *ids, int64_t n, const uint32_t **out) {
    if (!st->layout_valid) {
        LSQ_TRY(st->layout.ensure(sizeof(uint32_t) * (size_t)n));
        hipLaunchKernelGGL(label_layout_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, st->labels.as<uint32_t>(), ids, n, st->layout.as<uint32_t>());
        LSQ_HIP(hipGetLastError());
        st->layout_valid = true;
    }
    *out = st->layout.as<uint32_t>();
    return LSQ_OK;
}

namespace {

// one chunk of queries on either road: batches of tables, the scan, the merge where several blocks share a query
int label_batches(hipStream_t s, lsq_label_state *st, LabelScan a, const lsq_search_input &in, const lsq_ivf_probes *pr, int nq, int packed, int flags, int timed,
                  bool test_batch) {
    const bool ivf = pr != nullptr;
    const int m = in.m, nn = a.nn, QT = lsq_adc_lut_qt(m);
    const int qb = ivf ? 1 : lsq_label_qb(m, packed, nn);
    const size_t lds = lsq_label_lds_bytes(m, packed, nn, qb);
    const int rowb = packed ? m + 1 : m;                             // bytes of a row: the dword loader takes whole, aligned words
    const bool words = rowb % 4 == 0 && ((uintptr_t)a.codes & 3) == 0;
    int64_t batch = lsq_adc_batch_queries(nn);                       // a query's scratch is its runs: at most 2048 + batch of them, of nn records, in a batch
    if (test_batch) batch = std::min<int64_t>(batch, 8);             // LSQ_IVF_TEST_BATCH: the test hook of lsq_index_search_ivf, honoured here
    a.QT = QT; a.P = lsq_ivfsel_pool_records(nn);
    st->info.queries_per_block = qb; st->info.pool_records = a.P;
    lsq_ivfsel_call mg{};                                            // what ivf_merge_kernel reads
    mg.nn = nn; mg.idbits = a.idbits; mg.dists = a.dists; mg.out_ids = a.out_ids; mg.stat = a.stat;
    for (int q0 = 0; q0 < nq; q0 += (int)batch) {
        const int nqb = (int)std::min<int64_t>(batch, nq - q0), tiles = (nqb + QT - 1) / QT, groups = (nqb + qb - 1) / qb;
        int splits = 1;
        int64_t per = 0;
        if (ivf) splits = (flags & LSQ_LABEL_TEST_ONE_SPLIT) ? 1 : lsq_ivfsel_splits(nqb, a.nprobe);
        else lsq_label_split(a.n, groups, (flags & LSQ_LABEL_TEST_ONE_SPLIT) != 0, &splits, &per);
        LSQ_TRY(st->lut.ensure(sizeof(float) * (size_t)tiles * m * LSQ_H * QT));
        if (splits > 1) {
            LSQ_TRY(st->part.ensure(sizeof(uint64_t) * (size_t)nqb * splits * nn));
            LSQ_TRY(st->pcount.ensure(sizeof(unsigned) * (size_t)nqb * splits));
        }
        a.LUT = st->lut.as<float>(); a.part = mg.part = st->part.as<uint64_t>(); a.pcount = mg.pcount = st->pcount.as<unsigned>();
        a.q0 = q0; a.nqb = nqb; a.per = per;
        LSQ_TRY(st->clock.begin(timed != 0));
        LSQ_TRY(st->clock.mark(s));
        LSQ_TRY(lsq_adc_launch_lut(s, in, nullptr, q0, nqb, st->lut.as<float>()));
        LSQ_TRY(st->clock.mark(s));
        const dim3 grid((unsigned)groups, (unsigned)splits);
        if (words && rowb == 4) LSQ_TRY(launch_rows<1>(s, a, packed != 0, ivf, qb, grid, lds));
        else if (words && rowb == 8) LSQ_TRY(launch_rows<2>(s, a, packed != 0, ivf, qb, grid, lds));
        else if (words && rowb == 12) LSQ_TRY(launch_rows<3>(s, a, packed != 0, ivf, qb, grid, lds));
        else if (words && rowb == 16) LSQ_TRY(launch_rows<4>(s, a, packed != 0, ivf, qb, grid, lds));
        else LSQ_TRY(launch_rows<0>(s, a, packed != 0, ivf, qb, grid, lds));
        LSQ_TRY(st->clock.mark(s));
        if (splits > 1) LSQ_TRY(lsq_ivfsel_launch_merge(s, mg, q0, nqb, splits));
        LSQ_TRY(st->clock.mark(s));
        LSQ_HIP(hipStreamSynchronize(s));                            // the next batch writes the same tables and runs
        st->info.batches += 1;
        st->info.blocks_per_query = std::max<int64_t>(st->info.blocks_per_query, splits);
        if (splits > 1) st->info.merged_runs += (int64_t)nqb * splits;
        if (timed) {
            float ms[3];
            LSQ_TRY(st->clock.read(ms));
            st->info.lut_ms += ms[0]; st->info.scan_ms += ms[1]; st->info.merge_ms += ms[2];
        }
    }
    return LSQ_OK;
}

}  // namespace

int lsq_label_search(hipStream_t s, lsq_label_state *st, const lsq_label_call &c) {
    const int nq = c.nq, nn = c.nn;
    st->info = lsq_label_info{};
    st->info.queries = nq;
    if (nq == 0) return LSQ_OK;
    LSQ_TRY(st->qmask.ensure(sizeof(uint32_t) * (size_t)nq));
    LSQ_TRY(st->qwant.ensure(sizeof(uint32_t) * (size_t)nq));
    LSQ_HIP(hipMemcpyAsync(st->qmask.p, c.q_mask, sizeof(uint32_t) * (size_t)nq, hipMemcpyDefault, s));
    LSQ_HIP(hipMemcpyAsync(st->qwant.p, c.q_want, sizeof(uint32_t) * (size_t)nq, hipMemcpyDefault, s));
    LSQ_TRY(st->stat.ensure(3 * sizeof(unsigned long long)));
    hipLaunchKernelGGL(label_clear_kernel, dim3(1), dim3(64), 0, s, st->stat.as<unsigned long long>());
    LSQ_HIP(hipGetLastError());
    LabelScan a{};
    a.nn = nn; a.m = c.in.m; a.n = c.in.n; a.idbits = lsq_adc_idbits(c.in.n); a.any = (c.flags & LSQ_LABEL_ANY) ? 1 : 0;
    a.stat = st->stat.as<unsigned long long>();
    if (!c.ivf) {
        a.codes = c.in.codes; a.norms = c.in.dbnorms; a.labels = st->labels.as<uint32_t>(); a.bits = c.bits;
        a.qmask = st->qmask.as<uint32_t>(); a.qwant = st->qwant.as<uint32_t>(); a.dists = c.dists; a.out_ids = c.ids;
        LSQ_TRY(label_batches(s, st, a, c.in, nullptr, nq, c.in.packed, c.flags, c.timed, false));
    } else {
        // chunks of queries whose per-(query, probe) words stay below 2^28 (lsq_ivf_search's rule); the coarse step's scratch holds one chunk
        int64_t qc = (int64_t)(1u << 28) / ((int64_t)c.nprobe + 1);
        if (qc < 1) qc = 1;
        for (int64_t c0 = 0; c0 < nq; c0 += qc) {
            const int cn = (int)std::min<int64_t>(qc, nq - c0);
            lsq_ivf_probes pr{};
            double coarse_ms = 0.0;
            LSQ_TRY(lsq_ivf_coarse(s, c.ivf, c.adc, c.q_coarse + c0 * c.ldc, c.ldc, cn, c.nprobe, c.coarse, c.timed, &pr, &coarse_ms));
            st->info.coarse_ms += coarse_ms;
            if (!st->layout_valid) st->info.layout_builds += 1;
            LabelScan b = a;
            LSQ_TRY(lsq_label_layout(s, st, pr.ids, pr.n, &b.labels));
            b.codes = pr.codes; b.norms = pr.norms; b.ids = pr.ids; b.off = pr.off; b.probe = pr.probe; b.coarse = pr.coarse;
            b.bits = c.bits; b.nprobe = c.nprobe; b.add = (c.ivf_flags & LSQ_IVF_ADD_COARSE) ? 1 : 0;
            b.qmask = st->qmask.as<uint32_t>() + c0; b.qwant = st->qwant.as<uint32_t>() + c0; b.dists = c.dists + c0 * nn; b.out_ids = c.ids + c0 * nn;
            lsq_search_input in = c.in;
            in.Q = static_cast<const float *>(c.in.Q) + c0 * c.in.qstride;
            LSQ_TRY(label_batches(s, st, b, in, &pr, cn, pr.packed, c.flags, c.timed, (c.ivf_flags & LSQ_IVF_TEST_BATCH) != 0));
        }
    }
    unsigned long long stat[3] = {0, 0, 0};
    LSQ_HIP(hipMemcpyAsync(stat, st->stat.p, sizeof(stat), hipMemcpyDeviceToHost, s));
    LSQ_HIP(hipStreamSynchronize(s));
    st->info.offered = (int64_t)stat[0]; st->info.compactions = (int64_t)stat[1]; st->info.allowed_pairs = (int64_t)stat[2];
    return LSQ_OK;
}
