// lsq_ivf.hip -- inverted lists on a resident index ON THE DEVICE (gfx950): a search that reads only the rows of each query's probed lists.
//
// The reference has no counterpart (its scan, src/linscan/Linscan.jl:46-73, reads every code); the arithmetic is the scans' own, so that with every list
// probed the result is lsq_adc.hip's bit for bit:
//
//   coarse(q, l) = lsq_knn.hip's distance of q_coarse to centroid l; the probed lists are the nprobe smallest (coarse, l) pairs   (the exact search, unchanged)
//   table[e]     = adc_lut_kernel's, from q_scan                                                                              (lsq_adc.hip, unchanged)
//   dist(i)      = (((0 + table[0 h + b_i0]) + table[1 h + b_i1]) + ...) + dbnorms[i]   [ + coarse(q, l) with LSQ_IVF_ADD_COARSE ]
//   result       = the nn smallest (dist, original id) pairs over the probed rows, (+inf, 0) past them                       (lsq_adc_select, unchanged)
//
// What is new here is the layout and the scan:
//   LAYOUT  lsq_ivf_set_lists sorts the keys (list << 32 | row) once (hipcub radix sort: stable, no atomics, the same bits on every call) and gathers codes,
//           norms and original ids into that order: list l is rows off[l] .. off[l + 1] of three arrays, ascending by original id inside.  A PACKED index
//           (lsq_index_create_packed) has two: rows of m + 1 bytes -- the code bytes and the norm byte -- and the ids; its norms are a table of 256 floats.
//   PLAN    ivf_plan_kernel, one thread per query: the prefix sums of its probed lists' lengths in rank order (where each list's records go), the HEAD
//           -- the first lists that hold nn rows together -- and the totals the host sizes its batches by.
//   SCAN    ivf_scan_kernel: a block owns ONE query and every gridDim.y-th of its probed lists.  The query's table -- m KiB, against the 128 KiB tile of
//           adc_scan_kernel -- is staged once per block, read as a column of adc_lut_kernel's [entry][query] tile (a strided read of m * 256 floats, from
//           L2, once per block and not once per list: a list of n / nlist rows is no longer than a table).  A lane owns a row of the list: m LDS gathers and
//           m adds in adc_scan_kernel's order.  What bounds it is the LDS gather rate, as there, at one query per row instead of four.
//   ROADS   every record: record (key << idbits | original id + 1) of the i-th row of the r-th probed list goes to slot prefix[r] + i of the query's segment,
//           padding records fill it up to nn, lsq_adc_select sorts and hands out.  Thresholded: the head's lists are written like that and sorted, the
//           head's nn-th record is an upper bound tau of the answer's nn-th (a bound, not an estimate: a list never comes out short), the other lists
//           append records with !(dist > tau) -- ties and NaN kept -- behind the head's by one wave-aggregated atomic per wave step that has any (a block
//           serves one query, so the per-query staging of adc_scan_kernel's MODE 0 has nothing to separate), up to the segment's capacity; an overflowing
//           query is redone with every record.  The order in which the tail's records land varies from run to run; the records are distinct, so the sorted
//           segment does not.
#include <hipcub/hipcub.hpp>
#include <string.h>

#include <algorithm>
#include <thread>
#include <type_traits>
#include <vector>

#include "lsq_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int IVF_THREADS = 256;
constexpr int IVF_TEST_BATCH = 8;            // LSQ_IVF_TEST_BATCH: queries per batch
constexpr int IVF_FLAGS = LSQ_IVF_ADD_COARSE | LSQ_IVF_EVERY_RECORD | LSQ_IVF_TEST_BATCH;

// ---- the layout -----------------------------------------------------------------------------------------------------------------------------------
// keys[i] = list << 32 | row; *bad += entries outside [0, nlist) (a flag: no position depends on it)
__global__ void ivf_keys_kernel(const int32_t *__restrict__ lor, int64_t n, int nlist, uint64_t *__restrict__ keys, unsigned *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t l = lor[i];
    const bool ok = l >= 0 && l < nlist;
    keys[i] = ok ? (((uint64_t)(uint32_t)l << 32) | (uint64_t)i) : ~0ull;
    if (!ok) atomicAdd(bad, 1u);
}

// off[l] = the first position of list l in the sorted keys, off[nlist] = n: position p opens every list after its predecessor's up to its own
__global__ void ivf_offsets_kernel(const uint64_t *__restrict__ sorted, int64_t n, int nlist, int *__restrict__ off) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > n) return;
    const int lo = p == 0 ? 0 : (int)(sorted[p - 1] >> 32) + 1;
    const int hi = p == n ? nlist : (int)(sorted[p] >> 32);
    for (int l = lo; l <= hi; ++l) off[l] = (int)p;
}

__global__ void ivf_layout_kernel(const uint64_t *__restrict__ sorted, int64_t n, int m, const uint8_t *__restrict__ codes, const float *__restrict__ norms,
                                  uint8_t *__restrict__ icodes, float *__restrict__ inorms, int *__restrict__ iids) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int64_t row = (int64_t)(uint32_t)sorted[p];
    for (int j = 0; j < m; ++j) icodes[p * m + j] = codes[row * m + j];
    inorms[p] = norms[row];
    iids[p] = (int)row;
}

// the layout of a PACKED index: rows of m + 1 bytes (code bytes, norm byte) and the original id -- m + 5 bytes per row and no norm array
__global__ void ivf_layout_packed_kernel(const uint64_t *__restrict__ sorted, int64_t n, int rowb, const uint8_t *__restrict__ rows,
                                         uint8_t *__restrict__ irows, int *__restrict__ iids) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int64_t row = (int64_t)(uint32_t)sorted[p];
    for (int j = 0; j < rowb; ++j) irows[p * rowb + j] = rows[row * rowb + j];
    iids[p] = (int)row;
}

// ---- the plan of a query: pos[q][r] = rows of its probed lists of rank < r (pos[q][nprobe] = all of them); plan[q] = {rows, rows of the head, lists of
// the head}.  The head: the first lists, in rank order, that together hold at least nn rows; all of them when there are fewer than nn rows
// Under a row filter (lbits / lpre: its bitmap in layout order and the prefix of its words' popcounts, lsq_filter.hip; null: none) the head is chosen on
// ALLOWED rows -- its nn-th record is then a finite, exact bound whenever the probed lists hold nn allowed rows -- while every position and total stays
// that of the full lengths
__device__ inline int ivf_allowed_before(const uint32_t *__restrict__ lbits, const int *__restrict__ lpre, int p) {
    const int w = p >> 5, b = p & 31;                                // (b == 0: the word is not read -- p may be n, one past the last word)
    return lpre[w] + (b ? __popc(lbits[w] & ((1u << b) - 1u)) : 0);
}
__global__ void ivf_plan_kernel(const int *__restrict__ probe, const int *__restrict__ off, int nq, int nprobe, int nn, int *__restrict__ pos,
                                int *__restrict__ plan, const uint32_t *__restrict__ lbits, const int *__restrict__ lpre) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const int *pr = probe + (int64_t)q * nprobe;
    int *ps = pos + (int64_t)q * (nprobe + 1);
    int sum = 0, head_n = nprobe, head_rows = -1, allowed = 0;
    for (int r = 0; r < nprobe; ++r) {
        const int l = pr[r];
        ps[r] = sum;
        sum += off[l + 1] - off[l];                                  // disjoint lists: at most n < 2^31 in all
        if (lpre) allowed += ivf_allowed_before(lbits, lpre, off[l + 1]) - ivf_allowed_before(lbits, lpre, off[l]);
        if (head_rows < 0 && (lpre ? allowed : sum) >= nn) { head_n = r + 1; head_rows = sum; }
    }
    ps[nprobe] = sum;
    plan[3 * (int64_t)q] = sum;
    plan[3 * (int64_t)q + 1] = head_rows < 0 ? sum : head_rows;
    plan[3 * (int64_t)q + 2] = head_n;
}

// ---- the scan --------------------------------------------------------------------------------------------------------------------------------------
struct IvfScan {
    const float *LUT; int QT;                        // adc_lut_kernel's tiles of this batch
    const uint8_t *codes; const float *norms; const int *ids; const int *off;      // the inverted layout
    const int *probe; const float *coarse;           // [.][nprobe]: the probed lists in rank order and their coarse distances
    const int *pos, *plan;                           // ivf_plan_kernel's
    const int *qsel; int q0;                         // query of a slot: qsel[slot] or q0 + slot
    int nprobe, m, nn, cap, idbits, add;
    const float *tau;                                // [slot][nn]: the head's sorted distances (PART 2)
    unsigned *count;                                 // [slot]: records in the segment
    uint64_t *out;                                   // [slot][cap]
};
// what a FILTERED scan is launched with: the same, and a row filter's bitmap in layout order.  A type of its own: the unfiltered kernels keep their
// argument block, byte for byte
struct IvfScanF : IvfScan {
    const uint32_t *lbits;
};

// PART 0: every record of every probed list; 1: the same of the head's lists; 2: the records with !(dist > tau) of the lists after the head, appended.
// MW > 0: rows of 4 MW bytes, read as dwords (an allocation of the index's own: aligned); MW = 0: any m, byte reads.  PACKED: a row is its m code bytes and
// then its norm byte (m = 4 MW - 1 on the dword loader), a.norms is the norm table of 256 floats, staged beside the query's table.
// FILT (a row filter): bit p of a.lbits says whether layout row p is allowed -- read where the row's code is read, no gather through a.ids.  PART 0 / 1: a
// filtered row writes the padding record into its slot (the segment is sized by list lengths: every slot up to `have` is written); PART 2 appends allowed
// rows only.  FILT = false: the kernel as it was.
template <int MW, int PART, bool PACKED = false, bool FILT = false>
__global__ __launch_bounds__(IVF_THREADS) void ivf_scan_kernel(const std::conditional_t<FILT, IvfScanF, IvfScan> a) {
    __shared__ float lut[LSQ_MAX_M * LSQ_H + (PACKED ? 256 : 0)];    // the query's table: m KiB used; PACKED: the norm table behind all 16 KiB
    constexpr int NT = PACKED ? 4 * MW - 1 : 4 * MW;                 // bytes of a dword-loaded row that index tables
    const int t = threadIdx.x, slot = blockIdx.x;
    const int q = a.qsel ? a.qsel[slot] : a.q0 + slot;
    const int *pl = a.plan + 3 * (int64_t)q;
    const int head_n = pl[2];
    const int lo = PART == 2 ? head_n : 0, hi = PART == 1 ? head_n : a.nprobe;
    uint64_t *__restrict__ out = a.out + (int64_t)slot * a.cap;
    if (PART != 2 && blockIdx.y == 0) {
        // fewer probed rows than nn (the head is then every list): (+inf, id field 0) under the bit above the key, lsq_rerank.hip's record of an id outside the base
        const int have = PART == 0 ? pl[0] : pl[1];
        const uint64_t pad = (1ull << (32 + a.idbits)) | ((uint64_t)lsq_adc_key(__builtin_inff()) << a.idbits);
        for (int i = have + t; i < a.nn; i += IVF_THREADS) out[i] = pad;
        if (t == 0) a.count[slot] = (unsigned)(have > a.nn ? have : a.nn);
    }
    if (lo + (int)blockIdx.y >= hi) return;                          // (block-uniform) none of this part's lists is this block's
    const int entries = a.m * LSQ_H;
    {
        const float *__restrict__ src = a.LUT + (int64_t)(slot / a.QT) * entries * a.QT + slot % a.QT;
        for (int e = t; e < entries; e += IVF_THREADS) lut[e] = src[(int64_t)e * a.QT];
        if constexpr (PACKED) lut[LSQ_MAX_M * LSQ_H + t] = a.norms[t];      // (IVF_THREADS == 256 entries)
    }
    __syncthreads();
    const int *__restrict__ probe = a.probe + (int64_t)q * a.nprobe;
    const int *__restrict__ pos = a.pos + (int64_t)q * (a.nprobe + 1);
    const float tau = PART == 2 ? a.tau[(int64_t)slot * a.nn + a.nn - 1] : 0.0f;
    const int lane = t & 63;
    for (int r = lo + (int)blockIdx.y; r < hi; r += (int)gridDim.y) {
        const int l = probe[r];
        const int b = a.off[l], len = a.off[l + 1] - b;
        const float cq = a.add ? a.coarse[(int64_t)q * a.nprobe + r] : 0.0f;
        const int p0 = pos[r];
        for (int i0 = 0; i0 < len; i0 += IVF_THREADS) {              // (block-uniform trip count; len >= 1 inside: row b exists)
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
            uint64_t rec = ((uint64_t)lsq_adc_key(dist) << a.idbits) | (uint64_t)(uint32_t)(a.ids[row] + 1);      // the ORIGINAL id, 1-based
            bool allowed = true;
            if constexpr (FILT) {
                allowed = ((a.lbits[row >> 5] >> (row & 31)) & 1u) != 0;
                if (!allowed) rec = (1ull << (32 + a.idbits)) | ((uint64_t)lsq_adc_key(__builtin_inff()) << a.idbits);
            }
            if (PART != 2) {
                const int at = p0 + i;                               // < the query's rows <= cap: the host sized cap by them
                if (live && at < a.cap) out[at] = rec;
            } else {
                const bool hit = live && allowed && !(dist > tau);   // a NaN on either side is kept
                const unsigned long long mask = __ballot(hit);
                if (mask) {                                          // (wave-uniform) one atomic for the wave's records of this step
                    const int leader = __ffsll((long long)mask) - 1;
                    unsigned base = 0;
                    if (lane == leader) base = atomicAdd(&a.count[slot], (unsigned)__popcll(mask));
                    base = __shfl(base, leader, 64);
                    const unsigned at = base + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
                    if (hit && at < (unsigned)a.cap) out[at] = rec;
                }
            }
        }
    }
}

template <int PART>
int launch_scan(hipStream_t s, const IvfScan &a, int nqb, bool packed, const uint32_t *lbits) {
    IvfScanF f;
    static_cast<IvfScan &>(f) = a;
    f.lbits = lbits;
    const int rowb = packed ? a.m + 1 : a.m;                         // bytes of a row: the dword loader takes whole words
    // enough blocks to fill the chip a few times over when the queries are few; a block's lists share one staged table
    int splits = (2048 + nqb - 1) / nqb;
    if (splits > a.nprobe) splits = a.nprobe;
    if (splits > 65535) splits = 65535;
    if (splits < 1) splits = 1;
    const dim3 grid((unsigned)nqb, (unsigned)splits), block(IVF_THREADS);
#define IVF_LAUNCH(MWV)                                                                                 \
    do {                                                                                                \
        if (lbits) {                                                                                    \
            if (packed) hipLaunchKernelGGL((ivf_scan_kernel<MWV, PART, true, true>), grid, block, 0, s, f);    \
            else hipLaunchKernelGGL((ivf_scan_kernel<MWV, PART, false, true>), grid, block, 0, s, f);          \
        } else if (packed) hipLaunchKernelGGL((ivf_scan_kernel<MWV, PART, true>), grid, block, 0, s, a);       \
        else hipLaunchKernelGGL((ivf_scan_kernel<MWV, PART, false>), grid, block, 0, s, a);             \
    } while (0)
    if (rowb == 4) IVF_LAUNCH(1);
    else if (rowb == 8) IVF_LAUNCH(2);
    else if (rowb == 12) IVF_LAUNCH(3);
    else if (rowb == 16) IVF_LAUNCH(4);
    else IVF_LAUNCH(0);
#undef IVF_LAUNCH
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

}  // namespace

// ---- rows grouped by list: the one sort behind lsq_index_set_lists and lsq_partition_update (lsq_partition.hip) -----------------------------------------
// keys (list << 32 | row), ~0 for an entry outside [0, nlist): *bad = how many of those (the call waits for the count); nothing else has been touched then
int lsq_rows_keys(hipStream_t s, lsq_row_groups &g, const int32_t *list_of_row, int on_device, int64_t n, int nlist, unsigned *bad) {
    const int32_t *lor = list_of_row;
    if (!on_device) {
        LSQ_TRY(g.s_lor.ensure(sizeof(int32_t) * (size_t)n));
        LSQ_HIP(hipMemcpyAsync(g.s_lor.p, list_of_row, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
        lor = g.s_lor.as<int32_t>();
    }
    LSQ_TRY(g.keys_a.ensure(sizeof(uint64_t) * (size_t)n));
    LSQ_TRY(g.keys_b.ensure(sizeof(uint64_t) * (size_t)n));
    LSQ_TRY(g.flag.ensure(sizeof(unsigned)));
    LSQ_HIP(hipMemsetAsync(g.flag.p, 0, sizeof(unsigned), s));
    hipLaunchKernelGGL(ivf_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, lor, n, nlist, g.keys_a.as<uint64_t>(), g.flag.as<unsigned>());
    LSQ_HIP(hipGetLastError());
    LSQ_HIP(hipMemcpyAsync(bad, g.flag.p, sizeof(*bad), hipMemcpyDeviceToHost, s));
    LSQ_HIP(hipStreamSynchronize(s));
    return LSQ_OK;
}

// the keys sorted (hipcub radix sort: stable, no atomics, the same bits on every call): list by list and, within a list, ascending by row
int lsq_rows_sort(hipStream_t s, lsq_row_groups &g, int64_t n, int nlist, const uint64_t **sorted) {
    int list_bits = 1;
    while ((nlist - 1) >> list_bits) ++list_bits;
    size_t bytes = 0;
    LSQ_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, g.keys_a.as<uint64_t>(), g.keys_b.as<uint64_t>(), (int)n, 0, 32 + list_bits, s));
    LSQ_TRY(g.tmp.ensure(bytes > 0 ? bytes : 16));
    LSQ_HIP(hipcub::DeviceRadixSort::SortKeys(g.tmp.p, bytes, g.keys_a.as<uint64_t>(), g.keys_b.as<uint64_t>(), (int)n, 0, 32 + list_bits, s));
    *sorted = g.keys_b.as<uint64_t>();
    return LSQ_OK;
}

// off[l] = the first position of list l in the sorted keys, off[nlist] = n
int lsq_rows_offsets(hipStream_t s, const uint64_t *sorted, int64_t n, int nlist, int *off) {
    hipLaunchKernelGGL(ivf_offsets_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, s, sorted, n, nlist, off);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

struct lsq_ivf_state {
    int nlist = 0, m = 0, d = 0, packed = 0;
    int64_t n = 0;
    const float *table = nullptr;                                    // packed: the index's norm table (256 floats, alive as long as the index)
    DevBuf cent, codes, norms, ids, off;                             // the layout: centroids, and per position the code row (packed: with its norm byte), the norm (not packed), the original id
    lsq_row_groups rows;                                             // set_lists' scratch: the rows grouped by list
    DevBuf alt_codes, alt_norms, alt_ids, alt_off, add_off;          // lsq_index_add: the spare half a merge is written into (it becomes the layout at the commit), the new rows' offsets
    DevBuf cd, ci, pos, plan, lut, rec_a, rec_b, seg, count, fail, qsel, head_d, head_i;      // the search's
    PhaseClock<6> clock;                                             // one batch: tables, scan, selection and, thresholded, the tail's scan and selection
    lsq_ivf_info info{};
};

void lsq_ivf_free(lsq_ivf_state *st) {
    if (!st) return;
    DevBuf *all[] = {&st->cent, &st->codes, &st->norms, &st->ids, &st->off, &st->alt_codes, &st->alt_norms, &st->alt_ids, &st->alt_off, &st->add_off, &st->cd, &st->ci,
                     &st->pos, &st->plan, &st->lut, &st->rec_a, &st->rec_b, &st->seg, &st->count, &st->fail, &st->qsel, &st->head_d, &st->head_i};
    for (DevBuf *b : all) b->release();
    st->rows.release();
    st->clock.release();
    delete st;
}

int lsq_ivf_nlist(const lsq_ivf_state *st) { return st ? st->nlist : 0; }

void lsq_ivf_layout(const lsq_ivf_state *st, const int **ids, const int **off) {
    const bool have = st && st->nlist > 0;
    *ids = have ? st->ids.as<int>() : nullptr;
    *off = have ? st->off.as<int>() : nullptr;
}

const float *lsq_ivf_centroids(const lsq_ivf_state *st) { return st && st->nlist > 0 ? st->cent.as<float>() : nullptr; }

void lsq_ivf_get_info(const lsq_ivf_state *st, lsq_ivf_info *out) { *out = st ? st->info : lsq_ivf_info{}; }

int lsq_ivf_set_lists(hipStream_t s, lsq_ivf_state **pst, const uint8_t *codes, const float *norms, int packed, int64_t n, int m, int d,
                      const lsq_ivf_desc *desc) {
    if (!*pst) *pst = new lsq_ivf_state();
    lsq_ivf_state *st = *pst;
    const int nlist = desc->nlist;
    const unsigned blocks_n = (unsigned)((n + 255) / 256);
    // the range check: the one kernel that reads the entries; nothing of the layout is touched before its verdict
    unsigned bad = 0;
    LSQ_TRY(lsq_rows_keys(s, st->rows, desc->list_of_row, desc->on_device, n, nlist, &bad));
    if (bad) {
        lsq_set_error("lsq_index_set_lists: %u entries of list_of_row lie outside [0, %d)", bad, nlist);
        return LSQ_EINVAL;
    }
    st->nlist = 0;                                                   // no lists while they are rebuilt
    const uint64_t *sorted = nullptr;
    LSQ_TRY(lsq_rows_sort(s, st->rows, n, nlist, &sorted));
    LSQ_TRY(st->cent.ensure(sizeof(float) * (size_t)nlist * d));
    const int rowb = packed ? m + 1 : m;
    LSQ_TRY(st->codes.ensure((size_t)n * rowb + 16));                // 16 bytes of slack past the last row, never read
    if (!packed) LSQ_TRY(st->norms.ensure(sizeof(float) * (size_t)n));
    LSQ_TRY(st->ids.ensure(sizeof(int) * (size_t)n));
    LSQ_TRY(st->off.ensure(sizeof(int) * ((size_t)nlist + 1)));
    LSQ_HIP(hipMemcpyAsync(st->cent.p, desc->centroids, sizeof(float) * (size_t)nlist * d, hipMemcpyDefault, s));
    LSQ_TRY(lsq_rows_offsets(s, sorted, n, nlist, st->off.as<int>()));
    if (packed)
        hipLaunchKernelGGL(ivf_layout_packed_kernel, dim3(blocks_n), dim3(256), 0, s, sorted, n, rowb, codes, st->codes.as<uint8_t>(), st->ids.as<int>());
    else
        hipLaunchKernelGGL(ivf_layout_kernel, dim3(blocks_n), dim3(256), 0, s, sorted, n, m, codes, norms, st->codes.as<uint8_t>(), st->norms.as<float>(),
                           st->ids.as<int>());
    LSQ_HIP(hipGetLastError());
    LSQ_HIP(hipStreamSynchronize(s));
    st->nlist = nlist; st->n = n; st->m = m; st->d = d; st->packed = packed; st->table = packed ? norms : nullptr;
    return LSQ_OK;
}

// ---- lsq_index_add's part (the kernels: lsq_grow.hip) ---------------------------------------------------------------------------------------------------
// The layout of n + count rows is written into the spare half and swapped in at the commit: until then every search reads the former one.  Nothing else
// of this state depends on n: the search's scratch is sized per call, idbits and the scan's input are read from st->n at every call
int lsq_ivf_add_check(hipStream_t s, lsq_ivf_state *st, const int32_t *list_of_row, int on_device, int64_t count, unsigned *bad) {
    return lsq_rows_keys(s, st->rows, list_of_row, on_device, count, st->nlist, bad);
}

namespace {
// bytes of the layout's arrays at a capacity of `rows` rows (code rows end in 16 bytes of slack, never read as rows)
size_t ivf_code_bytes(const lsq_ivf_state *st, int64_t rows) { return (size_t)rows * (size_t)(st->packed ? st->m + 1 : st->m) + 16; }
int ivf_ensure_spare(lsq_ivf_state *st, int64_t cap_rows, int *realloc) {
    const size_t before[3] = {st->alt_codes.cap, st->alt_norms.cap, st->alt_ids.cap};
    LSQ_TRY(st->alt_codes.ensure(ivf_code_bytes(st, cap_rows)));
    if (!st->packed) LSQ_TRY(st->alt_norms.ensure(sizeof(float) * (size_t)cap_rows));
    LSQ_TRY(st->alt_ids.ensure(sizeof(int) * (size_t)cap_rows));
    LSQ_TRY(st->alt_off.ensure(sizeof(int) * ((size_t)st->nlist + 1)));
    LSQ_TRY(st->add_off.ensure(sizeof(int) * ((size_t)st->nlist + 1)));
    if (before[0] != st->alt_codes.cap || before[1] != st->alt_norms.cap || before[2] != st->alt_ids.cap) *realloc = 1;
    return LSQ_OK;
}
}  // namespace

int lsq_ivf_reserve(hipStream_t s, lsq_ivf_state *st, int64_t cap_rows, int *realloc) {
    if (!st || st->nlist < 1) return LSQ_OK;
    LSQ_TRY(ivf_ensure_spare(st, cap_rows, realloc));
    const size_t before[3] = {st->codes.cap, st->norms.cap, st->ids.cap};
    const int rowb = st->packed ? st->m + 1 : st->m;
    LSQ_TRY(lsq_devbuf_grow(s, st->codes, ivf_code_bytes(st, cap_rows), (size_t)st->n * rowb));
    if (!st->packed) LSQ_TRY(lsq_devbuf_grow(s, st->norms, sizeof(float) * (size_t)cap_rows, sizeof(float) * (size_t)st->n));
    LSQ_TRY(lsq_devbuf_grow(s, st->ids, sizeof(int) * (size_t)cap_rows, sizeof(int) * (size_t)st->n));
    if (before[0] != st->codes.cap || before[1] != st->norms.cap || before[2] != st->ids.cap) *realloc = 1;
    return LSQ_OK;
}

int lsq_ivf_add_merge(hipStream_t s, lsq_ivf_state *st, const uint8_t *add_rows, const float *add_norms, int64_t count, int64_t cap_rows, int *realloc) {
    LSQ_TRY(ivf_ensure_spare(st, cap_rows, realloc));
    const uint64_t *sorted = nullptr;
    LSQ_TRY(lsq_rows_sort(s, st->rows, count, st->nlist, &sorted));
    LSQ_TRY(lsq_rows_offsets(s, sorted, count, st->nlist, st->add_off.as<int>()));
    lsq_grow_merge g{};
    g.src_codes = st->codes.as<uint8_t>(); g.src_norms = st->packed ? nullptr : st->norms.as<float>(); g.src_ids = st->ids.as<int>(); g.off = st->off.as<int>();
    g.dst_codes = st->alt_codes.as<uint8_t>(); g.dst_norms = st->packed ? nullptr : st->alt_norms.as<float>(); g.dst_ids = st->alt_ids.as<int>();
    g.noff = st->alt_off.as<int>();
    g.add_off = st->add_off.as<int>(); g.sorted = sorted; g.add_rows = add_rows; g.add_norms = add_norms;
    g.n = st->n; g.count = count; g.nlist = st->nlist; g.rowb = st->packed ? st->m + 1 : st->m;
    return lsq_grow_launch_merge(s, g);
}

void lsq_ivf_add_commit(lsq_ivf_state *st, int64_t count) {
    std::swap(st->codes, st->alt_codes);
    std::swap(st->norms, st->alt_norms);
    std::swap(st->ids, st->alt_ids);
    std::swap(st->off, st->alt_off);
    st->n += count;
}

// ---- lsq_index_compact's part (the kernels: lsq_compact.hip) ----------------------------------------------------------------------------------------------
// The layout of the surviving rows is written into the spare half and swapped in at the commit, as an add's merge is.  exact (LSQ_COMPACT_SHRINK): the
// spare half is dropped and made again at just cap_rows rows (it holds nothing); the other half follows after the commit (lsq_ivf_fit)
int lsq_ivf_compact(hipStream_t s, lsq_ivf_state *st, const lsq_filter_view &v, const int *lsel, int64_t rows_out, int64_t cap_rows, bool exact, int64_t *bytes) {
    if (exact) { st->alt_codes.release(); st->alt_norms.release(); st->alt_ids.release(); }
    int moved = 0;
    LSQ_TRY(ivf_ensure_spare(st, cap_rows, &moved));
    lsq_compact_layout g{};
    g.src_codes = st->codes.as<uint8_t>(); g.src_norms = st->packed ? nullptr : st->norms.as<float>(); g.src_ids = st->ids.as<int>(); g.off = st->off.as<int>();
    g.dst_codes = st->alt_codes.as<uint8_t>(); g.dst_norms = st->packed ? nullptr : st->alt_norms.as<float>(); g.dst_ids = st->alt_ids.as<int>();
    g.noff = st->alt_off.as<int>();
    g.lbits = v.lbits; g.lpre = v.lpre; g.lsel = lsel; g.bits = v.bits; g.pre = v.pre;
    g.rows_out = rows_out; g.nlist = st->nlist; g.rowb = st->packed ? st->m + 1 : st->m;
    return lsq_compact_launch_layout(s, g, bytes);
}

void lsq_ivf_compact_commit(lsq_ivf_state *st, int64_t rows_out) {
    std::swap(st->codes, st->alt_codes);
    std::swap(st->norms, st->alt_norms);
    std::swap(st->ids, st->alt_ids);
    std::swap(st->off, st->alt_off);
    st->n = rows_out;
}

int lsq_ivf_fit(hipStream_t s, lsq_ivf_state *st, int64_t rows) {
    if (!st || st->nlist < 1) return LSQ_OK;
    const size_t rowb = (size_t)(st->packed ? st->m + 1 : st->m), n = (size_t)st->n;
    LSQ_TRY(lsq_devbuf_fit(s, st->codes, ivf_code_bytes(st, rows), n * rowb));
    if (!st->packed) LSQ_TRY(lsq_devbuf_fit(s, st->norms, sizeof(float) * (size_t)rows, sizeof(float) * n));
    LSQ_TRY(lsq_devbuf_fit(s, st->ids, sizeof(int) * (size_t)rows, sizeof(int) * n));
    LSQ_TRY(lsq_devbuf_fit(s, st->alt_codes, ivf_code_bytes(st, rows), 0));
    if (!st->packed) LSQ_TRY(lsq_devbuf_fit(s, st->alt_norms, sizeof(float) * (size_t)rows, 0));
    return lsq_devbuf_fit(s, st->alt_ids, sizeof(int) * (size_t)rows, 0);
}

// the probed lists of nq queries: the exact search with the centroids as base, on the index's scan state -> st->ci (lists in rank order) and st->cd (their
// coarse distances), [nq][nprobe].  out (optional): those two and the layout, for a scan outside this file (lsq_range.hip); valid until the next call on st
int lsq_ivf_coarse(hipStream_t s, lsq_ivf_state *st, lsq_adc_state **adc, const float *q_coarse, int64_t ldc, int nq, int nprobe, const lsq_search_opts &coarse,
                   int timed, lsq_ivf_probes *out, double *coarse_ms) {
    LSQ_TRY(st->cd.ensure(sizeof(float) * (size_t)nq * nprobe));
    LSQ_TRY(st->ci.ensure(sizeof(int) * (size_t)nq * nprobe));
    lsq_search_input ex{};
    ex.kind = LSQ_SEARCH_EXACT; ex.Q = q_coarse; ex.qstride = (int)ldc; ex.n = st->nlist; ex.d = st->d; ex.base = st->cent.p; ex.bstride = st->d;
    lsq_linscan_stats cs{};
    lsq_search_opts co = coarse;
    co.stats = &cs; co.timed = timed ? 1 : 0;
    LSQ_TRY(lsq_adc_search(s, adc, st->cd.as<float>(), st->ci.as<int>(), ex, nq, nprobe, co));
    if (coarse_ms) *coarse_ms = cs.lut_ms + cs.sample_ms + cs.scan_ms + cs.select_ms;
    if (out) {
        out->probe = st->ci.as<int>(); out->coarse = st->cd.as<float>();
        out->codes = st->codes.as<uint8_t>(); out->norms = st->packed ? st->table : st->norms.as<float>(); out->ids = st->ids.as<int>(); out->off = st->off.as<int>();
        out->n = st->n; out->nlist = st->nlist; out->m = st->m; out->d = st->d; out->packed = st->packed;
    }
    return LSQ_OK;
}

namespace {

struct Chunk {                       // one run of queries whose plan fits the scratch: everything below counts queries from its first
    hipStream_t s;
    lsq_ivf_state *st;
    lsq_adc_state **adc;
    lsq_search_input in;             // the tables' input: q_scan of the chunk
    float *dists; int *ids;
    int nq, nprobe, nn, flags, idbits;
    bool timed;
    const uint32_t *lbits; const int *lpre;      // a row filter in layout order (lsq_filter.hip), or null
};

// one batch on either road: slots 0 .. nqb - 1 are queries q0 .. (or qsel[.]).  thresholded: h_fail[slot] = 1 for a query whose segment overflowed
int run_batch(const Chunk &c, const int *qsel, int q0, int nqb, int cap, bool thresholded, int *h_fail) {
    lsq_ivf_state *st = c.st;
    hipStream_t s = c.s;
    const int m = c.in.m, QT = lsq_adc_lut_qt(m), tiles = (nqb + QT - 1) / QT;
    LSQ_TRY(st->lut.ensure(sizeof(float) * (size_t)tiles * m * LSQ_H * QT));
    LSQ_TRY(st->rec_a.ensure(sizeof(uint64_t) * (size_t)nqb * cap));
    LSQ_TRY(st->rec_b.ensure(sizeof(uint64_t) * (size_t)nqb * cap));
    LSQ_TRY(st->seg.ensure(sizeof(int) * 2 * (size_t)nqb));
    LSQ_TRY(st->count.ensure(sizeof(unsigned) * (size_t)nqb));
    LSQ_TRY(st->fail.ensure(sizeof(int) * (size_t)nqb));
    LSQ_TRY(st->clock.begin(c.timed));
    LSQ_TRY(st->clock.mark(s));
    LSQ_TRY(lsq_adc_launch_lut(s, c.in, qsel, q0, nqb, st->lut.as<float>()));
    LSQ_TRY(st->clock.mark(s));
    IvfScan a{};
    a.LUT = st->lut.as<float>(); a.QT = QT;
    a.codes = st->codes.as<uint8_t>(); a.norms = st->packed ? st->table : st->norms.as<float>(); a.ids = st->ids.as<int>(); a.off = st->off.as<int>();
    a.probe = st->ci.as<int>(); a.coarse = st->cd.as<float>(); a.pos = st->pos.as<int>(); a.plan = st->plan.as<int>();
    a.qsel = qsel; a.q0 = q0;
    a.nprobe = c.nprobe; a.m = m; a.nn = c.nn; a.cap = cap; a.idbits = c.idbits; a.add = (c.flags & LSQ_IVF_ADD_COARSE) ? 1 : 0;
    a.count = st->count.as<unsigned>(); a.out = st->rec_a.as<uint64_t>();
    const bool packed = st->packed != 0;
    // records: (padding bit, distance key, original id + 1), sorted on 33 + idbits bits; the hand-out drops the bit: (+inf, 0) for padding
    if (!thresholded) {
        LSQ_TRY(launch_scan<0>(s, a, nqb, packed, c.lbits));
        LSQ_TRY(st->clock.mark(s));
        LSQ_TRY(lsq_adc_select(c.adc, s, st->rec_a.as<uint64_t>(), st->rec_b.as<uint64_t>(), st->seg.as<int>(), st->count.as<unsigned>(), nullptr, qsel, q0,
                               nqb, cap, c.nn, c.dists, c.ids, c.idbits, 33 + c.idbits, 0));
    } else {
        LSQ_TRY(st->head_d.ensure(sizeof(float) * (size_t)nqb * c.nn));
        LSQ_TRY(st->head_i.ensure(sizeof(int) * (size_t)nqb * c.nn));
        LSQ_TRY(launch_scan<1>(s, a, nqb, packed, c.lbits));
        LSQ_TRY(st->clock.mark(s));
        // the head, sorted: head_d[slot][nn - 1] is tau
        LSQ_TRY(lsq_adc_select(c.adc, s, st->rec_a.as<uint64_t>(), st->rec_b.as<uint64_t>(), st->seg.as<int>(), st->count.as<unsigned>(), nullptr, nullptr, 0,
                               nqb, cap, c.nn, st->head_d.as<float>(), st->head_i.as<int>(), c.idbits, 33 + c.idbits, 0));
        LSQ_TRY(st->clock.mark(s));
        a.tau = st->head_d.as<float>();
        LSQ_TRY(launch_scan<2>(s, a, nqb, packed, c.lbits));
        LSQ_TRY(st->clock.mark(s));
        LSQ_TRY(lsq_adc_select(c.adc, s, st->rec_a.as<uint64_t>(), st->rec_b.as<uint64_t>(), st->seg.as<int>(), st->count.as<unsigned>(), st->fail.as<int>(),
                               qsel, q0, nqb, cap, c.nn, c.dists, c.ids, c.idbits, 33 + c.idbits, 0));
        LSQ_HIP(hipMemcpyAsync(h_fail, st->fail.p, sizeof(int) * (size_t)nqb, hipMemcpyDeviceToHost, s));
    }
    LSQ_TRY(st->clock.mark(s));
    std::vector<unsigned> hc((size_t)nqb);
    LSQ_HIP(hipMemcpyAsync(hc.data(), st->count.p, sizeof(unsigned) * (size_t)nqb, hipMemcpyDeviceToHost, s));
    LSQ_HIP(hipStreamSynchronize(s));
    for (unsigned v : hc) st->info.records += v < (unsigned)cap ? v : (unsigned)cap;
    st->info.batches += 1;
    if (c.timed) {
        float ms[5];
        LSQ_TRY(st->clock.read(ms));
        st->info.lut_ms += ms[0];
        st->info.scan_ms += ms[1] + (thresholded ? ms[3] : 0.0f);
        st->info.select_ms += ms[2] + (thresholded ? ms[4] : 0.0f);
    }
    return LSQ_OK;
}

int64_t batch_queries(int cap, int flags) {
    const int64_t qb = lsq_adc_batch_queries(cap);                   // cap record slots per query (one query's records are one batch)
    return (flags & LSQ_IVF_TEST_BATCH) && qb > IVF_TEST_BATCH ? IVF_TEST_BATCH : qb;
}

int run_chunk(Chunk &c, const float *q_coarse, int64_t ldc, const lsq_search_opts &coarse) {
    lsq_ivf_state *st = c.st;
    hipStream_t s = c.s;
    const int nq = c.nq, nprobe = c.nprobe, nn = c.nn;
    // the probed lists
    double coarse_ms = 0.0;
    LSQ_TRY(lsq_ivf_coarse(s, st, c.adc, q_coarse, ldc, nq, nprobe, coarse, c.timed ? 1 : 0, nullptr, &coarse_ms));
    st->info.coarse_ms += coarse_ms;
    // the plan
    LSQ_TRY(st->pos.ensure(sizeof(int) * (size_t)nq * ((size_t)nprobe + 1)));
    LSQ_TRY(st->plan.ensure(sizeof(int) * 3 * (size_t)nq));
    hipLaunchKernelGGL(ivf_plan_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, st->ci.as<int>(), st->off.as<int>(), nq, nprobe, nn,
                       st->pos.as<int>(), st->plan.as<int>(), c.lbits, c.lpre);
    LSQ_HIP(hipGetLastError());
    std::vector<int> plan(3 * (size_t)nq);
    LSQ_HIP(hipMemcpyAsync(plan.data(), st->plan.p, sizeof(int) * plan.size(), hipMemcpyDeviceToHost, s));
    LSQ_HIP(hipStreamSynchronize(s));
    int max_rows = 0, max_head = 0, max_tail = 0;
    for (int q = 0; q < nq; ++q) {
        const int rows = plan[3 * (size_t)q], head = plan[3 * (size_t)q + 1];
        max_rows = std::max(max_rows, rows);
        max_head = std::max(max_head, head);
        max_tail = std::max(max_tail, rows - head);
        st->info.probed_rows += rows;
    }
    // segment capacities: every record -- the longest query's rows; thresholded -- the longest head and 8 nn + 256 slots of tail.  The tail's size is a bet
    // on speed (lists are probed nearest first, so few of the tail's rows pass the head's nn-th distance), never on the answer: an overflow is redone
    const int cap_e = std::max(max_rows, nn);
    const int64_t tail_want = 8 * (int64_t)nn + 256;
    const int tail_cap = (int)std::min<int64_t>(max_tail, tail_want);
    const int cap_t = (int)std::min<int64_t>((int64_t)std::max(max_head, nn) + tail_cap, cap_e);
    const bool thresholded = !(c.flags & LSQ_IVF_EVERY_RECORD) && max_tail > 0;
    const int64_t qb_e = batch_queries(cap_e, c.flags), qb_t = batch_queries(cap_t, c.flags);
    st->info.tail_capacity = thresholded ? tail_cap : 0;
    st->info.batch_queries = std::max<int64_t>(st->info.batch_queries, std::min<int64_t>(thresholded ? qb_t : qb_e, nq));
    std::vector<int> failed, h_fail;
    if (thresholded) {
        for (int q0 = 0; q0 < nq; q0 += (int)qb_t) {
            const int nqb = (int)std::min<int64_t>(qb_t, nq - q0);
            h_fail.assign((size_t)nqb, 0);
            LSQ_TRY(run_batch(c, nullptr, q0, nqb, cap_t, true, h_fail.data()));
            for (int t = 0; t < nqb; ++t) if (h_fail[(size_t)t]) failed.push_back(q0 + t);
        }
        st->info.threshold_queries += nq - (int64_t)failed.size();
        st->info.fallback_queries += (int64_t)failed.size();
        if (!failed.empty()) {
            LSQ_TRY(st->qsel.ensure(sizeof(int) * failed.size()));
            LSQ_HIP(hipMemcpyAsync(st->qsel.p, failed.data(), sizeof(int) * failed.size(), hipMemcpyHostToDevice, s));
            for (size_t f0 = 0; f0 < failed.size(); f0 += (size_t)qb_e) {
                const int nqb = (int)std::min<size_t>((size_t)qb_e, failed.size() - f0);
                LSQ_TRY(run_batch(c, st->qsel.as<int>() + f0, 0, nqb, cap_e, false, nullptr));
            }
        }
    } else {
        for (int q0 = 0; q0 < nq; q0 += (int)qb_e) {
            const int nqb = (int)std::min<int64_t>(qb_e, nq - q0);
            LSQ_TRY(run_batch(c, nullptr, q0, nqb, cap_e, false, nullptr));
        }
    }
    return LSQ_OK;
}

}  // namespace

int lsq_ivf_search(hipStream_t s, lsq_ivf_state *st, lsq_adc_state **adc, const float *K, float *dists, int *ids, const float *q_scan,
                   const float *q_coarse, int64_t ldc, int nq, int nprobe, int nn, int flags, const lsq_search_opts &coarse, int timed,
                   const lsq_filter_view *flt) {
    st->info = lsq_ivf_info{};
    // chunks of queries whose per-(query, probe) words stay below 2^28
    int64_t qc = (int64_t)(1u << 28) / ((int64_t)nprobe + 1);
    if (qc < 1) qc = 1;
    for (int64_t c0 = 0; c0 < nq; c0 += qc) {
        Chunk c{};
        c.s = s; c.st = st; c.adc = adc;
        c.nq = (int)std::min<int64_t>(qc, nq - c0); c.nprobe = nprobe; c.nn = nn; c.flags = flags; c.idbits = lsq_adc_idbits(st->n); c.timed = timed != 0;
        c.in = lsq_search_input{};
        c.in.kind = LSQ_SEARCH_LSQ; c.in.Q = q_scan + c0 * st->d; c.in.qstride = st->d; c.in.K = K; c.in.n = (int)st->n; c.in.m = st->m; c.in.d = st->d;
        c.dists = dists + c0 * nn; c.ids = ids + c0 * nn;
        c.lbits = flt ? flt->lbits : nullptr; c.lpre = flt ? flt->lpre : nullptr;
        LSQ_TRY(run_chunk(c, q_coarse + c0 * ldc, ldc, coarse));
    }
    st->info.queries = nq;
    LSQ_HIP(hipStreamSynchronize(s));
    return LSQ_OK;
}

// ---- the host checker and engine-less road: the contract on plain arrays, rows walked in their original order ------------------------------------------
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

struct IvfCpu {
    float *dists; int *ids;
    const uint8_t *codes; const float *K, *dbnorms, *cent; const int32_t *lor; const float *q_scan, *q_coarse;
    int n, m, h, d, nlist, ldq, nprobe, nn, add;
};

void ivf_queries(const IvfCpu a, int q0, int q1) {
    const int total = a.m * a.h;
    std::vector<float> table((size_t)total), coarse((size_t)a.nlist);
    std::vector<uint64_t> ckeys((size_t)a.nlist), heap;
    std::vector<char> probed((size_t)a.nlist);
    heap.reserve((size_t)a.nn + 1);
    for (int q = q0; q < q1; ++q) {
        const float *qc = a.q_coarse + (size_t)q * a.ldq, *qs = a.q_scan + (size_t)q * a.ldq;
        for (int l = 0; l < a.nlist; ++l) {                          // lsq_knn_exact_cpu's distance
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
        for (int j = 0; j < total; ++j) {                            // lsq_linscan_aqd_query_extra_byte's table
            const float *c = a.K + (size_t)j * a.d;
            float t = 0.0f;
            for (int k = 0; k < a.d; ++k) t -= 2 * qs[k] * c[k];
            table[(size_t)j] = t;
        }
        heap.clear();
        for (int i = 0; i < a.n; ++i) {
            const int l = a.lor[i];
            if (!probed[(size_t)l]) continue;
            const uint8_t *code = a.codes + (size_t)i * a.m;
            float acc = 0.0f;
            for (int k = 0; k < a.m; ++k) acc += table[(size_t)a.h * k + code[k]];
            acc += a.dbnorms[i];
            if (a.add) acc += coarse[(size_t)l];
            const uint64_t cand = ((uint64_t)host_key(acc) << 32) | (uint32_t)(i + 1);      // ids are 1-based
            if ((int)heap.size() < a.nn) {
                heap.push_back(cand);
                std::push_heap(heap.begin(), heap.end());
            } else if (cand < heap.front()) {
                std::pop_heap(heap.begin(), heap.end());
                heap.back() = cand;
                std::push_heap(heap.begin(), heap.end());
            }
        }
        std::sort_heap(heap.begin(), heap.end());
        for (int r = 0; r < a.nn; ++r) {
            const bool have = r < (int)heap.size();
            a.dists[(size_t)q * a.nn + r] = have ? host_unkey((uint32_t)(heap[(size_t)r] >> 32)) : __builtin_inff();
            a.ids[(size_t)q * a.nn + r] = have ? (int)(uint32_t)heap[(size_t)r] : 0;
        }
    }
}

}  // namespace

extern "C" int lsq_ivf_search_cpu(float *dists, int *ids, const uint8_t *codes, const float *codebooks, const float *dbnorms, const float *centroids,
                                  const int32_t *list_of_row, const float *q_scan, const float *q_coarse, int n, int m, int h, int d, int nlist, int nq,
                                  int ldq, int nprobe, int nn, int flags, int nthreads) {
    const char *fn = "lsq_ivf_search_cpu";
    if (n < 1 || m < 1 || h < 1 || h > 256 || d < 1 || nq < 0 || ldq < d || nn < 1) {
        lsq_set_error("%s: bad shape n=%d m=%d h=%d d=%d nq=%d ldq=%d nn=%d", fn, n, m, h, d, nq, ldq, nn);
        return LSQ_EINVAL;
    }
    if (nlist < 1 || nlist > (1 << 24)) { lsq_set_error("%s: needs 1 <= nlist <= 2^24 (got %d)", fn, nlist); return LSQ_EINVAL; }
    if (nprobe < 1 || nprobe > nlist) { lsq_set_error("%s: needs 1 <= nprobe <= nlist (got nprobe=%d nlist=%d)", fn, nprobe, nlist); return LSQ_EINVAL; }
    if (flags & ~IVF_FLAGS) { lsq_set_error("%s: unknown flags %d", fn, flags); return LSQ_EINVAL; }
    if (!dists || !ids || !codes || !codebooks || !dbnorms || !centroids || !list_of_row || !q_scan) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    for (int i = 0; i < n; ++i)
        if (list_of_row[i] < 0 || list_of_row[i] >= nlist) {
            lsq_set_error("%s: list_of_row[%d] = %d lies outside [0, %d)", fn, i, list_of_row[i], nlist);
            return LSQ_EINVAL;
        }
    if (nq == 0) return LSQ_OK;
    const IvfCpu a{dists, ids, codes, codebooks, dbnorms, centroids, list_of_row, q_scan, q_coarse ? q_coarse : q_scan,
                   n, m, h, d, nlist, ldq, nprobe, nn, (flags & LSQ_IVF_ADD_COARSE) ? 1 : 0};
    int nt = nthreads > 0 ? nthreads : (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if (nt > nq) nt = nq;
    std::vector<std::thread> pool;
    pool.reserve((size_t)nt);
    for (int t = 0; t < nt; ++t) pool.emplace_back(ivf_queries, a, (int)((int64_t)nq * t / nt), (int)((int64_t)nq * (t + 1) / nt));
    for (auto &th : pool) th.join();
    return LSQ_OK;
}
