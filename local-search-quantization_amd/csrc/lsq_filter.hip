// lsq_filter.hip -- row filters on a resident index ON THE DEVICE (gfx950): the set A of allowed rows in the forms the scans read.
//
// The reference has no counterpart (its scan, src/linscan/Linscan.jl:46-73, answers over every code).  A filter is state of the index, always an owned
// copy, built once per lsq_index_set_filter from any of three inputs and kept in four forms:
//
//   bits   [ceil(n/32)] uint32, bit (i & 31) of word i >> 5 = row i is allowed; the bits at and past n are zero.  The DENSE road of the scans reads the
//          word of a row beside its code: consecutive lanes read consecutive rows, one dword per 32 rows.
//   pre    [ceil(n/32) + 1] int32, the exclusive prefix of the words' popcounts (hipcub's scan); pre[last] = |A|.
//   rows   [|A|] int32, the allowed rows ascending: word w writes its set bits from pre[w] on -- no atomic decides a position, the same array on every
//          call.  The COMPACT road of the scans walks it instead of 0 .. n-1.
//   lbits  the bitmap in the ORDER OF THE INVERTED LAYOUT (bit p = allowed(ids[p])) with its own prefix lpre, present while the index has inverted lists:
//          the IVF scan reads the bit of layout row p without a dependent gather through ids, and the allowed rows of list l are
//          P(off[l + 1]) - P(off[l]),  P(p) = lpre[p >> 5] + popc(lbits[p >> 5] & ((1 << (p & 31)) - 1)).
//
// Inputs: BYTES -> bits by one ballot per 64 rows; IDS -> a range check (the one kernel that reads the entries counts the bad ones and turns none of them
// into an address), then atomicOr into zeroed words (OR commutes: the same bits on every call, duplicates are harmless); BITS -> copied.  DENY inverts the
// words; the bits at and past n are then zeroed in the last word.  Everything is built into fresh buffers and swapped in at the end, so a refused call
// leaves the former filter in force.  lsq_index_remove (further down) is a fourth input: the bitmap in force copied, the given rows' bits cleared with
// atomicAnd by the one kernel that reads the ids, then the same finish / prefix / row-list kernels and the same swap.
#include <hipcub/hipcub.hpp>

#include <utility>

#include "lsq_internal.h"

namespace {

constexpr int FLT_THREADS = 256;

// words[i >> 5] bit (i & 31) = pred(i), i < n: one ballot per 64 rows, lane 0 writes the wave's two words
template <class Pred>
__device__ inline void flt_ballot_words(int64_t n, int64_t nwords, uint32_t *__restrict__ words, Pred pred) {
    const int64_t i = (int64_t)blockIdx.x * FLT_THREADS + threadIdx.x;      // (whole waves: no lane leaves before the ballot)
    const bool v = i < n && pred(i);
    const unsigned long long mask = __ballot(v);
    if ((threadIdx.x & 63) == 0) {
        const int64_t w = (i >> 6) * 2;
        if (w < nwords) words[w] = (uint32_t)mask;
        if (w + 1 < nwords) words[w + 1] = (uint32_t)(mask >> 32);
    }
}

__global__ __launch_bounds__(FLT_THREADS) void flt_bytes_kernel(const uint8_t *__restrict__ bytes, int64_t n, int64_t nwords, uint32_t *__restrict__ words) {
    flt_ballot_words(n, nwords, words, [&](int64_t i) { return bytes[i] != 0; });
}

// layout order: bit p = the bit of the original row ids[p] (0 <= ids[p] < n: the layout's own array)
__global__ __launch_bounds__(FLT_THREADS) void flt_layout_kernel(const int *__restrict__ ids, const uint32_t *__restrict__ bits, int64_t n, int64_t nwords,
                                                                 uint32_t *__restrict__ words) {
    flt_ballot_words(n, nwords, words, [&](int64_t p) {
        const int row = ids[p];
        return ((bits[row >> 5] >> (row & 31)) & 1u) != 0;
    });
}

// ids in id_base -> bits; *bad += entries outside [id_base, id_base + n): counted, never used as an address
__global__ __launch_bounds__(FLT_THREADS) void flt_ids_kernel(const int32_t *__restrict__ ids, int64_t count, int id_base, int64_t n,
                                                              uint32_t *__restrict__ words, unsigned *__restrict__ bad) {
    const int64_t t = (int64_t)blockIdx.x * FLT_THREADS + threadIdx.x;
    if (t >= count) return;
    const int64_t row = (int64_t)ids[t] - id_base;
    if (row < 0 || row >= n) { atomicAdd(bad, 1u); return; }
    atomicOr(&words[row >> 5], 1u << (row & 31));
}

// lsq_index_remove: ids in id_base -> their bits CLEARED in a copy of the bitmap in force (AND commutes: the same bits on every call, duplicates and
// rows already removed are harmless); *bad += entries outside [id_base, id_base + n): counted, never used as an address
__global__ __launch_bounds__(FLT_THREADS) void flt_remove_kernel(const int32_t *__restrict__ ids, int64_t count, int id_base, int64_t n,
                                                                 uint32_t *__restrict__ words, unsigned *__restrict__ bad) {
    const int64_t t = (int64_t)blockIdx.x * FLT_THREADS + threadIdx.x;
    if (t >= count) return;
    const int64_t row = (int64_t)ids[t] - id_base;
    if (row < 0 || row >= n) { atomicAdd(bad, 1u); return; }
    atomicAnd(&words[row >> 5], ~(1u << (row & 31)));
}

// DENY: inverted; the bits at and past n zeroed; cnt[w] = popcount, cnt[nwords] = 0 (the scan's last output is then the total)
__global__ __launch_bounds__(FLT_THREADS) void flt_finish_kernel(uint32_t *__restrict__ words, int64_t n, int64_t nwords, int deny, int *__restrict__ cnt) {
    const int64_t w = (int64_t)blockIdx.x * FLT_THREADS + threadIdx.x;
    if (w > nwords) return;
    if (w == nwords) { cnt[w] = 0; return; }
    uint32_t v = words[w];
    if (deny) v = ~v;
    if (w == nwords - 1 && (n & 31) != 0) v &= (1u << (n & 31)) - 1u;
    words[w] = v;
    cnt[w] = __popc(v);
}

// rows[pre[w] ..] = the set bits of word w, ascending
__global__ __launch_bounds__(FLT_THREADS) void flt_compact_kernel(const uint32_t *__restrict__ words, const int *__restrict__ pre, int64_t nwords,
                                                                  int *__restrict__ rows) {
    const int64_t w = (int64_t)blockIdx.x * FLT_THREADS + threadIdx.x;
    if (w >= nwords) return;
    uint32_t v = words[w];
    int at = pre[w];                                                 // < pre[nwords] = the length of rows
    while (v) {
        const int b = __ffs((int)v) - 1;
        rows[at++] = (int)(w * 32 + b);
        v &= v - 1u;
    }
}

__device__ inline int flt_prefix_at(const uint32_t *__restrict__ lbits, const int *__restrict__ lpre, int p) {
    const int w = p >> 5, b = p & 31;                                // (b == 0: the word is not read -- p may be n, one past the last word)
    return lpre[w] + (b ? __popc(lbits[w] & ((1u << b) - 1u)) : 0);
}

// *none += lists without an allowed row
__global__ __launch_bounds__(FLT_THREADS) void flt_lists_kernel(const uint32_t *__restrict__ lbits, const int *__restrict__ lpre, const int *__restrict__ off,
                                                                int nlist, unsigned *__restrict__ none) {
    const int l = blockIdx.x * FLT_THREADS + threadIdx.x;
    if (l >= nlist) return;
    if (flt_prefix_at(lbits, lpre, off[l + 1]) == flt_prefix_at(lbits, lpre, off[l])) atomicAdd(none, 1u);
}

struct FilterBufs {
    DevBuf bits, pre, rows;
    void release() { bits.release(); pre.release(); rows.release(); }
};

int exclusive_sum(hipStream_t s, DevBuf &tmp, const int *in, int *out, int64_t items) {
    size_t bytes = 0;
    LSQ_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, (int)items, s));
    LSQ_TRY(tmp.ensure(bytes > 0 ? bytes : 16));
    LSQ_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, bytes, in, out, (int)items, s));
    return LSQ_OK;
}

unsigned blocks_for(int64_t items) { return (unsigned)((items + FLT_THREADS - 1) / FLT_THREADS); }

}  // namespace

struct lsq_filter_state {
    bool active = false;
    int64_t n = 0, allowed = 0;
    int force = 0;
    FilterBufs cur, next;                            // the filter in force; the one a set call is building
    DevBuf lbits, lpre;                              // layout order (with inverted lists)
    DevBuf lrows;                                    // lsq_index_compact: the set bits of lbits, ascending -- the compact form of the layout, for one call
    int nlist = 0;
    int64_t lists_without = 0;
    DevBuf cnt, tmp, flag, stage;                    // popcounts, the scan's workspace, a counter, a host input's staging
    int road = 0;
};

void lsq_filter_free(lsq_filter_state *st) {
    if (!st) return;
    st->cur.release(); st->next.release();
    DevBuf *all[] = {&st->lbits, &st->lpre, &st->lrows, &st->cnt, &st->tmp, &st->flag, &st->stage};
    for (DevBuf *b : all) b->release();
    delete st;
}

bool lsq_filter_active(const lsq_filter_state *st) { return st && st->active; }

void lsq_filter_clear(lsq_filter_state *st) {
    if (!st) return;
    st->active = false; st->allowed = 0; st->force = 0; st->lists_without = 0; st->road = 0;
}

lsq_filter_view lsq_filter_get(const lsq_filter_state *st) {
    lsq_filter_view v;
    if (!lsq_filter_active(st)) return v;
    v.bits = st->cur.bits.as<uint32_t>();
    v.rows = st->cur.rows.as<int>();
    v.pre = st->cur.pre.as<int>();
    v.allowed = st->allowed;
    v.force = st->force;
    if (st->nlist > 0) { v.lbits = st->lbits.as<uint32_t>(); v.lpre = st->lpre.as<int>(); }
    return v;
}

void lsq_filter_note_road(lsq_filter_state *st, int road) { if (st) st->road = road; }

void lsq_filter_get_info(const lsq_filter_state *st, int64_t n, lsq_filter_info *out) {
    *out = lsq_filter_info{};
    out->n = n;
    out->crossover_rows = lsq_filter_crossover(n);
    if (!st) return;
    out->road = st->road;
    if (!st->active) return;
    out->active = 1;
    out->allowed = st->allowed;
    out->lists = st->nlist;
    out->lists_without_allowed = st->nlist > 0 ? st->lists_without : 0;
}

int lsq_filter_set(hipStream_t s, lsq_filter_state **pst, int64_t n, const lsq_filter_desc *desc) {
    const char *fn = "lsq_index_set_filter";
    if (!desc->data) { lsq_set_error("%s: null data", fn); return LSQ_EINVAL; }
    if (desc->form != LSQ_FILTER_BITS && desc->form != LSQ_FILTER_BYTES && desc->form != LSQ_FILTER_IDS) {
        lsq_set_error("%s: unknown form %d", fn, desc->form);
        return LSQ_EINVAL;
    }
    const int known = LSQ_FILTER_DENY | LSQ_FILTER_FORCE_DENSE | LSQ_FILTER_FORCE_COMPACT;
    if (desc->flags & ~known) { lsq_set_error("%s: unknown flags %d", fn, desc->flags); return LSQ_EINVAL; }
    if ((desc->flags & LSQ_FILTER_FORCE_DENSE) && (desc->flags & LSQ_FILTER_FORCE_COMPACT)) {
        lsq_set_error("%s: LSQ_FILTER_FORCE_DENSE and LSQ_FILTER_FORCE_COMPACT together", fn);
        return LSQ_EINVAL;
    }
    if (desc->form == LSQ_FILTER_IDS) {
        if (desc->count < 0 || desc->count > (int64_t)INT32_MAX) { lsq_set_error("%s: needs 0 <= count <= 2^31 - 1 (got %lld)", fn, (long long)desc->count); return LSQ_EINVAL; }
        if (desc->id_base != 0 && desc->id_base != 1) { lsq_set_error("%s: id_base must be 0 or 1 (got %d)", fn, desc->id_base); return LSQ_EINVAL; }
    }
    if (!*pst) *pst = new lsq_filter_state();
    lsq_filter_state *st = *pst;
    const int64_t nwords = (n + 31) / 32;
    FilterBufs &nb = st->next;
    LSQ_TRY(nb.bits.ensure(sizeof(uint32_t) * (size_t)nwords));
    LSQ_TRY(nb.pre.ensure(sizeof(int) * ((size_t)nwords + 1)));
    LSQ_TRY(st->cnt.ensure(sizeof(int) * ((size_t)nwords + 1)));
    LSQ_TRY(st->flag.ensure(sizeof(unsigned)));
    uint32_t *words = nb.bits.as<uint32_t>();
    // the caller's array where the device reads it
    const size_t in_bytes = desc->form == LSQ_FILTER_BITS ? sizeof(uint32_t) * (size_t)nwords
                            : desc->form == LSQ_FILTER_BYTES ? (size_t)n : sizeof(int32_t) * (size_t)desc->count;
    const void *din = desc->data;
    if (!desc->on_device && desc->form != LSQ_FILTER_BITS && in_bytes > 0) {
        LSQ_TRY(st->stage.ensure(in_bytes));
        LSQ_HIP(hipMemcpyAsync(st->stage.p, desc->data, in_bytes, hipMemcpyHostToDevice, s));
        din = st->stage.p;
    }
    unsigned bad = 0;
    if (desc->form == LSQ_FILTER_BITS) {
        LSQ_HIP(hipMemcpyAsync(words, desc->data, in_bytes, desc->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    } else if (desc->form == LSQ_FILTER_BYTES) {
        hipLaunchKernelGGL(flt_bytes_kernel, dim3(blocks_for(n)), dim3(FLT_THREADS), 0, s, static_cast<const uint8_t *>(din), n, nwords, words);
        LSQ_HIP(hipGetLastError());
    } else {
        LSQ_HIP(hipMemsetAsync(words, 0, sizeof(uint32_t) * (size_t)nwords, s));
        LSQ_HIP(hipMemsetAsync(st->flag.p, 0, sizeof(unsigned), s));
        if (desc->count > 0) {
            hipLaunchKernelGGL(flt_ids_kernel, dim3(blocks_for(desc->count)), dim3(FLT_THREADS), 0, s, static_cast<const int32_t *>(din), desc->count,
                               desc->id_base, n, words, st->flag.as<unsigned>());
            LSQ_HIP(hipGetLastError());
        }
        LSQ_HIP(hipMemcpyAsync(&bad, st->flag.p, sizeof(bad), hipMemcpyDeviceToHost, s));
        LSQ_HIP(hipStreamSynchronize(s));
        if (bad) {
            lsq_set_error("%s: %u ids lie outside [%d, %lld)", fn, bad, desc->id_base, (long long)(desc->id_base + n));
            return LSQ_EINVAL;
        }
    }
    hipLaunchKernelGGL(flt_finish_kernel, dim3(blocks_for(nwords + 1)), dim3(FLT_THREADS), 0, s, words, n, nwords, (desc->flags & LSQ_FILTER_DENY) ? 1 : 0,
                       st->cnt.as<int>());
    LSQ_HIP(hipGetLastError());
    LSQ_TRY(exclusive_sum(s, st->tmp, st->cnt.as<int>(), nb.pre.as<int>(), nwords + 1));
    int allowed = 0;
    LSQ_HIP(hipMemcpyAsync(&allowed, nb.pre.as<int>() + nwords, sizeof(int), hipMemcpyDeviceToHost, s));
    LSQ_HIP(hipStreamSynchronize(s));
    LSQ_TRY(nb.rows.ensure(sizeof(int) * (size_t)(allowed > 0 ? allowed : 1)));
    hipLaunchKernelGGL(flt_compact_kernel, dim3(blocks_for(nwords)), dim3(FLT_THREADS), 0, s, words, nb.pre.as<int>(), nwords, nb.rows.as<int>());
    LSQ_HIP(hipGetLastError());
    LSQ_HIP(hipStreamSynchronize(s));
    // the new filter is whole: it takes the place of the former one
    std::swap(st->cur, st->next);
    st->active = true; st->n = n; st->allowed = allowed;
    st->force = desc->flags & (LSQ_FILTER_FORCE_DENSE | LSQ_FILTER_FORCE_COMPACT);
    st->nlist = 0; st->lists_without = 0;            // the layout bits belong to the former filter: lsq_filter_layout rebuilds them
    return LSQ_OK;
}

// ---- lsq_index_add's part: the filter of n_new rows = the one in force and every row from its n on.  Built in the spare buffers like a set call's (the
// bitmap copied and extended: lsq_grow.hip; count, prefix and row list by the kernels above), in force at the commit
int lsq_filter_grow(hipStream_t s, lsq_filter_state *st, int64_t n_new) {
    if (!lsq_filter_active(st) || n_new <= st->n) return LSQ_OK;
    const int64_t nwords = (n_new + 31) / 32, owords = (st->n + 31) / 32, allowed = st->allowed + (n_new - st->n);
    FilterBufs &nb = st->next;
    LSQ_TRY(nb.bits.ensure(sizeof(uint32_t) * (size_t)nwords));
    LSQ_TRY(nb.pre.ensure(sizeof(int) * ((size_t)nwords + 1)));
    LSQ_TRY(nb.rows.ensure(sizeof(int) * (size_t)allowed));
    LSQ_TRY(st->cnt.ensure(sizeof(int) * ((size_t)nwords + 1)));
    uint32_t *words = nb.bits.as<uint32_t>();
    LSQ_HIP(hipMemsetAsync(words, 0, sizeof(uint32_t) * (size_t)nwords, s));
    LSQ_HIP(hipMemcpyAsync(words, st->cur.bits.p, sizeof(uint32_t) * (size_t)owords, hipMemcpyDeviceToDevice, s));      // (its bits at and past the former n are zero)
    LSQ_TRY(lsq_grow_launch_set_bits(s, words, st->n, n_new));
    hipLaunchKernelGGL(flt_finish_kernel, dim3(blocks_for(nwords + 1)), dim3(FLT_THREADS), 0, s, words, n_new, nwords, 0, st->cnt.as<int>());
    LSQ_HIP(hipGetLastError());
    LSQ_TRY(exclusive_sum(s, st->tmp, st->cnt.as<int>(), nb.pre.as<int>(), nwords + 1));
    hipLaunchKernelGGL(flt_compact_kernel, dim3(blocks_for(nwords)), dim3(FLT_THREADS), 0, s, words, nb.pre.as<int>(), nwords, nb.rows.as<int>());
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

void lsq_filter_grow_commit(lsq_filter_state *st, int64_t n_new) {
    if (!lsq_filter_active(st) || n_new <= st->n) return;
    std::swap(st->cur, st->next);
    st->allowed += n_new - st->n;
    st->n = n_new;
    st->nlist = 0; st->lists_without = 0;            // lsq_filter_layout rebuilds the layout-order bits
}

// ---- lsq_index_remove's part: the filter in force (without one: every row) minus the given rows.  Built in the spare buffers like a set call's: the bitmap
// copied, the bits cleared by the one kernel that reads the ids -- it counts the bad ones and turns none of them into an address; what it writes is the
// spare bitmap, which is nothing until the swap --, then count, prefix and row list by the kernels above
int lsq_filter_remove(hipStream_t s, lsq_filter_state **pst, int64_t n, const int32_t *ids, int64_t count, int id_base, int on_device, unsigned *bad,
                      int64_t *cleared) {
    if (!*pst) *pst = new lsq_filter_state();
    lsq_filter_state *st = *pst;
    const int64_t nwords = (n + 31) / 32;
    FilterBufs &nb = st->next;
    LSQ_TRY(nb.bits.ensure(sizeof(uint32_t) * (size_t)nwords));
    LSQ_TRY(nb.pre.ensure(sizeof(int) * ((size_t)nwords + 1)));
    LSQ_TRY(st->cnt.ensure(sizeof(int) * ((size_t)nwords + 1)));
    LSQ_TRY(st->flag.ensure(sizeof(unsigned)));
    uint32_t *words = nb.bits.as<uint32_t>();
    const int32_t *din = ids;
    if (!on_device) {
        LSQ_TRY(st->stage.ensure(sizeof(int32_t) * (size_t)count));
        LSQ_HIP(hipMemcpyAsync(st->stage.p, ids, sizeof(int32_t) * (size_t)count, hipMemcpyHostToDevice, s));
        din = st->stage.as<int32_t>();
    }
    if (st->active) LSQ_HIP(hipMemcpyAsync(words, st->cur.bits.p, sizeof(uint32_t) * (size_t)nwords, hipMemcpyDeviceToDevice, s));
    else LSQ_HIP(hipMemsetAsync(words, 0xff, sizeof(uint32_t) * (size_t)nwords, s));      // (the bits at and past n: zeroed by the finish kernel)
    LSQ_HIP(hipMemsetAsync(st->flag.p, 0, sizeof(unsigned), s));
    hipLaunchKernelGGL(flt_remove_kernel, dim3(blocks_for(count)), dim3(FLT_THREADS), 0, s, din, count, id_base, n, words, st->flag.as<unsigned>());
    LSQ_HIP(hipGetLastError());
    LSQ_HIP(hipMemcpyAsync(bad, st->flag.p, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    LSQ_HIP(hipStreamSynchronize(s));
    if (*bad) return LSQ_OK;                          // the caller refuses: only the spare bitmap was written
    hipLaunchKernelGGL(flt_finish_kernel, dim3(blocks_for(nwords + 1)), dim3(FLT_THREADS), 0, s, words, n, nwords, 0, st->cnt.as<int>());
    LSQ_HIP(hipGetLastError());
    LSQ_TRY(exclusive_sum(s, st->tmp, st->cnt.as<int>(), nb.pre.as<int>(), nwords + 1));
    int allowed = 0;
    LSQ_HIP(hipMemcpyAsync(&allowed, nb.pre.as<int>() + nwords, sizeof(int), hipMemcpyDeviceToHost, s));
    LSQ_HIP(hipStreamSynchronize(s));
    LSQ_TRY(nb.rows.ensure(sizeof(int) * (size_t)(allowed > 0 ? allowed : 1)));
    hipLaunchKernelGGL(flt_compact_kernel, dim3(blocks_for(nwords)), dim3(FLT_THREADS), 0, s, words, nb.pre.as<int>(), nwords, nb.rows.as<int>());
    LSQ_HIP(hipGetLastError());
    LSQ_HIP(hipStreamSynchronize(s));
    *cleared = (st->active ? st->allowed : n) - allowed;
    std::swap(st->cur, st->next);
    if (!st->active) st->force = 0;                   // a FORCE flag of the filter in force stays in force
    st->active = true; st->n = n; st->allowed = allowed;
    st->nlist = 0; st->lists_without = 0;            // lsq_filter_layout rebuilds the layout-order bits
    return LSQ_OK;
}

// ---- lsq_index_compact's part: the compact form of the layout -- the positions of the allowed rows, ascending -- from the layout-order bitmap and its
// prefix by the kernel that makes the row list; lpre[nwords] = their number = allowed
int lsq_filter_layout_rows(hipStream_t s, lsq_filter_state *st, int64_t n, const int **lsel) {
    if (!lsq_filter_active(st) || st->nlist < 1) { lsq_set_error("lsq_index_compact: the filter has no bits in layout order"); return LSQ_EINVAL; }
    const int64_t nwords = (n + 31) / 32;
    LSQ_TRY(st->lrows.ensure(sizeof(int) * (size_t)(st->allowed > 0 ? st->allowed : 1)));
    hipLaunchKernelGGL(flt_compact_kernel, dim3(blocks_for(nwords)), dim3(FLT_THREADS), 0, s, st->lbits.as<uint32_t>(), st->lpre.as<int>(), nwords, st->lrows.as<int>());
    LSQ_HIP(hipGetLastError());
    *lsel = st->lrows.as<int>();
    return LSQ_OK;
}

int lsq_filter_layout(hipStream_t s, lsq_filter_state *st, const int *ids, const int *off, int64_t n, int nlist) {
    if (!st) return LSQ_OK;
    st->nlist = 0; st->lists_without = 0;
    if (!st->active || nlist < 1 || !ids || !off) return LSQ_OK;
    const int64_t nwords = (n + 31) / 32;
    LSQ_TRY(st->lbits.ensure(sizeof(uint32_t) * (size_t)nwords));
    LSQ_TRY(st->lpre.ensure(sizeof(int) * ((size_t)nwords + 1)));
    LSQ_TRY(st->cnt.ensure(sizeof(int) * ((size_t)nwords + 1)));
    LSQ_TRY(st->flag.ensure(sizeof(unsigned)));
    hipLaunchKernelGGL(flt_layout_kernel, dim3(blocks_for(n)), dim3(FLT_THREADS), 0, s, ids, st->cur.bits.as<uint32_t>(), n, nwords, st->lbits.as<uint32_t>());
    hipLaunchKernelGGL(flt_finish_kernel, dim3(blocks_for(nwords + 1)), dim3(FLT_THREADS), 0, s, st->lbits.as<uint32_t>(), n, nwords, 0, st->cnt.as<int>());
    LSQ_HIP(hipGetLastError());
    LSQ_TRY(exclusive_sum(s, st->tmp, st->cnt.as<int>(), st->lpre.as<int>(), nwords + 1));
    LSQ_HIP(hipMemsetAsync(st->flag.p, 0, sizeof(unsigned), s));
    hipLaunchKernelGGL(flt_lists_kernel, dim3(blocks_for(nlist)), dim3(FLT_THREADS), 0, s, st->lbits.as<uint32_t>(), st->lpre.as<int>(), off, nlist,
                       st->flag.as<unsigned>());
    LSQ_HIP(hipGetLastError());
    unsigned none = 0;
    LSQ_HIP(hipMemcpyAsync(&none, st->flag.p, sizeof(none), hipMemcpyDeviceToHost, s));
    LSQ_HIP(hipStreamSynchronize(s));
    st->nlist = nlist; st->lists_without = (int64_t)none;
    return LSQ_OK;
}
