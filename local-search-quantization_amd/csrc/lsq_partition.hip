// lsq_partition.hip -- the coarse partition of a residual inverted-list index ON THE DEVICE (gfx950): what lies between a base set in HBM and an index whose
// rows encode x - c_l (include/lsq_mi355x.h, section 3i).
//
// The reference has no counterpart: it neither partitions its base nor encodes residuals.  The search side is lsq_ivf.hip (LSQ_IVF_ADD_COARSE); the trainer
// and the encoder that run on the residuals are the resident ones, unchanged.  This file holds the four steps they leave open and their host checkers:
//
//   ASSIGN      no kernel of its own: the exact search of lsq_knn.hip with the centroids as base and one neighbour, through a base-only lsq_index that borrows
//               the handle's centroid buffer (so an update is seen by the next assign without a copy).
//   UPDATE      one Lloyd half-step whose bits are numpy's: per (list, dimension) a chain of float64 adds in ascending row id, from +0.0, divided by the count
//               in float64, rounded to f32.  The rows are grouped by the radix sort lsq_index_set_lists uses (lsq_rows_*: stable, no atomics); a block then
//               owns ONE list and up to 256 dimensions, a lane one dimension: a row is read by consecutive lanes (512 contiguous bytes at d = 128, f32), the
//               row ids one coalesced load per batch, handed from lane to scalar register.  The chain is sequential by contract, the loads are not: UPD_PREFETCH rows are in flight while the
//               previous UPD_PREFETCH are added.  What bounds it: a list of L rows is L dependent v_add_f64 (a handful of cycles each) behind L / UPD_PREFETCH
//               load round trips; with balanced lists (n / nlist rows, nlist blocks per 256 dimensions) the chip is full and the bound is the gather of n rows
//               from HBM; with one giant list it is that list's chain on ONE block (DESIGN 4.21 says what was measured).
//   RESIDUALS   R[i][t] = x_it - c_{l_i, t}, one rounded subtraction.  A streaming kernel: n d (4 or 1) bytes in, 4 n d bytes out, the centroid rows from L2
//               (nlist d floats: 512 KB at nlist = 1024, d = 128).  A thread owns four components of a row, so consecutive lanes read consecutive pieces
//               and write consecutive 16 bytes.  The loader follows lsq_xload.h: by what the base pointer and the pitch in bytes are both multiples of,
//               an f32 piece is one 16-byte load or four dwords, a uint8 piece one dword or four bytes; the row's last, partial piece is read element
//               by element and nothing past the d-th component is touched, in X or in R.
//   CODE_NORMS  quantize_norms_kernel's loop (lsq_norms.hip: the same reconstruction order, the same chain a) with a second chain b = SUM c_t r^_t beside it
//               and s = a + (b + b); then that kernel's nearest-scalar rule.  One thread per row, codeword and centroid rows from L2.
//
// A list_of_row entry outside [0, nlist) is never used as an offset: UPDATE finds it in ivf_keys_kernel before anything is sorted, the other two kernels
// test the entry they have just read, count it and skip the row; the host turns a non-zero count into LSQ_EINVAL.
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "lsq_internal.h"
#include "lsq_xload.h"

#pragma clang fp contract(off)

namespace {

constexpr int PT_THREADS = 256;
constexpr int UPD_PREFETCH = 32;             // (a power of two <= 64) rows of a list whose loads are in flight ahead of the float64 chain (tests walk lists of 1 .. 2 * 32 + 1 rows)

// ---- residuals ----------------------------------------------------------------------------------------------------------------------------------------------
// A thread owns FOUR components of a row (ppr = pieces per row), whatever the element type: consecutive lanes then write consecutive 16 bytes of R, 1 KiB per
// wave and store instruction.  ALIGN: how the piece is read -- f32: one 16-byte load or four dwords; uint8: one dword or four bytes -- by what the base
// pointer and the row pitch in bytes are both multiples of.  (uint8 rows are not read 16 bytes per lane even where they could be: such a lane has 64 bytes to
// write, 16 every 64 per store instruction; exchanging the results inside a quad of lanes first mends the stores and measured 0.238 ms at 10^6 x 128 against
// 0.160 ms for the dword road: DESIGN 4.21.)  cvec / rvec: the centroid rows / the rows of R may be read / written 16 bytes at a time
template <typename T, int ALIGN>
__global__ __launch_bounds__(PT_THREADS) void residual_kernel(const T *__restrict__ X, int64_t ldx, int64_t n, int d, const float *__restrict__ cent, int nlist,
                                                              const int32_t *__restrict__ lor, float *__restrict__ R, int64_t ldr, int ppr, int cvec, int rvec,
                                                              unsigned *__restrict__ bad) {
    const int64_t g = (int64_t)blockIdx.x * PT_THREADS + threadIdx.x;
    const int64_t i = g / ppr;
    if (i >= n) return;
    const int k0 = (int)(g - i * ppr) * 4;
    const int32_t l = lor[i];
    if (l < 0 || l >= nlist) {                                       // counted once per row, never an offset
        if (k0 == 0) atomicAdd(bad, 1u);
        return;
    }
    const T *__restrict__ x = X + i * ldx + k0;
    const float *__restrict__ c = cent + (int64_t)l * d + k0;
    float *__restrict__ r = R + i * ldr + k0;
    const int left = d - k0;                                         // >= 1: components of the row from k0 on
    if (left >= 4) {
        lsq_f32x4 xv, cv;
        if constexpr (sizeof(T) == 4) {
            if constexpr (ALIGN == 16) {
                xv = lsq_ld4_nt(x);
            } else {
                xv.x = __builtin_nontemporal_load(x); xv.y = __builtin_nontemporal_load(x + 1);
                xv.z = __builtin_nontemporal_load(x + 2); xv.w = __builtin_nontemporal_load(x + 3);
            }
        } else {
            if constexpr (ALIGN >= 4) xv = lsq_ld4_nt(x);             // one dword, widened in registers
            else xv = lsq_widen4((uint32_t)x[0] | ((uint32_t)x[1] << 8) | ((uint32_t)x[2] << 16) | ((uint32_t)x[3] << 24));
        }
        if (cvec) {
            cv = *reinterpret_cast<const lsq_f32x4 *>(c);
        } else {
            cv.x = c[0]; cv.y = c[1]; cv.z = c[2]; cv.w = c[3];
        }
        const lsq_f32x4 v = xv - cv;                                 // four rounded subtractions
        if (rvec) {
            __builtin_nontemporal_store(v, reinterpret_cast<lsq_f32x4 *>(r));
        } else {
            r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
        }
    } else {                                                         // the row's last, partial piece: element by element, nothing past the d-th component
        for (int k = 0; k < left; ++k) r[k] = (float)x[k] - c[k];
    }
}

template <typename T>
int launch_residuals(hipStream_t s, const T *X, int64_t ldx, int64_t n, int d, const float *cent, int nlist, const int32_t *lor, float *R, int64_t ldr,
                     unsigned *bad, int *loader) {
    const uintptr_t a = (uintptr_t)X | (uintptr_t)(ldx * (int64_t)sizeof(T));
    int align = (a & 15) == 0 ? 16 : ((a & 3) == 0 ? 4 : 1);
    if (sizeof(T) == 1 && align == 16) align = 4;                    // the widest load of a uint8 piece is its dword
    const int ppr = (d + 3) / 4;
    const int cvec = (d & 3) == 0 && ((uintptr_t)cent & 15) == 0;
    const int rvec = (((uintptr_t)R | (uintptr_t)(ldr * (int64_t)sizeof(float))) & 15) == 0;
    const int64_t blocks = (n * ppr + PT_THREADS - 1) / PT_THREADS;  // n < 2^31, ppr <= d / 4 + 1
    if (blocks > (int64_t)INT32_MAX) { lsq_set_error("lsq_partition_residuals: n * d = %lld * %d is beyond one launch", (long long)n, d); return LSQ_EINVAL; }
    const dim3 grid((unsigned)blocks), block(PT_THREADS);
#define PT_LAUNCH(AL) hipLaunchKernelGGL((residual_kernel<T, AL>), grid, block, 0, s, X, ldx, n, d, cent, nlist, lor, R, ldr, ppr, cvec, rvec, bad)
    if (align == 16) PT_LAUNCH(16);
    else if (align == 4) PT_LAUNCH(4);
    else if constexpr (sizeof(T) == 1) PT_LAUNCH(1);
    else { lsq_set_error("lsq_partition_residuals: the f32 rows are not 4-byte aligned"); return LSQ_EINVAL; }
#undef PT_LAUNCH
    LSQ_HIP(hipGetLastError());
    *loader = align;
    return LSQ_OK;
}

// ---- update -------------------------------------------------------------------------------------------------------------------------------------------------
// block (l, y): list l, dimensions y * blockDim.x ..; sorted / off: lsq_rows_sort's keys and lsq_rows_offsets' starts.  stats[0] += empty lists,
// stats[1] = max list length (figures for lsq_partition_info: no result depends on them)
template <typename T>
__global__ __launch_bounds__(PT_THREADS) void update_kernel(const T *__restrict__ X, int64_t ldx, int d, const uint64_t *__restrict__ sorted,
                                                            const int *__restrict__ off, float *__restrict__ cent, int32_t *__restrict__ counts,
                                                            unsigned *__restrict__ stats) {
    const int l = blockIdx.x;
    const int t = blockIdx.y * blockDim.x + threadIdx.x;
    const int b = off[l], e = off[l + 1];
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        if (counts) counts[l] = e - b;
        if (e == b) atomicAdd(&stats[0], 1u);
        else atomicMax(&stats[1], (unsigned)(e - b));
    }
    if (e == b) return;                                              // (block-uniform) a list without rows keeps its centroid's bits
    // Every lane stays to the end -- a lane past the d-th dimension reads dimension d - 1 and stores nothing --, because the row ids travel through the
    // wave: lane j holds the id of the batch's j-th row (one coalesced load per batch) and hands it out by v_readlane, which makes each row's address
    // scalar.  (Ids read at block-uniform addresses become scalar loads whose waits the compiler places between the row loads: four round trips in a row
    // per batch, measured 74 ns per row of the longest list.)
    const T *__restrict__ col = X + (t < d ? t : d - 1);
    const int lane = threadIdx.x & (UPD_PREFETCH - 1);
    const int nbt = (e - b + UPD_PREFETCH - 1) / UPD_PREFETCH;       // batches, the last one maybe short
    auto load_ids = [&](int p) -> int {                              // past the list: its last row again, loaded and never added.  No branch: the
        const int q = p + lane < e ? p + lane : e - 1;               // compiler counts its waits exactly only along straight-line code
        return (int)(uint32_t)sorted[q];
    };
    double acc = 0.0;
    float bufa[UPD_PREFETCH], bufb[UPD_PREFETCH];                    // two batches of rows, filled in turn: no batch is ever copied
    auto fetch = [&](float (&dst)[UPD_PREFETCH], int ids) {
#pragma unroll
        for (int j = 0; j < UPD_PREFETCH; ++j) dst[j] = (float)col[(int64_t)(uint32_t)__builtin_amdgcn_readlane(ids, j) * ldx];
    };
    auto chain = [&](const float (&src)[UPD_PREFETCH], int cnt) {    // cnt: rows of the batch that exist (>= UPD_PREFETCH in every batch but the last)
#pragma unroll
        for (int j = 0; j < UPD_PREFETCH; ++j)
            if (j < cnt) acc = acc + (double)src[j];                 // ascending row id: the order of the sorted keys
    };
    // program order is wait order (loads return in order): the ids of batch k + 2 are asked for BEFORE the rows of batch k + 1, so that waiting for ids
    // never waits for rows, and the rows of batch k + 1 are on their way while those of batch k are still arriving: up to 2 UPD_PREFETCH rows in flight
    const int ids0 = load_ids(b);
    int ids1 = load_ids(b + UPD_PREFETCH);
    fetch(bufa, ids0);
    for (int k = 0; k < nbt; k += 2) {                               // (every branch below is block-uniform)
        if (k + 1 < nbt) {
            const int ids2 = load_ids(b + (k + 2) * UPD_PREFETCH);
            fetch(bufb, ids1);
            ids1 = ids2;
        }
        chain(bufa, e - (b + k * UPD_PREFETCH));
        if (k + 1 >= nbt) break;
        if (k + 2 < nbt) {
            const int ids2 = load_ids(b + (k + 3) * UPD_PREFETCH);
            fetch(bufa, ids1);
            ids1 = ids2;
        }
        chain(bufb, e - (b + (k + 1) * UPD_PREFETCH));
    }
    if (t < d) cent[(int64_t)l * d + t] = (float)(acc / (double)(e - b));
}

template <typename T>
int launch_update(hipStream_t s, const T *X, int64_t ldx, int d, const uint64_t *sorted, const int *off, int nlist, float *cent, int32_t *counts,
                  unsigned *stats) {
    const int threads = d >= PT_THREADS ? PT_THREADS : ((d + 63) / 64) * 64;
    const int ys = (d + threads - 1) / threads;
    if (ys > 65535) { lsq_set_error("lsq_partition_update: d = %d is beyond one launch", d); return LSQ_EINVAL; }
    hipLaunchKernelGGL((update_kernel<T>), dim3((unsigned)nlist, (unsigned)ys), dim3((unsigned)threads), 0, s, X, ldx, d, sorted, off, cent, counts, stats);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

// ---- code_norms ---------------------------------------------------------------------------------------------------------------------------------------------
// one thread per row, as quantize_norms_kernel: m codeword rows and the centroid row streamed along the dimension, 4 dimensions at a time where K allows
__global__ __launch_bounds__(PT_THREADS) void code_norms_kernel(const uint8_t *__restrict__ codes, const float *__restrict__ K, const float *__restrict__ cent,
                                                                int nlist, const int32_t *__restrict__ lor, const float *__restrict__ cb, int ncb, int64_t n,
                                                                int d, int m, float *__restrict__ norms, uint8_t *__restrict__ norm_codes,
                                                                float *__restrict__ dbnorms, unsigned *__restrict__ bad) {
    __shared__ float cbs[LSQ_H];
    if (cb) for (int t = threadIdx.x; t < ncb; t += PT_THREADS) cbs[t] = cb[t];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * PT_THREADS + threadIdx.x;
    if (i >= n) return;
    const int32_t l = lor[i];
    if (l < 0 || l >= nlist) { atomicAdd(bad, 1u); return; }
    const float *row[LSQ_MAX_M];
    for (int j = 0; j < m; ++j) row[j] = K + ((int64_t)j * LSQ_H + codes[i * m + j]) * d;
    const float *__restrict__ c = cent + (int64_t)l * d;
    float a = 0.0f, b = 0.0f;
    const bool vec = (d & 3) == 0 && ((((uintptr_t)K | (uintptr_t)cent) & 15) == 0);
    if (vec) {
        for (int t = 0; t < d; t += 4) {
            lsq_f32x4 acc = *reinterpret_cast<const lsq_f32x4 *>(row[0] + t);
            for (int j = 1; j < m; ++j) acc = acc + *reinterpret_cast<const lsq_f32x4 *>(row[j] + t);      // codebooks ascending
            const lsq_f32x4 cv = *reinterpret_cast<const lsq_f32x4 *>(c + t);
            a = a + acc.x * acc.x; b = b + cv.x * acc.x;                                                  // dimensions ascending; product rounded, then the add
            a = a + acc.y * acc.y; b = b + cv.y * acc.y;
            a = a + acc.z * acc.z; b = b + cv.z * acc.z;
            a = a + acc.w * acc.w; b = b + cv.w * acc.w;
        }
    } else {
        for (int t = 0; t < d; ++t) {
            float acc = row[0][t];
            for (int j = 1; j < m; ++j) acc = acc + row[j][t];
            a = a + acc * acc;
            b = b + c[t] * acc;
        }
    }
    const float sv = a + (b + b);
    if (norms) norms[i] = sv;
    if (!cb) return;
    int best = 0;
    float bd = (sv - cbs[0]) * (sv - cbs[0]);
    for (int j = 1; j < ncb; ++j) {
        const float df = sv - cbs[j], dd = df * df;
        if (dd < bd) { bd = dd; best = j; }                                                              // strict <: the first minimum
    }
    if (norm_codes) norm_codes[i] = (uint8_t)best;
    if (dbnorms) dbnorms[i] = cbs[best];
}

}  // namespace

// ---- the handle ---------------------------------------------------------------------------------------------------------------------------------------------
struct lsq_partition {
    lsq_ctx *ctx = nullptr;
    int nlist = 0, d = 0;
    DevBuf cent;                                       // the centroids: the handle's own copy, replaced in place by update
    lsq_index *ix = nullptr;                           // assign: a base-only index that BORROWS cent (its own scan state and staging)
    lsq_row_groups rows;                               // update: the rows grouped by list
    DevBuf off, words;                                 // update: list starts; the control words of a call (4 unsigned: bad entries, empty lists, longest list)
    DevBuf s_x, s_lor, s_out, s_cnt, s_dist;           // staging of host-buffer calls (and assign's unwanted distances)
    DevBuf s_codes, s_K, s_cb, s_nc, s_dbn;            // code_norms' staging
    PhaseClock<3> clock;
    lsq_partition_info info{};
};

extern "C" int lsq_partition_destroy(lsq_partition *p) {
    if (!p) return LSQ_OK;
    hipStream_t s = nullptr;
    int profile = 0;
    if (lsq_ctx_bind(p->ctx, &s, &profile) == LSQ_OK) (void)hipStreamSynchronize(s);
    (void)lsq_index_destroy(p->ix);
    DevBuf *bufs[] = {&p->cent, &p->off, &p->words, &p->s_x, &p->s_lor, &p->s_out, &p->s_cnt, &p->s_dist, &p->s_codes, &p->s_K, &p->s_cb, &p->s_nc, &p->s_dbn};
    for (DevBuf *b : bufs) b->release();
    p->rows.release();
    p->clock.release();
    delete p;
    return LSQ_OK;
}

extern "C" int lsq_partition_create(lsq_partition **out, lsq_ctx *c, const lsq_partition_desc *desc) {
    const char *fn = "lsq_partition_create";
    if (!out) { lsq_set_error("%s: null out pointer", fn); return LSQ_EINVAL; }
    *out = nullptr;
    if (!c || !desc) { lsq_set_error("%s: null %s", fn, c ? "description" : "context"); return LSQ_EINVAL; }
    if (desc->nlist < 1 || desc->nlist > (1 << 24) || desc->d < 1) {
        lsq_set_error("%s: needs 1 <= nlist <= 2^24 and d >= 1 (got nlist=%d d=%d)", fn, desc->nlist, desc->d);
        return LSQ_EINVAL;
    }
    if (!desc->centroids) { lsq_set_error("%s: null centroids", fn); return LSQ_EINVAL; }
    hipStream_t s = nullptr;
    int profile = 0;
    LSQ_TRY(lsq_ctx_bind(c, &s, &profile));
    lsq_partition *p = new lsq_partition();
    p->ctx = c; p->nlist = desc->nlist; p->d = desc->d;
    auto build = [&]() -> int {
        const size_t bytes = sizeof(float) * (size_t)desc->nlist * (size_t)desc->d;
        LSQ_TRY(p->cent.ensure(bytes));
        LSQ_TRY(p->words.ensure(4 * sizeof(unsigned)));
        LSQ_HIP(hipMemcpyAsync(p->cent.p, desc->centroids, bytes, desc->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        LSQ_HIP(hipStreamSynchronize(s));
        lsq_index_desc id{};
        id.n = desc->nlist; id.d = desc->d; id.base = p->cent.p; id.base_u8 = 0; id.ldb = desc->d; id.on_device = 1;
        return lsq_index_create(&p->ix, c, &id);
    };
    const int rc = build();
    if (rc != LSQ_OK) { (void)lsq_partition_destroy(p); return rc; }
    *out = p;
    return LSQ_OK;
}

extern "C" int lsq_partition_get_centroids(lsq_partition *p, float *out, int on_device) {
    if (!p || !out) { lsq_set_error("lsq_partition_get_centroids: null %s", p ? "pointer" : "partition"); return LSQ_EINVAL; }
    hipStream_t s = nullptr;
    int profile = 0;
    LSQ_TRY(lsq_ctx_bind(p->ctx, &s, &profile));
    LSQ_HIP(hipMemcpyAsync(out, p->cent.p, sizeof(float) * (size_t)p->nlist * (size_t)p->d, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    LSQ_HIP(hipStreamSynchronize(s));
    return LSQ_OK;
}

extern "C" int lsq_partition_get_info(lsq_partition *p, lsq_partition_info *out) {
    if (!p || !out) { lsq_set_error("lsq_partition_get_info: null argument"); return LSQ_EINVAL; }
    *out = p->info;
    return LSQ_OK;
}

namespace {

// the checks every call on rows of X shares; 0 or LSQ_EINVAL with the message set
int rows_check(const char *fn, const lsq_partition *p, const void *X, int x_u8, int64_t n, int64_t ldx) {
    if (!p) { lsq_set_error("%s: null partition", fn); return LSQ_EINVAL; }
    if (n < 0 || n > (int64_t)INT32_MAX - 1) { lsq_set_error("%s: needs 0 <= n <= 2^31 - 2 (got %lld)", fn, (long long)n); return LSQ_EINVAL; }
    if (ldx < p->d) { lsq_set_error("%s: needs ldx >= d (got ldx=%lld d=%d)", fn, (long long)ldx, p->d); return LSQ_EINVAL; }
    if (n > 0 && !X) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    if (!x_u8 && ((uintptr_t)X & 3) != 0) { lsq_set_error("%s: the f32 rows are not 4-byte aligned", fn); return LSQ_EINVAL; }
    return LSQ_OK;
}

// a host-buffer call's rows of X on the device, as they lie (up to the d-th element of the last row); a device call's rows where they are
int stage_rows(hipStream_t s, lsq_partition *p, const void *X, int x_u8, int64_t n, int64_t ldx, int on_device, const void **dX) {
    *dX = X;
    if (on_device) return LSQ_OK;
    const size_t bytes = ((size_t)(n - 1) * (size_t)ldx + (size_t)p->d) * (x_u8 ? 1 : sizeof(float));
    LSQ_TRY(p->s_x.ensure(bytes));
    LSQ_HIP(hipMemcpyAsync(p->s_x.p, X, bytes, hipMemcpyHostToDevice, s));
    *dX = p->s_x.p;
    return LSQ_OK;
}

template <class T>
int stage_array(hipStream_t s, DevBuf &buf, const T *src, size_t count, int on_device, const T **dst) {
    *dst = src;
    if (on_device || !src) return LSQ_OK;
    LSQ_TRY(buf.ensure(sizeof(T) * count));
    LSQ_HIP(hipMemcpyAsync(buf.p, src, sizeof(T) * count, hipMemcpyHostToDevice, s));
    *dst = buf.as<T>();
    return LSQ_OK;
}

// the count of bad entries a kernel left in words[0] -> the host; waits for the stream
int read_words(hipStream_t s, lsq_partition *p, unsigned *w) {
    LSQ_HIP(hipMemcpyAsync(w, p->words.p, 4 * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    LSQ_HIP(hipStreamSynchronize(s));
    return LSQ_OK;
}

int bad_lists(const char *fn, unsigned bad, int nlist) {
    lsq_set_error("%s: %u entries of list_of_row lie outside [0, %d)", fn, bad, nlist);
    return LSQ_EINVAL;
}

}  // namespace

extern "C" int lsq_partition_assign(lsq_partition *p, const void *X, int x_u8, int64_t n, int ldx, int32_t *list_of_row, float *dist, int on_device) {
    const char *fn = "lsq_partition_assign";
    LSQ_TRY(rows_check(fn, p, X, x_u8, n, ldx));
    if (n > 0 && !list_of_row) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    if (n == 0) return LSQ_OK;
    hipStream_t s = nullptr;
    int profile = 0;
    LSQ_TRY(lsq_ctx_bind(p->ctx, &s, &profile));
    std::vector<float> hd;
    float *dd = dist;
    if (!dd) {                                         // the search hands out distances; unwanted ones go to scratch on the call's side
        if (on_device) { LSQ_TRY(p->s_dist.ensure(sizeof(float) * (size_t)n)); dd = p->s_dist.as<float>(); }
        else { hd.resize((size_t)n); dd = hd.data(); }
    }
    // ids [n][1] int32 0-based: the lists as they are
    LSQ_TRY(lsq_index_knn(p->ix, dd, list_of_row, X, x_u8 != 0, (int)n, ldx, 1, 0, on_device));
    if (on_device) LSQ_HIP(hipStreamSynchronize(s));
    lsq_index_knn_info ki{};
    LSQ_TRY(lsq_index_get_knn_info(p->ix, &ki));
    lsq_partition_info info{};
    info.call = LSQ_PARTITION_ASSIGN; info.rows = n;
    info.kernel_ms = ki.norms_ms + ki.scan_ms + ki.select_ms;
    p->info = info;
    return LSQ_OK;
}

extern "C" int lsq_partition_update(lsq_partition *p, const void *X, int x_u8, int64_t n, int ldx, const int32_t *list_of_row, int32_t *counts,
                                    int on_device) {
    const char *fn = "lsq_partition_update";
    LSQ_TRY(rows_check(fn, p, X, x_u8, n, ldx));
    if (n > 0 && !list_of_row) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    hipStream_t s = nullptr;
    int profile = 0;
    LSQ_TRY(lsq_ctx_bind(p->ctx, &s, &profile));
    const int nlist = p->nlist, d = p->d;
    lsq_partition_info info{};
    info.call = LSQ_PARTITION_UPDATE; info.rows = n; info.loader_bytes = x_u8 ? 1 : 4;
    if (n == 0) {                                      // every list is empty: the centroids stay, the counts are zero
        if (counts) {
            if (on_device) { LSQ_HIP(hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)nlist, s)); LSQ_HIP(hipStreamSynchronize(s)); }
            else memset(counts, 0, sizeof(int32_t) * (size_t)nlist);
        }
        info.empty_lists = nlist;
        p->info = info;
        return LSQ_OK;
    }
    const void *dX = nullptr;
    LSQ_TRY(stage_rows(s, p, X, x_u8, n, ldx, on_device, &dX));
    LSQ_TRY(p->clock.begin(profile != 0));
    LSQ_TRY(p->clock.mark(s));
    unsigned bad = 0;
    LSQ_TRY(lsq_rows_keys(s, p->rows, list_of_row, on_device, n, nlist, &bad));
    if (bad) return bad_lists(fn, bad, nlist);         // before the sort, before a centroid is written
    const uint64_t *sorted = nullptr;
    LSQ_TRY(lsq_rows_sort(s, p->rows, n, nlist, &sorted));
    LSQ_TRY(p->off.ensure(sizeof(int) * ((size_t)nlist + 1)));
    LSQ_TRY(lsq_rows_offsets(s, sorted, n, nlist, p->off.as<int>()));
    LSQ_TRY(p->clock.mark(s));
    int32_t *dcounts = counts;
    if (counts && !on_device) { LSQ_TRY(p->s_cnt.ensure(sizeof(int32_t) * (size_t)nlist)); dcounts = p->s_cnt.as<int32_t>(); }
    LSQ_HIP(hipMemsetAsync(p->words.p, 0, 4 * sizeof(unsigned), s));
    unsigned *stats = p->words.as<unsigned>() + 1;
    if (x_u8) LSQ_TRY(launch_update(s, static_cast<const uint8_t *>(dX), (int64_t)ldx, d, sorted, p->off.as<int>(), nlist, p->cent.as<float>(), dcounts, stats));
    else LSQ_TRY(launch_update(s, static_cast<const float *>(dX), (int64_t)ldx, d, sorted, p->off.as<int>(), nlist, p->cent.as<float>(), dcounts, stats));
    LSQ_TRY(p->clock.mark(s));
    if (counts && !on_device) LSQ_HIP(hipMemcpyAsync(counts, dcounts, sizeof(int32_t) * (size_t)nlist, hipMemcpyDeviceToHost, s));
    unsigned w[4];
    LSQ_TRY(read_words(s, p, w));
    float ms[2];
    LSQ_TRY(p->clock.read(ms));
    info.empty_lists = w[1]; info.lists_touched = nlist - (int64_t)w[1]; info.max_list_rows = w[2];
    info.group_ms = ms[0]; info.kernel_ms = ms[1];
    p->info = info;
    return LSQ_OK;
}

extern "C" int lsq_partition_residuals(lsq_partition *p, const void *X, int x_u8, int64_t n, int ldx, const int32_t *list_of_row, float *R, int ldr,
                                       int on_device) {
    const char *fn = "lsq_partition_residuals";
    LSQ_TRY(rows_check(fn, p, X, x_u8, n, ldx));
    if (ldr < p->d) { lsq_set_error("%s: needs ldr >= d (got ldr=%d d=%d)", fn, ldr, p->d); return LSQ_EINVAL; }
    if (n > 0 && (!list_of_row || !R)) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    if (((uintptr_t)R & 3) != 0) { lsq_set_error("%s: R is not 4-byte aligned", fn); return LSQ_EINVAL; }
    if (n == 0) return LSQ_OK;
    hipStream_t s = nullptr;
    int profile = 0;
    LSQ_TRY(lsq_ctx_bind(p->ctx, &s, &profile));
    const int nlist = p->nlist, d = p->d;
    const void *dX = nullptr;
    const int32_t *dlor = nullptr;
    LSQ_TRY(stage_rows(s, p, X, x_u8, n, ldx, on_device, &dX));
    LSQ_TRY(stage_array(s, p->s_lor, list_of_row, (size_t)n, on_device, &dlor));
    float *dR = R;
    int64_t dldr = ldr;
    if (!on_device) {                                  // the host form's rows d floats apart on the device, copied out at the caller's pitch: the gaps are not touched
        LSQ_TRY(p->s_out.ensure(sizeof(float) * (size_t)n * (size_t)d));
        dR = p->s_out.as<float>(); dldr = d;
    }
    LSQ_HIP(hipMemsetAsync(p->words.p, 0, 4 * sizeof(unsigned), s));
    LSQ_TRY(p->clock.begin(profile != 0));
    LSQ_TRY(p->clock.mark(s));
    int loader = 0;
    if (x_u8) LSQ_TRY(launch_residuals(s, static_cast<const uint8_t *>(dX), (int64_t)ldx, n, d, p->cent.as<float>(), nlist, dlor, dR, dldr, p->words.as<unsigned>(), &loader));
    else LSQ_TRY(launch_residuals(s, static_cast<const float *>(dX), (int64_t)ldx, n, d, p->cent.as<float>(), nlist, dlor, dR, dldr, p->words.as<unsigned>(), &loader));
    LSQ_TRY(p->clock.mark(s));
    unsigned w[4];
    LSQ_TRY(read_words(s, p, w));
    if (w[0]) return bad_lists(fn, w[0], nlist);
    if (!on_device) {
        LSQ_HIP(hipMemcpy2DAsync(R, sizeof(float) * (size_t)ldr, dR, sizeof(float) * (size_t)d, sizeof(float) * (size_t)d, (size_t)n, hipMemcpyDeviceToHost, s));
        LSQ_HIP(hipStreamSynchronize(s));
    }
    float ms[2];
    LSQ_TRY(p->clock.read(ms));
    lsq_partition_info info{};
    info.call = LSQ_PARTITION_RESIDUALS; info.rows = n; info.loader_bytes = loader; info.kernel_ms = ms[0];
    p->info = info;
    return LSQ_OK;
}

extern "C" int lsq_partition_code_norms(lsq_partition *p, const uint8_t *codes, const float *codebooks, int64_t n, int m, int h, const int32_t *list_of_row,
                                        const float *cbnorms, int ncb, float *norms, uint8_t *norm_codes, float *dbnorms, int on_device) {
    const char *fn = "lsq_partition_code_norms";
    if (!p) { lsq_set_error("%s: null partition", fn); return LSQ_EINVAL; }
    if (n < 0 || n > (int64_t)INT32_MAX - 1) { lsq_set_error("%s: needs 0 <= n <= 2^31 - 2 (got %lld)", fn, (long long)n); return LSQ_EINVAL; }
    if (h != LSQ_H || m < 1 || m > LSQ_MAX_M) { lsq_set_error("%s: needs h == 256 and 1 <= m <= 16 (got h=%d m=%d)", fn, h, m); return LSQ_EINVAL; }
    if (cbnorms && (ncb < 1 || ncb > 256)) { lsq_set_error("%s: needs 1 <= ncb <= 256 (got %d)", fn, ncb); return LSQ_EINVAL; }
    if (!cbnorms && !norms) { lsq_set_error("%s: without cbnorms the call needs norms", fn); return LSQ_EINVAL; }
    if (!codebooks || (n > 0 && (!codes || !list_of_row))) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    if (!cbnorms) { norm_codes = nullptr; dbnorms = nullptr; }
    if (n == 0) return LSQ_OK;
    hipStream_t s = nullptr;
    int profile = 0;
    LSQ_TRY(lsq_ctx_bind(p->ctx, &s, &profile));
    const int nlist = p->nlist, d = p->d;
    const uint8_t *dcodes = nullptr;
    const float *dK = nullptr, *dcb = nullptr;
    const int32_t *dlor = nullptr;
    LSQ_TRY(stage_array(s, p->s_codes, codes, (size_t)n * (size_t)m, on_device, &dcodes));
    LSQ_TRY(stage_array(s, p->s_K, codebooks, (size_t)m * LSQ_H * (size_t)d, on_device, &dK));
    LSQ_TRY(stage_array(s, p->s_cb, cbnorms, (size_t)(cbnorms ? ncb : 0), on_device, &dcb));
    LSQ_TRY(stage_array(s, p->s_lor, list_of_row, (size_t)n, on_device, &dlor));
    float *dn = norms, *ddb = dbnorms;
    uint8_t *dnc = norm_codes;
    if (!on_device) {
        if (norms) { LSQ_TRY(p->s_out.ensure(sizeof(float) * (size_t)n)); dn = p->s_out.as<float>(); }
        if (dbnorms) { LSQ_TRY(p->s_dbn.ensure(sizeof(float) * (size_t)n)); ddb = p->s_dbn.as<float>(); }
        if (norm_codes) { LSQ_TRY(p->s_nc.ensure((size_t)n)); dnc = p->s_nc.as<uint8_t>(); }
    }
    LSQ_HIP(hipMemsetAsync(p->words.p, 0, 4 * sizeof(unsigned), s));
    LSQ_TRY(p->clock.begin(profile != 0));
    LSQ_TRY(p->clock.mark(s));
    hipLaunchKernelGGL(code_norms_kernel, dim3((unsigned)((n + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS), 0, s, dcodes, dK, p->cent.as<float>(), nlist,
                       dlor, dcb, ncb, n, d, m, dn, dnc, ddb, p->words.as<unsigned>());
    LSQ_HIP(hipGetLastError());
    LSQ_TRY(p->clock.mark(s));
    unsigned w[4];
    LSQ_TRY(read_words(s, p, w));
    if (w[0]) return bad_lists(fn, w[0], nlist);
    if (!on_device) {
        if (norms) LSQ_HIP(hipMemcpyAsync(norms, dn, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, s));
        if (dbnorms) LSQ_HIP(hipMemcpyAsync(dbnorms, ddb, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, s));
        if (norm_codes) LSQ_HIP(hipMemcpyAsync(norm_codes, dnc, (size_t)n, hipMemcpyDeviceToHost, s));
        LSQ_HIP(hipStreamSynchronize(s));
    }
    float ms[2];
    LSQ_TRY(p->clock.read(ms));
    lsq_partition_info info{};
    info.call = LSQ_PARTITION_CODE_NORMS; info.rows = n; info.kernel_ms = ms[0];
    p->info = info;
    return LSQ_OK;
}

// ---- the host checkers and engine-less roads: the contracts on plain arrays -----------------------------------------------------------------------------------
namespace {

int cpu_check(const char *fn, int64_t n, int d, int nlist, const int32_t *lor) {
    if (n < 0 || n > (int64_t)INT32_MAX - 1) { lsq_set_error("%s: needs 0 <= n <= 2^31 - 2 (got %lld)", fn, (long long)n); return LSQ_EINVAL; }
    if (nlist < 1 || nlist > (1 << 24) || d < 1) { lsq_set_error("%s: needs 1 <= nlist <= 2^24 and d >= 1 (got nlist=%d d=%d)", fn, nlist, d); return LSQ_EINVAL; }
    if (n > 0 && !lor) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    for (int64_t i = 0; i < n; ++i)
        if (lor[i] < 0 || lor[i] >= nlist) {
            lsq_set_error("%s: list_of_row[%lld] = %d lies outside [0, %d)", fn, (long long)i, lor[i], nlist);
            return LSQ_EINVAL;
        }
    return LSQ_OK;
}

int x_check(const char *fn, const void *X, int x_u8, int64_t n, int d, int64_t ldx) {
    if (ldx < d) { lsq_set_error("%s: needs ldx >= d (got ldx=%lld d=%d)", fn, (long long)ldx, d); return LSQ_EINVAL; }
    if (n > 0 && !X) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    if (!x_u8 && ((uintptr_t)X & 3) != 0) { lsq_set_error("%s: the f32 rows are not 4-byte aligned", fn); return LSQ_EINVAL; }
    return LSQ_OK;
}

int workers(int nthreads, int64_t items) {
    int nt = nthreads > 0 ? nthreads : (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if ((int64_t)nt > items) nt = (int)items;
    return nt < 1 ? 1 : nt;
}

// dimensions [t0, t1): float64 sums of every list in ascending row id, then the means of the lists that have rows
template <typename T>
void update_dims(float *cent, const T *X, int64_t n, int d, int64_t ldx, const int32_t *lor, int nlist, const int32_t *counts, int t0, int t1) {
    const int w = t1 - t0;
    std::vector<double> sums((size_t)nlist * (size_t)w, 0.0);
    for (int64_t i = 0; i < n; ++i) {
        double *sr = sums.data() + (size_t)lor[i] * (size_t)w;
        const T *x = X + i * ldx + t0;
        for (int t = 0; t < w; ++t) sr[t] = sr[t] + (double)(float)x[t];
    }
    for (int l = 0; l < nlist; ++l) {
        if (counts[l] == 0) continue;
        for (int t = 0; t < w; ++t) cent[(size_t)l * d + t0 + t] = (float)(sums[(size_t)l * w + t] / (double)counts[l]);
    }
}

template <typename T>
void residual_rows(float *R, int64_t ldr, const T *X, int64_t ldx, int d, const float *cent, const int32_t *lor, int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; ++i) {
        const T *x = X + i * ldx;
        const float *c = cent + (size_t)lor[i] * d;
        float *r = R + i * ldr;
        for (int t = 0; t < d; ++t) r[t] = (float)x[t] - c[t];
    }
}

struct NormsCpu {
    float *norms; uint8_t *norm_codes; float *dbnorms;
    const uint8_t *codes; const float *K, *cent; const int32_t *lor; const float *cb;
    int m, h, d, ncb;
};

void code_norm_rows(const NormsCpu a, int64_t i0, int64_t i1) {
    std::vector<float> rec((size_t)a.d);
    for (int64_t i = i0; i < i1; ++i) {
        const uint8_t *code = a.codes + (size_t)i * a.m;
        for (int j = 0; j < a.m; ++j) {                              // codebooks ascending, starting from the first codeword
            const float *row = a.K + ((size_t)j * a.h + code[j]) * a.d;
            if (j == 0) for (int t = 0; t < a.d; ++t) rec[(size_t)t] = row[t];
            else for (int t = 0; t < a.d; ++t) rec[(size_t)t] = rec[(size_t)t] + row[t];
        }
        const float *c = a.cent + (size_t)a.lor[i] * a.d;
        float av = 0.0f, bv = 0.0f;
        for (int t = 0; t < a.d; ++t) {
            const float r = rec[(size_t)t];
            av = av + r * r;                                         // product rounded, then the add (-ffp-contract=off)
            bv = bv + c[t] * r;
        }
        const float sv = av + (bv + bv);
        if (a.norms) a.norms[i] = sv;
        if (!a.cb) continue;
        int best = 0;
        float bd = (sv - a.cb[0]) * (sv - a.cb[0]);
        for (int j = 1; j < a.ncb; ++j) {
            const float df = sv - a.cb[j], dd = df * df;
            if (dd < bd) { bd = dd; best = j; }
        }
        if (a.norm_codes) a.norm_codes[i] = (uint8_t)best;
        if (a.dbnorms) a.dbnorms[i] = a.cb[best];
    }
}

}  // namespace

extern "C" int lsq_partition_update_cpu(float *centroids, int32_t *counts, const void *X, int x_u8, int64_t n, int d, int ldx, const int32_t *list_of_row,
                                        int nlist, int nthreads) {
    const char *fn = "lsq_partition_update_cpu";
    if (!centroids) { lsq_set_error("%s: null centroids", fn); return LSQ_EINVAL; }
    LSQ_TRY(cpu_check(fn, n, d, nlist, list_of_row));
    LSQ_TRY(x_check(fn, X, x_u8, n, d, ldx));
    std::vector<int32_t> cnt((size_t)nlist, 0);
    for (int64_t i = 0; i < n; ++i) cnt[(size_t)list_of_row[i]] += 1;
    if (counts) memcpy(counts, cnt.data(), sizeof(int32_t) * (size_t)nlist);
    if (n == 0) return LSQ_OK;
    const int nt = workers(nthreads, d);
    std::vector<std::thread> pool;
    pool.reserve((size_t)nt);
    for (int t = 0; t < nt; ++t) {
        const int t0 = (int)((int64_t)d * t / nt), t1 = (int)((int64_t)d * (t + 1) / nt);
        if (x_u8) pool.emplace_back(update_dims<uint8_t>, centroids, static_cast<const uint8_t *>(X), n, d, (int64_t)ldx, list_of_row, nlist, cnt.data(), t0, t1);
        else pool.emplace_back(update_dims<float>, centroids, static_cast<const float *>(X), n, d, (int64_t)ldx, list_of_row, nlist, cnt.data(), t0, t1);
    }
    for (auto &th : pool) th.join();
    return LSQ_OK;
}

extern "C" int lsq_partition_residuals_cpu(float *R, int ldr, const void *X, int x_u8, int64_t n, int d, int ldx, const float *centroids,
                                           const int32_t *list_of_row, int nlist, int nthreads) {
    const char *fn = "lsq_partition_residuals_cpu";
    if (!centroids || (n > 0 && !R)) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    if (ldr < d) { lsq_set_error("%s: needs ldr >= d (got ldr=%d d=%d)", fn, ldr, d); return LSQ_EINVAL; }
    LSQ_TRY(cpu_check(fn, n, d, nlist, list_of_row));
    LSQ_TRY(x_check(fn, X, x_u8, n, d, ldx));
    if (n == 0) return LSQ_OK;
    const int nt = workers(nthreads, n);
    std::vector<std::thread> pool;
    pool.reserve((size_t)nt);
    for (int t = 0; t < nt; ++t) {
        const int64_t i0 = n * t / nt, i1 = n * (t + 1) / nt;
        if (x_u8) pool.emplace_back(residual_rows<uint8_t>, R, (int64_t)ldr, static_cast<const uint8_t *>(X), (int64_t)ldx, d, centroids, list_of_row, i0, i1);
        else pool.emplace_back(residual_rows<float>, R, (int64_t)ldr, static_cast<const float *>(X), (int64_t)ldx, d, centroids, list_of_row, i0, i1);
    }
    for (auto &th : pool) th.join();
    return LSQ_OK;
}

extern "C" int lsq_partition_code_norms_cpu(float *norms, uint8_t *norm_codes, float *dbnorms, const uint8_t *codes, const float *codebooks,
                                            const float *centroids, const int32_t *list_of_row, int64_t n, int m, int h, int d, int nlist,
                                            const float *cbnorms, int ncb, int nthreads) {
    const char *fn = "lsq_partition_code_norms_cpu";
    if (h != LSQ_H || m < 1 || m > LSQ_MAX_M) { lsq_set_error("%s: needs h == 256 and 1 <= m <= 16 (got h=%d m=%d)", fn, h, m); return LSQ_EINVAL; }
    if (cbnorms && (ncb < 1 || ncb > 256)) { lsq_set_error("%s: needs 1 <= ncb <= 256 (got %d)", fn, ncb); return LSQ_EINVAL; }
    if (!cbnorms && !norms) { lsq_set_error("%s: without cbnorms the call needs norms", fn); return LSQ_EINVAL; }
    if (!codebooks || !centroids || (n > 0 && !codes)) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    LSQ_TRY(cpu_check(fn, n, d, nlist, list_of_row));
    if (n == 0) return LSQ_OK;
    const NormsCpu a{norms, cbnorms ? norm_codes : nullptr, cbnorms ? dbnorms : nullptr, codes, codebooks, centroids, list_of_row, cbnorms, m, h, d, ncb};
    const int nt = workers(nthreads, n);
    std::vector<std::thread> pool;
    pool.reserve((size_t)nt);
    for (int t = 0; t < nt; ++t) pool.emplace_back(code_norm_rows, a, n * t / nt, n * (t + 1) / nt);
    for (auto &th : pool) th.join();
    return LSQ_OK;
}
