// lsq_grow.hip -- appending rows to a resident index ON THE DEVICE (gfx950): the kernels of lsq_index_add.
//
// The reference has no counterpart.  The contract (Identity G): after an add the index is, array for array, the one a fresh build over the
// concatenation would hold.  The flat arrays are appended in place (owned storage with capacity: lsq_devbuf_grow keeps the contents when it has to move).
// The kernel work is the INVERTED LAYOUT (lsq_ivf.hip): list l is positions off[l] .. off[l + 1] of codes / norms / ids, ascending by original id inside.
// New ids are larger than every old one, so the new rows of a list go at the END of its segment and no position depends on an atomic:
//
//   keys     (list << 32 | r) of the `count` new rows, sorted: lsq_rows_keys / lsq_rows_sort over count keys, add_off[nlist + 1] from lsq_rows_offsets
//   noff     noff[l] = off[l] + add_off[l]                                                                                      grow_offsets_kernel
//   old rows position q of list l -> q + add_off[l]: per stream (code rows, norms, ids) ONE SEGMENTED BYTE SHIFT                  grow_shift_kernel
//   new rows the j-th sorted key (list l, new row r) -> position off[l + 1] + j, id n + r                                       grow_place_kernel
//
// The merge is written OUT OF PLACE, into the spare half of the layout's double buffers: it is never an overlapping shift across blocks.
//
// grow_shift_kernel is a bandwidth kernel.  A stream is bytes: rows of rowb = 1 .. 17 bytes (4 for norms and ids) at arbitrary byte offsets.  A lane owns 16
// DESTINATION bytes at a 16-byte boundary (one global_store_dwordx4; a wave stores 1 KiB contiguous); when all 16 lie in old rows of one list -- all but
// the chunks at a list's boundary -- their source is the 16 bytes add_off[l] * rowb earlier: one dwordx4 load where that shift is a multiple of 16, else
// the five dwords around it funnelled with v_alignbyte_b32 (the shift is the same for every lane inside a list: no divergence there).  The list of a chunk
// is found ONCE PER BLOCK by two binary searches over noff (the block's first and last row) and then, per chunk, inside that window -- held in LDS, a
// handful of lists for 16 KiB of rows -- instead of a 24-step search of global memory per row.  Boundary chunks go byte by byte.
#include <utility>

#include "lsq_internal.h"

namespace {

constexpr int GROW_THREADS = 256;
constexpr int GROW_CHUNKS = 4;                                       // 16-byte chunks per lane
constexpr int GROW_TILE = GROW_THREADS * GROW_CHUNKS * 16;           // destination bytes per block: 16 KiB
constexpr int GROW_WIN = 1024;                                       // lists of a block's window held in LDS; a longer window is searched in global memory

__global__ void grow_offsets_kernel(const int *__restrict__ off, const int *__restrict__ add_off, int nlist, int *__restrict__ noff) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l <= nlist) noff[l] = off[l] + add_off[l];
}

// 16 bytes from any byte address: whole dwords around it (at most 3 bytes before p and 3 past p + 16 are read: the streams' allocations end in 16 bytes
// of slack, and a dword that holds a wanted byte lies inside the allocation at its front)
__device__ inline uint4 grow_load16(const uint8_t *p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const unsigned sh = (unsigned)(a & 3u);
    if ((a & 15u) == 0) return *reinterpret_cast<const uint4 *>(p);
    const uint32_t *w = reinterpret_cast<const uint32_t *>(a - sh);
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
    uint4 r;
    if (sh == 0) {
        r.x = w0; r.y = w1; r.z = w2; r.w = w3;
    } else {
        const uint32_t w4 = w[4];
        r.x = __builtin_amdgcn_alignbyte(w1, w0, sh);
        r.y = __builtin_amdgcn_alignbyte(w2, w1, sh);
        r.z = __builtin_amdgcn_alignbyte(w3, w2, sh);
        r.w = __builtin_amdgcn_alignbyte(w4, w3, sh);
    }
    return r;
}

// the last list l in [lo, hi] with f(l) <= p (f ascending, f(lo) <= p)
template <class F>
__device__ inline int grow_list_of(int lo, int hi, int p, F f) {
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (f(mid) <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The old rows of one stream: dst byte D of an old row of list l = src byte D - rowb * (noff[l] - off[l]).  total = (n + count) * rowb destination bytes;
// the bytes of the new rows are grow_place_kernel's and are not touched here
__global__ __launch_bounds__(GROW_THREADS) void grow_shift_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const int *__restrict__ off,
                                                                  const int *__restrict__ noff, int nlist, int rowb, int64_t total) {
    __shared__ int s_edge[2];
    __shared__ int w_noff[GROW_WIN + 1], w_off[GROW_WIN + 1];
    const int t = threadIdx.x;
    const int64_t B0 = (int64_t)blockIdx.x * GROW_TILE;
    const int64_t B1 = B0 + GROW_TILE < total ? B0 + GROW_TILE : total;
    const int row_lo = (int)(B0 / rowb), rem0 = (int)(B0 % rowb), row_hi = (int)((B1 - 1) / rowb);      // (block-uniform)
    if (t < 2) s_edge[t] = grow_list_of(0, nlist - 1, t ? row_hi : row_lo, [&](int l) { return noff[l]; });      // noff[0] = 0 <= every row
    __syncthreads();
    const int l0 = s_edge[0], l1 = s_edge[1], nl = l1 - l0 + 1;
    const bool win = nl <= GROW_WIN;
    if (win)
        for (int i = t; i <= nl; i += GROW_THREADS) { w_noff[i] = noff[l0 + i]; w_off[i] = off[l0 + i]; }
    __syncthreads();
    auto NOFF = [&](int l) { return win ? w_noff[l - l0] : noff[l]; };
    auto OFF = [&](int l) { return win ? w_off[l - l0] : off[l]; };
    const int span = (int)(B1 - B0);
#pragma unroll
    for (int c = 0; c < GROW_CHUNKS; ++c) {
        const int rel = (c * GROW_THREADS + t) * 16;
        if (rel >= span) continue;
        const int len = span - rel < 16 ? span - rel : 16;
        const int p = row_lo + (int)((unsigned)(rem0 + rel) / (unsigned)rowb);
        const int pe = row_lo + (int)((unsigned)(rem0 + rel + len - 1) / (unsigned)rowb);
        int l = grow_list_of(l0, l1, p, NOFF);
        int a = NOFF(l), b = OFF(l), old_end = a + (OFF(l + 1) - b);      // positions a .. old_end - 1 of the new layout are list l's old rows
        const int64_t D = B0 + rel;
        if (len == 16 && pe < old_end) {
            const uint4 v = grow_load16(src + (D - (int64_t)(a - b) * rowb));
            *reinterpret_cast<uint4 *>(dst + D) = v;
            continue;
        }
        int pk = p, within = (int)((unsigned)(rem0 + rel) % (unsigned)rowb);
        for (int k = 0; k < len; ++k) {
            while (pk >= NOFF(l + 1)) { ++l; a = NOFF(l); b = OFF(l); old_end = a + (OFF(l + 1) - b); }      // pk <= row_hi < noff[l1 + 1]: l stays <= l1
            if (pk < old_end) dst[D + k] = src[D + k - (int64_t)(a - b) * rowb];
            if (++within == rowb) { within = 0; ++pk; }
        }
    }
}

// the new rows: sorted key j = (list l, new row r) -> position off[l + 1] + j (off: the OLD offsets; add_off[l] keys of smaller lists and the key's rank
// inside its list are both in j)
__global__ void grow_place_kernel(const uint64_t *__restrict__ sorted, int64_t count, const int *__restrict__ off, int rowb,
                                  const uint8_t *__restrict__ add_rows, const float *__restrict__ add_norms, int64_t n, uint8_t *__restrict__ codes,
                                  float *__restrict__ norms, int *__restrict__ ids) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const uint64_t key = sorted[j];
    const int l = (int)(key >> 32);
    const int64_t r = (int64_t)(uint32_t)key;
    const int64_t at = (int64_t)off[l + 1] + j;                      // < n + count: off[l + 1] <= n
    for (int k = 0; k < rowb; ++k) codes[at * rowb + k] = add_rows[r * rowb + k];
    if (norms) norms[at] = add_norms[r];
    ids[at] = (int)(n + r);
}

// bits n0 .. n1 - 1 set: one thread per word, no atomic
__global__ void grow_bits_kernel(uint32_t *__restrict__ words, int64_t n0, int64_t n1) {
    const int64_t w = (n0 >> 5) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w > ((n1 - 1) >> 5)) return;
    const int64_t lo = w * 32 > n0 ? w * 32 : n0, hi = (w + 1) * 32 < n1 ? (w + 1) * 32 : n1;      // [lo, hi) inside word w, hi > lo
    const uint32_t upto_hi = hi - w * 32 == 32 ? 0xffffffffu : (1u << (hi - w * 32)) - 1u;
    const uint32_t below_lo = (1u << (lo - w * 32)) - 1u;
    words[w] |= upto_hi & ~below_lo;
}

int shift_stream(hipStream_t s, const void *src, void *dst, const lsq_grow_merge &g, int rowb) {
    const int64_t total = (g.n + g.count) * (int64_t)rowb;
    const int64_t blocks = (total + GROW_TILE - 1) / GROW_TILE;      // <= 2^31 * 17 / 2^14 blocks
    hipLaunchKernelGGL(grow_shift_kernel, dim3((unsigned)blocks), dim3(GROW_THREADS), 0, s, static_cast<const uint8_t *>(src), static_cast<uint8_t *>(dst),
                       g.off, g.noff, g.nlist, rowb, total);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

}  // namespace

int lsq_devbuf_grow(hipStream_t s, DevBuf &b, size_t bytes, size_t keep, const void *src) {
    if (!src) src = b.p;
    if (bytes <= b.cap && !b.view && src == b.p) return LSQ_OK;
    if (bytes < b.cap) bytes = b.cap;
    void *p = nullptr;
    LSQ_HIP(hipMalloc(&p, bytes));
    if (keep > 0 && src) {
        const hipError_t e = hipMemcpyAsync(p, src, keep < bytes ? keep : bytes, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) { (void)hipFree(p); LSQ_HIP(e); }
        const hipError_t w = hipStreamSynchronize(s);
        if (w != hipSuccess) { (void)hipFree(p); LSQ_HIP(w); }
    }
    void *old = b.view ? nullptr : b.p;
    b.p = p; b.cap = bytes; b.view = false;
    if (old) LSQ_HIP(hipFree(old));
    return LSQ_OK;
}

int lsq_grow_launch_merge(hipStream_t s, const lsq_grow_merge &g) {
    hipLaunchKernelGGL(grow_offsets_kernel, dim3((unsigned)((g.nlist + 1 + 255) / 256)), dim3(256), 0, s, g.off, g.add_off, g.nlist, g.noff);
    LSQ_HIP(hipGetLastError());
    LSQ_TRY(shift_stream(s, g.src_codes, g.dst_codes, g, g.rowb));
    if (g.src_norms) LSQ_TRY(shift_stream(s, g.src_norms, g.dst_norms, g, 4));
    LSQ_TRY(shift_stream(s, g.src_ids, g.dst_ids, g, 4));
    if (g.count > 0) {
        hipLaunchKernelGGL(grow_place_kernel, dim3((unsigned)((g.count + 255) / 256)), dim3(256), 0, s, g.sorted, g.count, g.off, g.rowb, g.add_rows,
                           g.add_norms, g.n, g.dst_codes, g.src_norms ? g.dst_norms : nullptr, g.dst_ids);
        LSQ_HIP(hipGetLastError());
    }
    return LSQ_OK;
}

int lsq_grow_launch_set_bits(hipStream_t s, uint32_t *words, int64_t n0, int64_t n1) {
    if (n1 <= n0) return LSQ_OK;
    const int64_t nw = ((n1 - 1) >> 5) - (n0 >> 5) + 1;
    hipLaunchKernelGGL(grow_bits_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, words, n0, n1);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}
