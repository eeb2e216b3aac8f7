// lsq_compact.hip -- rows leaving a resident index ON THE DEVICE (gfx950): the kernels of lsq_index_compact.
//
// The reference has no counterpart.  The contract (Identity C): after a compact the index is, array for array, the one a fresh build over the
// surviving rows would hold.  Every array of the index that has one entry per row -- flat code rows, flat norms, base rows, and the inverted layout's code
// rows, norms and ids -- is a STREAM OF BYTES gathered by one map:
//
//   flat arrays   destination row j = source row sel[j], sel = the filter's ascending row list (lsq_filter.hip: rows)          compact_gather_kernel
//   layout        sel = the set bits of the filter's LAYOUT-ORDER bitmap, ascending (flt_compact_kernel over lbits / lpre: the compact form of the
//                 layout, alive for this call only); a list keeps its surviving positions in order                                 compact_gather_kernel
//   offsets       off'[l] = P(off[l]),  P(p) = lpre[p >> 5] + popc(lbits[p >> 5] & below(p))                                   compact_offsets_kernel
//   ids           the id at a new position = the RANK of the old id among the allowed rows, pre[id >> 5] + popc(bits[id >> 5] & below(id)); the rank
//                 is monotone, so a list stays ascending by id: the layout equals the radix-sorted one of a fresh set_lists       compact_ids_kernel
//   maps          new_of_old[i] = rank(i) or -1, old_of_new[j] = rows[j], for the caller                                          compact_maps_kernel
//
// No atomic decides a position anywhere.  Everything is written OUT OF PLACE (fresh flat arrays, the spare half of the layout) and committed by the caller.
//
// compact_gather_kernel is a bandwidth kernel.  A lane owns 16 DESTINATION bytes at a 16-byte boundary (one global_store_dwordx4; a wave stores 1 KiB
// contiguous).  With p .. pe the destination rows the chunk touches: sel[pe] - sel[p] == pe - p means the survivors are a run and the 16 source bytes are
// contiguous -- one dwordx4 load from an aligned source, else the dwords around it funnelled with v_alignbyte_b32 (every dword read holds a wanted byte:
// none lies outside the source's allocation).  A chunk that straddles survivors that were not neighbours is put together byte by byte in registers and
// still stored once.  sel is the whole map: no search, no per-block prologue, no LDS.
#include <utility>

#include "lsq_internal.h"

namespace {

constexpr int CMP_THREADS = 256;
constexpr int CMP_CHUNKS = 4;                                        // 16-byte chunks per lane
constexpr int CMP_TILE = CMP_THREADS * CMP_CHUNKS * 16;              // destination bytes per block: 16 KiB

// 16 bytes from any byte address: whole dwords, each of which holds at least one of the wanted bytes
__device__ inline uint4 compact_load16(const uint8_t *p) {
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

// the set bits below position p of a bitmap with the exclusive prefix of its words' popcounts (p a multiple of 32: the word is not read -- p may be one
// past the last word)
__device__ inline int compact_prefix_at(const uint32_t *__restrict__ bits, const int *__restrict__ pre, int p) {
    const int w = p >> 5, b = p & 31;
    return pre[w] + (b ? __popc(bits[w] & ((1u << b) - 1u)) : 0);
}

// dst row j = src row sel[j], rows rowb bytes apart in both; rows_out rows, the last one lastb <= rowb bytes long: total = (rows_out - 1) * rowb + lastb
// destination bytes, and no source byte past the lastb-th of row sel[rows_out - 1] is wanted
__global__ __launch_bounds__(CMP_THREADS) void compact_gather_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const int *__restrict__ sel,
                                                                     int rowb, int64_t rows_out, int lastb) {
    const int64_t total = (rows_out - 1) * (int64_t)rowb + lastb;
    const int64_t B0 = (int64_t)blockIdx.x * CMP_TILE;
    const int64_t B1 = B0 + CMP_TILE < total ? B0 + CMP_TILE : total;
    const int64_t row_lo = B0 / rowb;                                // (block-uniform)
    const unsigned rem0 = (unsigned)(B0 - row_lo * rowb);
    const int span = (int)(B1 - B0);
    const int t = threadIdx.x;
#pragma unroll
    for (int c = 0; c < CMP_CHUNKS; ++c) {
        const int rel = (c * CMP_THREADS + t) * 16;
        if (rel >= span) continue;
        const int len = span - rel < 16 ? span - rel : 16;
        const unsigned x = rem0 + (unsigned)rel;                     // < rowb + 16 KiB <= 2^30 + 2^14
        const unsigned q = x / (unsigned)rowb;
        unsigned within = x - q * (unsigned)rowb;
        const int64_t p = row_lo + q, pe = row_lo + (x + (unsigned)len - 1u) / (unsigned)rowb;      // pe < rows_out: D + len <= total
        const int64_t D = B0 + rel;
        const int sp = sel[p];
        if (len == 16 && (p == pe || (int64_t)sel[pe] - sp == pe - p)) {      // a run of survivors: 16 contiguous source bytes
            *reinterpret_cast<uint4 *>(dst + D) = compact_load16(src + (int64_t)sp * rowb + within);
            continue;
        }
        int64_t pk = p;
        const uint8_t *row = src + (int64_t)sp * rowb;
        if (len == 16) {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                w[k >> 2] |= (uint32_t)row[within] << (8 * (k & 3));
                if (++within == (unsigned)rowb && k < 15) { within = 0; row = src + (int64_t)sel[++pk] * rowb; }      // pk <= pe here
            }
            *reinterpret_cast<uint4 *>(dst + D) = make_uint4(w[0], w[1], w[2], w[3]);
            continue;
        }
        for (int k = 0; k < len; ++k) {                              // the stream's last chunk
            dst[D + k] = row[within];
            if (++within == (unsigned)rowb && k + 1 < len) { within = 0; row = src + (int64_t)sel[++pk] * rowb; }
        }
    }
}

__global__ void compact_offsets_kernel(const uint32_t *__restrict__ lbits, const int *__restrict__ lpre, const int *__restrict__ off, int nlist,
                                       int *__restrict__ noff) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l <= nlist) noff[l] = compact_prefix_at(lbits, lpre, off[l]);
}

// new position j holds old position lsel[j]; its id is the rank of the old id (an allowed row: its bit is set)
__global__ void compact_ids_kernel(const int *__restrict__ src_ids, const int *__restrict__ lsel, const uint32_t *__restrict__ bits,
                                   const int *__restrict__ pre, int64_t rows_out, int *__restrict__ dst_ids) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= rows_out) return;
    dst_ids[j] = compact_prefix_at(bits, pre, src_ids[lsel[j]]);
}

// the caller's maps; bits == null: nothing was dropped, both are identities
__global__ void compact_maps_kernel(const uint32_t *__restrict__ bits, const int *__restrict__ pre, const int *__restrict__ rows, int64_t n, int64_t allowed,
                                    int id_base, int *__restrict__ old_of_new, int *__restrict__ new_of_old) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (new_of_old && i < n) {
        int r = (int)i;
        if (bits) r = ((bits[i >> 5] >> (i & 31)) & 1u) ? compact_prefix_at(bits, pre, (int)i) : -1;
        new_of_old[i] = r < 0 ? -1 : r + id_base;
    }
    if (old_of_new && i < allowed) old_of_new[i] = (rows ? rows[i] : (int)i) + id_base;
}

}  // namespace

int lsq_compact_launch_gather(hipStream_t s, const void *src, void *dst, const int *sel, int64_t rowb, int64_t rows_out, int64_t lastb, int64_t *bytes) {
    if (rows_out < 1) return LSQ_OK;
    if (rowb < 1 || rowb > ((int64_t)1 << 30) || lastb < 1 || lastb > rowb) { lsq_set_error("lsq_index_compact: a row of %lld bytes cannot be gathered", (long long)rowb); return LSQ_EINVAL; }
    const int64_t total = lsq_compact_stream_bytes(rows_out, rowb, lastb);
    const int64_t blocks = (total + CMP_TILE - 1) / CMP_TILE;        // <= 2^31 * 2^30 / 2^14: the caller's arrays are far smaller
    if (blocks > (int64_t)INT32_MAX) { lsq_set_error("lsq_index_compact: a stream of %lld bytes is too long", (long long)total); return LSQ_EINVAL; }
    hipLaunchKernelGGL(compact_gather_kernel, dim3((unsigned)blocks), dim3(CMP_THREADS), 0, s, static_cast<const uint8_t *>(src), static_cast<uint8_t *>(dst),
                       sel, (int)rowb, rows_out, (int)lastb);
    LSQ_HIP(hipGetLastError());
    if (bytes) *bytes += total;
    return LSQ_OK;
}

int lsq_compact_launch_layout(hipStream_t s, const lsq_compact_layout &g, int64_t *bytes) {
    hipLaunchKernelGGL(compact_offsets_kernel, dim3((unsigned)((g.nlist + 1 + 255) / 256)), dim3(256), 0, s, g.lbits, g.lpre, g.off, g.nlist, g.noff);
    LSQ_HIP(hipGetLastError());
    LSQ_TRY(lsq_compact_launch_gather(s, g.src_codes, g.dst_codes, g.lsel, g.rowb, g.rows_out, g.rowb, bytes));
    if (g.src_norms) LSQ_TRY(lsq_compact_launch_gather(s, g.src_norms, g.dst_norms, g.lsel, 4, g.rows_out, 4, bytes));
    hipLaunchKernelGGL(compact_ids_kernel, dim3((unsigned)((g.rows_out + 255) / 256)), dim3(256), 0, s, g.src_ids, g.lsel, g.bits, g.pre, g.rows_out, g.dst_ids);
    LSQ_HIP(hipGetLastError());
    if (bytes) *bytes += 4 * g.rows_out;
    return LSQ_OK;
}

int lsq_compact_launch_maps(hipStream_t s, const uint32_t *bits, const int *pre, const int *rows, int64_t n, int64_t allowed, int id_base, int *old_of_new,
                            int *new_of_old) {
    if (!old_of_new && !new_of_old) return LSQ_OK;
    hipLaunchKernelGGL(compact_maps_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, bits, pre, rows, n, allowed, id_base, old_of_new, new_of_old);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

int lsq_devbuf_fit(hipStream_t s, DevBuf &b, size_t bytes, size_t keep) {
    if (!b.p || b.view || b.cap == bytes) return LSQ_OK;
    void *p = nullptr;
    LSQ_HIP(hipMalloc(&p, bytes));
    if (keep > bytes) keep = bytes;
    if (keep > 0) {
        hipError_t e = hipMemcpyAsync(p, b.p, keep, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { (void)hipFree(p); LSQ_HIP(e); }
    }
    void *old = b.p;
    b.p = p; b.cap = bytes;
    LSQ_HIP(hipFree(old));
    return LSQ_OK;
}
