// lsq_snapshot.hip -- snapshots of a resident index ON THE DEVICE (gfx950): the two streaming kernels behind lsq_index_save / _load / _export /
// _digest, and the host-only entry points lsq_snapshot_write_cpu / _read_cpu / _inspect_cpu / _digest_cpu (bodies: lsq_snapshot_check.h).  The reference has
// no counterpart: it keeps no resident index.
//
//   snap_digest_kernel   the digest of include/lsq_mi355x.h (3p) over a device byte range of ANY start alignment and length.  The range's first byte is byte 0 of
//                        word first_word of its section, so the section's words lie at ptr + 4 t whatever ptr & 3 is.  A lane takes one ALIGNED 16-byte
//                        vector (global_load_dwordx4, non-temporal) of the range and, when ptr & 3 != 0, the dword after it; the section's words are funnelled
//                        out of neighbouring dwords with v_alignbyte_b32.  Words before the range's start (the first vector) and past its last whole word are
//                        masked, never dereferenced beyond an aligned dword that holds a byte of the range.  The zero-padded last word (bytes & 3 != 0) is
//                        read byte by byte by one thread.  A term is two 32-bit multiplies for the mixer, one for the position key and one 32 x 32 -> 64
//                        multiply; terms add up mod 2^64 per lane, over the wave (shuffles), per wave in LDS, and ONE 64-bit partial per block is written:
//                        no atomics, no order.  snap_sum_kernel adds the partials and the length term into the section's accumulator: chunks of a
//                        section add up in stream order.
//   snap_unpack_kernel   packed rows of m + 1 bytes (codes, norm byte) -> the CODES stream [n][m] and the NORM_CODES stream [n], any sub-range of either.
//                        From the OUTPUT side: a lane owns 16 output bytes.  Output byte o of the codes stream is source byte o + o / m: per output dword the
//                        three aligned dwords around its source span (at most 7 bytes; with the alignment, 10) are loaded and the four bytes picked with two
//                        v_perm_b32; one 16-byte store where the destination allows, byte stores at a range's ragged end.  Row widths 2 .. 17 take the same
//                        path; at m + 1 = 4, 8, 12, 16 the source dwords are whole rows.  A norm byte is one aligned dword load and a shift.
#include "lsq_internal.h"

namespace {

constexpr int SNAP_THREADS = 256;
constexpr int SNAP_MAX_BLOCKS = LSQ_SNAP_PARTIALS;

typedef uint32_t snap_u32x4 __attribute__((ext_vector_type(4)));

__device__ inline uint64_t snap_wave_sum(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, off, 64), hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// one partial per block: partials[blockIdx.x] = the block's sum (every block writes, so the caller reads gridDim.x of them)
__device__ inline void snap_block_partial(uint64_t sum, unsigned long long *__restrict__ partials) {
    __shared__ unsigned long long wsum[SNAP_THREADS / 64];
    sum = snap_wave_sum(sum);
    const int t = threadIdx.x;
    if ((t & 63) == 0) wsum[t >> 6] = sum;
    __syncthreads();
    if (t == 0) {
        unsigned long long total = 0;
#pragma unroll
        for (int w = 0; w < SNAP_THREADS / 64; ++w) total += wsum[w];
        partials[blockIdx.x] = total;
    }
}

// a0: ptr rounded down to 16 bytes; q: dwords between a0 and ptr's dword (0 .. 3); sh = ptr & 3; nvec: aligned vectors that hold a byte of the range;
// nfull = bytes / 4.  Word t of the range (0 <= t < nfull) is the funnel of dwords q + t and q + t + 1 counted from a0
__global__ __launch_bounds__(SNAP_THREADS) void snap_digest_kernel(const uint8_t *__restrict__ ptr, unsigned long long bytes, unsigned long long first_word,
                                                                   unsigned long long *__restrict__ partials) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(ptr), a0 = p & ~(uintptr_t)15, end = p + bytes;
    const unsigned sh = (unsigned)(p & 3u);
    const long long q = (long long)((p - a0) >> 2);
    const long long nfull = (long long)(bytes >> 2);
    const long long nvec = bytes ? (long long)((end - a0 + 15) >> 4) : 0;
    uint64_t sum = 0;
    for (long long j = (long long)blockIdx.x * SNAP_THREADS + threadIdx.x; j < nvec; j += (long long)gridDim.x * SNAP_THREADS) {
        const uintptr_t a = a0 + ((uintptr_t)j << 4);
        const snap_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const snap_u32x4 *>(a));
        uint32_t next = 0;
        if (sh != 0 && a + 16 < end) next = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(a + 16));      // a dword that holds a byte of the range
        const uint32_t w[5] = {v.x, v.y, v.z, v.w, next};
        const long long t0 = 4 * j - q;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long t = t0 + k;
            const uint32_t word = sh ? __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh) : w[k];
            if (t >= 0 && t < nfull) sum += lsq_snap_term(word, first_word + (uint64_t)t);
        }
    }
    if ((bytes & 3u) && blockIdx.x == 0 && threadIdx.x == 0) {          // the zero-padded last word
        uint32_t word = 0;
        for (unsigned b = 0; b < (unsigned)(bytes & 3u); ++b) word |= (uint32_t)ptr[(uint64_t)nfull * 4 + b] << (8 * b);
        sum += lsq_snap_term(word, first_word + (uint64_t)nfull);
    }
    snap_block_partial(sum, partials);
}

// *acc += the first `count` partials + add (one block; the accumulator is written by one thread, in stream order)
__global__ __launch_bounds__(SNAP_THREADS) void snap_sum_kernel(const unsigned long long *__restrict__ partials, int count, unsigned long long add,
                                                                unsigned long long *__restrict__ acc) {
    __shared__ unsigned long long wsum[SNAP_THREADS / 64];
    uint64_t sum = 0;
    for (int k = threadIdx.x; k < count; k += SNAP_THREADS) sum += partials[k];
    sum = snap_wave_sum(sum);
    const int t = threadIdx.x;
    if ((t & 63) == 0) wsum[t >> 6] = sum;
    __syncthreads();
    if (t == 0) {
        unsigned long long total = add;
#pragma unroll
        for (int w = 0; w < SNAP_THREADS / 64; ++w) total += wsum[w];
        *acc += total;
    }
}

// four bytes of a byte stream picked out of memory: byte b (b < valid) is rows[src[b]], src ascending with src[3] - src[0] <= 6.  Aligned dword loads only, each
// of a dword that holds a wanted byte
__device__ inline uint32_t snap_pick4(const uint8_t *__restrict__ rows, const long long *src, int valid) {
    const uintptr_t first = reinterpret_cast<uintptr_t>(rows) + (uintptr_t)src[0], last = reinterpret_cast<uintptr_t>(rows) + (uintptr_t)src[valid - 1];
    const uintptr_t a = first & ~(uintptr_t)3;
    const uint32_t x0 = *reinterpret_cast<const uint32_t *>(a);
    const uint32_t x1 = a + 4 <= last ? *reinterpret_cast<const uint32_t *>(a + 4) : 0u;
    const uint32_t x2 = a + 8 <= last ? *reinterpret_cast<const uint32_t *>(a + 8) : 0u;
    uint32_t sel_a = 0, sel_b = 0;                    // v_perm_b32 selectors: 0 .. 3 the low operand's bytes, 4 .. 7 the high operand's, 0x0c a zero byte
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const unsigned rel = b < valid ? (unsigned)(reinterpret_cast<uintptr_t>(rows) + (uintptr_t)src[b] - a) : 99u;      // 0 .. 9
        const uint32_t sa = rel < 8u ? rel : 0x0cu, sb = (rel >= 8u && rel < 12u) ? rel - 4u : 0x0cu;
        sel_a |= sa << (8 * b);
        sel_b |= sb << (8 * b);
    }
    return __builtin_amdgcn_perm(x1, x0, sel_a) | __builtin_amdgcn_perm(x2, x1, sel_b);
}

// codes_out[o - c0] = stream byte o for o in [c0, c0 + cbytes); norms_out[r - r0] = row r's norm byte for r in [r0, r0 + rcount).  c0 + cbytes <= n m,
// r0 + rcount <= n.  vc / vn: the destination is 16-byte aligned
__global__ __launch_bounds__(SNAP_THREADS) void snap_unpack_kernel(const uint8_t *__restrict__ rows, int m, uint8_t *__restrict__ codes_out, long long c0,
                                                                   long long cbytes, uint8_t *__restrict__ norms_out, long long r0, long long rcount, int vc,
                                                                   int vn) {
    const long long citems = (cbytes + 15) >> 4, nitems = (rcount + 15) >> 4;
    for (long long it = (long long)blockIdx.x * SNAP_THREADS + threadIdx.x; it < citems + nitems; it += (long long)gridDim.x * SNAP_THREADS) {
        uint32_t out[4] = {0, 0, 0, 0};
        uint8_t *dst;
        int valid, vec;
        if (it < citems) {
            const long long o0 = c0 + (it << 4);
            valid = (int)(cbytes - (it << 4) < 16 ? cbytes - (it << 4) : 16);
            long long row = o0 / m;
            int rem = (int)(o0 - row * m);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                long long src[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    src[b] = o0 + 4 * g + b + row;                       // o + o / m
                    if (++rem == m) { rem = 0; ++row; }
                }
                const int gv = valid - 4 * g;
                if (gv > 0) out[g] = snap_pick4(rows, src, gv < 4 ? gv : 4);
            }
            dst = codes_out + (it << 4);
            vec = vc;
        } else {
            const long long j = it - citems;
            valid = (int)(rcount - (j << 4) < 16 ? rcount - (j << 4) : 16);
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                if (b < valid) {
                    const uintptr_t a = reinterpret_cast<uintptr_t>(rows) + (uintptr_t)((r0 + (j << 4) + b) * (long long)(m + 1) + m);
                    const uint32_t w = *reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
                    out[b >> 2] |= ((w >> (8 * (unsigned)(a & 3u))) & 0xffu) << (8 * (b & 3));
                }
            }
            dst = norms_out + (j << 4);
            vec = vn;
        }
        if (vec && valid == 16) {
            snap_u32x4 w;
            w.x = out[0]; w.y = out[1]; w.z = out[2]; w.w = out[3];
            *reinterpret_cast<snap_u32x4 *>(dst) = w;
        } else {
#pragma unroll
            for (int b = 0; b < 16; ++b)
                if (b < valid) dst[b] = (uint8_t)(out[b >> 2] >> (8 * (b & 3)));
        }
    }
}

inline unsigned snap_grid(long long items) {
    long long blocks = (items + SNAP_THREADS - 1) / SNAP_THREADS;
    if (blocks > SNAP_MAX_BLOCKS) blocks = SNAP_MAX_BLOCKS;            // grid-stride from here on: a few blocks per CU
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

}  // namespace

int lsq_snap_launch_digest(hipStream_t s, const void *p, uint64_t bytes, uint64_t first_word, unsigned long long *partials, unsigned long long *acc) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const long long nvec = bytes ? (long long)((a + bytes - (a & ~(uintptr_t)15) + 15) >> 4) : 0;
    const unsigned grid = snap_grid(nvec);
    hipLaunchKernelGGL(snap_digest_kernel, dim3(grid), dim3(SNAP_THREADS), 0, s, static_cast<const uint8_t *>(p), (unsigned long long)bytes,
                       (unsigned long long)first_word, partials);
    LSQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(snap_sum_kernel, dim3(1), dim3(SNAP_THREADS), 0, s, partials, (int)grid, (unsigned long long)(bytes * LSQ_SNAP_GOLD64), acc);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

int lsq_snap_launch_unpack(hipStream_t s, const uint8_t *rows, int64_t n, int m, uint8_t *codes_out, int64_t c0, int64_t cbytes, uint8_t *norms_out, int64_t r0,
                           int64_t rcount) {
    if (!codes_out) cbytes = 0;
    if (!norms_out) rcount = 0;
    if (c0 < 0 || cbytes < 0 || c0 + cbytes > n * m || r0 < 0 || rcount < 0 || r0 + rcount > n) {
        lsq_set_error("lsq_snap_launch_unpack: a range leaves the rows (c0=%lld cbytes=%lld r0=%lld rcount=%lld n=%lld m=%d)", (long long)c0, (long long)cbytes,
                      (long long)r0, (long long)rcount, (long long)n, m);
        return LSQ_EINVAL;
    }
    const long long items = ((cbytes + 15) >> 4) + ((rcount + 15) >> 4);
    if (items == 0) return LSQ_OK;
    const int vc = (reinterpret_cast<uintptr_t>(codes_out) & 15) == 0, vn = (reinterpret_cast<uintptr_t>(norms_out) & 15) == 0;
    hipLaunchKernelGGL(snap_unpack_kernel, dim3(snap_grid(items)), dim3(SNAP_THREADS), 0, s, rows, m, codes_out, (long long)c0, (long long)cbytes, norms_out,
                       (long long)r0, (long long)rcount, vc, vn);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

// ---- the host-only road (bodies: lsq_snapshot_check.h) ------------------------------------------------------------------------------------------------
extern "C" int lsq_snapshot_digest_cpu(const void *data, int64_t bytes, int64_t first_word, uint64_t *out) {
    if (!out || bytes < 0 || first_word < 0 || (bytes > 0 && !data)) { lsq_set_error("lsq_snapshot_digest_cpu: null pointer or negative size"); return LSQ_EINVAL; }
    *out = lsq_snap_digest(data, (uint64_t)bytes, (uint64_t)first_word);
    return LSQ_OK;
}

extern "C" int lsq_snapshot_write_cpu(const char *path, const lsq_snapshot_arrays *arrays) {
    lsq_snap_error err;
    const int rc = lsq_snap_write_file(path, arrays, &err);
    if (rc != LSQ_OK) lsq_set_error("lsq_snapshot_write_cpu: %s", err.text);
    return rc;
}

extern "C" int lsq_snapshot_inspect_cpu(const char *path, lsq_snapshot_info *out, int verify) {
    lsq_snap_error err;
    const int rc = lsq_snap_read_file(path, out, verify, nullptr, &err);
    if (rc != LSQ_OK) lsq_set_error("lsq_snapshot_inspect_cpu: %s", err.text);
    return rc;
}

extern "C" int lsq_snapshot_read_cpu(const char *path, lsq_snapshot_arrays *out) {
    if (!out) { lsq_set_error("lsq_snapshot_read_cpu: null argument"); return LSQ_EINVAL; }
    lsq_snap_error err;
    lsq_snapshot_info info;
    const int rc = lsq_snap_read_file(path, &info, 1, out, &err);
    if (rc != LSQ_OK) lsq_set_error("lsq_snapshot_read_cpu: %s", err.text);
    return rc;
}
