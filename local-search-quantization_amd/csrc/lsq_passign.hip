// lsq_passign.hip -- the coarse partition's ASSIGN on the f32 matrix cores (gfx950; option "partition_mfma").
//
// lsq_partition_assign answers "the nearest of nlist centroids for each of n rows" with the exact search of lsq_knn.hip: three VALU element-ops per
// (row, centroid, dimension), in a kernel laid out for 10^4 queries against 10^6 base rows.  The assign shape is the inverse -- 10^6 "queries", 10^3 .. 10^5
// base rows that fit in L2 -- and its answer is ONE id per row.  This unit finds it on the matrix cores and leaves the contract's bits to a recheck:
//
//   norms    knnm_norms_kernel (lsq_knnm.hip)   Nx[i] = SUM_s x_i[s]^2,  Nc[c] = SUM_s c[s]^2   (f32 fma sums; the centroids' every call: update rewrites them)
//   MFMA     passign_scan_kernel<TX, RES>       a = (Nc + Nx) - 2 <c, x> with <c, x> by v_mfma_f32_32x32x2_f32,  w = kappa_d (Nc + Nx) + eta_d,
//                                               lo = a - w, hi = a + w;  per row a running U = min hi (NaN ignored);  centroid c is a CANDIDATE of the row
//                                               unless lo > U, and joins the row's PENDING list
//   recheck  passign_recheck_kernel<TX>         the direct chain of every pending pair (subtract, multiply, add each rounded, s ascending from +0: the
//                                               contract's bits), the minimum by (lsq_adc_key(dist), list id) -> list_of_row, dist
//
// lo <= f <= hi for the chain's value f of a pair whenever hi is finite (lsq_knn_prefilter_bound's kappa, eta; the two-sided proof is DESIGN 4.35).  The
// argmin's f is at most every f_c', hence at most every hi that ever lowered U, and its own lo is at most its f: the winner and every exact tie with it are
// candidates whatever the order of the walk, however stale U is, and however the centroids are split among blocks (each part keeps a U of its own).  A NaN
// makes `lo > U` false: the pair is kept.  What the window cannot bound is how MANY candidates a row collects: a row whose list overflows, and a row
// whose Nx is not finite, is gathered and redone by the direct search (the host code below).
//
// passign_scan_kernel: 256 threads = 4 waves.  A block OWNS 128 data rows for the whole walk and streams the centroids of its part past them in tiles of
// 128: MFMA M carries the centroids, N the data rows, so a data row is a lane's accumulator COLUMN and the minimum over a tile's centroids is a reduction
// over the lane's own 64 accumulator values and one exchange with lane ^ 32.  Wave w owns rows 32 w .. 32 w + 31 against all 128 centroids of the tile
// (four 32 x 32 accumulators, 64 registers): a row's U, Nx and liveness live in ONE wave's registers, no barrier or LDS word is spent on them.
// RES = 1: the block's rows are staged ONCE, widened to f32, [128][ceil16(d) + 4] floats (pitch = 4 mod 8: sixteen lanes' 16-byte reads fall on sixteen
// distinct bank quads), and read from LDS for every centroid tile; only the centroid chunks (16 dimensions, double-buffered, the next chunk's global
// loads in flight under the MFMAs, one barrier per chunk) come from memory -- from L2, where nlist d 4 bytes of centroids stay.  RES = 0 (d > 256): both
// operands are staged per chunk, as knnm_scan_kernel does.  Rows >= n, centroids past the part and dimensions >= d are staged as zeros (padded centroids
// carry Nc = +inf: their hi never lowers U) and never emit; nothing at or past a row's d-th element is loaded.
#include <math.h>

#include <algorithm>

#include "lsq_internal.h"
#include "lsq_xload.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int PA_THREADS = 256;
constexpr int PA_T = 128;                    // data rows per block = centroids per tile
constexpr int PA_BK = 16;                    // dimensions staged per chunk
constexpr int PA_LD = PA_BK + 4;             // LDS pitch of a chunk panel (floats): 16-byte aligned rows, LD / 4 odd
constexpr int PA_SL = PA_T * PA_BK / PA_THREADS;      // staged elements per thread, chunk and operand (8)
constexpr int PA_FIXED = 2 * PA_T * PA_LD + 2 * PA_T; // floats of LDS before the row panel: the centroid panels [2][128][20], Nc of two tiles [2][128]
constexpr int PA_RES_MAX_D = 256;            // RES = 1 serves ceil16(d) <= 256: (5376 + 128 * 260) * 4 = 154 624 bytes of the CU's 160 KiB, one block per CU
constexpr int PA_CAP = 32;                   // default pending capacity of a row walked by one part (measured appends per row)
constexpr int PA_MAX_SPLITS = 64;

template <typename TX, int RES>
__global__ __launch_bounds__(PA_THREADS) void passign_scan_kernel(const TX *__restrict__ X, int64_t ldx, int n, int d, const float *__restrict__ cent,
                                                                  int nlist, int per_part, const float *__restrict__ nx, const float *__restrict__ nc,
                                                                  float kappa, float eta, unsigned *pcount, int pcap, int32_t *__restrict__ pend,
                                                                  int xpitch, int xvec) {
    extern __shared__ __attribute__((aligned(16))) float pa_lds[];
    float *cs = pa_lds;                                             // [2][PA_T * PA_LD]
    float *ncs = pa_lds + 2 * PA_T * PA_LD;                         // [2][PA_T]
    float *xs = pa_lds + PA_FIXED;                                  // RES: [PA_T][xpitch]; else [2][PA_T * PA_LD]
    const int t = threadIdx.x;
    const int r0 = blockIdx.x * PA_T;                               // the block's rows
    const int first = blockIdx.y * per_part;                        // the block's centroids: [first, last)
    const int last = first + per_part < nlist ? first + per_part : nlist;
    if (first >= last) return;
    const int nk = (d + PA_BK - 1) / PA_BK;
    // staging roles per chunk: element j of this thread is (centroid / row (t >> 4) + 16 j, dimension t & 15 of the chunk)
    const int kk = t & (PA_BK - 1), sr = t >> 4;
    float creg[PA_SL];
    TX xreg[RES ? 1 : PA_SL];
    auto fetch = [&](int c0, int k0) {                              // global -> registers: chunk k0 of centroids c0 .. c0 + 127 (RES = 0: and of the rows)
        const int k = k0 + kk;
#pragma unroll
        for (int j = 0; j < PA_SL; ++j) {
            const int c = c0 + sr + 16 * j;
            creg[j] = (c < last && k < d) ? cent[(int64_t)c * d + k] : 0.0f;
        }
        if constexpr (!RES) {
#pragma unroll
            for (int j = 0; j < PA_SL; ++j) {
                const int row = r0 + sr + 16 * j;
                xreg[j] = (row < n && k < d) ? X[(int64_t)row * ldx + k] : (TX)0;
            }
        }
    };
    auto stage = [&](int buf) {                                     // registers -> LDS, widened (exact)
#pragma unroll
        for (int j = 0; j < PA_SL; ++j) {
            cs[buf * PA_T * PA_LD + (sr + 16 * j) * PA_LD + kk] = creg[j];
            if constexpr (!RES) xs[buf * PA_T * PA_LD + (sr + 16 * j) * PA_LD + kk] = (float)xreg[j];
        }
    };
    if constexpr (RES) {
        // the block's rows, once: a thread moves FOUR components (f32: one 16-byte load, uint8: one dword, where the matrix and its pitch allow: xvec;
        // the row's last, partial quad and every unaligned matrix go element by element) and stores them as one 16-byte LDS write
        const int qq = t & 31, qr = t >> 5;
        const int dpad = nk * PA_BK;
        for (int k = 4 * qq; k < dpad; k += 128) {
#pragma unroll 4
            for (int j = 0; j < PA_T / 8; ++j) {
                const int rl = qr + 8 * j, row = r0 + rl;
                lsq_f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
                if (row < n && k < d) {
                    const TX *px = X + (int64_t)row * ldx + k;
                    if (xvec && k + 4 <= d) {
                        v = lsq_ld4(px);
                    } else {
                        v.x = (float)px[0];
                        if (k + 1 < d) v.y = (float)px[1];
                        if (k + 2 < d) v.z = (float)px[2];
                        if (k + 3 < d) v.w = (float)px[3];
                    }
                }
                *reinterpret_cast<lsq_f32x4 *>(xs + rl * xpitch + k) = v;
            }
        }
    }
    // compute roles: the lane's data row is column l31 of its wave's N tile
    const int lane = t & 63, wave = t >> 6, l31 = lane & 31, lhi = lane >> 5;
    const int grow = r0 + wave * 32 + l31;
    float nxv = grow < n ? nx[grow] : 0.0f;
    const bool live = grow < n && fabsf(nxv) < INFINITY;            // a row without a finite norm is redone by the direct search: it never emits
    if (!live) nxv = 0.0f;
    float U = INFINITY;
    fetch(first, 0);
    stage(0);
    int cur = 0, par = 0;
    for (int c0 = first; c0 < last; c0 += PA_T, par ^= 1) {
        // Nc of this tile's centroids: read after at least one barrier of the chunk loop, overwritten two tiles later (after the next tile's barriers)
        if (t < PA_T) ncs[par * PA_T + t] = c0 + t < last ? nc[c0 + t] : INFINITY;
        // a row whose pending list has already overflowed is redone whatever else it collects: stop its atomics
        const bool open = live && __hip_atomic_load(&pcount[grow], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= (unsigned)pcap;
        f32x16 acc[4];
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ti][r] = 0.0f;
        __syncthreads();                                            // the staged chunk (first tile: and the resident rows), ncs
        for (int kc = 0; kc < nk; ++kc) {
            const bool more_k = kc + 1 < nk, more = more_k || c0 + PA_T < last;
            if (more_k) fetch(c0, (kc + 1) * PA_BK);
            else if (more) fetch(c0 + PA_T, 0);
            const lsq_f32x4 *ap = reinterpret_cast<const lsq_f32x4 *>(cs + cur * PA_T * PA_LD + l31 * PA_LD + 8 * lhi);
            const lsq_f32x4 *bp = RES ? reinterpret_cast<const lsq_f32x4 *>(xs + (wave * 32 + l31) * xpitch + kc * PA_BK + 8 * lhi)
                                      : reinterpret_cast<const lsq_f32x4 *>(xs + cur * PA_T * PA_LD + (wave * 32 + l31) * PA_LD + 8 * lhi);
            const lsq_f32x4 b[2] = {bp[0], bp[1]};
            lsq_f32x4 a[4][2];
#pragma unroll
            for (int ti = 0; ti < 4; ++ti) { a[ti][0] = ap[ti * 32 * PA_LD / 4]; a[ti][1] = ap[ti * 32 * PA_LD / 4 + 1]; }
#pragma unroll
            for (int s = 0; s < 8; ++s) {                           // step s: dimensions s (lanes 0-31) and 8 + s (lanes 32-63) of the chunk
                const float bv = b[s >> 2][s & 3];
#pragma unroll
                for (int ti = 0; ti < 4; ++ti) acc[ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ti][s >> 2][s & 3], bv, acc[ti], 0, 0, 0);
            }
            if (more) stage(cur ^ 1);                               // the other buffer was last read one chunk ago (barrier below)
            __syncthreads();
            cur ^= 1;
        }
        // epilogue: accumulator ti[r] is centroid c0 + 32 ti + (r & 3) + 8 (r >> 2) + 4 lhi against the lane's row.  Branch-free first: the tile's
        // smallest hi of the column (this lane's 64 values, then lane ^ 32's) lowers U; then one bit per pair under the UPDATED U; then the rare appends
        const float *ncl = ncs + par * PA_T + 4 * lhi;
        float m = INFINITY;
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float nsum = ncl[ti * 32 + (r & 3) + 8 * (r >> 2)] + nxv;
                const float av = fmaf(-2.0f, acc[ti][r], nsum);     // (Nc + Nx) - 2 dot: 2 dot is exact, one rounding
                const float hi = av + (kappa * nsum + eta);
                m = hi < m ? hi : m;                                // NaN is ignored
            }
        }
        const float mo = __shfl_xor(m, 32);
        m = mo < m ? mo : m;
        U = m < U ? m : U;
        uint32_t keep[2] = {0u, 0u};
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float nsum = ncl[ti * 32 + (r & 3) + 8 * (r >> 2)] + nxv;
                const float av = fmaf(-2.0f, acc[ti][r], nsum);
                const float lo = av - (kappa * nsum + eta);
                keep[ti >> 1] |= (lo > U) ? 0u : (1u << (16 * (ti & 1) + r));      // the negated form: NaN anywhere keeps the pair
            }
        }
        if (open) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                uint32_t w = keep[h];
                while (w) {
                    const int bit = __builtin_ctz(w);
                    w &= w - 1u;
                    const int c = c0 + (2 * h + (bit >> 4)) * 32 + (bit & 3) + 8 * ((bit & 15) >> 2) + 4 * lhi;
                    if (c >= last) continue;                        // a padded centroid never emits
                    const unsigned at = atomicAdd(&pcount[grow], 1u);
                    if (at < (unsigned)pcap) pend[(int64_t)grow * pcap + at] = c;
                }
            }
        }
    }
}

// words of a call (unsigned long long [4], zeroed by the host): rows to redo, rows without a finite norm, rows whose list overflowed, appends
enum { PW_REDO = 0, PW_NONFINITE = 1, PW_OVERFLOW = 2, PW_PENDING = 3 };

// Sixteen lanes own ONE row and walk its candidates one after another.  Per 16 dimensions: the lanes read 16 consecutive elements of the centroid and of
// the row (64 contiguous bytes of an f32 row), each forms its rounded difference and its rounded square, and the chain acc = acc + e_s e_s runs in
// ascending s over the sixteen squares handed round the group -- every lane adds the same values in the same order and holds the same acc.  The minimum
// by (key, id) needs no exchange for the same reason.  A row that cannot be decided here joins the redo list (one atomic per such row).
template <typename TX>
__global__ __launch_bounds__(PA_THREADS) void passign_recheck_kernel(const TX *__restrict__ X, int64_t ldx, int n, int d, const float *__restrict__ cent,
                                                                     const float *__restrict__ nx, const unsigned *__restrict__ pcount, int pcap,
                                                                     const int32_t *__restrict__ pend, int32_t *__restrict__ lor, float *__restrict__ dist,
                                                                     int32_t *__restrict__ redo, unsigned long long *__restrict__ words) {
    const int l16 = threadIdx.x & 15;
    const int row = blockIdx.x * (PA_THREADS / 16) + (threadIdx.x >> 4);
    unsigned have = 0;
    bool finite = true;
    if (row < n) {
        have = pcount[row];
        finite = fabsf(nx[row]) < INFINITY;
    }
    const bool over = have > (unsigned)pcap;
    const bool again = row < n && (!finite || over || have == 0);
    if (l16 == 0 && row < n) {
        if (again) {
            redo[atomicAdd(&words[PW_REDO], 1ull)] = row;
            atomicAdd(&words[!finite ? PW_NONFINITE : PW_OVERFLOW], 1ull);
        }
        atomicAdd(&words[PW_PENDING], (unsigned long long)have);
    }
    if (row >= n || again) have = 0;                                 // (the group stays: its shuffles are group-wide)
    const TX *__restrict__ x = X + (int64_t)(row < n ? row : 0) * ldx;
    uint32_t bkey = 0xffffffffu;
    int32_t bid = INT32_MAX;
    for (unsigned j = 0; j < have; ++j) {
        const int32_t c = pend[(int64_t)row * pcap + j];
        const float *__restrict__ cr = cent + (int64_t)c * d;
        float acc = 0.0f;
        for (int k0 = 0; k0 < d; k0 += 16) {
            const int s = k0 + l16;
            float sq = 0.0f;
            if (s < d) {
                const float e = cr[s] - (float)x[s];                // rounded; the square, rounded; then the adds (no FMA)
                sq = e * e;
            }
            const int kc = d - k0 < 16 ? d - k0 : 16;
            for (int q = 0; q < kc; ++q) acc = acc + __shfl(sq, q, 16);
        }
        const uint32_t key = lsq_adc_key(acc);
        if (key < bkey || (key == bkey && c < bid)) { bkey = key; bid = c; }
    }
    if (have > 0 && l16 == 0) {
        lor[row] = bid;
        if (dist) dist[row] = lsq_adc_unkey(bkey);
    }
}

// the redo rows, dense: stage [j][d] = X[redo[j]][0 .. d)
template <typename TX>
__global__ __launch_bounds__(PA_THREADS) void passign_gather_kernel(const TX *__restrict__ X, int64_t ldx, int d, const int32_t *__restrict__ redo, int count,
                                                                    TX *__restrict__ stage) {
    const int j = blockIdx.x;
    if (j >= count) return;
    const TX *__restrict__ x = X + (int64_t)redo[j] * ldx;
    for (int s = threadIdx.x; s < d; s += PA_THREADS) stage[(int64_t)j * d + s] = x[s];
}

__global__ __launch_bounds__(PA_THREADS) void passign_scatter_kernel(const int32_t *__restrict__ redo, int count, const int32_t *__restrict__ ids,
                                                                     const float *__restrict__ dd, int32_t *__restrict__ lor, float *__restrict__ dist) {
    const int j = blockIdx.x * PA_THREADS + threadIdx.x;
    if (j >= count) return;
    lor[redo[j]] = ids[j];
    if (dist) dist[redo[j]] = dd[j];
}

__global__ void passign_clear_kernel(unsigned *__restrict__ pcount, int n, unsigned long long *__restrict__ words) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) pcount[i] = 0u;
    if (i < 4) words[i] = 0ull;
}

// ---- the host rules: which kernel, how much LDS, how the centroids are split -------------------------------------------------------------------------------
struct Geometry { int resident, xpitch, splits, per_part, cap; size_t lds; };

// lds_limit: the LDS one block may have on this device.  RES = 1 iff ceil16(d) <= 256 and its panel fits; splits > 1 iff the row blocks alone would not
// fill the chip: then ~512 blocks, parts of whole tiles, at most PA_MAX_SPLITS.  cap: a part contributes about 1 + ln(its tiles) candidates per row
Geometry passign_geometry(int64_t n, int nlist, int d, size_t lds_limit, int cap_opt) {
    Geometry g{};
    const int dpad = (d + PA_BK - 1) / PA_BK * PA_BK;
    g.xpitch = dpad + 4;
    g.lds = sizeof(float) * ((size_t)PA_FIXED + (size_t)PA_T * (size_t)g.xpitch);
    g.resident = dpad <= PA_RES_MAX_D && g.lds <= lds_limit;
    if (!g.resident) { g.xpitch = PA_LD; g.lds = sizeof(float) * ((size_t)PA_FIXED + 2 * PA_T * PA_LD); }
    const int64_t row_blocks = (n + PA_T - 1) / PA_T;
    const int tiles = (nlist + PA_T - 1) / PA_T;
    int splits = 1;
    if (row_blocks < 256) splits = (int)std::min<int64_t>(std::min(tiles, PA_MAX_SPLITS), (512 + row_blocks - 1) / row_blocks);
    const int part_tiles = (tiles + splits - 1) / splits;
    g.per_part = part_tiles * PA_T;
    g.splits = (nlist + g.per_part - 1) / g.per_part;
    g.cap = cap_opt > 0 ? cap_opt : (g.splits == 1 ? PA_CAP : PA_CAP + 8 * g.splits);
    return g;
}

template <typename TX>
int launch_scan(hipStream_t s, const Geometry &g, const TX *X, int64_t ldx, int n, int d, const float *cent, int nlist, const float *nx, const float *nc,
                float kappa, float eta, unsigned *pcount, int32_t *pend) {
    const uintptr_t al = (uintptr_t)X | (uintptr_t)(ldx * (int64_t)sizeof(TX));
    const int xvec = sizeof(TX) == 4 ? (al & 15) == 0 : (al & 3) == 0;
    const dim3 grid((unsigned)((n + PA_T - 1) / PA_T), (unsigned)g.splits), block(PA_THREADS);
#define PA_LAUNCH(R)                                                                                                                                       \
    do {                                                                                                                                                   \
        LSQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&passign_scan_kernel<TX, R>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds)); \
        hipLaunchKernelGGL((passign_scan_kernel<TX, R>), grid, block, g.lds, s, X, ldx, n, d, cent, nlist, g.per_part, nx, nc, kappa, eta, pcount, g.cap,   \
                           pend, g.xpitch, xvec);                                                                                                          \
    } while (0)
    if (g.resident) PA_LAUNCH(1);
    else PA_LAUNCH(0);
#undef PA_LAUNCH
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

}  // namespace

struct lsq_passign_state {
    DevBuf nx, nc, pcount, pend, redo, words, g_rows, g_ids, g_dist;
    PhaseClock<5> clock;
    size_t lds_limit = 160 * 1024;                     // gfx950: the LDS of a CU, all of which one block may have
};

void lsq_passign_free(lsq_passign_state *st) {
    if (!st) return;
    DevBuf *bufs[] = {&st->nx, &st->nc, &st->pcount, &st->pend, &st->redo, &st->words, &st->g_rows, &st->g_ids, &st->g_dist};
    for (DevBuf *b : bufs) b->release();
    st->clock.release();
    delete st;
}

namespace {

// rows [0, n) of one pass: every buffer is the state's; *redo_rows etc. are added to the account
template <typename TX>
int run_rows(hipStream_t s, lsq_passign_state *st, const lsq_passign_call &c, const Geometry &g, const TX *X, int n, int32_t *lor, float *dist, float kappa,
             float eta, lsq_partition_mfma_info *info, bool *off) {
    const int d = c.d;
    LSQ_TRY(st->nx.ensure(sizeof(float) * (size_t)n));
    LSQ_TRY(st->pcount.ensure(sizeof(unsigned) * (size_t)n));
    LSQ_TRY(st->pend.ensure(sizeof(int32_t) * (size_t)n * (size_t)g.cap));
    LSQ_TRY(st->redo.ensure(sizeof(int32_t) * (size_t)n));
    unsigned long long *words = st->words.as<unsigned long long>();
    LSQ_TRY(st->clock.begin(c.profile != 0));
    LSQ_TRY(st->clock.mark(s));
    hipLaunchKernelGGL(passign_clear_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, st->pcount.as<unsigned>(), n, words);
    LSQ_HIP(hipGetLastError());
    LSQ_TRY(lsq_knnm_launch_row_norms(s, X, sizeof(TX) == 1, c.ldx, n, d, st->nx.as<float>()));
    LSQ_TRY(lsq_knnm_launch_row_norms(s, c.cent, 0, d, c.nlist, d, st->nc.as<float>()));
    LSQ_TRY(st->clock.mark(s));
    LSQ_TRY(launch_scan(s, g, X, c.ldx, n, d, c.cent, c.nlist, st->nx.as<float>(), st->nc.as<float>(), kappa, eta, st->pcount.as<unsigned>(),
                        st->pend.as<int32_t>()));
    LSQ_TRY(st->clock.mark(s));
    hipLaunchKernelGGL((passign_recheck_kernel<TX>), dim3((unsigned)((n + 15) / 16)), dim3(PA_THREADS), 0, s, X, c.ldx, n, d, c.cent, st->nx.as<float>(),
                       st->pcount.as<unsigned>(), g.cap, st->pend.as<int32_t>(), lor, dist, st->redo.as<int32_t>(), words);
    LSQ_HIP(hipGetLastError());
    LSQ_TRY(st->clock.mark(s));
    unsigned long long w[4];
    LSQ_HIP(hipMemcpyAsync(w, words, sizeof(w), hipMemcpyDeviceToHost, s));
    LSQ_HIP(hipStreamSynchronize(s));
    const int count = (int)w[PW_REDO];
    info->nonfinite_rows += (int64_t)w[PW_NONFINITE];
    info->overflow_rows += (int64_t)w[PW_OVERFLOW];
    info->pending += (int64_t)w[PW_PENDING];
    info->redo_rows += count;
    if ((int64_t)count * 2 > (int64_t)n) *off = true;                // the window decides too little on this data: the caller finishes on the direct road
    if (count > 0 && !*off) {
        LSQ_TRY(st->g_rows.ensure(sizeof(TX) * (size_t)count * (size_t)d));
        LSQ_TRY(st->g_ids.ensure(sizeof(int32_t) * (size_t)count));
        LSQ_TRY(st->g_dist.ensure(sizeof(float) * (size_t)count));
        hipLaunchKernelGGL((passign_gather_kernel<TX>), dim3((unsigned)count), dim3(PA_THREADS), 0, s, X, c.ldx, d, st->redo.as<int32_t>(), count,
                           st->g_rows.as<TX>());
        LSQ_HIP(hipGetLastError());
        LSQ_TRY(lsq_index_knn(c.ix, st->g_dist.as<float>(), st->g_ids.as<int>(), st->g_rows.p, sizeof(TX) == 1, count, d, 1, 0, 1));
        hipLaunchKernelGGL(passign_scatter_kernel, dim3((unsigned)((count + PA_THREADS - 1) / PA_THREADS)), dim3(PA_THREADS), 0, s, st->redo.as<int32_t>(),
                           count, st->g_ids.as<int32_t>(), st->g_dist.as<float>(), lor, dist);
        LSQ_HIP(hipGetLastError());
    }
    LSQ_TRY(st->clock.mark(s));
    float ms[4];
    LSQ_TRY(st->clock.read(ms));
    info->norms_ms += ms[0]; info->scan_ms += ms[1]; info->recheck_ms += ms[2]; info->redo_ms += ms[3];
    return LSQ_OK;
}

}  // namespace

// The call on device buffers.  *done = 1: lor (and dist, if wanted) hold the answer.  *done = 0: the road did not serve the call (info->reason) or
// switched itself off (info->switched_off): nothing of lor / dist counts, the caller runs the direct search
int lsq_passign_run(hipStream_t s, lsq_passign_state **stp, const lsq_passign_call &c, lsq_partition_mfma_info *info, int *done) {
    *done = 0;
    *info = lsq_partition_mfma_info{};
    info->rows = c.n; info->nlist = c.nlist;
    if (c.d > LSQ_KNN_PREFILTER_MAX_D) { info->reason = LSQ_PARTITION_MFMA_WIDE; return LSQ_OK; }
    if (!*stp) *stp = new lsq_passign_state();
    lsq_passign_state *st = *stp;
    float kappa = 0.0f, eta = 0.0f;
    LSQ_TRY(lsq_knn_prefilter_bound(c.d, &kappa, &eta));
    // rows per pass: the pending lists of one pass stay within 256 MiB
    const Geometry g0 = passign_geometry(c.n, c.nlist, c.d, st->lds_limit, c.cap_opt);
    int64_t pass = ((int64_t)64 << 20) / g0.cap / PA_T * PA_T;
    if (pass < PA_T) pass = PA_T;
    if (pass > c.n) pass = c.n;
    const Geometry g = pass == c.n ? g0 : passign_geometry(pass, c.nlist, c.d, st->lds_limit, c.cap_opt);
    info->served = 1; info->resident = g.resident; info->splits = g.splits; info->cap = g.cap;
    info->pairs = c.n * (int64_t)c.nlist; info->kappa = kappa; info->eta = eta;
    LSQ_TRY(st->nc.ensure(sizeof(float) * (size_t)c.nlist));
    LSQ_TRY(st->words.ensure(4 * sizeof(unsigned long long)));
    bool off = false;
    for (int64_t i0 = 0; i0 < c.n && !off; i0 += pass) {
        const int rows = (int)std::min<int64_t>(pass, c.n - i0);
        float *dd = c.dist ? c.dist + i0 : nullptr;
        if (c.x_u8) LSQ_TRY(run_rows(s, st, c, g, static_cast<const uint8_t *>(c.X) + i0 * c.ldx, rows, c.lor + i0, dd, kappa, eta, info, &off));
        else LSQ_TRY(run_rows(s, st, c, g, static_cast<const float *>(c.X) + i0 * c.ldx, rows, c.lor + i0, dd, kappa, eta, info, &off));
    }
    info->switched_off = off;
    *done = !off;
    return LSQ_OK;
}
