// lsq_kmeans.hip -- the two steps of PQ / OPQ training that were host glue: cluster means and k-means++ seeding, for all m sub-spaces of a
// vector set in one call, X resident in device memory.
//
// The sub-space structure is a cover map dim2C (d x m, 0 / 1; HOST bytes [m][d], checked by the caller) as in the structured codebook update (lsq_lsqr.hip):
// codebook j sees the dimensions it covers only, K (m h, d) is exactly +0.0 elsewhere.  PQ / OPQ: codebook j covers splitarray(1:d, m)[j]; plain k-means: m = 1.
//
// (a) CLUSTER MEANS    update_centers!, src/opq/kmeans.jl:77-123.  The rows are sorted by (codebook, code) once per call (lsq_sort_rows_by_code, the sort of the
//     device LSQR) and one thread per (column c, dimension t) walks the column's rows in ascending order adding X[row][t] with plain f32 adds from +0.0 --
//     numpy's np.add.at order, no atomics -- then divides by the count in double and rounds to f32 (numpy's `f32 /= int64`): the bits of the host trainers'
//     _centers.  An empty cluster takes its row of K_prev (NULL: zero); K_prev may be K_out itself.  The walk is a chain of n / h dependent adds per thread with
//     16 loads in flight: latency-bound, not byte-bound.
// (b) K-MEANS++ SEEDING    Clustering.kmeans(..., init=:kmpp), src/pq/PQ.jl:60.  No RNG on the device: the caller draws u (m x h doubles in [0, 1)).
//     step 0      row min(n - 1, floor(u[j][0] n))
//     step k >= 1 d2[i][j] = min(d2[i][j], SUM_t (x_it - c_t)^2): f32, direct form, covered dimensions ascending, no FMA (the convention of lsq_knn.hip), c the
//                 centre chosen at step k - 1; tot = SUM_i d2[i][j] in double; tot > 0: the first row whose double prefix sum exceeds u[j][k] tot (a row at
//                 distance 0 adds nothing and is never that row); else row min(n - 1, floor(u[j][k] n)).
//     One step = kpp_dist (one pass over X: distances, minima, per-block double partial sums) + kpp_locate (m blocks: the prefix search and the copy of the chosen
//     row into K).  The chosen index stays on the device between steps; nothing waits for the host.
//     ORDER OF THE DOUBLE SUMS (fixed by n alone, so two calls return the same rows): a block owns rpb = 64 ceil(n / (64 * 4096)) consecutive rows (at most 4096
//     blocks); inside it tiles of 64 rows are summed by a 64-lane xor butterfly (32, 16, ..., 1) and the tiles added in ascending order.  kpp_locate: thread q
//     adds its per = ceil(nblocks / 256) consecutive block sums in ascending order; 16 consecutive thread sums make a group sum, added in ascending order; tot =
//     the 16 group sums added in ascending order.  The prefix runs through the group sums, then the thread sums of the group it crosses in, then the block sums
//     of that thread, then the rows of that block: 256 at a time, through sums of 16 consecutive rows and then row by row.  Rounding can leave a level without a
//     crossing although the level above found one: the last entry with a positive value is taken there (within the rounding of the sums).
#include "lsq_internal.h"

#include <cmath>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr int TILE = 64;           // rows per tile of the distance pass
constexpr int MAXBLK = 4096;       // blocks (per-block partial sums per sub-space) of the distance pass
constexpr int CH = 64;             // dimensions of a tile staged through LDS at a time (measured against 32 and 128: DESIGN 4.14)
constexpr int LDT = CH + 4;        // floats per staged row
constexpr int CEN_MAX = 10900;     // floats of centre values that fit the rest of the distance pass's 64 KiB of LDS

// the cover map as the kernels read it (device memory)
struct KCover {
    const uint8_t *map;   // [m][d] 0 / 1
    const int *dims;      // [m][d] the dimensions codebook j covers, ascending (the first cnt[j] entries of row j)
    const int *cnt;       // [m]
    const int *off;       // [m] where codebook j's centre starts in the LDS window: the prefix sum of the cnt rounded up to multiples of 4
    const int *lo;        // [m] first covered dimension
    const int *shape;     // [m] 0: any list, 1: contiguous lo .. lo + cnt - 1, 2: contiguous and float4-aligned (lo, cnt, d multiples of 4)
};

// ---- (a) cluster means ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void kmeans_centers_walk(const float *__restrict__ X, const uint64_t *__restrict__ sorted, const int64_t *__restrict__ seg,
                                                          const uint8_t *__restrict__ map, const float *Kprev, int d, float *K, int *__restrict__ counts) {
    const int c = blockIdx.x;
    const int t = blockIdx.y * 64 + threadIdx.x;
    const int64_t e0 = seg[c], e1 = seg[c + 1];
    if (t == 0 && counts) counts[c] = (int)(e1 - e0);
    if (t >= d) return;
    const int64_t o = (int64_t)c * d + t;
    if (!map[(int64_t)(c / LSQ_H) * d + t]) { K[o] = 0.0f; return; }
    if (e1 == e0) { K[o] = Kprev ? Kprev[o] : 0.0f; return; }      // Kprev may alias K: the thread that reads an entry is the one that writes it
    float acc = 0.0f;
    int64_t e = e0;
    constexpr int F = 16;                                          // rows in flight; the additions stay in row order
    for (; e + F <= e1; e += F) {
        float x[F];
#pragma unroll
        for (int q = 0; q < F; ++q) x[q] = X[(int64_t)(uint32_t)sorted[e + q] * d + t];
#pragma unroll
        for (int q = 0; q < F; ++q) acc += x[q];
    }
    for (; e < e1; ++e) acc += X[(int64_t)(uint32_t)sorted[e] * d + t];
    K[o] = (float)((double)acc / (double)(e1 - e0));
}

// ---- (b) seeding ------------------------------------------------------------------------------------------------------------------------------------
__device__ inline int64_t kpp_uniform_row(double u, int64_t n) {
    int64_t r = (int64_t)floor(u * (double)n);
    if (r > n - 1) r = n - 1;
    return r < 0 ? 0 : r;
}

// one pass over X: d2[i][j] = min(d2[i][j], ||x_i - c_j||^2 over codebook j's dimensions) (first: no minimum), part[j][block] = the block's sum of the new d2.
// A tile of TILE rows goes through LDS CH dimensions at a time (coalesced float4 loads; a row-per-lane walk straight from memory touches 64 cache lines per
// load and spills the L1 at wide sub-spaces); wave w then adds, for the sub-spaces w, w + 4, ... and one row per lane, the covered dimensions of the chunk to
// its running sums -- chunks ascending, dimensions ascending inside a chunk: the order of the rule.  Rows of CH + 4 floats: the float4 reads of the 16 lanes an
// LDS cycle serves fall on 16 different 4-bank slots.
// dynamic LDS: [16] doubles (the block's running sums), [TILE * 16] floats (the tile's d2), [TILE][CH + 4] floats (the chunk), [total] floats (the m centres)
template <bool LDS_CEN>
__global__ __launch_bounds__(256) void kpp_dist(const float *__restrict__ X, int64_t n, int d, int m, int64_t rpb, int nblocks, KCover C,
                                                const int64_t *__restrict__ cur, float *__restrict__ d2, double *__restrict__ part, int first, int vec_ok) {
    extern __shared__ double smem[];
    double *accp = smem;
    float *sv = reinterpret_cast<float *>(smem + LSQ_MAX_M);
    float *tile = sv + TILE * LSQ_MAX_M;
    float *cen = tile + TILE * LDT;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < LSQ_MAX_M) accp[tid] = 0.0;
    if (LDS_CEN) {
        for (int j = 0; j < m; ++j) {
            const int64_t ci = cur[j];
            for (int k = tid; k < C.cnt[j]; k += 256) cen[C.off[j] + k] = X[ci * d + C.dims[(int64_t)j * d + k]];
        }
    }
    __syncthreads();
    const bool vec = vec_ok && (d & 3) == 0;                       // float4 loads need 16-byte aligned rows
    const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = r0 + rpb < n ? r0 + rpb : n;
    for (int64_t q0 = r0; q0 < r1; q0 += TILE) {
        const int rows = (int)(r1 - q0 < TILE ? r1 - q0 : TILE);
        float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};                      // running sums of (row `lane`, sub-space w + 4 q)
        int kp[4] = {0, 0, 0, 0};                                   // list covers: the next entry of the sub-space's list
        for (int c0 = 0; c0 < d; c0 += CH) {
            const int cw = d - c0 < CH ? d - c0 : CH;
            if (vec) {
                const int c = 4 * (tid % (CH / 4));
                if (c < cw)
                    for (int r = tid / (CH / 4); r < rows; r += 256 / (CH / 4))
                        *reinterpret_cast<float4 *>(tile + r * LDT + c) = *reinterpret_cast<const float4 *>(X + (q0 + r) * d + c0 + c);
            } else {
                const int c = tid % CH;
                if (c < cw)
                    for (int r = tid / CH; r < rows; r += 256 / CH) tile[r * LDT + c] = X[(q0 + r) * d + c0 + c];
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = w + 4 * q;
                if (j < m && lane < rows) {
                    const int cnt = C.cnt[j], lo = C.lo[j], shape = C.shape[j];
                    const float *row = tile + lane * LDT - c0;      // row[t]: dimension t of this lane's row
                    const float *cg = LDS_CEN ? cen + C.off[j] : nullptr;
                    const float *cx = X + cur[j] * d;               // !LDS_CEN: the centre's row, read through the caches
                    float acc = s[q];
                    if (shape != 0) {
                        const int t0 = lo > c0 ? lo : c0, t1 = lo + cnt < c0 + cw ? lo + cnt : c0 + cw;
                        if (shape == 2 && vec) {
                            for (int t = t0; t < t1; t += 4) {
                                const float4 a = *reinterpret_cast<const float4 *>(row + t);
                                const float4 b = *reinterpret_cast<const float4 *>(LDS_CEN ? cg + (t - lo) : cx + t);      // off[j], lo and t are multiples of 4
                                const float e0 = a.x - b.x, e1 = a.y - b.y, e2 = a.z - b.z, e3 = a.w - b.w;
                                acc = acc + e0 * e0; acc = acc + e1 * e1; acc = acc + e2 * e2; acc = acc + e3 * e3;
                            }
                        } else {
                            for (int t = t0; t < t1; ++t) { const float e = row[t] - (LDS_CEN ? cg[t - lo] : cx[t]); acc = acc + e * e; }
                        }
                    } else {
                        const int *dj = C.dims + (int64_t)j * d;
                        int k = kp[q];
                        while (k < cnt) {
                            const int t = dj[k];
                            if (t >= c0 + cw) break;
                            const float e = row[t] - (LDS_CEN ? cg[k] : cx[t]);
                            acc = acc + e * e;
                            ++k;
                        }
                        kp[q] = k;
                    }
                    s[q] = acc;
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (w + 4 * q < m) sv[lane * m + w + 4 * q] = s[q];
        __syncthreads();
        for (int e = tid; e < TILE * m; e += 256) {                 // vector-major, as d2 lies in memory
            float v = 0.0f;
            if (e < rows * m) {
                const int64_t o = q0 * m + e;
                v = sv[e];
                if (!first) { const float old = d2[o]; v = v < old ? v : old; }
                d2[o] = v;
            }
            sv[e] = v;
        }
        __syncthreads();
        for (int j = w; j < m; j += 4) {                            // wave w sums the tile's rows of the sub-spaces w, w + 4, ...: one row per lane, xor butterfly
            double v = (double)sv[lane * m + j];
#pragma unroll
            for (int x = 32; x >= 1; x >>= 1) v += __shfl_xor(v, x);
            if (lane == 0) accp[j] += v;
        }
        __syncthreads();
    }
    if (tid < m) part[(int64_t)tid * nblocks + blockIdx.x] = accp[tid];
}

// Prefix search, thread 0.  kpp_find: the first entry of v[0 .. cnt) at which the running sum, started at `run`, exceeds target (crossed), else the last
// entry with a positive value (the rounding of the level above), else idx = -1; before = the sum in front of that entry, after = the sum past all cnt.
// cnt <= 16 here; no early exit, so that the loads are not serialised behind the comparisons.
struct KppHit { int idx; bool crossed; double before, after; };
template <class T>
__device__ inline KppHit kpp_find(const T *v, int cnt, double target, double run) {
    double r = run, before = run, last_before = run;
    int sel = -1, last = -1;
    for (int q = 0; q < cnt; ++q) {
        const double x = (double)v[q];
        const double nx = r + x;
        if (sel < 0 && nx > target) { sel = q; before = r; }
        if (x > 0.0) { last = q; last_before = r; }
        r = nx;
    }
    KppHit h;
    h.crossed = sel >= 0;
    h.idx = sel >= 0 ? sel : last;
    h.before = sel >= 0 ? before : last_before;
    h.after = r;
    return h;
}
// two levels over v[0 .. cnt), cnt <= 256: g[q] = v[16 q] + ... + v[16 q + 15] (added in ascending order by kpp_groups); the prefix runs through the group
// sums, then through the entries of the group it crosses in
template <class T>
__device__ inline KppHit kpp_find2(const T *v, const double *g, int cnt, double target, double run) {
    KppHit a = kpp_find(g, (cnt + 15) >> 4, target, run);
    if (a.idx < 0) return a;
    const int base = a.idx << 4;
    KppHit b = kpp_find(v + base, cnt - base < 16 ? cnt - base : 16, target, a.before);
    b.idx = b.idx < 0 ? -1 : base + b.idx;
    b.crossed = a.crossed;
    b.after = a.after;
    return b;
}
template <class T>
__device__ inline void kpp_groups(const T *v, int cnt, double *g) {      // threads 0 .. 15
    const int q = threadIdx.x;
    if (q >= 16) return;
    double s = 0.0;
    for (int e = q << 4; e < (q << 4) + 16 && e < cnt; ++e) s += (double)v[e];
    g[q] = s;
}

struct KppU { double u[LSQ_MAX_M]; };      // u[j][k] of one step, by value

// block j: choose the row of step k for sub-space j (see the head of the file), remember it (cur, idxs) and copy it into K, zero outside the cover
__global__ __launch_bounds__(256) void kpp_locate(const float *__restrict__ X, int64_t n, int d, int64_t rpb, int nblocks, const uint8_t *__restrict__ map,
                                                  KppU U, int k, const float *__restrict__ d2, int m, const double *__restrict__ part,
                                                  int64_t *__restrict__ cur, int64_t *__restrict__ idxs, float *__restrict__ K) {
    __shared__ double S[256];
    __shared__ double P[16];
    __shared__ double G[16];
    __shared__ float rowv[256];
    __shared__ int64_t pick_s;
    __shared__ int blk_s, state_s;      // state: 0 searching, 1 found
    __shared__ double run_s, target_s;
    const int j = blockIdx.x, tid = threadIdx.x;
    const double uk = U.u[j];
    if (k == 0) {
        if (tid == 0) pick_s = kpp_uniform_row(uk, n);
        __syncthreads();
    } else {
        const int per = (nblocks + 255) / 256;                    // <= 16 (nblocks <= 4096)
        {
            const int b0 = tid * per, b1 = b0 + per < nblocks ? b0 + per : nblocks;
            double s = 0.0;
            for (int b = b0; b < b1; ++b) s += part[(int64_t)j * nblocks + b];
            S[tid] = s;
        }
        __syncthreads();
        kpp_groups(S, 256, G);
        __syncthreads();
        if (tid == 0) {
            double tot = 0.0;
            for (int q = 0; q < 16; ++q) tot += G[q];
            state_s = 0; blk_s = 0;
            if (!(tot > 0.0)) { pick_s = kpp_uniform_row(uk, n); state_s = 1; }
            else {
                const double target = uk * tot;
                const KppHit h = kpp_find2(S, G, 256, target, 0.0);      // idx >= 0: tot > 0
                blk_s = (h.idx < 0 ? 0 : h.idx) * per;
                run_s = h.before; target_s = target;
            }
        }
        __syncthreads();
        if (state_s == 0) {                                       // the block sums of the thread the prefix crosses in
            const int b0 = blk_s;
            const int cntb = b0 + per < nblocks ? per : nblocks - b0;
            if (tid < cntb) P[tid] = part[(int64_t)j * nblocks + b0 + tid];
            __syncthreads();
            if (tid == 0) {
                const KppHit h = kpp_find(P, cntb, target_s, run_s);
                blk_s = b0 + (h.idx < 0 ? 0 : h.idx);
                run_s = h.before;
                pick_s = -1;
            }
            __syncthreads();
            const int64_t r0 = (int64_t)blk_s * rpb, r1 = r0 + rpb < n ? r0 + rpb : n;
            int64_t last_pos = -1;                                // thread 0: the last row of the block at a positive distance
            for (int64_t q0 = r0; q0 < r1; q0 += 256) {           // the rows of that block, 256 at a time
                const int rows = (int)(r1 - q0 < 256 ? r1 - q0 : 256);
                if (tid < rows) rowv[tid] = d2[(q0 + tid) * m + j];
                __syncthreads();
                kpp_groups(rowv, rows, G);
                __syncthreads();
                if (tid == 0) {
                    const KppHit h = kpp_find2(rowv, G, rows, target_s, run_s);
                    if (h.crossed && h.idx >= 0) { pick_s = q0 + h.idx; state_s = 1; }
                    else { if (h.idx >= 0) last_pos = q0 + h.idx; run_s = h.after; }
                }
                __syncthreads();
                if (state_s == 1) break;
            }
            if (tid == 0 && state_s == 0) pick_s = last_pos >= 0 ? last_pos : kpp_uniform_row(uk, n);
            __syncthreads();
        }
    }
    int64_t pick = pick_s;
    if (pick > n - 1) pick = n - 1;
    if (pick < 0) pick = 0;
    if (tid == 0) { cur[j] = pick; if (idxs) idxs[(int64_t)j * LSQ_H + k] = pick; }
    const int64_t o = ((int64_t)j * LSQ_H + k) * d;
    for (int t = tid; t < d; t += 256) K[o + t] = map[(int64_t)j * d + t] ? X[pick * d + t] : 0.0f;
}

__global__ void kmeans_fill_i64(int64_t *p, int64_t count, int64_t v) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < count) p[e] = v;
}

}  // namespace

struct lsq_kmeans_state {
    DevBuf keys;      // means: (column, row) keys, sorted keys, segment starts, the sort's temporary storage
    DevBuf cover;     // the cover map and its lists
    DevBuf work;      // seeding: d2 (when the caller wants none), the per-block partial sums, the chosen rows
    std::vector<char> cover_host;      // host image of `cover`
    std::vector<uint8_t> cover_key;    // the map `cover` was built from, and its shape: an unchanged map is not uploaded again
    int cover_d = 0, cover_m = 0;
    int total = 0;                     // floats of the LDS window of the centres
    KCover C{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};

void lsq_kmeans_free(lsq_kmeans_state *st) {
    if (!st) return;
    st->keys.release();
    st->cover.release();
    st->work.release();
    delete st;
}

// the map's lists, built on the host and uploaded when the map differs from the one already there
static int kmeans_cover(hipStream_t s, lsq_kmeans_state *st, const uint8_t *cover, int d, int m) {
    const size_t bytes = (size_t)d * m;
    if (st->cover_d == d && st->cover_m == m && st->cover_key.size() == bytes && memcmp(st->cover_key.data(), cover, bytes) == 0) return LSQ_OK;
    const size_t o_dims = 0, o_cnt = o_dims + bytes * 4, o_off = o_cnt + (size_t)m * 4, o_lo = o_off + (size_t)m * 4, o_shape = o_lo + (size_t)m * 4,
                 o_map = o_shape + (size_t)m * 4, total = o_map + bytes;
    st->cover_host.assign(total, 0);
    char *hb = st->cover_host.data();
    int *dims = reinterpret_cast<int *>(hb + o_dims), *cnt = reinterpret_cast<int *>(hb + o_cnt), *off = reinterpret_cast<int *>(hb + o_off),
        *lo = reinterpret_cast<int *>(hb + o_lo), *shape = reinterpret_cast<int *>(hb + o_shape);
    memcpy(hb + o_map, cover, bytes);
    int run = 0;
    for (int j = 0; j < m; ++j) {
        for (int t = 0; t < d; ++t)
            if (cover[(size_t)j * d + t]) dims[(size_t)j * d + cnt[j]++] = t;
        off[j] = run;
        run += (cnt[j] + 3) & ~3;                                  // every centre starts on a float4 boundary of the LDS window
        lo[j] = cnt[j] ? dims[(size_t)j * d] : 0;
        const bool contig = cnt[j] > 0 && dims[(size_t)j * d + cnt[j] - 1] == lo[j] + cnt[j] - 1;
        shape[j] = !contig ? 0 : (lo[j] % 4 == 0 && cnt[j] % 4 == 0 && d % 4 == 0) ? 2 : 1;
    }
    st->cover_key.clear();                                        // not valid until the upload below is enqueued (a pageable source is staged before
                                                                  // hipMemcpyAsync returns, as for the cover lists of lsq_lsqr.hip)
    LSQ_TRY(st->cover.ensure(total));
    char *db = st->cover.as<char>();
    LSQ_HIP(hipMemcpyAsync(db, hb, total, hipMemcpyHostToDevice, s));
    st->C = KCover{reinterpret_cast<const uint8_t *>(db + o_map), reinterpret_cast<const int *>(db + o_dims), reinterpret_cast<const int *>(db + o_cnt),
                   reinterpret_cast<const int *>(db + o_off), reinterpret_cast<const int *>(db + o_lo), reinterpret_cast<const int *>(db + o_shape)};
    st->total = run;
    st->cover_key.assign(cover, cover + bytes);
    st->cover_d = d; st->cover_m = m;
    return LSQ_OK;
}

// dX [n][d], dcodes [n][m] u8 0-based, dKprev [m*256][d] or null (may be dK), dK [m*256][d] (fully written), dcounts [m*256] int32 or null: device pointers.
// cover: HOST bytes [m][d], 0 / 1, every codebook covering something (checked by the caller).  n >= 0.
int lsq_kmeans_update_centers(hipStream_t s, lsq_kmeans_state **pst, const float *dX, const uint8_t *dcodes, const uint8_t *cover, const float *dKprev, int d,
                              int64_t n, int m, float *dK, int *dcounts) {
    if (!*pst) *pst = new lsq_kmeans_state();
    lsq_kmeans_state *st = *pst;
    const int cols = m * LSQ_H;
    LSQ_TRY(kmeans_cover(s, st, cover, d, m));
    const uint64_t *sorted = nullptr;
    const int64_t *seg = nullptr;
    if (n > 0) LSQ_TRY(lsq_sort_rows_by_code(s, st->keys, dcodes, n, m, &sorted, &seg));
    else {                                                        // no rows: every segment is empty
        LSQ_TRY(st->keys.ensure(((size_t)cols + 1) * 8));
        LSQ_HIP(hipMemsetAsync(st->keys.p, 0, ((size_t)cols + 1) * 8, s));
        seg = st->keys.as<int64_t>();
    }
    hipLaunchKernelGGL(kmeans_centers_walk, dim3((unsigned)cols, (unsigned)((d + 63) / 64)), dim3(64), 0, s, dX, sorted, seg, st->C.map, dKprev, d, dK, dcounts);
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

// dX [n][d], dK [m*256][d] (fully written), didx [m][256] int64 or null, dd2 [n][m] f32 or null: device pointers.  cover as above; u: HOST, [m][256] doubles
// in [0, 1) (checked by the caller).  n >= 1.
int lsq_kmeans_seed(hipStream_t s, lsq_kmeans_state **pst, const float *dX, const uint8_t *cover, const double *u, int d, int64_t n, int m, float *dK,
                    int64_t *didx, float *dd2) {
    if (!*pst) *pst = new lsq_kmeans_state();
    lsq_kmeans_state *st = *pst;
    LSQ_TRY(kmeans_cover(s, st, cover, d, m));
    const int64_t rpb = TILE * ((n + (int64_t)TILE * MAXBLK - 1) / ((int64_t)TILE * MAXBLK));
    const int nblocks = (int)((n + rpb - 1) / rpb);
    const size_t o_part = 0, o_cur = o_part + (size_t)m * nblocks * 8, o_d2 = (o_cur + (size_t)m * 8 + 255) & ~(size_t)255,
                 wtotal = o_d2 + (dd2 ? 0 : (size_t)n * m * 4);
    LSQ_TRY(st->work.ensure(wtotal));
    char *base = st->work.as<char>();
    double *part = reinterpret_cast<double *>(base + o_part);
    int64_t *cur = reinterpret_cast<int64_t *>(base + o_cur);
    float *d2 = dd2 ? dd2 : reinterpret_cast<float *>(base + o_d2);
    const bool lds = st->total <= CEN_MAX;
    const size_t shm = LSQ_MAX_M * 8 + (size_t)TILE * LSQ_MAX_M * 4 + (size_t)TILE * LDT * 4 + (lds ? (size_t)st->total * 4 : 0);
    const auto dist = lds ? kpp_dist<true> : kpp_dist<false>;
    const int vec_ok = (reinterpret_cast<uintptr_t>(dX) & 15) == 0;
    for (int k = 0; k < LSQ_H; ++k) {
        if (k > 0) hipLaunchKernelGGL(dist, dim3((unsigned)nblocks), dim3(256), shm, s, dX, n, d, m, rpb, nblocks, st->C, cur, d2, part, k == 1 ? 1 : 0, vec_ok);
        KppU U;
        for (int j = 0; j < LSQ_MAX_M; ++j) U.u[j] = j < m ? u[(size_t)j * LSQ_H + k] : 0.0;
        hipLaunchKernelGGL(kpp_locate, dim3((unsigned)m), dim3(256), 0, s, dX, n, d, rpb, nblocks, st->C.map, U, k, d2, m, part, cur, didx, dK);
    }
    if (dd2) hipLaunchKernelGGL(dist, dim3((unsigned)nblocks), dim3(256), shm, s, dX, n, d, m, rpb, nblocks, st->C, cur, d2, part, 0, vec_ok);      // the last centre too
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

int lsq_kmeans_fill_i64(hipStream_t s, int64_t *p, int64_t count, int64_t v) {
    if (count > 0) hipLaunchKernelGGL(kmeans_fill_i64, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, p, count, v);
    return LSQ_OK;
}
