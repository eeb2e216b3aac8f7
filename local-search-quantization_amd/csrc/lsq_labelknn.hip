// lsq_labelknn.hip -- labelled exact k-NN on the resident index: the ground truth of a labelled search (gfx950).
//
// CONTRACT (Identity LK).  Query q carries (mask, want); row r is a candidate iff (label[r] & mask) == want -- or, with LSQ_LABEL_ANY, iff (label[r] & mask) != 0
// -- AND the index's filter in force allows r.  The result row of q is, bit for bit, what lsq_index_knn returns for that single query after
// lsq_index_set_filter(that candidate set): lsq_knn.hip's distance
//
//   dist(q, i) = ((0 + e_0 e_0) + e_1 e_1) + ... + e_{d-1} e_{d-1},   e_s = x_i[s] - q[s]     f32, s ascending, every op rounded (no FMA)
//
// ranked by (dist, id) with NaN last, the other rows removed, cut to nn, (+inf, id_base - 1) behind it.
//
// lsq_knn.hip's kernels write records for lsq_adc.hip's selection: ONE threshold per query, estimated from a sample of the rows.  With a candidate set per query
// there is nothing to estimate from (the argument of lsq_label.hip).  This kernel selects inside its walk, into the pools of lsq_pool.h, and answers every query
// in one pass.  The matrix cores do not fit: (x - q)^2 has no matrix shape, and the expanded form would need DESIGN 4.29's window and recheck per predicate.
//
//   GEOMETRY  256 threads, a lane owns a ROW, the block owns QB QUERIES and one of `splits` row ranges (a multiple of 256 rows each: lsq_label_split).
//             QB = 4096 / P, P = 2 pow2ceil(max(nn, 256)): 8 / 4 / 2 / 1 at nn <= 256 / 512 / 1024 / 2048.  QB pools of 8 P bytes = 32 KiB, the staged tile
//             ~17 KiB: ~49 KiB a block, three blocks per CU.
//   STAGING   KD = 16 dimensions at a time.  The 256 rows of a step go to xs[KD][256 + 4], transposed: element j of thread t is (row (t >> 4) + 16 j, dimension
//             t & 15), so 16 consecutive threads read one row's 64-byte chunk (knn_scan_kernel's rule); the QB queries go to qs[KD][QB].  Rows and queries are
//             widened (exactly) where the staged registers are stored to LDS.  The next chunk's global loads are in flight in registers while the current
//             chunk is walked.  Columns past d are staged as zeros (0 - 0 = +0 leaves every partial sum unchanged: any d runs the same unrolled loop); a
//             position past the range's end is never loaded.
//   WALK      per staged dimension a lane reads its own row's component (one conflict-free ds_read_b32) and the QB queries (QB / 4 broadcast ds_read_b128), and
//             issues QB / 2 each of v_pk_add_f32 (the subtract), v_pk_mul_f32 and v_pk_add_f32 into QB accumulators: 1.5 VALU instructions per (row, query)
//             and dimension, knn_scan_kernel's ratio.
//   PREDICATE the lane's label and filter bit are read once per step, before the walk, and tested per (row, query).  A wave none of whose 64 x QB pairs is a
//             candidate skips the walk and the selection of the step (wave-uniform, by __ballot); it still stages and still meets the barriers.
//   SELECTION after a step's last chunk the lane forms lsq_adc_key(dist) << idbits | row + 1 per query and takes a slot of that query's pool where the pair is
//             a candidate and the record is below the pool's bound (pool_place).  ONE barrier serves the QB pools, then pool_settle per pool (block-uniform).
//   FINISH    gridDim.y == 1: the pool is sorted and handed out here, ids in id_base.  gridDim.y > 1: every block writes its <= nn sorted records per query as
//             a run, ivf_merge_kernel (lsq_ivfsel.hip) streams a query's runs through pool_offer and hands out 1-BASED ids with 0 as the padding id, and
//             label_knn_shift_kernel moves them to id_base where that is not 1.
// Atomics: integer adds in LDS, and one non-returning integer add per block and statistic (sums of integers: the same on every call).  No inline assembly.
#include <algorithm>

#include "lsq_internal.h"
#include "lsq_pool.h"
#include "lsq_xload.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int LK_KD = 16;                            // dimensions staged per pass
constexpr int LK_XP = SEL_THREADS + 4;               // padded pitch of the transposed rows (floats): the staging stores of a wave hit distinct banks
constexpr int LK_RL = SEL_THREADS * LK_KD / SEL_THREADS;      // staged row elements per thread (16)
constexpr int LK_POOL_RECORDS = 4096;                // QB P: the records of a block's pools (32 KiB)
constexpr int LK_STATS = 4;

constexpr int lk_qp(int qb) { return qb < 2 ? 2 : qb; }       // floats of a staged dimension of the queries: whole pairs

struct LabelKnn {
    const void *X; int64_t ldb;                      // the rows, ldb elements apart
    const void *Q; int64_t ldq;                      // the queries of the CALL, ldq elements apart
    const uint32_t *labels;                          // [n]
    const uint32_t *bits;                            // FILT: the filter's bits by row
    const uint32_t *qmask; const uint32_t *qwant;    // [.] by query of the call
    int q0, nqb;                                     // the query of a slot is q0 + slot
    int64_t n, per;                                  // rows; rows of a range
    int d, nn, P, idbits, any, id_sub;               // ids leave as (the record's id field 1 .. n) - id_sub
    float *dists; int *out_ids;                      // [.][nn]: the caller's rows
    uint64_t *part; unsigned *pcount;                // gridDim.y > 1: the runs [slot][y][nn] and their lengths [slot][y]
    unsigned long long *stat;                        // [0] += records that entered pools, [1] += compactions, [2] += pairs that passed both tests, [3] += skipped wave steps
};

template <typename TX, typename TQ, bool FILT, int QB>
__global__ __launch_bounds__(SEL_THREADS) void label_knn_kernel(const LabelKnn a) {
    constexpr int QP = lk_qp(QB), NP = QP / 2;
    extern __shared__ __align__(16) unsigned char lk_lds[];          // the QB pools
    __shared__ __align__(16) float xs[LK_KD * LK_XP];
    __shared__ __align__(16) float qs[LK_KD * QP];
    __shared__ unsigned tick[3 * QB];                                // pool i's three step counters at [3 i ..]
    __shared__ unsigned long long bstat[3];                          // the block's records placed, pairs passed and wave steps skipped
    const int t = threadIdx.x, lane = t & 63;
    const int slot0 = (int)blockIdx.x * QB;
    const int nqg = a.nqb - slot0 < QB ? a.nqb - slot0 : QB;         // queries of this group (block-uniform, >= 1)
    const int64_t first = (int64_t)blockIdx.y * a.per;
    const int64_t last = first + a.per < a.n ? first + a.per : a.n;
    const int d = a.d;
    const TX *__restrict__ X = static_cast<const TX *>(a.X);
    Pool p[QB];
    uint32_t qm[QB], qw[QB];
#pragma unroll
    for (int i = 0; i < QB; ++i) {
        p[i].rec = reinterpret_cast<uint64_t *>(lk_lds) + (size_t)i * a.P; p[i].tick = tick + 3 * i;
        p[i].bound = ~0ull; p[i].fill = 0; p[i].P = a.P; p[i].nn = a.nn; p[i].step = 0u; p[i].compactions = 0u;
        qm[i] = qw[i] = 0u;
        if (i < nqg) { qm[i] = a.qmask[a.q0 + slot0 + i]; qw[i] = a.qwant[a.q0 + slot0 + i]; }
    }
    for (int e = t; e < LK_KD * QP; e += SEL_THREADS) qs[e] = 0.0f;  // (QB = 1: the second half of the one pair stays zero)
    if (t < 3 * QB) tick[t] = 0u;
    if (t < 3) bstat[t] = 0ull;
    // staging roles: element j of this thread is (row (t >> 4) + 16 j, dimension t & 15); threads with t >> 4 < QB stage query t >> 4 as well
    const int kk = t & (LK_KD - 1), sr = t >> 4;
    const TQ *__restrict__ qrow = sr < nqg ? static_cast<const TQ *>(a.Q) + (int64_t)(a.q0 + slot0 + sr) * a.ldq : nullptr;
    TX xreg[LK_RL];
    TQ qreg = (TQ)0;
    auto fetch = [&](int64_t r0, int k0) {                           // global -> registers: chunk k0 of rows r0 .. r0 + 255 and of the queries
        const int k = k0 + kk;
        const TX *__restrict__ src = X + (r0 + sr) * a.ldb + k;
#pragma unroll
        for (int j = 0; j < LK_RL; ++j) xreg[j] = (r0 + sr + 16 * j < last && k < d) ? src[(int64_t)(16 * j) * a.ldb] : (TX)0;
        if (sr < QB) qreg = (qrow && k < d) ? qrow[k] : (TQ)0;
    };
    const int nk = (d + LK_KD - 1) / LK_KD;
    unsigned long long placed = 0, pairs = 0, skipped = 0;          // (wave-uniform)
    fetch(first, 0);
    for (int64_t r0 = first; r0 < last; r0 += SEL_THREADS) {         // (block-uniform trip count)
        const int64_t row = r0 + t;
        const bool live = row < last;
        const uint32_t lab = live ? a.labels[row] : 0u;
        bool ok = live;
        if constexpr (FILT) ok = live && ((a.bits[row >> 5] >> (row & 31)) & 1u) != 0;
        unsigned pm = 0u;                                            // bit i: this row is a candidate of the group's query i
#pragma unroll
        for (int i = 0; i < QB; ++i) {
            const uint32_t v = lab & qm[i];
            if (i < nqg && ok && (a.any ? v != 0u : v == qw[i])) pm |= 1u << i;
        }
        const bool walk = __ballot(pm != 0u) != 0ull;                // (wave-uniform) a wave without a candidate computes nothing
        f32x2 acc[NP];
#pragma unroll
        for (int c = 0; c < NP; ++c) acc[c] = (f32x2){0.0f, 0.0f};
        for (int kc = 0; kc < nk; ++kc) {
            __syncthreads();                                         // the previous chunk has been walked
#pragma unroll
            for (int j = 0; j < LK_RL; ++j) xs[kk * LK_XP + sr + 16 * j] = (float)xreg[j];
            if (sr < QB) qs[kk * QP + sr] = (float)qreg;
            __syncthreads();
            if (kc + 1 < nk) fetch(r0, (kc + 1) * LK_KD);
            else if (r0 + SEL_THREADS < last) fetch(r0 + SEL_THREADS, 0);
            if (walk) {
#pragma unroll
                for (int s = 0; s < LK_KD; ++s) {
                    const float x = xs[s * LK_XP + t];
                    f32x2 qv[NP];
                    if constexpr (QP >= 4) {
#pragma unroll
                        for (int c = 0; c < QP / 4; ++c) {
                            const f32x4 q4 = *reinterpret_cast<const f32x4 *>(qs + s * QP + 4 * c);
                            qv[2 * c] = q4.xy; qv[2 * c + 1] = q4.zw;
                        }
                    } else {
                        qv[0] = *reinterpret_cast<const f32x2 *>(qs + s * QP);
                    }
#pragma unroll
                    for (int c = 0; c < NP; ++c) {
                        const f32x2 e = (f32x2){x, x} - qv[c];      // x - q, rounded; the square, rounded; then the add (no FMA)
                        acc[c] = acc[c] + e * e;
                    }
                }
            }
        }
        if (walk) {
#pragma unroll
            for (int i = 0; i < QB; ++i) {
                if (i >= nqg) continue;                              // (block-uniform)
                const float dist = (i & 1) ? acc[i >> 1].y : acc[i >> 1].x;
                const uint64_t rec = ((uint64_t)lsq_adc_key(dist) << a.idbits) | (uint64_t)(row + 1);
                const bool pass = ((pm >> i) & 1u) != 0u;
                const bool hit = pass && rec < p[i].bound;
                pairs += (unsigned long long)__popcll(__ballot(pass));
                placed += (unsigned long long)__popcll(__ballot(hit));
                pool_place(p[i], rec, hit);
            }
        } else {
            skipped += 1ull;
        }
        __syncthreads();                                             // the step's one barrier
#pragma unroll
        for (int i = 0; i < QB; ++i)
            if (i < nqg) pool_settle(p[i]);
    }
    if (lane == 0) {                                                 // (read behind the barriers below)
        if (placed) atomicAdd(&bstat[0], placed);
        if (pairs) atomicAdd(&bstat[1], pairs);
        if (skipped) atomicAdd(&bstat[2], skipped);
    }
    unsigned compactions = 0;
    const uint64_t idmask = (1ull << a.idbits) - 1ull;
#pragma unroll
    for (int i = 0; i < QB; ++i) {
        if (i >= nqg) continue;
        const int slot = slot0 + i;
        pool_sort(p[i]);
        const int have = p[i].fill < p[i].nn ? p[i].fill : p[i].nn;
        if (gridDim.y == 1) {                                        // the hand-out, ids in id_base: (+inf, id_base - 1) past the records
            const int64_t o = (int64_t)(a.q0 + slot) * a.nn;
            for (int r = t; r < a.nn; r += SEL_THREADS) {
                const uint64_t rec = r < have ? p[i].rec[r] : 0ull;
                a.dists[o + r] = r < have ? lsq_adc_unkey((uint32_t)(rec >> a.idbits)) : __builtin_inff();
                a.out_ids[o + r] = (int)(uint32_t)(rec & idmask) - a.id_sub;
            }
        } else {
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
        if (bstat[2]) atomicAdd(&a.stat[3], bstat[2]);
    }
}

// the merge hands out the record's 1-based id field: ids [count] -= sub moves them (and the padding id 0) to id_base
__global__ void label_knn_shift_kernel(int *__restrict__ ids, int64_t count, int sub) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) ids[i] -= sub;
}

// the statistics' words are cleared by a kernel (a memset node has no place in a captured stream)
__global__ void label_knn_clear_kernel(unsigned long long *stat) {
    if (threadIdx.x < LK_STATS) stat[threadIdx.x] = 0ull;
}

// what a block allocates: the kernel's static arrays and the QB pools
size_t lk_lds_bytes(int qb, int P) {
    return sizeof(float) * LK_KD * (LK_XP + lk_qp(qb)) + sizeof(unsigned) * 3 * qb + 3 * sizeof(unsigned long long) + sizeof(uint64_t) * (size_t)qb * P;
}

template <typename TX, typename TQ, bool FILT>
int launch_qb(hipStream_t s, const LabelKnn &a, int qb, dim3 grid) {
    const size_t pools = sizeof(uint64_t) * (size_t)qb * a.P;
#define LK_GO(QBV)                                                                                                                      \
    do {                                                                                                                                \
        LSQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&label_knn_kernel<TX, TQ, FILT, QBV>),                               \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)pools));                                           \
        hipLaunchKernelGGL((label_knn_kernel<TX, TQ, FILT, QBV>), grid, dim3(SEL_THREADS), pools, s, a);                                \
    } while (0)
    if (qb == 8) LK_GO(8);
    else if (qb == 4) LK_GO(4);
    else if (qb == 2) LK_GO(2);
    else LK_GO(1);
#undef LK_GO
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}

template <typename TX>
int launch_rows(hipStream_t s, const LabelKnn &a, int q_u8, int qb, dim3 grid) {
    if (a.bits) return q_u8 ? launch_qb<TX, uint8_t, true>(s, a, qb, grid) : launch_qb<TX, float, true>(s, a, qb, grid);
    return q_u8 ? launch_qb<TX, uint8_t, false>(s, a, qb, grid) : launch_qb<TX, float, false>(s, a, qb, grid);
}

int lk_qb(int nn) { return LK_POOL_RECORDS / lsq_ivfsel_pool_records(nn); }

}  // namespace

// ---- the geometry, as a host function: the rule the launch below runs on --------------------------------------------------------------------------------------
extern "C" int lsq_label_knn_geometry(int64_t n, int d, int nn, int nq, int flags, lsq_label_geometry_info *out) {
    if (!out || n < 1 || d < 1 || nn < 1 || nn > LSQ_IVF_SELECT_MAX_NN || nq < 1 || (flags & ~(LSQ_LABEL_ANY | LSQ_LABEL_TEST_ONE_SPLIT))) {
        lsq_set_error("lsq_label_knn_geometry: needs n >= 1, d >= 1, 1 <= nn <= %d, nq >= 1, known flags and an output (got n=%lld d=%d nn=%d nq=%d flags=%d)",
                      LSQ_IVF_SELECT_MAX_NN, (long long)n, d, nn, nq, flags);
        return LSQ_EINVAL;
    }
    const int qb = lk_qb(nn), P = lsq_ivfsel_pool_records(nn);
    int splits = 0;
    int64_t per = 0;
    lsq_label_split(n, (nq + qb - 1) / qb, (flags & LSQ_LABEL_TEST_ONE_SPLIT) != 0, &splits, &per);
    out->queries_per_block = qb; out->pool_records = P; out->lds_bytes = (int64_t)lk_lds_bytes(qb, P);
    out->query_groups = (nq + qb - 1) / qb; out->blocks_per_query = splits; out->rows_per_block = per;
    return LSQ_OK;
}

// ---- the scratch of the index's labelled k-NN calls, and one call -----------------------------------------------------------------------------------------------
struct lsq_labelknn_state {
    DevBuf qmask, qwant, part, pcount, stat;
    PhaseClock<3> clock;                             // one batch: scan, merge
};

void lsq_labelknn_free(lsq_labelknn_state *st) {
    if (!st) return;
    DevBuf *all[] = {&st->qmask, &st->qwant, &st->part, &st->pcount, &st->stat};
    for (DevBuf *b : all) b->release();
    st->clock.release();
    delete st;
}

int lsq_labelknn_search(hipStream_t s, lsq_labelknn_state **pst, const lsq_labelknn_call &c, lsq_label_knn_info *info) {
    if (!*pst) *pst = new lsq_labelknn_state();
    lsq_labelknn_state *st = *pst;
    const int nq = c.nq, nn = c.nn;
    *info = lsq_label_knn_info{};
    info->queries = nq; info->rows = c.n;
    if (nq == 0) return LSQ_OK;
    LSQ_TRY(st->qmask.ensure(sizeof(uint32_t) * (size_t)nq));
    LSQ_TRY(st->qwant.ensure(sizeof(uint32_t) * (size_t)nq));
    LSQ_HIP(hipMemcpyAsync(st->qmask.p, c.q_mask, sizeof(uint32_t) * (size_t)nq, hipMemcpyDefault, s));
    LSQ_HIP(hipMemcpyAsync(st->qwant.p, c.q_want, sizeof(uint32_t) * (size_t)nq, hipMemcpyDefault, s));
    LSQ_TRY(st->stat.ensure(LK_STATS * sizeof(unsigned long long)));
    hipLaunchKernelGGL(label_knn_clear_kernel, dim3(1), dim3(64), 0, s, st->stat.as<unsigned long long>());
    LSQ_HIP(hipGetLastError());
    const int qb = lk_qb(nn);
    LabelKnn a{};
    a.X = c.base; a.ldb = c.ldb; a.Q = c.Q; a.ldq = c.ldq; a.labels = c.labels; a.bits = c.bits;
    a.qmask = st->qmask.as<uint32_t>(); a.qwant = st->qwant.as<uint32_t>();
    a.n = c.n; a.d = c.d; a.nn = nn; a.P = lsq_ivfsel_pool_records(nn); a.idbits = lsq_adc_idbits(c.n);
    a.any = (c.flags & LSQ_LABEL_ANY) ? 1 : 0; a.id_sub = 1 - c.id_base;
    a.dists = c.dists; a.out_ids = c.ids; a.stat = st->stat.as<unsigned long long>();
    info->queries_per_block = qb; info->pool_records = a.P; info->lds_bytes = (int64_t)lk_lds_bytes(qb, a.P);
    lsq_ivfsel_call mg{};                                            // what ivf_merge_kernel reads
    mg.nn = nn; mg.idbits = a.idbits; mg.dists = a.dists; mg.out_ids = a.out_ids; mg.stat = a.stat;
    const int64_t batch = lsq_adc_batch_queries(nn);                 // a query's scratch is its runs: at most 2048 QB + batch of them, of nn records, in a batch
    for (int q0 = 0; q0 < nq; q0 += (int)batch) {
        const int nqb = (int)std::min<int64_t>(batch, nq - q0), groups = (nqb + qb - 1) / qb;
        int splits = 1;
        int64_t per = 0;
        lsq_label_split(c.n, groups, (c.flags & LSQ_LABEL_TEST_ONE_SPLIT) != 0, &splits, &per);
        if (splits > 1) {
            LSQ_TRY(st->part.ensure(sizeof(uint64_t) * (size_t)nqb * splits * nn));
            LSQ_TRY(st->pcount.ensure(sizeof(unsigned) * (size_t)nqb * splits));
        }
        a.part = mg.part = st->part.as<uint64_t>(); a.pcount = mg.pcount = st->pcount.as<unsigned>();
        a.q0 = q0; a.nqb = nqb; a.per = per;
        LSQ_TRY(st->clock.begin(c.timed != 0));
        LSQ_TRY(st->clock.mark(s));
        const dim3 grid((unsigned)groups, (unsigned)splits);
        if (c.base_fmt == LSQ_BASE_F16) LSQ_TRY(launch_rows<lsq_f16>(s, a, c.q_u8, qb, grid));
        else if (c.base_fmt == LSQ_BASE_BF16) LSQ_TRY(launch_rows<lsq_bf16>(s, a, c.q_u8, qb, grid));
        else if (c.base_fmt) LSQ_TRY(launch_rows<uint8_t>(s, a, c.q_u8, qb, grid));
        else LSQ_TRY(launch_rows<float>(s, a, c.q_u8, qb, grid));
        LSQ_TRY(st->clock.mark(s));
        if (splits > 1) {
            LSQ_TRY(lsq_ivfsel_launch_merge(s, mg, q0, nqb, splits));
            if (a.id_sub) {
                const int64_t count = (int64_t)nqb * nn;
                hipLaunchKernelGGL(label_knn_shift_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, c.ids + (int64_t)q0 * nn, count, a.id_sub);
                LSQ_HIP(hipGetLastError());
            }
        }
        LSQ_TRY(st->clock.mark(s));
        LSQ_HIP(hipStreamSynchronize(s));                            // the next batch writes the same runs
        info->batches += 1;
        info->blocks_per_query = std::max<int64_t>(info->blocks_per_query, splits);
        if (splits > 1) info->merged_runs += (int64_t)nqb * splits;
        if (c.timed) {
            float ms[2];
            LSQ_TRY(st->clock.read(ms));
            info->scan_ms += ms[0]; info->merge_ms += ms[1];
        }
    }
    unsigned long long stat[LK_STATS] = {0, 0, 0, 0};
    LSQ_HIP(hipMemcpyAsync(stat, st->stat.p, sizeof(stat), hipMemcpyDeviceToHost, s));
    LSQ_HIP(hipStreamSynchronize(s));
    info->offered = (int64_t)stat[0]; info->compactions = (int64_t)stat[1]; info->allowed_pairs = (int64_t)stat[2]; info->skipped_wave_steps = (int64_t)stat[3];
    return LSQ_OK;
}
