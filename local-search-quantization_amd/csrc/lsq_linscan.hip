// lsq_linscan.hip -- ADC linear scan for codes + separately stored database norms (HOST code).
//
// SURVEY 8(f)-1 / north_star: "linscan asymmetric-distance table sums stay on the host but call into the
// same C-ABI".  Replaces linscan_aqd_query_extra_byte of the reference
// (src/linscan/cpp/linscan_aqd_pairwise_byte.cpp:14-104, bound at src/linscan/Linscan.jl:63-69), written from
// scratch: same arithmetic order (so distances are bit-identical to the reference build in oracle/_ref and the
// ids agree including ties), different machinery -- a bounded max-heap per query instead of materialising
// 10^7 (dist, id) pairs and partial_sort-ing them, std::thread workers instead of OpenMP (no second OpenMP
// runtime next to torch's).
//
//   table[j]   = ((0 - (2 q0) c_j0) - (2 q1) c_j1) - ...           (f32, k ascending; no FMA: -ffp-contract=off)
//   dist(i)    = (((0 + table[0*h + b_i0]) + table[1*h + b_i1]) + ...) + dbnorms[i]
//   result     = the nn smallest (dist, id) pairs in lexicographic order, ids 1-BASED like the reference (:75).
//
// Below it, the reference's other scan (PQ / OPQ codes, no norm term): lsq_linscan_aqd_query; then exact k-NN (lsq_knn_exact_cpu).
#include <algorithm>
#include <cstring>
#include <thread>
#include <utility>
#include <vector>

#include "lsq_internal.h"

namespace {

// A (dist, id) pair as ONE 64-bit key: order-preserving distance bits << 32 | id.  Its integer order is the lexicographic pair order for every non-NaN
// distance (no sum of the scans below is ever -0.0: each chain starts from +0.0) and puts NaN last, as one NaN -- what the device scan does.  A
// std::pair<float, int> has no order with a NaN in it: a heap built on it loses its invariant and hands back NaN among, or before, the finite distances.
inline uint64_t pq_key(float v, uint32_t id) {
    uint32_t b;
    memcpy(&b, &v, 4);
    const uint32_t k = v != v ? 0xffffffffu : b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
    return ((uint64_t)k << 32) | id;
}
inline float pq_unkey(uint64_t key) {
    const uint32_t k = (uint32_t)(key >> 32);
    const uint32_t b = k == 0xffffffffu ? 0x7fc00000u : ((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
    float v;
    memcpy(&v, &b, 4);
    return v;
}

void scan_queries(float *dists, int *idx, const unsigned char *codes, const float *queries, const float *codebooks,
                  const float *dbnorms, int q0, int q1, int ncodes, int m, int h, int d, int nn) {
    const int total = m * h;
    std::vector<float> table((size_t)total);
    std::vector<uint64_t> heap;
    heap.reserve((size_t)nn + 1);
    for (int q = q0; q < q1; ++q) {
        const float *query = queries + (size_t)q * d;
        for (int j = 0; j < total; ++j) {
            const float *c = codebooks + (size_t)j * d;
            float t = 0.0f;
            for (int k = 0; k < d; ++k) t -= 2 * query[k] * c[k];      // (2*q)*c, then one rounded subtract
            table[(size_t)j] = t;
        }
        heap.clear();
        const unsigned char *code = codes;
        bool full = false;
        float worst = 0.0f;                                             // the heap's largest distance once it is full
        for (int i = 0; i < ncodes; ++i, code += m) {
            float acc = 0.0f;
            for (int k = 0; k < m; ++k) acc += table[(size_t)h * k + code[k]];
            acc += dbnorms[i];
            if (full && acc > worst) continue;                          // strictly farther (false with a NaN on either side: the keys decide)
            const uint64_t cand = pq_key(acc, (uint32_t)(i + 1));      // ids are 1-BASED (:75)
            if (!full) {
                heap.push_back(cand);
                std::push_heap(heap.begin(), heap.end());               // max-heap on (dist, id)
            } else if (cand < heap.front()) {
                std::pop_heap(heap.begin(), heap.end());
                heap.back() = cand;
                std::push_heap(heap.begin(), heap.end());
            } else {
                continue;
            }
            full = (int)heap.size() == nn;
            if (full) worst = pq_unkey(heap.front());
        }
        std::sort_heap(heap.begin(), heap.end());                       // ascending (dist, id)
        for (int r = 0; r < nn; ++r) {
            dists[(size_t)q * nn + r] = pq_unkey(heap[(size_t)r]);
            idx[(size_t)q * nn + r] = (int)(uint32_t)heap[(size_t)r];
        }
    }
}

}  // namespace

extern "C" int lsq_linscan_aqd_query_extra_byte(float *dists, int *idx, const unsigned char *codes, const float *queries,
                                                const float *codebooks, const float *dbnorms, int nqueries, int ncodes,
                                                int m, int h, int d, int nn, int nthreads) {
    if (nqueries < 0 || ncodes < 0 || m < 1 || h < 1 || h > 256 || d < 1 || nn < 1) {
        lsq_set_error("lsq_linscan_aqd_query_extra_byte: bad shape nq=%d n=%d m=%d h=%d d=%d nn=%d", nqueries, ncodes, m, h, d, nn);
        return LSQ_EINVAL;
    }
    if (nn > ncodes) { lsq_set_error("lsq_linscan_aqd_query_extra_byte: nn=%d exceeds the database size %d", nn, ncodes); return LSQ_EINVAL; }
    if (nqueries == 0) return LSQ_OK;
    if (!dists || !idx || !codes || !queries || !codebooks || !dbnorms) { lsq_set_error("lsq_linscan_aqd_query_extra_byte: null pointer"); return LSQ_EINVAL; }
    int nt = nthreads > 0 ? nthreads : (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if (nt > nqueries) nt = nqueries;
    std::vector<std::thread> pool;
    pool.reserve((size_t)nt);
    for (int t = 0; t < nt; ++t) {
        const int q0 = (int)((int64_t)nqueries * t / nt), q1 = (int)((int64_t)nqueries * (t + 1) / nt);
        pool.emplace_back(scan_queries, dists, idx, codes, queries, codebooks, dbnorms, q0, q1, ncodes, m, h, d, nn);
    }
    for (auto &th : pool) th.join();
    return LSQ_OK;
}

// ---- PQ / OPQ: linscan_aqd_query of the reference (src/linscan/cpp/linscan_aqd.cpp:37-114, bound by linscan_pq / linscan_opq at
// src/linscan/Linscan.jl:5-43), written from scratch with the same arithmetic order:
//
//   table[k 256 + r] = ((0 + d_0 d_0) + d_1 d_1) + ...,   d_s = c[k][r][s] - q[k subdim + s]     (f32, s ascending; no FMA)
//   dist(i)          = ((0 + table[0 256 + b_i0]) + table[1 256 + b_i1]) + ...                    (k ascending; no norm term)
//   result           = the K smallest (dist, id) pairs in lexicographic order, ids 0-BASED uint32 (:93-101)
//
// The reference's chunks of 10^7 pairs return exactly the K lexicographically smallest pairs (what a pair left over from an earlier chunk
// could displace was already smaller); a bounded heap per query does the same, on the 64-bit keys of pq_key above (NaN last: the reference's
// partial_sort leaves NaN undefined).
namespace {

void pq_scan_queries(float *dists, uint32_t *res, const uint8_t *codes, const float *centers, const float *queries, int64_t q0, int64_t q1,
                     int N, int m, int K, int dim1codes, int dim1queries, int subdim) {
    std::vector<float> table((size_t)m * LSQ_H);
    std::vector<uint64_t> heap;
    heap.reserve((size_t)K + 1);
    for (int64_t q = q0; q < q1; ++q) {
        const float *query = queries + q * dim1queries;
        for (int k = 0; k < m; ++k) {
            const float *qk = query + (size_t)k * subdim;
            for (int r = 0; r < LSQ_H; ++r) {
                const float *c = centers + ((size_t)k * LSQ_H + r) * subdim;
                float t = 0.0f;
                for (int s = 0; s < subdim; ++s) {
                    const float e = c[s] - qk[s];
                    t += e * e;                                          // product rounded, then the add (-ffp-contract=off)
                }
                table[(size_t)k * LSQ_H + r] = t;
            }
        }
        heap.clear();
        const uint8_t *code = codes;
        for (int i = 0; i < N; ++i, code += dim1codes) {
            float acc = 0.0f;
            for (int k = 0; k < m; ++k) acc += table[(size_t)LSQ_H * k + code[k]];
            const uint64_t cand = pq_key(acc, (uint32_t)i);
            if ((int)heap.size() < K) {
                heap.push_back(cand);
                std::push_heap(heap.begin(), heap.end());               // max-heap on (dist, id)
            } else if (cand < heap.front()) {
                std::pop_heap(heap.begin(), heap.end());
                heap.back() = cand;
                std::push_heap(heap.begin(), heap.end());
            }
        }
        std::sort_heap(heap.begin(), heap.end());                       // ascending (dist, id)
        for (int j = 0; j < K; ++j) {
            dists[q * K + j] = pq_unkey(heap[(size_t)j]);
            res[q * K + j] = (uint32_t)heap[(size_t)j];
        }
    }
}

}  // namespace

// Argument checks shared with the device scan (lsq_api.hip): 0 or LSQ_EINVAL with the message set.
int lsq_linscan_pq_check(const char *fn, const void *dists, const void *res, const void *codes, const void *centers, const void *queries, int N,
                         uint32_t NQ, int B, int K, int dim1codes, int dim1queries, int subdim) {
    if (B < 8 || B % 8 != 0) { lsq_set_error("%s: B=%d bits must be a positive multiple of 8 (h = 256)", fn, B); return LSQ_EINVAL; }
    const int m = B / 8;
    if (m > dim1codes) { lsq_set_error("%s: B/8=%d exceeds dim1codes=%d", fn, m, dim1codes); return LSQ_EINVAL; }
    if (subdim < 1) { lsq_set_error("%s: subdim=%d must be >= 1", fn, subdim); return LSQ_EINVAL; }
    if ((int64_t)m * subdim > (int64_t)dim1queries) {
        lsq_set_error("%s: (B/8)*subdim=%lld exceeds dim1queries=%d", fn, (long long)m * subdim, dim1queries);
        return LSQ_EINVAL;
    }
    if (K < 1 || K > N) { lsq_set_error("%s: needs 1 <= K <= N (got K=%d N=%d)", fn, K, N); return LSQ_EINVAL; }
    if (NQ > 0 && (!dists || !res || !codes || !centers || !queries)) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    return LSQ_OK;
}

extern "C" int lsq_linscan_aqd_query(float *dists, uint32_t *res, const uint8_t *codes, const float *centers, const float *queries, int N,
                                     uint32_t NQ, int B, int K, int dim1codes, int dim1queries, int subdim) {
    LSQ_TRY(lsq_linscan_pq_check("lsq_linscan_aqd_query", dists, res, codes, centers, queries, N, NQ, B, K, dim1codes, dim1queries, subdim));
    if (NQ == 0) return LSQ_OK;
    int64_t nt = (int64_t)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if (nt > (int64_t)NQ) nt = (int64_t)NQ;
    std::vector<std::thread> pool;
    pool.reserve((size_t)nt);
    for (int64_t t = 0; t < nt; ++t) {
        const int64_t q0 = (int64_t)NQ * t / nt, q1 = (int64_t)NQ * (t + 1) / nt;
        pool.emplace_back(pq_scan_queries, dists, res, codes, centers, queries, q0, q1, N, B / 8, K, dim1codes, dim1queries, subdim);
    }
    for (auto &th : pool) th.join();
    return LSQ_OK;
}

// ---- exact k-NN (ground truth; the device form is lsq_knn.hip):
//
//   dist(q, i) = ((0 + e_0 e_0) + e_1 e_1) + ...,   e_s = x_i[s] - q[s]      (f32, s ascending; no FMA)
//   result     = the nn smallest (dist, id) pairs in lexicographic order, ids 0-BASED uint32, NaN last
//
// -- the PQ table rule above with one sub-space of width d.  Four queries share a pass over the base (four independent add chains per row).
namespace {

void knn_queries(float *dists, uint32_t *ids, const float *base, const float *queries, int q0, int q1, int n, int d, int ldb, int ldq, int nn) {
    constexpr int QB = 4;
    std::vector<uint64_t> heap[QB];
    for (auto &h : heap) h.reserve((size_t)nn + 1);
    for (int qa = q0; qa < q1; qa += QB) {
        const int nb = q1 - qa < QB ? q1 - qa : QB;
        const float *qp[QB];
        for (int b = 0; b < QB; ++b) qp[b] = queries + (size_t)(qa + (b < nb ? b : 0)) * ldq;
        for (auto &h : heap) h.clear();
        const float *x = base;
        for (int i = 0; i < n; ++i, x += ldb) {
            float acc[QB] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int s = 0; s < d; ++s) {
                const float xs = x[s];
                for (int b = 0; b < QB; ++b) {
                    const float e = xs - qp[b][s];
                    acc[b] += e * e;                                     // product rounded, then the add (-ffp-contract=off)
                }
            }
            for (int b = 0; b < nb; ++b) {
                const uint64_t cand = pq_key(acc[b], (uint32_t)i);
                std::vector<uint64_t> &h = heap[b];
                if ((int)h.size() < nn) {
                    h.push_back(cand);
                    std::push_heap(h.begin(), h.end());                 // max-heap on (dist, id)
                } else if (cand < h.front()) {
                    std::pop_heap(h.begin(), h.end());
                    h.back() = cand;
                    std::push_heap(h.begin(), h.end());
                }
            }
        }
        for (int b = 0; b < nb; ++b) {
            std::sort_heap(heap[b].begin(), heap[b].end());              // ascending (dist, id)
            const size_t q = (size_t)(qa + b);
            for (int j = 0; j < nn; ++j) {
                dists[q * nn + j] = pq_unkey(heap[b][(size_t)j]);
                ids[q * nn + j] = (uint32_t)heap[b][(size_t)j];
            }
        }
    }
}

}  // namespace

// Argument checks shared with the device search (lsq_api.hip): 0 or LSQ_EINVAL with the message set.
int lsq_knn_exact_check(const char *fn, const void *dists, const void *ids, const void *base, const void *queries, int n, int nq, int d, int ldb,
                        int ldq, int nn) {
    if (d < 1 || ldb < d || ldq < d) { lsq_set_error("%s: needs d >= 1, ldb >= d, ldq >= d (got d=%d ldb=%d ldq=%d)", fn, d, ldb, ldq); return LSQ_EINVAL; }
    if (nq < 1) { lsq_set_error("%s: needs nq >= 1 (got %d)", fn, nq); return LSQ_EINVAL; }
    if (nn < 1 || nn > n) { lsq_set_error("%s: needs 1 <= nn <= n (got nn=%d n=%d)", fn, nn, n); return LSQ_EINVAL; }
    if (!dists || !ids || !base || !queries) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    return LSQ_OK;
}

extern "C" int lsq_knn_exact_cpu(float *dists, uint32_t *ids, const float *base, const float *queries, int n, int nq, int d, int ldb, int ldq, int nn,
                                 int nthreads) {
    LSQ_TRY(lsq_knn_exact_check("lsq_knn_exact_cpu", dists, ids, base, queries, n, nq, d, ldb, ldq, nn));
    int nt = nthreads > 0 ? nthreads : (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if (nt > nq) nt = nq;
    std::vector<std::thread> pool;
    pool.reserve((size_t)nt);
    for (int t = 0; t < nt; ++t) {
        const int q0 = (int)((int64_t)nq * t / nt), q1 = (int)((int64_t)nq * (t + 1) / nt);
        pool.emplace_back(knn_queries, dists, ids, base, queries, q0, q1, n, d, ldb, ldq, nn);
    }
    for (auto &th : pool) th.join();
    return LSQ_OK;
}

// ---- the same for rows and queries that are f32 or uint8 at any byte alignment: elements are read one at a time (memcpy for f32), uint8 widened, and
// the f32 chain above runs on them -- the contract for EVERY d; the device's integer road (lsq_knn.hip) is held to these bits, not the other way round.
namespace {

inline float knn_elem(const uint8_t *p, int fmt, int64_t i) {     // fmt: lsq_base_format's (0 f32, 1 uint8, the two halves)
    if (fmt == 1) return (float)p[i];
    if (fmt) {
        uint16_t h;
        memcpy(&h, p + 2 * i, 2);
        return lsq_widen_half(h, fmt);
    }
    float v;
    memcpy(&v, p + 4 * i, 4);
    return v;
}

void knn_queries_any(float *dists, uint32_t *ids, const uint8_t *base, int base_u8, const uint8_t *queries, int q_u8, int q0, int q1, int n, int d,
                     int ldb, int ldq, int nn) {
    std::vector<uint64_t> heap;
    heap.reserve((size_t)nn + 1);
    std::vector<float> q((size_t)d), x((size_t)d);
    for (int qi = q0; qi < q1; ++qi) {
        for (int s = 0; s < d; ++s) q[(size_t)s] = knn_elem(queries, q_u8, (int64_t)qi * ldq + s);
        heap.clear();
        for (int i = 0; i < n; ++i) {
            for (int s = 0; s < d; ++s) x[(size_t)s] = knn_elem(base, base_u8, (int64_t)i * ldb + s);
            float acc = 0.0f;
            for (int s = 0; s < d; ++s) {
                const float e = x[(size_t)s] - q[(size_t)s];
                acc += e * e;                                           // product rounded, then the add (-ffp-contract=off)
            }
            const uint64_t cand = pq_key(acc, (uint32_t)i);
            if ((int)heap.size() < nn) {
                heap.push_back(cand);
                std::push_heap(heap.begin(), heap.end());
            } else if (cand < heap.front()) {
                std::pop_heap(heap.begin(), heap.end());
                heap.back() = cand;
                std::push_heap(heap.begin(), heap.end());
            }
        }
        std::sort_heap(heap.begin(), heap.end());
        for (int j = 0; j < nn; ++j) {
            dists[(size_t)qi * nn + j] = pq_unkey(heap[(size_t)j]);
            ids[(size_t)qi * nn + j] = (uint32_t)heap[(size_t)j];
        }
    }
}

}  // namespace

extern "C" int lsq_knn_exact_u8_cpu(float *dists, uint32_t *ids, const void *base, int base_u8, const void *queries, int queries_u8, int n, int nq, int d,
                                    int ldb, int ldq, int nn, int nthreads) {
    LSQ_TRY(lsq_knn_exact_check("lsq_knn_exact_u8_cpu", dists, ids, base, queries, n, nq, d, ldb, ldq, nn));
    int nt = nthreads > 0 ? nthreads : (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if (nt > nq) nt = nq;
    std::vector<std::thread> pool;
    pool.reserve((size_t)nt);
    for (int t = 0; t < nt; ++t) {
        const int q0 = (int)((int64_t)nq * t / nt), q1 = (int)((int64_t)nq * (t + 1) / nt);
        pool.emplace_back(knn_queries_any, dists, ids, static_cast<const uint8_t *>(base), lsq_base_format(base_u8), static_cast<const uint8_t *>(queries),
                          queries_u8 != 0 ? 1 : 0, q0, q1, n, d, ldb, ldq, nn);
    }
    for (auto &th : pool) th.join();
    return LSQ_OK;
}
