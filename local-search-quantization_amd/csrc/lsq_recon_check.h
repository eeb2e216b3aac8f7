// lsq_recon_check.h -- the parts of the decode (lsq_reconstruct_cpu, lsq_index_reconstruct, lsq_index_search_rows) that need no device: the argument rules, the
// chunk rule of the host-buffer form, the check of host ids and the host decode itself (lsq_reconstruct_cpu's body).  Plain C++ over the public header alone,
// so that a stand-alone host program can exercise them (tools/recon_check_main.cpp).
#pragma once

#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

#include "../../include/lsq_mi355x.h"

// rows per staging chunk of a host-buffer lsq_index_reconstruct: as many as keep the staged output at or below `budget` bytes (the default: 64 MiB), never fewer than one, never
// more than n; `option` > 0 (option "recon_chunk", a test hook) only makes chunks smaller.  d >= 1
constexpr int64_t LSQ_RECON_STAGE_BYTES = 64ll << 20;
inline int64_t lsq_recon_chunk_rows(int64_t n, int d, int64_t option, int64_t budget = LSQ_RECON_STAGE_BYTES) {
    int64_t rows = budget / ((int64_t)sizeof(float) * (int64_t)d);
    if (rows < 1) rows = 1;
    if (option > 0 && option < rows) rows = option;
    if (rows > n) rows = n;
    return rows < 1 ? 1 : rows;
}
inline int64_t lsq_recon_chunks(int64_t n, int64_t rows) { return n < 1 ? 0 : (n + rows - 1) / rows; }

// the shape rules every form shares.  null: acceptable; else what is wrong (a string literal)
inline const char *lsq_recon_shape_refusal(int d, int64_t n, int m, int h, int64_t ldc, int64_t ldo) {
    if (d < 1) return "d < 1";
    if (n < 0) return "n < 0";
    if (n > (int64_t)INT32_MAX - 1) return "n exceeds 2^31 - 2";
    if (m < 1 || m > 16) return "m must lie in 1..16";
    if (h < 1 || h > 256) return "h must lie in 1..256";
    if (ldc < m) return "ldc < m";
    if (ldo < d) return "ldo < d";
    return nullptr;
}

// lsq_index_reconstruct's / lsq_reconstruct_cpu's selection: ids == null -> rows [start, start + count), else ids [count] in id_base.  n: the rows addressable
inline const char *lsq_recon_select_refusal(const void *ids, int64_t start, int64_t count, int id_base, int64_t n, int flags, bool have_lists) {
    if (count < 0) return "count < 0";
    if (count > (int64_t)INT32_MAX) return "count exceeds 2^31 - 1";
    if (id_base != 0 && id_base != 1) return "id_base must be 0 or 1";
    if (flags & ~(LSQ_RECON_ADD_COARSE | LSQ_RECON_PAD_NAN)) return "unknown flags";
    if ((flags & LSQ_RECON_ADD_COARSE) && !have_lists) return "LSQ_RECON_ADD_COARSE without lists";
    if (!ids && (start < 0 || start > n || count > n - start)) return "the range [start, start + count) leaves the index";
    return nullptr;
}

// ids outside [id_base, id_base + n) among ids [count]; *first (optional): the position of the first one
inline int64_t lsq_recon_count_bad_ids(const int32_t *ids, int64_t count, int id_base, int64_t n, int64_t *first = nullptr) {
    int64_t bad = 0;
    for (int64_t i = 0; i < count; ++i) {
        const int64_t r = (int64_t)ids[i] - id_base;
        if (r < 0 || r >= n) { if (!bad && first) *first = i; ++bad; }
    }
    return bad;
}

// ---- the host decode.  THE CONTRACT: x^[t] = (((+0.0f + K[(0 h + b_0) d + t]) + K[(1 h + b_1) d + t]) + ...) + K[((m - 1) h + b_(m-1)) d + t], f32, every
// add rounded, codebooks ascending, the sum STARTING FROM +0.0 (a component whose m codewords are all -0.0 is +0.0); with the coarse flag one more rounded add
// of centroid[list_of_row[row]][t].  Compiled without contraction or reassociation (no -ffast-math anywhere in this project): each += below is one IEEE add
struct lsq_recon_cpu_args {
    float *out; int64_t ldo;
    const uint8_t *codes; int64_t ldc;
    const float *K;
    const int32_t *ids; int64_t count; int id_base;
    int64_t n; int m, h, d;
    const float *centroids; const int32_t *list_of_row;
    int flags;
};

inline void lsq_recon_cpu_rows(const lsq_recon_cpu_args a, int64_t r0, int64_t r1) {
    const uint32_t nan_bits = 0x7FC00000u;
    for (int64_t r = r0; r < r1; ++r) {
        float *o = a.out + r * a.ldo;
        const int64_t row = a.ids ? (int64_t)a.ids[r] - a.id_base : r;
        if (row < 0 || row >= a.n) {                  // only with LSQ_RECON_PAD_NAN (the caller checked): never dereferenced
            for (int t = 0; t < a.d; ++t) memcpy(o + t, &nan_bits, 4);
            continue;
        }
        const uint8_t *b = a.codes + row * a.ldc;
        for (int t = 0; t < a.d; ++t) o[t] = 0.0f;
        for (int j = 0; j < a.m; ++j) {
            const float *c = a.K + ((int64_t)j * a.h + b[j]) * a.d;
            for (int t = 0; t < a.d; ++t) o[t] += c[t];
        }
        if (a.flags & LSQ_RECON_ADD_COARSE) {
            const float *c = a.centroids + (int64_t)a.list_of_row[row] * a.d;
            for (int t = 0; t < a.d; ++t) o[t] += c[t];
        }
    }
}

// null: done; else what is wrong -- and then nothing was written.  *invalid (optional): the ids padded with NaN rows
inline const char *lsq_recon_cpu(const lsq_recon_cpu_args &a, int nthreads, int64_t *invalid = nullptr) {
    if (invalid) *invalid = 0;
    if (const char *why = lsq_recon_shape_refusal(a.d, a.n, a.m, a.h, a.ldc, a.ldo)) return why;
    if (const char *why = lsq_recon_select_refusal(a.ids, 0, a.count, a.id_base, a.n, a.flags, a.centroids && a.list_of_row)) return why;
    if (a.count == 0) return nullptr;
    if (!a.out || !a.codes || !a.K) return "null pointer";
    const int64_t bad = a.ids ? lsq_recon_count_bad_ids(a.ids, a.count, a.id_base, a.n) : 0;
    if (bad && !(a.flags & LSQ_RECON_PAD_NAN)) return "an id lies outside [id_base, id_base + n)";
    for (int64_t r = 0; r < a.count; ++r) {           // the codes read: below h
        const int64_t row = a.ids ? (int64_t)a.ids[r] - a.id_base : r;
        if (row < 0 || row >= a.n) continue;
        for (int j = 0; j < a.m; ++j)
            if (a.codes[row * a.ldc + j] >= a.h) return "a code lies outside [0, h)";
    }
    int nt = nthreads > 0 ? nthreads : (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if ((int64_t)nt > a.count) nt = (int)a.count;
    if (nt == 1) lsq_recon_cpu_rows(a, 0, a.count);
    else {
        std::vector<std::thread> pool;
        pool.reserve((size_t)nt);
        for (int t = 0; t < nt; ++t) pool.emplace_back(lsq_recon_cpu_rows, a, a.count * t / nt, a.count * (t + 1) / nt);
        for (auto &th : pool) th.join();
    }
    if (invalid) *invalid = bad;
    return nullptr;
}
