// lsq_grow_check.h -- the parts of lsq_index_add / lsq_index_reserve that need no device: the argument rules, the 2^31 bound and the capacity arithmetic.
// Plain C++ over the public header alone, so that a stand-alone host program can exercise them (tools/grow_check_main.cpp).
#pragma once

#include <stdint.h>

#include "../../include/lsq_mi355x.h"

// what an index is, as far as the rules go
struct lsq_grow_shape {
    int64_t n;
    int d;
    int has_codes, has_base, packed, base_u8, has_lists;      // base_u8: the format of the base rows (0 f32, 1 uint8, LSQ_BASE_F16, LSQ_BASE_BF16)
};

constexpr int64_t LSQ_GROW_MAX_ROWS = (int64_t)INT32_MAX - 1;        // 2^31 - 2: lsq_index_create's bound on n

// the capacity rule (growth factor 3/2): rows the storage is re-allocated to when `need` rows do not fit `cap`; never beyond the bound on n unless need is
inline int64_t lsq_grow_capacity(int64_t cap, int64_t need) {
    int64_t geo = cap + cap / 2;                                     // cap <= 2^31 - 2: no overflow in 64 bits
    if (geo > LSQ_GROW_MAX_ROWS) geo = LSQ_GROW_MAX_ROWS;
    return need > geo ? need : geo;
}

// null: the description is acceptable as far as the host can tell; else what is wrong with it (a string literal)
inline const char *lsq_grow_add_refusal(const lsq_grow_shape &ix, const lsq_index_add_desc *desc) {
    if (!desc) return "null description";
    if (desc->count < 0) return "count < 0";
    if (desc->count > LSQ_GROW_MAX_ROWS - ix.n) return "n + count exceeds 2^31 - 2";      // (n <= the bound: no overflow)
    if (desc->dbnorms && (ix.packed || !ix.has_codes)) return "dbnorms given to an index that keeps none (packed, or without codes)";
    if (desc->norm_codes && !ix.packed) return "norm_codes given to an index that is not packed";
    if (desc->list_of_row && !ix.has_lists) return "list_of_row given, but the index has no lists";
    if (desc->codes && !ix.has_codes) return "codes given to an index that holds none";
    if (desc->base && !ix.has_base) return "base rows given to an index that holds none";
    if (desc->count == 0) return nullptr;                            // a no-op: nothing is required of it
    if (ix.has_codes && !desc->codes) return "the index holds codes: codes are required";
    if (ix.has_codes && !ix.packed && !desc->dbnorms) return "the index holds codes: dbnorms are required";
    if (ix.packed && !desc->norm_codes) return "the index is packed: norm_codes are required";
    if (ix.has_lists && !desc->list_of_row) return "the index has lists: list_of_row is required";
    if (ix.has_base) {
        if (!desc->base) return "the index holds base rows: base is required";
        if (desc->ldb < ix.d) return "ldb < d";
        if (!ix.base_u8 && ((uintptr_t)desc->base & 3) != 0) return "the f32 base is not 4-byte aligned";
        if ((ix.base_u8 == LSQ_BASE_F16 || ix.base_u8 == LSQ_BASE_BF16) && ((uintptr_t)desc->base & 1) != 0) return "the half-precision base is not 2-byte aligned";
    }
    return nullptr;
}

inline const char *lsq_grow_reserve_refusal(int64_t n, int64_t rows) {
    if (rows < n) return "rows < n";
    if (rows > LSQ_GROW_MAX_ROWS) return "rows exceeds 2^31 - 2";
    return nullptr;
}
