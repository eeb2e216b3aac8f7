// lsq_compact_check.h -- the parts of lsq_index_remove / lsq_index_compact that need no device: the argument rules, the capacity an index keeps and the byte
// counts of the gathered streams.  Plain C++ over the public header alone, so that a stand-alone host program can exercise them
// (tools/compact_check_main.cpp).
#pragma once

#include <stdint.h>

#include "../../include/lsq_mi355x.h"

// null: the arguments are acceptable as far as the host can tell (the ids' range is the device's to check); else what is wrong (a string literal)
inline const char *lsq_compact_remove_refusal(const int32_t *ids, int64_t count, int id_base) {
    if (count < 0) return "count < 0";
    if (count > (int64_t)INT32_MAX) return "count exceeds 2^31 - 1";
    if (id_base != 0 && id_base != 1) return "id_base must be 0 or 1";
    if (count > 0 && !ids) return "null ids with count > 0";
    return nullptr;
}

// desc may be null: no map wanted, no flags
inline const char *lsq_compact_refusal(const lsq_index_compact_desc *desc) {
    if (!desc) return nullptr;
    if (desc->flags & ~LSQ_COMPACT_SHRINK) return "unknown flags";
    if (desc->id_base != 0 && desc->id_base != 1) return "id_base must be 0 or 1";
    return nullptr;
}

// the rows that stay: an index holds at least one (active: a filter is in force; without one every row stays)
inline const char *lsq_compact_allowed_refusal(int active, int64_t allowed) {
    if (active && allowed < 1) return "no allowed row: an index holds at least one row";
    return nullptr;
}

// rows the owned storage holds after the call: kept, unless LSQ_COMPACT_SHRINK sizes it to the survivors
inline int64_t lsq_compact_capacity(int64_t cap_rows, int64_t n_after, int flags) {
    return (flags & LSQ_COMPACT_SHRINK) || cap_rows < n_after ? n_after : cap_rows;
}

// destination bytes of one gathered stream: `rows` rows `rowb` bytes apart, the last one `lastb` <= rowb bytes long (base rows: the pitch is kept, the
// last row ends at its d-th element).  rows <= 2^31 - 2 and rowb <= 2^33: no overflow in 64 bits
inline int64_t lsq_compact_stream_bytes(int64_t rows, int64_t rowb, int64_t lastb) {
    return rows < 1 ? 0 : (rows - 1) * rowb + lastb;
}

// 0-based new row of old row i under the bitmap / prefix pair (what the device's rank computes): -1 when the bit is clear
inline int64_t lsq_compact_rank(const uint32_t *bits, const int32_t *pre, int64_t i) {
    const uint32_t w = bits[i >> 5], b = (uint32_t)(i & 31);
    if (!((w >> b) & 1u)) return -1;
    return (int64_t)pre[i >> 5] + __builtin_popcount(w & ((1u << b) - 1u));
}
