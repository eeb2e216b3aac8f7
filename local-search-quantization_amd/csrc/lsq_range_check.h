// lsq_range_check.h -- the parts of lsq_index_range_search that need no device: the argument rules, the prefix that turns per-query counts into lims, and
// the rule that cuts the queries into fill batches.  Plain C++ over the public header alone, so that a stand-alone host program can exercise them
// (tools/range_check_main.cpp).
#pragma once

#include <stdint.h>

#include <vector>

#include "../../include/lsq_mi355x.h"

constexpr int64_t LSQ_RANGE_BATCH_RECORDS = (int64_t)1 << 28;      // records of a fill batch when option "range_batch" is 0: two record buffers of 2 GiB

// null: the arguments are acceptable; else what is wrong (a string literal).  has_codes: the index holds codes; nlist: its lists (0: none yet); d: its dimension
inline const char *lsq_range_refusal(const void *lims, const void *q_scan, const void *radius, int has_codes, int nlist, int d, int nq, int64_t ldq, int nprobe,
                                     int flags) {
    if (!lims || !q_scan || !radius) return "null pointer";
    if (!has_codes) return "the index holds no codes";
    if (nq < 0) return "nq < 0";
    if (ldq < d) return "ldq < d";
    if (nprobe < 0) return "nprobe < 0";
    if (flags & ~LSQ_IVF_ADD_COARSE) return "unknown flags";
    if (nprobe == 0 && flags) return "LSQ_IVF_ADD_COARSE needs nprobe >= 1";
    if (nprobe >= 1 && nlist < 1) return "the index has no lists (call lsq_index_set_lists first)";
    if (nprobe > nlist && nprobe >= 1) return "nprobe exceeds nlist";
    return nullptr;
}

// lims[0] = 0, lims[q + 1] = lims[q] + count[q]: the CSR of the result.  Returns the largest count (0 for nq == 0).  A count is at most n <= 2^31 - 2 and
// nq <= 2^31 - 1: the sum stays below 2^62
inline int64_t lsq_range_prefix(const uint32_t *count, int64_t nq, int64_t *lims) {
    int64_t most = 0;
    lims[0] = 0;
    for (int64_t q = 0; q < nq; ++q) {
        const int64_t c = (int64_t)count[q];
        lims[q + 1] = lims[q] + c;
        if (c > most) most = c;
    }
    return most;
}

// The fill batches of queries lo .. hi - 1: cuts[0] = lo < cuts[1] < ... < cuts.back() = hi, batch b = queries cuts[b] .. cuts[b + 1] - 1.  A batch takes
// queries while its records (lims[end] - lims[begin]) stay within `budget`; a query whose own result exceeds the budget is a batch of its own -- nothing is
// truncated, the budget bounds scratch and not the answer.  Greedy from the left, so the cut depends on the counts alone.  budget < 1 counts as 1.
// lo == hi: no batch (cuts = {lo})
inline void lsq_range_cut(const int64_t *lims, int64_t lo, int64_t hi, int64_t budget, std::vector<int64_t> *cuts) {
    if (budget < 1) budget = 1;
    cuts->clear();
    cuts->push_back(lo);
    int64_t begin = lo;
    while (begin < hi) {
        int64_t end = begin + 1;                                     // a batch holds at least one query, whatever its size
        while (end < hi && lims[end + 1] - lims[begin] <= budget) ++end;
        cuts->push_back(end);
        begin = end;
    }
}

// the record budget of a call: option "range_batch", or the default
inline int64_t lsq_range_budget(int64_t range_batch) { return range_batch > 0 ? range_batch : LSQ_RANGE_BATCH_RECORDS; }
