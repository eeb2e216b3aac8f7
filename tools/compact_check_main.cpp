// compact_check_main.cpp -- a stand-alone host program over csrc/lsq_compact_check.h: the argument rules of lsq_index_remove / lsq_index_compact, the
// capacity an index keeps, the byte counts of the gathered streams and the rank that renumbers the rows, which need no device.  Built with the host
// compiler alone, usually under -fsanitize=address,undefined (tests/test_index_compact.py does that where the compiler has the runtimes): signed overflow
// in a byte count or a read past the bitmap is then an error, not a wrong number.
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/compact_check_main.cpp -o compact_check && ./compact_check
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../local-search-quantization_amd/csrc/lsq_compact_check.h"

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static bool has(const char *why, const char *word) { return why && strstr(why, word); }

int main() {
    static int32_t ids[4] = {0, 1, 2, 3};
    // ---- lsq_index_remove: every refusal, every legal edge
    EXPECT(lsq_compact_remove_refusal(ids, 4, 0) == nullptr);
    EXPECT(lsq_compact_remove_refusal(ids, 4, 1) == nullptr);
    EXPECT(lsq_compact_remove_refusal(nullptr, 0, 0) == nullptr);            // count == 0: a no-op, nothing is required of it
    EXPECT(lsq_compact_remove_refusal(ids, 0, 1) == nullptr);
    EXPECT(lsq_compact_remove_refusal(ids, (int64_t)INT32_MAX, 0) == nullptr);
    EXPECT(has(lsq_compact_remove_refusal(ids, -1, 0), "count < 0"));
    EXPECT(has(lsq_compact_remove_refusal(ids, INT64_MIN, 0), "count < 0"));
    EXPECT(has(lsq_compact_remove_refusal(ids, (int64_t)INT32_MAX + 1, 0), "2^31"));
    EXPECT(has(lsq_compact_remove_refusal(ids, INT64_MAX, 0), "2^31"));
    EXPECT(has(lsq_compact_remove_refusal(ids, 4, 2), "id_base"));
    EXPECT(has(lsq_compact_remove_refusal(ids, 4, -1), "id_base"));
    EXPECT(has(lsq_compact_remove_refusal(ids, 4, INT32_MIN), "id_base"));
    EXPECT(has(lsq_compact_remove_refusal(nullptr, 1, 0), "null ids"));
    EXPECT(has(lsq_compact_remove_refusal(nullptr, 0, 2), "id_base"));       // a bad id_base is refused even by a no-op
    // ---- lsq_index_compact
    EXPECT(lsq_compact_refusal(nullptr) == nullptr);                         // no map wanted, no flags
    lsq_index_compact_desc d{};
    EXPECT(lsq_compact_refusal(&d) == nullptr);
    d.flags = LSQ_COMPACT_SHRINK; d.id_base = 1; d.on_device = 1;
    EXPECT(lsq_compact_refusal(&d) == nullptr);
    d.flags = 2;
    EXPECT(has(lsq_compact_refusal(&d), "flags"));
    d.flags = LSQ_COMPACT_SHRINK | 4;
    EXPECT(has(lsq_compact_refusal(&d), "flags"));
    d.flags = INT32_MIN;
    EXPECT(has(lsq_compact_refusal(&d), "flags"));
    d.flags = -1;
    EXPECT(has(lsq_compact_refusal(&d), "flags"));
    d.flags = 0; d.id_base = 2;
    EXPECT(has(lsq_compact_refusal(&d), "id_base"));
    d.id_base = -1;
    EXPECT(has(lsq_compact_refusal(&d), "id_base"));
    EXPECT(has(lsq_compact_allowed_refusal(1, 0), "at least one"));
    EXPECT(lsq_compact_allowed_refusal(1, 1) == nullptr);
    EXPECT(lsq_compact_allowed_refusal(0, 0) == nullptr);                    // no filter: every row stays, `allowed` means nothing
    // ---- the capacity: kept, unless SHRINK
    EXPECT(lsq_compact_capacity(1000, 400, 0) == 1000);
    EXPECT(lsq_compact_capacity(1000, 400, LSQ_COMPACT_SHRINK) == 400);
    EXPECT(lsq_compact_capacity(1000, 1000, LSQ_COMPACT_SHRINK) == 1000);
    EXPECT(lsq_compact_capacity(1, 1, 0) == 1);
    EXPECT(lsq_compact_capacity((int64_t)INT32_MAX - 1, 1, 0) == (int64_t)INT32_MAX - 1);
    EXPECT(lsq_compact_capacity(0, 5, 0) == 5);                              // never below the rows held
    // ---- stream bytes: no overflow at the largest index and the longest row
    EXPECT(lsq_compact_stream_bytes(0, 17, 17) == 0);
    EXPECT(lsq_compact_stream_bytes(1, 100, 96) == 96);
    EXPECT(lsq_compact_stream_bytes(2065, 17, 17) == 2065 * 17);
    EXPECT(lsq_compact_stream_bytes(3, 100, 96) == 296);
    EXPECT(lsq_compact_stream_bytes((int64_t)INT32_MAX - 1, (int64_t)1 << 30, 1) == ((int64_t)INT32_MAX - 2) * ((int64_t)1 << 30) + 1);
    // ---- the rank: against a count by hand, at every position of a bitmap whose last word is partial
    const int64_t n = 2065;
    const int64_t nwords = (n + 31) / 32;
    std::vector<uint32_t> bits((size_t)nwords, 0u);
    std::vector<int32_t> pre((size_t)nwords + 1, 0);
    for (int64_t i = 0; i < n; ++i)
        if (i % 3 != 1 && !(i >= 64 && i < 96)) bits[(size_t)(i >> 5)] |= 1u << (i & 31);      // a whole word removed among them
    for (int64_t w = 0; w < nwords; ++w) pre[(size_t)w + 1] = pre[(size_t)w] + __builtin_popcount(bits[(size_t)w]);
    int64_t seen = 0;
    for (int64_t i = 0; i < n; ++i) {
        const bool set = (bits[(size_t)(i >> 5)] >> (i & 31)) & 1u;
        const int64_t r = lsq_compact_rank(bits.data(), pre.data(), i);
        EXPECT(r == (set ? seen : -1));
        seen += set;
    }
    EXPECT(seen == pre[(size_t)nwords]);
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("compact_check: all passed\n");
    return 0;
}
