// grow_check_main.cpp -- a stand-alone host program over csrc/lsq_grow_check.h: the argument rules of lsq_index_add / lsq_index_reserve, the 2^31 - 2 bound
// and the capacity arithmetic, which need no device.  Built with the host compiler alone, usually under -fsanitize=address,undefined (tests/test_index_add.py
// does that where the compiler has the runtimes): signed overflow in the bound or in the growth rule is then an error, not a wrong number.
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/grow_check_main.cpp -o grow_check && ./grow_check
#include <stdio.h>
#include <string.h>

#include "../local-search-quantization_amd/csrc/lsq_grow_check.h"

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static bool refused(const lsq_grow_shape &ix, const lsq_index_add_desc &d, const char *word) {
    const char *why = lsq_grow_add_refusal(ix, &d);
    return why && strstr(why, word);
}

int main() {
    static uint8_t codes[64], nc[8];
    static float norms[8], base[8 * 6];
    static int32_t lor[8];
    const lsq_grow_shape plain{1000, 4, 1, 0, 0, 0, 0}, packed{1000, 4, 1, 0, 1, 0, 0}, with_lists{1000, 4, 1, 0, 0, 0, 1}, with_base{1000, 4, 1, 1, 0, 0, 0},
        base_only{1000, 4, 0, 1, 0, 0, 0}, u8_base{1000, 4, 0, 1, 0, 1, 0};
    lsq_index_add_desc ok{};
    ok.count = 8; ok.codes = codes; ok.dbnorms = norms;
    EXPECT(lsq_grow_add_refusal(plain, &ok) == nullptr);
    EXPECT(lsq_grow_add_refusal(plain, nullptr) != nullptr);

    lsq_index_add_desc d = ok;
    d.count = -1;
    EXPECT(refused(plain, d, "count < 0"));
    d = ok; d.count = INT64_MIN;
    EXPECT(refused(plain, d, "count < 0"));
    // the bound: n + count <= 2^31 - 2, whatever count is
    d = ok; d.count = LSQ_GROW_MAX_ROWS - 1000;
    EXPECT(lsq_grow_add_refusal(plain, &d) == nullptr);
    d.count += 1;
    EXPECT(refused(plain, d, "2^31"));
    d.count = INT64_MAX;
    EXPECT(refused(plain, d, "2^31"));
    const lsq_grow_shape full{LSQ_GROW_MAX_ROWS, 4, 1, 0, 0, 0, 0};
    d = ok; d.count = 1;
    EXPECT(refused(full, d, "2^31"));
    d.count = 0; d.codes = nullptr; d.dbnorms = nullptr;
    EXPECT(lsq_grow_add_refusal(full, &d) == nullptr);                // count == 0: a no-op, nothing required
    // required arrays and the wrong ones
    d = ok; d.codes = nullptr;
    EXPECT(refused(plain, d, "codes are required"));
    d = ok; d.dbnorms = nullptr;
    EXPECT(refused(plain, d, "dbnorms are required"));
    d = ok; d.norm_codes = nc;
    EXPECT(refused(plain, d, "not packed"));
    d = ok;
    EXPECT(refused(packed, d, "dbnorms given"));
    d.dbnorms = nullptr;
    EXPECT(refused(packed, d, "norm_codes are required"));
    d.norm_codes = nc;
    EXPECT(lsq_grow_add_refusal(packed, &d) == nullptr);
    d = ok; d.list_of_row = lor;
    EXPECT(refused(plain, d, "no lists"));
    EXPECT(lsq_grow_add_refusal(with_lists, &d) == nullptr);
    d.list_of_row = nullptr;
    EXPECT(refused(with_lists, d, "list_of_row is required"));
    d = ok;
    EXPECT(refused(with_base, d, "base is required"));
    d.base = base; d.ldb = 3;
    EXPECT(refused(with_base, d, "ldb < d"));
    d.ldb = 6;
    EXPECT(lsq_grow_add_refusal(with_base, &d) == nullptr);
    d.base = reinterpret_cast<const char *>(base) + 1;
    EXPECT(refused(with_base, d, "4-byte aligned"));
    lsq_index_add_desc b{};
    b.count = 8; b.base = reinterpret_cast<const char *>(base) + 1; b.ldb = 4;
    EXPECT(lsq_grow_add_refusal(u8_base, &b) == nullptr);             // bytes may start anywhere
    EXPECT(refused(base_only, b, "4-byte aligned"));
    b.codes = codes;
    EXPECT(refused(u8_base, b, "holds none"));
    d = ok; d.base = base; d.ldb = 4;
    EXPECT(refused(plain, d, "holds none"));

    // reserve
    EXPECT(lsq_grow_reserve_refusal(1000, 999) != nullptr);
    EXPECT(lsq_grow_reserve_refusal(1000, 1000) == nullptr);
    EXPECT(lsq_grow_reserve_refusal(1000, INT64_MIN) != nullptr);
    EXPECT(lsq_grow_reserve_refusal(1000, LSQ_GROW_MAX_ROWS) == nullptr);
    EXPECT(lsq_grow_reserve_refusal(1000, LSQ_GROW_MAX_ROWS + 1) != nullptr);
    EXPECT(lsq_grow_reserve_refusal(1000, INT64_MAX) != nullptr);

    // the capacity rule: at least what is needed, the factor 3/2 otherwise, never past the bound unless asked, monotone, and a logarithmic number of moves
    EXPECT(lsq_grow_capacity(1000, 1001) == 1500);
    EXPECT(lsq_grow_capacity(1000, 5000) == 5000);
    EXPECT(lsq_grow_capacity(1, 2) == 2);
    EXPECT(lsq_grow_capacity(0, 1) == 1);
    EXPECT(lsq_grow_capacity(LSQ_GROW_MAX_ROWS - 1, LSQ_GROW_MAX_ROWS) == LSQ_GROW_MAX_ROWS);
    EXPECT(lsq_grow_capacity(LSQ_GROW_MAX_ROWS, LSQ_GROW_MAX_ROWS) == LSQ_GROW_MAX_ROWS);
    int64_t cap = 1, moves = 0;
    for (int64_t n = 1; n < LSQ_GROW_MAX_ROWS; n = n + 1 + n / 7) {
        if (n > cap) {
            const int64_t next = lsq_grow_capacity(cap, n);
            EXPECT(next >= n && next >= cap && next <= LSQ_GROW_MAX_ROWS);
            cap = next;
            ++moves;
        }
    }
    EXPECT(moves > 10 && moves < 80);
    // the byte counts the library derives from a capacity stay inside size_t: the widest row (17 bytes) and a base of 4096 floats per row at the bound
    const uint64_t rows = (uint64_t)LSQ_GROW_MAX_ROWS;
    EXPECT(rows * 17u + 16u > rows && rows * 4096u * 4u / 4096u / 4u == rows);
    if (failures) printf("grow_check: %d FAILED\n", failures);
    else printf("grow_check: all passed\n");
    return failures ? 1 : 0;
}
