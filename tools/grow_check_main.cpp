// grow_check_main.cpp -- a stand-alone host program over csrc/lsq_grow_check.h: the argument rules of lsq_index_add / lsq_index_reserve, the 2^31 - 2 bound
// the capacity arithmetic and the sizes of the index's row arrays (every shape against the written-out formulas, and at the bounds), which need no device.  Built with the host compiler alone, usually under -fsanitize=address,undefined (tests/test_index_add.py
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

    // the row arrays: for every shape the description gives the sizes the library used to write out by hand
    const int formats[4] = {0, 1, LSQ_BASE_F16, LSQ_BASE_BF16};
    const uint64_t elem[4] = {4, 1, 2, 2};
    const uint64_t n = 1000, cap2 = 1500, m = 7, dim = 12;
    for (int has_codes = 0; has_codes < 2; ++has_codes)
        for (int pk = 0; pk < 2; ++pk)
            for (int has_base = 0; has_base < 2; ++has_base)
                for (int f = 0; f < 4; ++f)
                    for (uint64_t ldb = dim; ldb <= dim + 1; ++ldb) {
                        if (pk && !has_codes) continue;
                        lsq_rows_desc r[LSQ_ROWS_KINDS];
                        lsq_rows_describe(has_codes != 0, pk != 0, (int)m, has_base != 0, (int)dim, (int64_t)ldb, formats[f], r);
                        const lsq_rows_desc &cd = r[LSQ_ROWS_CODES], &nd = r[LSQ_ROWS_NORMS], &bd = r[LSQ_ROWS_BASE];
                        const uint64_t rowb = pk ? m + 1 : m, e = elem[f];
                        EXPECT((cd.pitch != 0) == (has_codes != 0));
                        EXPECT((nd.pitch != 0) == (has_codes && !pk));                              // norms exist iff codes && !packed
                        EXPECT((bd.pitch != 0) == (has_base != 0));
                        if (has_codes) {
                            EXPECT(cd.pitch == rowb && cd.width == rowb);
                            EXPECT(cd.bytes_for((int64_t)cap2) == cap2 * rowb + 16 && cd.bytes_used((int64_t)n) == n * rowb);      // index_capacity
                            EXPECT(cd.bytes_for((int64_t)n) == n * rowb + 16);                       // the SHRINK fit; create_packed's n * (m + 1) + 16
                        }
                        if (has_codes && !pk) {
                            EXPECT(nd.pitch == 4 && nd.width == 4);                                 // the gather's (4, 4)
                            EXPECT(nd.bytes_for((int64_t)cap2) == 4 * cap2 && nd.bytes_used((int64_t)n) == 4 * n && nd.bytes_for((int64_t)n) == 4 * n);
                        }
                        if (has_base) {
                            EXPECT(bd.pitch == ldb * e && bd.width == dim * e);                         // the gather's and the 2-D copy's pitch and width
                            EXPECT(bd.bytes_for((int64_t)cap2) == cap2 * ldb * e && bd.bytes_used((int64_t)n) == ((n - 1) * ldb + dim) * e);
                            EXPECT(bd.bytes_for((int64_t)n) == n * ldb * e);
                            EXPECT(bd.bytes_used(1) == dim * e);
                            if (e == 2 && ldb == dim) EXPECT(bd.bytes_for((int64_t)cap2) == cap2 * dim * 2);      // narrow_base's new buffer
                        }
                    }
    // nothing overflows 64 unsigned bits: the widest arrays at the bounds, against 128-bit arithmetic
    {
        lsq_rows_desc r[LSQ_ROWS_KINDS];
        const int64_t top = LSQ_GROW_MAX_ROWS, wide = INT32_MAX;
        lsq_rows_describe(true, true, 16, true, INT32_MAX, wide, 0, r);
        for (const lsq_rows_desc &a : r) {
            const unsigned __int128 need = (unsigned __int128)top * a.pitch + a.slack, used = (unsigned __int128)(top - 1) * a.pitch + a.width;
            EXPECT(need <= UINT64_MAX && used <= UINT64_MAX);
            EXPECT((unsigned __int128)a.bytes_for(top) == need && (unsigned __int128)a.bytes_used(top) == used);
        }
        EXPECT(r[LSQ_ROWS_BASE].pitch == (uint64_t)INT32_MAX * 4 && r[LSQ_ROWS_CODES].pitch == 17 && r[LSQ_ROWS_NORMS].pitch == 0);
    }
    if (failures) printf("grow_check: %d FAILED\n", failures);
    else printf("grow_check: all passed\n");
    return failures ? 1 : 0;
}
