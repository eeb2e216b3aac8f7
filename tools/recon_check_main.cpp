// recon_check_main.cpp -- a stand-alone host program over csrc/lsq_recon_check.h: the chunk rule of a host-buffer lsq_index_reconstruct, the argument rules of the decode's
// entry points and lsq_reconstruct_cpu's body at the edge extents (count 0, one row, a partial last chunk, ids at both ends of the range), which need no
// device.  Built with the host compiler alone, usually under -fsanitize=address,undefined (tests/test_reconstruct.py does that where the compiler has the
// runtimes): a read past a code row, a write past an output row or signed overflow in an offset is then an error, not a wrong number.
//   c++ -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all tools/recon_check_main.cpp -o recon_check && ./recon_check
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../local-search-quantization_amd/csrc/lsq_recon_check.h"

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static bool has(const char *why, const char *word) { return why && strstr(why, word); }
static uint32_t bits(float v) { uint32_t b; memcpy(&b, &v, 4); return b; }

// the contract by hand, one element
static float chain(const std::vector<float> &K, const uint8_t *b, int m, int h, int d, int t) {
    float acc = 0.0f;
    for (int j = 0; j < m; ++j) acc += K[((size_t)j * h + b[j]) * d + t];
    return acc;
}

int main() {
    // ---- the chunk rule: never 0 rows, never more than n, the budget honoured, the option only shrinks
    EXPECT(lsq_recon_chunk_rows(1, 128, 0) == 1);
    EXPECT(lsq_recon_chunk_rows(1000, 128, 0) == 1000);
    EXPECT(lsq_recon_chunk_rows(1000000, 128, 0) == LSQ_RECON_STAGE_BYTES / 512);
    EXPECT(lsq_recon_chunk_rows(1000000, 128, 7) == 7);
    EXPECT(lsq_recon_chunk_rows(5, 128, 7) == 5);
    EXPECT(lsq_recon_chunk_rows(1000, 128, INT64_MAX) == 1000);
    EXPECT(lsq_recon_chunk_rows(10, INT32_MAX, 0) == 1);                     // one row over the budget: still one row
    EXPECT(lsq_recon_chunk_rows(0, 4, 0) == 1);                              // (n == 0 never reaches a chunk loop)
    EXPECT(lsq_recon_chunk_rows((int64_t)INT32_MAX - 1, 1, 0) == LSQ_RECON_STAGE_BYTES / 4);
    EXPECT(lsq_recon_chunks(0, 5) == 0 && lsq_recon_chunks(1, 5) == 1 && lsq_recon_chunks(5, 5) == 1 && lsq_recon_chunks(6, 5) == 2);
    for (int64_t n : {1, 2, 63, 64, 65, 1000}) {
        for (int64_t opt : {0, 1, 3, 64, 999, 1000, 1001}) {
            const int64_t rows = lsq_recon_chunk_rows(n, 24, opt);
            int64_t covered = 0, chunks = 0;
            for (int64_t r0 = 0; r0 < n; r0 += rows) { covered += (n - r0 < rows ? n - r0 : rows); ++chunks; }
            EXPECT(rows >= 1 && rows <= n && covered == n && chunks == lsq_recon_chunks(n, rows));
        }
    }
    // ---- the shape and selection rules
    EXPECT(lsq_recon_shape_refusal(4, 10, 8, 256, 8, 4) == nullptr);
    EXPECT(lsq_recon_shape_refusal(4, 0, 1, 1, 1, 4) == nullptr);
    EXPECT(has(lsq_recon_shape_refusal(0, 10, 8, 256, 8, 4), "d < 1"));
    EXPECT(has(lsq_recon_shape_refusal(4, -1, 8, 256, 8, 4), "n < 0"));
    EXPECT(has(lsq_recon_shape_refusal(4, (int64_t)INT32_MAX, 8, 256, 8, 4), "2^31"));
    EXPECT(has(lsq_recon_shape_refusal(4, 10, 0, 256, 8, 4), "m must"));
    EXPECT(has(lsq_recon_shape_refusal(4, 10, 17, 256, 17, 4), "m must"));
    EXPECT(has(lsq_recon_shape_refusal(4, 10, 8, 257, 8, 4), "h must"));
    EXPECT(has(lsq_recon_shape_refusal(4, 10, 8, 256, 7, 4), "ldc < m"));
    EXPECT(has(lsq_recon_shape_refusal(4, 10, 8, 256, 8, 3), "ldo < d"));
    static int32_t some[2] = {0, 1};
    EXPECT(lsq_recon_select_refusal(nullptr, 0, 10, 0, 10, 0, false) == nullptr);
    EXPECT(lsq_recon_select_refusal(nullptr, 10, 0, 0, 10, 0, false) == nullptr);       // the empty range at the end
    EXPECT(lsq_recon_select_refusal(nullptr, 9, 1, 1, 10, LSQ_RECON_PAD_NAN, false) == nullptr);
    EXPECT(has(lsq_recon_select_refusal(nullptr, 9, 2, 0, 10, 0, false), "range"));
    EXPECT(has(lsq_recon_select_refusal(nullptr, -1, 1, 0, 10, 0, false), "range"));
    EXPECT(has(lsq_recon_select_refusal(nullptr, 11, 0, 0, 10, 0, false), "range"));
    EXPECT(has(lsq_recon_select_refusal(nullptr, INT64_MAX, 1, 0, 10, 0, false), "range"));      // no overflow in start + count
    EXPECT(has(lsq_recon_select_refusal(nullptr, 1, INT64_MAX, 0, 10, 0, false), "2^31"));
    EXPECT(lsq_recon_select_refusal(some, INT64_MAX, 2, 1, 10, 0, false) == nullptr);  // ids: start is not read
    EXPECT(has(lsq_recon_select_refusal(some, 0, -1, 0, 10, 0, false), "count < 0"));
    EXPECT(has(lsq_recon_select_refusal(some, 0, 2, 2, 10, 0, false), "id_base"));
    EXPECT(has(lsq_recon_select_refusal(some, 0, 2, -1, 10, 0, false), "id_base"));
    EXPECT(has(lsq_recon_select_refusal(some, 0, 2, 0, 10, 4, false), "flags"));
    EXPECT(has(lsq_recon_select_refusal(some, 0, 2, 0, 10, -1, true), "flags"));
    EXPECT(has(lsq_recon_select_refusal(some, 0, 2, 0, 10, LSQ_RECON_ADD_COARSE, false), "without lists"));
    EXPECT(lsq_recon_select_refusal(some, 0, 2, 0, 10, LSQ_RECON_ADD_COARSE | LSQ_RECON_PAD_NAN, true) == nullptr);
    {
        const int32_t ids[6] = {0, 9, 10, -1, INT32_MAX, INT32_MIN};
        int64_t first = -1;
        EXPECT(lsq_recon_count_bad_ids(ids, 6, 0, 10, &first) == 4 && first == 2);
        EXPECT(lsq_recon_count_bad_ids(ids, 2, 0, 10) == 0);
        EXPECT(lsq_recon_count_bad_ids(ids, 6, 1, 10) == 4);                 // 0 leaves, 10 enters; INT32_MIN - 1 does not wrap
        EXPECT(lsq_recon_count_bad_ids(ids, 0, 0, 10) == 0);
    }
    // ---- the decode at the edge extents: exactly-sized arrays, so that a byte read or written outside them is the sanitizer's to report
    const int h = 256;
    for (int m : {1, 7, 16}) {
        for (int d : {1, 5, 8}) {
            for (int64_t n : {1, 2, 67}) {
                for (int pitch : {0, 1}) {
                    const int64_t ldc = m + pitch, ldo = d + 3 * pitch;
                    std::vector<float> K((size_t)m * h * d);
                    for (size_t e = 0; e < K.size(); ++e) K[e] = (float)((int)(e * 2654435761u % 2001u) - 1000) * 0.37f;
                    for (int e = 0; e < m * h; ++e) K[(size_t)e * d] = -0.0f;                   // column 0: every codeword -0.0
                    std::vector<uint8_t> codes((size_t)((n - 1) * ldc + m));                  // the last row ends at its m-th byte
                    for (size_t e = 0; e < codes.size(); ++e) codes[e] = (uint8_t)(e * 131u + 7u);
                    std::vector<float> cent((size_t)3 * d);
                    for (size_t e = 0; e < cent.size(); ++e) cent[e] = 0.5f + (float)e;
                    std::vector<int32_t> lor((size_t)n);
                    for (int64_t i = 0; i < n; ++i) lor[(size_t)i] = (int32_t)(i % 3);
                    // every row, several threads (more than rows when n is small); the last output row ends at its d-th float
                    std::vector<float> out((size_t)((n - 1) * ldo + d), 7.0f);
                    lsq_recon_cpu_args a{out.data(), ldo, codes.data(), ldc, K.data(), nullptr, n, 0, n, m, h, d, nullptr, nullptr, 0};
                    EXPECT(lsq_recon_cpu(a, 5) == nullptr);
                    for (int64_t i = 0; i < n; ++i)
                        for (int t = 0; t < d; ++t) EXPECT(bits(out[(size_t)(i * ldo + t)]) == bits(chain(K, &codes[(size_t)(i * ldc)], m, h, d, t)));
                    EXPECT(bits(out[0]) == 0u);                                               // +0.0, not -0.0
                    for (int64_t i = 0; i + 1 < n; ++i)
                        for (int64_t t = d; t < ldo; ++t) EXPECT(out[(size_t)(i * ldo + t)] == 7.0f);      // the gaps between rows keep their sentinel
                    // ids at both ends of the range, repeated, descending, in base 1; outside ids at both ends with the pad; the coarse add
                    const int32_t ids[7] = {(int32_t)n, 1, (int32_t)n, 0, (int32_t)n + 1, 1, INT32_MIN};
                    std::vector<float> o2((size_t)(6 * ldo + d), 7.0f);
                    lsq_recon_cpu_args b{o2.data(), ldo, codes.data(), ldc, K.data(), ids, 7, 1, n, m, h, d, cent.data(), lor.data(),
                                         LSQ_RECON_ADD_COARSE | LSQ_RECON_PAD_NAN};
                    int64_t invalid = -1;
                    EXPECT(lsq_recon_cpu(b, 3, &invalid) == nullptr && invalid == 3);
                    for (int r = 0; r < 7; ++r) {
                        const int64_t row = (int64_t)ids[r] - 1;
                        for (int t = 0; t < d; ++t) {
                            const uint32_t got = bits(o2[(size_t)(r * ldo + t)]);
                            if (row < 0 || row >= n) EXPECT(got == 0x7FC00000u);
                            else EXPECT(got == bits(chain(K, &codes[(size_t)(row * ldc)], m, h, d, t) + cent[(size_t)(lor[(size_t)row] * d + t)]));
                        }
                    }
                    // without the pad the same ids are refused and nothing is written
                    std::vector<float> o3((size_t)(6 * ldo + d), 7.0f);
                    lsq_recon_cpu_args c = b;
                    c.out = o3.data(); c.flags = LSQ_RECON_ADD_COARSE;
                    EXPECT(has(lsq_recon_cpu(c, 3), "outside"));
                    for (float v : o3) EXPECT(v == 7.0f);
                    // count 0: nothing is read, nothing is written -- not even null pointers
                    lsq_recon_cpu_args z{nullptr, ldo, nullptr, ldc, nullptr, nullptr, 0, 0, n, m, h, d, nullptr, nullptr, 0};
                    EXPECT(lsq_recon_cpu(z, 4) == nullptr);
                    z.count = 1;
                    EXPECT(has(lsq_recon_cpu(z, 4), "null pointer"));
                }
            }
        }
    }
    // a code at or above h is refused before anything is written (h < 256)
    {
        const int m = 2, d = 3, hh = 4;
        std::vector<float> K((size_t)m * hh * d, 1.0f), out(6, 7.0f);
        const uint8_t codes[4] = {0, 3, 1, 4};
        lsq_recon_cpu_args a{out.data(), d, codes, m, K.data(), nullptr, 2, 0, 2, m, hh, d, nullptr, nullptr, 0};
        EXPECT(has(lsq_recon_cpu(a, 1), "code"));
        for (float v : out) EXPECT(v == 7.0f);
        a.count = 1;                                                             // the first row alone is fine
        EXPECT(lsq_recon_cpu(a, 1) == nullptr && out[0] == 2.0f && out[3] == 7.0f);
    }
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("recon_check: all passed\n");
    return 0;
}
