// half_check_main.cpp -- a stand-alone host program over csrc/lsq_half_check.h: the narrowing and widening rules of the half-precision base rows at their edge
// values (against expected bits written out by hand and against the hardware's own float arithmetic), the format field, the alignment and argument rules of
// lsq_narrow_rows_cpu / lsq_index_narrow_base / lsq_index_get_base, the staging-chunk rule of a host-buffer lsq_index_get_base and lsq_narrow_rows_cpu's body
// over ragged shapes in exactly-sized arrays -- none of which needs a device.  Built with the host compiler alone, usually under
// -fsanitize=address,undefined (tests/test_half_base.py does that where the compiler has the runtimes): a read past a source row, a write past a destination
// row, a shift by a negative count or signed overflow in an offset is then an error, not a wrong number.
//   c++ -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all tools/half_check_main.cpp -o half_check && ./half_check
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../local-search-quantization_amd/csrc/lsq_half_check.h"

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static bool has(const char *why, const char *word) { return why && strstr(why, word); }
static float f(uint32_t u) { return lsq_half_float(u); }

// a small generator: the program must not depend on the C library's rand
static uint32_t next(uint64_t *s) { *s = *s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(*s >> 32); }

// round-to-nearest-even of |x| to a multiple of `step` (a power of two), by the hardware: the reference the integer rule is held to in the normal range
static float rne_to_step(float x, float step) { return nearbyintf(x / step) * step; }

int main() {
    // ---- the format field: 0 f32, 2 / 3 the halves, everything else uint8 as before it was a format
    EXPECT(lsq_base_format(0) == 0 && lsq_base_format(1) == 1 && lsq_base_format(LSQ_BASE_F16) == 2 && lsq_base_format(LSQ_BASE_BF16) == 3);
    EXPECT(lsq_base_format(4) == 1 && lsq_base_format(-1) == 1 && lsq_base_format(255) == 1 && lsq_base_format(INT32_MIN) == 1);
    EXPECT(lsq_base_elem_bytes(0) == 4 && lsq_base_elem_bytes(1) == 1 && lsq_base_elem_bytes(2) == 2 && lsq_base_elem_bytes(3) == 2);
    alignas(16) static unsigned char buf[32];
    EXPECT(lsq_base_align_refusal(0, buf) == nullptr && has(lsq_base_align_refusal(0, buf + 2), "4-byte"));
    EXPECT(lsq_base_align_refusal(2, buf + 2) == nullptr && has(lsq_base_align_refusal(2, buf + 1), "2-byte") && has(lsq_base_align_refusal(3, buf + 3), "2-byte"));
    EXPECT(lsq_base_align_refusal(1, buf + 1) == nullptr);

    // ---- Identity N at the edge values: (f32 bits, f16 bits, bf16 bits)
    struct Case { uint32_t x; uint16_t h, b; };
    const Case cases[] = {
        {0x00000000u, 0x0000, 0x0000}, {0x80000000u, 0x8000, 0x8000},
        {0x33000000u, 0x0000, 0x3300},                  // 2^-25: half of the smallest f16 subnormal, the tie goes to the even 0
        {0x33000001u, 0x0001, 0x3300}, {0x33800000u, 0x0001, 0x3380}, {0x33C00000u, 0x0002, 0x33C0},      // just above; 2^-24; 1.5 2^-24: a tie, up to the even 2
        {0x387FC000u, 0x03FF, 0x3880},                  // the largest f16 subnormal
        {0x387FE000u, 0x0400, 0x3880},                  // the tie above it rounds into the smallest normal
        {0x38800000u, 0x0400, 0x3880},                  // 2^-14
        {0x3F800000u, 0x3C00, 0x3F80}, {0x3F801000u, 0x3C00, 0x3F80}, {0x3F803000u, 0x3C02, 0x3F80},      // f16 ties: down at an even mantissa, up at an odd one
        {0x3F800FFFu, 0x3C00, 0x3F80}, {0x3F801001u, 0x3C01, 0x3F80},
        {0x3F808000u, 0x3C04, 0x3F80}, {0x3F818000u, 0x3C0C, 0x3F82}, {0x3F808001u, 0x3C04, 0x3F81}, {0x3F817FFFu, 0x3C0C, 0x3F81},      // the same for bf16
        {0x477FE000u, 0x7BFF, 0x4780}, {0x477FEFFFu, 0x7BFF, 0x4780}, {0x477FF000u, 0x7C00, 0x4780}, {0x47800000u, 0x7C00, 0x4780},      // 65504, 65519.99, 65520 (overflows f16), 65536
        {0xC77FF000u, 0xFC00, 0xC780},
        {0x3F7FFFFFu, 0x3C00, 0x3F80},                  // the bf16 carry runs into the exponent (and the f16 one too)
        {0x3F7F7FFFu, 0x3BFC, 0x3F7F}, {0x3F7F8000u, 0x3BFC, 0x3F80},
        {0x7F7FFFFFu, 0x7C00, 0x7F80},                  // f32 max: bf16 inf
        {0x7F7F7FFFu, 0x7C00, 0x7F7F}, {0x7F7F8000u, 0x7C00, 0x7F80},
        {0x00000001u, 0x0000, 0x0000}, {0x007FFFFFu, 0x0000, 0x0080}, {0x00008000u, 0x0000, 0x0000}, {0x00018000u, 0x0000, 0x0002}, {0x00010000u, 0x0000, 0x0001},
        {0x0000FFFFu, 0x0000, 0x0001}, {0x00400000u, 0x0000, 0x0040}, {0x807F8000u, 0x8000, 0x8080},      // f32 subnormals: bf16 keeps them (ties to even)
        {0x7F800000u, 0x7C00, 0x7F80}, {0xFF800000u, 0xFC00, 0xFF80},
    };
    for (const Case &c : cases) {
        EXPECT(lsq_narrow_f16(f(c.x)) == c.h);
        EXPECT(lsq_narrow_bf16(f(c.x)) == c.b);
        if (lsq_narrow_f16(f(c.x)) != c.h || lsq_narrow_bf16(f(c.x)) != c.b)
            printf("  x=%08x: f16 %04x (want %04x) bf16 %04x (want %04x)\n", c.x, lsq_narrow_f16(f(c.x)), c.h, lsq_narrow_bf16(f(c.x)), c.b);
    }
    // NaN -> a NaN of the same sign, whatever the payload (a truncation would turn 0x7F800001 into inf)
    for (uint32_t x : {0x7FC00000u, 0x7F800001u, 0x7FFFFFFFu, 0x7F80FFFFu, 0xFFC00000u, 0xFF800001u}) {
        const uint16_t h = lsq_narrow_f16(f(x)), b = lsq_narrow_bf16(f(x));
        EXPECT((h & 0x7C00) == 0x7C00 && (h & 0x03FF) != 0 && (h >> 15) == (x >> 31));
        EXPECT((b & 0x7F80) == 0x7F80 && (b & 0x007F) != 0 && (b >> 15) == (x >> 31));
        const float wh = lsq_widen_f16(h), wb = lsq_widen_bf16(b);
        EXPECT(wh != wh && wb != wb);
    }
    // ---- Identity W: every half widens to the float whose narrowing it is (all 65536 bit patterns, both formats), subnormals included
    for (uint32_t h = 0; h < 65536; ++h) {
        const float wh = lsq_widen_f16((uint16_t)h), wb = lsq_widen_bf16((uint16_t)h);
        if (wh == wh) EXPECT(lsq_narrow_f16(wh) == h);
        if (wb == wb) EXPECT(lsq_narrow_bf16(wb) == h);
        if (failures > 20) break;
    }
    EXPECT(lsq_half_bits(lsq_widen_f16(0x0001)) == 0x33800000u && lsq_half_bits(lsq_widen_f16(0x03FF)) == 0x387FC000u && lsq_half_bits(lsq_widen_f16(0x8400)) == 0xB8800000u);
    EXPECT(lsq_half_bits(lsq_widen_bf16(0x0001)) == 0x00010000u && lsq_half_bits(lsq_widen_bf16(0xFF80)) == 0xFF800000u);
    // ---- random floats across the exponent range against the hardware's arithmetic: the nearest-even multiple of the half's spacing at that magnitude
    uint64_t seed = 2500;
    for (int i = 0; i < 200000 && failures < 20; ++i) {
        const uint32_t u = next(&seed);
        const float x = f(u), a = fabsf(x);
        if (x != x) continue;
        {   // f16: spacing 2^(e - 10) for 2^e <= a < 2^(e + 1) in the normal range, 2^-24 below 2^-14
            float want;
            if (a >= 65520.0f) want = INFINITY;
            else {
                int e;
                (void)frexpf(a, &e);                                         // a = m 2^e, 0.5 <= m < 1: the binade is 2^(e - 1)
                const float step = a < 6.103515625e-05f ? 5.9604644775390625e-08f : ldexpf(1.0f, e - 1 - 10);
                want = rne_to_step(a, step);
            }
            const float got = lsq_widen_f16(lsq_narrow_f16(x));
            EXPECT(lsq_half_bits(fabsf(got)) == lsq_half_bits(want) && signbit(got) == signbit(x));
        }
        {   // bf16: 8 significant bits, f32's exponent range -- in double, so that the quotient of a subnormal is exact
            const double ad = (double)a;
            double want;
            if (a == INFINITY) want = (double)INFINITY;
            else if (a == 0.0f) want = 0.0;
            else {
                int e;
                (void)frexp(ad, &e);
                const int e2 = e - 1 < -126 ? -126 : e - 1;                   // subnormals share the spacing of the smallest binade
                const double step = ldexp(1.0, e2 - 7);
                want = nearbyint(ad / step) * step;
                if (want > 3.3895313892515355e+38) want = (double)INFINITY;  // past the largest finite bf16 (0x7F7F)
            }
            const float got = lsq_widen_bf16(lsq_narrow_bf16(x));
            EXPECT((double)fabsf(got) == want && signbit(got) == signbit(x));
        }
    }
    // ---- the counts
    {
        lsq_narrow_counts c;
        const float xs[] = {65520.0f, -1e30f, 1e-30f, 0.0f, -0.0f, f(0x7FC00000u), INFINITY, 1.0f, f(0x33000000u)};
        for (float x : xs) lsq_narrow_count(x, lsq_narrow_f16(x), LSQ_BASE_F16, &c);
        EXPECT(c.to_inf == 2 && c.to_zero == 2 && c.nans == 1);
        lsq_narrow_counts b;
        for (float x : xs) lsq_narrow_count(x, lsq_narrow_bf16(x), LSQ_BASE_BF16, &b);
        EXPECT(b.to_inf == 0 && b.to_zero == 0 && b.nans == 1);
        lsq_narrow_count(f(0x7F7FFFFFu), lsq_narrow_bf16(f(0x7F7FFFFFu)), LSQ_BASE_BF16, &b);
        lsq_narrow_count(f(0x00000001u), lsq_narrow_bf16(f(0x00000001u)), LSQ_BASE_BF16, &b);
        EXPECT(b.to_inf == 1 && b.to_zero == 1);
    }
    // ---- the argument rules
    alignas(16) static float src4[16];
    alignas(16) static uint16_t dst4[16];
    EXPECT(lsq_narrow_rows_refusal(dst4, src4, 2, 3, 3, 3, LSQ_BASE_F16) == nullptr && lsq_narrow_rows_refusal(nullptr, nullptr, 0, 3, 3, 3, LSQ_BASE_BF16) == nullptr);
    EXPECT(has(lsq_narrow_rows_refusal(dst4, src4, 2, 3, 3, 3, 0), "format") && has(lsq_narrow_rows_refusal(dst4, src4, 2, 3, 3, 3, 1), "format") &&
           has(lsq_narrow_rows_refusal(dst4, src4, 2, 3, 3, 3, 7), "format"));
    EXPECT(has(lsq_narrow_rows_refusal(dst4, src4, -1, 3, 3, 3, 2), "n < 0") && has(lsq_narrow_rows_refusal(dst4, src4, 2, 0, 3, 3, 2), "d < 1"));
    EXPECT(has(lsq_narrow_rows_refusal(dst4, src4, 2, 3, 2, 3, 2), "lds < d") && has(lsq_narrow_rows_refusal(dst4, src4, 2, 3, 3, 2, 2), "ldd < d"));
    EXPECT(has(lsq_narrow_rows_refusal(nullptr, src4, 2, 3, 3, 3, 2), "null") && has(lsq_narrow_rows_refusal(dst4, nullptr, 2, 3, 3, 3, 2), "null"));
    EXPECT(has(lsq_narrow_rows_refusal(reinterpret_cast<char *>(dst4) + 1, src4, 2, 3, 3, 3, 2), "2-byte") &&
           has(lsq_narrow_rows_refusal(dst4, reinterpret_cast<char *>(src4) + 2, 2, 3, 3, 3, 2), "4-byte"));
    EXPECT(lsq_narrow_base_refusal(true, 0, 2) == nullptr && lsq_narrow_base_refusal(true, 0, 3) == nullptr);
    EXPECT(has(lsq_narrow_base_refusal(false, 0, 2), "no base") && has(lsq_narrow_base_refusal(true, 1, 2), "not f32") && has(lsq_narrow_base_refusal(true, 2, 2), "not f32") &&
           has(lsq_narrow_base_refusal(true, 0, 7), "format") && has(lsq_narrow_base_refusal(true, 0, 0), "format") && has(lsq_narrow_base_refusal(true, 0, 1), "format"));
    EXPECT(lsq_get_base_refusal(true, 10, 4, 0, 10, 4, src4) == nullptr && lsq_get_base_refusal(true, 10, 4, 10, 0, 4, nullptr) == nullptr);      // the empty range at n
    EXPECT(has(lsq_get_base_refusal(false, 10, 4, 0, 1, 4, src4), "no base") && has(lsq_get_base_refusal(true, 10, 4, 0, -1, 4, src4), "count < 0"));
    EXPECT(has(lsq_get_base_refusal(true, 10, 4, -1, 1, 4, src4), "leaves") && has(lsq_get_base_refusal(true, 10, 4, 11, 0, 4, src4), "leaves") &&
           has(lsq_get_base_refusal(true, 10, 4, 5, 6, 4, src4), "leaves") && has(lsq_get_base_refusal(true, 10, 4, INT64_MAX, 1, 4, src4), "leaves") &&
           has(lsq_get_base_refusal(true, 10, 4, 1, INT64_MAX, 4, src4), "leaves"));
    EXPECT(has(lsq_get_base_refusal(true, 10, 4, 0, 1, 3, src4), "ldo < d") && has(lsq_get_base_refusal(true, 10, 4, 0, 1, 4, nullptr), "null") &&
           has(lsq_get_base_refusal(true, 10, 4, 0, 1, 4, reinterpret_cast<char *>(src4) + 1), "4-byte"));
    // ---- the chunk rule of a host-buffer get_base: never 0 rows, never more than count, the budget honoured, the option only shrinks; the chunks cover the range
    EXPECT(lsq_base_chunk_rows(1, 128, 0) == 1 && lsq_base_chunk_rows(1000, 128, 0) == 1000 && lsq_base_chunk_rows(1000000, 128, 0) == LSQ_BASE_STAGE_BYTES / 512);
    EXPECT(lsq_base_chunk_rows(1000000, 128, 7) == 7 && lsq_base_chunk_rows(5, 128, 7) == 5 && lsq_base_chunk_rows(1000, 128, INT64_MAX) == 1000);
    EXPECT(lsq_base_chunk_rows(10, INT32_MAX, 0) == 1 && lsq_base_chunk_rows(0, 4, 0) == 1 && lsq_base_chunk_rows((int64_t)INT32_MAX - 1, 1, 0) == LSQ_BASE_STAGE_BYTES / 4);
    for (int64_t n : {1, 2, 63, 64, 65, 1000}) {
        for (int64_t opt : {0, 1, 3, 64, 999, 1000, 1001}) {
            const int64_t rows = lsq_base_chunk_rows(n, 24, opt);
            int64_t covered = 0, chunks = 0;
            for (int64_t r0 = 0; r0 < n; r0 += rows) { covered += (n - r0 < rows ? n - r0 : rows); ++chunks; }
            EXPECT(rows >= 1 && rows <= n && covered == n && chunks == lsq_base_chunks(n, rows));
        }
    }
    // ---- lsq_narrow_rows_cpu's body over ragged shapes: exactly-sized arrays (the last row ends at its d-th element), padded pitches, one thread and several
    for (int format : {LSQ_BASE_F16, LSQ_BASE_BF16}) {
        for (int d : {1, 7, 8, 9, 40}) {
            for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)33, (int64_t)3000}) {
                for (int pad : {0, 1, 3}) {
                    for (int nt : {1, 3}) {
                        const int64_t lds = d + pad, ldd = d + (pad ? pad + 1 : 0);
                        std::vector<float> src(n ? (size_t)((n - 1) * lds + d) : 0);
                        std::vector<uint16_t> dst(n ? (size_t)((n - 1) * ldd + d) : 0, (uint16_t)0xABCD);
                        for (float &v : src) v = f(next(&seed));
                        lsq_narrow_counts got, want;
                        const char *why = lsq_narrow_rows_host(n ? dst.data() : nullptr, n ? src.data() : nullptr, n, d, lds, ldd, format, nt, &got);
                        EXPECT(why == nullptr);
                        bool ok = true;
                        for (int64_t i = 0; i < n && ok; ++i) {
                            for (int t = 0; t < d; ++t) {
                                const float x = src[(size_t)(i * lds + t)];
                                const uint16_t h = lsq_narrow_half(x, format);
                                lsq_narrow_count(x, h, format, &want);
                                ok = ok && dst[(size_t)(i * ldd + t)] == h;
                            }
                            for (int64_t t = d; t < ldd && i + 1 < n; ++t) ok = ok && dst[(size_t)(i * ldd + t)] == 0xABCD;      // the gaps are not written
                        }
                        EXPECT(ok && got.to_inf == want.to_inf && got.to_zero == want.to_zero && got.nans == want.nans);
                    }
                }
            }
        }
    }
    // a refusal writes nothing
    {
        std::vector<float> src(12, 1.0f);
        std::vector<uint16_t> dst(12, (uint16_t)0xABCD);
        EXPECT(has(lsq_narrow_rows_host(dst.data(), src.data(), 3, 4, 3, 4, LSQ_BASE_F16, 1), "lds < d"));
        EXPECT(has(lsq_narrow_rows_host(dst.data(), src.data(), 3, 4, 4, 4, 1, 1), "format"));
        bool untouched = true;
        for (uint16_t v : dst) untouched = untouched && v == 0xABCD;
        EXPECT(untouched);
    }
    if (failures) { printf("%d checks FAILED\n", failures); return 1; }
    printf("half_check: all passed\n");
    return 0;
}
