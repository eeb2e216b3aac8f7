// lsq_half_check.h -- the parts of the half-precision base rows that need no device: the format field, the narrowing and widening rules in
// integer arithmetic (Identity N / Identity W), the alignment rule of a base pointer, the argument rules of lsq_index_narrow_base / lsq_index_get_base /
// lsq_narrow_rows_cpu, the staging-chunk rule of a host-buffer lsq_index_get_base and lsq_narrow_rows_cpu's body.  Plain C++ over the public header alone, so
// that a stand-alone host program can exercise them (tools/half_check_main.cpp).
#pragma once

#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

#include "../../include/lsq_mi355x.h"

// the format a base_u8 field stands for: 0 f32, LSQ_BASE_F16, LSQ_BASE_BF16, and uint8 for EVERY other value (as before the field was a format)
inline int lsq_base_format(int base_u8) { return base_u8 == 0 ? 0 : (base_u8 == LSQ_BASE_F16 || base_u8 == LSQ_BASE_BF16) ? base_u8 : 1; }
inline bool lsq_base_is_half(int format) { return format == LSQ_BASE_F16 || format == LSQ_BASE_BF16; }
inline size_t lsq_base_elem_bytes(int format) { return format == 0 ? 4 : lsq_base_is_half(format) ? 2 : 1; }
// null: a base of `format` may start at p; else what is wrong (f32: 4-byte aligned, half: 2-byte aligned, uint8: anywhere)
inline const char *lsq_base_align_refusal(int format, const void *p) {
    if (format == 0 && ((uintptr_t)p & 3) != 0) return "the f32 base is not 4-byte aligned";
    if (lsq_base_is_half(format) && ((uintptr_t)p & 1) != 0) return "the half-precision base is not 2-byte aligned";
    return nullptr;
}

inline uint32_t lsq_half_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
inline float lsq_half_float(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

// ---- Identity N: round to nearest even ------------------------------------------------------------------------------------------------------------
// bf16 = the upper 16 bits of a binary32: (u + 0x7fff + ((u >> 16) & 1)) >> 16 -- the carry may run into the exponent (0x3f7fffff -> 0x3f80) and on
// into +-inf (f32 max -> 0x7f80), subnormals round like everything else; a NaN keeps its sign and its upper payload bits and has bit 6 set
inline uint16_t lsq_narrow_bf16(float x) {
    const uint32_t u = lsq_half_bits(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
// binary16: overflow to +-inf (from 65520 on), subnormals kept (steps of 2^-24; |x| <= 2^-25 -> +-0), NaN -> a quiet NaN with the upper payload bits: the
// bits of numpy's astype(float16)
inline uint16_t lsq_narrow_f16(float x) {
    const uint32_t u = lsq_half_bits(x), a = u & 0x7fffffffu;
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u | ((a >> 13) & 0x03ffu));
    if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);           // 65520 = the half-way point above 65504 (an even mantissa below it: the tie goes up)
    if (a < 0x38800000u) {                                            // below 2^-14: a subnormal half, value m 2^-24
        if (a < 0x33000000u) return sign;                             // below 2^-25: nearer to 0 than to 2^-24
        const uint32_t e = a >> 23, man = (a & 0x007fffffu) | 0x00800000u;      // value = man 2^(e - 150), 102 <= e <= 112
        const uint32_t shift = 126u - e;                              // m = man >> shift, 14 <= shift <= 24
        uint32_t m = man >> shift;
        const uint32_t rem = man & ((1u << shift) - 1u), half = 1u << (shift - 1u);
        if (rem > half || (rem == half && (m & 1u))) ++m;             // (m = 0x400 is the smallest normal: the right bits)
        return (uint16_t)(sign | m);
    }
    const uint32_t r = a + 0x0fffu + ((a >> 13) & 1u);                // RNE on the 13 dropped bits; a carry moves to the next exponent
    return (uint16_t)(sign | ((r - 0x38000000u) >> 13));
}

// ---- Identity W: exact ------------------------------------------------------------------------------------------------------------------------------
inline float lsq_widen_bf16(uint16_t h) { return lsq_half_float((uint32_t)h << 16); }
inline float lsq_widen_f16(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, man = h & 0x03ffu;
    if (e == 0x1fu) return lsq_half_float(sign | 0x7f800000u | (man << 13));      // inf, NaN (payload kept)
    if (e != 0u) return lsq_half_float(sign | ((e + 112u) << 23) | (man << 13));
    if (man == 0u) return lsq_half_float(sign);
    int s = 0;                                                        // a subnormal half man 2^-24: normalised (never flushed)
    uint32_t mm = man;
    while (!(mm & 0x0400u)) { mm <<= 1; ++s; }
    return lsq_half_float(sign | ((uint32_t)(113 - s) << 23) | ((mm & 0x03ffu) << 13));
}
inline uint16_t lsq_narrow_half(float x, int format) { return format == LSQ_BASE_F16 ? lsq_narrow_f16(x) : lsq_narrow_bf16(x); }
inline float lsq_widen_half(uint16_t h, int format) { return format == LSQ_BASE_F16 ? lsq_widen_f16(h) : lsq_widen_bf16(h); }

// what lsq_index_narrow_base counts (lsq_index_base_info): a finite value that became +-inf, a non-zero value that became +-0, a NaN
struct lsq_narrow_counts { int64_t to_inf = 0, to_zero = 0, nans = 0; };
inline void lsq_narrow_count(float x, uint16_t h, int format, lsq_narrow_counts *c) {
    const uint32_t a = lsq_half_bits(x) & 0x7fffffffu;
    const uint16_t inf = format == LSQ_BASE_F16 ? 0x7c00u : 0x7f80u, m = (uint16_t)(h & 0x7fffu);
    if (a > 0x7f800000u) c->nans += 1;
    else if (a < 0x7f800000u && m == inf) c->to_inf += 1;
    else if (a != 0u && m == 0u) c->to_zero += 1;
}

// ---- argument rules.  null: acceptable; else what is wrong (a string literal) ----------------------------------------------------------------------
inline const char *lsq_narrow_rows_refusal(const void *dst, const void *src, int64_t n, int d, int64_t lds, int64_t ldd, int format) {
    if (!lsq_base_is_half(format)) return "format must be LSQ_BASE_F16 or LSQ_BASE_BF16";
    if (n < 0) return "n < 0";
    if (d < 1) return "d < 1";
    if (lds < d) return "lds < d";
    if (ldd < d) return "ldd < d";
    if (n > 0 && (!dst || !src)) return "null pointer";
    if (((uintptr_t)dst & 1) != 0) return "dst is not 2-byte aligned";
    if (((uintptr_t)src & 3) != 0) return "src is not 4-byte aligned";
    return nullptr;
}
// lsq_index_narrow_base: has_base / base_format describe the index
inline const char *lsq_narrow_base_refusal(bool has_base, int base_format, int format) {
    if (!has_base) return "the index holds no base rows";
    if (base_format != 0) return "the base rows are not f32";
    if (!lsq_base_is_half(format)) return "format must be LSQ_BASE_F16 or LSQ_BASE_BF16";
    return nullptr;
}
// lsq_index_get_base: rows [start, start + count) of an index of n rows of d components
inline const char *lsq_get_base_refusal(bool has_base, int64_t n, int d, int64_t start, int64_t count, int64_t ldo, const void *out) {
    if (!has_base) return "the index holds no base rows";
    if (count < 0) return "count < 0";
    if (start < 0 || start > n || count > n - start) return "the range [start, start + count) leaves the index";
    if (ldo < d) return "ldo < d";
    if (count > 0 && !out) return "null pointer";
    if (((uintptr_t)out & 3) != 0) return "out is not 4-byte aligned";
    return nullptr;
}

// rows per staging chunk of a host-buffer lsq_index_get_base (lsq_index_reconstruct's rule): as many as keep the staged f32 rows at or below `budget` bytes,
// never fewer than one, never more than count; `option` > 0 (option "recon_chunk", a test hook) only makes chunks smaller.  d >= 1
constexpr int64_t LSQ_BASE_STAGE_BYTES = 64ll << 20;
inline int64_t lsq_base_chunk_rows(int64_t count, int d, int64_t option, int64_t budget = LSQ_BASE_STAGE_BYTES) {
    int64_t rows = budget / ((int64_t)sizeof(float) * (int64_t)d);
    if (rows < 1) rows = 1;
    if (option > 0 && option < rows) rows = option;
    if (rows > count) rows = count;
    return rows < 1 ? 1 : rows;
}
inline int64_t lsq_base_chunks(int64_t count, int64_t rows) { return count < 1 ? 0 : (count + rows - 1) / rows; }

// ---- lsq_narrow_rows_cpu's body: dst row i (ldd halves apart) = narrow(src row i, lds floats apart), d components; nothing else of dst is written ------
inline void lsq_narrow_rows_range(uint16_t *dst, const float *src, int64_t r0, int64_t r1, int d, int64_t lds, int64_t ldd, int format,
                                  lsq_narrow_counts *counts) {
    for (int64_t i = r0; i < r1; ++i) {
        const float *s = src + i * lds;
        uint16_t *o = dst + i * ldd;
        for (int t = 0; t < d; ++t) {
            o[t] = lsq_narrow_half(s[t], format);
            if (counts) lsq_narrow_count(s[t], o[t], format, counts);
        }
    }
}

inline const char *lsq_narrow_rows_host(void *dst, const float *src, int64_t n, int d, int64_t lds, int64_t ldd, int format, int nthreads,
                                        lsq_narrow_counts *counts = nullptr) {
    if (counts) *counts = lsq_narrow_counts{};
    if (const char *why = lsq_narrow_rows_refusal(dst, src, n, d, lds, ldd, format)) return why;
    if (n == 0) return nullptr;
    int nt = nthreads > 0 ? nthreads : (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if ((int64_t)nt > n) nt = (int)n;
    if ((int64_t)n * d < (1 << 16)) nt = 1;                           // not worth a thread
    uint16_t *o = static_cast<uint16_t *>(dst);
    if (nt == 1) { lsq_narrow_rows_range(o, src, 0, n, d, lds, ldd, format, counts); return nullptr; }
    std::vector<lsq_narrow_counts> part((size_t)nt);
    std::vector<std::thread> pool;
    pool.reserve((size_t)nt);
    for (int t = 0; t < nt; ++t)
        pool.emplace_back(lsq_narrow_rows_range, o, src, n * t / nt, n * (t + 1) / nt, d, lds, ldd, format, counts ? &part[(size_t)t] : nullptr);
    for (auto &th : pool) th.join();
    if (counts)
        for (const lsq_narrow_counts &p : part) { counts->to_inf += p.to_inf; counts->to_zero += p.to_zero; counts->nans += p.nans; }
    return nullptr;
}
