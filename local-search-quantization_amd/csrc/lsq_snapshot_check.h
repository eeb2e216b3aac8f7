// lsq_snapshot_check.h -- the parts of the snapshots that need no device: the digest, the header and section-table layout, the plan of a file
// from its scalars with overflow-checked sizes, the validation of a header and table, and the host-only writer / reader / inspector behind
// lsq_snapshot_write_cpu / _read_cpu / _inspect_cpu.  Plain C++ over the public header alone, so that a stand-alone host program can exercise them
// (tools/snapshot_check_main.cpp).  The reference has no counterpart.
//
// THE DIGEST (pinned in three places that agree bit for bit: include/lsq_mi355x.h (3p), lsq_snap_digest here, tests/snapshot_check.py):
//   range digest = SUM_i (uint64) fmix32(w_i ^ (uint32)(i * 0x9E3779B1)) * (uint64)(uint32)(2 i + 1)  +  bytes * 0x9E3779B97F4A7C15   (mod 2^64)
//   over the range's little-endian 32-bit words w_i, i counted from the section's first word, the last word zero-padded
#pragma once

#include <errno.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/lsq_mi355x.h"

constexpr uint32_t LSQ_SNAP_GOLD32 = 0x9E3779B1u;
constexpr uint64_t LSQ_SNAP_GOLD64 = 0x9E3779B97F4A7C15ull;
constexpr int64_t LSQ_SNAP_HEADER_BYTES = 128, LSQ_SNAP_ENTRY_BYTES = 32, LSQ_SNAP_ALIGN = 64;
constexpr uint32_t LSQ_SNAP_ENDIAN = 0x01020304u;
constexpr int64_t LSQ_SNAP_CHUNK_DEFAULT = 8ll << 20;         // measured: profiles/snapshot.jsonl
inline constexpr char LSQ_SNAP_MAGIC[8] = {'L', 'S', 'Q', 'S', 'N', 'A', 'P', '\0'};

#if defined(__HIPCC__)
#define LSQ_SNAP_HD __host__ __device__
#else
#define LSQ_SNAP_HD
#endif

LSQ_SNAP_HD inline uint32_t lsq_snap_fmix32(uint32_t x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}
// the term of word w at position i of its section
LSQ_SNAP_HD inline uint64_t lsq_snap_term(uint32_t w, uint64_t i) {
    return (uint64_t)lsq_snap_fmix32(w ^ ((uint32_t)i * LSQ_SNAP_GOLD32)) * (uint64_t)(uint32_t)(2u * (uint32_t)i + 1u);
}
// the digest of `bytes` bytes at `data` (any alignment) whose first byte is byte 0 of word first_word of the section
inline uint64_t lsq_snap_digest(const void *data, uint64_t bytes, uint64_t first_word) {
    const unsigned char *p = static_cast<const unsigned char *>(data);
    uint64_t sum = bytes * LSQ_SNAP_GOLD64, i = first_word;
    uint64_t k = 0;
    for (; k + 4 <= bytes; k += 4, ++i) {
        const uint32_t w = (uint32_t)p[k] | ((uint32_t)p[k + 1] << 8) | ((uint32_t)p[k + 2] << 16) | ((uint32_t)p[k + 3] << 24);
        sum += lsq_snap_term(w, i);
    }
    if (k < bytes) {
        uint32_t w = 0;
        for (int b = 0; k + (uint64_t)b < bytes; ++b) w |= (uint32_t)p[k + (uint64_t)b] << (8 * b);
        sum += lsq_snap_term(w, i);
    }
    return sum;
}

inline const char *lsq_snap_kind_name(int64_t kind) {
    static const char *names[] = {"?", "CODEBOOKS", "CODES", "DBNORMS", "NORM_CODES", "CBNORMS", "BASE", "CENTROIDS", "LIST_OF_ROW", "FILTER_BITS"};
    return kind >= 1 && kind <= LSQ_SNAP_MAX_SECTIONS ? names[kind] : names[0];
}

// ---- little-endian fields, whatever the host ------------------------------------------------------------------------------------------------------
inline void lsq_snap_put32(unsigned char *p, uint32_t v) { for (int b = 0; b < 4; ++b) p[b] = (unsigned char)(v >> (8 * b)); }
inline void lsq_snap_put64(unsigned char *p, uint64_t v) { for (int b = 0; b < 8; ++b) p[b] = (unsigned char)(v >> (8 * b)); }
inline uint32_t lsq_snap_get32(const unsigned char *p) { uint32_t v = 0; for (int b = 0; b < 4; ++b) v |= (uint32_t)p[b] << (8 * b); return v; }
inline uint64_t lsq_snap_get64(const unsigned char *p) { uint64_t v = 0; for (int b = 0; b < 8; ++b) v |= (uint64_t)p[b] << (8 * b); return v; }

// ---- overflow-checked sizes: false when the product or sum leaves [0, INT64_MAX] ------------------------------------------------------------------
inline bool lsq_snap_mul(int64_t a, int64_t b, int64_t *out) { return a >= 0 && b >= 0 && !__builtin_mul_overflow(a, b, out); }
inline bool lsq_snap_add(int64_t a, int64_t b, int64_t *out) { return a >= 0 && b >= 0 && !__builtin_add_overflow(a, b, out); }
inline bool lsq_snap_align(int64_t a, int64_t *out) {
    int64_t t;
    if (!lsq_snap_add(a, LSQ_SNAP_ALIGN - 1, &t)) return false;
    *out = t / LSQ_SNAP_ALIGN * LSQ_SNAP_ALIGN;
    return true;
}

struct lsq_snap_error {
    char text[256];
    lsq_snap_error() { text[0] = 0; }
    void set(const char *fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(text, sizeof(text), fmt, ap);
        va_end(ap);
    }
};

inline int lsq_snap_base_elem(int64_t format) { return format == 0 ? 4 : (format == LSQ_BASE_F16 || format == LSQ_BASE_BF16) ? 2 : 1; }

// ---- the plan: scalars -> sections (kind, element bytes, offset, bytes) and the file's length.  info's scalars are read, its table and file_bytes
// written.  false (err set): scalars out of range or inconsistent, or a size that overflows ----------------------------------------------------------
inline bool lsq_snap_plan(lsq_snapshot_info *s, lsq_snap_error *err) {
    if (s->n < 1 || s->n > (int64_t)INT32_MAX - 1) { err->set("n = %lld lies outside 1 .. 2^31 - 2", (long long)s->n); return false; }
    if (s->d < 1 || s->d > INT32_MAX) { err->set("d = %lld lies outside 1 .. 2^31 - 1", (long long)s->d); return false; }
    if (s->has_codes != 0 && s->has_codes != 1) { err->set("the codes flag is %lld", (long long)s->has_codes); return false; }
    if (s->has_base != 0 && s->has_base != 1) { err->set("the base flag is %lld", (long long)s->has_base); return false; }
    if (!s->has_codes && !s->has_base) { err->set("neither codes nor base rows"); return false; }
    if (s->has_codes ? (s->m < 1 || s->m > 16 || s->h != 256) : (s->m != 0 || s->h != 0)) {
        err->set("m = %lld, h = %lld do not fit an index %s codes", (long long)s->m, (long long)s->h, s->has_codes ? "with" : "without");
        return false;
    }
    if (s->packed != 0 && s->packed != 1) { err->set("packed = %lld", (long long)s->packed); return false; }
    if (s->packed ? (!s->has_codes || s->ncb < 1 || s->ncb > 256) : s->ncb != 0) { err->set("packed = %lld with ncb = %lld", (long long)s->packed, (long long)s->ncb); return false; }
    if (s->has_base ? (s->base_format < 0 || s->base_format > 3) : s->base_format != 0) { err->set("base format %lld", (long long)s->base_format); return false; }
    if (s->nlist < 0 || s->nlist > (1 << 24) || (s->nlist > 0 && !s->has_codes)) { err->set("nlist = %lld", (long long)s->nlist); return false; }
    if (s->filter_active != 0 && s->filter_active != 1) { err->set("the filter flag is %lld", (long long)s->filter_active); return false; }
    if (s->filter_active ? (s->filter_force != 0 && s->filter_force != LSQ_FILTER_FORCE_DENSE && s->filter_force != LSQ_FILTER_FORCE_COMPACT) : s->filter_force != 0) {
        err->set("the filter's FORCE flag is %lld", (long long)s->filter_force);
        return false;
    }
    if (s->filter_active ? (s->allowed < 0 || s->allowed > s->n) : s->allowed != 0) { err->set("allowed = %lld of n = %lld", (long long)s->allowed, (long long)s->n); return false; }
    int ns = 0;
    bool ok = true;
    auto section = [&](int64_t kind, int64_t elem, int64_t a, int64_t b) {
        int64_t count = 0, bytes = 0;
        if (!lsq_snap_mul(a, b, &count) || !lsq_snap_mul(count, elem, &bytes)) {
            if (ok) err->set("section %s: %lld x %lld elements of %lld bytes overflow 64 bits", lsq_snap_kind_name(kind), (long long)a, (long long)b, (long long)elem);
            ok = false;
            return;
        }
        s->sections[ns].kind = kind; s->sections[ns].elem_bytes = elem; s->sections[ns].bytes = bytes; s->sections[ns].offset = 0;
        ++ns;
    };
    if (s->has_codes) {
        section(LSQ_SNAP_CODEBOOKS, 4, s->m * 256, s->d);
        section(LSQ_SNAP_CODES, 1, s->n, s->m);
        if (!s->packed) section(LSQ_SNAP_DBNORMS, 4, s->n, 1);
        else { section(LSQ_SNAP_NORM_CODES, 1, s->n, 1); section(LSQ_SNAP_CBNORMS, 4, s->ncb, 1); }
    }
    if (s->has_base) section(LSQ_SNAP_BASE, lsq_snap_base_elem(s->base_format), s->n, s->d);
    if (s->nlist > 0) { section(LSQ_SNAP_CENTROIDS, 4, s->nlist, s->d); section(LSQ_SNAP_LIST_OF_ROW, 4, s->n, 1); }
    if (s->filter_active) section(LSQ_SNAP_FILTER_BITS, 4, (s->n + 31) / 32, 1);
    if (!ok) return false;
    s->nsections = ns;
    int64_t end = LSQ_SNAP_HEADER_BYTES + LSQ_SNAP_ENTRY_BYTES * ns + 8;
    for (int k = 0; k < ns; ++k) {
        int64_t off = 0;
        if (!lsq_snap_align(end, &off) || !lsq_snap_add(off, s->sections[k].bytes, &end)) {
            err->set("section %s: its end overflows 64 bits", lsq_snap_kind_name(s->sections[k].kind));
            return false;
        }
        s->sections[k].offset = off;
    }
    s->file_bytes = end;
    s->format = LSQ_SNAPSHOT_FORMAT;
    return true;
}
inline int64_t lsq_snap_table_end(int64_t nsections) { return LSQ_SNAP_HEADER_BYTES + LSQ_SNAP_ENTRY_BYTES * nsections + 8; }

// ---- the header and table as bytes: lsq_snap_table_end(nsections) of them; the sections' digests are read from info, header_digest is written ----------
inline void lsq_snap_encode(lsq_snapshot_info *s, std::vector<unsigned char> *out) {
    const int64_t len = lsq_snap_table_end(s->nsections);
    out->assign((size_t)len, 0);
    unsigned char *p = out->data();
    memcpy(p, LSQ_SNAP_MAGIC, 8);
    lsq_snap_put32(p + 8, LSQ_SNAPSHOT_FORMAT); lsq_snap_put32(p + 12, LSQ_SNAP_ENDIAN); lsq_snap_put32(p + 16, (uint32_t)LSQ_SNAP_HEADER_BYTES);
    lsq_snap_put32(p + 20, (uint32_t)s->nsections); lsq_snap_put64(p + 24, (uint64_t)s->n);
    lsq_snap_put32(p + 32, (uint32_t)s->d); lsq_snap_put32(p + 36, (uint32_t)s->m); lsq_snap_put32(p + 40, (uint32_t)s->h); lsq_snap_put32(p + 44, (uint32_t)s->packed);
    lsq_snap_put32(p + 48, (uint32_t)s->ncb); lsq_snap_put32(p + 52, (uint32_t)s->base_format); lsq_snap_put32(p + 56, (uint32_t)s->nlist);
    lsq_snap_put32(p + 60, (uint32_t)((s->has_codes ? 1 : 0) | (s->has_base ? 2 : 0) | (s->filter_active ? 4 : 0)));
    lsq_snap_put32(p + 64, (uint32_t)s->filter_force);
    lsq_snap_put64(p + 72, (uint64_t)s->allowed); lsq_snap_put64(p + 80, (uint64_t)s->file_bytes);
    for (int k = 0; k < (int)s->nsections; ++k) {
        unsigned char *e = p + LSQ_SNAP_HEADER_BYTES + LSQ_SNAP_ENTRY_BYTES * k;
        lsq_snap_put32(e, (uint32_t)s->sections[k].kind); lsq_snap_put32(e + 4, (uint32_t)s->sections[k].elem_bytes);
        lsq_snap_put64(e + 8, (uint64_t)s->sections[k].offset); lsq_snap_put64(e + 16, (uint64_t)s->sections[k].bytes); lsq_snap_put64(e + 24, s->sections[k].digest);
    }
    s->header_digest = lsq_snap_digest(p, (uint64_t)(len - 8), 0);
    lsq_snap_put64(p + len - 8, s->header_digest);
}

// ---- validation of the first `have` bytes of a file of `file_size` bytes.  LSQ_OK: *s holds scalars and table.  Nothing is allocated -------------------
// (the caller reads LSQ_SNAP_HEADER_BYTES first, asks lsq_snap_header_sections for the table's length, reads on, and then calls this)
inline int lsq_snap_header_sections(const unsigned char *p, int64_t have, int64_t *nsections, lsq_snap_error *err) {
    if (have < LSQ_SNAP_HEADER_BYTES) { err->set("truncated: %lld bytes are no header", (long long)have); return LSQ_EFORMAT; }
    if (memcmp(p, LSQ_SNAP_MAGIC, 8) != 0) { err->set("not a snapshot: wrong magic"); return LSQ_EFORMAT; }
    const uint32_t endian = lsq_snap_get32(p + 12);
    if (endian == 0x04030201u) { err->set("a big-endian snapshot: no reader for it"); return LSQ_EFORMAT; }
    if (endian != LSQ_SNAP_ENDIAN) { err->set("the endianness marker is 0x%08x", endian); return LSQ_EFORMAT; }
    const uint32_t version = lsq_snap_get32(p + 8);
    if (version > LSQ_SNAPSHOT_FORMAT) { err->set("format version %u is newer than this library's %d", version, LSQ_SNAPSHOT_FORMAT); return LSQ_EFORMAT; }
    if (version < 1) { err->set("format version %u", version); return LSQ_EFORMAT; }
    if (lsq_snap_get32(p + 16) != (uint32_t)LSQ_SNAP_HEADER_BYTES) { err->set("the header length is %u, not %lld", lsq_snap_get32(p + 16), (long long)LSQ_SNAP_HEADER_BYTES); return LSQ_EFORMAT; }
    const uint32_t ns = lsq_snap_get32(p + 20);
    if (ns < 1 || ns > LSQ_SNAP_MAX_SECTIONS) { err->set("%u sections", ns); return LSQ_EFORMAT; }
    *nsections = ns;
    return LSQ_OK;
}
inline int lsq_snap_validate(const unsigned char *p, int64_t have, int64_t file_size, lsq_snapshot_info *s, lsq_snap_error *err) {
    int64_t ns = 0;
    if (int rc = lsq_snap_header_sections(p, have, &ns, err)) return rc;
    const int64_t len = lsq_snap_table_end(ns);
    if (have < len || file_size < len) { err->set("truncated: the section table ends at byte %lld of %lld", (long long)len, (long long)(have < file_size ? have : file_size)); return LSQ_EFORMAT; }
    *s = lsq_snapshot_info{};
    s->n = (int64_t)lsq_snap_get64(p + 24);
    s->d = (int32_t)lsq_snap_get32(p + 32); s->m = (int32_t)lsq_snap_get32(p + 36); s->h = (int32_t)lsq_snap_get32(p + 40); s->packed = (int32_t)lsq_snap_get32(p + 44);
    s->ncb = (int32_t)lsq_snap_get32(p + 48); s->base_format = (int32_t)lsq_snap_get32(p + 52); s->nlist = (int32_t)lsq_snap_get32(p + 56);
    const uint32_t flags = lsq_snap_get32(p + 60);
    if (flags > 7) { err->set("header flags 0x%x", flags); return LSQ_EFORMAT; }
    s->has_codes = flags & 1; s->has_base = (flags >> 1) & 1; s->filter_active = (flags >> 2) & 1;
    s->filter_force = (int32_t)lsq_snap_get32(p + 64);
    s->allowed = (int64_t)lsq_snap_get64(p + 72);
    const int64_t file_bytes = (int64_t)lsq_snap_get64(p + 80);
    if (lsq_snap_get32(p + 68) != 0) { err->set("a reserved header field is not zero"); return LSQ_EFORMAT; }
    for (int64_t k = 88; k < LSQ_SNAP_HEADER_BYTES; ++k)
        if (p[k]) { err->set("a reserved header byte is not zero"); return LSQ_EFORMAT; }
    const uint64_t hd = lsq_snap_digest(p, (uint64_t)(len - 8), 0), stored = lsq_snap_get64(p + len - 8);
    if (!lsq_snap_plan(s, err)) {                      // what the scalars demand (sizes overflow-checked), before the table is believed
        lsq_snap_error why = *err;
        err->set("inconsistent header: %s", why.text);
        return LSQ_EFORMAT;
    }
    if (file_size < file_bytes) { err->set("truncated: the file holds %lld bytes, the header says %lld", (long long)file_size, (long long)file_bytes); return LSQ_EFORMAT; }
    if (s->nsections != ns) { err->set("the header's scalars demand %lld sections, the table has %lld", (long long)s->nsections, (long long)ns); return LSQ_EFORMAT; }
    int64_t prev_end = len;
    for (int k = 0; k < (int)ns; ++k) {
        const unsigned char *e = p + LSQ_SNAP_HEADER_BYTES + LSQ_SNAP_ENTRY_BYTES * k;
        const int64_t kind = lsq_snap_get32(e), elem = lsq_snap_get32(e + 4), off = (int64_t)lsq_snap_get64(e + 8), bytes = (int64_t)lsq_snap_get64(e + 16);
        const lsq_snapshot_section &want = s->sections[k];
        const char *name = lsq_snap_kind_name(want.kind);
        if (kind != want.kind) { err->set("section %d is of kind %lld (%s), the header's scalars demand %s there", k, (long long)kind, lsq_snap_kind_name(kind), name); return LSQ_EFORMAT; }
        if (elem != want.elem_bytes) { err->set("section %s: elements of %lld bytes, not %lld", name, (long long)elem, (long long)want.elem_bytes); return LSQ_EFORMAT; }
        if (bytes != want.bytes) { err->set("section %s: %lld bytes are inconsistent with n, d, m (%lld)", name, (long long)bytes, (long long)want.bytes); return LSQ_EFORMAT; }
        if (off < 0 || off % LSQ_SNAP_ALIGN != 0) { err->set("section %s: offset %lld is not a multiple of %lld", name, (long long)off, (long long)LSQ_SNAP_ALIGN); return LSQ_EFORMAT; }
        if (off < prev_end) { err->set("section %s: offset %lld overlaps what ends at %lld", name, (long long)off, (long long)prev_end); return LSQ_EFORMAT; }
        int64_t end = 0;
        if (!lsq_snap_add(off, bytes, &end) || end > file_size) { err->set("section %s: it ends past the end of the file (%lld bytes)", name, (long long)file_size); return LSQ_EFORMAT; }
        if (off != want.offset) { err->set("section %s: offset %lld is not the canonical %lld", name, (long long)off, (long long)want.offset); return LSQ_EFORMAT; }
        s->sections[k].digest = lsq_snap_get64(e + 24);
        prev_end = end;
    }
    if (hd != stored) { err->set("the header's digest does not match its bytes"); return LSQ_EFORMAT; }
    if (file_bytes != s->file_bytes) { err->set("the header says %lld bytes, its sections end at %lld", (long long)file_bytes, (long long)s->file_bytes); return LSQ_EFORMAT; }
    if (file_size != s->file_bytes) { err->set("%s: the file holds %lld bytes, the header says %lld", file_size < s->file_bytes ? "truncated" : "trailing bytes", (long long)file_size, (long long)s->file_bytes); return LSQ_EFORMAT; }
    s->header_digest = stored;
    return LSQ_OK;
}

// ---- scalars of a description -> info (the writer's and the exporter's first step) ------------------------------------------------------------------
inline void lsq_snap_scalars(const lsq_snapshot_arrays *a, bool has_codes, bool has_base, lsq_snapshot_info *s) {
    *s = lsq_snapshot_info{};
    s->n = a->n; s->d = a->d; s->m = has_codes ? a->m : 0; s->h = has_codes ? a->h : 0; s->packed = a->packed ? 1 : 0; s->ncb = a->packed ? a->ncb : 0;
    s->base_format = has_base ? a->base_format : 0; s->nlist = a->nlist; s->has_codes = has_codes; s->has_base = has_base;
    s->filter_active = a->filter_active ? 1 : 0; s->filter_force = a->filter_active ? a->filter_force : 0; s->allowed = a->filter_active ? a->allowed : 0;
}
inline void *lsq_snap_array(const lsq_snapshot_arrays *a, int64_t kind) {
    switch (kind) {
    case LSQ_SNAP_CODEBOOKS: return a->codebooks;
    case LSQ_SNAP_CODES: return a->codes;
    case LSQ_SNAP_DBNORMS: return a->dbnorms;
    case LSQ_SNAP_NORM_CODES: return a->norm_codes;
    case LSQ_SNAP_CBNORMS: return a->cbnorms;
    case LSQ_SNAP_BASE: return a->base;
    case LSQ_SNAP_CENTROIDS: return a->centroids;
    case LSQ_SNAP_LIST_OF_ROW: return a->list_of_row;
    case LSQ_SNAP_FILTER_BITS: return a->filter_bits;
    }
    return nullptr;
}
inline void lsq_snap_scalars_out(const lsq_snapshot_info *s, lsq_snapshot_arrays *a) {
    a->n = s->n; a->d = (int)s->d; a->m = (int)s->m; a->h = (int)s->h; a->packed = (int)s->packed; a->ncb = (int)s->ncb; a->base_format = (int)s->base_format;
    a->nlist = (int)s->nlist; a->filter_active = (int)s->filter_active; a->filter_force = (int)s->filter_force; a->reserved = 0; a->allowed = s->allowed;
}

// a FILE that closes itself, and a temporary that removes itself unless it was renamed into place
struct lsq_snap_file {
    FILE *f = nullptr;
    ~lsq_snap_file() { if (f) fclose(f); }
    int close() { const int rc = f ? fclose(f) : 0; f = nullptr; return rc; }
};
struct lsq_snap_temp {
    std::string tmp, path;
    bool made = false, done = false;                  // made: this call created the temporary (what stood there before is not this call's to remove)
    explicit lsq_snap_temp(const char *target) : tmp(std::string(target) + ".tmp-snapshot"), path(target) {}
    ~lsq_snap_temp() { if (made && !done) (void)remove(tmp.c_str()); }
    bool commit() { done = rename(tmp.c_str(), path.c_str()) == 0; return done; }
};
inline int64_t lsq_snap_file_size(FILE *f) {
    if (fseeko(f, 0, SEEK_END) != 0) return -1;
    const int64_t size = (int64_t)ftello(f);
    if (fseeko(f, 0, SEEK_SET) != 0) return -1;
    return size;
}
// zero bytes up to `to` (a section's offset) -- written, or read and checked
inline bool lsq_snap_write_pad(FILE *f, int64_t at, int64_t to) {
    static const unsigned char zero[LSQ_SNAP_ALIGN] = {0};
    return to == at || fwrite(zero, 1, (size_t)(to - at), f) == (size_t)(to - at);
}
inline int lsq_snap_read_pad(FILE *f, int64_t at, int64_t to, const char *before, lsq_snap_error *err) {
    unsigned char pad[LSQ_SNAP_ALIGN];
    if (to - at < 0 || to - at >= LSQ_SNAP_ALIGN) { err->set("the padding before section %s is %lld bytes", before, (long long)(to - at)); return LSQ_EFORMAT; }
    if (to == at) return LSQ_OK;
    if (fread(pad, 1, (size_t)(to - at), f) != (size_t)(to - at)) { err->set("read failed in the padding before section %s", before); return LSQ_EIO; }
    for (int64_t k = 0; k < to - at; ++k)
        if (pad[k]) { err->set("non-zero padding before section %s (byte %lld of the file)", before, (long long)(at + k)); return LSQ_EFORMAT; }
    return LSQ_OK;
}
// header and table of an open file: read, validated; the file is left at lsq_snap_table_end(nsections)
inline int lsq_snap_read_header(FILE *f, lsq_snapshot_info *s, lsq_snap_error *err) {
    const int64_t size = lsq_snap_file_size(f);
    if (size < 0) { err->set("cannot seek: %s", strerror(errno)); return LSQ_EIO; }
    unsigned char buf[LSQ_SNAP_HEADER_BYTES + LSQ_SNAP_ENTRY_BYTES * LSQ_SNAP_MAX_SECTIONS + 8];
    int64_t have = (int64_t)fread(buf, 1, (size_t)LSQ_SNAP_HEADER_BYTES, f), ns = 0;
    if (int rc = lsq_snap_header_sections(buf, have, &ns, err)) return rc;
    const int64_t rest = lsq_snap_table_end(ns) - LSQ_SNAP_HEADER_BYTES;
    have += (int64_t)fread(buf + LSQ_SNAP_HEADER_BYTES, 1, (size_t)rest, f);
    return lsq_snap_validate(buf, have, size, s, err);
}

// ---- the host-only writer: arrays -> file.  Bits of FILTER_BITS at or past n are written as zero and `allowed` is recounted ------------------------------
inline int lsq_snap_write_file(const char *path, const lsq_snapshot_arrays *a, lsq_snap_error *err) {
    if (!path || !a) { err->set("null argument"); return LSQ_EINVAL; }
    lsq_snapshot_info s;
    const bool has_codes = a->codes != nullptr, has_base = a->base != nullptr;
    lsq_snap_scalars(a, has_codes, has_base, &s);
    std::vector<uint32_t> bits;
    if (s.filter_active && a->filter_bits && a->n >= 1 && a->n <= (int64_t)INT32_MAX - 1) {
        const int64_t words = (a->n + 31) / 32;
        bits.resize((size_t)words);
        memcpy(bits.data(), a->filter_bits, (size_t)words * 4);
        if (a->n % 32) bits[(size_t)words - 1] &= (1u << (a->n % 32)) - 1u;
        int64_t allowed = 0;
        for (uint32_t w : bits) allowed += __builtin_popcount(w);
        s.allowed = allowed;
    }
    if (!lsq_snap_plan(&s, err)) return LSQ_EINVAL;
    for (int k = 0; k < (int)s.nsections; ++k)
        if (!lsq_snap_array(a, s.sections[k].kind)) { err->set("section %s: null pointer", lsq_snap_kind_name(s.sections[k].kind)); return LSQ_EINVAL; }
    for (int k = 0; k < (int)s.nsections; ++k) {
        const void *src = s.sections[k].kind == LSQ_SNAP_FILTER_BITS ? bits.data() : lsq_snap_array(a, s.sections[k].kind);
        s.sections[k].digest = lsq_snap_digest(src, (uint64_t)s.sections[k].bytes, 0);
    }
    std::vector<unsigned char> head;
    lsq_snap_encode(&s, &head);
    lsq_snap_temp temp(path);
    lsq_snap_file out;
    out.f = fopen(temp.tmp.c_str(), "wb");
    if (!out.f) { err->set("cannot open %s: %s", temp.tmp.c_str(), strerror(errno)); return LSQ_EIO; }
    temp.made = true;
    bool ok = fwrite(head.data(), 1, head.size(), out.f) == head.size();
    int64_t at = (int64_t)head.size();
    for (int k = 0; ok && k < (int)s.nsections; ++k) {
        const void *src = s.sections[k].kind == LSQ_SNAP_FILTER_BITS ? bits.data() : lsq_snap_array(a, s.sections[k].kind);
        ok = lsq_snap_write_pad(out.f, at, s.sections[k].offset) && fwrite(src, 1, (size_t)s.sections[k].bytes, out.f) == (size_t)s.sections[k].bytes;
        at = s.sections[k].offset + s.sections[k].bytes;
    }
    if (!ok) { err->set("short write to %s: %s", temp.tmp.c_str(), strerror(errno)); return LSQ_EIO; }
    if (out.close() != 0) { err->set("cannot close %s: %s", temp.tmp.c_str(), strerror(errno)); return LSQ_EIO; }
    if (!temp.commit()) { err->set("cannot rename %s to %s: %s", temp.tmp.c_str(), path, strerror(errno)); return LSQ_EIO; }
    return LSQ_OK;
}

// ---- the host-only inspector and reader.  verify: every section's digest and every padding byte.  arrays (optional): the non-null ones are filled, through
// a bounce buffer of 1 MiB (a failed read leaves them partly written; their digests are verified whatever `verify` says) ---------------------------------
inline int lsq_snap_read_file(const char *path, lsq_snapshot_info *info, int verify, lsq_snapshot_arrays *arrays, lsq_snap_error *err) {
    if (!path || !info) { err->set("null argument"); return LSQ_EINVAL; }
    *info = lsq_snapshot_info{};
    lsq_snap_file in;
    in.f = fopen(path, "rb");
    if (!in.f) { err->set("cannot open %s: %s", path, strerror(errno)); return LSQ_EIO; }
    lsq_snapshot_info s;
    if (int rc = lsq_snap_read_header(in.f, &s, err)) return rc;
    if (arrays) {
        lsq_snapshot_arrays want = *arrays;
        for (int64_t kind = 1; kind <= LSQ_SNAP_MAX_SECTIONS; ++kind) {
            bool present = false;
            for (int k = 0; k < (int)s.nsections; ++k) present = present || s.sections[k].kind == kind;
            if (lsq_snap_array(&want, kind) && !present) { err->set("section %s is requested and the file has none", lsq_snap_kind_name(kind)); return LSQ_EINVAL; }
        }
    }
    if (verify || arrays) {
        std::vector<unsigned char> bounce((size_t)1 << 20);
        int64_t at = lsq_snap_table_end(s.nsections);
        for (int k = 0; k < (int)s.nsections; ++k) {
            const lsq_snapshot_section &sec = s.sections[k];
            const char *name = lsq_snap_kind_name(sec.kind);
            if (int rc = lsq_snap_read_pad(in.f, at, sec.offset, name, err)) return rc;
            unsigned char *dst = arrays ? static_cast<unsigned char *>(lsq_snap_array(arrays, sec.kind)) : nullptr;
            uint64_t digest = 0;
            for (int64_t off = 0; off < sec.bytes; off += (int64_t)bounce.size()) {
                const size_t len = (size_t)(sec.bytes - off < (int64_t)bounce.size() ? sec.bytes - off : (int64_t)bounce.size());
                if (fread(bounce.data(), 1, len, in.f) != len) { err->set("section %s: read failed at byte %lld", name, (long long)off); return LSQ_EIO; }
                digest += lsq_snap_digest(bounce.data(), len, (uint64_t)off / 4);
                if (dst) memcpy(dst + off, bounce.data(), len);
            }
            if (sec.bytes == 0) digest = 0;
            if (digest != sec.digest) { err->set("section %s: digest mismatch (the table says %016llx, the bytes give %016llx)", name, (unsigned long long)sec.digest, (unsigned long long)digest); return LSQ_EFORMAT; }
            at = sec.offset + sec.bytes;
        }
    }
    *info = s;
    if (arrays) lsq_snap_scalars_out(&s, arrays);
    return LSQ_OK;
}
