// snapshot_check_main.cpp -- a stand-alone host program over csrc/lsq_snapshot_check.h: the digest (pinned values, additivity over every split, the position and
// length terms), the overflow-checked plan of a file, and the host-only writer / reader on a snapshot of under 4 KiB -- EVERY PREFIX LENGTH of the file and EVERY
// SINGLE-BYTE CHANGE of its header and section table must come back as an error code, never as a crash, a hang or a read outside a buffer.  None of it needs a
// device.  Built with the host compiler alone, usually under -fsanitize=address,undefined (tests/test_snapshot.py does that where the compiler has the runtimes).
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/snapshot_check_main.cpp -o snapshot_check && ./snapshot_check DIR
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "../local-search-quantization_amd/csrc/lsq_snapshot_check.h"

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

// a small generator: the program must not depend on the C library's rand
static uint32_t next(uint64_t *s) { *s = *s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(*s >> 32); }

static bool put_file(const std::string &path, const unsigned char *p, size_t len) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(p, 1, len, f) == len;
    return fclose(f) == 0 && ok;
}

// the arrays of the program's one index, exactly sized (a write past any of them is the sanitizer's to find)
struct State {
    int64_t n = 33;
    int d = 1, m = 1, nlist = 3;
    std::vector<float> K, dbn, cent;
    std::vector<uint8_t> codes;
    std::vector<uint16_t> base;
    std::vector<int32_t> lor;
    std::vector<uint32_t> bits;
    State() : K(256), dbn(33), cent(3), codes(33), base(33), lor(33), bits(2) {
        uint64_t s = 7;
        for (float &x : K) x = (float)next(&s) / 65536.0f;
        for (float &x : dbn) x = (float)next(&s) / 1024.0f;
        for (float &x : cent) x = (float)next(&s);
        for (uint8_t &x : codes) x = (uint8_t)next(&s);
        for (uint16_t &x : base) x = (uint16_t)next(&s);
        for (int32_t &x : lor) x = (int32_t)(next(&s) % 3u);
        bits[0] = next(&s); bits[1] = 1u;
    }
    lsq_snapshot_arrays arrays() {
        lsq_snapshot_arrays a{};
        a.n = n; a.d = d; a.m = m; a.h = 256; a.base_format = LSQ_BASE_F16; a.nlist = nlist; a.filter_active = 1; a.filter_force = LSQ_FILTER_FORCE_COMPACT;
        a.codebooks = K.data(); a.codes = codes.data(); a.dbnorms = dbn.data(); a.base = base.data(); a.centroids = cent.data(); a.list_of_row = lor.data();
        a.filter_bits = bits.data();
        return a;
    }
};

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    lsq_snap_error err;

    // ---- the digest: pinned values, the length term, the position term, additivity over every split at a multiple of 4
    EXPECT(lsq_snap_fmix32(0) == 0 && lsq_snap_fmix32(1) == 0x514E28B7u);
    EXPECT(lsq_snap_digest(nullptr, 0, 0) == 0 && lsq_snap_digest(nullptr, 0, 99) == 0);
    const unsigned char zero4[4] = {0, 0, 0, 0}, one[1] = {1}, one4[4] = {1, 0, 0, 0};
    EXPECT(lsq_snap_digest(zero4, 4, 0) == 4 * LSQ_SNAP_GOLD64);                          // fmix32(0 ^ 0) = 0: the length alone
    EXPECT(lsq_snap_digest(one, 1, 0) == (uint64_t)0x514E28B7u + LSQ_SNAP_GOLD64);         // the zero-padded word, weight 1
    EXPECT(lsq_snap_digest(one4, 4, 0) - lsq_snap_digest(one, 1, 0) == 3 * LSQ_SNAP_GOLD64);      // the same word; the byte length enters
    EXPECT(lsq_snap_digest(one4, 4, 1) == (uint64_t)lsq_snap_fmix32(1u ^ LSQ_SNAP_GOLD32) * 3u + 4 * LSQ_SNAP_GOLD64);
    EXPECT(lsq_snap_term(5, 1) != lsq_snap_term(5, 2) && lsq_snap_term(5, (1ull << 32) + 1) == lsq_snap_term(5, 1));      // the position enters mod 2^32
    {
        std::vector<unsigned char> buf(1024 + 3);
        uint64_t s = 11;
        for (unsigned char &b : buf) b = (unsigned char)next(&s);
        for (size_t len : {(size_t)0, (size_t)1, (size_t)3, (size_t)4, (size_t)5, (size_t)255, (size_t)256, (size_t)257, (size_t)1024, (size_t)1027}) {
            const uint64_t whole = lsq_snap_digest(buf.data(), len, 0);
            for (size_t cut = 0; cut <= len; cut += 4)
                EXPECT(lsq_snap_digest(buf.data(), cut, 0) + lsq_snap_digest(buf.data() + cut, len - cut, cut / 4) == whole);
            if (len) {                                                                   // any single byte changes it; swapping two unequal words changes it
                std::vector<unsigned char> other(buf.begin(), buf.begin() + (long)len);
                other[len / 2] ^= 0x10;
                EXPECT(lsq_snap_digest(other.data(), len, 0) != whole);
            }
        }
        std::vector<unsigned char> sw(buf.begin(), buf.begin() + 16);
        for (int b = 0; b < 4; ++b) std::swap(sw[(size_t)b], sw[(size_t)(8 + b)]);
        EXPECT(lsq_snap_digest(sw.data(), 16, 0) != lsq_snap_digest(buf.data(), 16, 0));
        for (size_t a = 1; a < 4; ++a) EXPECT(lsq_snap_digest(buf.data() + a, 64, 5) == lsq_snap_digest(std::vector<unsigned char>(buf.begin() + (long)a, buf.begin() + (long)a + 64).data(), 64, 5));
    }

    // ---- overflow-checked sizes and the plan
    int64_t r = 0;
    EXPECT(lsq_snap_mul(1ll << 31, 1ll << 31, &r) && r == (1ll << 62) && !lsq_snap_mul(1ll << 32, 1ll << 31, &r) && !lsq_snap_mul(-1, 2, &r));
    EXPECT(lsq_snap_add(INT64_MAX - 1, 1, &r) && !lsq_snap_add(INT64_MAX, 1, &r) && !lsq_snap_align(INT64_MAX - 10, &r) && lsq_snap_align(65, &r) && r == 128);
    {
        lsq_snapshot_info s{};
        s.n = (int64_t)INT32_MAX - 1; s.d = INT32_MAX; s.has_base = 1;                   // n d 4 bytes of f32 rows: past 2^63
        EXPECT(!lsq_snap_plan(&s, &err) && strstr(err.text, "overflow") && strstr(err.text, "BASE"));
        s.base_format = 1;                                                               // uint8 rows: fits
        EXPECT(lsq_snap_plan(&s, &err) && s.nsections == 1 && s.sections[0].offset == 192 && s.file_bytes == 192 + s.n * s.d);
        s = lsq_snapshot_info{}; s.n = 5; s.d = 2;
        EXPECT(!lsq_snap_plan(&s, &err));                                                // neither codes nor base rows
        s.has_codes = 1; s.m = 17; s.h = 256;
        EXPECT(!lsq_snap_plan(&s, &err));
        s.m = 16; s.nlist = 2; s.filter_active = 1; s.allowed = 6;
        EXPECT(!lsq_snap_plan(&s, &err));                                                // allowed > n
        s.allowed = 5; s.filter_force = 3;
        EXPECT(!lsq_snap_plan(&s, &err));
        s.filter_force = LSQ_FILTER_FORCE_DENSE;
        EXPECT(lsq_snap_plan(&s, &err) && s.nsections == 6 && s.sections[5].kind == LSQ_SNAP_FILTER_BITS && s.sections[5].bytes == 4);
        for (int k = 0; k < 6; ++k) EXPECT(s.sections[k].offset % 64 == 0 && (k == 0 || s.sections[k].offset >= s.sections[k - 1].offset + s.sections[k - 1].bytes));
    }

    // ---- the writer and the reader on one small file
    State st;
    const std::string path = dir + "/snapshot_check.snap", cut = dir + "/snapshot_check.cut";
    lsq_snapshot_arrays a = st.arrays();
    EXPECT(lsq_snap_write_file(path.c_str(), &a, &err) == LSQ_OK);
    lsq_snapshot_info info;
    EXPECT(lsq_snap_read_file(path.c_str(), &info, 1, nullptr, &err) == LSQ_OK);
    EXPECT(info.nsections == 7 && info.n == 33 && info.allowed == 1 + __builtin_popcount(st.bits[0]) && info.file_bytes < 4096 && info.filter_force == LSQ_FILTER_FORCE_COMPACT);
    std::vector<unsigned char> file((size_t)info.file_bytes);
    {
        FILE *f = fopen(path.c_str(), "rb");
        EXPECT(f && fread(file.data(), 1, file.size(), f) == file.size());
        if (f) fclose(f);
    }
    State back;                                                                          // other contents, the same exact sizes
    for (float &x : back.K) x = 0;
    lsq_snapshot_arrays b = back.arrays();
    b.filter_force = 0;
    EXPECT(lsq_snap_read_file(path.c_str(), &info, 0, &b, &err) == LSQ_OK);
    EXPECT(back.K == st.K && back.codes == st.codes && back.dbn == st.dbn && back.base == st.base && back.cent == st.cent && back.lor == st.lor && back.bits == st.bits);
    EXPECT(b.filter_force == LSQ_FILTER_FORCE_COMPACT && b.n == 33 && b.nlist == 3 && b.allowed == info.allowed);
    lsq_snapshot_arrays absent = back.arrays();
    std::vector<uint8_t> nc(33);
    absent.norm_codes = nc.data();                                                       // an array the file does not have
    EXPECT(lsq_snap_read_file(path.c_str(), &info, 0, &absent, &err) == LSQ_EINVAL && strstr(err.text, "NORM_CODES"));
    // a missing directory: LSQ_EIO, and a failed write leaves the file that is there alone
    EXPECT(lsq_snap_write_file((dir + "/no-such-directory/x.snap").c_str(), &a, &err) == LSQ_EIO);
    EXPECT(lsq_snap_read_file((dir + "/no-such-file.snap").c_str(), &info, 0, nullptr, &err) == LSQ_EIO);

    {                                                                                    // the temporary cannot be made: LSQ_EIO, the file stays, and what stood in the way is not removed
        const std::string blocked = path + ".tmp-snapshot";
        State other;
        other.codes[0] ^= 1;
        lsq_snapshot_arrays o = other.arrays();
        EXPECT(mkdir(blocked.c_str(), 0700) == 0);
        EXPECT(lsq_snap_write_file(path.c_str(), &o, &err) == LSQ_EIO);
        EXPECT(rmdir(blocked.c_str()) == 0);                                             // still there
        EXPECT(lsq_snap_read_file(path.c_str(), &info, 0, &b, &err) == LSQ_OK && back.codes == st.codes);
    }

    // ---- every prefix of the file is refused: by the inspector, by the verifying inspector and by the reader into exactly-sized arrays
    int refused = 0;
    for (size_t len = 0; len < file.size(); ++len) {
        EXPECT(put_file(cut, file.data(), len));
        const int r0 = lsq_snap_read_file(cut.c_str(), &info, 0, nullptr, &err), r1 = lsq_snap_read_file(cut.c_str(), &info, 1, nullptr, &err);
        State into;
        lsq_snapshot_arrays c = into.arrays();
        const int r2 = lsq_snap_read_file(cut.c_str(), &info, 0, &c, &err);
        EXPECT(r0 == LSQ_EFORMAT && r1 == LSQ_EFORMAT && r2 == LSQ_EFORMAT);
        refused += r0 != LSQ_OK;
    }
    EXPECT(refused == (int)file.size());
    {                                                                                    // and one byte too many
        std::vector<unsigned char> more(file);
        more.push_back(0);
        EXPECT(put_file(cut, more.data(), more.size()) && lsq_snap_read_file(cut.c_str(), &info, 0, nullptr, &err) == LSQ_EFORMAT && strstr(err.text, "trailing"));
    }

    // ---- every single-byte change of the header and the table is refused: every value in memory, three values through the file
    const size_t head = (size_t)lsq_snap_table_end(7);
    long changed = 0;
    for (size_t at = 0; at < head; ++at) {
        std::vector<unsigned char> mut(file.begin(), file.begin() + (long)head);
        for (int v = 1; v < 256; ++v) {
            mut[at] = (unsigned char)(file[at] ^ v);
            EXPECT(lsq_snap_validate(mut.data(), (int64_t)head, (int64_t)file.size(), &info, &err) == LSQ_EFORMAT);
            EXPECT(lsq_snap_validate(mut.data(), (int64_t)at, (int64_t)file.size(), &info, &err) == LSQ_EFORMAT);      // ... and of a header cut there
            ++changed;
        }
        for (int v : {0x01, 0x80, 0xff}) {
            std::vector<unsigned char> whole(file);
            whole[at] = (unsigned char)(file[at] ^ v);
            EXPECT(put_file(cut, whole.data(), whole.size()));
            State into;
            lsq_snapshot_arrays c = into.arrays();
            EXPECT(lsq_snap_read_file(cut.c_str(), &info, 1, &c, &err) == LSQ_EFORMAT);
        }
    }
    // a changed payload or padding byte: only the verifying calls can see it, and they name the section
    for (int k = 0; k < 7; ++k) {
        std::vector<unsigned char> whole(file);
        lsq_snapshot_info good;
        EXPECT(lsq_snap_validate(file.data(), (int64_t)head, (int64_t)file.size(), &good, &err) == LSQ_OK);
        whole[(size_t)good.sections[k].offset] ^= 0x04;
        EXPECT(put_file(cut, whole.data(), whole.size()));
        EXPECT(lsq_snap_read_file(cut.c_str(), &info, 0, nullptr, &err) == LSQ_OK);
        EXPECT(lsq_snap_read_file(cut.c_str(), &info, 1, nullptr, &err) == LSQ_EFORMAT && strstr(err.text, lsq_snap_kind_name(good.sections[k].kind)) && strstr(err.text, "digest"));
        const int64_t prev_end = k ? good.sections[k - 1].offset + good.sections[k - 1].bytes : (int64_t)head;
        if (good.sections[k].offset > prev_end) {
            whole = file;
            whole[(size_t)prev_end] = 0x20;
            EXPECT(put_file(cut, whole.data(), whole.size()));
            EXPECT(lsq_snap_read_file(cut.c_str(), &info, 1, nullptr, &err) == LSQ_EFORMAT && strstr(err.text, "padding") && strstr(err.text, lsq_snap_kind_name(good.sections[k].kind)));
        }
    }
    (void)remove(path.c_str());
    (void)remove(cut.c_str());
    printf("%d prefixes and %ld header bytes refused\n", refused, changed);
    if (failures) { printf("%d checks FAILED\n", failures); return 1; }
    printf("all passed\n");
    return 0;
}
