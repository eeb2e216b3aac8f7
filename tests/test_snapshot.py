"""Snapshots, the parts that need no GPU: the C ABI of the nine symbols of v2600 and the binding's structs against the header's, the host digest held bit for
bit to the numpy statement of tests/snapshot_check.py, lsq_snapshot_write_cpu held byte for byte to the numpy writer over every combination that changes
the section set, the read round trip, every refusal of a malformed file -- each naming what was wrong -- and the host-only rules
(csrc/lsq_snapshot_check.h) run by the stand-alone program tools/snapshot_check_main.cpp under the address and undefined-behaviour sanitizers."""
import ctypes as C
import itertools
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import snapshot_check as SC  # noqa: E402
from packed_check import header, header_struct_fields  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lsq_index_save", "lsq_index_load", "lsq_index_export", "lsq_index_digest", "lsq_index_get_snapshot_info", "lsq_snapshot_write_cpu",
       "lsq_snapshot_read_cpu", "lsq_snapshot_inspect_cpu", "lsq_snapshot_digest_cpu")
LENGTHS = (0, 1, 3, 4, 5, 255, 256, 257, 65535, 65537)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_symbols_the_codes_and_the_structs(lsq):
    hdr = header()
    assert int(re.search(r"#define LSQ_VERSION (\d+)", hdr).group(1)) >= 2600
    declared = re.findall(r"LSQ_API\s+[\w\s\*]*?\b(lsq_\w+)\s*\(", hdr)
    assert set(NEW) <= set(declared) and len(declared) == len(set(declared)) and len(declared) >= 125      # 116 symbols before this section, nine in it
    assert re.search(r"LSQ_EIO = -6\b", hdr) and re.search(r"LSQ_EFORMAT = -7\b", hdr) and re.search(r"#define LSQ_SNAPSHOT_FORMAT 1\b", hdr)
    for name in NEW[5:]:
        assert not re.search(r"\b%s\s*\(\s*(struct\s+)?lsq_(ctx|index)" % name, hdr), name      # the host-only road takes no handle
    assert "(3p)" in hdr and "IDENTITY S" in hdr and "IDENTITY F" in hdr and hdr.count("THE REFERENCE HAS NO COUNTERPART") >= 6
    # the digest is pinned in the header's comment: the constants of the numpy statement appear there
    for const in ("0x9E3779B1", "0x9E3779B97F4A7C15", "0x85EBCA6B", "0xC2B2AE35"):
        assert const in hdr, const
    assert header_struct_fields("lsq_snapshot_section") == ["kind", "elem_bytes", "offset", "bytes", "digest"]
    assert header_struct_fields("lsq_snapshot_arrays")[:12] == ["n", "d", "m", "h", "packed", "ncb", "base_format", "nlist", "filter_active", "filter_force", "reserved", "allowed"]
    kinds = dict(re.findall(r"LSQ_SNAP_(\w+) = (\d+)", re.search(r"enum \{ LSQ_SNAP_CODEBOOKS.*?\};", hdr, flags=re.S).group(0)))
    assert {k.lower(): int(v) for k, v in kinds.items() if k != "MAX_SECTIONS"} == SC.KINDS and int(kinds["MAX_SECTIONS"]) == 9


def test_binding_agrees_with_the_header(lsq):
    B = lsq._lib
    assert B.MIN_VERSION >= 2600 and (B.LSQ_EIO, B.LSQ_EFORMAT) == (SC.EIO, SC.EFORMAT) == (-6, -7)
    for struct_name, cls in (("lsq_snapshot_arrays", B.SnapshotArrays), ("lsq_snapshot_section", B.SnapshotSection), ("lsq_snapshot_info", B.SnapshotInfo),
                             ("lsq_snapshot_io_info", B.SnapshotIoInfo)):
        assert [f for f, _ in cls._fields_] == header_struct_fields(struct_name), struct_name
    assert C.sizeof(B.SnapshotSection) == 40 and C.sizeof(B.SnapshotInfo) == 17 * 8 + 9 * 40 and C.sizeof(B.SnapshotArrays) == 8 + 10 * 4 + 8 + 9 * 8
    assert C.sizeof(B.SnapshotIoInfo) == 11 * 8 and [t for _, t in B.SnapshotIoInfo._fields_] == [C.c_int64] * 6 + [C.c_double] * 5
    assert B.SnapshotArrays.allowed.offset == 48 and B.SnapshotArrays.codebooks.offset == 56
    vp, i, i64, s = C.c_void_p, C.c_int, C.c_int64, C.c_char_p
    assert B.SIGNATURES["lsq_index_save"][1] == [vp, s, i] and B.SIGNATURES["lsq_index_load"][1][1:] == [vp, s, i]
    assert B.SIGNATURES["lsq_snapshot_digest_cpu"][1][:3] == [vp, i64, i64] and len(B.SIGNATURES) >= 125
    assert B.SNAP_NAMES == SC.NAMES and B.SNAPSHOT_FORMAT == SC.FORMAT
    assert {"snapshot_info", "snapshot_write", "snapshot_read", "snapshot_digest"} <= set(lsq.__all__)
    for method in ("save", "export", "digest", "snapshot_info"):
        assert callable(getattr(lsq.Index, method))
    assert callable(lsq.Engine.load_index)
    for tuning in (False, True):
        raw = C.CDLL(B.TUNING_LIB_PATH if tuning else B.LIB_PATH)
        assert B.load(tuning=tuning).lsq_version() >= 2600 and all(hasattr(raw, name) for name in NEW)
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "125 symbols" in f.read()


def test_null_handles_are_refused_without_a_device(lsq):
    L = lsq._lib.load()
    info, io, arrays, handle = lsq._lib.SnapshotInfo(), lsq._lib.SnapshotIoInfo(), lsq._lib.SnapshotArrays(), C.c_void_p(123)
    assert L.lsq_index_save(None, b"/nowhere", 0) == SC.EINVAL and b"lsq_index_save" in L.lsq_last_error()
    assert L.lsq_index_load(C.byref(handle), None, b"/nowhere", 0) == SC.EINVAL and handle.value is None
    assert L.lsq_index_export(None, C.byref(arrays), 0) == SC.EINVAL and L.lsq_index_digest(None, C.byref(info)) == SC.EINVAL
    assert L.lsq_index_get_snapshot_info(None, C.byref(io)) == SC.EINVAL
    out = C.c_uint64(5)
    assert L.lsq_snapshot_digest_cpu(None, 4, 0, C.byref(out)) == SC.EINVAL and L.lsq_snapshot_digest_cpu(None, -1, 0, C.byref(out)) == SC.EINVAL and out.value == 5
    assert L.lsq_snapshot_write_cpu(None, C.byref(arrays)) == SC.EINVAL and L.lsq_snapshot_inspect_cpu(b"/nowhere", None, 0) == SC.EINVAL


# ---- the digest: host against numpy ---------------------------------------------------------------------------------------------------------------------
def test_numpy_statement_says_what_the_header_pins():
    assert int(SC.fmix32(np.array([0, 1], np.uint32))[1]) == 0x514E28B7 and int(SC.fmix32(np.array([0], np.uint32))[0]) == 0
    assert SC.digest(b"") == 0 and SC.digest(b"\0\0\0\0") == 4 * SC.GOLD64 & SC.M64
    assert SC.digest(b"\1") == 0x514E28B7 + SC.GOLD64 and SC.digest(b"\1\0\0\0") == (0x514E28B7 + 4 * SC.GOLD64) & SC.M64
    w = int(SC.fmix32(np.array([1 ^ SC.GOLD32], np.uint32))[0])
    assert SC.digest(b"\1\0\0\0", first_word=1) == (w * 3 + 4 * SC.GOLD64) & SC.M64
    # position: swapping two unequal words changes it; the position key wraps at 2^32 words, the weight at 2^31
    a, b = struct.pack("<II", 5, 9), struct.pack("<II", 9, 5)
    assert SC.digest(a) != SC.digest(b)
    assert SC.digest(a, first_word=1 << 32) == SC.digest(a)
    # the per-word mix is a bijection for a fixed position: 2^16 words at one position give 2^16 different terms
    words = np.arange(1 << 16, dtype=np.uint32) * np.uint32(65537)
    terms = {SC.digest(struct.pack("<I", int(x)), first_word=77) for x in words[:4096]}
    assert len(terms) == 4096


@pytest.mark.parametrize("length", LENGTHS)
def test_host_digest_equals_numpy(lsq, length):
    rng = np.random.default_rng(length)
    buf = rng.integers(0, 256, length + 8, dtype=np.uint8)
    for start in (0, 1, 3):                                                  # any alignment of the data
        data = buf[start:start + length]
        for fw in (0, 1, 12345, (1 << 31) - 1, (1 << 32) + 5):
            assert lsq.snapshot_digest(data, fw) == SC.digest(data, fw), (length, start, fw)
    if length:
        other = buf[:length].copy()
        other[length // 2] ^= 0x40
        assert lsq.snapshot_digest(other) != lsq.snapshot_digest(buf[:length])            # any single byte changes it
        assert lsq.snapshot_digest(buf[:length]) != lsq.snapshot_digest(np.concatenate([buf[:length], np.zeros(1, np.uint8)]))      # the length enters


def test_digests_of_every_split_of_a_kib_add_up(lsq):
    rng = np.random.default_rng(1024)
    buf = rng.integers(0, 256, 1024, dtype=np.uint8)
    whole = lsq.snapshot_digest(buf)
    assert whole == SC.digest(buf)
    for cut in range(0, 1025, 4):
        got = (lsq.snapshot_digest(buf[:cut]) + lsq.snapshot_digest(buf[cut:], cut // 4)) & SC.M64
        assert got == whole and (SC.digest(buf[:cut]) + SC.digest(buf[cut:], cut // 4)) & SC.M64 == whole, cut
    # three pieces, in any order
    parts = [(0, 100), (100, 512), (512, 1024)]
    assert sum(lsq.snapshot_digest(buf[a:b], a // 4) for a, b in reversed(parts)) & SC.M64 == whole


# ---- the writer: lsq_snapshot_write_cpu against the numpy writer, byte for byte ------------------------------------------------------------------------
def _variants():
    """(kind, base, nlist, filter, force): every combination that changes the section set"""
    out = []
    for kind in ("plain", "packed", "base-only", "scan-only"):
        bases = (None,) if kind == "scan-only" else ("f32", "u8", "f16", "bf16") if kind == "base-only" else (None, "f32", "u8", "f16", "bf16")
        for base in bases:
            for nlist in ((0,) if kind == "base-only" else (0, 3)):
                for filt, force in ((False, 0), (True, 0), (True, SC.FORCE_DENSE), (True, SC.FORCE_COMPACT)):
                    out.append((kind, base, nlist, filt, force))
    return out


VARIANTS = _variants()


def _written(lsq, path, state):
    lsq.snapshot_write(path, **SC.write_args(state))
    with open(path, "rb") as f:
        return f.read()


def test_writer_equals_numpy_on_every_section_set(lsq, tmp_path):
    path = str(tmp_path / "a.snap")
    for k, (kind, base, nlist, filt, force) in enumerate(VARIANTS):
        state = SC.make_state(np.random.default_rng(k), 33, 7, 3, kind, base, nlist, filt, force)
        want = SC.file_bytes_of(state)
        assert _written(lsq, path, state) == want, VARIANTS[k]
        sc, table, back = SC.parse(want)                                     # the numpy reader agrees with its writer
        assert SC.same_state(back, state)
        info = lsq.snapshot_info(path, verify=True)
        assert [(s["kind"], s["elem_bytes"], s["offset"], s["bytes"], s["digest"]) for s in info["sections"]] == table
        assert all(info[key] == sc[key] for key in sc) and info["file_bytes"] == len(want) and info["format"] == 1
        assert info["header_digest"] == struct.unpack_from("<Q", want, SC.table_end(len(table)) - 8)[0]
        assert SC.same_state(lsq.snapshot_read(path), state)                 # the read round trip: the same bytes, NaN payloads included
        assert not [f for f in os.listdir(tmp_path) if f != "a.snap"]        # no temporary is left behind


@pytest.mark.parametrize("n", [1, 31, 32, 33])
def test_writer_equals_numpy_over_the_shapes(lsq, tmp_path, n):
    path = str(tmp_path / "a.snap")
    for k, (m, d) in enumerate(itertools.product((1, 7, 8, 16), (1, 3, 32))):
        kind, base, nlist, filt, force = VARIANTS[(7 * k + n) % len(VARIANTS)]
        state = SC.make_state(np.random.default_rng(100 * n + k), n, m, d, kind, base, nlist, filt, force)
        assert _written(lsq, path, state) == SC.file_bytes_of(state), (n, m, d, kind, base, nlist, filt)
        assert SC.same_state(lsq.snapshot_read(path), state)


def test_writer_drops_filter_bits_past_n_and_recounts(lsq, tmp_path):
    state = SC.make_state(np.random.default_rng(5), 33, 2, 3, "plain", None, 0, True)
    dirty = dict(state, filter_bits=state["filter_bits"] | np.array([0, 0xFFFFFFFC], np.uint32))
    path = str(tmp_path / "a.snap")
    clean = _written(lsq, path, state)
    assert _written(lsq, path, dirty) == clean == SC.file_bytes_of(dirty)
    assert lsq.snapshot_info(path)["allowed"] == sum(bin(int(w)).count("1") for w in state["filter_bits"])


def test_writer_refusals(lsq, tmp_path):
    L, B = lsq._lib.load(), lsq._lib
    state = SC.make_state(np.random.default_rng(6), 9, 2, 3, "plain", "f32", 2, True)
    path = str(tmp_path / "a.snap")
    good = _written(lsq, path, state)

    def arrays(**over):
        a = B.SnapshotArrays()
        a.n, a.d, a.m, a.h, a.nlist, a.filter_active = 9, 3, 2, 256, 2, 1
        keep = {k: np.ascontiguousarray(v) for k, v in state.items() if k != "filter_force"}
        for k, v in keep.items():
            setattr(a, k, v.ctypes.data)
        for k, v in over.items():
            setattr(a, k, v)
        return a, keep

    for over, word in ((dict(n=0), b"n = 0"), (dict(m=17), b"m = 17"), (dict(h=128), b"h = 128"), (dict(codebooks=None), b"CODEBOOKS"), (dict(list_of_row=None), b"LIST_OF_ROW"),
                       (dict(base_format=4), b"base format"), (dict(filter_force=1), b"FORCE"), (dict(packed=1, ncb=0), b"ncb"), (dict(nlist=-1), b"nlist")):
        a, keep = arrays(**over)
        assert L.lsq_snapshot_write_cpu(path.encode(), C.byref(a)) == SC.EINVAL and word in L.lsq_last_error(), (over, L.lsq_last_error())
    # LSQ_EIO: a directory that does not exist; the file that is there stays as it was
    a, keep = arrays()
    assert L.lsq_snapshot_write_cpu(str(tmp_path / "missing" / "a.snap").encode(), C.byref(a)) == SC.EIO
    with open(path, "rb") as f:
        assert f.read() == good
    with pytest.raises(ValueError):
        lsq.snapshot_write(path, codes=state["codes"], codebooks=state["codebooks"])                      # neither dbnorms nor norm bytes
    with pytest.raises(ValueError):
        lsq.snapshot_write(path, codes=state["codes"], codebooks=state["codebooks"], dbnorms=state["dbnorms"][:-1])
    with pytest.raises(TypeError):
        lsq.snapshot_write(path, base=np.zeros((3, 3), np.int16))


# ---- refusals of a malformed file ---------------------------------------------------------------------------------------------------------------------
def _refused(lsq, tmp_path, raw, code, *words, verify=False):
    """the inspector (and the reader) refuse the file with `code`, naming every word"""
    path = str(tmp_path / "bad.snap")
    with open(path, "wb") as f:
        f.write(raw)
    L, info = lsq._lib.load(), lsq._lib.SnapshotInfo()
    rc = L.lsq_snapshot_inspect_cpu(path.encode(), C.byref(info), int(verify))
    msg = L.lsq_last_error().decode()
    assert rc == code and all(w in msg for w in words) and "lsq_snapshot_inspect_cpu" in msg, (rc, msg, words)
    assert info.n == 0 and info.nsections == 0                               # nothing is handed out
    with pytest.raises(lsq._lib.LsqError) as e:
        lsq.snapshot_read(path)
    assert e.value.code == code
    return msg


@pytest.fixture(scope="module")
def good_file():
    state = SC.make_state(np.random.default_rng(9), 33, 7, 3, "packed", "f16", 3, True, SC.FORCE_DENSE)
    return state, SC.file_bytes_of(state)


def test_header_refusals(lsq, tmp_path, good_file):
    state, raw = good_file
    E = SC.EFORMAT
    _refused(lsq, tmp_path, b"LSQSNAQ\0" + raw[8:], E, "magic")
    _refused(lsq, tmp_path, b"", E, "truncated")
    _refused(lsq, tmp_path, SC.patch_header(raw, 8, "<I", 2), E, "newer", "version 2")
    _refused(lsq, tmp_path, SC.patch_header(raw, 12, ">I", SC.ENDIAN), E, "big-endian")
    _refused(lsq, tmp_path, SC.patch_header(raw, 16, "<I", 136), E, "header length")
    _refused(lsq, tmp_path, SC.patch_header(raw, 20, "<I", 10), E, "10 sections")
    _refused(lsq, tmp_path, SC.patch_header(raw, 24, "<q", 34), E, "inconsistent with n, d, m")      # n changed, the table not
    _refused(lsq, tmp_path, SC.patch_header(raw, 32, "<i", 4), E, "CODEBOOKS", "inconsistent with n, d, m")
    _refused(lsq, tmp_path, SC.patch_header(raw, 36, "<i", 17), E, "m = 17")
    _refused(lsq, tmp_path, SC.patch_header(raw, 48, "<i", 300), E, "ncb = 300")
    _refused(lsq, tmp_path, SC.patch_header(raw, 60, "<I", 5), E, "base format")                     # the base flag dropped under a base format
    _refused(lsq, tmp_path, SC.patch_header(raw, 64, "<i", 1), E, "FORCE")
    _refused(lsq, tmp_path, SC.patch_header(raw, 68, "<i", 1), E, "reserved")
    _refused(lsq, tmp_path, SC.patch_header(raw, 72, "<q", 34), E, "allowed = 34")
    _refused(lsq, tmp_path, SC.patch_header(raw, 80, "<q", len(raw) + 64), E, "the header says")
    _refused(lsq, tmp_path, SC.patch_header(raw, 100, "<B", 1), E, "reserved")
    _refused(lsq, tmp_path, SC.patch_entry(raw, 0, "digest", 1, seal=False), E, "header's digest")
    # sizes whose product overflows 64 bits: refused from the header alone -- the file is 4 KiB, nothing is allocated for what it claims
    huge = SC.patch_header(SC.patch_header(SC.patch_header(raw, 24, "<q", (1 << 31) - 2, seal=False), 52, "<i", 0, seal=False), 32, "<i", (1 << 31) - 1)
    _refused(lsq, tmp_path, huge, E, "overflow", "BASE")                     # (2^31 - 2) (2^31 - 1) float32 rows


def test_table_refusals(lsq, tmp_path, good_file):
    state, raw = good_file
    E = SC.EFORMAT
    sc, table, _ = SC.parse(raw)
    assert [SC.NAMES[t[0]] for t in table] == ["codebooks", "codes", "norm_codes", "cbnorms", "base", "centroids", "list_of_row", "filter_bits"]
    _refused(lsq, tmp_path, SC.patch_entry(raw, 1, "offset", table[1][2] + 4), E, "CODES", "not a multiple of 64")
    _refused(lsq, tmp_path, SC.patch_entry(raw, 2, "offset", table[1][2]), E, "NORM_CODES", "overlaps")
    _refused(lsq, tmp_path, SC.patch_entry(raw, 7, "offset", SC.align(len(raw)) + 64), E, "FILTER_BITS", "past the end")
    _refused(lsq, tmp_path, SC.patch_entry(raw, 4, "offset", table[4][2] + 64), E, "BASE")           # aligned, in bounds, not canonical (or overlapping the next)
    _refused(lsq, tmp_path, SC.patch_entry(raw, 1, "bytes", table[1][3] + 7), E, "CODES", "inconsistent with n, d, m")
    _refused(lsq, tmp_path, SC.patch_entry(raw, 4, "elem", 4), E, "BASE", "elements of 4 bytes")
    _refused(lsq, tmp_path, SC.patch_entry(raw, 2, "kind", 3), E, "DBNORMS", "NORM_CODES")
    _refused(lsq, tmp_path, raw[:-1], E, "truncated")                        # one byte short
    _refused(lsq, tmp_path, raw + b"\0", E, "trailing")
    _refused(lsq, tmp_path, raw[:SC.table_end(len(table)) - 3], E, "truncated")


def test_payload_refusals_need_verify_and_name_the_section(lsq, tmp_path, good_file):
    state, raw = good_file
    sc, table, _ = SC.parse(raw)
    L, info = lsq._lib.load(), lsq._lib.SnapshotInfo()
    path = str(tmp_path / "bad.snap")
    for k, entry in enumerate(table):
        name = SC.SECTION_NAMES[entry[0]]
        bad = SC.flip_payload_bit(raw, k, byte=entry[3] - 1, bit=7)          # the last bit of the section
        with open(path, "wb") as f:
            f.write(bad)
        assert L.lsq_snapshot_inspect_cpu(path.encode(), C.byref(info), 0) == 0          # header and table are fine
        _refused(lsq, tmp_path, bad, SC.EFORMAT, name, "digest mismatch", verify=True)
        pad = SC.nonzero_padding(raw, k)
        if pad is not None:
            _refused(lsq, tmp_path, pad, SC.EFORMAT, name, "non-zero padding", verify=True)
    assert sum(SC.nonzero_padding(raw, k) is not None for k in range(len(table))) >= 4
    # a payload changed under a RECOMPUTED table is a valid file: the digests cannot know what a list id means
    odd = SC.corrupt_payload_valid_table(raw, "list_of_row", lambda a: np.full_like(a, 3))
    with open(path, "wb") as f:
        f.write(odd)
    assert lsq.snapshot_info(path, verify=True)["nlist"] == 3 and int(lsq.snapshot_read(path)["list_of_row"][0]) == 3


def test_missing_file_is_an_io_error(lsq, tmp_path):
    with pytest.raises(lsq._lib.LsqError) as e:
        lsq.snapshot_info(str(tmp_path / "nothing.snap"))
    assert e.value.code == SC.EIO and "cannot open" in str(e.value)


# ---- the host rules under the sanitizers ----------------------------------------------------------------------------------------------------------------
def test_host_rules_under_the_sanitizers(tmp_path):
    """the digest's pinned values and additivity, the overflow-checked plan, and -- over a snapshot of under 4 KiB -- EVERY prefix length and EVERY
    single-byte change of the header and table refused with an error code, in a stand-alone program with its own main, built under
    -fsanitize=address,undefined and run directly.  The plain build stands in ONLY where the compiler says that it has no sanitizer runtime to link
    (then the test prints so); any other compile error fails the test, and so does a sanitizer report at run time"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = os.path.join(ROOT, "tools", "snapshot_check_main.cpp"), str(tmp_path / "snapshot_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", src, "-o", exe]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    sanitized = p.returncode == 0
    if not sanitized:
        missing = re.search(r"cannot find -l(asan|ubsan)|lib(asan|ubsan)[\w.\-]*: No such file|libclang_rt\.(asan|ubsan)|unsupported option '-fsanitize|unrecognized.*-fsanitize", p.stderr)
        assert missing, "the sanitized build failed for another reason than a missing runtime:\n" + p.stderr[-2000:]
        p = subprocess.run(base, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
    print("snapshot_check built %s" % ("under ASan + UBSan" if sanitized else "WITHOUT sanitizers: the compiler has no runtime for them (%s)" % missing.group(0)))
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True)
    assert r.returncode == 0 and "all passed" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    assert re.search(r"(\d+) prefixes", r.stdout) and int(re.search(r"(\d+) prefixes", r.stdout).group(1)) > 1000
