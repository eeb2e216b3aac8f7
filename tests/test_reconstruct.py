"""The decode, the parts that need no GPU: the C ABI of lsq_reconstruct_cpu, lsq_index_reconstruct, lsq_index_search_rows and
lsq_index_get_recon_info (v2400), the binding's struct against the header's, Index.reconstruct / Index.search_rows reaching their symbols (calls recorded by
the stand-in of tests/engine_calls.py), the refusals that need no device, the host-only rules (csrc/lsq_recon_check.h) run by the stand-alone program
tools/recon_check_main.cpp under the address and undefined-behaviour sanitizers -- and lsq_reconstruct_cpu held, bit for bit, to the contract of
tests/recon_check.py."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recon_check as RC  # noqa: E402
from engine_calls import _Recorder, _offline  # noqa: E402
from packed_check import header, header_struct_fields  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lsq_reconstruct_cpu", "lsq_index_reconstruct", "lsq_index_search_rows", "lsq_index_get_recon_info")
INFO_FIELDS = ["rows", "invalid", "map_rebuilt", "map_rebuilds", "road", "calls", "map_ms", "decode_ms"]
EINVAL = -1
H = 256
SENTINEL = 0xDEADBEEF


def test_header_declares_the_symbols_and_struct(lsq):
    hdr = header()
    assert int(re.search(r"#define LSQ_VERSION (\d+)", hdr).group(1)) >= 2400
    declared = set(re.findall(r"LSQ_API\s+[\w\s\*]*?\b(lsq_\w+)\s*\(", hdr))
    assert set(NEW) <= declared
    for name in NEW[1:]:
        assert re.search(r"\b%s\s*\(\s*lsq_index\s*\*" % name, hdr), name
    assert header_struct_fields("lsq_index_recon_info") == INFO_FIELDS
    assert "(3n)" in hdr and '"recon_chunk"' in hdr and "LSQ_RECON_ADD_COARSE 1" in hdr and "LSQ_RECON_PAD_NAN 2" in hdr
    assert len(declared) >= 112                                              # 108 symbols before this section, four in it (the two context forms: DESIGN 4.26)


def test_both_libraries_export_them_at_v2400(lsq):
    assert lsq._lib.MIN_VERSION >= 2400
    for tuning in (False, True):
        L = lsq._lib.load(tuning=tuning)
        assert L.lsq_version() >= 2400
        raw = C.CDLL(lsq._lib.TUNING_LIB_PATH if tuning else lsq._lib.LIB_PATH)
        for name in NEW:
            assert hasattr(raw, name), name


def test_binding_struct_equals_the_headers(lsq):
    B = lsq._lib
    assert [f for f, _ in B.IndexReconInfo._fields_] == INFO_FIELDS
    assert [t for _, t in B.IndexReconInfo._fields_] == [C.c_int64] * 6 + [C.c_double] * 2 and C.sizeof(B.IndexReconInfo) == 64
    assert set(NEW) <= set(B.SIGNATURES)
    vp, i, i64 = C.c_void_p, C.c_int, C.c_int64
    assert B.SIGNATURES["lsq_reconstruct_cpu"][1] == [vp, i64, vp, i64, vp, vp, i64, i, i64, i, i, i, vp, vp, i, i]
    assert B.SIGNATURES["lsq_index_reconstruct"][1] == [vp, vp, i64, vp, i64, i64, i, i, i]
    assert B.SIGNATURES["lsq_index_search_rows"][1] == [vp, vp, vp, vp, i, i, i, i, i, i]
    assert (B.RECON_ADD_COARSE, B.RECON_PAD_NAN) == (1, 2)
    assert "reconstruct_cpu" in lsq.__all__ and "reconstruct" in lsq.__all__


def test_null_handles_are_refused_without_a_device(lsq):
    L = lsq._lib.load()
    info = lsq._lib.IndexReconInfo()
    out, ids = np.zeros(8, np.float32), np.zeros(2, np.int32)
    assert L.lsq_index_reconstruct(None, out.ctypes.data, 4, ids.ctypes.data, 0, 2, 0, 0, 0) == EINVAL and b"lsq_index_reconstruct" in L.lsq_last_error()
    assert L.lsq_index_search_rows(None, out.ctypes.data, ids.ctypes.data, ids.ctypes.data, 2, 0, 1, 0, 0, 0) == EINVAL
    assert b"lsq_index_search_rows" in L.lsq_last_error()
    assert L.lsq_index_get_recon_info(None, C.byref(info)) == EINVAL and b"lsq_index_get_recon_info" in L.lsq_last_error()
    assert np.all(out == 0) and np.all(ids == 0)                             # nothing was written


def _offline_index(lsq, dev=False):
    eng = _offline(lsq.Engine)
    eng._L = _Recorder()
    ix = lsq.engine.Index.__new__(lsq.engine.Index)
    ix._eng, ix._L, ix._dev, ix._h, ix._keep = eng, eng._L, dev, C.c_void_p(2), None
    ix.n, ix.d, ix.m, ix._u8, ix._has_codes, ix._has_base, ix._packed = 100, 5, 3, False, True, False, False
    return ix


def test_reconstruct_and_search_rows_reach_their_symbols(lsq):
    B = lsq._lib
    ix = _offline_index(lsq)
    out = ix.reconstruct()                                                   # every row
    (name, args), = ix._L.calls
    assert name == "lsq_index_reconstruct" and out.shape == (100, 5) and out.dtype == np.float32
    assert args[0].value == 2 and args[1:] == (out.ctypes.data, 5, None, 0, 100, 0, 0, 0)
    ix._L.calls.clear()
    out = ix.reconstruct(start=90)                                           # to the last row
    assert ix._L.calls[0][1][1:] == (out.ctypes.data, 5, None, 90, 10, 0, 0, 0) and out.shape == (10, 5)
    ix._L.calls.clear()
    ids = np.array([7, 7, 3, 100, 1], dtype=np.int32)
    big = np.zeros((5, 9), dtype=np.float32)
    got = ix.reconstruct(ids=ids, add_coarse=True, pad_nan=True, id_base=1, out=big[:, 1:7])      # rows of pitch 9, 4 bytes into the buffer
    args = ix._L.calls[0][1]
    assert got.ctypes.data == big.ctypes.data + 4 and args[1:] == (big.ctypes.data + 4, 9, ids.ctypes.data, 0, 5, 1, B.RECON_ADD_COARSE | B.RECON_PAD_NAN, 0)
    ix._L.calls.clear()
    assert ix.reconstruct(ids=np.zeros(0, np.int32)).shape == (0, 5)         # count == 0 still reaches the library, without pointers
    assert ix._L.calls[0][1][1:] == (None, 5, None, 0, 0, 0, 0, 0)
    with pytest.raises(ValueError):
        ix.reconstruct(out=np.zeros((100, 4), np.float32))                   # fewer than d columns
    with pytest.raises(ValueError):
        ix.reconstruct(ids=ids, out=np.zeros((4, 5), np.float32))            # one row per id
    with pytest.raises(ValueError):
        ix.reconstruct(out=np.zeros((100, 5), np.float64))
    # search by stored row
    ix._L.calls.clear()
    rows = np.array([0, 99, 5], dtype=np.int32)
    dists, nbr = ix.search_rows(rows, 4)
    (name, args), = ix._L.calls
    assert name == "lsq_index_search_rows" and dists.shape == nbr.shape == (3, 4) and dists.dtype == np.float32 and nbr.dtype == np.int32
    assert args[1:] == (dists.ctypes.data, nbr.ctypes.data, rows.ctypes.data, 3, 0, 4, 0, 0, 0)
    ix._L.calls.clear()
    dists, nbr = ix.search_rows(rows, 2, nprobe=6, add_coarse=True, id_base=1)
    assert ix._L.calls[0][1][1:] == (dists.ctypes.data, nbr.ctypes.data, rows.ctypes.data, 3, 1, 2, 6, B.IVF_ADD_COARSE, 0)
    assert set(ix.recon_info()) == set(INFO_FIELDS)


def test_host_rules_under_the_sanitizers(tmp_path):
    """the chunk rule, the argument rules and lsq_reconstruct_cpu's body at the edge extents (count 0, one row, a partial last chunk, ids at both ends of
    the range, exactly-sized arrays) in a stand-alone program with its own main, built under -fsanitize=address,undefined and run directly.  The plain
    build stands in ONLY where the compiler says that it has no sanitizer runtime to link (then the test prints so); any other compile error fails the
    test, and so does a sanitizer report at run time"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = os.path.join(ROOT, "tools", "recon_check_main.cpp"), str(tmp_path / "recon_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", src, "-o", exe]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    sanitized = p.returncode == 0
    if not sanitized:
        missing = re.search(r"cannot find -l(asan|ubsan)|lib(asan|ubsan)[\w.\-]*: No such file|libclang_rt\.(asan|ubsan)|unsupported option '-fsanitize|unrecognized.*-fsanitize", p.stderr)
        assert missing, "the sanitized build failed for another reason than a missing runtime:\n" + p.stderr[-2000:]
        p = subprocess.run(base, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
    print("recon_check built %s" % ("under ASan + UBSan" if sanitized else "WITHOUT sanitizers: the compiler has no runtime for them (%s)" % missing.group(0)))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all passed" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# ---- lsq_reconstruct_cpu against the contract ---------------------------------------------------------------------------------------------------------
def _problem(n, m, d, seed, packed):
    rng = np.random.default_rng(seed)
    K = RC.special_codebooks(rng, m, d)
    rows = rng.integers(0, H, (n, m + 1)).astype(np.uint8)                    # rows of m + 1 bytes: the last one a norm byte the decode must not read as a code
    codes = rows[:, :m] if packed else np.ascontiguousarray(rows[:, :m])      # ldc = m + 1 in place, or m
    return rng, K, codes


@pytest.mark.parametrize("m", [1, 2, 7, 8, 16])
@pytest.mark.parametrize("d", [1, 3, 4, 5, 127, 128, 129])
def test_cpu_decode_equals_the_contract(lsq, m, d):
    lib = lsq._lib.load()
    n = 41
    for packed in (False, True):
        rng, K, codes = _problem(n, m, d, 1000 * m + d, packed)
        want = RC.decode(codes, K, m)
        assert RC.bits(want[:, 0]).max() == 0                                # the -0.0 column: +0.0 by the contract ...
        assert RC.bits(K[codes[:, 0].astype(np.int64), 0]).min() == 0x80000000      # ... where starting from the first codeword gives -0.0
        if d > 1 and m > 1:
            assert np.isnan(want[:, 1]).all()                                # inf - inf
        cent = rng.standard_normal((5, d)).astype(np.float32)
        lor = rng.integers(0, 5, n).astype(np.int32)
        for ldo in (d, d + 3):
            # ids == NULL: rows 0 .. n - 1; one thread and several
            for nt in (1, 3):
                rc, out = RC.reconstruct_cpu(lib, codes, K, m, ldo=ldo, nthreads=nt, sentinel=SENTINEL)
                assert rc == 0 and RC.same_bits(np.ascontiguousarray(out[:, :d]), want)
                assert np.all(out.view(np.uint32)[:, d:] == SENTINEL)        # the gaps between rows are not written
            # ids: repeated, descending, in both bases; with the coarse add
            for ids in (np.array([5, 5, 5, 0, n - 1, 5]), np.arange(n)[::-1], np.array([n - 1])):
                for base in (0, 1):
                    rc, out = RC.reconstruct_cpu(lib, codes, K, m, ids=ids + base, id_base=base, ldo=ldo, sentinel=SENTINEL)
                    assert rc == 0 and RC.same_bits(np.ascontiguousarray(out[:, :d]), RC.decode_ids(codes, K, m, ids))
                rc, out = RC.reconstruct_cpu(lib, codes, K, m, ids=ids, ldo=ldo, cent=cent, lor=lor, flags=lsq._lib.RECON_ADD_COARSE)
                assert rc == 0 and RC.same_bits(np.ascontiguousarray(out[:, :d]), RC.decode_ids(codes, K, m, ids, cent=cent, lor=lor))
            rc, out = RC.reconstruct_cpu(lib, codes, K, m, ldo=ldo, cent=cent, lor=lor, flags=lsq._lib.RECON_ADD_COARSE)
            assert rc == 0 and RC.same_bits(np.ascontiguousarray(out[:, :d]), RC.add_coarse(want, cent, lor))
            # ids outside at both ends: padded with the flag, refused without -- and then nothing is written
            ids = np.array([-1, 0, n, n - 1, 2 ** 31 - 1, -2 ** 31])
            both = lsq._lib.RECON_PAD_NAN | lsq._lib.RECON_ADD_COARSE
            rc, out = RC.reconstruct_cpu(lib, codes, K, m, ids=ids, ldo=ldo, cent=cent, lor=lor, flags=both, sentinel=SENTINEL)
            exp = RC.decode_ids(codes, K, m, ids, pad_nan=True, cent=cent, lor=lor)
            assert rc == 0 and RC.same_bits(np.ascontiguousarray(out[:, :d]), exp)
            assert np.all(out.view(np.uint32)[[0, 2, 4, 5], :d] == RC.NAN_BITS)
            rc, out = RC.reconstruct_cpu(lib, codes, K, m, ids=ids, ldo=ldo, sentinel=SENTINEL)
            assert rc == EINVAL and np.all(out.view(np.uint32) == SENTINEL) and b"lsq_reconstruct_cpu" in lib.lsq_last_error()


def test_cpu_decode_is_order_and_width_sensitive(lsq):
    codes, K = RC.order_sensitive(200, 8, 16, seed=3)                        # asserts that the case tells the orders and the widths apart
    rc, out = RC.reconstruct_cpu(lsq._lib.load(), codes, K, 8)
    assert rc == 0 and RC.same_bits(out, RC.decode(codes, K, 8))


def test_cpu_refusals_write_nothing(lsq):
    lib = lsq._lib.load()
    rng, K, codes = _problem(9, 3, 4, 5, False)
    out = np.full((9, 4), 7.0, np.float32)
    f = lambda **kw: lib.lsq_reconstruct_cpu(*[kw.get(k, v) for k, v in (      # noqa: E731
        ("out", out.ctypes.data), ("ldo", 4), ("codes", codes.ctypes.data), ("ldc", 3), ("K", K.ctypes.data), ("ids", None), ("count", 9), ("id_base", 0),
        ("n", 9), ("m", 3), ("h", H), ("d", 4), ("cent", None), ("lor", None), ("flags", 0), ("nt", 1))])
    assert f() == 0 and RC.same_bits(out, RC.decode(codes, K, 3))
    out[...] = 7.0
    for bad in (dict(ldo=3), dict(ldc=2), dict(count=-1), dict(count=10), dict(id_base=2), dict(m=0), dict(m=17), dict(h=257), dict(d=0), dict(flags=4),
                dict(flags=1), dict(out=None), dict(codes=None), dict(K=None)):
        assert f(**bad) == EINVAL, bad
        assert np.all(out == 7.0), bad
    assert f(count=0, out=None, codes=None, K=None) == 0                     # count == 0: LSQ_OK, nothing needed


def test_reference_reconstruct_without_an_engine_is_unchanged(lsq):
    rng = np.random.default_rng(11)
    m, d, n = 4, 6, 30
    Cs = [rng.standard_normal((d, H)).astype(np.float32) for _ in range(m)]
    B = rng.integers(1, H + 1, (m, n)).astype(np.int16)
    got = lsq.reconstruct(B, Cs)
    want = np.zeros((d, n), dtype=np.float32)
    for i in range(m):
        want += Cs[i][:, B[i].astype(np.int64) - 1]
    assert got.shape == (d, n) and got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the package's host decode agrees with it (rows <-> columns)
    K = np.ascontiguousarray(np.concatenate([c.T for c in Cs], axis=0))
    assert RC.same_bits(lsq.reconstruct_cpu((B.T - 1).astype(np.uint8), K, m), np.ascontiguousarray(want.T))
    assert RC.same_bits(RC.decode((B.T - 1).astype(np.uint8), K, m), np.ascontiguousarray(want.T))
