"""Appending rows to the resident index, the parts that need no GPU: the C ABI of lsq_index_add / lsq_index_reserve / lsq_index_get_growth_info (v2100),
the binding's structs against the header's, Index.add handing over the arrays and element types it was given (calls recorded by the stand-in of
tests/engine_calls.py), the refusals that need no device, and the host-only rules (csrc/lsq_grow_check.h: argument checks, the 2^31 - 2 bound, the
capacity arithmetic) run by the stand-alone program tools/grow_check_main.cpp under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from engine_calls import _Recorder, _offline  # noqa: E402
from packed_check import header, header_struct_fields  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lsq_index_add", "lsq_index_reserve", "lsq_index_get_growth_info")
EINVAL = -1
ADD_FIELDS = ["count", "codes", "dbnorms", "norm_codes", "base", "ldb", "list_of_row", "on_device"]
INFO_FIELDS = ["n", "capacity_rows", "adds", "rows_added", "reallocations", "adopted", "merged_rows", "append_ms", "merge_ms", "filter_ms"]


def test_header_declares_the_symbols_and_structs(lsq):
    hdr = header()
    assert int(re.search(r"#define LSQ_VERSION (\d+)", hdr).group(1)) >= 2100
    declared = set(re.findall(r"LSQ_API\s+[\w\s\*]*?\b(lsq_\w+)\s*\(", hdr))
    assert set(NEW) <= declared
    first = set(re.findall(r"\b(lsq_\w+)\s*\(\s*(?:struct\s+)?lsq_ctx\s*\*", hdr))      # none takes the context first: the context walks stay closed
    assert not first & set(NEW)
    for name in NEW:
        assert re.search(r"\b%s\s*\(\s*lsq_index\s*\*" % name, hdr), name
    assert header_struct_fields("lsq_index_add_desc") == ADD_FIELDS
    assert header_struct_fields("lsq_index_growth_info") == INFO_FIELDS
    assert "(3k)" in hdr


def test_both_libraries_export_them_at_v2100(lsq):
    assert lsq._lib.MIN_VERSION >= 2100
    for tuning in (False, True):
        L = lsq._lib.load(tuning=tuning)
        assert L.lsq_version() >= 2100
        raw = C.CDLL(lsq._lib.TUNING_LIB_PATH if tuning else lsq._lib.LIB_PATH)
        for name in NEW:
            assert hasattr(raw, name), name


def test_binding_structs_equal_the_headers(lsq):
    B = lsq._lib
    assert [f for f, _ in B.IndexAddDesc._fields_] == ADD_FIELDS
    assert [f for f, _ in B.IndexGrowthInfo._fields_] == INFO_FIELDS
    assert [t for _, t in B.IndexAddDesc._fields_] == [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    assert C.sizeof(B.IndexAddDesc) == 64                                  # int64, four pointers, int, pad, pointer, int, pad
    assert [t for _, t in B.IndexGrowthInfo._fields_] == [C.c_int64] * 7 + [C.c_double] * 3 and C.sizeof(B.IndexGrowthInfo) == 80
    assert set(NEW) <= set(B.SIGNATURES)
    assert B.SIGNATURES["lsq_index_reserve"][1] == [C.c_void_p, C.c_int64]


def test_null_handles_are_refused_without_a_device(lsq):
    L = lsq._lib.load()
    desc, info = lsq._lib.IndexAddDesc(), lsq._lib.IndexGrowthInfo()
    assert L.lsq_index_add(None, C.byref(desc)) == EINVAL and b"lsq_index_add" in L.lsq_last_error()
    assert L.lsq_index_reserve(None, 10) == EINVAL and b"lsq_index_reserve" in L.lsq_last_error()
    assert L.lsq_index_get_growth_info(None, C.byref(info)) == EINVAL and b"lsq_index_get_growth_info" in L.lsq_last_error()


class _Grown(_Recorder):
    """the recorder, with a growth info that reports n = 1234 and a copy of every add description while its call is open"""

    def __init__(self):
        super().__init__()
        self.descs = []

    def __getattr__(self, name):
        def fn(*args):
            if name == "lsq_index_get_growth_info":
                args[1]._obj.n = 1234
            if name == "lsq_index_add":
                d = args[1]._obj
                self.descs.append({f: getattr(d, f) for f, _ in d._fields_})
            self.calls.append((name, args))
            return 0
        return fn


def _offline_index(lsq, m=3, d=5, n=100, packed=False, has_codes=True, has_base=True, u8=False):
    eng = _offline(lsq.Engine)
    eng._L = _Grown()
    ix = lsq.engine.Index.__new__(lsq.engine.Index)
    ix._eng, ix._L, ix._dev, ix._h, ix._keep = eng, eng._L, False, C.c_void_p(2), None
    ix.n, ix.d, ix.m, ix._u8, ix._has_codes, ix._has_base, ix._packed = n, d, m, u8, has_codes, has_base, packed
    return ix


def test_add_passes_the_arrays_and_types_it_was_given(lsq):
    rng = np.random.default_rng(0)
    ix = _offline_index(lsq)
    codes = rng.integers(0, 256, (7, 3)).astype(np.uint8)
    dbn = rng.standard_normal(7).astype(np.float32)
    lor = rng.integers(0, 4, 7).astype(np.int32)
    wide = rng.standard_normal((7, 9)).astype(np.float32)
    base = wide[:, 2:7]                                                    # 5 columns of a 9-column buffer: pitch 9, read in place
    ix.add(codes=codes, dbnorms=dbn, base=base, assign=lor)
    (desc,) = ix._L.descs
    assert desc["count"] == 7 and desc["on_device"] == 0 and desc["ldb"] == 9
    assert desc["codes"] == codes.ctypes.data and desc["dbnorms"] == dbn.ctypes.data and desc["list_of_row"] == lor.ctypes.data
    assert desc["base"] == base.ctypes.data and desc["norm_codes"] is None
    assert [c[0] for c in ix._L.calls] == ["lsq_index_add", "lsq_index_get_growth_info"]
    assert ix.n == 1234                                                    # Index.n follows the handle
    # other element types are converted like everywhere on the host side; a float64 base becomes contiguous f32 rows
    ix._L.descs.clear()
    ix.add(codes=codes.astype(np.int64), dbnorms=dbn.astype(np.float64), base=base.astype(np.float64))
    (desc,) = ix._L.descs
    assert desc["count"] == 7 and desc["ldb"] == 5 and desc["list_of_row"] is None
    # a uint8 base index: bytes at an odd offset, read in place
    ux = _offline_index(lsq, u8=True, has_codes=False)
    buf = rng.integers(0, 256, 7 * 11 + 1).astype(np.uint8)
    view = buf[1:].reshape(7, 11)[:, :5]
    ux.add(base=view)
    (desc,) = ux._L.descs
    assert desc["base"] == buf.ctypes.data + 1 and desc["ldb"] == 11 and desc["codes"] is None and desc["count"] == 7
    # a packed index takes norm bytes
    px = _offline_index(lsq, packed=True, has_base=False)
    nc = rng.integers(0, 256, 7).astype(np.uint8)
    px.add(codes=codes, norm_codes=nc)
    (desc,) = px._L.descs
    assert desc["norm_codes"] == nc.ctypes.data and desc["dbnorms"] is None and desc["base"] is None


def test_add_refuses_what_it_would_have_to_guess(lsq):
    rng = np.random.default_rng(1)
    ix = _offline_index(lsq)
    codes = rng.integers(0, 256, (7, 3)).astype(np.uint8)
    with pytest.raises(ValueError):
        ix.add()
    with pytest.raises(TypeError):                                         # a norm byte is an index: never narrowed
        _offline_index(lsq, packed=True).add(codes=codes, norm_codes=np.arange(7))
    with pytest.raises(TypeError):                                         # the base's type is the index's own
        ix.add(codes=codes, dbnorms=np.zeros(7, np.float32), base=np.zeros((7, 5), np.uint8))
    with pytest.raises(ValueError):                                        # row counts differ
        ix.add(codes=codes, dbnorms=np.zeros(6, np.float32), base=np.zeros((7, 5), np.float32))
    with pytest.raises(ValueError):                                        # fewer than d columns
        ix.add(codes=codes, dbnorms=np.zeros(7, np.float32), base=np.zeros((7, 4), np.float32))
    with pytest.raises(ValueError):                                        # m columns of codes
        ix.add(codes=codes[:, :2], dbnorms=np.zeros(7, np.float32), base=np.zeros((7, 5), np.float32))
    assert not ix._L.descs                                 # none of them reached the library


def test_reserve_and_growth_info_reach_their_symbols(lsq):
    ix = _offline_index(lsq)
    ix.reserve(5000)
    name, args = ix._L.calls[-1]
    assert name == "lsq_index_reserve" and args[1] == 5000
    assert ix.growth_info()["n"] == 1234 and set(ix.growth_info()) == set(INFO_FIELDS)


def test_host_rules_under_the_sanitizers(tmp_path):
    """the argument rules, the 2^31 - 2 bound and the capacity arithmetic in a stand-alone program with its own main, built under
    -fsanitize=address,undefined.  The plain build stands in ONLY where the compiler says that it has no sanitizer runtime to link (then the test prints
    so); any other compile error fails the test, and so does a sanitizer report at run time"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = os.path.join(ROOT, "tools", "grow_check_main.cpp"), str(tmp_path / "grow_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", src, "-o", exe]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    sanitized = p.returncode == 0
    if not sanitized:
        missing = re.search(r"cannot find -l(asan|ubsan)|lib(asan|ubsan)[\w.\-]*: No such file|libclang_rt\.(asan|ubsan)|unsupported option '-fsanitize|unrecognized.*-fsanitize", p.stderr)
        assert missing, "the sanitized build failed for another reason than a missing runtime:\n" + p.stderr[-2000:]
        p = subprocess.run(base, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
    print("grow_check built %s" % ("under ASan + UBSan" if sanitized else "WITHOUT sanitizers: the compiler has no runtime for them (%s)" % missing.group(0)))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all passed" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    if sanitized:                                                            # the binary really carries the runtimes
        syms = subprocess.run(["nm", "-D", exe] if shutil.which("nm") else ["true"], capture_output=True, text=True).stdout
        assert not shutil.which("nm") or "asan" in syms.lower() or "__ubsan" in syms or "asan" in open(exe, "rb").read().decode("latin1").lower()
