"""Removing rows from the resident index, the parts that need no GPU: the C ABI of lsq_index_remove / lsq_index_compact / lsq_index_get_compact_info
(v2200), the binding's structs against the header's, Index.remove / compact reaching their symbols (calls recorded by the stand-in of
tests/engine_calls.py), the refusals that need no device, the host-only rules (csrc/lsq_compact_check.h) run by the stand-alone program
tools/compact_check_main.cpp under the address and undefined-behaviour sanitizers -- and the MODEL of the GPU tests held to the host checkers: the host
scan and lsq_ivf_search_cpu over the survivors' arrays equal the full ranking over all rows, filtered in numpy as tests/filter_check.py does, with the
ids mapped by new_of_old.  So the yardstick of tests/test_gpu_index_compact.py (a fresh index over the survivors) is not the code under test."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_check as FC  # noqa: E402
import index_add_check as IA  # noqa: E402
import index_compact_check as IC  # noqa: E402
import ivf_check as ic  # noqa: E402
import packed_check as PC  # noqa: E402
from engine_calls import _Recorder, _offline  # noqa: E402
from packed_check import header, header_struct_fields  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lsq_index_remove", "lsq_index_compact", "lsq_index_get_compact_info")
EINVAL = -1
DESC_FIELDS = ["old_of_new", "new_of_old", "id_base", "flags", "on_device"]
INFO_FIELDS = ["n_before", "n_after", "removes", "rows_tombstoned", "compactions", "rows_dropped", "moved_bytes", "shrunk", "tombstone_ms", "gather_ms",
               "layout_ms"]


def test_header_declares_the_symbols_and_structs(lsq):
    hdr = header()
    assert int(re.search(r"#define LSQ_VERSION (\d+)", hdr).group(1)) >= 2200
    declared = set(re.findall(r"LSQ_API\s+[\w\s\*]*?\b(lsq_\w+)\s*\(", hdr))
    assert set(NEW) <= declared
    for name in NEW:
        assert re.search(r"\b%s\s*\(\s*lsq_index\s*\*" % name, hdr), name
    assert header_struct_fields("lsq_index_compact_desc") == DESC_FIELDS
    assert header_struct_fields("lsq_index_compact_info") == INFO_FIELDS
    assert "(3l)" in hdr and re.search(r"LSQ_COMPACT_SHRINK\s*=\s*1\b", hdr)
    assert len(declared) >= 104                                              # 101 symbols before this section, three in it


def test_both_libraries_export_them_at_v2200(lsq):
    assert lsq._lib.MIN_VERSION >= 2200
    for tuning in (False, True):
        L = lsq._lib.load(tuning=tuning)
        assert L.lsq_version() >= 2200
        raw = C.CDLL(lsq._lib.TUNING_LIB_PATH if tuning else lsq._lib.LIB_PATH)
        for name in NEW:
            assert hasattr(raw, name), name


def test_binding_structs_equal_the_headers(lsq):
    B = lsq._lib
    assert [f for f, _ in B.IndexCompactDesc._fields_] == DESC_FIELDS
    assert [f for f, _ in B.IndexCompactInfo._fields_] == INFO_FIELDS
    assert [t for _, t in B.IndexCompactDesc._fields_] == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    assert C.sizeof(B.IndexCompactDesc) == 32                                # two pointers, three ints, pad
    assert [t for _, t in B.IndexCompactInfo._fields_] == [C.c_int64] * 8 + [C.c_double] * 3 and C.sizeof(B.IndexCompactInfo) == 88
    assert B.COMPACT_SHRINK == 1 and set(NEW) <= set(B.SIGNATURES)
    assert B.SIGNATURES["lsq_index_remove"][1] == [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int]


def test_null_handles_are_refused_without_a_device(lsq):
    L = lsq._lib.load()
    desc, info = lsq._lib.IndexCompactDesc(), lsq._lib.IndexCompactInfo()
    ids = np.zeros(4, np.int32)
    assert L.lsq_index_remove(None, ids.ctypes.data, 4, 0, 0) == EINVAL and b"lsq_index_remove" in L.lsq_last_error()
    assert L.lsq_index_compact(None, C.byref(desc)) == EINVAL and b"lsq_index_compact" in L.lsq_last_error()
    assert L.lsq_index_compact(None, None) == EINVAL
    assert L.lsq_index_get_compact_info(None, C.byref(info)) == EINVAL and b"lsq_index_get_compact_info" in L.lsq_last_error()


class _Filtered(_Recorder):
    """the recorder, with a filter info that reports 40 allowed rows of 100, a growth info that reports n = 40, and a copy of every compact description"""

    def __init__(self, active=1):
        super().__init__()
        self.descs, self.active = [], active

    def __getattr__(self, name):
        def fn(*args):
            if name == "lsq_index_get_filter_info":
                args[1]._obj.active, args[1]._obj.n, args[1]._obj.allowed = self.active, 100, 40
            if name == "lsq_index_get_growth_info":
                args[1]._obj.n = 40
            if name == "lsq_index_compact":
                d = args[1]._obj
                self.descs.append({f: getattr(d, f) for f, _ in d._fields_})
            self.calls.append((name, args))
            return 0
        return fn


def _offline_index(lsq, active=1):
    eng = _offline(lsq.Engine)
    eng._L = _Filtered(active)
    ix = lsq.engine.Index.__new__(lsq.engine.Index)
    ix._eng, ix._L, ix._dev, ix._h, ix._keep = eng, eng._L, False, C.c_void_p(2), None
    ix.n, ix.d, ix.m, ix._u8, ix._has_codes, ix._has_base, ix._packed = 100, 5, 3, False, True, False, False
    return ix


def test_remove_and_compact_reach_their_symbols(lsq):
    ix = _offline_index(lsq)
    ids = np.array([3, 1, 3], dtype=np.int32)
    ix.remove(ids, id_base=1)
    name, args = ix._L.calls[-1]
    assert name == "lsq_index_remove" and args[1:] == (ids.ctypes.data, 3, 1, 0)
    ix.remove(np.array([7, 8], dtype=np.int64))                              # other integer types are converted on the host side
    assert ix._L.calls[-1][1][2:] == (2, 0, 0)
    ix.remove(np.zeros(0, np.int32))                                         # nothing to remove: no address is handed over
    assert ix._L.calls[-1][1][1:] == (None, 0, 0, 0)
    with pytest.raises(ValueError):
        ix.remove(np.zeros((2, 2), np.int32))
    # compact: the map has one entry per allowed row, Index.n follows the handle
    out = ix.compact()
    (desc,) = ix._L.descs
    assert out.dtype == np.int32 and out.shape == (40,) and desc["old_of_new"] == out.ctypes.data
    assert desc["new_of_old"] is None and (desc["flags"], desc["id_base"], desc["on_device"]) == (0, 0, 0)
    assert ix.n == 40
    ix._L.descs.clear()
    assert ix.compact(shrink=True, want_map=False) is None
    (desc,) = ix._L.descs
    assert desc["old_of_new"] is None and desc["flags"] == lsq._lib.COMPACT_SHRINK
    # without a filter the map is the identity's size
    nx = _offline_index(lsq, active=0)
    assert nx.compact().shape == (100,)
    assert set(ix.compact_info()) == set(INFO_FIELDS)


def test_host_rules_under_the_sanitizers(tmp_path):
    """the argument rules, the capacity, the stream byte counts and the rank in a stand-alone program with its own main, built under
    -fsanitize=address,undefined and run directly.  The plain build stands in ONLY where the compiler says that it has no sanitizer runtime to link (then
    the test prints so); any other compile error fails the test, and so does a sanitizer report at run time"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = os.path.join(ROOT, "tools", "compact_check_main.cpp"), str(tmp_path / "compact_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", src, "-o", exe]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    sanitized = p.returncode == 0
    if not sanitized:
        missing = re.search(r"cannot find -l(asan|ubsan)|lib(asan|ubsan)[\w.\-]*: No such file|libclang_rt\.(asan|ubsan)|unsupported option '-fsanitize|unrecognized.*-fsanitize", p.stderr)
        assert missing, "the sanitized build failed for another reason than a missing runtime:\n" + p.stderr[-2000:]
        p = subprocess.run(base, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
    print("compact_check built %s" % ("under ASan + UBSan" if sanitized else "WITHOUT sanitizers: the compiler has no runtime for them (%s)" % missing.group(0)))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all passed" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# ---- the model of the GPU tests against the host checkers -----------------------------------------------------------------------------------------------
def _model_problem(nlist, packed, seed):
    """600 skewed rows with ties (rows 100 .. 139 repeat rows 0 .. 39, code row and norm) and NaN norms (every 53rd row) present"""
    P = IA.problem(600, 7 if packed else 8, 16, 9, seed, nlist=nlist)
    P["codes"][100:140], P["dbn"][100:140] = P["codes"][0:40], P["dbn"][0:40]
    P["dbn"][::53] = np.float32(np.nan)
    if packed:
        P["cb"], P["nc"] = PC.quantize(P["dbn"])
        P["dbn"] = P["cb"][P["nc"]]
    return P


def _removed(n, rng):
    """a tie's first member, a NaN row, the first and the last row, a whole bitmap word and a random third of the rest"""
    return np.unique(np.concatenate([[0, 3, 53, n - 1], np.arange(64, 96), rng.permutation(n)[: n // 3]]))


@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
@pytest.mark.parametrize("nlist", [1, 7, 300])
def test_the_model_equals_the_host_checkers(lsq, nlist, packed):
    lib = lsq._lib.load()
    P = _model_problem(nlist, packed, 900 + nlist + packed)
    n, nn = P["n"], 25
    old_of_new, new_of_old = IC.maps(n, _removed(n, np.random.default_rng(nlist)))
    allowed = new_of_old >= 0
    S = IC.sub(P, old_of_new)
    assert S["n"] == int(allowed.sum()) and np.array_equal(np.flatnonzero(allowed), old_of_new)
    assert np.isnan(S["dbn"]).any() and np.isnan(P["dbn"][~allowed]).any()   # NaN rows on both sides of the removal
    # the scan: the full ranking filtered and renumbered against the host scan over the survivors
    fd, fi = FC.filtered(*FC.full_scan(lib, P["codes"], P["K"], P["dbn"], P["Q"]), allowed, nn, 0)
    sd, si = PC.host_scan(lib, S["codes"], S["K"], S["dbn"], S["Q"], nn)
    assert np.array_equal(IA.bits(fd), IA.bits(sd)) and np.array_equal(IC.map_ids(fi, new_of_old, 1), si)
    # the inverted lists: lsq_ivf_search_cpu, the same way, with and without the coarse term
    for nprobe in sorted({1, min(3, nlist), nlist}):
        for flags in (0, 1):                                                 # LSQ_IVF_ADD_COARSE
            p = (P["codes"], P["K"], P["dbn"], P["cent"], P["lor"], P["Q"], P["Qc"])
            fd, fi = FC.filtered(*FC.full_ivf(lib, p, nprobe, flags=flags), allowed, nn, 0)
            rc, sd, si = ic.ivf_cpu(lib, S["codes"], S["K"], S["dbn"], S["cent"], S["lor"], S["Q"], S["Qc"], nprobe, nn, flags=flags)
            assert rc == 0 and np.array_equal(IA.bits(fd), IA.bits(sd)) and np.array_equal(IC.map_ids(fi, new_of_old, 1), si), (nprobe, flags)


def test_maps_and_identity_m_helper():
    old_of_new, new_of_old = IC.maps(10, [1, 1, 9, 4])
    assert old_of_new.tolist() == [0, 2, 3, 5, 6, 7, 8] and new_of_old.tolist() == [0, -1, 1, 2, -1, 3, 4, 5, 6, -1]
    assert IC.map_ids(np.array([[1, 3, 0]]), new_of_old, 1).tolist() == [[1, 2, 0]]      # 1-based, padding stays padding
    with pytest.raises(AssertionError):
        IC.map_ids(np.array([[2]]), new_of_old, 1)                           # a removed row in an answer
    d = np.array([[1.0, 2.0]], np.float32)
    before = {("search", 2): ((d, np.array([[3, 6]], np.int32)), None)}
    assert IC.held_M(before, {("search", 2): ((d, np.array([[2, 4]], np.int32)), None)}, new_of_old) == []
    assert IC.held_M(before, {("search", 2): ((d, np.array([[2, 5]], np.int32)), None)}, new_of_old) == [("search", 2)]
