"""Range search, the parts that need no GPU: the C ABI of lsq_index_range_search / lsq_index_range_fetch / lsq_index_get_range_info / lsq_range_search_cpu
(v2300), the binding's struct against the header's, Index.range_search reaching its symbols (calls recorded by the stand-in of tests/engine_calls.py), the
refusals that need no device, the host-only rules (csrc/lsq_range_check.h) run by the stand-alone program tools/range_check_main.cpp under the address and
undefined-behaviour sanitizers -- and lsq_range_search_cpu held, bit for bit, to the contract of tests/range_check.py over the full rankings of the host
checkers the project already has (the untouched host scan, lsq_ivf_search_cpu)."""
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
import ivf_check as ic  # noqa: E402
import range_check as RC  # noqa: E402
from engine_calls import _Recorder, _offline  # noqa: E402
from packed_check import header, header_struct_fields  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lsq_index_range_search", "lsq_index_range_fetch", "lsq_index_get_range_info", "lsq_range_search_cpu")
EINVAL = -1
INFO_FIELDS = ["queries", "rows_walked", "results", "max_per_query", "batches", "road", "held_bytes", "coarse_ms", "lut_ms", "count_ms", "fill_ms", "sort_ms"]
H = 256


def test_header_declares_the_symbols_and_struct(lsq):
    hdr = header()
    assert int(re.search(r"#define LSQ_VERSION (\d+)", hdr).group(1)) >= 2300
    declared = set(re.findall(r"LSQ_API\s+[\w\s\*]*?\b(lsq_\w+)\s*\(", hdr))
    assert set(NEW) <= declared
    for name in NEW[:3]:
        assert re.search(r"\b%s\s*\(\s*lsq_index\s*\*" % name, hdr), name
    assert header_struct_fields("lsq_range_info") == INFO_FIELDS
    assert "(3m)" in hdr and '"range_batch"' in hdr
    assert len(declared) >= 108                                              # 104 symbols before this section, four in it


def test_both_libraries_export_them_at_v2300(lsq):
    assert lsq._lib.MIN_VERSION >= 2300
    for tuning in (False, True):
        L = lsq._lib.load(tuning=tuning)
        assert L.lsq_version() >= 2300
        raw = C.CDLL(lsq._lib.TUNING_LIB_PATH if tuning else lsq._lib.LIB_PATH)
        for name in NEW:
            assert hasattr(raw, name), name


def test_binding_struct_equals_the_headers(lsq):
    B = lsq._lib
    assert [f for f, _ in B.RangeInfo._fields_] == INFO_FIELDS
    assert [t for _, t in B.RangeInfo._fields_] == [C.c_int64] * 7 + [C.c_double] * 5 and C.sizeof(B.RangeInfo) == 96
    assert set(NEW) <= set(B.SIGNATURES)
    assert B.SIGNATURES["lsq_index_range_search"][1] == [C.c_void_p] * 5 + [C.c_int] * 5
    assert B.SIGNATURES["lsq_index_range_fetch"][1] == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
    assert len(B.SIGNATURES["lsq_range_search_cpu"][1]) == 23


def test_null_handles_are_refused_without_a_device(lsq):
    L = lsq._lib.load()
    info = lsq._lib.RangeInfo()
    lims, q, r = np.zeros(2, np.int64), np.zeros(4, np.float32), np.zeros(1, np.float32)
    assert L.lsq_index_range_search(None, lims.ctypes.data, q.ctypes.data, None, r.ctypes.data, 1, 4, 0, 0, 0) == EINVAL
    assert b"lsq_index_range_search" in L.lsq_last_error()
    assert L.lsq_index_range_fetch(None, q.ctypes.data, lims.ctypes.data, 1, 0) == EINVAL and b"lsq_index_range_fetch" in L.lsq_last_error()
    assert L.lsq_index_get_range_info(None, C.byref(info)) == EINVAL and b"lsq_index_get_range_info" in L.lsq_last_error()
    assert np.all(lims == 0) and np.all(q == 0)                              # nothing was written


class _Ranged(_Recorder):
    """the recorder, with a range info that reports five results"""

    def __getattr__(self, name):
        def fn(*args):
            if name == "lsq_index_get_range_info":
                args[1]._obj.results = 5
            self.calls.append((name, args))
            return 0
        return fn


def _offline_index(lsq):
    eng = _offline(lsq.Engine)
    eng._L = _Ranged()
    ix = lsq.engine.Index.__new__(lsq.engine.Index)
    ix._eng, ix._L, ix._dev, ix._h, ix._keep = eng, eng._L, False, C.c_void_p(2), None
    ix.n, ix.d, ix.m, ix._u8, ix._has_codes, ix._has_base, ix._packed = 100, 5, 3, False, True, False, False
    return ix


def test_range_search_reaches_its_symbols(lsq):
    ix = _offline_index(lsq)
    Q = np.arange(15, dtype=np.float32).reshape(3, 5)
    lims, dists, ids = ix.range_search(Q, 2.5)
    names = [c[0] for c in ix._L.calls]
    assert names == ["lsq_index_range_search", "lsq_index_get_range_info", "lsq_index_range_fetch"]      # one search, the size, one fetch
    search, fetch = ix._L.calls[0][1], ix._L.calls[2][1]
    assert lims.dtype == np.int64 and lims.shape == (4,) and search[1] == lims.ctypes.data and search[2] == Q.ctypes.data
    assert search[3] is None and search[5:] == (3, 5, 0, 0, 0)               # nprobe == 0: no coarse queries, no flag, host form
    assert dists.dtype == np.float32 and ids.dtype == np.int32 and dists.shape == ids.shape == (5,)      # exactly the reported size
    assert fetch[1:] == (dists.ctypes.data, ids.ctypes.data, 5, 0)
    # a per-query radius, the list road with its coarse queries and the flag
    ix._L.calls.clear()
    rad = np.array([1, np.inf, np.nan], dtype=np.float32)
    Qc = Q + 1
    ix.range_search(Q, rad, nprobe=4, Q_coarse=Qc, add_coarse=True)
    search = ix._L.calls[0][1]
    assert search[3] == Qc.ctypes.data and search[4] == rad.ctypes.data and search[5:] == (3, 5, 4, lsq._lib.IVF_ADD_COARSE, 0)
    ix._L.calls.clear()
    ix.range_search(Q, rad, nprobe=2)                                         # default coarse queries: the scan's
    assert ix._L.calls[0][1][3] == Q.ctypes.data
    with pytest.raises(ValueError):
        ix.range_search(Q, np.zeros(4, np.float32))                          # one radius per query
    with pytest.raises(ValueError):
        ix.range_search(np.zeros((3, 4), np.float32), 1.0)                   # d columns
    assert set(ix.range_info()) == set(INFO_FIELDS)


def test_host_rules_under_the_sanitizers(tmp_path):
    """the argument rules, the prefix and the batch cutting (a query over the budget, zero counts, one query, budget 1) in a stand-alone program with its
    own main, built under -fsanitize=address,undefined and run directly.  The plain build stands in ONLY where the compiler says that it has no sanitizer
    runtime to link (then the test prints so); any other compile error fails the test, and so does a sanitizer report at run time"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = os.path.join(ROOT, "tools", "range_check_main.cpp"), str(tmp_path / "range_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", src, "-o", exe]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    sanitized = p.returncode == 0
    if not sanitized:
        missing = re.search(r"cannot find -l(asan|ubsan)|lib(asan|ubsan)[\w.\-]*: No such file|libclang_rt\.(asan|ubsan)|unsupported option '-fsanitize|unrecognized.*-fsanitize", p.stderr)
        assert missing, "the sanitized build failed for another reason than a missing runtime:\n" + p.stderr[-2000:]
        p = subprocess.run(base, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
    print("range_check built %s" % ("under ASan + UBSan" if sanitized else "WITHOUT sanitizers: the compiler has no runtime for them (%s)" % missing.group(0)))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all passed" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# ---- lsq_range_search_cpu against the contract -----------------------------------------------------------------------------------------------------------
def _scan_problem(n, m, d, nq, seed):
    rng = np.random.default_rng(seed)
    K = (rng.standard_normal((m * H, d)) / np.sqrt(m)).astype(np.float32)
    codes = rng.integers(0, H, (n, m)).astype(np.uint8)
    recon = sum(K[j * H + codes[:, j].astype(np.int64)] for j in range(m))
    dbn = (recon.astype(np.float64) ** 2).sum(1).astype(np.float32)
    return codes, K, dbn, rng.standard_normal((nq, d)).astype(np.float32)


def _check_all_radii(lib, full, pad_id, seen, **cpu_args):
    """every case of range_check.radii against range_of(full); seen: the non-vacuity counters"""
    for name, rad in RC.radii(full[0]).items():
        want = RC.range_of(*full, rad, pad_id)
        rc, lims, dists, ids = RC.range_cpu(lib, radius=rad, **cpu_args)
        assert rc == 0 and RC.same((lims, dists, ids), want), name
        counts = np.diff(want[0])
        seen["empty"] += int((counts == 0).sum())
        seen["pairs"] += int(want[0][-1])
        seen["most"] = max(seen["most"], int(counts.max()))
        seen["ties"] += RC.tie_cut_at_last_member(*full, rad, pad_id)


@pytest.mark.parametrize("m", [5, 8, 16])
def test_cpu_every_row_equals_the_prefix_of_the_host_scan(lsq, m):
    lib = lsq._lib.load()
    n, nq, d = 1000, 37, 24
    codes, K, dbn, Q = _scan_problem(n, m, d, nq, 300 + m)
    full = FC.full_scan(lib, codes, K, dbn, Q)
    seen = {"empty": 0, "pairs": 0, "most": 0, "ties": 0}
    _check_all_radii(lib, full, 0, seen, codes=codes, K=K, dbn=dbn, Q=Q)
    assert seen["empty"] >= 3 * nq and seen["most"] == n and seen["pairs"] > 10 ** 4, seen      # -inf, NaN, below-min: nothing; +inf: all n rows
    # a single thread and many give the same bits
    rad = RC.radii(full[0])["half"]
    a, b = RC.range_cpu(lib, codes, K, dbn, Q, rad, nthreads=1), RC.range_cpu(lib, codes, K, dbn, Q, rad, nthreads=7)
    assert RC.same(a[1:], b[1:])


def test_cpu_ties_straddle_the_radius(lsq):
    lib = lsq._lib.load()
    codes, K, dbn, cent, lor, Qs, Qc = ic.problem(1000, 5, 8, 16, 37, 41, small_int=True)
    full = FC.full_scan(lib, codes, K, dbn, Qs)
    seen = {"empty": 0, "pairs": 0, "most": 0, "ties": 0}
    _check_all_radii(lib, full, 0, seen, codes=codes, K=K, dbn=dbn, Q=Qs)
    assert seen["ties"] > 0, seen                                            # a radius equal to a tied distance: the group is cut at its last member
    # ... and one float below the tied distance leaves the whole group out
    rad = RC.radii(full[0])["10th"]
    below = np.nextafter(rad, np.float32(-np.inf)).astype(np.float32)
    at, under = RC.range_of(*full, rad, 0), RC.range_of(*full, below, 0)
    assert np.all(np.diff(at[0]) > np.diff(under[0]))
    rc, lims, dists, ids = RC.range_cpu(lib, codes, K, dbn, Qs, below)
    assert rc == 0 and RC.same((lims, dists, ids), under)


@pytest.mark.parametrize("add_coarse", [False, True], ids=["plain", "add-coarse"])
@pytest.mark.parametrize("nprobe", [1, 4, 16])
def test_cpu_probed_lists_equal_the_prefix_of_lsq_ivf_search_cpu(lsq, nprobe, add_coarse):
    lib = lsq._lib.load()
    p = ic.problem(1000, 24, 8, 16, 37, 43)                                  # 16 skewed lists: empty ones, one-row ones, one of half the base
    codes, K, dbn, cent, lor, Qs, Qc = p
    assert np.bincount(lor, minlength=16).min() == 0
    flags = ic.ADD_COARSE if add_coarse else 0
    full = FC.full_ivf(lib, p, nprobe, flags=flags)
    seen = {"empty": 0, "pairs": 0, "most": 0, "ties": 0}
    _check_all_radii(lib, full, 0, seen, codes=codes, K=K, dbn=dbn, Q=Qs, cent=cent, lor=lor, nprobe=nprobe, flags=flags, Qc=Qc)
    assert seen["empty"] > 0 and seen["pairs"] > 0
    if nprobe == 16 and not add_coarse:                                      # every list probed, no flag: the every-row result
        rad = RC.radii(full[0])["half"]
        a = RC.range_cpu(lib, codes, K, dbn, Qs, rad, cent=cent, lor=lor, nprobe=16, Qc=Qc)
        b = RC.range_cpu(lib, codes, K, dbn, Qs, rad)
        assert RC.same(a[1:], b[1:]) and seen["most"] == 1000


def test_cpu_allowed_mask_and_nan_norms(lsq):
    lib = lsq._lib.load()
    n, nq = 1000, 37
    codes, K, dbn, Q = _scan_problem(n, 8, 24, nq, 47)
    dbn[::53] = np.float32(np.nan)
    full = FC.full_scan(lib, codes, K, dbn, Q)
    # NaN rows are never returned, not even at r = +inf; a NaN radius returns nothing
    rc, lims, dists, ids = RC.range_cpu(lib, codes, K, dbn, Q, np.inf)
    assert rc == 0 and np.all(np.diff(lims) == n - len(range(0, n, 53))) and not np.isnan(dists).any() and not np.isin(ids - 1, np.arange(0, n, 53)).any()
    assert RC.same((lims, dists, ids), RC.range_of(*full, np.inf, 0))
    rc, lims, dists, ids = RC.range_cpu(lib, codes, K, dbn, Q, np.nan)
    assert rc == 0 and lims[-1] == 0
    for name, allowed in FC.masks(n).items():
        ranked = FC.filtered(*full, allowed, n, 0)                           # the full ranking of the allowed rows, then (+inf, 0)
        for rname in ("+inf", "half", "10th"):
            rad = RC.radii(full[0])[rname]
            rc, lims, dists, ids = RC.range_cpu(lib, codes, K, dbn, Q, rad, allowed=allowed)
            assert rc == 0 and RC.same((lims, dists, ids), RC.range_of(*ranked, rad, 0)), (name, rname)


def test_cpu_two_call_protocol_and_refusals(lsq):
    lib = lsq._lib.load()
    codes, K, dbn, Q = _scan_problem(200, 5, 8, 9, 51)
    full = FC.full_scan(lib, codes, K, dbn, Q)
    rad = RC.radii(full[0])["half"]
    want = RC.range_of(*full, rad, 0)
    total = int(want[0][-1])
    assert total > 1
    # capacity = total - 1: lims is written, the poisoned outputs are untouched
    rc, lims, dists, ids = RC.range_cpu(lib, codes, K, dbn, Q, rad, capacity=total - 1, poison=-77)
    assert rc == 0 and np.array_equal(lims, want[0]) and np.all(dists == -77) and np.all(ids == -77)
    # capacity = total (and more): written
    rc, lims, dists, ids = RC.range_cpu(lib, codes, K, dbn, Q, rad, capacity=total + 3, poison=-77)
    assert rc == 0 and RC.same((lims, dists[:total], ids[:total]), want) and np.all(dists[total:] == -77) and np.all(ids[total:] == -77)
    # refusals: nothing is written
    cent, lor = np.zeros((4, 8), np.float32), np.zeros(200, np.int32)
    for kw in (dict(nprobe=-1), dict(nprobe=1), dict(flags=ic.ADD_COARSE), dict(flags=2, nprobe=1, cent=cent, lor=lor), dict(nprobe=5, cent=cent, lor=lor),
               dict(nprobe=1, cent=cent, lor=np.full(200, 4, np.int32)), dict(capacity=-1)):
        rc, lims, dists, ids = RC.range_cpu(lib, codes, K, dbn, Q, rad, **{"capacity": 0, **kw})
        assert rc == EINVAL and np.all(lims == -7) and b"lsq_range_search_cpu" in lib.lsq_last_error(), kw
    # nq == 0
    rc, lims, dists, ids = RC.range_cpu(lib, codes, K, dbn, Q[:0], np.zeros(0, np.float32))
    assert rc == 0 and lims.tolist() == [0]


def test_range_search_lsq_is_the_host_road(lsq):
    lib = lsq._lib.load()
    p = ic.problem(300, 8, 4, 7, 5, 59)
    codes, K, dbn, cent, lor, Qs, Qc = p
    Cs = [np.ascontiguousarray(K[j * H:(j + 1) * H].T) for j in range(4)]
    R = np.eye(8, dtype=np.float32)
    full = FC.full_scan(lib, codes, K, dbn, Qs)
    rad = RC.radii(full[0])["10th"]
    got = lsq.range_search_lsq(codes.T, Qs.T, Cs, dbn, R, rad)
    assert RC.same(got, RC.range_of(*full, rad, 0))
    fi = FC.full_ivf(lib, p, 3, flags=ic.ADD_COARSE)
    rad = RC.radii(fi[0])["10th"]
    got = lsq.range_search_lsq(codes.T, Qs.T, Cs, dbn, R, rad, centroids=cent.T, assign=lor, nprobe=3, add_coarse=True, X_coarse=Qc.T)
    assert RC.same(got, RC.range_of(*fi, rad, 0))
    allowed = np.arange(300) % 3 == 0
    got = lsq.range_search_lsq(codes.T, Qs.T, Cs, dbn, R, np.float32(np.inf), allowed=allowed)
    assert RC.same(got, RC.range_of(*FC.filtered(*full, allowed, 300, 0), np.inf, 0))
