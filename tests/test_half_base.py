"""Half-precision base rows, the parts that need no GPU: the C ABI of lsq_narrow_rows_cpu, lsq_index_narrow_base, lsq_index_get_base and
lsq_index_get_base_info (v2500), the binding's struct against the header's, lsq_narrow_rows_cpu held bit for bit to the numpy contract of
tests/half_check.py (Identity N), lsq_rerank_cpu / lsq_knn_exact_u8_cpu on half rows held to the same call on the widened matrix (Identity W), the binding's
refusals -- all before any library call, recorded by the stand-in of tests/engine_calls.py -- and the host-only rules (csrc/lsq_half_check.h) run by the
stand-alone program tools/half_check_main.cpp under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import half_check as HC  # noqa: E402
from engine_calls import offline_engine  # noqa: E402
from packed_check import header, header_struct_fields  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lsq_narrow_rows_cpu", "lsq_index_narrow_base", "lsq_index_get_base", "lsq_index_get_base_info")
INFO_FIELDS = ["format", "elem_bytes", "ldb", "owned", "resident_bytes", "to_inf", "to_zero", "nans", "narrow_ms"]
EINVAL = -1
SENTINEL = 0xABCD


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_symbols_the_formats_and_the_struct(lsq):
    hdr = header()
    assert int(re.search(r"#define LSQ_VERSION (\d+)", hdr).group(1)) >= 2500
    declared = re.findall(r"LSQ_API\s+[\w\s\*]*?\b(lsq_\w+)\s*\(", hdr)
    assert set(NEW) <= set(declared) and len(declared) == len(set(declared))
    assert len(declared) >= 116                                              # 112 symbols before this section, four in it
    for name in NEW[1:]:
        assert re.search(r"\b%s\s*\(\s*lsq_index\s*\*" % name, hdr), name    # everything goes through the index: no new context-first symbol
    assert not re.search(r"\blsq_narrow_rows_cpu\s*\(\s*(struct\s+)?lsq_ctx", hdr)
    assert re.search(r"#define LSQ_BASE_F16 2\b", hdr) and re.search(r"#define LSQ_BASE_BF16 3\b", hdr)
    assert header_struct_fields("lsq_index_base_info") == INFO_FIELDS
    assert "(3o)" in hdr and "IDENTITY W" in hdr and "IDENTITY N" in hdr and "OLD\n *                           PLUS NEW" in hdr
    # the layouts of the descriptions are ABI: the format lives in the field that was the uint8 flag
    assert header_struct_fields("lsq_index_desc") == ["n", "d", "m", "h", "codes", "codebooks", "dbnorms", "base", "base_u8", "ldb", "on_device"]
    assert header_struct_fields("lsq_index_packed_desc")[-4:] == ["base", "base_u8", "ldb", "on_device"]


def test_both_libraries_export_them_at_v2500(lsq):
    assert lsq._lib.MIN_VERSION >= 2500
    for tuning in (False, True):
        L = lsq._lib.load(tuning=tuning)
        assert L.lsq_version() >= 2500
        raw = C.CDLL(lsq._lib.TUNING_LIB_PATH if tuning else lsq._lib.LIB_PATH)
        for name in NEW:
            assert hasattr(raw, name), name


def test_binding_agrees_with_the_header(lsq):
    B = lsq._lib
    assert [f for f, _ in B.IndexBaseInfo._fields_] == INFO_FIELDS
    assert [t for _, t in B.IndexBaseInfo._fields_] == [C.c_int64] * 8 + [C.c_double] and C.sizeof(B.IndexBaseInfo) == 72
    assert set(NEW) <= set(B.SIGNATURES) and len(B.SIGNATURES) >= 116
    vp, i, i64 = C.c_void_p, C.c_int, C.c_int64
    assert B.SIGNATURES["lsq_narrow_rows_cpu"][1] == [vp, vp, i64, i, i64, i64, i, i]
    assert B.SIGNATURES["lsq_index_narrow_base"][1] == [vp, i]
    assert B.SIGNATURES["lsq_index_get_base"][1] == [vp, vp, i64, i64, i64, i]
    assert (B.BASE_F32, B.BASE_U8, B.BASE_F16, B.BASE_BF16) == (0, 1, 2, 3) == (0, 1, HC.F16, HC.BF16)
    assert C.sizeof(B.IndexDesc) == 72 and C.sizeof(B.IndexPackedDesc) == 88     # unchanged by the format
    assert "narrow_rows" in lsq.__all__
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "116 symbols" in f.read()


def test_null_handles_are_refused_without_a_device(lsq):
    L = lsq._lib.load()
    info = lsq._lib.IndexBaseInfo()
    out = np.zeros(8, np.float32)
    assert L.lsq_index_narrow_base(None, 2) == EINVAL and b"lsq_index_narrow_base" in L.lsq_last_error()
    assert L.lsq_index_get_base(None, out.ctypes.data, 0, 2, 4, 0) == EINVAL and b"lsq_index_get_base" in L.lsq_last_error()
    assert L.lsq_index_get_base_info(None, C.byref(info)) == EINVAL and b"lsq_index_get_base_info" in L.lsq_last_error()
    assert np.all(out == 0)


# ---- Identity N: lsq_narrow_rows_cpu against the numpy contract -----------------------------------------------------------------------------------------
def _narrow_cpu(lib, X, fmt, ldd, nthreads=1):
    n, d = X.shape
    dst = np.full((n, ldd), SENTINEL, dtype=np.uint16)
    lds = X.strides[0] // 4 if n > 1 else d
    rc = lib.lsq_narrow_rows_cpu(dst.ctypes.data, X.ctypes.data, n, d, lds, ldd, HC.FORMATS[fmt], nthreads)
    return rc, dst


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
@pytest.mark.parametrize("d", [1, 7, 8, 9])
def test_cpu_narrowing_equals_the_contract(lsq, fmt, d):
    lib = lsq._lib.load()
    rng = np.random.default_rng(100 * d + HC.FORMATS[fmt])
    x = np.concatenate([HC.edge_values(), HC.random_floats(rng, 10000)])
    n = len(x) // d
    for lds, ldd in ((d, d), (d + 3, d + 2), (d + 1, d + 5)):                # padded source and destination pitches
        big = np.full((n, lds), np.float32(np.nan))                          # NaN between the rows: a component read past d would show
        big[:, :d] = x[:n * d].reshape(n, d)
        X = big[:, :d]
        for nt in (1, 3):
            rc, dst = _narrow_cpu(lib, X, fmt, ldd, nt)
            assert rc == 0
            assert HC.same_halves(np.ascontiguousarray(dst[:, :d]), HC.narrow(X, fmt), fmt)
            assert np.all(dst[:, d:] == SENTINEL)                            # the gaps between destination rows are not written
    # every edge value by itself, and what it widens back to
    e = HC.edge_values().reshape(-1, 1)
    rc, dst = _narrow_cpu(lib, np.ascontiguousarray(e), fmt, 1)
    want = HC.narrow(e, fmt)
    assert rc == 0 and HC.same_halves(dst, want, fmt) and HC.same_bits(HC.widen(dst, fmt), HC.widen(want, fmt))
    # the package's host function is this call
    got = lsq.narrow_rows(big[:, :d], fmt)
    assert got.dtype == HC.HOST_DTYPE[fmt] and got.shape == (n, d) and HC.same_halves(got, HC.narrow(big[:, :d], fmt), fmt)


def test_contract_says_what_the_issue_pins():
    """the numpy statement itself: the pinned values of Identity N"""
    f = lambda u: HC.from_bits(np.array([u], np.uint32))                     # noqa: E731
    h16 = lambda u: int(HC.half_bits(HC.narrow_f16(f(u)))[0])                # noqa: E731
    b16 = lambda u: int(HC.narrow_bf16(f(u))[0])                             # noqa: E731
    assert h16(0x477FE000) == 0x7BFF and h16(0x477FEFFF) == 0x7BFF and h16(0x477FF000) == 0x7C00      # 65504, 65519.99, 65520
    assert h16(0x33000000) == 0 and h16(0x33000001) == 1 and h16(0x387FC000) == 0x03FF and h16(0x38800000) == 0x0400      # subnormals are kept
    assert h16(0x3F801000) == 0x3C00 and h16(0x3F803000) == 0x3C02           # ties to even
    assert b16(0x3F7FFFFF) == 0x3F80 and b16(0x7F7FFFFF) == 0x7F80           # the carry into the exponent; f32 max -> inf
    assert b16(0x3F808000) == 0x3F80 and b16(0x3F818000) == 0x3F82 and b16(0x00018000) == 0x0002
    assert np.isnan(HC.widen(HC.narrow_bf16(f(0x7F800001)), "bf16"))[0] and np.isnan(HC.widen(HC.narrow_f16(f(0x7F800001)), "f16"))[0]
    x = np.array([65520.0, 1e-30, 0.0, np.nan, 1.0, -1e30], np.float32)
    assert HC.counts(x, "f16") == (2, 1, 1) and HC.counts(x, "bf16") == (0, 0, 1)


def test_bf16_rule_is_torchs(lsq):
    import torch
    rng = np.random.default_rng(7)
    x = np.concatenate([HC.edge_values(), HC.random_floats(rng, 10000)])
    x = x[~np.isnan(x)]
    t = torch.tensor(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(t, HC.narrow_bf16(x))
    assert np.array_equal(HC.half_bits(lsq.narrow_rows(x.reshape(-1, 1), "bf16")).reshape(-1), t)
    t16 = torch.tensor(x).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(t16, HC.half_bits(HC.narrow_f16(x)))


def test_cpu_narrowing_refusals_write_nothing(lsq):
    lib = lsq._lib.load()
    src = np.ones((3, 4), np.float32)
    dst = np.full((3, 4), SENTINEL, np.uint16)
    f = lambda **kw: lib.lsq_narrow_rows_cpu(*[kw.get(k, v) for k, v in (      # noqa: E731
        ("dst", dst.ctypes.data), ("src", src.ctypes.data), ("n", 3), ("d", 4), ("lds", 4), ("ldd", 4), ("format", 2), ("nt", 1))])
    for bad in (dict(format=0), dict(format=1), dict(format=7), dict(n=-1), dict(d=0), dict(lds=3), dict(ldd=3), dict(dst=None), dict(src=None),
                dict(dst=dst.ctypes.data + 1), dict(src=src.ctypes.data + 2)):
        assert f(**bad) == EINVAL, bad
        assert b"lsq_narrow_rows_cpu" in lib.lsq_last_error() and np.all(dst == SENTINEL), bad
    assert f(n=0, dst=None, src=None) == 0
    assert f() == 0 and np.all(dst == 0x3C00)


# ---- Identity W on the host checkers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f16", "bf16"])
@pytest.mark.parametrize("d", [1, 17, 64, 65])
def test_cpu_rerank_and_knn_on_half_rows_equal_the_widened_call(lsq, fmt, d):
    lib = lsq._lib.load()
    n, nq, L, k = 200, 5, 60, 10
    rng = np.random.default_rng(1000 * d + HC.FORMATS[fmt])
    X = HC.matrix(rng, n, d)
    special = HC.special_rows(X, rng)
    H = HC.narrow(X, fmt)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    cand = rng.integers(-2, n + 2, (nq, L)).astype(np.int32)                 # ids outside the base among them
    cand[:, :5] = special
    for ldb in (d + 1, d + 2):                                               # an odd and an even pitch (one of each, whatever d is)
        Hp = np.zeros((n, ldb), dtype=H.dtype)
        Hp[:, :d] = H
        Hp.view(np.uint16)[:, d:] = 0x7E00 if fmt == "f16" else 0x7FC0       # NaN in the padding columns
        W = np.full((n, ldb), np.float32(np.nan))
        W[:, :d] = HC.widen(H, fmt)

        def rerank(base, code):
            dd, ii = np.zeros((nq, k), np.float32), np.zeros((nq, k), np.int32)
            assert lib.lsq_rerank_cpu(dd.ctypes.data, ii.ctypes.data, base.ctypes.data, code, Q.ctypes.data, cand.ctypes.data, n, nq, d, ldb, d, L, k, 0, 2) == 0
            return dd, ii

        def knn(base, code, kk):
            dd, ii = np.zeros((nq, kk), np.float32), np.zeros((nq, kk), np.uint32)
            assert lib.lsq_knn_exact_u8_cpu(dd.ctypes.data, ii.ctypes.data, base.ctypes.data, code, Q.ctypes.data, 0, n, nq, d, ldb, d, kk, 2) == 0
            return dd, ii

        (gd, gi), (wd, wi) = rerank(Hp, HC.FORMATS[fmt]), rerank(W, 0)
        assert HC.same_bits(gd, wd) and np.array_equal(gi, wi)
        assert np.isfinite(gd[:, 0]).all() and not np.isnan(gd[:, :3]).any()
        for kk in (1, k, n):
            (gd, gi), (wd, wi) = knn(Hp, HC.FORMATS[fmt], kk), knn(W, 0, kk)
            assert HC.same_bits(gd, wd) and np.array_equal(gi, wi)
        assert np.isnan(gd[:, -1]).all()                                     # k = n: the NaN row comes last
    # a half base at an odd address is refused (uint8 rows may lie anywhere, f32 rows are the caller's to align as before)
    raw = np.zeros(2 * n * d + 2, np.uint8)
    dd, ii = np.zeros((nq, k), np.float32), np.zeros((nq, k), np.int32)
    assert lib.lsq_rerank_cpu(dd.ctypes.data, ii.ctypes.data, raw.ctypes.data + 1, HC.FORMATS[fmt], Q.ctypes.data, cand.ctypes.data, n, nq, d, d, d, L, k, 0, 1) == EINVAL


def test_other_non_zero_formats_still_mean_uint8(lsq):
    lib = lsq._lib.load()
    rng = np.random.default_rng(3)
    n, nq, d, L, k = 50, 3, 9, 20, 5
    X8 = rng.integers(0, 256, (n, d), dtype=np.uint8)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    cand = rng.integers(0, n, (nq, L)).astype(np.int32)
    res = []
    for code in (1, 4, 255, -1):
        dd, ii = np.zeros((nq, k), np.float32), np.zeros((nq, k), np.int32)
        assert lib.lsq_rerank_cpu(dd.ctypes.data, ii.ctypes.data, X8.ctypes.data, code, Q.ctypes.data, cand.ctypes.data, n, nq, d, d, d, L, k, 0, 1) == 0
        res.append((dd, ii))
    assert all(np.array_equal(res[0][0], r[0]) and np.array_equal(res[0][1], r[1]) for r in res[1:])


# ---- the binding: refusals before any library call, and what reaches the library -----------------------------------------------------------------------
def _created(eng):
    """(symbol, description) of the one create call the stand-in recorded"""
    made = [(name, args[2]._obj) for name, args in eng._L.calls if name in ("lsq_index_create", "lsq_index_create_packed")]
    assert len(made) == 1
    return made[0]


def test_python_refusals_happen_before_any_library_call(lsq):
    rng = np.random.default_rng(5)
    X = rng.standard_normal((20, 6)).astype(np.float32)
    codes = rng.integers(0, 256, (20, 2), dtype=np.uint8)
    K = rng.standard_normal((2 * 256, 6)).astype(np.float32)
    nc, cb = rng.integers(0, 4, 20, dtype=np.uint8), rng.standard_normal(4).astype(np.float32)
    eng = offline_engine(lsq)
    cases = [
        (ValueError, dict(base=X, base_format="fp16")),                      # a bad format string
        (ValueError, dict(base=X, base_format=2)),
        (ValueError, dict(base=X, base_format="F16")),
        (TypeError, dict(base=X.view(np.int16)[:, :6], base_format="bf16")),   # bf16 bits that are not uint16
        (TypeError, dict(base=X.astype(np.int32), base_format="bf16")),
        (TypeError, dict(base=X.view(np.uint8)[:, :6], base_format="bf16")),
        (TypeError, dict(base=X.view(np.uint16)[:, :6], base_format="f16")),   # f16 rows are float16, not bits
        (TypeError, dict(base=X.astype(np.int8), base_format="f16")),        # int8
        (TypeError, dict(base=X.astype(np.int8), base_format="bf16")),
        (ValueError, dict(base=None, base_format="f16")),                    # a format without rows
    ]
    for exc, kw in cases:
        base = kw.pop("base")
        with pytest.raises(exc):
            eng.index(codes, K, np.zeros(20, np.float32), 2, base=base, **kw)
        with pytest.raises(exc):
            eng.index_packed(codes, K, nc, cb, 2, base=base, **kw)
        with pytest.raises(exc):
            eng.index(None, None, None, 0, base=base, **kw) if base is not None else eng.index(codes, K, np.zeros(20, np.float32), 2, **kw)
    assert eng._L.calls == []                                                # nothing reached the library
    with pytest.raises(ValueError):
        lsq.narrow_rows(X, "half")
    with pytest.raises(ValueError):
        lsq.narrow_rows(X, None)
    with pytest.raises(ValueError):
        lsq.linscan_lsq_rerank(None, None, None, None, None, None, 10, 5, base_format="f16")      # the host road keeps no resident base


def test_what_reaches_the_library(lsq):
    B = lsq._lib
    rng = np.random.default_rng(6)
    X = rng.standard_normal((20, 6)).astype(np.float32)
    # base_format=None with a float16 host array: still an f32 base, as ever
    eng = offline_engine(lsq)
    ix = eng.index(None, None, None, 0, base=X.astype(np.float16))
    name, desc = _created(eng)
    assert name == "lsq_index_create" and desc.base_u8 == B.BASE_F32 and desc.ldb == 6 and [c[0] for c in eng._L.calls] == ["lsq_index_create"]
    assert np.array_equal(np.ctypeslib.as_array(C.cast(desc.base, C.POINTER(C.c_float)), (20, 6)), X.astype(np.float16).astype(np.float32))
    assert ix._format() == B.BASE_F32
    # a format with float rows: narrowed by lsq_narrow_rows_cpu first, then created with the format (the stand-in records the call, it does not narrow)
    for fmt, code, dtype in (("f16", B.BASE_F16, np.float16), ("bf16", B.BASE_BF16, np.uint16)):
        eng = offline_engine(lsq)
        ix = eng.index(None, None, None, 0, base=X, base_format=fmt)
        assert [c[0] for c in eng._L.calls] == ["lsq_narrow_rows_cpu", "lsq_index_create"]
        nargs = eng._L.calls[0][1]
        assert nargs[1] == X.ctypes.data and nargs[2:] == (20, 6, 6, 6, code, 0)
        name, desc = _created(eng)
        assert desc.base_u8 == code and desc.ldb == 6 and desc.base == nargs[0] and ix._format() == code and ix._keep[-1].dtype == dtype
        # rows already in the format are taken as they are: a row view in place, at its own pitch
        big = np.zeros((20, 9), dtype=dtype)
        eng = offline_engine(lsq)
        ix = eng.index(None, None, None, 0, base=big[:, 1:7], base_format=fmt)
        name, desc = _created(eng)
        assert [c[0] for c in eng._L.calls] == ["lsq_index_create"] and desc.base == big.ctypes.data + 2 and desc.ldb == 9 and desc.base_u8 == code
        # add: float rows are narrowed, rows in the format pass, anything else is refused before the library
        eng._L.calls.clear()
        ix.add(base=X[:3])
        assert [c[0] for c in eng._L.calls][:2] == ["lsq_narrow_rows_cpu", "lsq_index_add"]
        eng._L.calls.clear()
        ix.add(base=big[:3, 1:7])
        assert [c[0] for c in eng._L.calls][:1] == ["lsq_index_add"] and eng._L.calls[0][1][1]._obj.base == big.ctypes.data + 2 and eng._L.calls[0][1][1]._obj.ldb == 9
        eng._L.calls.clear()
        with pytest.raises(TypeError):
            ix.add(base=np.zeros((3, 6), np.uint8))
        assert eng._L.calls == []
        # narrow_base, base_info, base_rows reach their symbols
        ix.n = 20                                                            # (add read n from the stand-in's empty growth info)
        ix.narrow_base(fmt)
        out = ix.base_rows(start=5)
        info = ix.base_info()
        assert [c[0] for c in eng._L.calls] == ["lsq_index_narrow_base", "lsq_index_get_base", "lsq_index_get_base_info"]
        assert eng._L.calls[0][1][1:] == (code,) and eng._L.calls[1][1][1:] == (out.ctypes.data, 5, 15, 6, 0) and out.shape == (15, 6) and set(info) == set(INFO_FIELDS)
        with pytest.raises(ValueError):
            ix.narrow_base("fp16")
        with pytest.raises(ValueError):
            ix.base_rows(out=np.zeros((20, 5), np.float32))                  # fewer than d columns
        assert len(eng._L.calls) == 3
    # the packed form carries the format too
    eng = offline_engine(lsq)
    codes, K = rng.integers(0, 256, (20, 2), dtype=np.uint8), rng.standard_normal((512, 6)).astype(np.float32)
    eng.index_packed(codes, K, rng.integers(0, 4, 20, dtype=np.uint8), rng.standard_normal(4).astype(np.float32), 2, base=X, base_format="bf16")
    name, desc = _created(eng)
    assert name == "lsq_index_create_packed" and desc.base_u8 == B.BASE_BF16


# ---- the host rules under the sanitizers ----------------------------------------------------------------------------------------------------------------
def test_host_rules_under_the_sanitizers(tmp_path):
    """the narrowing and widening rules at the edge values, the format field, the alignment and argument rules, the staging-chunk rule of a host-buffer
    get_base and lsq_narrow_rows_cpu's body over ragged shapes in exactly-sized arrays, in a stand-alone program with its own main, built under
    -fsanitize=address,undefined and run directly.  The plain build stands in ONLY where the compiler says that it has no sanitizer runtime to link
    (then the test prints so); any other compile error fails the test, and so does a sanitizer report at run time"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = os.path.join(ROOT, "tools", "half_check_main.cpp"), str(tmp_path / "half_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", src, "-o", exe]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    sanitized = p.returncode == 0
    if not sanitized:
        missing = re.search(r"cannot find -l(asan|ubsan)|lib(asan|ubsan)[\w.\-]*: No such file|libclang_rt\.(asan|ubsan)|unsupported option '-fsanitize|unrecognized.*-fsanitize", p.stderr)
        assert missing, "the sanitized build failed for another reason than a missing runtime:\n" + p.stderr[-2000:]
        p = subprocess.run(base, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
    print("half_check built %s" % ("under ASan + UBSan" if sanitized else "WITHOUT sanitizers: the compiler has no runtime for them (%s)" % missing.group(0)))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all passed" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
