"""The packed index without a GPU: the boundary (header, binding, both libraries), linscan_lsq_bytes' engine-less road against linscan_lsq on the widened
norms bit for bit, and the refusals that must happen in Python before any library call."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packed_check as pc  # noqa: E402
from knn_check import same_bits  # noqa: E402

H = 256
SYMBOLS = ("lsq_index_create_packed", "lsq_index_get_packed_info", "lsq_index_get_scan_stats")


def test_header_binding_and_libraries_agree(lsq):
    hdr = pc.header()
    L, tun = lsq._lib.load(), lsq._lib.load(tuning=True)
    for s in SYMBOLS:
        assert re.search(r"LSQ_API\s+int\s+%s\s*\(\s*lsq_index\b" % s, hdr), "%s is not declared index-first" % s
        assert s in lsq._lib.SIGNATURES and hasattr(L, s) and hasattr(tun, s)
    for struct, binding in (("lsq_index_packed_desc", lsq._lib.IndexPackedDesc), ("lsq_index_packed_info", lsq._lib.IndexPackedInfo)):
        assert [f for f, _ in binding._fields_] == pc.header_struct_fields(struct), struct
    assert C.sizeof(lsq._lib.IndexPackedInfo) == 5 * 8
    assert lsq._lib.SIGNATURES["lsq_index_get_scan_stats"][1][1]._type_ is lsq._lib.LinscanStats
    version = int(re.search(r"#define\s+LSQ_VERSION\s+(\d+)", hdr).group(1))
    assert version >= 1800 and L.lsq_version() == version and tun.lsq_version() == version
    # lsq_index_desc is ABI: the packed form came as a struct of its own
    assert pc.header_struct_fields("lsq_index_desc") == [f for f, _ in lsq._lib.IndexDesc._fields_] == \
        ["n", "d", "m", "h", "codes", "codebooks", "dbnorms", "base", "base_u8", "ldb", "on_device"]


def _julia_problem(m, ncb, seed, n=300, d=8, nq=7, special=True):
    rng = np.random.default_rng(seed)
    codes, K, nc, cb, Q = pc.problem(rng, n, m, d, nq, ncb=ncb, special=special)
    Cs = [np.ascontiguousarray(K[j * H:(j + 1) * H].T) for j in range(m)]      # list of (d, h)
    R = np.linalg.qr(rng.standard_normal((d, d)))[0].astype(np.float32)
    return np.ascontiguousarray(codes.T), np.ascontiguousarray(Q.T), Cs, cb, nc.astype(np.int16) + 1, R


@pytest.mark.parametrize("m", [1, 7, 8])
@pytest.mark.parametrize("ncb", [1, 37, 256])
def test_linscan_lsq_bytes_without_an_engine_is_linscan_lsq_on_the_widened_norms(lsq, m, ncb):
    B, X, Cs, cb, bn, R = _julia_problem(m, ncb, 11 * m + ncb)
    if ncb >= 4:
        assert np.isnan(cb).any() and np.isposinf(cb).any() and np.isneginf(cb).any() and (np.signbit(cb) & (cb == 0)).any()
    for k in (1, 10, B.shape[1]):
        wd, wi = lsq.linscan_lsq(B, X, Cs, cb[bn.astype(np.int64) - 1], R, k)
        gd, gi = lsq.linscan_lsq_bytes(B, X, Cs, cb, bn, R, k)
        assert gd.shape == (k, X.shape[1]) and same_bits(gd, wd) and np.array_equal(gi, wi)
    # any integer type of B_norms, as train_lsq may hand it over
    for ty in (np.uint8, np.int64):
        if ncb < 256 or ty is not np.uint8:                                     # (256 does not fit a 1-based uint8)
            gd, gi = lsq.linscan_lsq_bytes(B, X, Cs, cb, bn.astype(ty), R, 10)
            wd, wi = lsq.linscan_lsq(B, X, Cs, cb[bn.astype(np.int64) - 1], R, 10)
            assert same_bits(gd, wd) and np.array_equal(gi, wi)


class _Untouchable:
    """an engine that fails the test when anything is asked of it: a refusal must come before the first call"""

    def __getattr__(self, name):
        raise AssertionError("the engine was used (%s) before the arguments were refused" % name)


@pytest.mark.parametrize("engine", [None, _Untouchable()], ids=["host", "engine"])
def test_python_side_refusals_come_before_any_library_call(lsq, engine, monkeypatch):
    B, X, Cs, cb, bn, R = _julia_problem(7, 37, 5, special=False)
    monkeypatch.setattr(lsq._lib, "load", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the library was loaded before the refusal")))
    call = lambda **kw: lsq.linscan_lsq_bytes(kw.get("B", B), X, Cs, kw.get("cb", cb), kw.get("bn", bn), R, 5, engine=engine)      # noqa: E731
    low, high = bn.copy(), bn.copy()
    low[3], high[-1] = 0, 38
    for bad in (low, high):
        with pytest.raises(ValueError, match=r"1 \.\. 37"):
            call(bn=bad)
    with pytest.raises(TypeError, match="B_norms"):
        call(bn=bn.astype(np.float32))
    with pytest.raises(TypeError, match="cbnorms"):
        call(cb=cb.astype(np.float64))
    with pytest.raises(TypeError, match="uint8"):
        call(B=B.astype(np.int16))
    with pytest.raises(ValueError, match="one entry per code"):
        call(bn=bn[:-1])
    with pytest.raises(ValueError, match="one entry per code"):
        call(bn=np.concatenate([bn, bn[:1]]))
    with pytest.raises(ValueError, match="1 .. 256"):
        call(cb=np.zeros(257, dtype=np.float32))
    with pytest.raises(ValueError, match="1 .. 256"):
        call(cb=np.zeros(0, dtype=np.float32))
