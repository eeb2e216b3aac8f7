"""Exact k-NN on 8-bit sets, the parts that need no GPU: the C ABI of lsq_index_knn / lsq_index_get_knn_info / lsq_knn_exact_u8_cpu, and the host drop-in
lsq_knn_exact_u8_cpu against the two checkers of tests/index_knn_check.py (lsq_knn_exact_cpu on the widened matrices; int64 arithmetic for d <= 258) --
every element-type combination, bases and queries at byte offsets 1-3 with odd pitches and padding of 255, the largest distances d = 258 allows, and
d = 960 where the f32 chain rounds and the integer does not: the host function returns the CHAIN's bits."""
import os
import re

import numpy as np
import pytest

import index_knn_check as IK
import knn_check as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lsq_index_knn", "lsq_index_get_knn_info", "lsq_knn_exact_u8_cpu")
EINVAL = -1


def test_header_and_abi(lsq):
    hdr = open(os.path.join(ROOT, "include", "lsq_mi355x.h")).read()
    assert int(re.search(r"#define LSQ_VERSION (\d+)", hdr).group(1)) >= 1500
    declared = set(re.findall(r"LSQ_API\s+[\w\s\*]*?\b(lsq_\w+)\s*\(", hdr))
    assert set(NEW) <= declared
    first = set(re.findall(r"\b(lsq_\w+)\s*\(\s*(?:struct\s+)?lsq_ctx\s*\*", hdr))      # the closed sets of context-first entry points stay closed
    assert not first & set(NEW)
    assert "(3f)" in hdr and "sift_groundtruth.ivecs" in hdr.split("(3f)")[1] and "Linscan.jl:76-117" in hdr.split("(3f)")[1]
    assert lsq._lib.load().lsq_version() >= 1500
    tun = lsq._lib.load(tuning=True)
    for s in NEW:
        assert s in lsq._lib.SIGNATURES and hasattr(tun, s)
    assert lsq._lib.LSQ_EINVAL == EINVAL


def _u8_cpu(lsq, Xb, Xq, nn, base_u8=True, q_u8=True):
    B = np.ascontiguousarray(Xb if base_u8 else Xb.astype(np.float32))
    Q = np.ascontiguousarray(Xq if q_u8 else Xq.astype(np.float32))
    rc, dists, ids = IK.knn_u8_cpu(lsq._lib.load(), B.ctypes.data, base_u8, Q.ctypes.data, q_u8, B.shape[0], Q.shape[0], B.shape[1], B.shape[1], Q.shape[1], nn)
    assert rc == 0
    return dists, ids


@pytest.mark.parametrize("d", [1, 3, 4, 5, 127, 128, 258, 259, 300, 960])
def test_host_widths(lsq, d):
    Xb, Xq = IK.u8_data(d, 400, 9, d)
    got = _u8_cpu(lsq, Xb, Xq, 10)
    IK.same(*got, *IK.knn_widened(lsq._lib.load(), Xb, Xq, 10))
    if d <= 258:
        IK.same(*got, *IK.knn_int64(Xb, Xq, 10))


def test_host_extreme_pair_d258(lsq):
    Xb, Xq = IK.extreme(70, 5, 258)
    dists, ids = _u8_cpu(lsq, Xb, Xq, 70)
    IK.same(dists, ids, *IK.knn_int64(Xb, Xq, 70))
    IK.same(dists, ids, *IK.knn_widened(lsq._lib.load(), Xb, Xq, 70))
    assert dists[0, ids[0] == 0][0] == np.float32(16776450.0) == 258 * 255 * 255      # the all-255 row against the all-0 query, exactly


def test_host_d960_returns_the_chain_not_the_integer(lsq):
    Xb, Xq = IK.extreme(200, 4, 960)
    dists, ids = _u8_cpu(lsq, Xb, Xq, 200)
    IK.same(dists, ids, *IK.knn_widened(lsq._lib.load(), Xb, Xq, 200))
    IK.same(dists, ids, *KC.knn_np(Xb.astype(np.float32), Xq.astype(np.float32), 200))
    D = ((Xb.astype(np.int64)[None] - Xq.astype(np.int64)[:, None]) ** 2).sum(2)
    exact = np.take_along_axis(D, ids.astype(np.int64), axis=1)
    assert exact.max() > 1 << 24 and (dists.astype(np.float64) != exact).any()      # the chain rounded somewhere: these inputs tell the two apart


@pytest.mark.parametrize("base_u8,q_u8", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_host_element_types(lsq, base_u8, q_u8):
    Xb, Xq = IK.u8_data(3, 300, 7, 33)
    IK.same(*_u8_cpu(lsq, Xb, Xq, 12, base_u8, q_u8), *IK.knn_widened(lsq._lib.load(), Xb, Xq, 12))
    # non-integer f32 queries against either base type
    if not q_u8:
        Qf = (Xq.astype(np.float32) + np.float32(0.37))
        B = np.ascontiguousarray(Xb if base_u8 else Xb.astype(np.float32))
        rc, dists, ids = IK.knn_u8_cpu(lsq._lib.load(), B.ctypes.data, base_u8, Qf.ctypes.data, 0, 300, 7, 33, 33, 33, 12)
        assert rc == 0
        IK.same(dists, ids, *KC.knn_np(Xb.astype(np.float32), Qf, 12))


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("base_u8,q_u8", [(1, 1), (0, 0), (1, 0)])
def test_host_byte_offsets_odd_pitches_padding(lsq, off, base_u8, q_u8):
    d, n, nq = 13, 150, 6
    Xb, Xq = IK.u8_data(10 + off, n, nq, d)
    ldb, ldq = d + 2 * off + 1, d + off
    _, bbuf = IK.laid_out(Xb, ldb, off, None if base_u8 else np.float32)
    _, qbuf = IK.laid_out(Xq, ldq, 4 - off, None if q_u8 else np.float32)
    rc, dists, ids = IK.knn_u8_cpu(lsq._lib.load(), bbuf.ctypes.data + off, base_u8, qbuf.ctypes.data + 4 - off, q_u8, n, nq, d, ldb, ldq, 9)
    assert rc == 0
    IK.same(dists, ids, *IK.knn_int64(Xb, Xq, 9))


def test_host_einval(lsq):
    L = lsq._lib.load()
    Xb, Xq = IK.u8_data(1, 50, 3, 8)
    b, q = Xb.ctypes.data, Xq.ctypes.data

    def call(bp=b, qp=q, n=50, nq=3, d=8, ldb=8, ldq=8, nn=5, out=True):
        dists, ids = np.zeros((3, 64), np.float32), np.zeros((3, 64), np.uint32)
        return L.lsq_knn_exact_u8_cpu(dists.ctypes.data if out else None, ids.ctypes.data, bp, 1, qp, 1, n, nq, d, ldb, ldq, nn, 1)

    assert call() == 0
    for bad in (dict(nn=0), dict(nn=51), dict(nq=0), dict(ldq=7), dict(ldb=7), dict(d=0), dict(bp=None), dict(qp=None), dict(out=False)):
        assert call(**bad) == EINVAL, bad
        assert b"lsq_knn_exact_u8_cpu" in L.lsq_last_error()
    # the index calls reject a null index before anything else
    assert L.lsq_index_knn(None, b, b, q, 1, 3, 8, 5, 0, 0) == EINVAL
    assert L.lsq_index_get_knn_info(None, None) == EINVAL


def test_reference_api_hands_uint8_through(lsq):
    d, n, nq, k = 24, 500, 11, 15
    Xb, Xq = IK.u8_data(21, n, nq, d)
    X8, Q8 = np.ascontiguousarray(Xb.T), np.ascontiguousarray(Xq.T)          # (d, n), (d, nq): what bvecs_read returns
    want_d, want_i = lsq.knn_exact(X8.astype(np.float32), Q8.astype(np.float32), k, nthreads=2)
    for Q in (Q8, Q8.astype(np.float32)):
        dists, ids = lsq.knn_exact(X8, Q, k, nthreads=2)
        assert dists.shape == (k, nq) and ids.dtype == np.uint32 and ids.min() >= 1
        IK.same(dists, ids, want_d, want_i)
    wd, wi = IK.knn_int64(Xb, Xq, k)
    IK.same(want_d.T, want_i.T - 1, wd, wi)
