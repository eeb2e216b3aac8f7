"""lsq_rerank_cpu (the host drop-in of the exact re-rank) and its Python wrappers against numpy, bit for bit; the header's and the ABI's new ground."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from knn_check import knn_cpu, same_bits  # noqa: E402
from rerank_check import DIMS, LISTS, base_and_queries, padded, rerank_cpu, rerank_np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NQ = 1200, 5


def _agree(L, Xb, Xq, cand, d, nn, id_base, ref_base=None):
    rc, dd, di = rerank_cpu(L, Xb, Xq, cand, d, nn, id_base)
    assert rc == 0, L.lsq_last_error()
    rd, ri = rerank_np((Xb if ref_base is None else ref_base)[:, :d], Xq[:, :d], cand, nn, id_base)
    assert same_bits(dd, rd) and np.array_equal(di, ri), (d, cand.shape, nn, id_base)
    return dd, di


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("d", DIMS)
def test_random_candidates_match_numpy(lsq, d, pad):
    L = lsq._lib.load()
    Xb, Xq = base_and_queries(d, N, NQ, 100 + d)
    Xbp, Xqp = padded(Xb, pad, np.float32(np.nan)), padded(Xq, pad, np.float32(np.nan))      # what lies between the rows is never read
    rng = np.random.default_rng(d)
    for Lc in LISTS:
        for id_base in (0, 1):
            cand = rng.integers(id_base, N + id_base, (NQ, Lc)).astype(np.int32)
            for nn in sorted({1, Lc}):
                _agree(L, Xbp, Xqp, cand, d, nn, id_base)


def test_all_ids_equals_exact_knn(lsq):
    L = lsq._lib.load()
    n, d = 3000, 24
    Xb, Xq = base_and_queries(d, n, 4, 7)
    rng = np.random.default_rng(1)
    cand = np.stack([rng.permutation(n) for _ in range(4)]).astype(np.int32)
    rc, kd, ki = knn_cpu(L, Xb, Xq, d, n)
    assert rc == 0
    rc, dd, di = rerank_cpu(L, Xb, Xq, cand, d, n, 0)
    assert rc == 0 and same_bits(dd, kd) and np.array_equal(di, ki.astype(np.int32))
    rc, dd, di = rerank_cpu(L, Xb, Xq, cand + 1, d, 10, 1)
    assert rc == 0 and same_bits(dd, kd[:, :10]) and np.array_equal(di, ki[:, :10].astype(np.int32) + 1)


@pytest.mark.parametrize("d,pad", [(16, 0), (17, 3), (128, 0), (130, 1)])
def test_uint8_base_equals_the_widened_call(lsq, d, pad):
    L = lsq._lib.load()
    Xb, Xq = base_and_queries(d, N, NQ, 9, u8=True)
    cand = np.random.default_rng(2).integers(0, N, (NQ, 65)).astype(np.int32)
    Xbp = padded(Xb, pad, np.uint8(255))
    dd, di = _agree(L, Xbp, Xq, cand, d, 65, 0)
    rc, fd, fi = rerank_cpu(L, Xbp.astype(np.float32), Xq, cand, d, 65, 0)
    assert rc == 0 and same_bits(dd, fd) and np.array_equal(di, fi)


def test_massive_ties_are_ordered_by_id(lsq):
    L = lsq._lib.load()
    rng = np.random.default_rng(3)
    Xb = rng.integers(0, 4, (N, 3)).astype(np.float32)
    Xq = rng.integers(0, 4, (NQ, 3)).astype(np.float32)
    cand = np.stack([rng.permutation(N)[:1000] for _ in range(NQ)]).astype(np.int32) + 1
    dd, di = _agree(L, Xb, Xq, cand, 3, 1000, 1)
    assert len(np.unique(dd)) < 40                                             # a few dozen distinct distances among 1000
    for q in range(NQ):
        same = dd[q, 1:] == dd[q, :-1]
        assert same.sum() > 900 and np.all(di[q, 1:][same] > di[q, :-1][same])
    _agree(L, Xb.astype(np.uint8), Xq, cand, 3, 1000, 1)


def test_duplicated_rows_and_duplicated_candidates(lsq):
    L = lsq._lib.load()
    Xb, Xq = base_and_queries(17, N, NQ, 4)
    Xb[5] = Xb[900] = Xb[40]                                                   # three rows, one vector
    cand = np.random.default_rng(5).integers(0, N, (NQ, 64)).astype(np.int32)
    cand[:, :6] = [40, 900, 5, 40, 40, 7]                                      # and id 40 three times
    dd, di = _agree(L, Xb, Xq, cand, 17, 64, 0)
    for q in range(NQ):
        assert (di[q] == 40).sum() == 3 + (cand[q, 6:] == 40).sum()
        at = np.nonzero(np.isin(di[q], (5, 40, 900)))[0]
        assert np.all(np.diff(at) == 1) and len(set(dd[q, at].tolist())) == 1  # one run of equal distances, ids ascending inside it
        assert np.all(np.diff(di[q, at]) >= 0)


@pytest.mark.parametrize("id_base", [0, 1])
def test_ids_outside_the_base_come_last_after_nan(lsq, id_base):
    L = lsq._lib.load()
    Xb, Xq = base_and_queries(16, N, NQ, 6)
    Xb[11, 3] = np.nan                                                         # a NaN row
    cand = np.random.default_rng(7).integers(id_base, N + id_base, (NQ, 65)).astype(np.int32)
    cand[:, 0], cand[:, 9], cand[:, 33], cand[:, 64] = id_base - 1, N + id_base, -7, 2 ** 31 - 1
    cand[:, 20] = 11 + id_base
    dd, di = _agree(L, Xb, Xq, cand, 16, 65, id_base)
    assert np.all(np.isposinf(dd[:, -4:])) and np.all(di[:, -4:] == id_base - 1)
    assert np.all(np.isnan(dd[:, -5])) and np.all(di[:, -5] == 11 + id_base)
    assert np.all(np.isfinite(dd[:, :-5]))
    # a list of nothing but ids outside the base
    dd, di = _agree(L, Xb, Xq, np.full((NQ, 3), N + id_base, dtype=np.int32), 16, 3, id_base)
    assert np.all(np.isposinf(dd)) and np.all(di == id_base - 1)


def test_nan_in_a_row_and_in_a_query(lsq):
    L = lsq._lib.load()
    Xb, Xq = base_and_queries(130, N, NQ, 8)
    Xb[3, 129] = Xb[77, 0] = np.nan
    Xq[2, 64] = np.nan                                                         # every distance of query 2 is NaN: ids ascending
    others = np.setdiff1d(np.arange(N), (3, 77))
    cand = np.stack([np.random.default_rng(9 + q).permutation(others)[:200] for q in range(NQ)]).astype(np.int32)
    cand[:, 5], cand[:, 150] = 3, 77                                           # each of the two NaN rows once in every list
    dd, di = _agree(L, Xb, Xq, cand, 130, 200, 0)
    assert np.all(np.isnan(dd[2])) and np.all(np.diff(di[2]) > 0)
    assert np.all(np.isnan(dd[0, -2:])) and di[0, -2:].tolist() == [3, 77] and np.all(np.isfinite(dd[0, :-2]))
    assert np.all(dd.view(np.uint32)[np.isnan(dd)] == 0x7FC00000)


def test_bad_arguments(lsq):
    L = lsq._lib.load()
    EINVAL = lsq._lib.LSQ_EINVAL
    Xb, Xq = base_and_queries(8, 50, 3, 1)
    cand = np.zeros((3, 4), dtype=np.int32)
    assert rerank_cpu(L, Xb, Xq, cand, 8, 5, 0)[0] == EINVAL and b"nn" in L.lsq_last_error()          # nn > L
    assert rerank_cpu(L, Xb, Xq, cand, 8, 0, 0)[0] == EINVAL
    assert rerank_cpu(L, Xb, Xq, cand, 9, 1, 0)[0] == EINVAL                                            # ldb < d
    assert rerank_cpu(L, Xb, Xq, cand, 0, 1, 0)[0] == EINVAL
    assert rerank_cpu(L, Xb, Xq, cand, 8, 1, 2)[0] == EINVAL
    out_d, out_i = np.zeros((3, 1), np.float32), np.zeros((3, 1), np.int32)
    good = [out_d.ctypes.data, out_i.ctypes.data, Xb.ctypes.data, 0, Xq.ctypes.data, cand.ctypes.data, 50, 3, 8, 8, 8, 4, 1, 0, 1]
    assert L.lsq_rerank_cpu(*good) == 0
    for at in (0, 1, 2, 4, 5):
        args = list(good)
        args[at] = None
        assert L.lsq_rerank_cpu(*args) == EINVAL and b"null" in L.lsq_last_error()
    # the index takes no null handle and no null description, with or without a device
    assert L.lsq_index_search(None, out_d.ctypes.data, out_i.ctypes.data, Xq.ctypes.data, None, 3, 8, 0, 1, 0) == EINVAL
    assert L.lsq_index_rerank(None, out_d.ctypes.data, out_i.ctypes.data, Xq.ctypes.data, cand.ctypes.data, 3, 8, 4, 1, 0, 0) == EINVAL
    assert L.lsq_index_get_stats(None, None) == EINVAL
    assert L.lsq_index_create(None, None, None) == EINVAL
    assert L.lsq_index_destroy(None) == 0


def test_python_wrappers_in_julia_shapes(lsq):
    d, n, nq, Lc, k = 20, 400, 6, 50, 10
    Xb, Xq = base_and_queries(d, n, nq, 12)
    cand = np.random.default_rng(13).integers(1, n + 1, (nq, Lc)).astype(np.int32)
    rd, ri = rerank_np(Xb, Xq, cand, k, 1)
    dists, ids = lsq.rerank(Xb.T, Xq.T, cand.T, k)                                # (d, n), (d, nq), (L, nq) -> (k, nq)
    assert dists.shape == (k, nq) and ids.dtype == np.int32 and same_bits(dists.T, rd) and np.array_equal(ids.T, ri)
    X8 = np.random.default_rng(14).integers(0, 256, (d, n), dtype=np.uint8)        # what bvecs_read returns
    d8, i8 = lsq.rerank(X8, Xq.T, cand.T.astype(np.uint32), k)
    r8, j8 = rerank_np(X8.T, Xq, cand, k, 1)
    assert same_bits(d8.T, r8) and np.array_equal(i8.T, j8)
    # the two-stage call without an engine: the host scan's shortlist, re-ranked on the host
    m, h = 2, 256
    rng = np.random.default_rng(15)
    C = [rng.standard_normal((d, h)).astype(np.float32) for _ in range(m)]
    B = rng.integers(0, h, (m, n)).astype(np.uint8)
    dbn = rng.random(n).astype(np.float32)
    R = np.linalg.qr(rng.standard_normal((d, d)))[0].astype(np.float32)
    _, short = lsq.linscan_lsq(B, Xq.T, C, dbn, R, Lc)
    td, ti = lsq.linscan_lsq_rerank(B, Xq.T, C, dbn, R, Xb.T, Lc, k)
    rd, ri = rerank_np(Xb, Xq, short.T, k, 1)
    assert same_bits(td.T, rd) and np.array_equal(ti.T, ri)


def test_header_and_abi():
    hdr = open(os.path.join(ROOT, "include", "lsq_mi355x.h")).read()
    assert int(re.search(r"#define LSQ_VERSION (\d+)", hdr).group(1)) >= 1400
    new = ("lsq_rerank_cpu", "lsq_index_create", "lsq_index_destroy", "lsq_index_search", "lsq_index_rerank", "lsq_index_get_stats")
    declared = set(re.findall(r"LSQ_API\s+[\w\s\*]*?\b(lsq_\w+)\s*\(", hdr))
    assert set(new) <= declared
    # the closed sets of context-first entry points (tests/ctx_ops.py, tests/test_gpu_ctx_u8.py) stay closed: none of the new symbols takes the context first
    first = set(re.findall(r"\b(lsq_\w+)\s*\(\s*(?:struct\s+)?lsq_ctx\s*\*", hdr))
    assert not first & set(new) and not any(s.startswith(("lsq_index", "lsq_rerank")) for s in first)
    assert re.search(r"lsq_index_create\(lsq_index \*\*out, lsq_ctx \*ctx, const lsq_index_desc \*desc\)", hdr)
    assert "Linscan.jl:46-73" in hdr and re.search(r"NO COUNTERPART IN THE REFERENCE", hdr, flags=re.I)


def test_library_version_and_tuning_abi(lsq):
    assert lsq._lib.load().lsq_version() >= 1400
    tun = lsq._lib.load(tuning=True)
    for s in ("lsq_rerank_cpu", "lsq_index_create", "lsq_index_search", "lsq_index_rerank", "lsq_index_get_stats", "lsq_index_destroy"):
        assert hasattr(tun, s)
