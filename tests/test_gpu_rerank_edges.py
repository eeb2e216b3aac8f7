"""The device re-rank on the edge cases of tests/test_rerank.py, against lsq_rerank_cpu bit for bit: ids outside the base (never dereferenced, last,
after NaN), NaN in rows and in queries, massive ties, duplicated rows and ids -- each through a host-buffer and a borrowed-device index, f32 and uint8
rows -- and the 16-byte-aligned loaders on a row whose last 16-byte piece is partial."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from knn_check import same_bits  # noqa: E402
from rerank_check import base_and_queries, padded, rerank_cpu  # noqa: E402

pytestmark = pytest.mark.gpu
N = 1200
INT_MAX = 2 ** 31 - 1


def _both(lsq, engine, Xbp, d, Xq, cand, id_base, nns):
    """(dists, ids) of the host checker for nn = L, after the host-buffer index and the borrowed-device one gave its first nn columns for every nn"""
    import torch
    lib = lsq._lib.load()
    Lc = cand.shape[1]
    rc, rd, ri = rerank_cpu(lib, Xbp, Xq, cand, d, Lc, id_base)
    assert rc == 0
    dbase = torch.from_numpy(Xbp).cuda()[:, :d]
    tq, tc = torch.from_numpy(Xq).cuda(), torch.from_numpy(cand).cuda()
    with engine.index(None, None, None, 0, base=Xbp, d=d) as hix, engine.index_dev(None, None, None, 0, base=dbase, d=d) as dix:
        for nn in nns:
            hd, hi = hix.rerank(Xq, cand, nn, id_base=id_base)
            dd, di = dix.rerank(tq, tc, nn, id_base=id_base)
            dd, di = dd.cpu().numpy(), di.cpu().numpy()
            for what, gd, gi in (("host", hd, hi), ("device", dd, di)):
                assert same_bits(gd, rd[:, :nn]) and np.array_equal(gi, ri[:, :nn]), (what, Xbp.dtype, d, Lc, nn, id_base)
        outside = int(((cand.astype(np.int64) - id_base < 0) | (cand.astype(np.int64) - id_base >= Xbp.shape[0])).sum())
        st = hix.stats()
        assert st["invalid"] == outside * len(nns) and st["rows"] == (cand.size - outside) * len(nns) and dix.stats() == st
    return rd, ri


@pytest.mark.parametrize("id_base", [0, 1])
@pytest.mark.parametrize("u8", [False, True])
def test_ids_outside_the_base_come_last_after_nan(lsq, engine, u8, id_base):
    """id_base - 1, n + id_base, a negative id and INT_MAX in every list, next to a NaN distance: a NaN row (f32 rows) or a NaN query (uint8 rows hold
    no NaN).  L = 300: two tiles of the kernel, ids outside the base in both."""
    d, nq, Lc = 16, 5, 300
    Xb, Xq = base_and_queries(d, N, nq, 6, u8=u8)
    if not u8:
        Xb[11, 3] = np.nan
    else:
        Xq[4, 7] = np.nan                                                      # every distance of query 4 is NaN, and still comes before the ids outside
    cand = np.random.default_rng(7).integers(id_base, N + id_base, (nq, Lc)).astype(np.int32)
    cand[:, 0], cand[:, 9], cand[:, 33], cand[:, 64], cand[:, 257], cand[:, 299] = id_base - 1, N + id_base, -7, INT_MAX, -INT_MAX - 1, id_base - 1
    cand[cand == 11 + id_base] = 12 + id_base
    cand[:, 20] = 11 + id_base                                                 # the NaN row once in every list
    rd, ri = _both(lsq, engine, Xb, d, Xq, cand, id_base, (1, 295, Lc))
    assert np.all(np.isposinf(rd[:, -6:])) and np.all(ri[:, -6:] == id_base - 1) and np.all(ri[:, :-6] != id_base - 1)
    if not u8:
        assert np.all(np.isnan(rd[:, -7])) and np.all(ri[:, -7] == 11 + id_base) and np.all(np.isfinite(rd[:, :-7]))
    else:
        assert np.all(np.isnan(rd[4, :-6])) and np.all(np.diff(ri[4, :-6]) >= 0) and np.all(np.isfinite(rd[:4, :-6]))
    assert np.all(rd.view(np.uint32)[np.isnan(rd)] == 0x7FC00000)


@pytest.mark.parametrize("id_base", [0, 1])
def test_a_list_of_nothing_but_ids_outside_the_base(lsq, engine, id_base):
    Xb, Xq = base_and_queries(16, N, 3, 6)
    cand = np.tile(np.array([N + id_base, id_base - 1, -7, INT_MAX, N + id_base], dtype=np.int32), (3, 1))
    rd, ri = _both(lsq, engine, Xb, 16, Xq, cand, id_base, (1, 5))
    assert np.all(np.isposinf(rd)) and np.all(ri == id_base - 1)


def test_nan_in_a_row_and_in_a_query(lsq, engine):
    d, nq = 130, 5
    Xb, Xq = base_and_queries(d, N, nq, 8)
    Xb[3, 129] = Xb[77, 0] = np.nan                                            # in the row's last, partial line and in its first component
    Xq[2, 64] = np.nan                                                         # every distance of query 2 is NaN: ids ascending
    others = np.setdiff1d(np.arange(N), (3, 77))
    cand = np.stack([np.random.default_rng(9 + q).permutation(others)[:200] for q in range(nq)]).astype(np.int32)
    cand[:, 5], cand[:, 150] = 3, 77
    cand[:, 100] = N                                                           # ... and one id outside the base behind the NaNs
    rd, ri = _both(lsq, engine, Xb, d, Xq, cand, 0, (1, 198, 200))
    assert np.all(np.isnan(rd[2, :-1])) and np.all(np.diff(ri[2, :-1]) > 0)
    assert np.all(np.isnan(rd[0, -3:-1])) and ri[0, -3:].tolist() == [3, 77, -1] and np.all(np.isfinite(rd[0, :-3]))
    assert np.all(np.isposinf(rd[:, -1]))
    assert np.all(rd.view(np.uint32)[np.isnan(rd)] == 0x7FC00000)


@pytest.mark.parametrize("u8", [False, True])
def test_massive_ties_are_ordered_by_id(lsq, engine, u8):
    rng = np.random.default_rng(3)
    Xb = rng.integers(0, 4, (N, 3)).astype(np.uint8 if u8 else np.float32)
    Xq = rng.integers(0, 4, (5, 3)).astype(np.float32)
    cand = np.stack([rng.permutation(N)[:1000] for _ in range(5)]).astype(np.int32) + 1
    rd, ri = _both(lsq, engine, Xb, 3, Xq, cand, 1, (1, 1000))
    for q in range(5):
        same = rd[q, 1:] == rd[q, :-1]
        assert same.sum() > 900 and np.all(ri[q, 1:][same] > ri[q, :-1][same])


@pytest.mark.parametrize("u8", [False, True])
def test_duplicated_rows_and_duplicated_candidates(lsq, engine, u8):
    Xb, Xq = base_and_queries(17, N, 5, 4, u8=u8)
    Xb[5] = Xb[900] = Xb[40]                                                   # three rows, one vector
    cand = np.random.default_rng(5).integers(0, N, (5, 64)).astype(np.int32)
    cand[:, :6] = [40, 900, 5, 40, 40, 7]                                      # and id 40 three times
    rd, ri = _both(lsq, engine, Xb, 17, Xq, cand, 0, (1, 64))
    for q in range(5):
        assert (ri[q] == 40).sum() == 3 + (cand[q, 6:] == 40).sum()
        at = np.nonzero(np.isin(ri[q], (5, 40, 900)))[0]
        assert np.all(np.diff(at) == 1) and len(set(rd[q, at].tolist())) == 1 and np.all(np.diff(ri[q, at]) >= 0)


@pytest.mark.parametrize("u8,d,ldb", [(False, 18, 20), (True, 17, 32), (True, 130, 144)])
def test_aligned_rows_with_a_partial_last_piece(lsq, engine, u8, d, ldb):
    """base and pitch are multiples of 16 bytes, d is not: the 16-byte loaders meet a last piece of 8 bytes (f32), of 1 and of 2 bytes (uint8)"""
    import torch
    Xb, Xq = base_and_queries(d, N, 130, 50 + d, u8=u8)
    Xbp = padded(Xb, ldb - d, np.float32(np.nan) if not u8 else np.uint8(255))
    assert (ldb * Xbp.itemsize) % 16 == 0 and (d * Xbp.itemsize) % 16 != 0
    cand = np.random.default_rng(d).integers(1, N + 1, (130, 65)).astype(np.int32)
    rc, rd, ri = rerank_cpu(lsq._lib.load(), Xbp, Xq, cand, d, 65, 1)
    assert rc == 0
    dev = torch.from_numpy(Xbp).cuda()
    assert dev.data_ptr() % 16 == 0
    with engine.index_dev(None, None, None, 0, base=dev[:, :d], d=d) as ix:
        dd, di = ix.rerank(torch.from_numpy(Xq).cuda(), torch.from_numpy(cand).cuda(), 65, id_base=1)
    assert same_bits(dd.cpu().numpy(), rd) and np.array_equal(di.cpu().numpy(), ri)
    with engine.index(None, None, None, 0, base=Xbp, d=d) as ix:              # the index's own copy starts on an allocation
        dd, di = ix.rerank(Xq, cand, 65, id_base=1)
    assert same_bits(dd, rd) and np.array_equal(di, ri)


def test_a_closed_engine_closes_its_indexes(lsq):
    Xb, Xq = base_and_queries(8, 100, 2, 1)
    eng = lsq.Engine(0)
    ix = eng.index(None, None, None, 0, base=Xb)
    eng.close()
    assert ix._h is None
    ix.close()                                                                 # and closing it again is harmless
    with lsq.Engine(0) as eng2, eng2.index(None, None, None, 0, base=Xb) as ix2:
        dd, di = ix2.rerank(Xq, np.array([[1, 2], [3, 4]], dtype=np.int32), 2)
    assert np.all(np.isfinite(dd))


def test_a_list_longer_than_a_batch_is_rejected(lsq, engine):
    """one query's records are one batch of at most 2^28: a longer list (candidates may repeat, so L may exceed n) launches nothing"""
    lib = lsq._lib.load()
    Xb, Xq = base_and_queries(8, 100, 1, 1)
    cand = np.zeros((1, 4), dtype=np.int32)
    out_d, out_i = np.zeros((1, 1), np.float32), np.zeros((1, 1), np.int32)
    with engine.index(None, None, None, 0, base=Xb) as ix:
        rc = lib.lsq_index_rerank(ix._h, out_d.ctypes.data, out_i.ctypes.data, Xq.ctypes.data, cand.ctypes.data, 1, 8, 2 ** 28 + 1, 1, 0, 0)
        assert rc == lsq._lib.LSQ_EINVAL and b"2^28" in lib.lsq_last_error()
        assert ix.stats()["batches"] == 0 and ix.stats()["queries"] == 0
