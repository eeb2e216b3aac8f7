"""Labelled exact k-NN (csrc/lsq_labelknn.hip): Index.knn with where=(mask, want), a row predicate per query.  The contract is Identity LK: every query's row
equals, bit for bit, the host checker's full ranking (filter_check.full_knn, nn = n) with the rows that fail the query's predicate or the index's filter
removed, cut to k and padded with (+inf, id_base - 1) -- filter_check.filtered applied per query -- which is what set_filter(those rows) and a one-query knn
return."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_check as fc  # noqa: E402
import half_check as HC  # noqa: E402

pytestmark = pytest.mark.gpu

N, D, NQ = 5003, 19, 13                              # 19 steps of 256 rows and one of 139; one chunk of 16 dimensions and three columns; a short last group at every QB
CAT, TENANT, FLAG, RARE, ONE = 0xFF, 0xFFFF00, 1 << 24, 1 << 25, 1 << 23
# per query, mixed in one call and repeated over the queries: every row; no row (every label has a category bit; a zero mask); exactly one row; ~1/100 of the
# rows; ~1/8 of them; the rows of the last step alone; every row again
WHERE = [(0, 0), (CAT, 0), (TENANT, TENANT), (TENANT, 17 << 8), (CAT, 1 << 3), (FLAG, FLAG), (0, 0)]
ANY = [CAT, 0, ONE, RARE, 1 << 3, FLAG, CAT]
QB = {1: 8, 100: 8, 256: 8, 257: 4, 512: 4, 513: 2, 1024: 2, 1025: 1, 2048: 1}


def _labels(n):
    """a category bit, a tenant below 100 in bits 8 .. 23 (all ones on one row), a flag on the rows of the last step, a rare bit on ~1/100"""
    rng = np.random.default_rng(3)
    lab = (1 << rng.integers(0, 8, n)).astype(np.uint32) | (rng.integers(0, 100, n).astype(np.uint32) << 8)
    lab |= np.where(np.arange(n) >= (n - 1) // 256 * 256, FLAG, 0).astype(np.uint32) | np.where(rng.random(n) < 0.01, RARE, 0).astype(np.uint32)
    lab[n // 3] |= TENANT
    return lab


def _words(nq, any_of):
    w = np.array([(ANY[q % 7], 0) if any_of else WHERE[q % 7] for q in range(nq)], dtype=np.uint32)
    return w[:, 0].copy(), w[:, 1].copy()


def _allowed(labels, where, any_of):
    v = labels[None, :] & where[0][:, None]
    return v != 0 if any_of else v == where[1][:, None]


@functools.lru_cache(maxsize=None)
def _problem(lsq, fmt="f32", qfmt="f32", n=N, d=D, kind=None):
    """rows as the index takes them, the queries, the labels, and the checker's full ranking (ids 0-based) of the widened rows: computed once, read-only"""
    rng = np.random.default_rng(n + d)
    X = rng.integers(0, 256, (n, d)).astype(np.uint8) if fmt == "u8" else rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.integers(0, 256, (NQ, d)).astype(np.uint8) if qfmt == "u8" else (rng.standard_normal((NQ, d)) * (64 if fmt == "u8" else 1)).astype(np.float32)
    if kind == "falling":                               # the distance to every query falls with the row id: every candidate beats the bound
        X[:] = 0
        X[:, 0] = n - np.arange(n)
        Q = (Q * 0.25).astype(np.float32)
    if kind == "ties":                                  # small integers, every row twice, a NaN row, a NaN query, +-inf components
        X = np.tile(rng.integers(0, 3, (n // 2, d)).astype(np.float32), (3, 1))[:n].copy()
        Q = rng.integers(0, 3, (NQ, d)).astype(np.float32)
        X[7, 1], X[9, 0], X[11, 2], Q[4, 0], Q[5, 1] = np.nan, np.inf, -np.inf, np.nan, np.inf
    rows, W = X, X
    if fmt in HC.FORMATS:
        rows = HC.narrow(X, fmt)
        W = HC.widen(rows, fmt)
    out = (rows, Q, _labels(n)) + fc.full_knn(lsq._lib.load(), W, Q)
    for a in out:
        a.setflags(write=False)
    return out


def _want(full, ok, nn, id_base=0):
    rows = [fc.filtered(full[0][q:q + 1], full[1][q:q + 1] + id_base, ok[q], nn, id_base - 1) for q in range(ok.shape[0])]
    return np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])


def _dev(a, pitched=False):
    """a numpy array on the device (uint32 words as int32, bf16 bits as bfloat16); pitched: rows at an odd pitch behind one element of offset"""
    import torch
    t = torch.from_numpy(np.array(a.view(np.int32) if a.dtype == np.uint32 else a.view(np.int16) if a.dtype == np.uint16 else a)).cuda()      # (a copy: the shared data is read-only)
    t = t.view(torch.bfloat16) if a.dtype == np.uint16 else t
    if pitched:
        buf = torch.zeros(a.shape[0] * (a.shape[1] + 4) + 1, dtype=t.dtype, device="cuda")
        view = torch.as_strided(buf, a.shape, (a.shape[1] + 4, 1), storage_offset=1)
        view.copy_(t)
        return view
    return t


def _index(engine, rows, fmt="f32", dev=False):
    kw = dict(base_format=fmt) if fmt in HC.FORMATS else {}
    return engine.index_dev(None, None, None, 0, base=_dev(rows, pitched=True), **kw) if dev else engine.index(None, None, None, 0, base=rows, **kw)


def _knn(ix, Q, nn, where, **kw):
    if ix._dev:
        Q, where = _dev(Q), tuple(_dev(w) for w in where)
    dd, di = ix.knn(Q, nn, where=where, **kw)
    return (dd.cpu().numpy(), di.cpu().numpy()) if ix._dev else (dd, di)


def _both_splits(lsq, ix, Q, nn, where, ok, **kw):
    """the call with the default row ranges (runs merged) and with one range per query group (one pool sees every row); the account of each"""
    got = _knn(ix, Q, nn, where, **kw)
    info = ix.label_knn_info()
    assert (info["queries"], info["rows"], info["queries_per_block"], info["allowed_pairs"]) == (Q.shape[0], ix.n, QB.get(nn, 8), int(ok.sum())), info
    assert info["blocks_per_query"] > 1 and info["merged_runs"] == Q.shape[0] * info["blocks_per_query"] and info["lds_bytes"] <= 65536
    one = _knn(ix, Q, nn, where, flags=lsq._lib.LABEL_TEST_ONE_SPLIT, **kw)
    info = ix.label_knn_info()
    assert info["blocks_per_query"] == 1 and info["merged_runs"] == 0 and info["allowed_pairs"] == int(ok.sum())
    assert fc.same(one, got)
    return got


@pytest.mark.parametrize("any_of", [False, True], ids=["all-of", "any-of"])
@pytest.mark.parametrize("nn", sorted(QB))
def test_geometries(lsq, engine, nn, any_of):
    """every queries-per-block geometry (8, 4, 2, 1) at its nn edges, both rules, a mixed set of predicates in one call"""
    rows, Q, labels, *full = _problem(lsq)
    where = _words(NQ, any_of)
    ok = _allowed(labels, where, any_of)
    assert [int(c) for c in ok.sum(1)[:3]] == [N, 0, 1] and ok[5].sum() == N - (N - 1) // 256 * 256
    with _index(engine, rows) as ix:
        ix.set_labels(labels)
        assert fc.same(_both_splits(lsq, ix, Q, nn, where, ok, any_of=any_of), _want(full, ok, nn))


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device-pitched"])
@pytest.mark.parametrize("qfmt", ["f32", "u8"])
@pytest.mark.parametrize("fmt", ["f32", "u8", "f16", "bf16"])
def test_formats(lsq, engine, fmt, qfmt, dev):
    """every row and query format on both kinds of index (the device one: an odd pitch behind an offset), both id bases; an all-rows predicate is Index.knn"""
    rows, Q, labels, *full = _problem(lsq, fmt, qfmt)
    where = _words(NQ, False)
    ok = _allowed(labels, where, False)
    with _index(engine, rows, fmt, dev) as ix:
        ix.set_labels(_dev(labels) if dev else labels)
        for nn, id_base in ((100, 0), (100, 1), (2048, 1)):
            assert fc.same(_both_splits(lsq, ix, Q, nn, where, ok, id_base=id_base), _want(full, ok, nn, id_base)), (nn, id_base)
        zeros = np.zeros(NQ, np.uint32)
        plain = ix.knn(_dev(Q) if dev else Q, 100, id_base=1)
        assert fc.same(_knn(ix, Q, 100, (zeros, zeros), id_base=1), (plain[0].cpu().numpy(), plain[1].cpu().numpy()) if dev else plain)


@pytest.mark.parametrize("d", [1, 15, 16, 17, 32, 33, 130])
def test_widths(lsq, engine, d):
    rows, Q, labels, *full = _problem(lsq, n=700, d=d)
    where = _words(NQ, False)
    ok = _allowed(labels, where, False)
    with _index(engine, rows) as ix:
        ix.set_labels(labels)
        assert fc.same(_knn(ix, Q, 10, where), _want(full, ok, 10))


def test_falling_distances(lsq, engine):
    """one pool sees every row and every candidate enters it: the pool compacts again and again, the same number of times on every call"""
    rows, Q, labels, *full = _problem(lsq, kind="falling")
    where = _words(NQ, False)
    ok = _allowed(labels, where, False)
    with _index(engine, rows) as ix:
        ix.set_labels(labels)
        infos = []
        for _ in range(2):
            assert fc.same(_knn(ix, Q, 100, where, flags=lsq._lib.LABEL_TEST_ONE_SPLIT), _want(full, ok, 100))
            infos.append(ix.label_knn_info())
        assert infos[0] == infos[1] and infos[0]["offered"] == infos[0]["allowed_pairs"] and infos[0]["compactions"] >= 3 * (N // 412)      # three queries admit every row


@pytest.mark.parametrize("nn", [10, 257])
def test_ties_and_non_finite(lsq, engine, nn):
    rows, Q, labels, *full = _problem(lsq, kind="ties")
    where = _words(NQ, False)
    ok = _allowed(labels, where, False)
    want = _want(full, ok, nn + 1)
    assert np.any(want[0][:, nn - 1] == want[0][:, nn]) and np.isnan(want[0][4, 0]) and want[1][4, 0] >= 0      # nn cuts a tie group; a NaN candidate precedes the padding
    with _index(engine, rows) as ix:
        ix.set_labels(labels)
        assert fc.same(_both_splits(lsq, ix, Q, nn, where, ok), (want[0][:, :nn], want[1][:, :nn]))


@pytest.mark.parametrize("filt", ["set_filter", "removed", "skip"])
def test_on_top_of_a_filter(lsq, engine, filt):
    """a row must pass the index's filter as well (tombstones are one); waves whose 64 rows hold no candidate of any query of the block skip their arithmetic"""
    rows, Q, labels, *full = _problem(lsq)
    where = (np.full(NQ, FLAG, np.uint32),) * 2 if filt == "skip" else _words(NQ, False)
    keep = np.random.default_rng(11).random(N) < 0.5
    ok = _allowed(labels, where, False) & keep[None, :]
    with _index(engine, rows) as ix:
        ix.set_labels(labels)
        if filt == "removed":
            ix.remove(np.flatnonzero(~keep).astype(np.int32))
        else:
            ix.set_filter(mask=keep.copy())
        assert fc.same(_both_splits(lsq, ix, Q, 100, where, ok), _want(full, ok, 100))
        assert (ix.label_knn_info()["skipped_wave_steps"] >= 2 * 19 * 4) == (filt == "skip")      # (one split, two groups of queries, 19 steps without a flagged row)


def test_identity(lsq, engine):
    """the contract as the device states it: set_filter(a query's candidates) and a one-query knn return the labelled call's row"""
    rows, Q, labels, *full = _problem(lsq)
    where = _words(9, False)
    ok = _allowed(labels, where, False)
    with _index(engine, rows, dev=True) as ix:
        ix.set_labels(_dev(labels))
        got = _knn(ix, Q[:9], 100, where)
        for q in range(9):
            fc.set_filter(ix, mask=ok[q].copy())
            one = ix.knn(_dev(Q[q:q + 1]), 100)
            assert fc.same((one[0].cpu().numpy(), one[1].cpu().numpy()), (got[0][q:q + 1], got[1][q:q + 1])), q


def test_refusals(lsq, engine):
    """LSQ_EINVAL before an output is written"""
    rows, Q, labels, *_ = _problem(lsq)
    L, E, zeros = lsq._lib.load(), lsq._lib.LSQ_EINVAL, np.zeros(NQ, np.uint32)
    dd, di = np.full((NQ, 2049), -7, np.float32), np.full((NQ, 2049), -7, np.int32)

    def raw(ix, nn=10, flags=0):
        return L.lsq_index_knn_labelled(ix._h, dd.ctypes.data, di.ctypes.data, Q.ctypes.data, 0, zeros.ctypes.data, zeros.ctypes.data, NQ, D, nn, 0, flags, 0)

    rng = np.random.default_rng(1)
    codes, K = rng.integers(0, 256, (300, 2)).astype(np.uint8), rng.standard_normal((512, D)).astype(np.float32)
    with engine.index(codes, K, np.zeros(300, np.float32), 2) as ix:
        ix.set_labels(labels[:300])
        assert raw(ix) == E                                                 # no base rows
    with _index(engine, rows[:300]) as ix:
        assert raw(ix) == E                                                 # no labels
        ix.set_labels(labels[:300])
        assert raw(ix, 301) == E and raw(ix, flags=4) == E                  # nn > n; an unknown flag
        with pytest.raises(ValueError):
            ix.knn(Q, 10, where=(zeros[:5], zeros))                         # a mask of the wrong length
        assert np.all(dd == -7) and np.all(di == -7)
        assert raw(ix) == 0 and np.all(di.ravel()[:NQ * 10] >= 0)
    with _index(engine, rows) as ix:
        ix.set_labels(labels)
        dd[:], di[:] = -7, -7
        assert raw(ix, 2049) == E and np.all(dd == -7) and np.all(di == -7)  # nn > 2048
