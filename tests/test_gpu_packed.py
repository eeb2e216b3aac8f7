"""The packed index on the device (lsq_index_create_packed: rows of m code bytes and one norm byte, cbnorms once per index).  Its contract is an identity, so
every case is held to two references, bit for bit on distances and exactly on ids: (a) the untouched host scan lsq_linscan_aqd_query_extra_byte (or, with
inverted lists, lsq_ivf_search_cpu) on the widened norms cbnorms[norm_codes], and (b) a plain Index on the same engine with those norms -- whose
selection statistics (exhaustive flag, threshold rank, list capacity, candidates, fallback queries, batches) must be equal as well: the fallback road repairs
the results of a sample that read the wrong rows, the statistics show it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivf_check as ic  # noqa: E402
import packed_check as pc  # noqa: E402
from knn_check import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
H = 256


def _cuda(*arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _pair(engine, codes, K, nc, cb, base=None):
    """(a packed index, its plain sibling on the widened norms), host arrays in and out"""
    m = codes.shape[1]
    return engine.index_packed(codes, K, nc, cb, m, base=base), engine.index(codes, K, cb[nc], m, base=base)


def _same(got, want, what):
    assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]), what


def _same_stats(packed, plain, what):
    a, b = packed.scan_stats(), plain.scan_stats()
    assert {k: a[k] for k in pc.STAT_KEYS} == {k: b[k] for k in pc.STAT_KEYS}, what
    return b


@pytest.mark.parametrize("m", [1, 2, 3, 7, 8, 11, 15, 16])
@pytest.mark.parametrize("n", [1, 63, 257, 4099])
def test_exhaustive_road(lsq, engine, n, m):
    """every dword width (m + 1 = 4, 8, 12, 16) and the byte loader on both sides of each; ragged query tiles of 16 (m <= 8) and of 8; NaN, infinities and
    -0.0 in the table"""
    import torch
    rng = np.random.default_rng(1000 * m + n)
    codes, K, nc, cb, Q = pc.problem(rng, n, m, 12, 33, special=True)
    ref = pc.host_scan(lsq._lib.load(), codes, K, cb[nc], Q, n)               # every query's full order, once: a smaller call is its corner
    packed, plain = _pair(engine, codes, K, nc, cb)
    dev = engine.index_packed_dev(*_cuda(codes, K, nc, cb), m)
    with packed, plain, dev:
        info = packed.packed_info()
        assert info["row_bytes"] == m + 1 and info["dword_rows"] == (1 if m in (3, 7, 11, 15) else 0) and info["ncb"] == 256
        assert info["ivf_row_bytes"] == 0 and info["resident_bytes"] == n * (m + 1) + 4 * 256
        assert plain.packed_info() == dict.fromkeys(info, 0)
        for nq in (1, 5, 17, 33):
            for nn in sorted({1, min(10, n), n}):
                got, want = packed.search(Q[:nq], nn), plain.search(Q[:nq], nn)
                _same(got, (ref[0][:nq, :nn], ref[1][:nq, :nn]), ("host scan", nq, nn))
                _same(got, want, ("plain index", nq, nn))
                assert _same_stats(packed, plain, (nq, nn))["exhaustive"] == 1
            dd, di = dev.search(torch.from_numpy(Q[:nq]).cuda(), min(10, n))
            _same((dd.cpu().numpy(), di.cpu().numpy()), (ref[0][:nq, :min(10, n)], ref[1][:nq, :min(10, n)]), ("device form", nq))


@pytest.mark.parametrize("m,zero_K", [(7, False), (8, False), (15, False), (16, False), (7, True), (8, True)])
@pytest.mark.parametrize("n", [65_600, 98_304])
def test_thresholded_road(lsq, engine, n, m, zero_K):
    """n / 16384 = 4 and 6: the sample reads rows s * stride of the PACKED array.  Under the plan's own rank, under rank 1 (the fallback for most queries) and
    with the exhaustive road forced.  zero codebooks: the distance is the norm, <= 256 distinct values over n rows -- massive ties"""
    rng = np.random.default_rng(m + n + 7 * zero_K)
    codes, K, nc, cb, Q = pc.problem(rng, n, m, 8, 40, zero_K=zero_K)
    ref = pc.host_scan(lsq._lib.load(), codes, K, cb[nc], Q, 100)
    packed, plain = _pair(engine, codes, K, nc, cb)
    with packed, plain:
        try:
            for option in (None, "linscan_rank", "linscan_exhaustive"):
                if option:
                    engine.set_option(option, 1)
                for nn in (1, 100):
                    got, want = packed.search(Q, nn), plain.search(Q, nn)
                    _same(got, (ref[0][:, :nn], ref[1][:, :nn]), ("host scan", option, nn))
                    _same(got, want, ("plain index", option, nn))
                    st = _same_stats(packed, plain, (option, nn))
                    assert st["exhaustive"] == (1 if option == "linscan_exhaustive" else 0), (option, nn, st)
                    if option == "linscan_rank":
                        assert st["threshold_rank"] == 1
                        if nn == 100 and not zero_K:                          # a list of the rows below the sample's minimum is short of 100: redone
                            assert st["fallback_queries"] > 0                 # (zero codebooks: the n / 256 rows that tie the minimum fill it)
                    if option is None and not zero_K:
                        assert st["fallback_queries"] == 0 and st["candidates"] < 40 * n // 4      # exchangeable data: the threshold did the work
                if option:
                    engine.set_option(option, 0)
        finally:
            engine.set_option("linscan_rank", 0)
            engine.set_option("linscan_exhaustive", 0)


@pytest.mark.parametrize("m", [7, 8])
@pytest.mark.parametrize("edge", ["ncb1", "ncb256", "ncb37", "nan", "inf-negzero", "duplicates"])
def test_table_edges(lsq, engine, m, edge):
    rng = np.random.default_rng(31 * m + len(edge))
    n = 257
    ncb = {"ncb1": 1, "ncb37": 37}.get(edge, 256)
    codes, K, nc, cb, Q = pc.problem(rng, n, m, 12, 5, ncb=ncb)
    assert (nc == ncb - 1).any() and nc.max() == ncb - 1                       # the table's last entry is in use (byte 255, byte 36, byte 0)
    if edge == "nan":
        cb[[0, 100, 255]] = np.float32(np.nan)                                # NaN rows sort after every number
    if edge == "inf-negzero":
        cb[7], cb[8], cb[9] = np.float32(np.inf), np.float32(-0.0), np.float32(-np.inf)
        K[:] = 0                                                              # the distance is the norm itself: +inf, (0 + -0.0), -inf rows
    if edge == "duplicates":
        codes[n // 2:2 * (n // 2)] = codes[:n // 2]                           # equal rows with equal norm bytes: ties go by id
        nc[n // 2:2 * (n // 2)] = nc[:n // 2]
    ref = pc.host_scan(lsq._lib.load(), codes, K, cb[nc], Q, n)
    packed, plain = _pair(engine, codes, K, nc, cb)
    with packed, plain:
        assert packed.packed_info()["ncb"] == ncb and packed.packed_info()["resident_bytes"] == n * (m + 1) + 4 * ncb
        for nn in (1, 10, n):
            got = packed.search(Q, nn)
            _same(got, (ref[0][:, :nn], ref[1][:, :nn]), (edge, "host scan", nn))
            _same(got, plain.search(Q, nn), (edge, "plain index", nn))
            _same_stats(packed, plain, (edge, nn))
        if edge == "nan":
            assert np.isnan(got[0][:, -1]).all() and not np.isnan(got[0][:, 0]).any()
        if edge == "duplicates":
            first = got[1][:, 0]
            assert all((got[1][q, 1] == first[q] + n // 2) for q in range(5) if first[q] <= n // 2)


@pytest.mark.parametrize("form", ["host", "device"])
def test_a_norm_byte_outside_the_table_is_refused_before_the_index_exists(lsq, engine, form):
    rng = np.random.default_rng(3)
    n, m, ncb = 1000, 7, 37
    codes, K, nc, cb, Q = pc.problem(rng, n, m, 12, 5, ncb=ncb)
    for row in (0, n - 1, n // 2):
        bad = nc.copy()
        bad[row] = ncb
        args = (codes, bad, cb, K)
        rc, handle = pc.raw_create(lsq, engine, *(_cuda(*args) if form == "device" else args), on_device=form == "device")
        assert rc == lsq._lib.LSQ_EINVAL and handle is None, (row, rc, handle)
        assert b"norm bytes" in engine._L.lsq_last_error()
        with pytest.raises(lsq._lib.LsqError) as e:
            if form == "device":
                engine.index_packed_dev(*_cuda(codes, K, bad, cb), m)
            else:
                engine.index_packed(codes, K, bad, cb, m)
        assert e.value.code == lsq._lib.LSQ_EINVAL
    rc, handle = pc.raw_create(lsq, engine, *(_cuda(codes, nc, cb, K) if form == "device" else (codes, nc, cb, K)), on_device=form == "device")
    assert rc == 0 and handle                                                 # the same arrays with the byte in range
    # the engine is usable afterwards
    packed, plain = _pair(engine, codes, K, nc, cb)
    with packed, plain:
        _same(packed.search(Q, 10), plain.search(Q, 10), "after the refusals")
    with pytest.raises(TypeError):
        engine.index_packed(codes, K, nc.astype(np.int16), cb, m)
    with pytest.raises(ValueError):
        engine.index_packed(codes, K, nc[:-1], cb, m)
    with pytest.raises(ValueError):
        engine.index_packed(codes, K, nc, np.zeros(257, dtype=np.float32), m)


def test_the_index_owns_its_rows(lsq, engine):
    """device form: the caller's codes, norm bytes and table are read once; garbage written over them afterwards changes nothing"""
    import torch
    rng = np.random.default_rng(5)
    n, m = 3000, 7
    codes, K, nc, cb, Q = pc.problem(rng, n, m, 12, 9)
    cent = rng.standard_normal((8, 12)).astype(np.float32)
    lor = rng.integers(0, 8, n).astype(np.int32)
    dcodes, dK, dnc, dcb, dQ = _cuda(codes, K, nc, cb, Q)
    plain = engine.index(codes, K, cb[nc], m)
    packed = engine.index_packed_dev(dcodes, dK, dnc, dcb, m)
    with packed, plain:
        dcodes.fill_(255)
        dnc.fill_(255)
        dcb.fill_(float("nan"))
        torch.cuda.synchronize()
        plain.set_lists(cent, lor)
        packed.set_lists(*_cuda(cent, lor))
        for nn in (1, 50):
            dd, di = packed.search(dQ, nn)
            _same((dd.cpu().numpy(), di.cpu().numpy()), plain.search(Q, nn), ("search", nn))
            dd, di = packed.search_ivf(dQ, nn, 3)
            _same((dd.cpu().numpy(), di.cpu().numpy()), plain.search_ivf(Q, nn, 3), ("search_ivf", nn))


def _ivf_pair(engine, p, base=None):
    """the problem with its norms snapped to a table of <= 256 entries -> (the problem on those norms, packed index, plain index), lists set on both"""
    codes, K, dbn, cent, lor, Qs, Qc = p
    cb, nc = pc.quantize(dbn)
    q = (codes, K, cb[nc], cent, lor, Qs, Qc)
    packed, plain = _pair(engine, codes, K, nc, cb, base=base)
    packed.set_lists(cent, lor)
    plain.set_lists(cent, lor)
    return q, packed, plain


def _ivf_roads(lsq, q, packed, plain, nprobe, nn, what):
    """both roads, the small batches and the coarse add: the host checker on the widened norms, and the plain index with its road counts"""
    L = lsq._lib.load()
    Qs, Qc = q[5], q[6]
    for add in (0, ic.ADD_COARSE):
        rc, rd, ri = ic.ivf_cpu(L, *q, nprobe, nn, flags=add)
        assert rc == 0
        for flags in (0, ic.EVERY_RECORD, ic.TEST_BATCH, ic.TEST_BATCH | ic.EVERY_RECORD):
            got = packed.search_ivf(Qs, nn, nprobe, Q_coarse=Qc, flags=flags | add)
            a = packed.ivf_info()
            _same(got, (rd, ri), (what, "host checker", add, flags))
            _same(got, plain.search_ivf(Qs, nn, nprobe, Q_coarse=Qc, flags=flags | add), (what, "plain index", add, flags))
            b = plain.ivf_info()
            assert {k: a[k] for k in pc.IVF_KEYS} == {k: b[k] for k in pc.IVF_KEYS}, (what, add, flags)


@pytest.mark.parametrize("m", [7, 8, 12, 15])
def test_inverted_lists_on_a_packed_index(lsq, engine, m):
    """skewed lists: empty ones, one-row ones, one of half the base; m + 1 = 8 and 16 read dwords, 9 and 13 bytes"""
    p = ic.problem(ic.N, 32, m, 40, 37, 300 + m)
    p[2][5::97] = np.float32(np.nan)
    q, packed, plain = _ivf_pair(engine, p)
    with packed, plain:
        info = packed.packed_info()
        assert info["ivf_row_bytes"] == m + 5 and info["row_bytes"] == m + 1 and plain.packed_info()["ivf_row_bytes"] == 0
        for nn in (1, 300):                                                   # every list probed: the exhaustive scan's result
            _same(packed.search_ivf(q[5], nn, 40, Q_coarse=q[6]), packed.search(q[5], nn), ("nprobe = nlist", nn))
        for nprobe, nn in ((3, 10), (3, 300), (1, 1), (12, 10)):
            _ivf_roads(lsq, q, packed, plain, nprobe, nn, (m, nprobe, nn))


@pytest.mark.parametrize("name", sorted(ic.PROBLEMS))
def test_named_list_problems_on_a_packed_index(lsq, engine, name):
    """the routes a shape selects -- blocks that walk several lists, tails filled to the record and over, queries redone in fall-back batches, a NaN tau,
    infinities beside the padding, the layout's edges -- on packed rows"""
    p, nprobe, nn = ic.PROBLEMS[name]()
    q, packed, plain = _ivf_pair(engine, p)
    with packed, plain:
        _ivf_roads(lsq, q, packed, plain, nprobe, nn, name)
        if name in ("capacity-34", "mixed", "nan-tau"):
            packed.search_ivf(q[5], nn, nprobe, Q_coarse=q[6])
            assert packed.ivf_info()["fallback_queries"] > 0, name              # (the tails still overflow on the snapped norms)


@pytest.mark.parametrize("base_u8", [False, True])
def test_stage_two_and_knn_behind_a_packed_index(lsq, engine, base_u8):
    rng = np.random.default_rng(17 + base_u8)
    n, m, d = 3000, 7, 32
    codes, K, nc, cb, Qs = pc.problem(rng, n, m, d, 9)
    base = rng.integers(0, 256, (n, d)).astype(np.uint8) if base_u8 else rng.standard_normal((n, d)).astype(np.float32)
    Qe = rng.standard_normal((9, d)).astype(np.float32) * (64 if base_u8 else 1)
    cent = rng.standard_normal((8, d)).astype(np.float32)
    lor = rng.integers(0, 8, n).astype(np.int32)
    cand = rng.integers(0, n + 2, (9, 60)).astype(np.int32)                  # some ids outside the base
    packed, plain = _pair(engine, codes, K, nc, cb, base=base)
    with packed, plain:
        packed.set_lists(cent, lor)
        plain.set_lists(cent, lor)
        _same(packed.search(Qs, 10, shortlist=50, Q_exact=Qe), plain.search(Qs, 10, shortlist=50, Q_exact=Qe), "search(shortlist)")
        _same(packed.search_ivf(Qs, 10, 3, shortlist=50, Q_exact=Qe), plain.search_ivf(Qs, 10, 3, shortlist=50, Q_exact=Qe), "search_ivf(shortlist)")
        _same(packed.rerank(Qe, cand, 10), plain.rerank(Qe, cand, 10), "rerank")
        _same(packed.knn(Qe, 10), plain.knn(Qe, 10), "knn")
        if base_u8:
            Q8 = rng.integers(0, 256, (9, d)).astype(np.uint8)
            _same(packed.knn(Q8, 10), plain.knn(Q8, 10), "knn, integer road")
            assert packed.knn_info()["int_road"] == 1


def test_neighbours_on_one_context(lsq, engine):
    """a packed and a plain index of DIFFERENT data on one context, their calls interleaved, reproduce their solo results; set_lists again replaces the lists"""
    rng = np.random.default_rng(23)
    L = lsq._lib.load()
    a = pc.problem(rng, 70_000, 7, 8, 20)                                     # thresholded scans
    b = pc.problem(rng, 3000, 8, 8, 33)
    cent = rng.standard_normal((16, 8)).astype(np.float32)
    lor1, lor2 = rng.integers(0, 16, 70_000).astype(np.int32), rng.integers(0, 5, 70_000).astype(np.int32)
    packed = engine.index_packed(a[0], a[1], a[2], a[3], 7)
    plain = engine.index(b[0], b[1], b[3][b[2]], 8)
    with packed, plain:
        packed.set_lists(cent, lor1)
        solo_a = (packed.search(a[4], 100), packed.search_ivf(a[4], 10, 4))
        solo_b = plain.search(b[4], 10)
        for _ in range(2):
            _same(packed.search(a[4], 100), solo_a[0], "packed, interleaved")
            _same(plain.search(b[4], 10), solo_b, "plain, interleaved")
            _same(packed.search_ivf(a[4], 10, 4), solo_a[1], "packed lists, interleaved")
        _same(solo_a[0], pc.host_scan(L, a[0], a[1], a[3][a[2]], a[4], 100), "packed against the host scan")
        for lor, nlist in ((lor2, 5), (lor1, 16)):                             # replaced, and put back
            packed.set_lists(cent[:nlist], lor)
            rc, rd, ri = ic.ivf_cpu(L, a[0], a[1], a[3][a[2]], cent[:nlist], lor, a[4], None, 2, 10)
            assert rc == 0
            _same(packed.search_ivf(a[4], 10, 2), (rd, ri), ("lists replaced", nlist))
            assert packed.packed_info()["ivf_row_bytes"] == 12
