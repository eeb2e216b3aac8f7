"""Row filters on the resident index on the device (lsq_index_set_filter): search, search_ivf and knn under a filter against the contract of
tests/filter_check.py -- the full ranking of the project's own host checkers with the filtered rows removed, cut to nn, padded -- bit for bit: both roads
(dense: the bitmap beside every row; compact: the list of allowed rows), every input form, host-buffer and device-tensor indexes, the scans' every-distance
and thresholded selections, the inverted lists in either order with the filter, stage two behind a filtered stage one, the identities, the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_check as FC  # noqa: E402
import ivf_check as ic  # noqa: E402
import packed_check as PC  # noqa: E402

pytestmark = pytest.mark.gpu
H = 256
EINVAL = -1
ROADS = {"dense": 1, "compact": 2}


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def _call(ix, method, Q, *args, **kw):
    """an Index search method with numpy arguments on either kind of index -> numpy (dists, ids)"""
    if ix._dev:
        Q = _t(Q)
        kw = {k: (_t(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    d, i = getattr(ix, method)(Q, *args, **kw)
    return _np(d), _np(i)


def _scan_problem(n, m, d, nq, seed):
    rng = np.random.default_rng(seed)
    K = (rng.standard_normal((m * H, d)) / np.sqrt(m)).astype(np.float32)
    codes = rng.integers(0, H, (n, m)).astype(np.uint8)
    recon = sum(K[j * H + codes[:, j].astype(np.int64)] for j in range(m))
    dbn = (recon.astype(np.float64) ** 2).sum(1).astype(np.float32)
    return codes, K, dbn, rng.standard_normal((nq, d)).astype(np.float32)


def _pair(engine, codes, K, dbn, m, base=None, packed=None):
    """a host-buffer index and a device-tensor one over the same rows (packed: (norm bytes, table) instead of dbn)"""
    tb = None if base is None else _t(base)
    if packed is not None:
        nc, cb = packed
        return engine.index_packed(codes, K, nc, cb, m, base=base), engine.index_packed_dev(_t(codes), _t(K), _t(nc), _t(cb), m, base=tb)
    return engine.index(codes, K, dbn, m, base=base), engine.index_dev(_t(codes), _t(K), _t(dbn), m, base=tb)


# ---- the scan, every-distance road: n = 1000 (the last bitmap word holds 8 rows), 37 queries (a ragged query tile) -----------------------------------
FORMATS = {"m8": (8, False), "m16": (16, False), "m5": (5, False), "packed-m7": (7, True), "packed-m8": (8, True)}


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_scan_every_distance_road(lsq, engine, fmt):
    L = lsq._lib.load()
    m, packed = FORMATS[fmt]
    n, nq, d = 1000, 37, 24
    codes, K, dbn, Q = _scan_problem(n, m, d, nq, 100 + m + packed)
    pk = None
    if packed:
        cb, nc = PC.quantize(dbn)
        dbn, pk = cb[nc], (nc, cb)
    full = FC.full_scan(L, codes, K, dbn, Q)
    hix, dix = _pair(engine, codes, K, dbn, m, packed=pk)
    with hix, dix:
        plain = {nn: _call(hix, "search", Q, nn) for nn in (1, 10, 100)}
        for name, allowed in FC.masks(n).items():
            want = {nn: FC.filtered(*full, allowed, nn, 0) for nn in (1, 10, 100)}
            for label, kw in FC.forms(allowed):
                for road in ROADS:
                    for ix in (hix, dix):
                        FC.set_filter(ix, road=road, **kw)
                        assert ix.filter_info()["allowed"] == int(allowed.sum()), (fmt, name, label)
                        for nn in (1, 10, 100):
                            got = _call(ix, "search", Q, nn)
                            assert FC.same(got, want[nn]), (fmt, name, label, road, ix._dev, nn)
                            if name == "all":
                                assert FC.same(got, plain[nn])
                        assert ix.filter_info()["road"] == ROADS[road] and ix.scan_stats()["exhaustive"] == 1
        # |A| = 7 < nn = 10: seven rows, then (+inf, 0)
        d7, i7 = _call(hix, "search", Q, 10)
        assert np.all(i7[:, 7:] == 0) and np.all(np.isposinf(d7[:, 7:])) and np.all(i7[:, :7] > 0)


# ---- the scan, thresholded road: n = 70 001 (> 65 536, odd) --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(lsq):
    n, nq, m, d = 70001, 20, 8, 16
    codes, K, dbn, Q = _scan_problem(n, m, d, nq, 31)
    full = FC.full_scan(lsq._lib.load(), codes, K, dbn, Q)
    rng = np.random.default_rng(32)
    far = np.zeros(n, dtype=bool)
    far[full[1][0, -35000:] - 1] = True                                       # the 35 000 rows farthest from query 0
    filters = {"half": rng.random(n) < 0.5, "1/64": rng.random(n) < 1.0 / 64, "far-from-q0": far, "15/16": np.arange(n) % 16 != 0}
    return codes, K, dbn, Q, full, filters


def test_scan_thresholded_road(lsq, engine, big):
    codes, K, dbn, Q, full, filters = big
    n, nn, nq = codes.shape[0], 10, Q.shape[0]
    seen = {"thresholded": 0, "fallback": 0, "exhaustive": 0}
    with engine.index(codes, K, dbn, 8) as ix:
        try:
            for option, value in ((None, 0), ("linscan_rank", 1), ("linscan_exhaustive", 1)):
                if option:
                    engine.set_option(option, value)
                for name, allowed in filters.items():
                    want = FC.filtered(*full, allowed, nn, 0)
                    for road in ROADS:
                        ix.set_filter(mask=allowed, road=road)
                        got = ix.search(Q, nn)
                        assert FC.same(got, want), (option, name, road)
                        st, info = ix.scan_stats(), ix.filter_info()
                        assert info["road"] == ROADS[road] and info["allowed"] == int(allowed.sum())
                        walked = n if road == "dense" else int(allowed.sum())
                        assert st["codes"] == walked
                        assert st["exhaustive"] == int(option == "linscan_exhaustive" or walked <= 65536), (option, name, road)
                        if option == "linscan_rank" and not st["exhaustive"]:
                            assert st["fallback_queries"] > 0, (name, road)       # a rank of 1 lists too few rows: redone with every record
                        seen["exhaustive"] += st["exhaustive"] * nq
                        seen["fallback"] += st["fallback_queries"]
                        seen["thresholded"] += (1 - st["exhaustive"]) * (nq - st["fallback_queries"])
                if option:
                    engine.set_option(option, 0)
        finally:
            engine.set_option("linscan_rank", 0)
            engine.set_option("linscan_exhaustive", 0)
    assert seen["thresholded"] > 0 and seen["fallback"] > 0 and seen["exhaustive"] > 0, seen


def test_default_road_above_the_small_database_limit(lsq, engine, big):
    """the header's rule at n = 70 001: compact up to n / 2 allowed rows, but not for 65 536 rows or fewer with allowed * 64 > n (they would take the
    every-distance selection where the dense road does not); either way the contract's result"""
    codes, K, dbn, Q, full, filters = big
    n = codes.shape[0]
    cases = dict(filters, **{"500": np.arange(n) % 140 == 7, "1093": np.arange(n) < 1093, "1094": np.arange(n) < 1094})
    with engine.index(codes, K, dbn, 8) as ix:
        assert ix.filter_info()["crossover_rows"] == n // 2
        for name, allowed in cases.items():
            ix.set_filter(mask=allowed)
            assert FC.same(ix.search(Q, 10), FC.filtered(*full, allowed, 10, 0)), name
            a = int(allowed.sum())
            assert ix.filter_info()["road"] == (2 if a <= n // 2 and not (a <= 65536 and a * 64 > n) else 1), (name, a)


# ---- inverted lists -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ivf(lsq):
    """3000 rows on 40 skewed lists (empty lists, one-row lists, one list of half the rows), norms on a 256-entry table so that a plain and a packed index
    hold the same database"""
    L = lsq._lib.load()
    codes, K, dbn, cent, lor, Qs, Qc = ic.problem(ic.N, 32, 8, 40, 37, 77)
    cb, nc = PC.quantize(dbn)
    p = (codes, K, cb[nc], cent, lor, Qs, Qc)
    n = codes.shape[0]
    rng = np.random.default_rng(78)
    probes = ic.probes_np(cent, Qc, 3)[1]
    nearest = lor != probes[0, 0]                                             # every row of query 0's nearest list filtered
    few = np.zeros(n, dtype=bool)                                             # fewer than nn = 10 allowed rows in ANY three lists: 2 per list at most
    for l in range(40):
        few[np.flatnonzero(lor == l)[:2]] = True
    filters = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "half": rng.random(n) < 0.5, "tenth": rng.random(n) < 0.1,
               "nearest-list-of-q0": nearest, "few": few}
    full = {(nprobe, add): FC.full_ivf(L, p, nprobe, flags=ic.ADD_COARSE if add else 0) for nprobe in (1, 3, 40) for add in (False, True)}
    return p, (nc, cb), filters, full


@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
def test_ivf_under_a_filter(lsq, engine, ivf, packed):
    p, pk, filters, full = ivf
    codes, K, dbn, cent, lor, Qs, Qc = p
    n, nlist = codes.shape[0], cent.shape[0]
    hix, dix = _pair(engine, codes, K, dbn, 8, packed=pk if packed else None)
    thresholded = fallback = 0
    with hix, dix:
        for at, (name, allowed) in enumerate(filters.items()):
            for ix in (hix, dix):
                # the filter before the lists on even cases, after them on odd ones; each replaced once more afterwards in the other order
                steps = [lambda: FC.set_filter(ix, mask=allowed), lambda: ix.set_lists(*((_t(cent), _t(lor)) if ix._dev else (cent, lor)))]
                for step in (steps if at % 2 == 0 else steps[::-1]) + (steps[::-1] if at % 2 == 0 else steps):
                    step()
                info = ix.filter_info()
                assert (info["allowed"], info["lists"], info["lists_without_allowed"]) == \
                    (int(allowed.sum()), nlist, FC.lists_without_allowed(lor, allowed, nlist)), (name, ix._dev)
                for nprobe, nn in ((1, 10), (3, 10), (40, 10), (40, 300)):
                    for add in (False, True):
                        want = FC.filtered(*full[(nprobe, add)], allowed, nn, 0)
                        for every in (False, True):
                            for flags in ((0, ic.TEST_BATCH) if nprobe == 3 else (0,)):
                                got = _call(ix, "search_ivf", Qs, nn, nprobe, Q_coarse=Qc, add_coarse=add, every_record=every, flags=flags)
                                assert FC.same(got, want), (name, ix._dev, nprobe, nn, add, every, flags)
                                st = ix.ivf_info()
                                assert st["queries"] == Qs.shape[0]
                                if not every:
                                    thresholded += st["threshold_queries"]
                                    fallback += st["fallback_queries"]
                                else:
                                    assert st["threshold_queries"] == 0
                    if nprobe == 40 and nn == 10:                              # every list probed, no flag: the filtered scan of every row
                        assert FC.same(_call(ix, "search_ivf", Qs, nn, 40, Q_coarse=Qc), _call(ix, "search", Qs, nn)), (name, ix._dev)
        assert hix.filter_info()["road"] == 1
    assert thresholded > 0, "no filtered query was answered by the thresholded road: the head on allowed counts does not work"


def test_ivf_overflowing_tail_is_redone_under_a_filter(lsq, engine):
    """ivf_check's mixed problem: the even queries' tail rows all tie tau and overflow the tail -- under a filter that keeps 9 rows in 10 still 470 against
    264 slots -- while the odd queries are answered by the thresholded road"""
    L = lsq._lib.load()
    p, nprobe, nn = ic.mixed_problem()
    n = p[0].shape[0]
    allowed = np.arange(n) % 10 != 3
    want = FC.filtered(*FC.full_ivf(L, p, nprobe), allowed, nn, 0)
    with engine.index(p[0], p[1], p[2], 8) as ix:
        ix.set_lists(p[3], p[4])
        ix.set_filter(mask=allowed)
        for flags in (0, ic.TEST_BATCH):
            assert FC.same(ix.search_ivf(p[5], nn, nprobe, Q_coarse=p[6], flags=flags), want)
            st = ix.ivf_info()
            assert st["fallback_queries"] > 0 and st["threshold_queries"] > 0 and st["fallback_queries"] + st["threshold_queries"] == p[5].shape[0]
            assert st["probed_rows"] == nprobe * 75 * p[5].shape[0]           # filtered rows are read, and counted


# ---- exact k-NN -------------------------------------------------------------------------------------------------------------------------------------------
def _knn_case(kind, n, d, nq, seed):
    rng = np.random.default_rng(seed)
    if kind == "f32":
        return rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)
    base = rng.integers(0, 256, (n, d)).astype(np.uint8)
    Q = rng.integers(0, 256, (nq, d)).astype(np.uint8)
    return base, (Q if kind == "u8-u8" else Q.astype(np.float32))


@pytest.mark.parametrize("kind,n,d", [("f32", 777, 20), ("u8-u8", 777, 128), ("u8-f32", 777, 128), ("f32", 70001, 4), ("u8-u8", 70001, 8)],
                         ids=lambda v: str(v))
def test_knn_under_a_filter(lsq, engine, kind, n, d):
    """n = 777: every distance written; n = 70 001: the thresholded selection (dense, and compact over 65 626 rows) and its every-distance form (compact over
    fewer rows).  uint8 x uint8 takes the integer road, uint8 x f32 the widened one"""
    L = lsq._lib.load()
    base, Q = _knn_case(kind, n, d, 19, 40 + d)
    full = FC.full_knn(L, base, Q)
    masks = FC.masks(n, seed=n)
    names = ("all", "none", "half", "seven", "last-word") if n < 65536 else ("half", "hundredth")
    masks = {k: masks[k] for k in names}
    if n > 65536:
        masks["15/16"] = np.arange(n) % 16 != 0
    hix, dix = engine.index(None, None, None, 0, base=base), engine.index_dev(None, None, None, 0, base=_t(base))
    with hix, dix:
        for name, allowed in masks.items():
            for road in ROADS:
                for ix in (hix, dix):
                    FC.set_filter(ix, road=road, mask=allowed)
                    for id_base in (0, 1):
                        shifted = (full[0], full[1] + id_base)
                        for nn in (1, 10, 100):
                            got = _call(ix, "knn", Q, nn, id_base=id_base)
                            assert FC.same(got, FC.filtered(*shifted, allowed, nn, id_base - 1)), (kind, n, name, road, ix._dev, id_base, nn)
                    info, kinfo = ix.filter_info(), ix.knn_info()
                    assert info["road"] == ROADS[road] and kinfo["int_road"] == int(kind == "u8-u8")
                    walked = n if road == "dense" else int(allowed.sum())
                    assert kinfo["exhaustive"] == int(walked <= 65536), (name, road)


# ---- two stages ------------------------------------------------------------------------------------------------------------------------------------------
def test_shortlists_longer_than_the_allowed_set(lsq, engine, ivf):
    L = lsq._lib.load()
    p, _, filters, full_ivf = ivf
    codes, K, dbn, cent, lor, Qs, Qc = p
    n = codes.shape[0]
    base = np.random.default_rng(55).standard_normal((n, 32)).astype(np.float32)
    Qe = Qs + np.float32(0.5)
    full = FC.full_scan(L, codes, K, dbn, Qs)
    seven = FC.masks(n)["seven"]
    hix, dix = _pair(engine, codes, K, dbn, 8, base=base)
    with hix, dix:
        for ix in (hix, dix):
            ix.set_lists(*((_t(cent), _t(lor)) if ix._dev else (cent, lor)))
            for name, allowed in (("seven", seven), ("tenth", filters["tenth"])):
                FC.set_filter(ix, mask=allowed)
                Lst, nn = 50 if name == "seven" else 400, 10                    # 50 > 7, 400 > ~300 allowed rows
                assert Lst > allowed.sum()
                stage1 = FC.filtered(*full, allowed, Lst, 0)[1]
                assert FC.same(_call(ix, "search", Qs, nn, shortlist=Lst, Q_exact=Qe), FC.two_stage(L, stage1, base, Qe, nn)), (name, ix._dev)
                stage1 = FC.filtered(*full_ivf[(3, False)], allowed, Lst, 0)[1]
                got = _call(ix, "search_ivf", Qs, nn, 3, shortlist=Lst, Q_coarse=Qc, Q_exact=Qe)
                assert FC.same(got, FC.two_stage(L, stage1, base, Qe, nn)), (name, ix._dev)
                if name == "seven":
                    assert np.all(got[1][:, 7:] == 0) and np.all(np.isposinf(got[0][:, 7:]))


# ---- identities ------------------------------------------------------------------------------------------------------------------------------------------
def test_identities(lsq, engine, ivf):
    p, _, filters, _ = ivf
    codes, K, dbn, cent, lor, Qs, Qc = p
    n = codes.shape[0]
    base = np.random.default_rng(56).standard_normal((n, 32)).astype(np.float32)
    cand = np.random.default_rng(57).integers(0, n + 2, (Qs.shape[0], 40)).astype(np.int32)
    with engine.index(codes, K, dbn, 8, base=base) as ix, engine.index(codes, K, dbn, 8, base=base) as other:
        for x in (ix, other):
            x.set_lists(cent, lor)

        def everything(x):
            return [x.search(Qs, 10), x.search(Qs, 10, shortlist=30, Q_exact=Qs), x.search_ivf(Qs, 10, 3, Q_coarse=Qc), x.search_ivf(Qs, 300, 40, Q_coarse=Qc),
                    x.knn(Qs, 10), x.knn(Qs, 10, id_base=1), x.rerank(Qs, cand, 10, id_base=0)]

        plain = everything(ix)
        assert ix.filter_info()["active"] == 0 and ix.filter_info()["road"] == 0
        for road in (None, "dense", "compact"):
            ix.set_filter(mask=np.ones(n, dtype=bool), road=road)               # every row allowed: the unfiltered results
            assert ix.filter_info()["active"] == 1
            assert all(FC.same(a, b) for a, b in zip(everything(ix), plain)), road
        ix.set_filter(mask=filters["tenth"])
        under = everything(ix)
        assert FC.same(under[6], plain[6])                                      # rerank ignores the filter
        assert not FC.same(under[0], plain[0]) and not FC.same(under[4], plain[4])
        assert all(FC.same(a, b) for a, b in zip(everything(other), plain))     # a second index of the context knows nothing of it
        assert other.filter_info()["active"] == 0
        ix.clear_filter()
        info = ix.filter_info()
        assert info["active"] == 0 and info["allowed"] == 0
        assert all(FC.same(a, b) for a, b in zip(everything(ix), plain))
        assert ix.filter_info()["road"] == 0


# ---- refusals on the device, filter_info -----------------------------------------------------------------------------------------------------------------
def test_bad_ids_leave_the_former_filter_in_force(lsq, engine):
    L = lsq._lib.load()
    n = 1000
    codes, K, dbn, Q = _scan_problem(n, 8, 24, 5, 60)
    former = FC.masks(n)["tenth"]
    full = FC.full_scan(L, codes, K, dbn, Q)
    want = FC.filtered(*full, former, 10, 0)
    hix, dix = _pair(engine, codes, K, dbn, 8)
    with hix, dix:
        for ix in (hix, dix):
            FC.set_filter(ix, mask=former)
            for id_base in (0, 1):
                for bad in (id_base - 1, id_base + n):
                    ids = np.array([id_base, bad, id_base + n - 1], dtype=np.int32)
                    with pytest.raises(lsq._lib.LsqError) as e:
                        FC.set_filter(ix, ids=ids, id_base=id_base)
                    assert e.value.code == EINVAL and "outside" in str(e.value)
                    info = ix.filter_info()
                    assert info["active"] == 1 and info["allowed"] == int(former.sum())
                    assert FC.same(_call(ix, "search", Q, 10), want), (ix._dev, id_base, bad)
            FC.set_filter(ix, ids=np.array([id_base, id_base + n - 1], dtype=np.int32), id_base=id_base)      # the ends of the range are legal
            assert ix.filter_info()["allowed"] == 2
        # refusals that never reach the device: the former filter stays too
        desc = lsq._lib.FilterDesc()
        mask = np.ones(n, dtype=np.uint8)
        for form, data, count, id_base, flags in ((7, mask.ctypes.data, 0, 0, 0), (FC.BYTES, None, 0, 0, 0), (FC.BYTES, mask.ctypes.data, 0, 0, 8),
                                                  (FC.BYTES, mask.ctypes.data, 0, 0, FC.FORCE_DENSE | FC.FORCE_COMPACT),
                                                  (FC.IDS, mask.ctypes.data, -1, 0, 0), (FC.IDS, mask.ctypes.data, 1, 2, 0)):
            desc.form, desc.data, desc.count, desc.id_base, desc.flags, desc.on_device = form, data, count, id_base, flags, 0
            assert engine._L.lsq_index_set_filter(hix._h, C.byref(desc)) == EINVAL, (form, count, id_base, flags)
            assert hix.filter_info()["allowed"] == 2


def test_filter_info(lsq, engine):
    n = 1000
    codes, K, dbn, Q = _scan_problem(n, 8, 24, 3, 61)
    hix, dix = _pair(engine, codes, K, dbn, 8)
    with hix, dix:
        for ix in (hix, dix):
            info = ix.filter_info()
            assert (info["active"], info["n"], info["allowed"], info["lists"], info["lists_without_allowed"], info["road"]) == (0, n, 0, 0, 0, 0)
            assert info["crossover_rows"] == n // 2
            for name, allowed in FC.masks(n).items():
                for label, kw in FC.forms(allowed):
                    FC.set_filter(ix, **kw)
                    info = ix.filter_info()
                    assert (info["active"], info["n"], info["allowed"], info["lists"]) == (1, n, int(allowed.sum()), 0), (name, label)
                    _call(ix, "search", Q, 5)                                   # the default road: compact up to the crossover
                    assert ix.filter_info()["road"] == (2 if allowed.sum() <= info["crossover_rows"] else 1), (name, label)
            with pytest.raises(ValueError):
                ix.set_filter()
            with pytest.raises(ValueError):
                ix.set_filter(mask=np.ones(n, bool), ids=np.zeros(1, np.int32))
            with pytest.raises(ValueError):
                ix.set_filter(mask=np.ones(n, bool), road="sparse")
