"""Range search on the resident index on the device (lsq_index_range_search / _range_fetch): held, bit for bit -- lims, distances and ids -- to the contract
of tests/range_check.py, range_of(the host full ranking): the every-row walk in every row format and loader, ties and NaN, the fill batches (option
"range_batch"), the probed lists with and without the coarse term, the filter's roads, the index's life cycle (add, remove, compact), the held result and
the refusals.  Every case runs on a host-buffer index and on a device-tensor index over the same rows.  The non-vacuity conditions are asserted on the HOST
rankings."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_check as FC  # noqa: E402
import index_add_check as IA  # noqa: E402
import index_compact_check as IC  # noqa: E402
import ivf_check as ic  # noqa: E402
import packed_check as PC  # noqa: E402
import range_check as RC  # noqa: E402

pytestmark = pytest.mark.gpu
H = 256
EINVAL = -1
ROADS = {"dense": 1, "compact": 2}
FORMATS = {"m8": (8, False), "m16": (16, False), "m5": (5, False), "packed-m7": (7, True), "packed-m8": (8, True)}


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def _range(ix, Q, radius, **kw):
    """Index.range_search with numpy arguments on either kind of index -> numpy (lims, dists, ids)"""
    if ix._dev:
        Q = _t(Q)
        radius = _t(radius) if isinstance(radius, np.ndarray) else radius
        kw = {k: (_t(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    return tuple(_np(a) for a in ix.range_search(Q, radius, **kw))


def _scan_problem(n, m, d, nq, seed):
    rng = np.random.default_rng(seed)
    K = (rng.standard_normal((m * H, d)) / np.sqrt(m)).astype(np.float32)
    codes = rng.integers(0, H, (n, m)).astype(np.uint8)
    recon = sum(K[j * H + codes[:, j].astype(np.int64)] for j in range(m))
    dbn = (recon.astype(np.float64) ** 2).sum(1).astype(np.float32)
    return codes, K, dbn, rng.standard_normal((nq, d)).astype(np.float32)


def _pair(engine, codes, K, dbn, m, packed=None):
    """a host-buffer index and a device-tensor one over the same rows (packed: (norm bytes, table) instead of dbn)"""
    if packed is not None:
        nc, cb = packed
        return engine.index_packed(codes, K, nc, cb, m), engine.index_packed_dev(_t(codes), _t(K), _t(nc), _t(cb), m)
    return engine.index(codes, K, dbn, m), engine.index_dev(_t(codes), _t(K), _t(dbn), m)


def _formatted(fmt, n, d, nq, seed):
    """a scan problem in one of FORMATS -> codes, K, dbn (a packed format: the table's values), Q, packed (None or (norm bytes, table))"""
    m, packed = FORMATS[fmt]
    codes, K, dbn, Q = _scan_problem(n, m, d, nq, seed)
    pk = None
    if packed:
        cb, nc = PC.quantize(dbn)
        dbn, pk = cb[nc], (nc, cb)
    return m, codes, K, dbn, Q, pk


class _Seen:
    """the non-vacuity counters of a parametrisation, fed from the HOST rankings"""

    def __init__(self):
        self.empty = self.pairs = self.most = self.ties = 0

    def add(self, full, rad, want, pad_id=0, times=1):
        counts = np.diff(want[0])
        self.empty += int((counts == 0).sum())
        self.pairs += int(want[0][-1]) * times
        self.most = max(self.most, int(counts.max()))
        self.ties += RC.tie_cut_at_last_member(*full, rad, pad_id)


def _info_ok(ix, want, nq, road, rows_walked=None):
    info = ix.range_info()
    counts = np.diff(want[0])
    assert (info["queries"], info["results"], info["max_per_query"], info["road"]) == (nq, int(want[0][-1]), int(counts.max()), road), info
    assert info["held_bytes"] == 8 * int(want[0][-1]) and (info["batches"] >= 1) == (want[0][-1] > 0), info
    if rows_walked is not None:
        assert info["rows_walked"] == rows_walked, info


# ---- the every-row road: n = 1000 (the last bitmap word holds 8 rows, the row range is shorter than a block), 37 queries (a ragged tile at QT 16 and 8) --
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_every_row_road(lsq, engine, fmt):
    L = lsq._lib.load()
    n, nq, d = 1000, 37, 24
    m, codes, K, dbn, Q, pk = _formatted(fmt, n, d, nq, 500 + len(fmt))
    full = FC.full_scan(L, codes, K, dbn, Q)
    seen = _Seen()
    hix, dix = _pair(engine, codes, K, dbn, m, packed=pk)
    with hix, dix:
        for name, rad in RC.radii(full[0]).items():
            want = RC.range_of(*full, rad, 0)
            seen.add(full, rad, want, times=2)
            for ix in (hix, dix):
                assert RC.same(_range(ix, Q, rad), want), (fmt, name, ix._dev)
                _info_ok(ix, want, nq, 0, rows_walked=nq * n)
        # a scalar radius is every query's radius
        want = RC.range_of(*full, np.float32(full[0][0, 99]), 0)
        for ix in (hix, dix):
            assert RC.same(_range(ix, Q, float(full[0][0, 99])), want)
        # no query
        for ix in (hix, dix):
            lims, dists, ids = _range(ix, Q[:0], np.zeros(0, np.float32))
            assert lims.tolist() == [0] and dists.shape == ids.shape == (0,)
    assert seen.empty >= 3 * nq and seen.most == n and seen.pairs > 10 ** 5, vars(seen)      # -inf, NaN, below-min: nothing; +inf: all n rows


def test_several_row_ranges_per_tile(lsq, engine):
    """n = 9000: three row ranges per query tile, so a query's count is the sum over blocks and its segment is filled by several"""
    L = lsq._lib.load()
    n, nq, d, m = 9000, 37, 24, 8
    codes, K, dbn, Q = _scan_problem(n, m, d, nq, 71)
    full = FC.full_scan(L, codes, K, dbn, Q)
    radii = RC.radii(full[0])
    hix, dix = _pair(engine, codes, K, dbn, m)
    with hix, dix:
        for name in ("+inf", "half", "10th", "mid-10-11", "-inf"):
            want = RC.range_of(*full, radii[name], 0)
            for ix in (hix, dix):
                assert RC.same(_range(ix, Q, radii[name]), want), (name, ix._dev)
                _info_ok(ix, want, nq, 0, rows_walked=nq * n)
        assert np.all(np.diff(RC.range_of(*full, radii["+inf"], 0)[0]) == n)


def test_more_queries_than_a_chunk(lsq, engine):
    """16 384 + 21 queries: the tables of 16 384 are resident together, so the count pass runs in two chunks, the counts come back once, and the fill pass
    builds each chunk's tables (and probed lists) again; the second chunk is a ragged tile.  Small rows keep it quick: n = 200, m = 2 (the byte loader)"""
    L = lsq._lib.load()
    n, nq, nlist, m = 200, 16384 + 21, 4, 2
    P = IA.problem(n, m, 4, nq, 77, nlist=nlist, lists="random")
    p = (P["codes"], P["K"], P["dbn"], P["cent"], P["lor"], P["Q"], P["Qc"])
    full, full_l = FC.full_scan(L, *p[:3], P["Q"]), FC.full_ivf(L, p, 2, flags=ic.ADD_COARSE)
    rad, rad_l = RC.radii(full[0])["10th"], RC.radii(full_l[0])["10th"]
    rad[16384:] = np.inf                                                     # the second chunk: every row
    want, want_l = RC.range_of(*full, rad, 0), RC.range_of(*full_l, rad_l, 0)
    assert np.all(np.diff(want[0])[16384:] == n) and want_l[0][-1] > want_l[0][16384] > 0
    hix, dix = IA.fresh(engine, P, n, dev=False), IA.fresh(engine, P, n, dev=True)
    try:
        with hix, dix:
            for budget in (0, 4096):                                         # one batch per chunk, and batches that end inside the chunks
                engine.set_option("range_batch", budget)
                for ix in (hix, dix):
                    assert RC.same(_range(ix, P["Q"], rad), want), (budget, ix._dev)
                    _info_ok(ix, want, nq, 0, rows_walked=nq * n)
                    assert ix.range_info()["batches"] >= 2
                    assert RC.same(_range(ix, P["Q"], rad_l, nprobe=2, Q_coarse=P["Qc"], add_coarse=True), want_l), (budget, ix._dev)
    finally:
        engine.set_option("range_batch", 0)


# ---- ties and NaN ---------------------------------------------------------------------------------------------------------------------------------------
def test_ties_and_nan(lsq, engine):
    L = lsq._lib.load()
    codes, K, dbn, cent, lor, Qs, Qc = ic.problem(1000, 5, 8, 16, 37, 41, small_int=True)
    dbn[::53] = np.float32(np.nan)
    nan_rows = np.arange(0, 1000, 53)
    full = FC.full_scan(L, codes, K, dbn, Qs)
    seen = _Seen()
    hix, dix = _pair(engine, codes, K, dbn, 8)
    with hix, dix:
        for name, rad in RC.radii(full[0]).items():
            want = RC.range_of(*full, rad, 0)
            seen.add(full, rad, want)
            for ix in (hix, dix):
                got = _range(ix, Qs, rad)
                assert RC.same(got, want), (name, ix._dev)
                assert not np.isnan(got[1]).any() and not np.isin(got[2] - 1, nan_rows).any()      # a NaN distance is never within a radius
        for ix in (hix, dix):
            lims, dists, ids = _range(ix, Qs, np.inf)
            assert np.all(np.diff(lims) == 1000 - nan_rows.shape[0])
            assert _range(ix, Qs, np.nan)[0][-1] == 0
    assert seen.ties > 0 and seen.empty > 0, vars(seen)                       # a radius equal to a tied distance: the group is cut at its last member


# ---- the fill batches -----------------------------------------------------------------------------------------------------------------------------------
def _batches(counts, budget):
    """the fill batches that hold records, by the header's rule: a batch takes queries while its records stay within the budget (0: 2^28), a query larger
    than the budget is a batch of its own, a batch without records launches nothing"""
    budget, made, q = (budget or 1 << 28), 0, 0
    while q < len(counts):
        records, q = int(counts[q]), q + 1
        while q < len(counts) and records + int(counts[q]) <= budget:
            records, q = records + int(counts[q]), q + 1
        made += records > 0
    return made


def test_batches_give_the_same_bits(lsq, engine):
    L = lsq._lib.load()
    n, nq, d, m = 1000, 37, 24, 8
    codes, K, dbn, Q = _scan_problem(n, m, d, nq, 73)
    full = FC.full_scan(L, codes, K, dbn, Q)
    rng = np.random.default_rng(74)
    rad = full[0][np.arange(nq), rng.integers(0, 200, nq)].copy()             # results of 1 .. 200 rows: some above a budget of 64, some below
    rad[5] = -np.inf                                                         # an empty result between the others
    rad[10:14] = full[0][np.arange(10, 14), 5]                               # four neighbours of six rows each: one batch at a budget of 64, four at 1
    want = RC.range_of(*full, rad, 0)
    counts = np.diff(want[0])
    assert (counts > 64).any() and ((counts > 0) & (counts < 64)).any() and (counts == 0).any()      # queries over the budget are present
    hix, dix = _pair(engine, codes, K, dbn, m)
    try:
        with hix, dix:
            batches = {}
            for budget in (0, 1, 64, 1000):
                engine.set_option("range_batch", budget)
                for ix in (hix, dix):
                    assert RC.same(_range(ix, Q, rad), want), (budget, ix._dev)
                    batches[budget] = ix.range_info()["batches"]
                    assert RC.same(_range(ix, Q, np.inf), RC.range_of(*full, np.inf, 0)), (budget, ix._dev)      # every query over every budget but 0
            assert batches == {b: _batches(counts, b) for b in batches} and 1 == batches[0] < batches[1000] < batches[64] < batches[1], batches
    finally:
        engine.set_option("range_batch", 0)
    assert L.lsq_set_option(engine._h, b"range_batch", -1) == EINVAL


# ---- the probed lists: 16 skewed lists -- empty ones, one-row ones, one of half the base -----------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["m8", "m5", "packed-m7", "packed-m8"])
def test_probed_lists(lsq, engine, fmt):
    L = lsq._lib.load()
    m, packed = FORMATS[fmt]
    n, nq, nlist = 1000, 37, 16
    P = IA.problem(n, m, 24, nq, 80 + m + packed, nlist=nlist, packed=packed)
    p = (P["codes"], P["K"], P["dbn"], P["cent"], P["lor"], P["Q"], P["Qc"])
    sizes = np.bincount(P["lor"], minlength=nlist)
    assert sizes.min() == 0 and (sizes == 1).any() and sizes.max() >= n // 2
    seen = _Seen()
    hix, dix = IA.fresh(engine, P, n, dev=False), IA.fresh(engine, P, n, dev=True)
    with hix, dix:
        for nprobe in (1, 4, 16):
            walked = int(sizes[ic.probes_np(P["cent"], P["Qc"], nprobe)[1]].sum())
            for add in (False, True):
                full = FC.full_ivf(L, p, nprobe, flags=ic.ADD_COARSE if add else 0)
                for name, rad in RC.radii(full[0]).items():
                    want = RC.range_of(*full, rad, 0)
                    seen.add(full, rad, want, times=2)
                    for ix in (hix, dix):
                        got = _range(ix, P["Q"], rad, nprobe=nprobe, Q_coarse=P["Qc"], add_coarse=add)
                        assert RC.same(got, want), (fmt, nprobe, add, name, ix._dev)
                        _info_ok(ix, want, nq, 0, rows_walked=walked)
        # every list probed, no flag: the every-row call, bit for bit
        rad = RC.radii(FC.full_scan(L, P["codes"], P["K"], P["dbn"], P["Q"])[0])["half"]
        for ix in (hix, dix):
            assert RC.same(_range(ix, P["Q"], rad, nprobe=nlist, Q_coarse=P["Qc"]), _range(ix, P["Q"], rad))
    assert seen.empty > 0 and seen.most == n and seen.pairs > 10 ** 5, vars(seen)


# ---- filters ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["m8", "packed-m7", "m5"])
def test_filters_on_the_every_row_road(lsq, engine, fmt):
    L = lsq._lib.load()
    n, nq, d = 1000, 37, 24
    m, codes, K, dbn, Q, pk = _formatted(fmt, n, d, nq, 600 + len(fmt))
    full = FC.full_scan(L, codes, K, dbn, Q)
    radii = RC.radii(full[0])
    seen = _Seen()
    hix, dix = _pair(engine, codes, K, dbn, m, packed=pk)
    with hix, dix:
        plain = {name: _range(hix, Q, radii[name]) for name in ("+inf", "half", "10th")}
        for mname, allowed in FC.masks(n).items():
            ranked = FC.filtered(*full, allowed, n, 0)                       # the full ranking of the allowed rows, then (+inf, 0)
            count = int(allowed.sum())
            for road in ("dense", "compact", None):
                expect = ROADS[road] if road else (2 if count <= n // 2 else 1)
                for ix in (hix, dix):
                    FC.set_filter(ix, road=road, mask=allowed)
                    for name in plain:
                        want = RC.range_of(*ranked, radii[name], 0)
                        seen.add(ranked, radii[name], want)
                        assert RC.same(_range(ix, Q, radii[name]), want), (fmt, mname, road, name, ix._dev)
                        _info_ok(ix, want, nq, expect, rows_walked=nq * (count if expect == 2 else n))
                        assert ix.filter_info()["road"] == expect
                        if mname == "all":
                            assert RC.same(_range(ix, Q, radii[name]), plain[name])
        for ix in (hix, dix):
            ix.clear_filter()
            for name in plain:
                assert RC.same(_range(ix, Q, radii[name]), plain[name])
            assert ix.range_info()["road"] == 0
    assert seen.empty > 0 and seen.most == n, vars(seen)


@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
def test_filters_on_the_list_road(lsq, engine, packed):
    L = lsq._lib.load()
    n, nq, nlist, m = 1000, 37, 16, 7 if packed else 8
    P = IA.problem(n, m, 24, nq, 90 + packed, nlist=nlist, packed=packed)
    p = (P["codes"], P["K"], P["dbn"], P["cent"], P["lor"], P["Q"], P["Qc"])
    hix, dix = IA.fresh(engine, P, n, dev=False), IA.fresh(engine, P, n, dev=True)
    empties = 0
    with hix, dix:
        for nprobe, add in ((4, False), (4, True), (16, False)):
            full = FC.full_ivf(L, p, nprobe, flags=ic.ADD_COARSE if add else 0)
            radii = RC.radii(full[0])
            for mname, allowed in FC.masks(n).items():
                ranked = FC.filtered(*full, allowed, n, 0)
                for ix in (hix, dix):
                    FC.set_filter(ix, mask=allowed)
                    for name in ("+inf", "10th"):
                        want = RC.range_of(*ranked, radii[name], 0)
                        empties += int((np.diff(want[0]) == 0).sum())
                        assert RC.same(_range(ix, P["Q"], radii[name], nprobe=nprobe, Q_coarse=P["Qc"], add_coarse=add), want), (nprobe, add, mname, name, ix._dev)
                        assert ix.range_info()["road"] == 1 and ix.filter_info()["road"] == 1      # the layout-order bits: always the dense road
    assert empties > 0


# ---- the life cycle: add -> remove -> compact -> add on a listed index, against a fresh index over the same rows after each step -------------------------------
@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
def test_lifecycle(lsq, engine, packed):
    L = lsq._lib.load()
    n, n0, n1, nq, nlist, m = 1000, 600, 900, 37, 16, 7 if packed else 8
    P = IA.problem(n, m, 24, nq, 95 + packed, nlist=nlist, packed=packed)

    def calls(ix, Px, radii):
        """the compared calls on one index: every row and the probed lists, three radii"""
        out = {}
        for name in ("+inf", "half", "10th"):
            out["rows", name] = _range(ix, Px["Q"], radii[name])
            out["lists", name] = _range(ix, Px["Q"], radii[name], nprobe=4, Q_coarse=Px["Qc"], add_coarse=True)
        return out

    def agree(ix, Px, rows, allowed=None):
        """ix answers as the fresh index over the first `rows` rows of Px (under the same allowed set), and as the host drop-in"""
        radii = RC.radii(FC.full_scan(L, Px["codes"][:rows], Px["K"], Px["dbn"][:rows], Px["Q"])[0])
        with IA.fresh(engine, Px, rows, dev=ix._dev) as fx:
            if allowed is not None:
                FC.set_filter(fx, mask=allowed)
            got, want = calls(ix, Px, radii), calls(fx, Px, radii)
        for k in got:
            assert RC.same(got[k], want[k]), (k, rows)
        rc, lims, dists, ids = RC.range_cpu(L, Px["codes"][:rows], Px["K"], Px["dbn"][:rows], Px["Q"], radii["half"], allowed=allowed)
        assert rc == 0 and RC.same(got["rows", "half"], (lims, dists, ids)) and lims[-1] > 0

    for dev in (False, True):
        with IA.fresh(engine, P, n0, dev=dev) as ix:
            IA.grow(ix, P, n0, n1, dev=dev)                                  # add
            assert ix.n == n1
            agree(ix, P, n1)
            removed = np.unique(np.concatenate([[0, n1 - 1], np.arange(64, 96), np.random.default_rng(3).permutation(n1)[:n1 // 3]])).astype(np.int32)
            ix.remove(_t(removed) if dev else removed)                       # remove: the rows are hidden
            allowed = np.ones(n1, dtype=bool)
            allowed[removed] = False
            agree(ix, P, n1, allowed=allowed)
            old_of_new = _np(ix.compact())                                   # compact: the rows leave
            assert np.array_equal(old_of_new, np.flatnonzero(allowed))
            Ps = IC.sub({k: (v[:n1] if k in IC.PER_ROW else v) for k, v in P.items()}, old_of_new)
            agree(ix, Ps, Ps["n"])
            # add again: the last 100 rows of the problem behind the survivors
            Pg = dict(Ps)
            for k in IC.PER_ROW:
                if k in P:
                    Pg[k] = np.ascontiguousarray(np.concatenate([Ps[k], P[k][n1:]]))
            Pg["n"] = Ps["n"] + (n - n1)
            IA.grow(ix, Pg, Ps["n"], Pg["n"], dev=dev)
            agree(ix, Pg, Pg["n"])


# ---- the held result --------------------------------------------------------------------------------------------------------------------------------------
def _fetch(ix, capacity, guard=8, poison=-77):
    """lsq_index_range_fetch itself into poisoned arrays of capacity + guard entries -> (rc, dists, ids) as numpy"""
    size = max(capacity, 0) + guard
    if ix._dev:
        import torch
        d = torch.full((size,), float(poison), dtype=torch.float32, device="cuda")
        i = torch.full((size,), int(poison), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                                             # the poison has landed before the library's stream writes
        rc = ix._L.lsq_index_range_fetch(ix._h, d.data_ptr(), i.data_ptr(), capacity, 1)
        torch.cuda.synchronize()
        return rc, d.cpu().numpy(), i.cpu().numpy()
    d, i = np.full(size, poison, np.float32), np.full(size, poison, np.int32)
    return ix._L.lsq_index_range_fetch(ix._h, d.ctypes.data, i.ctypes.data, capacity, 0), d, i


def test_held_result(lsq, engine):
    L = lsq._lib.load()
    n, nq, m = 1000, 37, 8
    P = IA.problem(n + 50, m, 24, nq, 97, nlist=16)
    full = FC.full_scan(L, P["codes"][:n], P["K"], P["dbn"][:n], P["Q"])
    rad = RC.radii(full[0])["10th"]
    want = RC.range_of(*full, rad, 0)
    total = int(want[0][-1])
    assert total > 8
    for dev in (False, True):
        with IA.fresh(engine, P, n, dev=dev, lists=False) as ix:
            rc, d, i = _fetch(ix, 10)
            assert rc == EINVAL and b"lsq_index_range_fetch" in engine._L.lsq_last_error()      # nothing held yet
            assert RC.same(_range(ix, P["Q"], rad), want)
            for _ in range(2):                                               # fetch twice: the same bits, nothing past the result
                rc, d, i = _fetch(ix, total)
                assert rc == 0 and RC.same((want[0], d[:total], i[:total]), want) and np.all(d[total:] == -77) and np.all(i[total:] == -77)
            rc, d, i = _fetch(ix, total + 5)                                 # more room than needed: exactly `total` entries are written
            assert rc == 0 and RC.same((want[0], d[:total], i[:total]), want) and np.all(d[total:] == -77) and np.all(i[total:] == -77)
            rc, d, i = _fetch(ix, total - 1)                                 # too little: refused, nothing written, the guard zone untouched
            assert rc == EINVAL and np.all(d == -77) and np.all(i == -77)
            ix.search(_t(P["Q"]) if dev else P["Q"], 10)                     # a search does not drop it
            rc, d, i = _fetch(ix, total)
            assert rc == 0 and RC.same((want[0], d[:total], i[:total]), want)
            assert ix.range_info()["held_bytes"] == 8 * total
            # every call that changes what a search would see drops it
            def held():
                return _fetch(ix, total + 100)[0] == 0

            for change in ("set_filter", "clear_filter", "set_lists", "add", "remove", "compact"):
                _range(ix, P["Q"], rad)
                assert held(), change
                if change == "set_filter":
                    FC.set_filter(ix, mask=np.arange(ix.n) % 2 == 0)
                elif change == "clear_filter":
                    ix.clear_filter()
                elif change == "set_lists":
                    ix.set_lists(_t(P["cent"]) if dev else P["cent"], _t(P["lor"][:n]) if dev else P["lor"][:n])
                elif change == "add":
                    IA.grow(ix, P, n, n + 50, dev=dev)
                elif change == "remove":
                    ids = np.array([1, 2, 3], np.int32)
                    ix.remove(_t(ids) if dev else ids)
                else:
                    ix.compact()
                assert not held(), change
            # an add / remove of nothing changes nothing: the result stays
            _range(ix, P["Q"], rad)
            ix.remove(np.zeros(0, np.int32))
            assert held()


# ---- refusals: LSQ_EINVAL, nothing launched, a former held result still fetchable ----------------------------------------------------------------------------
def test_refusals(lsq, engine):
    L = lsq._lib.load()
    n, nq, m, d = 1000, 37, 8, 24
    P = IA.problem(n, m, d, nq, 99, nlist=16)
    full = FC.full_scan(L, P["codes"], P["K"], P["dbn"], P["Q"])
    rad = RC.radii(full[0])["10th"]
    want = RC.range_of(*full, rad, 0)
    total = int(want[0][-1])
    Q, lims = P["Q"], np.full(nq + 1, -7, np.int64)
    ptr = lambda a: a.ctypes.data      # noqa: E731
    with IA.fresh(engine, P, n, lists=False) as ix, engine.index(None, None, None, 0, base=np.zeros((4, d), np.float32), d=d) as bx:
        assert RC.same(_range(ix, Q, rad), want)
        raw = engine._L.lsq_index_range_search

        def refused(rc):
            assert rc == EINVAL and b"lsq_index_range_search" in engine._L.lsq_last_error() and np.all(lims == -7)
            rc2, dd, ii = _fetch(ix, total)
            assert rc2 == 0 and RC.same((want[0], dd[:total], ii[:total]), want)      # the former result is still there

        refused(raw(None, ptr(lims), ptr(Q), None, ptr(rad), nq, d, 0, 0, 0))
        refused(raw(ix._h, None, ptr(Q), None, ptr(rad), nq, d, 0, 0, 0))
        refused(raw(ix._h, ptr(lims), None, None, ptr(rad), nq, d, 0, 0, 0))
        refused(raw(ix._h, ptr(lims), ptr(Q), None, None, nq, d, 0, 0, 0))
        refused(raw(bx._h, ptr(lims), ptr(Q), None, ptr(rad), nq, d, 0, 0, 0))                 # an index without codes
        refused(raw(ix._h, ptr(lims), ptr(Q), None, ptr(rad), -1, d, 0, 0, 0))
        refused(raw(ix._h, ptr(lims), ptr(Q), None, ptr(rad), nq, d - 1, 0, 0, 0))
        refused(raw(ix._h, ptr(lims), ptr(Q), None, ptr(rad), nq, d, -1, 0, 0))
        refused(raw(ix._h, ptr(lims), ptr(Q), None, ptr(rad), nq, d, 1, 0, 0))                 # nprobe >= 1 before set_lists
        refused(raw(ix._h, ptr(lims), ptr(Q), None, ptr(rad), nq, d, 0, ic.ADD_COARSE, 0))     # the coarse term without lists probed
        refused(raw(ix._h, ptr(lims), ptr(Q), None, ptr(rad), nq, d, 0, 2, 0))                 # LSQ_IVF_EVERY_RECORD is not a range flag
        ix.set_lists(P["cent"], P["lor"])                                    # (drops the held result: made again)
        assert RC.same(_range(ix, Q, rad), want)
        refused(raw(ix._h, ptr(lims), ptr(Q), None, ptr(rad), nq, d, 17, 0, 0))                # nprobe > nlist
        refused(raw(ix._h, ptr(lims), ptr(Q), None, ptr(rad), nq, d, 4, 4, 0))                 # LSQ_IVF_TEST_BATCH
        refused(raw(ix._h, ptr(lims), ptr(Q), None, ptr(rad), nq, d, 4, ic.ADD_COARSE | 2, 0))
        # a padded query pitch is legal: ldq > d
        wide = np.zeros((nq, d + 3), np.float32)
        wide[:, :d] = Q
        assert raw(ix._h, ptr(lims), ptr(wide), None, ptr(rad), nq, d + 3, 0, 0, 0) == 0 and np.array_equal(lims, want[0])
        assert raw(ix._h, ptr(lims), ptr(wide), ptr(wide), ptr(rad), nq, d + 3, 16, 0, 0) == 0 and np.array_equal(lims, want[0])
        info = lsq._lib.RangeInfo()
        assert engine._L.lsq_index_get_range_info(ix._h, None) == EINVAL and engine._L.lsq_index_get_range_info(ix._h, C.byref(info)) == 0
        assert info.results == total
