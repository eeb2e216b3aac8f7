"""Labelled search (csrc/lsq_label.hip): Index.search / search_ivf with where=(mask, want), a row predicate per query.  The contract is Identity L: every
query's row equals, bit for bit, the host checker's full ranking of the candidate rows with the rows that fail the query's predicate or the index's filter
removed, cut to k and padded with (+inf, 0) -- filter_check.filtered applied per query -- which is what set_filter(those rows) and a one-query call return."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_check as fc  # noqa: E402
import ivf_check as ic  # noqa: E402
import packed_check as pk  # noqa: E402

pytestmark = pytest.mark.gpu

N, D, NQ, NLIST = 20011, 16, 9, 40                  # 79 steps of 256 rows, the last of 43; two groups of four queries and a group of one
LAST = np.arange(N) >= (N - 1) // 256 * 256          # the rows of the last step of the last range
CAT, TENANT, FLAG = 0xFF, 0xFFFF00, 1 << 24
# (mask, want) per query, mixed in one call: every row; no row (every label has a category bit); exactly one row; one tenant (~1/100); one category (~1/8);
# the rows of the last step alone; a tenant and a category together; every row again; another category
WHERE = np.array([(0, 0), (CAT, 0), (TENANT, TENANT), (TENANT, 17 << 8), (CAT, 1 << 3), (FLAG, FLAG), (TENANT | CAT, (5 << 8) | 4), (0, 0), (CAT, 1 << 7)],
                 dtype=np.uint32)
ANY = np.array([0b10101, 0, 0b111, 0b11100000, FLAG, 0b1001001, CAT, 0b1010, TENANT], dtype=np.uint32)      # three categories mostly; a zero mask admits no row


@functools.lru_cache(maxsize=None)
def _problem(lsq, m, packed=False, order=None):
    """the base with 40 skewed lists over it, its labels (a category bit, a 16-bit tenant, a flag on the last step's rows), the full ranking of every query"""
    codes, K, dbn, cent, lor, Qs, Qc = ic.problem(N, D, m, NLIST, NQ, 700 + m, small_int=(order == "tie-cut"))
    if order == "falling":                              # norms that dominate the tables and fall with the row id: every candidate beats the bound
        dbn = (np.arange(N, 0, -1) * 1000).astype(np.float32)
    cb = nc = None
    if packed:
        cb, nc = pk.quantize(dbn)
        dbn = cb[nc]
    rng = np.random.default_rng(3)
    labels = (1 << rng.integers(0, 8, N)).astype(np.uint32) | (rng.integers(0, 100, N).astype(np.uint32) << 8) | np.where(LAST, FLAG, 0).astype(np.uint32)
    labels[N // 3] |= TENANT
    p = (codes, K, dbn, cent, lor, Qs, Qc)
    return p, labels, (nc, cb), fc.full_scan(lsq._lib.load(), codes, K, dbn, Qs)


def _allowed(labels, any_of):
    """(NQ, N) bool: the rows each query's predicate admits"""
    if any_of:
        return (labels[None, :] & ANY[:, None]) != 0
    return (labels[None, :] & WHERE[:, 0, None]) == WHERE[:, 1, None]


def _want(full, ok, nn):
    """filter_check.filtered per query: ok (NQ, N) bool"""
    rows = [fc.filtered(full[0][q:q + 1], full[1][q:q + 1], ok[q], nn, 0) for q in range(ok.shape[0])]
    return np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])


def _index(engine, p, m, packed=None, dev=False, base=None):
    codes, K, dbn = p[:3]
    if not dev:
        ix = engine.index_packed(codes, K, packed[0], packed[1], m, base=base) if packed else engine.index(codes, K, dbn, m, base=base)
    else:
        import torch
        t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in ((codes, K) + tuple(packed) if packed else (codes, K, dbn))]
        ix = engine.index_packed_dev(*t, m) if packed else engine.index_dev(*t, m)
    return ix


def _np(ix, a):
    if not ix._dev or not isinstance(a, np.ndarray):
        return a
    import torch
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _call(ix, what, Qs, k, *args, any_of=False, where=True, **kw):
    """Index.search / search_ivf with numpy arguments on either kind of index -> numpy (dists, ids)"""
    if where is True:
        where = (ANY, np.zeros(NQ, np.uint32)) if any_of else (WHERE[:, 0].copy(), WHERE[:, 1].copy())
    if where is not None:
        kw.update(where=tuple(_np(ix, a) for a in where), any_of=any_of)
    dd, di = getattr(ix, what)(_np(ix, Qs), k, *args, **{a: _np(ix, v) for a, v in kw.items()})
    return (dd.cpu().numpy(), di.cpu().numpy()) if ix._dev else (dd, di)


@pytest.mark.parametrize("nn", [1, 100, 256, 257, 2048])
@pytest.mark.parametrize("m,packed", [(4, 0), (5, 0), (8, 0), (16, 0), (7, 1), (8, 1)], ids=["m4", "m5-bytes", "m8", "m16", "packed-m7", "packed-m8-bytes"])
def test_exhaustive(lsq, engine, m, packed, nn):
    """every loader and every queries-per-block geometry (4, 2, 1) against the checker, both rules; the account of the call"""
    p, labels, pck, full = _problem(lsq, m, bool(packed))
    geo = lsq._lib.LabelGeometryInfo()
    assert lsq._lib.load().lsq_label_geometry(N, m, packed, nn, NQ, 0, geo) == 0
    for dev in ([False, True] if nn == 100 else [False]):
        with _index(engine, p, m, pck if packed else None, dev) as ix:
            ix.set_labels(_np(ix, labels))
            for any_of in (False, True):
                ok = _allowed(labels, any_of)
                assert fc.same(_call(ix, "search", p[5], nn, any_of=any_of), _want(full, ok, nn)), (m, packed, nn, any_of, dev)
                info = ix.label_info()
                assert (info["labels_set"], info["rows"], info["queries"], info["allowed_pairs"]) == (1, N, NQ, int(ok.sum()))
                assert info["queries_per_block"] == geo.queries_per_block and info["blocks_per_query"] == geo.blocks_per_query > 1
                assert info["merged_runs"] == NQ * geo.blocks_per_query
                _call(ix, "search", p[5], nn, any_of=any_of)
                assert ix.label_info() == info          # sums of integers: the same on every call


@pytest.mark.parametrize("order", ["falling", "tie-cut"])
@pytest.mark.parametrize("m,packed,nn", [(8, 0, 100), (7, 1, 100), (16, 0, 257), (8, 0, 2048)])
def test_one_split(lsq, engine, order, m, packed, nn):
    """one block per query group: a single pool sees every row and compacts again and again -- falling norms: every candidate enters the pool, which takes at
    most P - nn <= 412 new records between compactions at nn = 100; small integers: nn cuts a group of equal distances"""
    p, labels, pck, full = _problem(lsq, m, bool(packed), order)
    ok = _allowed(labels, False)
    want = _want(full, ok, nn + 1)
    if order == "tie-cut":
        assert np.any(want[0][:, nn - 1] == want[0][:, nn])
    with _index(engine, p, m, pck if packed else None) as ix:
        ix.set_labels(labels)
        got = _call(ix, "search", p[5], nn, flags=lsq._lib.LABEL_TEST_ONE_SPLIT)
        assert fc.same(got, (want[0][:, :nn], want[1][:, :nn]))
        info = ix.label_info()
        assert info["blocks_per_query"] == 1 and info["merged_runs"] == 0
        if order == "falling" and not packed:            # (a packed norm has 256 levels: rows of one level need not beat the bound)
            assert info["offered"] == info["allowed_pairs"] and (nn != 100 or info["compactions"] >= 2 * (N // 412))      # two queries admit every row


@pytest.mark.parametrize("filt", ["dense", "compact", "removed"])
@pytest.mark.parametrize("m,packed", [(8, 0), (7, 1)], ids=["m8", "packed-m7"])
def test_filter_in_force(lsq, engine, m, packed, filt):
    """a row must pass the index's filter as well; and the device's own set_filter(predicate AND filter) + one-query search gives the same bits"""
    p, labels, pck, full = _problem(lsq, m, bool(packed))
    keep = np.random.default_rng(11).random(N) < 0.5
    ok = _allowed(labels, False) & keep[None, :]
    with _index(engine, p, m, pck if packed else None, dev=(filt == "compact")) as ix:
        ix.set_labels(_np(ix, labels))
        if filt == "removed":
            ix.remove(np.flatnonzero(~keep).astype(np.int32))
        else:
            fc.set_filter(ix, road=filt, mask=keep.copy())
        got = _call(ix, "search", p[5], 100)
        assert fc.same(got, _want(full, ok, 100)) and ix.label_info()["allowed_pairs"] == int(ok.sum())
        for q in (3, 4, 5) if filt != "removed" else ():
            fc.set_filter(ix, road=filt, mask=ok[q].copy())
            one = _call(ix, "search", p[5][q:q + 1], 100, where=None)
            assert fc.same(one, (got[0][q:q + 1], got[1][q:q + 1])), (filt, q)


@pytest.mark.parametrize("add", [0, 1], ids=["plain", "add-coarse"])
@pytest.mark.parametrize("nprobe", [1, 7, 40])
def test_lists(lsq, engine, nprobe, add):
    """40 skewed lists (empty ones, one-row ones, one of half the base): the checker's ranking of the probed rows, filtered per query; nprobe = nlist is the
    labelled exhaustive search; three queries through the device's own set_filter + one-query search_ivf"""
    p, labels, _, _ = _problem(lsq, 8)
    full = fc.full_ivf(lsq._lib.load(), p, nprobe, flags=ic.ADD_COARSE if add else 0)
    probed = np.zeros((NQ, N), dtype=bool)              # the rows of each query's probed lists: the ids of its full ranking
    for q in range(NQ):
        probed[q, full[1][q][full[1][q] > 0] - 1] = True
    for dev in (False, True):
        with _index(engine, p, 8, dev=dev) as ix:
            ix.set_lists(_np(ix, p[3]), _np(ix, p[4]))
            ix.set_labels(_np(ix, labels))
            for any_of in (False, True):
                ok = _allowed(labels, any_of)
                got = _call(ix, "search_ivf", p[5], 100, nprobe, any_of=any_of, Q_coarse=p[6], add_coarse=bool(add))
                assert fc.same(got, _want(full, ok, 100)), (nprobe, add, dev, any_of)
                assert ix.label_info()["allowed_pairs"] == int((ok & probed).sum())
                if nprobe == NLIST and not add:
                    assert fc.same(got, _call(ix, "search", p[5], 100, any_of=any_of))
            for q in (0, 3, 6):
                fc.set_filter(ix, mask=ok[q].copy())
                one = _call(ix, "search_ivf", p[5][q:q + 1], 100, nprobe, where=None, Q_coarse=p[6][q:q + 1], add_coarse=bool(add))
                assert fc.same(one, (got[0][q:q + 1], got[1][q:q + 1])), (nprobe, q)
                ix.clear_filter()


@pytest.mark.parametrize("filt", ["set_filter", "removed"])
@pytest.mark.parametrize("m,packed", [(7, 1), (8, 1), (5, 0), (16, 0)], ids=["packed-m7", "packed-m8-bytes", "m5-bytes", "m16"])
def test_lists_filter_in_force(lsq, engine, m, packed, filt):
    """the list road under a filter in force (its bits in layout order: a row must pass both), on packed rows and on both loaders, in one batch and -- the
    test hook of search_ivf, honoured -- in batches of 8 queries, and with one block per query"""
    p, labels, pck, _ = _problem(lsq, m, bool(packed))
    keep = np.random.default_rng(13).random(N) < 0.5
    ok = _allowed(labels, False) & keep[None, :]
    with _index(engine, p, m, pck if packed else None, dev=(filt == "removed" and not packed)) as ix:
        ix.set_lists(_np(ix, p[3]), _np(ix, p[4]))
        ix.set_labels(_np(ix, labels))
        if filt == "removed":
            ix.remove(_np(ix, np.flatnonzero(~keep).astype(np.int32)))
        else:
            fc.set_filter(ix, mask=keep.copy())
        for nprobe, add in ((7, 1), (40, 0)):
            full = fc.full_ivf(lsq._lib.load(), p, nprobe, flags=ic.ADD_COARSE if add else 0)
            want = _want(full, ok, 100)
            for kw in ({}, dict(flags=ic.TEST_BATCH), dict(label_flags=lsq._lib.LABEL_TEST_ONE_SPLIT)):
                assert fc.same(_call(ix, "search_ivf", p[5], 100, nprobe, Q_coarse=p[6], add_coarse=bool(add), **kw), want), (nprobe, kw)
                assert ix.label_info()["batches"] == (2 if "flags" in kw else 1)
            if not add:
                assert fc.same(_call(ix, "search", p[5], 100), want)


@pytest.mark.parametrize("u8", [0, 1], ids=["f32-base", "u8-base"])
def test_stage_two(lsq, engine, u8):
    """shortlist 300 -> 10: the labelled scan fills the shortlists, the exact re-rank follows, on both roads"""
    p, labels, _, full = _problem(lsq, 8)
    rng = np.random.default_rng(12)
    base = rng.integers(0, 256, (N, D)).astype(np.uint8) if u8 else rng.standard_normal((N, D)).astype(np.float32)
    L, ok = lsq._lib.load(), _allowed(labels, False)
    with _index(engine, p, 8, base=base) as ix:
        ix.set_labels(labels)
        ix.set_lists(p[3], p[4])
        want = fc.two_stage(L, _want(full, ok, 300)[1], base, p[5], 10)
        assert fc.same(_call(ix, "search", p[5], 10, shortlist=300, Q_exact=p[5]), want)
        want = fc.two_stage(L, _want(fc.full_ivf(L, p, 7), ok, 300)[1], base, p[5], 10)
        assert fc.same(_call(ix, "search_ivf", p[5], 10, 7, shortlist=300, Q_exact=p[5], Q_coarse=p[6]), want)


def test_plain_calls_and_refusals(lsq, engine):
    """where=None and an all-rows predicate are the plain calls bit for bit; what is refused is refused with LSQ_EINVAL before an output is written"""
    p, labels, _, _ = _problem(lsq, 8)
    L, zeros = lsq._lib.load(), np.zeros(NQ, np.uint32)
    with _index(engine, p, 8) as ix:
        ix.set_lists(p[3], p[4])
        dd, di = np.full((NQ, 2049), -7, np.float32), np.full((NQ, 2049), -7, np.int32)

        def raw(nn=10, ivf_flags=None):
            a = (ix._h, dd.ctypes.data, di.ctypes.data, p[5].ctypes.data)
            if ivf_flags is None:
                return L.lsq_index_search_labelled(*a, None, zeros.ctypes.data, zeros.ctypes.data, NQ, D, 0, nn, 0, 0)
            return L.lsq_index_search_ivf_labelled(*a, None, None, zeros.ctypes.data, zeros.ctypes.data, NQ, D, 7, 0, nn, ivf_flags, 0, 0)

        assert raw() == lsq._lib.LSQ_EINVAL and raw(ivf_flags=0) == lsq._lib.LSQ_EINVAL                       # no labels set
        assert L.lsq_index_set_labels(ix._h, labels.ctypes.data, N - 1, 0) == lsq._lib.LSQ_EINVAL and raw() == lsq._lib.LSQ_EINVAL
        ix.set_labels(labels)
        assert raw(2049) == lsq._lib.LSQ_EINVAL and raw(2049, 0) == lsq._lib.LSQ_EINVAL and raw(10, ic.EVERY_RECORD) == lsq._lib.LSQ_EINVAL
        assert np.all(dd == -7) and np.all(di == -7)
        assert raw() == 0 and raw(ivf_flags=0) == 0 and np.all(di.ravel()[:NQ * 10] > 0)
        for what, args, kw in (("search", (), {}), ("search_ivf", (7,), dict(Q_coarse=p[6]))):
            plain = _call(ix, what, p[5], 100, *args, where=None, **kw)
            assert fc.same(_call(ix, what, p[5], 100, *args, where=(zeros, zeros), **kw), plain)
            assert fc.same(getattr(ix, what)(p[5], 100, *args, **kw), plain)


def test_lifetime(lsq, engine):
    """remove and set_lists keep the labels (the layout-order copy follows the new lists), a second set_labels replaces the first, add and compact drop them"""
    p, labels, _, full = _problem(lsq, 8)
    L, ok = lsq._lib.load(), _allowed(labels, False)
    with _index(engine, p, 8) as ix:
        ix.set_lists(p[3], p[4])
        ix.set_labels(np.zeros(N, np.uint32))
        ix.set_labels(labels)
        assert fc.same(_call(ix, "search_ivf", p[5], 100, 7, Q_coarse=p[6]), _want(fc.full_ivf(L, p, 7), ok, 100))
        lor2 = ((np.arange(N) * 7) % NLIST).astype(np.int32)
        ix.set_lists(p[3], lor2)
        p2 = p[:4] + (lor2,) + p[5:]
        assert fc.same(_call(ix, "search_ivf", p[5], 100, 7, Q_coarse=p[6]), _want(fc.full_ivf(L, p2, 7), ok, 100)) and ix.label_info()["layout_builds"] == 1
        gone = np.arange(0, N, 3, dtype=np.int32)
        ix.remove(gone)
        keep = np.ones(N, dtype=bool)
        keep[gone] = False
        assert fc.same(_call(ix, "search", p[5], 100), _want(full, ok & keep[None, :], 100))
        ix.compact()
        assert ix.label_info()["labels_set"] == 0
        with pytest.raises(lsq._lib.LsqError) as e:
            _call(ix, "search", p[5], 100)
        assert e.value.code == lsq._lib.LSQ_EINVAL
        n2 = int(keep.sum())
        ix.set_labels(labels[keep])
        assert ix.label_info()["rows"] == n2
        ix.add(codes=p[0][:5], dbnorms=p[2][:5], assign=lor2[:5])
        assert ix.label_info()["labels_set"] == 0
        ix.set_labels(np.concatenate([labels[keep], labels[:5]]))
        ix.clear_labels()
        assert ix.label_info()["labels_set"] == 0
