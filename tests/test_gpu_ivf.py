"""The inverted-list search on the device (lsq_index_set_lists, lsq_index_search_ivf) against the host checker lsq_ivf_search_cpu bit for bit: both roads,
host and device forms, the padding, ties and NaN, batches, the two identities of the contract, stage two behind it, and the state of a shared context.
The named problems of tests/ivf_check.py reach the routes a shape selects -- a block that walks several lists, every loader width, a tail filled to the
record and eight over, some queries redone over several fall-back batches, a NaN tau, infinities beside the padding, the layout's edges -- and hold
lsq_ivf_info's road counts to what the numpy checker predicts (tail_hits_np, roads_np)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivf_check as ic  # noqa: E402
from knn_check import same_bits  # noqa: E402
from rerank_check import rerank_cpu  # noqa: E402

pytestmark = pytest.mark.gpu
H = 256


def _indexes(engine, p, base=None):
    """a host-buffer index and a borrowed-device one over the same problem, lists set on both"""
    import torch
    codes, K, dbn, cent, lor = p[:5]
    m = codes.shape[1]
    hix = engine.index(codes, K, dbn, m, base=base)
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (codes, K, dbn)]
    dix = engine.index_dev(t[0], t[1], t[2], m, base=None if base is None else torch.from_numpy(base).cuda())
    hix.set_lists(cent, lor)
    dix.set_lists(torch.from_numpy(cent).cuda(), torch.from_numpy(lor).cuda())
    return hix, dix


def _search(ix, Qs, Qc, k, nprobe, **kw):
    if ix._dev:
        import torch
        kw = {a: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for a, v in kw.items()}
        dd, di = ix.search_ivf(torch.from_numpy(Qs).cuda(), k, nprobe, Q_coarse=torch.from_numpy(Qc).cuda(), **kw)
        return dd.cpu().numpy(), di.cpu().numpy()
    return ix.search_ivf(Qs, k, nprobe, Q_coarse=Qc, **kw)


def _both_roads(lsq, ixs, p, nprobe, nn, what, flags=0, roads=None):
    """default and forced every-record road, with and without the coarse add, on every index: all equal to the checker.  roads: _roads' prediction, which
    the default road's counts are then held to"""
    L = lsq._lib.load()
    Qs, Qc = p[5], p[6]
    for add in (False, True):
        rc, rd, ri = ic.ivf_cpu(L, *p, nprobe, nn, flags=ic.ADD_COARSE if add else 0)
        assert rc == 0
        for ix in ixs:
            for every in (False, True):
                dd, di = _search(ix, Qs, Qc, nn, nprobe, add_coarse=add, every_record=every, flags=flags)
                assert same_bits(dd, rd) and np.array_equal(di, ri), (what, add, every, ix._dev)
                info = ix.ivf_info()
                assert info["queries"] == Qs.shape[0] and info["threshold_queries"] + info["fallback_queries"] in (0, Qs.shape[0])
                if every:
                    assert info["threshold_queries"] == 0 and info["fallback_queries"] == 0 and info["tail_capacity"] == 0
                elif roads is not None:
                    cap, fallback, records = roads[add][1]
                    assert (info["tail_capacity"], info["fallback_queries"], info["threshold_queries"], info["records"]) == \
                        (cap, len(fallback), Qs.shape[0] - len(fallback), records), (what, add, ix._dev)


def _roads(p, nprobe, nn):
    """per coarse-add flag: (tail_hits_np's counts, roads_np's prediction from them) -- which road every query takes, worked out from the checker alone"""
    out = {}
    for add in (False, True):
        hits = ic.tail_hits_np(*p, nprobe, nn, add_coarse=add)
        assert max(h[1] for h in hits) > 0                                   # some query has a tail: the call is thresholded
        out[add] = (hits, ic.roads_np(hits, nn))
    return out


def _run_named(lsq, engine, name, flags=0):
    """a named problem of ivf_check through _both_roads, its road counts held to the checker's -> (arrays, nprobe, nn, roads, host index's plain result)"""
    p, nprobe, nn = ic.PROBLEMS[name]()
    roads = _roads(p, nprobe, nn)
    hix, dix = _indexes(engine, p)
    with hix, dix:
        _both_roads(lsq, (hix, dix), p, nprobe, nn, name, flags=flags, roads=roads)
        got = hix.search_ivf(p[5], nn, nprobe, Q_coarse=p[6], flags=flags)
        batches = hix.ivf_info()["batches"]
    return p, nprobe, nn, roads, got, batches


@pytest.mark.parametrize("shape", ic.SHAPES, ids=lambda s: "d%d-m%d-nlist%d-nprobe%d-nn%d-nq%d" % s)
def test_device_equals_the_host_checker(lsq, engine, shape):
    """skewed lists (empty ones, one-row ones, one of half the rows), NaN norms, probed rows < nn where nprobe is small"""
    d, m, nlist, nprobe, nn, nq = shape
    p = ic.problem(ic.N, d, m, nlist, nq, 7 + sum(shape))
    p[2][5::97] = np.float32(np.nan)
    hix, dix = _indexes(engine, p)
    with hix, dix:
        _both_roads(lsq, (hix, dix), p, nprobe, nn, shape)


def test_probed_rows_below_nn_are_padded(lsq, engine):
    codes, K, dbn, cent, lor, Qs, Qc = ic.problem(ic.N, 32, 8, 40, 5, 3)
    lor[:] = 0
    lor[:4] = 3
    dbn[1] = np.float32(np.nan)
    cent[3] = 1000.0
    Qc[:] = 1000.0
    p = (codes, K, dbn, cent, lor, Qs, Qc)
    hix, dix = _indexes(engine, p)
    with hix, dix:
        _both_roads(lsq, (hix, dix), p, 1, 10, "padding")
        dd, di = hix.search_ivf(Qs, 10, 1, Q_coarse=Qc)
        assert np.all(di[:, 4:] == 0) and np.all(np.isposinf(dd[:, 4:])) and np.all(np.isnan(dd[:, 3])) and np.all(di[:, 3] == 2)
        assert hix.ivf_info()["probed_rows"] == 4 * 5


@pytest.mark.parametrize("m", [7, 8])
def test_exact_ties(lsq, engine, m):
    """small-integer codebooks and queries, code rows duplicated across lists, two equidistant centroids"""
    n, nlist = 2400, 7
    codes, K, dbn, cent, lor, Qs, Qc = ic.problem(n, 5, m, nlist, 37, 50 + m, small_int=True, lists="random")
    codes[n // 2:] = codes[:n // 2]
    dbn[n // 2:] = dbn[:n // 2]
    cent[4] = cent[2]
    Qc[::2] = cent[2]
    p = (codes, K, dbn, cent, lor, Qs, Qc)
    hix, dix = _indexes(engine, p)
    with hix, dix:
        for nprobe, nn in ((1, 10), (3, 300), (nlist, 300)):
            _both_roads(lsq, (hix, dix), p, nprobe, nn, ("ties", nprobe, nn))


def test_several_batches(lsq, engine):
    p = ic.problem(ic.N, 32, 8, 40, 37, 77)
    hix, dix = _indexes(engine, p)
    with hix, dix:
        _both_roads(lsq, (hix, dix), p, 3, 10, "batches", flags=ic.TEST_BATCH)
        hix.search_ivf(p[5], 10, 3, Q_coarse=p[6], flags=ic.TEST_BATCH)
        info = hix.ivf_info()
        assert info["batch_queries"] == 8 and info["batches"] >= 5
        hix.search_ivf(p[5], 10, 3, Q_coarse=p[6])
        assert hix.ivf_info()["batches"] == 1 and hix.ivf_info()["batch_queries"] == 37


def test_thresholded_road_answers_random_codes_without_falling_back(lsq, engine):
    """nn = 10, lists of ~50 rows, nprobe = 8: the head is one or two lists; the checker's own count of tail records within tau stays under the capacity"""
    n, nlist, nprobe, nn, nq = 2000, 40, 8, 10, 37
    p = ic.problem(n, 32, 8, nlist, nq, 91, lists="random")
    hits = ic.tail_hits_np(*p, nprobe, nn)
    cap = 8 * nn + 256
    assert all(h[1] > 0 for h in hits) and max(h[2] for h in hits) <= min(cap, max(h[1] for h in hits)) and max(h[2] for h in hits) < max(h[1] for h in hits)
    rc, rd, ri = ic.ivf_cpu(lsq._lib.load(), *p, nprobe, nn)
    hix, dix = _indexes(engine, p)
    with hix, dix:
        for ix in (hix, dix):
            dd, di = _search(ix, p[5], p[6], nn, nprobe)
            info = ix.ivf_info()
            assert same_bits(dd, rd) and np.array_equal(di, ri)
            assert info["threshold_queries"] == nq and info["fallback_queries"] == 0 and info["tail_capacity"] == min(cap, max(h[1] for h in hits))
            assert info["records"] == sum(max(h[0], nn) + h[2] for h in hits) and info["probed_rows"] == sum(h[0] + h[1] for h in hits)
            _search(ix, p[5], p[6], nn, nprobe, every_record=True)
            assert ix.ivf_info()["records"] == sum(h[0] + h[1] for h in hits)


def test_identical_rows_overflow_the_tail_and_fall_back(lsq, engine):
    """every tail record ties tau: 350 of them against 264 slots, every query is redone with every record and is still exact"""
    n, nlist, nprobe, nn, nq = 2000, 40, 8, 1, 37
    codes, K, dbn, cent, lor, Qs, Qc = ic.problem(n, 32, 8, nlist, nq, 92, lists="even")
    codes[:] = codes[0]
    dbn[:] = dbn[0]
    p = (codes, K, dbn, cent, lor, Qs, Qc)
    rc, rd, ri = ic.ivf_cpu(lsq._lib.load(), *p, nprobe, nn)
    hix, dix = _indexes(engine, p)
    with hix, dix:
        for ix in (hix, dix):
            dd, di = _search(ix, Qs, Qc, nn, nprobe)
            info = ix.ivf_info()
            assert same_bits(dd, rd) and np.array_equal(di, ri)
            assert info["fallback_queries"] == nq and info["threshold_queries"] == 0 and info["tail_capacity"] == 264


@pytest.mark.parametrize("name,flags,splits", [("stride-m8", 0, 7), ("stride-m8", ic.TEST_BATCH, 40), ("stride-m12", 0, 16)],
                         ids=["m8-splits7", "m8-test-batch", "m12-splits16"])
def test_a_block_walks_several_lists(lsq, engine, name, flags, splits):
    """more (query, list) pairs than the scan has blocks for: the stride of a block's list loop, the staged table used for a second list, and the
    thresholded tail's first list (the head's length) combined with that stride.  Without the batch flag a query gets `splits` < nprobe blocks"""
    p, nprobe, nn, roads, _, batches = _run_named(lsq, engine, name, flags=flags)
    nq = p[5].shape[0]
    assert nq * nprobe > ic.SCAN_BLOCKS
    assert ic.scan_splits(8 if flags else nq, nprobe) == splits and (flags or 1 < -(-nprobe // splits) <= 6)       # lists per block: up to 6, up to 3
    assert all(h[1] > 0 for h in roads[False][0])                            # every query has a tail
    if name == "stride-m12":                                                 # and here some overflow it and some do not: the redone queries are a subset
        assert 0 < len(roads[False][1][1]) < nq
    if flags:
        assert batches == -(-nq // 8) + -(-len(roads[False][1][1]) // 8)


@pytest.mark.parametrize("t,over", [(33, False), (34, True)], ids=["fills-the-tail", "eight-over"])
def test_tail_filled_to_the_record_and_eight_over(lsq, engine, t, over):
    """a segment fails with count > capacity and the scan writes at < capacity: 264 tail records within tau against 264 slots stay on the thresholded road,
    272 send every query to the every-record road"""
    p, nprobe, nn, roads, _, _ = _run_named(lsq, engine, "capacity-%d" % t)
    nq = p[5].shape[0]
    hits, (cap, fallback, records) = roads[False]
    assert cap == 8 * nn + 256 and all(h == (75, 8 * 75, 8 * t) for h in hits) and (8 * t > cap) == over and 8 * 33 == cap
    assert fallback == (list(range(nq)) if over else []) and (over or records == nq * (75 + cap))


@pytest.mark.parametrize("flags", [0, ic.TEST_BATCH], ids=["one-batch", "test-batch"])
def test_some_queries_fall_back_and_others_do_not(lsq, engine, flags):
    """the even queries overflow their tails (every record ties tau), the odd ones do not: the redone queries are a non-contiguous selection, and with
    batches of 8 they are three batches, the second and third starting 8 and 16 entries into it"""
    p, nprobe, nn, roads, _, batches = _run_named(lsq, engine, "mixed", flags=flags)
    nq = p[5].shape[0]
    hits, (cap, fallback, _) = roads[False]
    assert fallback == list(range(0, nq, 2)) and len(fallback) == 19 and all(hits[q][2] == 7 * 75 for q in fallback)
    assert max(hits[q][2] for q in range(1, nq, 2)) <= cap == 264
    assert batches == (5 + 3 if flags else 1 + 1)                            # thresholded batches + fall-back batches


def test_nan_tau_keeps_every_record_and_infinities_order(lsq, engine):
    """a head without a number: tau is NaN, !(dist > tau) keeps every tail record, the query overflows and is redone; +inf and -inf norms elsewhere"""
    p, nprobe, nn, roads, (dd, di), _ = _run_named(lsq, engine, "nan-tau")
    nq = p[5].shape[0]
    for add in (False, True):
        hits, (cap, fallback, _) = roads[add]
        assert fallback == list(range(0, nq, 2)) and all(hits[q][2] == hits[q][1] == 7 * 75 for q in fallback)     # kept: all of the tail
    assert np.all(np.isnan(dd[0::2])) and np.all(di[0::2] > 0)               # NaN distances with their real ids, the nn smallest ids of the probed rows
    assert np.all(np.isneginf(dd[1::2, 0])) and not np.any(np.isnan(dd[1::2]))


def test_real_infinities_and_nan_come_before_the_padding(lsq, engine):
    p, nprobe, nn = ic.PROBLEMS["short-list"]()
    hix, dix = _indexes(engine, p)
    with hix, dix:
        _both_roads(lsq, (hix, dix), p, nprobe, nn, "short-list")
        for ix in (hix, dix):
            dd, di = _search(ix, p[5], p[6], nn, nprobe)
            assert np.array_equal(di, np.tile([2, 1, 3, 4, 0, 0, 0, 0, 0, 0], (5, 1)))
            assert np.all(np.isneginf(dd[:, 0])) and np.all(np.isfinite(dd[:, 1])) and np.all(np.isposinf(dd[:, 2])) and np.all(np.isnan(dd[:, 3]))
            assert np.all(np.isposinf(dd[:, 4:]))


@pytest.mark.parametrize("n", [2047, 2048])
@pytest.mark.parametrize("nlist", [64, 65])
def test_layout_edges(lsq, engine, n, nlist):
    """lists 0, 1, 2 and the last three empty, nlist at a power of two and one above it, n at a power of two and one below it; the last row, whose id n is
    the largest the record's id field holds, is the nearest row of query 0.  Both forms of set_lists (host arrays, device tensors: _indexes)"""
    p, nprobe, nn, roads, (dd, di), _ = _run_named(lsq, engine, "layout-n%d-nlist%d" % (n, nlist))
    lor = p[4]
    assert p[0].shape[0] == n and p[3].shape[0] == nlist and lor.min() == 3 and lor.max() == nlist - 4
    assert di[0, 0] == n and (n & (n - 1) == 0) == (n == 2048)


def _database(n, d, m, nq, seed):
    rng = np.random.default_rng(seed)
    K = (rng.standard_normal((m * H, d)) / np.sqrt(m)).astype(np.float32)
    codes = rng.integers(0, H, (n, m)).astype(np.uint8)
    recon = sum(K[j * H + codes[:, j].astype(np.int64)] for j in range(m))
    dbn = (recon.astype(np.float64) ** 2).sum(1).astype(np.float32)
    Xb = (recon + 0.35 * rng.standard_normal((n, d))).astype(np.float32)
    Xq = (Xb[rng.integers(0, n, nq)] + 0.2 * rng.standard_normal((nq, d))).astype(np.float32)
    return codes, K, dbn, Xb, Xq


def test_the_two_identities_and_stage_two(lsq, engine):
    L = lsq._lib.load()
    n, d, m, nlist, nq = 2500, 32, 8, 7, 37
    codes, K, dbn, Xb, Xq = _database(n, d, m, nq, 5)
    cent, lor = lsq.train_coarse(Xb, nlist, niter=2, seed=3, engine=engine)
    assert np.array_equal(lor, lsq.ivf_assign(Xb, cent))                     # the device assigns as the host does
    with engine.index(codes, K, dbn, m, base=Xb) as ix:
        cand = np.random.default_rng(1).integers(1, n + 1, (nq, 40)).astype(np.int32)
        before = (ix.search(Xq, 20), ix.search(Xq, 5, shortlist=50), ix.rerank(Xq, cand, 7), ix.knn(Xq, 9))
        with pytest.raises(lsq._lib.LsqError):                               # a search before set_lists
            ix.search_ivf(Xq, 5, 1)
        ix.set_lists(cent, lor)
        after = (ix.search(Xq, 20), ix.search(Xq, 5, shortlist=50), ix.rerank(Xq, cand, 7), ix.knn(Xq, 9))
        for (bd, bi), (ad, ai) in zip(before, after):                        # identity 2: lists change nothing of the other searches
            assert same_bits(bd, ad) and np.array_equal(bi, ai)
        for nn in (1, 300):                                                  # identity 1: every list probed, no flag
            for every in (False, True):
                dd, di = ix.search_ivf(Xq, nn, nlist, every_record=every)
                sd, si = ix.search(Xq, nn)
                assert same_bits(dd, sd) and np.array_equal(di, si)
        # shortlist = L: lsq_rerank_cpu applied to the checker's L-shortlist, padding ids included
        for nprobe, Ls, nn in ((2, 60, 10), (nlist, 300, 300), (1, 2000, 5)):
            rc, _, ci = ic.ivf_cpu(L, codes, K, dbn, cent, lor, Xq, Xq, nprobe, Ls)
            rc2, rd, ri = rerank_cpu(L, Xb, Xq, ci, d, nn, 1)
            assert rc == 0 and rc2 == 0
            for every in (False, True):
                dd, di = ix.search_ivf(Xq, nn, nprobe, shortlist=Ls, every_record=every)
                assert same_bits(dd, rd) and np.array_equal(di, ri), (nprobe, Ls, nn, every)
        assert np.any(ic.ivf_cpu(L, codes, K, dbn, cent, lor, Xq, Xq, 1, 2000)[2] == 0)      # (the last case did have padding ids)


def test_set_lists_twice_gives_the_second_partition(lsq, engine):
    L = lsq._lib.load()
    p = ic.problem(ic.N, 32, 8, 40, 11, 17)
    rng = np.random.default_rng(2)
    cent2, lor2 = rng.standard_normal((7, 32)).astype(np.float32), rng.integers(0, 7, ic.N).astype(np.int32)
    with engine.index(p[0], p[1], p[2], 8) as ix:
        ix.set_lists(p[3], p[4])
        rc, rd, ri = ic.ivf_cpu(L, *p, 3, 10)
        dd, di = ix.search_ivf(p[5], 10, 3, Q_coarse=p[6])
        assert same_bits(dd, rd) and np.array_equal(di, ri)
        bad = lor2.copy()
        bad[100] = 7
        with pytest.raises(lsq._lib.LsqError) as e:                          # refused on the device: the first lists stay
            ix.set_lists(cent2, bad)
        assert e.value.code == lsq._lib.LSQ_EINVAL and "list_of_row" in str(e.value)
        dd, di = ix.search_ivf(p[5], 10, 3, Q_coarse=p[6])
        assert same_bits(dd, rd) and np.array_equal(di, ri)
        ix.set_lists(cent2, lor2)
        rc, rd, ri = ic.ivf_cpu(L, p[0], p[1], p[2], cent2, lor2, p[5], p[6], 3, 10)
        dd, di = ix.search_ivf(p[5], 10, 3, Q_coarse=p[6])
        assert same_bits(dd, rd) and np.array_equal(di, ri)
        with pytest.raises(lsq._lib.LsqError):
            ix.search_ivf(p[5], 10, 8)                                       # nprobe beyond the NEW nlist


def test_two_indexes_and_encodes_on_one_context(lsq, engine):
    import conftest
    L = lsq._lib.load()
    pa, pb = ic.problem(ic.N, 32, 8, 40, 37, 61), ic.problem(2100, 5, 7, 7, 9, 62)
    X, Ke, B0 = conftest.make_problem(32, 512, 8, seed=4)
    ra, rb = ic.ivf_cpu(L, *pa, 3, 10), ic.ivf_cpu(L, *pb, 3, 300, flags=ic.ADD_COARSE)
    with engine.index(pa[0], pa[1], pa[2], 8) as ia, engine.index(pb[0], pb[1], pb[2], 7) as ib:
        ia.set_lists(pa[3], pa[4])
        ib.set_lists(pb[3], pb[4])
        first = engine.encode_icm(X, B0, Ke, 8, [1], 2, 2, True, seed=9)
        for _ in range(2):
            dd, di = ia.search_ivf(pa[5], 10, 3, Q_coarse=pa[6])
            assert same_bits(dd, ra[1]) and np.array_equal(di, ra[2])
            again = engine.encode_icm(X, B0, Ke, 8, [1], 2, 2, True, seed=9)
            assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
            dd, di = ib.search_ivf(pb[5], 300, 3, Q_coarse=pb[6], add_coarse=True)
            assert same_bits(dd, rb[1]) and np.array_equal(di, rb[2])
            sd, si = engine.linscan(pa[0], pa[5], pa[1], pa[2], 8, 10)
            fd, fi = ia.search_ivf(pa[5], 10, 40)
            assert same_bits(fd, sd) and np.array_equal(fi, si)


def test_every_refusal_launches_nothing(lsq, engine):
    L, EINVAL = lsq._lib.load(), lsq._lib.LSQ_EINVAL
    codes, K, dbn, Xb, Xq = _database(600, 5, 2, 3, 8)
    cent, lor = np.ascontiguousarray(Xb[:7]), (np.arange(600) % 7).astype(np.int32)
    dd, di = np.zeros((3, 4), np.float32), np.zeros((3, 4), np.int32)
    desc = lsq._lib.IvfDesc()
    desc.nlist, desc.centroids, desc.list_of_row, desc.on_device = 7, cent.ctypes.data, lor.ctypes.data, 0

    def search(h, q_scan=Xq.ctypes.data, q_exact=None, nprobe=2, shortlist=0, nn=4, flags=0, dists=dd.ctypes.data, ids=di.ctypes.data, ldq=5):
        return L.lsq_index_search_ivf(h, dists, ids, q_scan, None, q_exact, 3, ldq, nprobe, shortlist, nn, flags, 0)

    with engine.index(None, None, None, 0, base=Xb) as bix:                   # an index without codes
        assert L.lsq_index_set_lists(bix._h, C.byref(desc)) == EINVAL and search(bix._h) == EINVAL
    with engine.index(codes, K, dbn, 2) as ix, engine.index(codes, K, dbn, 2, base=Xb) as fix:
        assert search(ix._h) == EINVAL and b"set_lists" in L.lsq_last_error()                   # before set_lists
        assert L.lsq_index_set_lists(ix._h, None) == EINVAL
        for nlist in (0, (1 << 24) + 1):
            desc.nlist = nlist
            assert L.lsq_index_set_lists(ix._h, C.byref(desc)) == EINVAL
        desc.nlist = 7
        for field in ("centroids", "list_of_row"):
            keep = getattr(desc, field)
            setattr(desc, field, None)
            assert L.lsq_index_set_lists(ix._h, C.byref(desc)) == EINVAL
            setattr(desc, field, keep)
        for entry in (-1, 7):
            lor[5] = entry
            assert L.lsq_index_set_lists(ix._h, C.byref(desc)) == EINVAL and search(ix._h) == EINVAL      # still no lists
        lor[5] = 5
        assert L.lsq_index_set_lists(ix._h, C.byref(desc)) == 0 and L.lsq_index_set_lists(fix._h, C.byref(desc)) == 0
        assert search(ix._h) == 0
        for kw in (dict(nprobe=0), dict(nprobe=8), dict(nn=0), dict(shortlist=3), dict(shortlist=-1), dict(flags=8), dict(flags=-1), dict(q_scan=None),
                   dict(dists=None), dict(ids=None), dict(ldq=4), dict(shortlist=10, q_exact=Xq.ctypes.data)):      # (the last: no base rows)
            assert search(ix._h, **kw) == EINVAL, kw
        assert search(fix._h, shortlist=10) == EINVAL                         # a shortlist without q_exact
        assert search(fix._h, shortlist=10, q_exact=Xq.ctypes.data) == 0
        assert L.lsq_index_get_ivf_info(ix._h, None) == EINVAL
