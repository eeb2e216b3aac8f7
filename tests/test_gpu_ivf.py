"""The inverted-list search on the device (lsq_index_set_lists, lsq_index_search_ivf) against the host checker lsq_ivf_search_cpu bit for bit: both roads,
host and device forms, the padding, ties and NaN, batches, the two identities of the contract, stage two behind it, and the state of a shared context.
The named problems of tests/ivf_check.py reach the routes a shape selects -- a block that walks several lists, every loader width, a tail filled to the
record and eight over, some queries redone over several fall-back batches, a NaN tau, infinities beside the padding, the layout's edges -- and hold
lsq_ivf_info's road counts to what the numpy checker predicts (tail_hits_np, roads_np).  The last section runs 256 .. 2^24 lists: the list-bit edges of the
grouping sort, the coarse search on its sampled road and under the context's two search options, nlist >> n."""
import ctypes as C
import os
import sys
import time

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


# ---- many lists: nlist from 2^16 to the contract's 2^24 (the problems of ivf_check, which tests/test_ivf.py holds to the numpy statement) ----------------
def _set_lists(ix, cent, lor):
    if ix._dev:
        import torch
        cent, lor = torch.from_numpy(cent).cuda(), torch.from_numpy(lor).cuda()
    ix.set_lists(cent, lor)


def _many(lsq, ixs, p, nprobe, nn, what, roads=None):
    """_both_roads behind the padding condition: the checker's own result holds rows, so that no case passes by comparing infinities"""
    for add in (0, ic.ADD_COARSE):
        rc, _, ri = ic.ivf_cpu(lsq._lib.load(), *p, nprobe, nn, flags=add)
        assert rc == 0 and ic.padding_ok(ri), (what, add)
    _both_roads(lsq, ixs, p, nprobe, nn, what, roads=roads)


def _coarse_search(engine, cent, Qc, nprobe):
    """the coarse step on its own -- engine.knn_exact_dev(centroids, Q_coarse, nprobe) -- -> its scan statistics, fallback_queries this call's alone"""
    import torch
    before = engine.linscan_stats()["fallback_queries"]
    engine.knn_exact_dev(torch.from_numpy(cent).cuda(), torch.from_numpy(Qc).cuda(), nprobe)
    st = engine.linscan_stats()
    st["fallback_queries"] -= before
    return st


@pytest.mark.parametrize("nlist", [256, 257, 65536, 65537])
def test_list_bit_edges_of_the_grouping_sort(lsq, engine, nlist):
    """reaches: lsq_rows_sort on 40, 41, 48 and 49 key bits (8, 9, 16, 17 list bits); from 65 536 on one thread of ivf_offsets_kernel opens runs of
    thousands of empty lists; at 65 537 the coarse step of search_ivf leaves the exhaustive road.  Evidence: ivf_info against roads_np, the direct
    search's `exhaustive`"""
    p, nprobe, nn = ic.list_edge_problem(nlist)
    counts = np.bincount(p[4], minlength=nlist)
    assert not counts[:3].any() and not counts[-3:].any() and (nlist < 65536 or (counts == 0).sum() > 64000)
    hix, dix = _indexes(engine, p)
    with hix, dix:
        assert hix.nlist == dix.nlist == nlist
        _many(lsq, (hix, dix), p, nprobe, nn, nlist, roads=_roads(p, nprobe, nn))
        assert _coarse_search(engine, p[3], p[6], nprobe)["exhaustive"] == (1 if nlist <= 65536 else 0)
        if nlist == 65537:                                                   # set_lists again with another partition: the second one wins
            cent2 = np.ascontiguousarray(p[3][np.random.default_rng(3).permutation(nlist)])
            lor2 = ic.near_lists(cent2, p[6], p[0].shape[0], nprobe, seed=1)
            assert not np.array_equal(lor2, p[4])
            p2 = p[:3] + (cent2, lor2) + p[5:]
            for ix in (hix, dix):
                _set_lists(ix, cent2, lor2)
            _many(lsq, (hix, dix), p2, nprobe, nn, "second partition", roads=_roads(p2, nprobe, nn))


def test_many_lists_under_every_coarse_road(lsq, engine):
    """reaches: the sampled coarse search (65 537 centroids, rank 45, lists of 640) as the coarse step of search_ivf, and c->search's two options handed to
    it.  Evidence: ivf_info against roads_np (276, no fall-back, 7809 records); the direct exact search on the same arrays under the same options"""
    p, nprobe, nn = ic.many_lists_problem()
    nq = p[5].shape[0]
    roads = _roads(p, nprobe, nn)
    assert roads[False][1] == (276, [], 7809)
    want = {add: ic.ivf_cpu(lsq._lib.load(), *p, nprobe, nn, flags=ic.ADD_COARSE if add else 0) for add in (False, True)}
    model = ic.coarse_stats(p[3], p[6], nprobe)
    hix, dix = _indexes(engine, p)
    with hix, dix:
        for ix in (hix, dix):                                                # (set again: the same lists, for the printed times)
            t0 = time.perf_counter()
            _set_lists(ix, p[3], p[4])
            t1 = time.perf_counter()
            _search(ix, p[5], p[6], nn, nprobe)
            print("nlist = 65537, n = 262148, %s form: set_lists (copies included) %.4f s, search_ivf of %d queries with nprobe = %d %.4f s"
                  % ("device" if ix._dev else "host", t1 - t0, nq, nprobe, time.perf_counter() - t1))
        _many(lsq, (hix, dix), p, nprobe, nn, "many-lists", roads=roads)
        try:
            for option in (None, "linscan_exhaustive", "linscan_rank"):
                if option:
                    engine.set_option(option, 1)
                for ix in (hix, dix):
                    for add in (False, True):
                        dd, di = _search(ix, p[5], p[6], nn, nprobe, add_coarse=add)
                        assert same_bits(dd, want[add][1]) and np.array_equal(di, want[add][2]), (option, ix._dev, add)
                st = _coarse_search(engine, p[3], p[6], nprobe)
                print("coarse search of %d queries on 65537 centroids for %d, option %s: %s" % (nq, nprobe, option, {k: st[k] for k in
                      ("exhaustive", "threshold_rank", "list_capacity", "fallback_queries", "candidates")}))
                if option is None:                                           # the model's plan (select_model.plan(65537, 64)) and its count of redone queries
                    assert (st["exhaustive"], st["threshold_rank"], st["list_capacity"]) == (0, 45, 640)
                    assert st["fallback_queries"] == model["fallback_queries"] < nq
                elif option == "linscan_exhaustive":
                    assert st["exhaustive"] == 1 and st["fallback_queries"] == 0
                else:
                    assert st["exhaustive"] == 0 and st["threshold_rank"] == 1 and st["fallback_queries"] == nq
                if option:
                    engine.set_option(option, 0)
        finally:
            engine.set_option("linscan_rank", 0)
            engine.set_option("linscan_exhaustive", 0)


@pytest.mark.parametrize("m", [7, 8], ids=["m7-dword-rows", "m8-byte-rows"])
def test_many_lists_on_a_packed_index(lsq, engine, m):
    """reaches: the packed scan (8-byte rows on the dword loader, 9-byte rows on the byte loader) behind the sampled coarse search, lists of about four
    rows.  Evidence: packed_info's row geometry, ivf_info's thresholded queries"""
    import packed_check as pk
    codes, K, dbn, cent, lor, Qs, Qc = ic.problem(262148, 8, m, ic.MANY, 37, seed=5, lists="random")
    cb, nc = pk.quantize(dbn)
    p, nprobe, nn = (codes, K, cb[nc], cent, lor, Qs, Qc), 64, 10
    with engine.index_packed(codes, K, nc, cb, m) as packed:
        packed.set_lists(cent, lor)
        info = packed.packed_info()
        assert (info["row_bytes"], info["ivf_row_bytes"], info["dword_rows"]) == (m + 1, m + 5, 1 if m == 7 else 0) and packed.nlist == ic.MANY
        _many(lsq, (packed,), p, nprobe, nn, ("packed", m))
        packed.search_ivf(Qs, nn, nprobe, Q_coarse=Qc)
        info = packed.ivf_info()
        assert info["threshold_queries"] + info["fallback_queries"] == 37 and info["tail_capacity"] > 0


def test_many_probes(lsq, engine):
    """reaches: nprobe = 1024 of 65 537 lists -- the coarse search's plan r = 352, cap = 3200, ivf_plan_kernel's prefix of 1025 positions with long runs
    of equal ones (most probed lists are empty), 2048 / 5 scan blocks per query.  Evidence: ivf_info against roads_np, the direct search's plan"""
    p, nprobe, nn = ic.many_probes_problem()
    roads = _roads(p, nprobe, nn)
    hix, dix = _indexes(engine, p)
    with hix, dix:
        _many(lsq, (hix, dix), p, nprobe, nn, "many-probes", roads=roads)
    st = _coarse_search(engine, p[3], p[6], nprobe)
    assert (st["exhaustive"], st["threshold_rank"], st["list_capacity"]) == (0, 352, 3200)
    assert st["fallback_queries"] == ic.coarse_stats(p[3], p[6], nprobe)["fallback_queries"]


def test_duplicated_centroids_make_a_mixed_coarse_batch(lsq, engine):
    """reaches: a coarse search in which some queries are served by their candidate lists and query 0 -- 40 000 centroids tie at its threshold -- is
    redone, inside search_ivf; the ties go to the smaller list id.  Evidence: the direct search's 1 <= fallback_queries < nq"""
    p, nprobe, nn = ic.duplicated_centroids_problem()
    nq = p[5].shape[0]
    hix, dix = _indexes(engine, p)
    with hix, dix:
        _many(lsq, (hix, dix), p, nprobe, nn, "duplicated-centroids", roads=_roads(p, nprobe, nn))
    st = _coarse_search(engine, p[3], p[6], nprobe)
    assert 1 <= st["fallback_queries"] < nq and st["fallback_queries"] == ic.coarse_stats(p[3], p[6], nprobe)["fallback_queries"], st


def test_the_contracts_bound_on_nlist(lsq, engine):
    """reaches: nlist = 2^24 (24 list bits: 56 key bits, the contract's most), offsets of 2^24 + 1 entries opened by 4097 threads, a coarse search over
    2^24 centroids with stride 1024, centroid rows at l * d up to 2^25.  Evidence: Index.nlist, probed_rows of ivf_info against the checker's lists"""
    import torch
    p, nprobe, nn = ic.bound_problem()
    codes, K, dbn, cent, lor, Qs, Qc = p
    nlist = cent.shape[0]
    assert nlist == ic.BOUND
    counts = np.bincount(lor, minlength=nlist)
    hix = engine.index(codes, K, dbn, 8)
    dix = engine.index_dev(*[torch.from_numpy(a).cuda() for a in (codes, K, dbn)], 8)
    dcent, dlor = torch.from_numpy(cent).cuda(), torch.from_numpy(lor).cuda()
    with hix, dix:
        for ix, args in ((hix, (cent, lor)), (dix, (dcent, dlor))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ix.set_lists(*args)
            torch.cuda.synchronize()
            print("set_lists at nlist = %d, n = %d, %s form: %.3f s" % (nlist, codes.shape[0], "device" if ix._dev else "host", time.perf_counter() - t0))
        assert hix.nlist == dix.nlist == nlist
        for k in (nprobe, 1):
            t0 = time.perf_counter()
            _many(lsq, (hix, dix), p, k, nn, ("bound", k))
            print("nprobe = %d: checker twice and 8 searches in %.3f s" % (k, time.perf_counter() - t0))
            t0 = time.perf_counter()
            got = hix.search_ivf(Qs, nn, k, Q_coarse=Qc)
            print("search_ivf at nlist = %d, nprobe = %d, host form: %.3f s" % (nlist, k, time.perf_counter() - t0))
            probes = lsq.knn_exact(np.ascontiguousarray(cent.T), np.ascontiguousarray(Qc.T), k)[1].T.astype(np.int64) - 1
            assert hix.ivf_info()["probed_rows"] == int(counts[probes].sum()) and np.all(got[1] > 0)
