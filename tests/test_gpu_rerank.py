"""The resident index on the device (lsq_index_*): the exact re-rank against lsq_rerank_cpu bit for bit on every road of the kernel, batch boundaries,
stage one against Engine.linscan, the two stages together against the host checker and exact k-NN, and the state of a context shared with other calls."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from knn_check import same_bits  # noqa: E402
from rerank_check import DIMS, LISTS, base_and_queries, padded, rerank_cpu  # noqa: E402

pytestmark = pytest.mark.gpu
H = 256
N = 1200
NQS = [1, 129, 300]                          # one query, more than 128 (two tiles of the scan's queries and one more), several hundred


def _check(lsq, ix, Xq, cand, k, id_base, ref, what):
    """one re-rank through the index (host arrays, or tensors for a borrowed-device index) against the host checker's (dists, ids)"""
    if ix._dev:
        import torch
        dd, di = ix.rerank(torch.from_numpy(Xq).cuda(), torch.from_numpy(cand).cuda(), k, id_base=id_base)
        dd, di = dd.cpu().numpy(), di.cpu().numpy()
    else:
        dd, di = ix.rerank(Xq, cand, k, id_base=id_base)
    assert same_bits(dd, ref[0][:, :k]) and np.array_equal(di, ref[1][:, :k]), what


def _matrix(lsq, engine, Xbp, d, u8, seed, dev_base=None):
    """every list length, both id bases, nn = 1 and L, each with its own nq, through a host-buffer index and a borrowed-device one"""
    import torch
    L = lsq._lib.load()
    rng = np.random.default_rng(seed)
    _, Xq = base_and_queries(d, 2, max(NQS), seed + 1, u8=u8)
    dbase = dev_base if dev_base is not None else torch.from_numpy(Xbp).cuda()[:, :d]
    calls = 0
    with engine.index(None, None, None, 0, base=Xbp, d=d) as hix, engine.index_dev(None, None, None, 0, base=dbase, d=d) as dix:
        for li, Lc in enumerate(LISTS):
            for id_base in (0, 1):
                nq = NQS[(li + id_base) % 3]
                cand = rng.integers(id_base, N + id_base, (nq, Lc)).astype(np.int32)
                cand[0, 0] = N + id_base                                       # one id outside the base in every call
                rc, rd, ri = rerank_cpu(L, Xbp, Xq[:nq], cand, d, Lc, id_base)
                assert rc == 0
                for nn in sorted({1, Lc}):
                    calls += 1
                    for ix in (hix, dix):
                        _check(lsq, ix, Xq[:nq], cand, nn, id_base, (rd, ri), (d, Xbp.shape, Lc, nn, id_base, nq, ix._dev))
        st = hix.stats()
        assert st["queries"] > 0 and st["invalid"] == calls and st["rows"] > 0 and st["batches"] == calls and dix.stats() == st


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("d", DIMS)
def test_f32_rerank_equals_the_host_checker(lsq, engine, d, pad):
    Xb, _ = base_and_queries(d, N, 1, 100 + d)
    _matrix(lsq, engine, padded(Xb, pad, np.float32(np.nan)), d, False, 10 * d + pad)


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("d", DIMS)
def test_uint8_rerank_equals_the_host_checker(lsq, engine, d, pad):
    L = lsq._lib.load()
    Xb, Xq = base_and_queries(d, N, 3, 200 + d, u8=True)
    Xbp = padded(Xb, pad, np.uint8(255))
    _matrix(lsq, engine, Xbp, d, True, 20 * d + pad)
    # ... and the f32 call on the widened base gives the same bits
    cand = np.random.default_rng(d).integers(0, N, (3, 65)).astype(np.int32)
    rc, rd, ri = rerank_cpu(L, Xbp, Xq, cand, d, 65, 0)
    with engine.index(None, None, None, 0, base=Xbp.astype(np.float32), d=d) as fix:
        _check(lsq, fix, Xq, cand, 65, 0, (rd, ri), "widened")


@pytest.mark.parametrize("d,ldb,offset", [(17, 19, 1), (128, 131, 1), (16, 20, 4), (130, 132, 4), (3, 3, 2)])
def test_uint8_rows_at_a_byte_offset(lsq, engine, d, ldb, offset):
    """a view into a larger byte buffer: offset 1 with an odd pitch takes the byte loads, offset 4 with a pitch that is a multiple of 4 the dword loads"""
    import torch
    Xb, _ = base_and_queries(d, N, 1, 300 + d, u8=True)
    Xbp = padded(Xb, ldb - d, np.uint8(7))
    flat = torch.zeros(offset + N * ldb + 64, dtype=torch.uint8, device="cuda")
    flat[offset:offset + N * ldb] = torch.from_numpy(Xbp.reshape(-1)).cuda()
    view = flat[offset:offset + N * ldb].view(N, ldb)[:, :d]
    assert view.data_ptr() % 16 == offset
    _matrix(lsq, engine, Xbp, d, True, 30 * d, dev_base=view)


@pytest.mark.parametrize("u8", [False, True])
def test_batch_boundaries(lsq, u8):
    L = lsq._lib.load()
    d, nq, Lc = 17, 300, 65
    Xb, Xq = base_and_queries(d, N, nq, 41, u8=u8)
    cand = np.random.default_rng(42).integers(1, N + 1, (nq, Lc)).astype(np.int32)
    rc, rd, ri = rerank_cpu(L, Xb, Xq, cand, d, Lc, 1)
    with lsq.Engine(0) as eng, eng.index(None, None, None, 0, base=Xb) as ix:
        for batch, batches in ((0, 1), (1, 300), (7, 43), (128, 3)):
            eng.set_option("rerank_batch", batch)
            before = ix.stats()["batches"]
            _check(lsq, ix, Xq, cand, 9, 1, (rd, ri), batch)
            assert ix.stats()["batches"] - before == batches


def _database(n, d, m, nq, seed):
    """codes, codebooks and norms of a quantised base: base rows = their reconstruction + noise, queries = base rows + noise"""
    rng = np.random.default_rng(seed)
    K = (rng.standard_normal((m * H, d)) / np.sqrt(m)).astype(np.float32)
    codes = rng.integers(0, H, (n, m)).astype(np.uint8)
    recon = sum(K[j * H + codes[:, j].astype(np.int64)] for j in range(m))
    dbn = (recon.astype(np.float64) ** 2).sum(1).astype(np.float32)
    Xb = (recon + 0.35 * rng.standard_normal((n, d))).astype(np.float32)
    Xq = (Xb[rng.integers(0, n, nq)] + 0.25 * rng.standard_normal((nq, d))).astype(np.float32)
    return codes, K, dbn, Xb, Xq


@pytest.mark.parametrize("n,m,d,nq", [(3000, 4, 24, 33), (70000, 8, 16, 64)])      # the scan's exhaustive road, and its threshold road
def test_stage_one_is_the_scan_unchanged(lsq, engine, n, m, d, nq):
    import torch
    codes, K, dbn, Xb, Xq = _database(n, d, m, nq, n)
    rd, ri = engine.linscan(codes, Xq, K, dbn, m, 10)
    with engine.index(codes, K, dbn, m) as ix:                                  # scan-only
        dd, di = ix.search(Xq, 10)
        assert same_bits(dd, rd) and np.array_equal(di, ri) and di.dtype == np.int32
    t = [torch.from_numpy(a).cuda() for a in (codes, K, dbn, Xb)]
    with engine.index_dev(t[0], t[1], t[2], m, base=t[3]) as ix:
        dd, di = ix.search(torch.from_numpy(Xq).cuda(), 10)
        assert same_bits(dd.cpu().numpy(), rd) and np.array_equal(di.cpu().numpy(), ri)
    assert engine.linscan_stats()["exhaustive"] == (1 if n <= 65536 else 0)


@pytest.mark.parametrize("n,m,d,nq,Lc", [(3000, 4, 24, 33, 100), (70000, 8, 16, 64, 200)])
def test_two_stage_search(lsq, engine, n, m, d, nq, Lc):
    import torch
    L = lsq._lib.load()
    codes, K, dbn, Y, Yq = _database(n, d, m, nq, n + 1)
    R = np.linalg.qr(np.random.default_rng(3).standard_normal((d, d)))[0].astype(np.float32)
    Xb, Xq = np.ascontiguousarray(Y @ R.T), np.ascontiguousarray(Yq @ R.T)      # the base set's own frame: the codes describe R'x
    Qs = np.ascontiguousarray((R.T @ Xq.T).T)                                   # what the scan reads (linscan_lsq's R'X) is not what the re-rank reads
    _, short = engine.linscan(codes, Qs, K, dbn, m, Lc)
    rc, rd, ri = rerank_cpu(L, Xb, Xq, short, d, Lc, 1)
    assert rc == 0
    with engine.index(codes, K, dbn, m, base=Xb) as ix:
        for k in (1, 10, Lc):
            dd, di = ix.search(Qs, k, shortlist=Lc, Q_exact=Xq)
            assert same_bits(dd, rd[:, :k]) and np.array_equal(di, ri[:, :k]), k
    t = [torch.from_numpy(a).cuda() for a in (codes, K, dbn, Xb)]
    with engine.index_dev(t[0], t[1], t[2], m, base=t[3]) as ix:
        dd, di = ix.search(torch.from_numpy(Qs).cuda(), 10, shortlist=Lc, Q_exact=torch.from_numpy(Xq).cuda())
        assert same_bits(dd.cpu().numpy(), rd[:, :10]) and np.array_equal(di.cpu().numpy(), ri[:, :10])
    # wherever the exact nearest neighbour made the shortlist, it comes out first
    _, gt = engine.knn_exact(Xb, Xq, 1)
    inside = (short == (gt.astype(np.int32) + 1)).any(axis=1)
    assert inside.sum() >= nq // 2 and np.array_equal(ri[inside, 0], gt[inside, 0].astype(np.int32) + 1)
    # the Julia-shaped call
    jd, ji = lsq.linscan_lsq_rerank(codes.T, Xq.T, [K[j * H:(j + 1) * H].T for j in range(m)], dbn, R, Xb.T, Lc, 10, engine=engine)
    assert same_bits(jd.T, rd[:, :10]) and np.array_equal(ji.T, ri[:, :10])


def test_shortlist_of_everything_is_exact_knn(lsq, engine):
    n, m, d, nq = 3000, 4, 24, 20
    codes, K, dbn, Xb, Xq = _database(n, d, m, nq, 5)
    kd, ki = engine.knn_exact(Xb, Xq, 50)
    with engine.index(codes, K, dbn, m, base=Xb) as ix:
        dd, di = ix.search(Xq, 50, shortlist=n)
    assert same_bits(dd, kd) and np.array_equal(di, ki.astype(np.int32) + 1)


def _state_ops(lsq):
    """name -> f(engine, indexes) -> a tuple of arrays: the calls whose every ordered pair shares one context"""
    n, m, d, nq = 2000, 4, 16, 40
    codes, K, dbn, Xb, Xq = _database(n, d, m, nq, 77)
    codes2, K2, dbn2, Xb2, Xq2 = _database(900, 12, 2, 17, 78)
    rng = np.random.default_rng(79)
    cand = rng.integers(0, n, (nq, 70)).astype(np.int32)
    Xe = rng.integers(0, 256, (300, d)).astype(np.float32)
    B0 = rng.integers(1, H + 1, (300, m)).astype(np.int16)
    # the host-buffer searches share one set of staging buffers: every kind of them, at two shapes, and one call that grows the buffers for the rest
    pq_codes = rng.integers(0, H, (1500, 7)).astype(np.uint8)                   # 3 of the 7 bytes of a row are codes
    pq_C = rng.standard_normal((3, H, 5)).astype(np.float32)
    pq_Q = rng.standard_normal((11, 17)).astype(np.float32)                     # 15 of the 17 floats of a row are read
    codes3, K3, dbn3, _, Xq3 = _database(70000, 16, 8, 16, 80)                  # above the exhaustive road's limit of 65536 codes
    make ={"a": lambda e: e.index(codes, K, dbn, m, base=Xb), "b": lambda e: e.index(codes2, K2, dbn2, 2, base=np.minimum(np.abs(Xb2) * 40, 255).astype(np.uint8))}
    ops = {
        "index.search": lambda e, ix: ix["a"].search(Xq, 5, shortlist=60),
        "index.rerank": lambda e, ix: ix["a"].rerank(Xq, cand, 70, id_base=0),
        "index2.search": lambda e, ix: ix["b"].search(Xq2, 3, shortlist=33),
        "linscan": lambda e, ix: e.linscan(codes, Xq, K, dbn, m, 25),
        "knn_exact": lambda e, ix: e.knn_exact(Xb, Xq, 7),
        "encode_icm": lambda e, ix: e.encode_icm(Xe, B0, K, m, [2], 2, 2, True, seed=3),
        "linscan_pq": lambda e, ix: e.linscan_pq(pq_codes, pq_Q, pq_C, 3, 20, 5),
        "knn_exact2": lambda e, ix: e.knn_exact(Xb2, Xq2, 5),
        "linscan2": lambda e, ix: e.linscan(codes2, Xq2, K2, dbn2, 2, 9),
        "linscan_big": lambda e, ix: e.linscan(codes3, Xq3, K3, dbn3, 8, 10),
    }
    return make, ops


def test_every_ordered_pair_on_one_context_equals_a_fresh_context(lsq):
    make, ops = _state_ops(lsq)
    fresh = {}
    for name, f in ops.items():
        with lsq.Engine(0) as e:
            ix = {k: mk(e) for k, mk in make.items()}
            fresh[name] = f(e, ix)
            for i in ix.values():
                i.close()
    with lsq.Engine(0) as e:
        ix = {k: mk(e) for k, mk in make.items()}
        for a in ops:
            for b in ops:
                for name in (a, b):
                    got = ops[name](e, ix)
                    assert all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(got, fresh[name])), (a, b, name)
        # a destroyed index leaves the context, and the other index, usable
        ix["a"].close()
        for name in ("index2.search", "linscan", "knn_exact", "encode_icm"):
            got = ops[name](e, ix)
            assert all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(got, fresh[name])), name
        ix["b"].close()
        got = ops["linscan"](e, ix)
        assert np.array_equal(got[1], fresh["linscan"][1])


def test_bad_arguments_launch_nothing(lsq, engine):
    EINVAL = lsq._lib.LSQ_EINVAL
    codes, K, dbn, Xb, Xq = _database(500, 8, 2, 4, 9)
    cand = np.zeros((4, 6), dtype=np.int32)

    def rejected(f, word):
        with pytest.raises(lsq._lib.LsqError) as err:
            f()
        assert err.value.code == EINVAL and word in str(err.value)
        assert word.encode() in lsq._lib.load().lsq_last_error()

    with engine.index(codes, K, dbn, 2, base=Xb) as ix, engine.index(codes, K, dbn, 2) as scan_only, \
            engine.index(None, None, None, 0, base=Xb) as base_only:
        before = [i.stats() for i in (ix, scan_only, base_only)]
        rejected(lambda: ix.rerank(Xq, cand, 7), "nn")                          # nn > L
        rejected(lambda: ix.rerank(Xq, cand, 0), "nn")
        rejected(lambda: ix.rerank(Xq, cand, 2, id_base=2), "id_base")
        rejected(lambda: ix.search(Xq, 5, shortlist=501), "shortlist")          # shortlist > n
        rejected(lambda: ix.search(Xq, 5, shortlist=3), "shortlist")            # shortlist < nn
        rejected(lambda: ix.search(Xq, 501), "exceeds")
        rejected(lambda: scan_only.rerank(Xq, cand, 2), "no base rows")
        rejected(lambda: scan_only.search(Xq, 2, shortlist=5), "base rows")
        rejected(lambda: base_only.search(Xq, 2), "no codes")
        L = lsq._lib.load()
        out_d, out_i = np.zeros((4, 2), np.float32), np.zeros((4, 2), np.int32)
        assert L.lsq_index_rerank(ix._h, out_d.ctypes.data, out_i.ctypes.data, None, cand.ctypes.data, 4, 8, 6, 2, 0, 0) == EINVAL
        assert L.lsq_index_rerank(ix._h, None, out_i.ctypes.data, Xq.ctypes.data, cand.ctypes.data, 4, 8, 6, 2, 0, 0) == EINVAL
        assert L.lsq_index_search(ix._h, out_d.ctypes.data, out_i.ctypes.data, None, None, 4, 8, 0, 2, 0) == EINVAL and b"null" in L.lsq_last_error()
        assert L.lsq_index_search(ix._h, out_d.ctypes.data, out_i.ctypes.data, Xq.ctypes.data, None, 4, 8, 5, 2, 0) == EINVAL
        assert L.lsq_index_search(ix._h, out_d.ctypes.data, out_i.ctypes.data, Xq.ctypes.data, Xq.ctypes.data, 4, 7, 5, 2, 0) == EINVAL      # ldq < d
        assert [i.stats() for i in (ix, scan_only, base_only)] == before        # nothing ran: no query, no batch, no row counted
        assert not out_d.any() and not out_i.any()
    # a description nothing can be built from
    for kw, word in ((dict(codes=None, K=None, dbnorms=None, m=0, base=None), None), (dict(codes=codes, K=K[:2 * 128], dbnorms=dbn, m=2, h=128), "h == 256")):
        with pytest.raises((ValueError, lsq._lib.LsqError)) as err:
            engine.index(kw["codes"], kw["K"], kw["dbnorms"], kw["m"], base=kw.get("base"), h=kw.get("h", H))
        assert word is None or word in str(err.value)
