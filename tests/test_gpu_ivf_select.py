"""Option "ivf_select" (csrc/lsq_ivfsel.hip): lsq_index_search_ivf with each query's nn best records kept in LDS while its probed lists are scanned.  The
contract is an identity: a served call returns, bit for bit, what the same call returns with the option off, which is the host checker's answer
(lsq_ivf_search_cpu; under a filter, its full ranking cut to the allowed rows).  Every case compares the three and holds lsq_ivf_select_info to
served_queries == queries and reason == 0, so that a silent fall-back cannot pass."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_check as fc  # noqa: E402
import ivf_check as ic  # noqa: E402
import packed_check as pk  # noqa: E402
from test_gpu_ivf import _indexes  # noqa: E402  (a host-buffer index and a borrowed-device one over the same problem, lists set on both)

pytestmark = pytest.mark.gpu


def _call(ix, what, Qs, k, nprobe, **kw):
    """Index.search_ivf / search_rows with numpy arguments on either kind of index -> numpy (dists, ids)"""
    if not ix._dev:
        return getattr(ix, what)(Qs, k, nprobe, **kw)
    import torch
    kw = {a: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for a, v in kw.items()}
    dd, di = getattr(ix, what)(torch.from_numpy(Qs).cuda(), k, nprobe, **kw)
    return dd.cpu().numpy(), di.cpu().numpy()


def _three(engine, ix, Qs, nn, nprobe, want=None, reason=0, what="search_ivf", **kw):
    """the call with the option off, with it on, and the checker's `want`: the same bits; the info says the pools answered (or `reason`) -> that info"""
    off = _call(ix, what, Qs, nn, nprobe, **kw)
    engine.set_option("ivf_select", 1)
    try:
        on = _call(ix, what, Qs, nn, nprobe, **kw)
        sel, info = ix.ivf_select_info(), ix.ivf_info()
    finally:
        engine.set_option("ivf_select", 0)
    assert fc.same(on, off) and (want is None or fc.same(on, want)), (ix._dev, nn, nprobe)
    nq = Qs.shape[0]
    assert sel["queries"] == nq and sel["reason"] == reason and sel["served_queries"] == (0 if reason else nq)
    if not reason:
        L = kw.get("shortlist") or nn
        assert sel["pool_records"] == 2 * max(256, 1 << (L - 1).bit_length()) and sel["pool_bytes"] == 8 * sel["pool_records"]
        assert (info["queries"], info["threshold_queries"], info["fallback_queries"], info["tail_capacity"]) == (nq, 0, 0, 0)
    return sel


def _cpu(lsq, p, nprobe, nn, flags=0):
    rc, rd, ri = ic.ivf_cpu(lsq._lib.load(), *p, nprobe, nn, flags=flags)
    assert rc == 0
    return rd, ri


@pytest.mark.parametrize("name", sorted(ic.PROBLEMS))
def test_named_problems(lsq, engine, name):
    p, nprobe, nn = ic.PROBLEMS[name]()
    want = _cpu(lsq, p, nprobe, nn)
    hix, dix = _indexes(engine, p)
    with hix, dix:
        for ix in (hix, dix):
            _three(engine, ix, p[5], nn, nprobe, want, Q_coarse=p[6])


@functools.lru_cache(maxsize=None)
def _skewed(m=8, nq=37):
    """3000 rows on 40 skewed lists (empty ones, one-row ones, one of half the rows), NaN norms sprinkled in"""
    p = ic.problem(ic.N, 32, m, 40, nq, 300 + m + nq)
    p[2][5::97] = np.float32(np.nan)
    return p


@pytest.mark.parametrize("nprobe", [40, 1])
@pytest.mark.parametrize("nn", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 2048, 2049])
def test_nn_edges(lsq, engine, nn, nprobe):
    """the pool's sizes (P = 512 up to nn = 256, then 1024, 2048, 4096) and both sides of each; nprobe = 1: lists shorter than nn, padded; nn = 2049 is not
    served and says so"""
    p = _skewed()
    with engine.index(*p[:3], 8) as ix:
        ix.set_lists(p[3], p[4])
        _three(engine, ix, p[5], nn, nprobe, _cpu(lsq, p, nprobe, nn), reason=lsq._lib.IVF_SELECT_NN_TOO_LARGE if nn > 2048 else 0, Q_coarse=p[6])


@pytest.mark.parametrize("order", ["decreasing", "increasing", "identical", "tie-cut"])
def test_arrival_order(lsq, engine, order):
    """one list of 5000 rows, m = 1, a block per query.  Norms that dominate the tables and fall with the row id: every row beats the bound; rising:
    none does after the first compaction; identical rows: the order is by id alone; small integers: nn cuts a group of equal distances"""
    nn, nq = 10, 3
    p = ic.problem(5000, 5, 1, 1, nq, 41, small_int=(order == "tie-cut"))
    if order in ("decreasing", "increasing"):
        ramp = np.arange(5000, dtype=np.float32) * np.float32(1000)
        p[2][:] = ramp[::-1] if order == "decreasing" else ramp
    elif order == "identical":
        p[0][:], p[2][:] = p[0][0], p[2][0]
    want = _cpu(lsq, p, 1, nn + 1)
    if order == "tie-cut":
        assert np.any(want[0][:, nn - 1] == want[0][:, nn])
    with engine.index(*p[:3], 1) as ix:
        ix.set_lists(p[3], p[4])
        sel = _three(engine, ix, p[5], nn, 1, (want[0][:, :nn], want[1][:, :nn]), Q_coarse=p[6])
        assert sel["blocks_per_query"] == 1 and sel["merged_runs"] == 0
        if order == "decreasing":
            assert sel["compactions"] >= 2 * nq
        if order == "increasing":
            assert sel["compactions"] == nq


@pytest.mark.parametrize("nq,flags", [(1, 0), (37, 0), (37, ic.TEST_BATCH), (2049, 0)], ids=["nq1", "nq37", "nq37-test-batch", "nq2049"])
def test_blocks_per_query(lsq, engine, nq, flags):
    """40 probed lists: 40 blocks per query and 40 runs merged while the batch has few queries, one block and no merge from 2048 queries on"""
    p = _skewed(nq=nq)
    splits = ic.scan_splits(8 if flags else nq, 40)
    assert splits == (1 if nq == 2049 else 40)
    with engine.index(*p[:3], 8) as ix:
        ix.set_lists(p[3], p[4])
        sel = _three(engine, ix, p[5], 10, 40, _cpu(lsq, p, 40, 10), Q_coarse=p[6], flags=flags)
        assert sel["blocks_per_query"] == splits and sel["merged_runs"] == (nq * splits if splits > 1 else 0)
        assert ix.ivf_info()["batches"] == (-(-nq // 8) if flags else 1)


@pytest.mark.parametrize("m,packed,add", [(4, 0, 0), (5, 0, 0), (8, 0, 0), (16, 0, 0), (7, 1, 0), (8, 1, 0), (8, 0, 1), (7, 1, 1)],
                         ids=["m4-dword", "m5-bytes", "m8-dwords", "m16-dwords", "packed-m7-dwords", "packed-m8-bytes", "m8-add-coarse", "packed-m7-add-coarse"])
@pytest.mark.parametrize("nprobe,nn", [(3, 10), (40, 300)])
def test_row_formats(lsq, engine, m, packed, add, nprobe, nn):
    codes, K, dbn, cent, lor, Qs, Qc = _skewed(m=m)
    cb, nc = pk.quantize(dbn)
    p = (codes, K, cb[nc] if packed else dbn, cent, lor, Qs, Qc)
    with (engine.index_packed(codes, K, nc, cb, m) if packed else engine.index(codes, K, dbn, m)) as ix:
        ix.set_lists(cent, lor)
        _three(engine, ix, Qs, nn, nprobe, _cpu(lsq, p, nprobe, nn, flags=ic.ADD_COARSE if add else 0), Q_coarse=Qc, add_coarse=bool(add))


@pytest.mark.parametrize("packed", [0, 1], ids=["plain", "packed"])
@pytest.mark.parametrize("which", ["all", "half", "one-in-64", "list-denied"])
def test_filters(lsq, engine, which, packed):
    codes, K, dbn, cent, lor, Qs, Qc = _skewed(m=7)
    rng = np.random.default_rng(8)
    allowed = {"all": np.ones(ic.N, dtype=bool), "half": rng.random(ic.N) < 0.5, "one-in-64": rng.random(ic.N) < 1 / 64, "list-denied": lor != 0}[which]
    cb, nc = pk.quantize(dbn)
    p = (codes, K, cb[nc] if packed else dbn, cent, lor, Qs, Qc)
    if packed:
        ixs = (engine.index_packed(codes, K, nc, cb, 7),)
        ixs[0].set_lists(cent, lor)
    else:
        ixs = _indexes(engine, p)
    for ix in ixs:
        with ix:
            fc.set_filter(ix, mask=allowed.copy())
            for nprobe, nn in ((3, 10), (40, 300)):
                want = fc.filtered(*fc.full_ivf(lsq._lib.load(), p, nprobe), allowed, nn, 0)
                _three(engine, ix, Qs, nn, nprobe, want, Q_coarse=Qc)


def test_behind_and_around(lsq, engine):
    """stage two on the pools' shortlist, search by stored row, and an index whose rows were added, removed and compacted"""
    p = _skewed()
    codes, K, dbn, cent, lor, Qs, Qc = p
    rng = np.random.default_rng(9)
    base = rng.standard_normal((ic.N, 32)).astype(np.float32)
    L = lsq._lib.load()
    hix, dix = _indexes(engine, p, base=base)
    with hix, dix:
        for ix in (hix, dix):
            want = fc.two_stage(L, _cpu(lsq, p, 40, 300)[1], base, Qs, 10)
            _three(engine, ix, Qs, 10, 40, want, Q_coarse=Qc, Q_exact=Qs, shortlist=300)
            _three(engine, ix, np.arange(0, 74, 2, dtype=np.int32), 10, 3, what="search_rows")
    with engine.index(codes[:2000], K, dbn[:2000], 8) as ix:
        ix.set_lists(cent, lor[:2000])
        ix.add(codes=codes[2000:], dbnorms=dbn[2000:], assign=lor[2000:])
        _three(engine, ix, Qs, 300, 40, _cpu(lsq, p, 40, 300), Q_coarse=Qc)
        gone = rng.permutation(ic.N)[:700].astype(np.int32)
        keep = np.ones(ic.N, dtype=bool)
        keep[gone] = False
        want = fc.filtered(*fc.full_ivf(L, p, 40), keep, 300, 0)
        ix.remove(gone)
        _three(engine, ix, Qs, 300, 40, want, Q_coarse=Qc)
        old = np.asarray(ix.compact())
        got = _three(engine, ix, Qs, 300, 40, None, Q_coarse=Qc)
        assert got["served_queries"] == 37
        dd, di = ix.search_ivf(Qs, 300, 40, Q_coarse=Qc)
        assert fc.same((dd, np.where(di > 0, old[np.maximum(di, 1) - 1] + 1, 0)), want)
