"""Labelled range search (csrc/lsq_labelrange.hip): Index.range_search with where=(mask, want), a row predicate per query.  The contract is Identity LR: every
query's lims, distances and ids equal, bit for bit, the host drop-in lsq_range_search_cpu for that single query with allowed = (its predicate AND the filter
in force) -- which is what set_filter(those rows) and a one-query range_search return."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_check as fc  # noqa: E402
import ivf_check as ic  # noqa: E402
import range_check as rc  # noqa: E402
import test_gpu_labels as tl  # noqa: E402  (its base, labels and predicates: 20 011 rows, 9 queries in groups of 4 + 4 + 1, 40 skewed lists)

pytestmark = pytest.mark.gpu

N, NQ, NLIST = tl.N, tl.NQ, tl.NLIST
# the radius of each query, by range_check.radii's names over the query's OWN candidates: all of them; (no row); the one row exactly; an exact 10th distance of
# the small-integer problem (a tie group is cut at a member); a midpoint; half of the last step's rows; one float below the minimum; nothing; NaN -- so the
# group of queries 4 .. 7 has empty cells and the group of query 8 has only empty cells
RADIUS = ("+inf", "+inf", "min", "10th", "mid-10-11", "half", "below-min", "-inf", "nan")


def _cpu(lsq, p, q, radius, allowed, nprobe, add):
    codes, K, dbn, cent, lor, Qs, Qc = p
    got = rc.range_cpu(lsq._lib.load(), codes, K, dbn, Qs[q:q + 1], radius, cent if nprobe else None, lor if nprobe else None, nprobe,
                       ic.ADD_COARSE if add else 0, Qc[q:q + 1] if nprobe else None, allowed=allowed)
    assert got[0] == 0
    return got[1:]


@functools.lru_cache(maxsize=None)
def _want(lsq, m, packed, nprobe, add, any_of, keep=None):
    """-> radius (NQ,), the reference (lims, dists, ids), the candidates of every query among the rows walked; keep: a key of _KEEP (a filter in force)"""
    p, labels, _, _ = tl._problem(lsq, m, packed, "tie-cut")
    ok = tl._allowed(labels, any_of) & (True if keep is None else _keep(keep)[None, :])
    radius, parts, cand = np.zeros(NQ, np.float32), [], 0
    for q in range(NQ):
        every = _cpu(lsq, p, q, np.inf, ok[q], nprobe, add)      # the query's candidates, ranked
        cand += int(every[0][-1])
        radius[q] = rc.radii(every[1][None, :])[RADIUS[q]][0] if every[1].size else np.float32(np.inf)
        parts.append(_cpu(lsq, p, q, radius[q], ok[q], nprobe, add))
    lims = np.concatenate([[0], np.cumsum([int(x[0][-1]) for x in parts])]).astype(np.int64)
    return radius, (lims, np.concatenate([x[1] for x in parts]), np.concatenate([x[2] for x in parts])), cand


def _keep(seed):
    return np.random.default_rng(seed).random(N) < 0.5


def _range(ix, p, radius, nprobe, add, any_of):
    where = (tl.ANY, np.zeros(NQ, np.uint32)) if any_of else (tl.WHERE[:, 0].copy(), tl.WHERE[:, 1].copy())
    got = ix.range_search(tl._np(ix, p[5]), tl._np(ix, radius), nprobe=nprobe, Q_coarse=tl._np(ix, p[6]), add_coarse=add,
                          where=tuple(tl._np(ix, a) for a in where), any_of=any_of)
    return tuple(a.cpu().numpy() for a in got) if ix._dev else got


@pytest.mark.parametrize("nprobe,add", [(0, False), (5, True), (NLIST, False)], ids=["every-row", "nprobe5-add", "nprobe-nlist"])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("m,packed", [(8, False), (5, False), (16, False), (7, True), (8, True)], ids=["m8", "m5-bytes", "m16", "packed-m7", "packed-m8-bytes"])
def test_identity(lsq, engine, m, packed, dev, nprobe, add):
    """both loaders, both queries-per-block, plain and packed rows on either road, both rules: bit for bit the host drop-in per query; the account of the call"""
    p, labels, pck, _ = tl._problem(lsq, m, packed, "tie-cut")
    with tl._index(engine, p, m, pck if packed else None, dev) as ix:
        ix.set_lists(tl._np(ix, p[3]), tl._np(ix, p[4]))
        ix.set_labels(tl._np(ix, labels))
        for any_of in (False, True):
            radius, want, cand = _want(lsq, m, packed, nprobe, add, any_of)
            counts = np.diff(want[0])
            assert counts.min() == 0 and (nprobe == 5 or any_of or counts.max() == N)      # an empty result; every row of the base
            assert rc.same(_range(ix, p, radius, nprobe, add, any_of), want), (m, packed, dev, nprobe, any_of)
            info = ix.label_range_info()
            assert info["cells_per_query"] >= 3 and info["cells"] == NQ * info["cells_per_query"] and info["queries_per_block"] == (1 if nprobe else 4 if m <= 8 else 2)
            assert 0 < info["cells_nonempty"] < info["cells"] and 0 < info["fill_blocks_skipped"] < info["fill_blocks_launched"]
            assert (info["results"], info["allowed_pairs"], info["queries"]) == (int(want[0][-1]), cand, NQ)
            assert ix.range_info()["results"] == info["results"] and ix.range_info()["max_per_query"] == counts.max()


@pytest.mark.parametrize("m,packed,nprobe,add", [(8, False, 0, False), (7, True, 5, True)], ids=["m8-every-row", "packed-m7-nprobe5-add"])
def test_filter_batches_and_the_held_result(lsq, engine, m, packed, nprobe, add):
    """a filter in force over removed rows; option range_batch = 1, 64 and 1000: the same result; the held result fetched twice, then dropped by set_filter"""
    p, labels, pck, _ = tl._problem(lsq, m, packed, "tie-cut")
    radius, want, cand = _want(lsq, m, packed, nprobe, add, False, keep=21)
    total, L = int(want[0][-1]), lsq._lib.load()
    keep = _keep(21)
    with tl._index(engine, p, m, pck if packed else None) as ix:
        ix.set_lists(p[3], p[4])
        ix.set_labels(labels)
        ix.remove(np.flatnonzero(~keep)[::2].astype(np.int32))       # half of the rows that the filter excludes are tombstones as well
        fc.set_filter(ix, mask=keep.copy())
        try:
            for budget in (1, 64, 1000, 0):
                engine.set_option("range_batch", budget)
                assert rc.same(_range(ix, p, radius, nprobe, add, False), want), budget
                info = ix.label_range_info()
                assert info["allowed_pairs"] == cand and (budget != 1 or info["batches"] == int((np.diff(want[0]) > 0).sum()))
        finally:
            engine.set_option("range_batch", 0)
        for _ in range(2):
            d, i = np.full(total + 8, -77, np.float32), np.full(total + 8, -77, np.int32)
            assert L.lsq_index_range_fetch(ix._h, d.ctypes.data, i.ctypes.data, total, 0) == 0
            assert rc.same((want[0], d[:total], i[:total]), want) and np.all(i[total:] == -77)
        fc.set_filter(ix, mask=keep.copy())
        assert L.lsq_index_range_fetch(ix._h, d.ctypes.data, i.ctypes.data, total, 0) == lsq._lib.LSQ_EINVAL


def test_plain_call_and_refusals(lsq, engine):
    """where=None is the unlabelled call; what is refused is refused with LSQ_EINVAL, lims untouched and the former held result still fetchable"""
    p, labels, _, _ = tl._problem(lsq, 8, False, "tie-cut")
    L, EINVAL = lsq._lib.load(), lsq._lib.LSQ_EINVAL
    radius, want, _ = _want(lsq, 8, False, 0, False, False)
    zeros, lims = np.zeros(NQ, np.uint32), np.full(NQ + 1, -7, np.int64)
    ptr = lambda a: a.ctypes.data      # noqa: E731
    with tl._index(engine, p, 8) as ix:
        plain = ix.range_search(p[5], radius)
        assert rc.same(plain, rc.range_cpu(L, p[0], p[1], p[2], p[5], radius)[1:]) and ix.range_info()["results"] == plain[0][-1] > 0
        total = int(plain[0][-1])

        def raw(h=ix._h, lm=ptr(lims), Q=ptr(p[5]), rad=ptr(radius), qm=ptr(zeros), qw=ptr(zeros), nq=NQ, ldq=tl.D, nprobe=0, flags=0, lf=0):
            code = L.lsq_index_range_search_labelled(h, lm, Q, None, rad, qm, qw, nq, ldq, nprobe, flags, lf, 0)
            d, i = np.zeros(total, np.float32), np.zeros(total, np.int32)
            held = L.lsq_index_range_fetch(ix._h, d.ctypes.data, i.ctypes.data, total, 0) == 0 and rc.same((plain[0], d, i), plain)
            return code == EINVAL and np.all(lims == -7) and held

        assert raw()                                                  # no labels in force
        ix.set_labels(labels)
        for bad in (dict(h=None), dict(lm=None), dict(Q=None), dict(rad=None), dict(qm=None), dict(qw=None), dict(nq=-1), dict(ldq=tl.D - 1), dict(nprobe=-1),
                    dict(nprobe=1), dict(flags=ic.ADD_COARSE), dict(flags=2), dict(lf=lsq._lib.LABEL_TEST_ONE_SPLIT), dict(lf=4)):
            assert raw(**bad), bad
        ix.set_lists(p[3], p[4])
        plain = ix.range_search(p[5], radius)
        assert raw(nprobe=NLIST + 1) and raw(nprobe=4, flags=ic.TEST_BATCH)
        assert rc.same(ix.range_search(p[5], radius, where=(zeros, zeros)), plain)      # an all-rows predicate is the plain call
        assert L.lsq_index_range_search_labelled(ix._h, ptr(lims), ptr(p[5]), None, ptr(radius), ptr(zeros), ptr(zeros), 0, tl.D, 0, 0, 0, 0) == 0 and lims[0] == 0
        assert tuple(a.shape[0] for a in ix.range_search(p[5][:0], radius[:0], where=(zeros[:0], zeros[:0]))) == (1, 0, 0)
        with pytest.raises(ValueError):
            ix.range_search(p[5], radius, any_of=True)
