"""The selection of csrc/lsq_adc.hip held to a model of its own plan (tests/select_model.py), for all four distance producers: every call's RESULTS
equal the model's `select` on the producer's full distance matrix bit for bit, ids included, and its STATISTICS -- exhaustive, threshold_rank,
list_capacity, fallback_queries, candidates, batches -- equal the model's exactly.  The fallback repairs any wrong threshold, so the results alone
cannot see a rank select that returns another order statistic, a scan that drops or doubles pairs at the threshold, or a plan off its formula; the
counts can (tests/test_select_model.py proves it on these very inputs, mutant by mutant).  Index.knn reports no candidates: knn_info()'s
fallback_queries, exhaustive and batches are held instead.

Sizes are the smallest on the thresholded road (n just above 65 536) unless a case says otherwise."""
import numpy as np
import pytest
import torch

import knn_check as KC
import select_cases as SC
import select_model as SM
from test_linscan import _ours
from test_linscan_pq import drop_in

pytestmark = pytest.mark.gpu
STATS = ("exhaustive", "threshold_rank", "list_capacity", "fallback_queries", "candidates", "batches", "queries", "codes")


def _same(d, i, want, what=""):
    dref, iref = want
    i = np.asarray(i)
    i = (i.view(np.uint32) if i.dtype == np.int32 else i).astype(np.int64)
    assert np.array_equal(i, iref), "%s: ids differ at %s" % (what, np.argwhere(i != iref)[:5].tolist())
    assert KC.same_bits(d, dref), "%s: distances differ" % (what,)


def _hold(st, want, what=""):
    print("%s: %s" % (what, {k: st[k] for k in STATS}))
    for k in STATS:
        assert st[k] == want[k], (what, k, st[k], want[k], {j: st[j] for j in STATS}, want)


def _call(eng, case, dev=False):
    """one search of the case through its producer's Engine entry point -> dists, ids (numpy)"""
    t = (lambda a: torch.tensor(a).cuda()) if dev else (lambda a: a)
    if case.producer == "lsq":
        codes, Q, K, dbnorms, m = case.inputs
        d, i = (eng.linscan_dev if dev else eng.linscan)(t(codes), t(Q), t(K), t(dbnorms), m, case.nn)
    elif case.producer == "pq":
        codes, centers, Q, m, subdim = case.inputs
        d, i = (eng.linscan_pq_dev if dev else eng.linscan_pq)(t(codes), t(Q), t(centers), m, case.nn, subdim)
    else:
        Xb, Xq = case.inputs
        d, i = (eng.knn_exact_dev if dev else eng.knn_exact)(t(Xb), t(Xq), case.nn)
    if dev:
        torch.cuda.synchronize()
        d, i = d.cpu().numpy(), i.cpu().numpy()
    return d, i


def _search(eng, case, want, model, rank=0, dev=False, what=""):
    """one call under option linscan_rank: its results against `want`, its statistics (this call's alone) against the model's"""
    eng.set_option("linscan_rank", rank)
    eng.reset_timings()
    d, i = _call(eng, case, dev)
    st = eng.linscan_stats()
    _same(d, i, want, what)
    _hold(st, model["stats"], what)


# ---- a. crafted key distributions: the rank select and the compare-and-append away from random normal data ---------------------------------------------
@pytest.mark.parametrize("m", SC.CRAFTED_M)
@pytest.mark.parametrize("name", SC.DISTRIBUTION_NAMES)
def test_crafted_key_distributions(lsq, name, m):
    """zero codebooks: dist(i) == dbnorms[i], so the norms ARE the keys the selection sees.  n = 98 304 (stride 6), 5 queries (one ragged tile), nn = 50;
    the plan's own rank, then every rank around the radix select's digit edges, the middle, the sample's last key and past it (clamped)"""
    case = SC.crafted(name, m)
    D = SC.matrix(lsq._lib.load(), case)
    assert np.array_equal(KC.order_keys(D), KC.order_keys(np.broadcast_to(case.inputs[3] + np.float32(0), D.shape)))      # -0.0 -> +0.0, the rest as they are
    want = SM.select(D, case.nn, case.id_base)
    with lsq.Engine(0) as eng:
        for rank in SC.RANKS:
            model = SM.predict(D, case.nn, **case.plan_args(rank))
            assert not model["plan"]["exhaustive"] and model["plan"]["r"] == (min(rank, 16384) if rank else 31)
            _search(eng, case, want, model, rank, what="%s rank %d" % (case.name, rank))


# ---- b. mixed batches: failed and served queries side by side ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("producer", ["lsq", "pq", "exact"])
def test_mixed_fallbacks(lsq, producer):
    """a run of identical entries: the queries pulled towards it see more ties at their threshold than a list holds and are redone through `qsel` --
    non-contiguous ids, a ragged last tile -- while their neighbours are served by their lists; twice on one engine (the lists fill in atomic order)"""
    case = SC.mixed(producer)
    D = SC.matrix(lsq._lib.load(), case)
    model = SM.predict(D, case.nn)
    assert not model["plan"]["exhaustive"] and 0 < model["failed"].sum() < case.nq, model["failed"]
    want = SM.select(D, case.nn, case.id_base)
    with lsq.Engine(0) as eng:
        for run in range(2):
            _search(eng, case, want, model, what="%s run %d" % (case.name, run))
        _search(eng, case, want, model, dev=True, what="%s device tensors" % case.name)


def test_mixed_fallbacks_index_knn_on_a_uint8_base(lsq):
    """the same through Index.knn on un-widened rows, integer road (knn_u8_int 1) and widened road (0); knn_info reports no candidates"""
    case = SC.mixed("u8")
    Xb, Xq = case.inputs
    D = SC.matrix(lsq._lib.load(), case)
    model = SM.predict(D, case.nn)
    assert not model["plan"]["exhaustive"] and 0 < model["failed"].sum() < case.nq, model["failed"]
    want = SM.select(D, case.nn, 0)
    with lsq.Engine(0) as eng, eng.index(None, None, None, 0, base=Xb) as ix:
        for int_road in (1, 0):
            eng.set_option("knn_u8_int", int_road)
            for run in range(2):
                d, i = ix.knn(Xq, case.nn)
                info = ix.knn_info()
                print("int_road %d run %d: %s" % (int_road, run, info))
                _same(d, i, want, "int_road %d run %d" % (int_road, run))
                assert info["int_road"] == int_road and info["queries"] == case.nq and info["rows"] == case.n, info
                for k in ("fallback_queries", "exhaustive", "batches"):
                    assert info[k] == model["stats"][k], (k, info, model["stats"])


# ---- c. more failed queries than one fallback batch ------------------------------------------------------------------------------------------------------
def test_more_failed_queries_than_one_fallback_batch(lsq):
    """n = 65 537, 4100 queries, linscan_rank = 1: every list holds the one pair at the sample's minimum, all 4100 are redone -- 4080 in the first fallback
    batch, 20 in the second, which reads qsel + 4080"""
    case = SC.many_failed()
    P, tau, count, failed, want = SC.many_failed_model(lsq._lib.load(), case)
    stats = SM.totals(P, case.n, case.nq, count, failed)
    assert failed.all() and stats["fallback_queries"] == 4100 and stats["batches"] == 3
    with lsq.Engine(0) as eng:
        _search(eng, case, want, dict(stats=stats), rank=1, what=case.name)


# ---- d. non-finite distances on the device --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("producer", ["lsq", "pq"])
@pytest.mark.parametrize("n", [SC.NONFINITE_SMALL, SC.NONFINITE_LARGE])
def test_non_finite_distances(lsq, producer, n):
    """NaN, +-Inf (and -0.0 among the LSQ norms): ties by id, Inf after finite, NaN last and as one NaN -- on the exhaustive road (n = 300) and on the
    thresholded one (n = 70 001, where a query whose distances are all Inf or NaN overflows its list), host buffers and device tensors, against
    `select` and against the host scan"""
    lib = lsq._lib.load()
    with lsq.Engine(0) as eng:
        for nn in SC.NONFINITE_NN[n]:
            case = SC.nonfinite(producer, n, nn)
            D = SC.matrix(lib, case)
            assert np.isnan(D).any() and np.isposinf(D).any() and np.isfinite(D).any()
            want = SM.select(D, nn, case.id_base)
            host = _ours(lsq, *case.inputs, nn) if producer == "lsq" else drop_in(lsq, *case.inputs, nn)
            _same(*host, want, "host scan")
            model = SM.predict(D, nn)
            assert model["plan"]["exhaustive"] == (n == SC.NONFINITE_SMALL)
            for dev in (False, True):
                _search(eng, case, want, model, dev=dev, what="%s dev %d" % (case.name, dev))


# ---- e. the rounding boundaries of the records' id field -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lists", "edge"])
@pytest.mark.parametrize("n", SC.IDBITS_N)
def test_id_field_boundaries(lsq, n, kind):
    """n = 2^16 - 1, 2^16 (exhaustive road) and 2^17 - 1, 2^17, 2^17 + 1 (thresholded): the id field of a record is 16 / 17 / 18 bits wide; the last id
    must come back, from a list ("lists": it is every query's nearest) and with the largest finite key above it ("edge": the answer's last pair)"""
    case = SC.idbits(n, kind)
    D = SC.matrix(lsq._lib.load(), case)
    want = SM.select(D, case.nn, 1)
    assert (want[1] == n).any(axis=1).all() and (kind == "lists" or (want[0][:, -1] == SC.FLT_MAX).all() and (want[1][:, -1] == n).all())
    model = SM.predict(D, case.nn)
    assert model["plan"]["exhaustive"] == (n <= 65536)
    if n > 65536:
        assert model["stats"]["fallback_queries"] == (0 if kind == "lists" else case.nq)
    with lsq.Engine(0) as eng:
        _search(eng, case, want, model, what=case.name)
