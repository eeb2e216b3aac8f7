"""The model of the search selection (tests/select_model.py) against the numbers the project states, the host scans on non-finite distances against the
model's `select`, and the proof that the inputs of tests/test_gpu_select_model.py can tell a wrong selection from a right one: every entry of
select_model.MUTANTS predicts other statistics than the model on at least one of them.  Host code: runs without a GPU."""
import numpy as np
import pytest

import knn_check as KC
import select_cases as SC
import select_model as SM
from test_linscan import _ours
from test_linscan_pq import drop_in


# ---- plan ---------------------------------------------------------------------------------------------------------------------------------------------
def test_plan_reproduces_the_stated_numbers():
    """csrc/lsq_adc.hip on make_plan: 'ks = 16.4, r = 45' at n = 10^6, nn = 1000, and a list of ~2.7 nn entries on average.  The stated r is the
    formula's real value (45.05); the plan's integer rank is its ceiling, 46"""
    P = SM.plan(10 ** 6, 1000)
    ks = 1000 * 16384 / 10 ** 6
    r = ks + 5.6 * ks ** 0.5 + 6
    assert round(ks, 1) == 16.4 and round(r) == 45 and 45 < r < 45.1
    assert (P["exhaustive"], P["ns"], P["stride"], P["r"]) == (False, 16384, 61, 46)
    assert 2.7 <= r * (10 ** 6 / 16384) / 1000 < 2.8
    cap = (r + 8 * r ** 0.5 + 32) * (10 ** 6 / 16384) + 1000                # rounded up to a multiple of 64
    assert P["cap"] % 64 == 0 and 0 <= P["cap"] - int(cap) < 64


def test_plan_exhaustive_cut_offs():
    assert SM.plan(65536, 10)["exhaustive"] and SM.plan(65536, 10)["cap"] == 65536 and SM.plan(65536, 10)["r"] == 0
    P = SM.plan(65537, 10)
    assert not P["exhaustive"] and P["stride"] == 4 and P["ns"] == 16384
    assert SM.plan(65537, 10, force_exhaustive=1)["exhaustive"]
    # the two exits.  cap / n = (r + 8 sqrt(r) + 32) / ns + nn / n grows with nn / n and passes 0.5 near ks = 3660, where r = 4005 < 0.25 ns = 4096:
    # the capacity exit is the one that binds, and every nn with r >= 0.25 ns lies beyond it
    for n in (70_001, 10 ** 6, 10 ** 7):
        edge = [nn for nn in range(1, n, max(1, n // 20000)) if SM.plan(n, nn)["exhaustive"]][0]
        for nn, exhaustive in ((edge - max(1, n // 20000), False), (edge, True)):
            ks = nn * 16384 / n
            r = ks + 5.6 * ks ** 0.5 + 6
            assert ((r + 8 * r ** 0.5 + 32) * (n / 16384) + nn >= 0.5 * n) == exhaustive and r < 0.25 * 16384
            assert SM.plan(n, nn)["exhaustive"] == exhaustive
        assert 3600 < edge * 16384 / n < 3700
        nn = int(3752 * n / 16384) + 1                          # r >= 0.25 ns from here on
        assert nn * 16384 / n + 5.6 * (nn * 16384 / n) ** 0.5 + 6 >= 0.25 * 16384 and SM.plan(n, nn)["exhaustive"] and SM.plan(n, n)["exhaustive"]


def test_plan_rank_override():
    base = SM.plan(98304, 50)
    assert base["r"] == 31 and base["cap"] == 704 and base["stride"] == 6
    for rank, want in ((1, 1), (255, 255), (16384, 16384), (20000, 16384)):
        P = SM.plan(98304, 50, rank=rank)
        assert P["r"] == want and P["cap"] == base["cap"] and not P["exhaustive"]
    assert SM.plan(60000, 50, rank=7) == SM.plan(60000, 50)                 # the exhaustive road ignores the hook
    assert SM.plan(98304, 50, force_exhaustive=1, rank=7)["r"] == 0


def test_batches():
    P = SM.plan(65537, 3, rank=1)
    assert SM.batches(P, 65537, 4100, 4100) == 3 and SM.batches(P, 65537, 4100, 4080) == 2 and SM.batches(P, 65537, 4100, 0) == 1
    assert SM.batches(SM.plan(70000, 3), 70000, 20000, 0) == 2               # 16 384 queries per thresholded batch at most
    assert SM.batches(SM.plan(60000, 5), 60000, 4500, 0) == 2               # (2^28 // 60 000) & ~15 = 4464 per exhaustive batch


def test_keys_round_trip_and_predict_on_a_worked_example():
    v = np.array([-np.inf, -1.5, -0.0, 0.0, 1e-45, 2.0, np.inf, np.nan], dtype=np.float32)
    k = KC.order_keys(v)
    assert np.all(np.diff(k.astype(np.int64)) > 0) and k[-1] == 0xFFFFFFFF
    assert np.array_equal(SM.unkey(k).view(np.uint32), np.where(np.isnan(v), np.float32(np.nan), v).view(np.uint32))
    # n = 131 074: stride 8, the sample is entries 0, 8, ...  Query 0: distance = the entry's index, so tau = 8 (r - 1) and count = 8 (r - 1) + 1.
    # Query 1: the same backwards; the sample's smallest is entry 8 * 16383 at distance 9.  Query 2: all equal -- every entry ties with tau: overflow
    n = 131074
    D = np.arange(n, dtype=np.float32)[None, :].repeat(3, axis=0)
    D[1] = D[1, ::-1]
    D[2] = 7.0
    out = SM.predict(D, 10)
    r, cap = out["plan"]["r"], out["plan"]["cap"]
    assert np.array_equal(SM.unkey(out["tau"]), np.float32([8 * (r - 1), 9 + 8 * (r - 1), 7]))
    assert np.array_equal(out["count"], [8 * (r - 1) + 1, 10 + 8 * (r - 1), n])
    assert np.array_equal(out["failed"], [False, False, True]) and out["count"][1] <= cap < n
    assert out["stats"]["fallback_queries"] == 1 and out["stats"]["candidates"] == int(out["count"].sum()) + n and out["stats"]["batches"] == 2
    d, i = SM.select(D, 3, id_base=1)
    assert np.array_equal(i, [[1, 2, 3], [n, n - 1, n - 2], [1, 2, 3]]) and np.array_equal(d, [[0, 1, 2], [0, 1, 2], [7, 7, 7]])
    short = SM.predict(D[:1], 8 * (r - 1) + 2)                               # one neighbour more than the list holds: too short
    assert short["plan"]["r"] >= r and SM.predict(D[:1], 10, rank=1)["failed"].all() and SM.predict(D[:1], 1, rank=1)["count"][0] == 1


# ---- the host scans on non-finite distances -------------------------------------------------------------------------------------------------------------
def _same(d, i, dref, iref):
    assert np.array_equal(np.asarray(i).astype(np.int64), iref), "ids differ at %s" % (np.argwhere(np.asarray(i).astype(np.int64) != iref)[:5].tolist(),)
    assert KC.same_bits(d, dref), "distances differ"


@pytest.mark.parametrize("nn", SC.NONFINITE_NN[SC.NONFINITE_SMALL])
def test_host_lsq_scan_on_non_finite_norms(lsq, nn):
    """ties by id, Inf after finite, NaN last: lsq_linscan_aqd_query_extra_byte against `select` on the numpy loop's distances"""
    codes, Q, K, dbnorms, m = SC.nonfinite_lsq(SC.NONFINITE_SMALL)
    D = SM.lsq_dists_np(codes, Q, K, dbnorms, m)
    assert np.isnan(D).any() and np.isposinf(D).any() and np.isneginf(D).any() and not np.signbit(D[D == 0]).any()
    assert (np.sort(D, axis=1)[:, 1:] == np.sort(D, axis=1)[:, :-1]).any()                                   # ties
    for nt in (1, 3):
        _same(*_ours(lsq, codes, Q, K, dbnorms, m, nn, nthreads=nt), *SM.select(D, nn, id_base=1))


@pytest.mark.parametrize("nn", SC.NONFINITE_NN[SC.NONFINITE_SMALL])
def test_host_pq_scan_on_non_finite_tables(lsq, nn):
    codes, centers, Q, m, subdim = SC.nonfinite_pq(SC.NONFINITE_SMALL)
    D = _pq_dists_np(codes, centers, Q, m, subdim)
    assert np.isnan(D).any() and np.isposinf(D).any() and np.isfinite(D).any()
    _same(*drop_in(lsq, codes, centers, Q, m, subdim, nn), *SM.select(D, nn, id_base=0))


def _pq_dists_np(codes, centers, Q, m, subdim):
    """tests/test_linscan_pq.py's pq_checker up to the distances (its lexsort has no place for NaN)"""
    n, nq = codes.shape[0], Q.shape[0]
    qs = Q[:, : m * subdim].reshape(nq, m, subdim)
    with np.errstate(invalid="ignore", over="ignore"):
        tab = np.zeros((nq, m, SM.H), np.float32)
        for s in range(subdim):
            e = centers[None, :m, :, s] - qs[:, :, None, s]
            tab = tab + e * e
        dist = np.zeros((nq, n), np.float32)
        for k in range(m):
            dist = dist + tab[:, k, codes[:, k]]
    return dist


def test_full_matrices_are_the_numpy_loops(lsq):
    """the host forms with nn = n, scattered back by id, against numpy loops in the contract's op order -- for each producer, at a small n"""
    lib = lsq._lib.load()
    codes, Q, K, dbnorms, m = SC.nonfinite_lsq(SC.NONFINITE_SMALL)
    assert np.array_equal(KC.order_keys(SM.full_matrix_lsq(lib, codes, Q, K, dbnorms, m)), KC.order_keys(SM.lsq_dists_np(codes, Q, K, dbnorms, m)))
    codes, centers, Q, m, subdim = SC.nonfinite_pq(SC.NONFINITE_SMALL)
    assert np.array_equal(KC.order_keys(SM.full_matrix_pq(lib, codes, centers, Q, m, subdim)), KC.order_keys(_pq_dists_np(codes, centers, Q, m, subdim)))
    rng = np.random.default_rng(1)
    Xb, Xq = rng.integers(0, 256, (500, 7), dtype=np.uint8), rng.integers(0, 256, (4, 7), dtype=np.uint8)
    want = KC.knn_dists(Xb.astype(np.float32), Xq.astype(np.float32))
    assert KC.same_bits(SM.full_matrix_exact_u8(lib, Xb, Xq), want) and KC.same_bits(SM.full_matrix_exact(lib, Xb.astype(np.float32), Xq.astype(np.float32)), want)
    case = SC.many_failed()
    assert KC.same_bits(SC.many_failed_rows(case, 5, 8), SM.full_matrix_lsq(lib, case.inputs[0], case.inputs[1][5:8], *case.inputs[2:]))


# ---- the GPU file's inputs: what the model says of them, and that they can tell a wrong selection from a right one ---------------------------------------
def test_mixed_cases_have_failed_and_served_queries(lsq):
    lib = lsq._lib.load()
    for p in ("lsq", "pq", "exact", "u8"):
        case = SC.mixed(p)
        out = SM.predict(SC.matrix(lib, case), case.nn)
        assert not out["plan"]["exhaustive"] and 0 < out["failed"].sum() < case.nq, (p, out["failed"])
        assert (out["count"][out["failed"]] > out["plan"]["cap"]).all(), (p, out["count"])          # overflowed, not short


def test_many_failed_case_fills_three_batches(lsq):
    case = SC.many_failed()
    P, tau, count, failed, (top_d, top_i) = SC.many_failed_model(lsq._lib.load(), case)
    assert failed.all() and failed.size == 4100 and (2 ** 28 // case.n) & ~15 == 4080
    st = SM.totals(P, case.n, case.nq, count, failed)
    assert st["batches"] == 3 and st["fallback_queries"] == 4100 and st["candidates"] == int(count.sum()) + 4100 * case.n
    # the short cut against the model proper on the matrix's first rows
    D = SC.many_failed_rows(case, 0, 64)
    t, c, f = SM.predict_rows(D, case.nn, P)
    assert KC.same_bits(SM.unkey(t), tau[:64]) and np.array_equal(c, count[:64]) and np.array_equal(f, failed[:64])
    d, i = SM.select(D, case.nn, id_base=1)
    assert KC.same_bits(d, top_d[:64]) and np.array_equal(i, top_i[:64])


def test_every_mutant_disagrees_on_the_gpu_inputs(lsq):
    lib = lsq._lib.load()
    caught = {name: [] for name, _ in SM.MUTANTS}
    for case, ranks in SC.every_case():
        D = SC.matrix(lib, case)
        for rank in ranks:
            args = case.plan_args(rank)
            st = SM.predict(D, case.nn, **args)["stats"]
            true = (st["fallback_queries"], st["candidates"])
            for name, slip in SM.MUTANTS:
                if SM.mutant_stats(D, case.nn, slip, **args) != true:
                    caught[name].append((case.name, rank))
    case = SC.many_failed()
    D = SC.many_failed_rows(case, 0, 256)                   # the first rows of the 4100: each mutant on the same rows as the model
    true = SM.mutant_stats(D, case.nn, None, rank=1)
    for name, slip in SM.MUTANTS:
        if SM.mutant_stats(D, case.nn, slip, rank=1) != true:
            caught[name].append((case.name, 1))
    for name, where in caught.items():
        print("%-24s differs on %3d (case, rank) pairs, e.g. %s" % (name, len(where), where[:3]))
    assert all(caught.values()), {k: len(v) for k, v in caught.items()}
