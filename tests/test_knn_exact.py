"""Exact k-NN on the host cores (lsq_knn_exact_cpu): the ground truth of a recall figure.  Bit for bit against the numpy restatement of the contract
(tests/knn_check.py) and against the PQ host scan run with one sub-space of width d; tie and NaN order; the argument rules; the reference-shaped
wrapper; and the float64 top-k check that makes the f32 answer the true k-NN up to rounding.  Host code: runs without a GPU."""
import numpy as np
import pytest

import f64ref as R
import knn_check as KC


def _case(seed, n, nq, d, ldb=None, ldq=None):
    """row arrays (n, ldb) / (nq, ldq), the floats past d filled with junk the search must not read"""
    rng = np.random.default_rng(seed)
    Xb = rng.standard_normal((n, ldb or d)).astype(np.float32)
    Xq = rng.standard_normal((nq, ldq or d)).astype(np.float32)
    Xb[:, d:] = np.nan
    Xq[:, d:] = np.inf
    return Xb, Xq


@pytest.mark.parametrize("d", [1, 2, 3, 5, 128, 129, 1000])
@pytest.mark.parametrize("nn_kind", ["one", "all"])
@pytest.mark.parametrize("strided", [False, True])
def test_cpu_matches_numpy(lsq, d, nn_kind, strided):
    n, nq = 301, 7
    nn = 1 if nn_kind == "one" else n
    Xb, Xq = _case(d * 7 + (nn == 1) + 2 * strided, n, nq, d, d + 3 if strided else d, d + 5 if strided else d)
    rc, dists, ids = KC.knn_cpu(lsq._lib.load(), Xb, Xq, d, nn)
    assert rc == 0, lsq._lib.load().lsq_last_error()
    rd, ri = KC.knn_np(Xb[:, :d], Xq[:, :d], nn)
    assert np.array_equal(ids, ri)
    assert KC.same_bits(dists, rd)


def test_thread_count_does_not_change_the_bits(lsq):
    Xb, Xq = _case(3, 2000, 37, 24)
    L = lsq._lib.load()
    _, d1, i1 = KC.knn_cpu(L, Xb, Xq, 24, 50, nthreads=1)
    for nt in (0, 3, 64):
        _, d2, i2 = KC.knn_cpu(L, Xb, Xq, 24, 50, nthreads=nt)
        assert np.array_equal(i1, i2) and KC.same_bits(d1, d2)


@pytest.mark.parametrize("d", [1, 3, 16, 128, 129])
def test_matches_pq_host_scan_with_one_subspace(lsq, d):
    """n = 256: the PQ host scan with B = 8, subdim = d, the base rows as the 256 centres and codes 0..255 computes the same distances."""
    n, nq, nn = 256, 9, 40
    Xb, Xq = _case(100 + d, n, nq, d)
    L = lsq._lib.load()
    rc, dists, ids = KC.knn_cpu(L, Xb, Xq, d, nn)
    assert rc == 0
    codes = np.arange(n, dtype=np.uint8).reshape(n, 1)
    pd = np.zeros((nq, nn), dtype=np.float32)
    pi = np.zeros((nq, nn), dtype=np.uint32)
    centers = np.ascontiguousarray(Xb[:, :d])
    Q = np.ascontiguousarray(Xq[:, :d])
    assert L.lsq_linscan_aqd_query(pd.ctypes.data, pi.ctypes.data, codes.ctypes.data, centers.ctypes.data, Q.ctypes.data, n, nq, 8, nn, 1, d, d) == 0
    assert np.array_equal(ids, pi) and KC.same_bits(dists, pd)


def test_ties_go_to_the_smaller_id(lsq):
    L = lsq._lib.load()
    rng = np.random.default_rng(5)
    half = rng.integers(-4, 5, size=(500, 6)).astype(np.float32)
    Xb = np.concatenate([half, half, half[:100]])                  # duplicated rows: equal distances
    Xq = rng.integers(-4, 5, size=(11, 6)).astype(np.float32)
    for nn in (1, 37, Xb.shape[0]):
        rc, dists, ids = KC.knn_cpu(L, Xb, Xq, 6, nn)
        rd, ri = KC.knn_np(Xb, Xq, nn)
        assert rc == 0 and np.array_equal(ids, ri) and KC.same_bits(dists, rd)
        for q in range(Xq.shape[0]):                               # non-decreasing (dist, id) pairs
            pairs = list(zip(dists[q].tolist(), ids[q].tolist()))
            assert pairs == sorted(pairs)
    same = np.full((300, 4), 2.5, dtype=np.float32)                # an all-equal base: ids 0 .. nn - 1
    rc, dists, ids = KC.knn_cpu(L, same, Xq[:, :4], 4, 120)
    assert rc == 0 and all(np.array_equal(ids[q], np.arange(120)) for q in range(Xq.shape[0]))


def test_inf_and_nan_rows_sort_last(lsq):
    L = lsq._lib.load()
    rng = np.random.default_rng(9)
    Xb = rng.standard_normal((200, 5)).astype(np.float32)
    Xb[[3, 50]] = np.nan                                           # NaN distances: after everything
    Xb[[7, 120], 2] = np.inf                                       # +inf distances: after every finite one, before NaN
    Xb[9, 0] = -np.inf
    Xq = rng.standard_normal((4, 5)).astype(np.float32)
    rc, dists, ids = KC.knn_cpu(L, Xb, Xq, 5, 200)
    rd, ri = KC.knn_np(Xb, Xq, 200)
    assert rc == 0 and np.array_equal(ids, ri) and KC.same_bits(dists, rd)
    for q in range(4):
        assert ids[q, -2:].tolist() == [3, 50] and np.isnan(dists[q, -2:]).all()
        assert ids[q, -5:-2].tolist() == [7, 9, 120] and np.isinf(dists[q, -5:-2]).all()
        assert np.isfinite(dists[q, :-5]).all()


def test_argument_rules(lsq):
    L = lsq._lib.load()
    EINVAL = -1
    Xb, Xq = _case(1, 50, 3, 8)
    buf_d = np.zeros((3, 50), np.float32)
    buf_i = np.zeros((3, 50), np.uint32)
    p = (buf_d.ctypes.data, buf_i.ctypes.data, Xb.ctypes.data, Xq.ctypes.data)

    def call(n=50, nq=3, d=8, ldb=8, ldq=8, nn=5, ptrs=p):
        return L.lsq_knn_exact_cpu(*ptrs, n, nq, d, ldb, ldq, nn, 0)

    assert call() == 0
    for kw in (dict(d=0), dict(ldb=7), dict(ldq=7), dict(nn=0), dict(nn=51), dict(nq=0), dict(nq=-1), dict(n=4)):
        assert call(**kw) == EINVAL, kw
    for j in range(4):
        ptrs = list(p)
        ptrs[j] = None
        assert call(ptrs=tuple(ptrs)) == EINVAL
    assert L.lsq_knn_exact(None, *p, 50, 3, 8, 8, 8, 5) == EINVAL       # null context
    assert L.lsq_knn_exact_dev(None, *p, 50, 3, 8, 8, 8, 5) == EINVAL


def test_reference_wrapper_is_one_based_and_feeds_eval_recall(lsq):
    rng = np.random.default_rng(4)
    d, n, nq, k = 12, 800, 25, 10
    X_base = rng.standard_normal((d, n)).astype(np.float32)        # Julia shapes: d x n, d x nq
    X_query = X_base[:, rng.choice(n, nq, replace=False)] + np.float32(1e-3) * rng.standard_normal((d, nq)).astype(np.float32)
    dists, ids = lsq.knn_exact(X_base, X_query, k, nthreads=2)
    assert dists.shape == (k, nq) and ids.shape == (k, nq) and ids.dtype == np.uint32
    rd, ri = KC.knn_np(X_base.T, X_query.T, k)
    assert np.array_equal(ids, ri.T + 1) and KC.same_bits(dists, rd.T)
    assert ids.min() >= 1 and ids.max() <= n
    rec = lsq.eval_recall(ids[0, :], ids, k)                       # the ground truth against itself: recall 1 at rank 1
    assert rec[0] == 1.0


@pytest.mark.parametrize("d,k", [(1, 5), (7, 1), (128, 50), (129, 300)])
def test_f32_ground_truth_is_the_true_knn_up_to_rounding(lsq, d, k):
    """float64 distances of the f32 inputs with the gamma_{d+2} bound of their f32 evaluation: R.check_topk accepts the selection."""
    Xb, Xq = _case(40 + d, 1500, 6, d)
    rc, dists, ids = KC.knn_cpu(lsq._lib.load(), Xb, Xq, d, k)
    assert rc == 0
    diff = Xb.astype(np.float64)[None, :, :] - Xq.astype(np.float64)[:, None, :]
    vals = (diff * diff).sum(2)
    R.check_topk(ids, dists, vals, R.gamma(d + 2) * vals, "exact k-NN d=%d k=%d" % (d, k))
