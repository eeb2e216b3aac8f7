"""The reference's other scan: linscan_aqd_query (src/linscan/cpp/linscan_aqd.cpp:37-114) for PQ / OPQ codes, bound by linscan_pq / linscan_opq
(src/linscan/Linscan.jl:5-43).  lsq_linscan_aqd_query must return what the reference's build returns -- distances as bits, 0-based ids, tie order --
on the stored outputs of tests/golden/linscan_pq/reference_outputs.npz (tests/golden/make_linscan_pq_golden.py), and what the numpy restatement
below returns on seeded random shapes.  Host code: runs without a GPU."""
import hashlib
import os

import numpy as np
import pytest

H = 256
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linscan_pq", "reference_outputs.npz")

# name -> (n, nq, m, subdim, dim1codes, dim1queries, K, kind).  kind: "normal" (Gaussian data), "dup" (the second half of the database repeats the
# first: equal distances, ties by id), "int" (integer-valued centres and queries, 4 distinct code values: massive ties)
FIXTURE_CASES = {
    "m8_s16": (5000, 20, 8, 16, 8, 128, 100, "normal"),
    "m4_s3_strided": (3000, 13, 4, 3, 6, 17, 50, "normal"),           # dim1codes > m, dim1queries > m * subdim
    "m16_s8_int_ties": (2000, 10, 16, 8, 16, 128, 200, "int"),
    "m8_s120": (20000, 6, 8, 120, 8, 960, 1000, "normal"),
    "m7_s1_dup_k_eq_n": (1500, 9, 7, 1, 7, 7, 1500, "dup"),           # subdim 1, m not a multiple of 4, K = N
    "m3_s5_dup_strided": (4000, 11, 3, 5, 5, 17, 64, "dup"),
    "m12_s4": (2500, 7, 12, 4, 12, 48, 33, "normal"),
    "m1_s32": (1000, 5, 1, 32, 1, 32, 20, "normal"),
}


def pq_case(seed, n, nq, m, subdim, dim1codes, dim1queries, kind="normal"):
    """-> codes (n, dim1codes) u8, centers (m, 256, subdim) f32, queries (nq, dim1queries) f32; the bytes / floats beyond m and m * subdim are
    filled too (the scan must not read them)"""
    rng = np.random.default_rng(seed)
    if kind == "int":
        centers = rng.integers(-3, 4, size=(m, H, subdim)).astype(np.float32)
        Q = rng.integers(-3, 4, size=(nq, dim1queries)).astype(np.float32)
        codes = rng.integers(0, 4, size=(n, dim1codes), dtype=np.uint8)
    else:
        centers = rng.standard_normal((m, H, subdim)).astype(np.float32)
        Q = rng.standard_normal((nq, dim1queries)).astype(np.float32)
        codes = rng.integers(0, H, size=(n, dim1codes), dtype=np.uint8)
    if kind == "dup":
        codes[n // 2:] = codes[: n - n // 2]
    return codes, centers, Q


def fixture_inputs(name):
    n, nq, m, subdim, dc, dq, K, kind = FIXTURE_CASES[name]
    return pq_case(sum(map(ord, name)), n, nq, m, subdim, dc, dq, kind)


def inputs_digest(codes, centers, Q):
    h = hashlib.sha256()
    for a in (codes, centers, Q):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def reference_outputs(name):
    """the reference build's outputs on the fixture case -> dists (nq, K) f32, ids (nq, K) uint32 0-based"""
    codes, centers, Q = fixture_inputs(name)
    z = np.load(GOLDEN)
    assert str(z[name + "_inputs"]) == inputs_digest(codes, centers, Q), "the seeded inputs of %s are not those the fixture was made from" % name
    return z[name + "_dists"], z[name + "_res"]


def pq_checker(codes, centers, Q, m, subdim, K):
    """bit-exact numpy restatement of linscan_aqd.cpp: f32 tables (s ascending, no FMA), f32 sums (k ascending), (dist, id) lexicographic"""
    n, nq = codes.shape[0], Q.shape[0]
    qs = Q[:, : m * subdim].reshape(nq, m, subdim)
    tab = np.zeros((nq, m, H), np.float32)
    for s in range(subdim):
        e = centers[None, :m, :, s] - qs[:, :, None, s]
        tab = tab + e * e
    dist = np.zeros((nq, n), np.float32)
    for k in range(m):
        dist = dist + tab[:, k, codes[:, k]]
    ids = np.arange(n, dtype=np.uint32)
    order = np.stack([np.lexsort((ids, dist[q]))[:K] for q in range(nq)])
    return np.take_along_axis(dist, order, 1), order.astype(np.uint32)


def drop_in(lsq, codes, centers, Q, m, subdim, K, B=None):
    L = lsq._lib.load()
    nq = Q.shape[0]
    dists = np.zeros((nq, K), np.float32)
    res = np.zeros((nq, K), np.uint32)
    lsq._lib.check(L.lsq_linscan_aqd_query(dists.ctypes.data, res.ctypes.data, codes.ctypes.data, centers.ctypes.data, Q.ctypes.data,
                                           codes.shape[0], nq, 8 * m if B is None else B, K, codes.shape[1], Q.shape[1], subdim))
    return dists, res


def assert_same(d, i, dref, iref):
    assert np.array_equal(i, iref), "%d of %d ids differ" % ((i != iref).sum(), i.size)
    assert np.array_equal(d.view(np.uint32), dref.view(np.uint32)), "max |diff| %g" % np.abs(d - dref).max()


@pytest.mark.parametrize("name", sorted(FIXTURE_CASES))
def test_matches_reference_outputs(lsq, name):
    n, nq, m, subdim, dc, dq, K, kind = FIXTURE_CASES[name]
    codes, centers, Q = fixture_inputs(name)
    dref, iref = reference_outputs(name)
    assert dref.shape == (nq, K) and iref.dtype == np.uint32
    d, i = drop_in(lsq, codes, centers, Q, m, subdim, K)
    assert_same(d, i, dref, iref)
    assert_same(*pq_checker(codes, centers, Q, m, subdim, K), dref, iref)        # the checker is the contract, too


@pytest.mark.parametrize("seed", range(8))
def test_matches_numpy_checker(lsq, seed):
    rng = np.random.default_rng(500 + seed)
    m = int(rng.integers(1, 17))
    subdim = int(rng.choice([1, 2, 3, 4, 7, 16, 33]))
    n = int(rng.integers(1, 6000))
    nq = int(rng.integers(1, 12))
    K = int(rng.integers(1, n + 1))
    dc, dq = m + int(rng.integers(0, 3)), m * subdim + int(rng.integers(0, 5))
    codes, centers, Q = pq_case(seed, n, nq, m, subdim, dc, dq, ["normal", "dup", "int"][seed % 3])
    assert_same(*drop_in(lsq, codes, centers, Q, m, subdim, K), *pq_checker(codes, centers, Q, m, subdim, K))


def test_bad_arguments(lsq):
    L = lsq._lib.load()
    codes, centers, Q = pq_case(1, 10, 2, 2, 3, 2, 6)
    d = np.zeros((2, 10), np.float32)
    r = np.zeros((2, 10), np.uint32)
    p = [d.ctypes.data, r.ctypes.data, codes.ctypes.data, centers.ctypes.data, Q.ctypes.data]

    def call(N=10, NQ=2, B=16, K=5, dc=2, dq=6, subdim=3, ptrs=p):
        return L.lsq_linscan_aqd_query(*ptrs, N, NQ, B, K, dc, dq, subdim)

    assert call() == 0
    bad = [dict(B=12), dict(B=0), dict(B=-8), dict(dc=1), dict(B=24, dc=2), dict(subdim=0), dict(dq=5), dict(K=0), dict(K=11), dict(N=0, K=1)]
    for i in range(5):
        ptrs = list(p)
        ptrs[i] = None
        bad.append(dict(ptrs=ptrs))
    for kw in bad:
        assert call(**kw) == lsq._lib.LSQ_EINVAL, kw
        assert L.lsq_last_error(), kw
    assert call(NQ=0, ptrs=[None] * 5) == 0                          # no queries: nothing to do


def test_reference_shaped_linscan_pq_and_opq(lsq):
    n, nq, m, subdim, K = 3000, 9, 4, 6, 40
    d = m * subdim
    codes, centers, Q = pq_case(77, n, nq, m, subdim, m, d)
    B, X = codes.T, Q.T                                              # Julia shapes: B (m, n), X (d, nq)
    C = [np.ascontiguousarray(centers[k].T) for k in range(m)]       # (subdim, h) each
    dists, res = lsq.linscan_pq(B, X, C, 8 * m, K)
    assert dists.shape == (K, nq) and res.shape == (K, nq) and dists.dtype == np.float32 and res.dtype == np.uint32
    dref, iref = drop_in(lsq, codes, centers, Q, m, subdim, K)
    assert np.array_equal(res.T, iref + 1) and res.min() >= 1 and res.max() <= n      # 1-based, as Linscan.jl returns them
    assert np.array_equal(dists.T.view(np.uint32), dref.view(np.uint32))
    R = np.linalg.qr(np.random.default_rng(3).standard_normal((d, d)))[0].astype(np.float32)
    do, ro = lsq.linscan_opq(B, X, C, 8 * m, R, K)
    dp, rp = lsq.linscan_pq(B, R.T @ X, C, 8 * m, K)
    assert np.array_equal(ro, rp) and np.array_equal(do.view(np.uint32), dp.view(np.uint32))
    assert not np.array_equal(ro, res)                               # the rotation did something
    rec = lsq.eval_recall(res[0], res, K)
    assert rec[0] == 1.0


def test_d_not_multiple_of_m_raises(lsq):
    codes, centers, Q = pq_case(2, 100, 3, 4, 2, 4, 10)
    C = [np.ascontiguousarray(centers[k].T) for k in range(4)]
    with pytest.raises(ValueError):
        lsq.linscan_pq(codes.T, Q.T, C, 32, 5)                      # d = 10, m = 4
    with pytest.raises(ValueError):
        lsq.linscan_opq(codes.T, Q.T, C, 32, np.eye(10, dtype=np.float32), 5)
