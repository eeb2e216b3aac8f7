"""CPU tests of the sparse codebook step: the float64 checker (tests/spgl1_check.py) against closed forms and brute force, and the product's
argument rules (ValueError before any device, LSQ_EINVAL / LSQ_ENODEV from the C-ABI)."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spgl1_check as chk  # noqa: E402

H = 256


def _problem(seed, n, d, m, scale=10.0):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, d)) * scale).astype(np.float32)
    codes = rng.integers(0, H, (n, m))
    return chk.Problem(X, codes, m)


def _least_squares(P):
    A = P.dense()
    k, *_ = np.linalg.lstsq(A, P.X.ravel(), rcond=None)
    return k.reshape(P.m * P.h, P.d)


def test_certificate_tau_zero_is_half_b_squared():
    P = _problem(1, 40, 3, 2)
    c = chk.certificate(P, np.zeros((2 * H, 3)), 0.0)
    assert c["f"] == pytest.approx(0.5 * float(np.sum(P.X ** 2)), rel=1e-15)
    assert c["gap"] == pytest.approx(0.0, abs=1e-9 * c["f"])          # K = 0 is the optimum of the tau = 0 problem


def test_certificate_large_tau_gives_least_squares_optimum():
    P = _problem(2, 30, 2, 1)                                           # 30 rows, 256 columns: unused codewords give zero columns
    Kls = _least_squares(P)
    tau = 1.5 * np.abs(Kls).sum()
    fstar = 0.5 * float(np.sum((P.X - P.A(Kls)) ** 2))
    c = chk.certificate(P, Kls, tau)
    assert abs(c["gap"]) <= 1e-9 * max(1.0, float(np.sum(P.X ** 2)))    # A'r = 0 at the least-squares point
    # a feasible non-optimal point: its gap bounds its excess
    K = 0.5 * Kls
    c2 = chk.certificate(P, K, tau)
    assert c2["f"] - fstar <= c2["gap"] * (1 + 1e-12) + 1e-9


def test_certificate_one_column_closed_form():
    # m = 1, every row has code 0: A = ones(n), min 1/2 ||k 1 - b||^2 s.t. |k| <= tau -> k = clip(mean b, -tau, tau)
    rng = np.random.default_rng(3)
    n = 50
    X = (rng.standard_normal((n, 1)) + 3).astype(np.float32)
    P = chk.Problem(X, np.zeros((n, 1), dtype=np.int64), 1)
    mean = float(P.X.mean())
    for tau in (0.0, 0.5 * mean, mean, 2 * mean):
        kstar = np.clip(mean, -tau, tau)
        K = np.zeros((H, 1))
        K[0, 0] = kstar
        fstar = 0.5 * float(np.sum((P.X[:, 0] - kstar) ** 2))
        c = chk.certificate(P, K, tau)
        assert c["f"] == pytest.approx(fstar, rel=1e-14)
        assert abs(c["gap"]) <= 1e-9 * max(1.0, fstar)
        for k in (0.0, 0.3 * kstar, 0.9 * kstar):                       # feasible points: f - f* <= gap
            K[0, 0] = k
            c = chk.certificate(P, K, tau)
            assert c["f"] - fstar <= c["gap"] + 1e-9 * fstar


def test_projection_matches_brute_force_and_kkt():
    rng = np.random.default_rng(4)
    for trial in range(30):
        v = rng.standard_normal(rng.integers(1, 7)) * 3
        if trial % 5 == 0:
            v[0] = v[-1] = 2.0                                          # ties
        tau = float(rng.uniform(0, 1.2) * np.abs(v).sum())
        p = chk.project_l1(v, tau)
        assert np.abs(p).sum() <= tau * (1 + 1e-12) + 1e-15
        # brute force: the projection onto the cross-polytope is the projection onto the closest face; compare with a fine search over theta
        best = None
        for theta in np.concatenate([[0.0], np.abs(v), np.linspace(0, np.abs(v).max(), 2001)]):
            q = np.sign(v) * np.maximum(np.abs(v) - theta, 0)
            if np.abs(q).sum() <= tau * (1 + 1e-12) + 1e-15:
                dist = np.sum((q - v) ** 2)
                best = dist if best is None else min(best, dist)
        assert np.sum((p - v) ** 2) <= best * (1 + 1e-9) + 1e-12
        # KKT: inside -> p = v; on the boundary -> v - p = theta sign(p) on the support, |v - p| <= theta off it
        if np.abs(v).sum() <= tau:
            assert np.array_equal(p, v)
        else:
            assert np.abs(p).sum() == pytest.approx(tau, rel=1e-12, abs=1e-14)
            w = v - p
            sup = p != 0
            if sup.any():
                theta = float(np.abs(w[sup]).max())
                assert np.allclose(w[sup], theta * np.sign(p[sup]), rtol=1e-10, atol=1e-12)
                assert np.all(np.abs(w[~sup]) <= theta * (1 + 1e-10) + 1e-12)


@pytest.mark.parametrize("n,d,m,frac", [(40, 2, 1, 0.3), (60, 3, 2, 0.05), (80, 2, 2, 0.5), (50, 1, 3, 2.0)])
def test_numpy_spg_reaches_tight_gap(n, d, m, frac):
    P = _problem(10 + n, n, d, m)
    Kls = _least_squares(P)
    tau = frac * np.abs(Kls).sum()
    K, info = chk.spg(P, tau, opt_tol=1e-8, max_iter=20000)
    assert info["status"] == chk.OPTIMAL
    assert np.abs(K).sum() <= tau * (1 + 1e-12)
    rnorm_rule = info["rnorm"] < 1e-8 * info["bnorm"]
    assert info["rel_gap"] <= 1e-8 or rnorm_rule
    if frac < 1:                                                        # compare with the dense LASSO optimum: f - f* <= gap
        fls = 0.5 * float(np.sum((P.X - P.A(Kls)) ** 2))
        assert info["f"] >= fls * (1 - 1e-12)


def test_threshold_orders_ties_like_julia():
    K = np.zeros((4, 3), dtype=np.float32)
    K.ravel()[[7, 2, 9, 4, 0]] = [-3.0, 3.0, 1.0, -1.0, 1.0]            # |3| at flat 2 and 7, |1| at flat 0, 4 and 9
    assert np.array_equal(chk.threshold(K, 1).ravel().nonzero()[0], [2])
    assert np.array_equal(chk.threshold(K, 2).ravel().nonzero()[0], [2, 7])
    assert np.array_equal(chk.threshold(K, 3).ravel().nonzero()[0], [0, 2, 7])
    assert np.array_equal(chk.threshold(K, 4).ravel().nonzero()[0], [0, 2, 4, 7])
    assert np.array_equal(chk.threshold(K, 100), K)
    assert np.array_equal(chk.threshold(K, -1), K)
    z = chk.threshold(K, 0)
    assert not z.any() and not np.signbit(z).any()                      # dropped entries are +0.0
    # Julia's sortperm(abs(K[:]), rev=true) is stable: a brute-force restatement
    rng = np.random.default_rng(5)
    K = rng.integers(-3, 4, (8, 5)).astype(np.float32)
    flat = K.ravel()
    order = sorted(range(flat.size), key=lambda i: (-abs(float(flat[i])), i))
    for S in range(flat.size + 1):
        want = np.zeros_like(flat)
        want[order[:S]] = flat[order[:S]]
        assert np.array_equal(chk.threshold(K, S).ravel(), want)


def test_rounding_allowance_covers_f32_rounding():
    P = _problem(6, 70, 3, 2)
    Kls = _least_squares(P)
    tau = 0.4 * np.abs(Kls).sum()
    K, _ = chk.spg(P, tau, opt_tol=1e-10, max_iter=20000)
    K32 = K.astype(np.float32)
    g64 = chk.certificate(P, K, tau)["gap"]
    g32 = chk.certificate(P, K32, tau)["gap"]
    assert abs(g32 - g64) <= chk.rounding_allowance(P, K32, tau)


# ---- the product's argument rules ----------------------------------------------------------------------------------------------------------
def _args(n=20, d=4, m=2):
    X = np.zeros((d, n), np.float32)
    B = np.ones((m, n), np.int16)
    C0 = [np.zeros((d, H), np.float32) for _ in range(m)]
    return X, B, C0


@pytest.mark.parametrize("tau", [-1.0, float("nan"), "x", None])
def test_python_rejects_bad_tau(lsq, tau):
    X, B, C0 = _args()
    with pytest.raises(ValueError):
        lsq.update_codebooks_spgl1(X, B, H, tau, C0)
    with pytest.raises(ValueError):
        lsq.update_codebooks_spgl1_threshold(X, B, H, tau, C0, 10)


@pytest.mark.parametrize("S", [1.5, "3", None, True])
def test_python_rejects_bad_S(lsq, S):
    X, B, C0 = _args()
    with pytest.raises(ValueError):
        lsq.update_codebooks_spgl1_threshold(X, B, H, 1.0, C0, S)


def test_python_rejects_bad_shapes(lsq):
    X, B, C0 = _args()
    bad = [
        (X[:, :5], B, C0),                                   # n differs
        (X, B, C0[:1]),                                      # m differs
        (X, B, [c[:3] for c in C0]),                         # d differs
        (X, np.ones((17, 20), np.int16), [np.zeros((4, H), np.float32)] * 17),   # m > 16
        (X.ravel(), B, C0),
        (X, B * 0, C0),                                      # codes are 1-based
    ]
    for Xb, Bb, Cb in bad:
        with pytest.raises(ValueError):
            lsq.update_codebooks_spgl1(Xb, Bb, H, 1.0, Cb)
    with pytest.raises(ValueError):
        lsq.update_codebooks_spgl1(X, B, 128, 1.0, [np.zeros((4, 128), np.float32)] * 2)
    with pytest.raises(ValueError):
        lsq.train_lsq_sparse(X, 2, H, 1, 1, 1, True, 1, 10, -2.0, B, [np.zeros((2, H), np.float32)] * 2, np.eye(4, dtype=np.float32), V=False)
    with pytest.raises(ValueError):
        lsq.train_lsq_sparse(X, 2, H, 1, 1, 1, True, 1, 10, 1.0, B, [np.zeros((2, H), np.float32)] * 2, np.eye(3, dtype=np.float32), V=False)


def test_engine_checks_arguments_before_the_device(lsq):
    check = lsq.engine.check_spgl1_args
    check((10, 4), (10, 2), 2, H, 0.0, -1)
    check((10, 4), (10, 2), 2, H, float("inf"), 5, (2 * H, 4))
    for args in [((10, 4), (10, 2), 2, H, -0.5, -1), ((10, 4), (9, 2), 2, H, 1.0, -1), ((10, 4), (10, 2), 2, H, 1.0, -1, (H, 4)),
                 ((0, 4), (0, 2), 2, H, 1.0, -1), ((10, 4), (10, 2), 2, H, 1.0, -1, None, 2.0), ((10, 4), (10, 2), 2, H, 1.0, -1, None, None, 0)]:
        with pytest.raises(ValueError):
            check(*args)


def _cabi(lsq, name, **kw):
    L = lsq._lib.load()
    n, d, m = 8, 3, 2
    X = np.zeros((n, d), np.float32)
    B = np.ones((n, m), np.int16)
    K = np.zeros((m * H, d), np.float32)
    info = lsq._lib.Spgl1Info()
    a = dict(d=d, n=n, m=m, h=H, tau=1.0, S=-1)
    a.update(kw)
    return getattr(L, name)(None, X.ctypes.data, B.ctypes.data, a["d"], a["n"], a["m"], a["h"], a["tau"], None, a["S"], None, K.ctypes.data,
                            C.byref(info))


def test_cabi_rejects_bad_arguments(lsq):
    for name in ("lsq_update_codebooks_spgl1", "lsq_update_codebooks_spgl1_dev"):
        for kw in (dict(tau=-1.0), dict(tau=float("nan")), dict(h=128), dict(m=17), dict(m=0), dict(d=0), dict(n=0)):
            assert _cabi(lsq, name, **kw) == lsq._lib.LSQ_EINVAL, (name, kw)
    assert lsq._lib.load().lsq_version() >= 800


def test_cabi_without_gpu_is_enodev(lsq):
    if lsq.device_count() > 0:
        pytest.skip("a GPU is present; the ENODEV path is for GPU-less hosts")
    for name in ("lsq_update_codebooks_spgl1", "lsq_update_codebooks_spgl1_dev"):
        assert _cabi(lsq, name) == lsq._lib.LSQ_ENODEV
    X, B, C0 = _args()
    with pytest.raises(lsq._lib.LsqError):
        lsq.update_codebooks_spgl1(X, B, H, 1.0, C0)


def test_reference_names_are_exported(lsq):
    for name in ("update_codebooks_spgl1", "update_codebooks_spgl1_threshold", "train_lsq_sparse"):
        assert name in lsq.__all__ and callable(getattr(lsq, name))
    assert "lsq_update_codebooks_spgl1" in lsq._lib.SIGNATURES and "lsq_update_codebooks_spgl1_dev" in lsq._lib.SIGNATURES


def test_brute_force_projection_small_grid():
    # every sign pattern of a 3-vector with planted equal magnitudes
    for signs in itertools.product((-1, 1), repeat=3):
        v = np.array(signs, dtype=np.float64) * np.array([2.0, 2.0, 1.0])
        p = chk.project_l1(v, 2.0)
        assert np.allclose(p, np.array(signs) * np.array([1.0, 1.0, 0.0]))
