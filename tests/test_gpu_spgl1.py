"""The SPGL1 (LASSO) codebook update on the device (csrc/lsq_spgl1.hip) against the float64 certificate of tests/spgl1_check.py.

K itself is never compared with another solver's K: S'S is singular (each codebook's indicator columns sum to the all-ones vector, unused
codewords give zero columns), so the minimiser is not unique.  What is checked is what the method guarantees: feasibility, the duality gap
(or SPGL1's residual rule), objectives, the thresholding rule bit for bit, and determinism."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spgl1_check as chk  # noqa: E402

pytestmark = pytest.mark.gpu

H = 256
TOL = 1e-4
MAXIT = 3000


def _data(seed, n, d, m, kind="sift"):
    rng = np.random.default_rng(seed)
    if kind == "sift":
        X = np.floor(rng.random((n, d)) * 64).astype(np.float32) * rng.uniform(0.2, 2.0, (1, d)).astype(np.float32)
    else:
        X = (rng.standard_normal((n, d)) * 5).astype(np.float32)
    codes = rng.integers(0, H, (n, m)).astype(np.uint8)
    return np.ascontiguousarray(X), np.ascontiguousarray(codes)


def _B(codes):
    return (codes.astype(np.int16) + 1)


def _pq_l1(X, codes, m):
    """||K_pq||_1 of PQ-style codebooks for these codes: codeword c of codebook j = the mean of its rows on sub-space j (0 elsewhere)."""
    n, d = X.shape
    tot = 0.0
    bounds = np.linspace(0, d, m + 1).astype(int) if d >= m else np.minimum(np.arange(m + 1), d)
    for j in range(m):
        lo, hi = bounds[j], bounds[j + 1]
        if hi <= lo:
            continue
        cnt = np.bincount(codes[:, j], minlength=H).astype(np.float64)
        for t in range(lo, hi):
            s = np.bincount(codes[:, j], weights=X[:, t].astype(np.float64), minlength=H)
            tot += float(np.abs(s[cnt > 0] / cnt[cnt > 0]).sum())
    return tot


def _certify(P, K, tau, info, opt_tol=TOL):
    """The returned f32 K is feasible and solved in float64, up to the rounding allowance of its f32 values; info agrees with the recomputation."""
    c = chk.certificate(P, K, tau)
    allow = chk.rounding_allowance(P, K, tau)
    assert c["l1"] <= tau * (1 + 1e-6) + 1e-30, (c["l1"], tau)
    assert info["status"] == 0, info
    gap_ok = c["rel_gap"] <= opt_tol + allow / max(1.0, c["f"])
    dr = float(np.sqrt(np.sum(P.A(np.abs(np.asarray(K, np.float64)) * 2.0 ** -24 + 2.0 ** -149) ** 2)))
    res_ok = c["rnorm"] <= opt_tol * c["bnorm"] + dr + 1e-12 * c["bnorm"]
    assert gap_ok or res_ok, (c, allow, info)
    assert abs(info["f"] - c["f"]) <= allow + 1e-9 * max(1.0, c["f"]), (info["f"], c["f"], allow)
    assert info["l1"] == pytest.approx(c["l1"], rel=1e-9, abs=1e-30)
    assert info["nnz_before_threshold"] == int(np.count_nonzero(K)) and info["tau"] == tau
    assert info["iterations"] <= info["line_search_trials"] or info["iterations"] == 0
    return c


SWEEP = [(1, 3, 2), (300, 1, 1), (300, 3, 7), (4103, 3, 16), (4103, 128, 8), (300, 128, 2), (64, 960, 2)]


@pytest.mark.parametrize("n,d,m", SWEEP, ids=["n%d_d%d_m%d" % s for s in SWEEP])
def test_certificate_sweep(engine, n, d, m):
    X, codes = _data(100 + n + d + m, n, d, m)
    P = chk.Problem(X, codes, m)
    Kls, _ = engine.update_codebooks(X, _B(codes), m)
    lls = float(np.abs(Kls.astype(np.float64)).sum())
    f_lsqr = chk.certificate(P, Kls, np.inf)["f"]
    taus = [0.0, 0.05 * lls, 0.7 * _pq_l1(X, codes, m), 1.5 * lls + 1.0]
    for q, tau in enumerate(taus):
        K, info = engine.update_codebooks_spgl1(X, _B(codes), m, tau, max_iter=MAXIT)
        if info["status"] != 0:
            # SPGL1 is slow on problems with about as many codewords as rows (m h >= n / 2 per dimension) and a binding tau: then the
            # restatement must stop at the same cap with the same objective, and the returned iterate must still be feasible
            assert 2 * m * H >= n and n * d <= 300 * 128 and info["status"] == 1 and info["iterations"] == MAXIT, info
            _, ref = chk.spg(P, tau, opt_tol=TOL, max_iter=MAXIT)
            c = chk.certificate(P, K, tau)
            assert ref["status"] == 1, ref                                 # the restatement does not certify within the cap either
            assert c["l1"] <= tau * (1 + 1e-6) and info["f"] == pytest.approx(c["f"], rel=1e-6)
            assert c["f"] <= 0.5 * float(np.sum(P.X ** 2)) and c["f"] <= 1.1 * ref["f"], (ref["f"], c["f"])      # descent from K = 0
            continue
        c = _certify(P, K, tau, info)
        if tau == 0.0:
            assert not K.any()
        if q == 3:                                                       # not binding: the least-squares residual, as the device LSQR's
            assert np.sqrt(2 * c["f"]) <= (1 + 1e-4) * np.sqrt(2 * f_lsqr) + 1e-9
        if n * d <= 300 * 128 and 0 < q < 3:                             # the checker's SPG reaches the same objective
            _, ref = chk.spg(P, tau, opt_tol=TOL, max_iter=MAXIT)
            assert abs(ref["f"] - c["f"]) <= 1e-4 * max(1.0, c["f"]), (ref["f"], c["f"])


def test_large_n_demo_tau(engine):
    n, d, m = 100_000, 128, 8
    X, codes = _data(7, n, d, m)
    P = chk.Problem(X, codes, m)
    tau = 0.7 * _pq_l1(X, codes, m)
    K, info = engine.update_codebooks_spgl1(X, _B(codes), m, tau, max_iter=MAXIT)
    _certify(P, K, tau, info)


def test_warm_starts(engine):
    n, d, m = 4103, 16, 4
    X, codes = _data(11, n, d, m)
    P = chk.Problem(X, codes, m)
    Kls, _ = engine.update_codebooks(X, _B(codes), m)
    tau = 0.3 * float(np.abs(Kls.astype(np.float64)).sum())
    K, info = engine.update_codebooks_spgl1(X, _B(codes), m, tau, max_iter=MAXIT)
    _certify(P, K, tau, info)
    # from the optimum: a few iterations at most
    K2, info2 = engine.update_codebooks_spgl1(X, _B(codes), m, tau, K_init=K, max_iter=MAXIT)
    _certify(P, K2, tau, info2)
    assert info2["iterations"] <= 3, info2
    # from an infeasible start: projected first, then solved
    K3, info3 = engine.update_codebooks_spgl1(X, _B(codes), m, tau, K_init=10 * Kls, max_iter=MAXIT)
    _certify(P, K3, tau, info3)
    # no K_init = a zero K_init, bit for bit
    K4, _ = engine.update_codebooks_spgl1(X, _B(codes), m, tau, K_init=np.zeros_like(K), max_iter=MAXIT)
    assert np.array_equal(K4.view(np.uint32), K.view(np.uint32))


@pytest.mark.parametrize("case", ["zero_data", "one_code", "unused_codewords", "duplicated_rows"])
def test_degenerate_data(engine, case):
    n, d, m = 500, 8, 3
    X, codes = _data(21, n, d, m)
    if case == "zero_data":
        X[:] = 0
    elif case == "one_code":
        codes[:] = 17
    elif case == "unused_codewords":
        codes = (codes % 5).astype(np.uint8)
    else:
        X[250:] = X[:250]
        codes[250:] = codes[:250]
    P = chk.Problem(X, codes, m)
    for tau in (0.0, 50.0, 1e4):
        K, info = engine.update_codebooks_spgl1(X, _B(codes), m, tau, max_iter=MAXIT)
        _certify(P, K, tau, info)
        if case == "zero_data":
            assert not K.any()


def test_threshold_is_the_julia_rule_bit_for_bit(engine):
    n, d, m = 2000, 4, 3
    X, codes = _data(31, n, d, m, kind="gauss")
    X[:, 1] = X[:, 0]                                                    # equal columns: every codeword's values tie across t = 0, 1
    P = chk.Problem(X, codes, m)
    tau = 200.0
    K, info = engine.update_codebooks_spgl1(X, _B(codes), m, tau, S=-1, max_iter=MAXIT)
    _certify(P, K, tau, info)
    nnz = int(np.count_nonzero(K))
    assert np.array_equal(K[:, 0], K[:, 1]) and nnz > 4
    for S in (0, 1, 2, 3, nnz - 1, nnz, nnz + 5, K.size):
        KS, iS = engine.update_codebooks_spgl1(X, _B(codes), m, tau, S=S, max_iter=MAXIT)
        want = chk.threshold(K, S)
        assert np.array_equal(KS.view(np.uint32), want.view(np.uint32)), S
        assert iS["nnz"] == int(np.count_nonzero(want)) <= max(S, 0) and iS["nnz_before_threshold"] == nnz


def test_deterministic_and_host_equals_dev(engine):
    import torch
    n, d, m = 4103, 32, 7
    X, codes = _data(41, n, d, m)
    K0 = (np.random.default_rng(1).standard_normal((m * H, d)) * 0.1).astype(np.float32)
    tau, S = 0.7 * _pq_l1(X, codes, m), d * H
    Ka, ia = engine.update_codebooks_spgl1(X, _B(codes), m, tau, K_init=K0, S=S, max_iter=MAXIT)
    Kb, ib = engine.update_codebooks_spgl1(X, _B(codes), m, tau, K_init=K0, S=S, max_iter=MAXIT)
    assert np.array_equal(Ka.view(np.uint32), Kb.view(np.uint32)) and ia == ib
    dX, dc, dK0 = torch.from_numpy(X).cuda(), torch.from_numpy(codes).cuda(), torch.from_numpy(K0).cuda()
    dK, idv = engine.update_codebooks_spgl1_dev(dX, dc, m, tau, dK_init=dK0, S=S, max_iter=MAXIT)
    torch.cuda.synchronize()
    assert np.array_equal(dK.cpu().numpy().view(np.uint32), Ka.view(np.uint32)) and idv == ia
    # offset views (contiguous, storage offset of one element) are handled; strided views are rejected
    bigX = torch.zeros(n * d + 1, dtype=torch.float32, device="cuda")
    bigX[1:] = dX.reshape(-1)
    bigc = torch.zeros(n * m + 1, dtype=torch.uint8, device="cuda")
    bigc[1:] = dc.reshape(-1)
    dK2, _ = engine.update_codebooks_spgl1_dev(bigX[1:].view(n, d), bigc[1:].view(n, m), m, tau, dK_init=dK0, S=S, max_iter=MAXIT)
    torch.cuda.synchronize()
    assert np.array_equal(dK2.cpu().numpy().view(np.uint32), Ka.view(np.uint32))
    with pytest.raises(ValueError):
        engine.update_codebooks_spgl1_dev(torch.zeros((d, n), dtype=torch.float32, device="cuda").T, dc, m, tau)
    with pytest.raises(ValueError):
        engine.update_codebooks_spgl1_dev(dX, dc, m, -1.0)


def _sparse_train(lsq, engine, seed):
    from importlib import import_module
    ini = import_module("local-search-quantization_amd.initializers")
    n, d, m, h = 10_000, 128, 7, H
    rng = np.random.default_rng(5)
    X = (np.floor(rng.random((d, n)) * 64) * rng.uniform(0.2, 2.0, (d, 1))).astype(np.float32)
    C, B, _ = ini.train_pq(X, m, h, seed=seed, engine=engine)
    tau = 0.7 * sum(float(np.abs(Cj.astype(np.float64)).sum()) for Cj in C)
    S = d * h
    infos = []
    out = lsq.train_lsq_sparse(X, m, h, 2, 8, 4, True, 4, S, tau, B, C, np.eye(d, dtype=np.float32), None, False, seed=seed, engine=engine,
                               infos=infos, max_iter=MAXIT)
    return out, infos, tau, S, (n, d, m)


def test_train_lsq_sparse_end_to_end(lsq, engine):
    (C, B, R, obj, cbnorms, objs), infos, tau, S, (n, d, m) = _sparse_train(lsq, engine, 3)
    assert len(C) == m and all(Cj.shape == (d, H) and Cj.dtype == np.float32 for Cj in C)
    assert B.shape == (m, n) and B.dtype == np.int16 and B.min() >= 1 and B.max() <= H
    assert R.shape == (d, d) and np.isfinite(obj) and cbnorms.dtype == np.float32 and cbnorms.size <= H
    assert objs.shape == (2,) and objs.dtype == np.float32 and np.all(np.isfinite(objs))
    assert len(infos) == 3
    for info in infos:
        assert info["status"] == 0 and info["l1"] <= tau * (1 + 1e-6) and info["nnz"] <= S
    assert sum(int(np.count_nonzero(Cj)) for Cj in C) == infos[-1]["nnz"]
    print("SLSQ1 objs", objs.tolist(), "final", obj, "iterations", [i["iterations"] for i in infos])
    (C2, B2, _, obj2, cb2, objs2), infos2, *_ = _sparse_train(lsq, engine, 3)
    assert all(np.array_equal(a, b) for a, b in zip(C, C2)) and np.array_equal(B, B2) and np.array_equal(objs, objs2) and obj == obj2
    assert np.array_equal(cbnorms, cb2)
