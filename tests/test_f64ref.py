"""The float64 references of tests/f64ref.py against the f32 outputs the CPU already has -- the oracle's tables, unaries and costs, the host scans,
the host LSQR, the checker's Viterbi and assignment -- which pins those restatements from outside themselves; and, for every comparator, a
corrupted copy of a correct output that must fail it.  Host code: runs without a GPU."""
import numpy as np
import pytest

import f64ref as R
import oracle.init_oracle as ini
from test_linscan import _case, _ours
from test_linscan_pq import drop_in, pq_case

H = 256


def _tables_case(seed, n, d, m):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    K = (rng.standard_normal((m * H, d)) / m).astype(np.float32)
    return X, K


@pytest.mark.parametrize("n,d,m", [(129, 33, 4), (17, 1030, 2), (5, 1, 3)])
def test_oracle_unaries_within_the_bound(oracle, n, d, m):
    X, K = _tables_case(n + d, n, d, m)
    U = oracle.unaries(X, K, m, H)
    ref, bnd = R.unaries(X, K, m)
    R.check_values(U, ref, bnd, "oracle unaries")
    with pytest.raises(AssertionError):                                     # the norm term dropped
        R.check_values(U - (K.astype(np.float64) ** 2).sum(1).reshape(m, 1, H), ref, bnd)


@pytest.mark.parametrize("d,m", [(20, 3), (129, 2)])
def test_oracle_pair_tables_within_the_bound(oracle, d, m):
    _, K = _tables_case(d, 1, d, m)
    T = oracle.tables(K, m, H)
    ref, bnd = R.pair_tables(K, m)
    R.check_values(T, ref, bnd, "oracle pair tables")
    bad = T.copy()
    bad[0, 1, 3, 5], bad[0, 1, 5, 3] = T[0, 1, 5, 3], T[0, 1, 3, 5]        # two table entries swapped (a transposed pair table)
    with pytest.raises(AssertionError):
        R.check_values(bad, ref, bnd)


def test_oracle_veccost_and_qerror_within_the_bound(oracle):
    X, K = _tables_case(7, 300, 40, 8)
    codes = np.random.default_rng(8).integers(0, H, size=(300, 8)).astype(np.uint8)
    cost = oracle.veccost(X, K, codes, H)
    ref, bnd = R.veccost(X, K, codes, 8)
    R.check_values(cost, ref, bnd, "oracle veccost")
    q = oracle.qerror(X, codes.astype(np.int16) + 1, K, 8, H)
    R.check_values(q, ref.mean(), R.mean_bound(bnd, ref), "oracle qerror")
    wrong = codes.copy()
    wrong[:, 2] = wrong[:, 3]                                               # the wrong codeword of one codebook
    with pytest.raises(AssertionError):
        R.check_values(oracle.veccost(X, K, wrong, H), ref, bnd)


@pytest.mark.parametrize("n,nq,d,m,k", [(4000, 25, 64, 8, 10), (300, 4, 33, 3, 300), (2000, 6, 16, 4, 50)])
def test_host_lsq_scan_selects_the_float64_neighbours(lsq, n, nq, d, m, k):
    rng = np.random.default_rng(n + d)
    codes, Q, K, dbn = _case(rng, n, nq, d, m)
    dists, ids = _ours(lsq, codes, Q, K, dbn, m, k)
    vals, bnd = R.lsq_adc(Q, K, codes, dbn, m)
    R.check_topk(ids - 1, dists, vals, bnd, "host LSQ scan")
    d0, i0 = _ours(lsq, codes, Q, K, np.zeros_like(dbn), m, k)              # the norm term dropped
    with pytest.raises(AssertionError):
        R.check_topk(i0 - 1, d0, vals, bnd)
    if k < n:
        d1, i1 = _ours(lsq, codes, Q, K, dbn, m, k + 1)
        bad_i, bad_d = i1[:, :k].copy(), d1[:, :k].copy()
        bad_i[0, 0], bad_d[0, 0] = i1[0, k], d1[0, k]                       # the nearest neighbour replaced by the (k+1)-th
        with pytest.raises(AssertionError):
            R.check_topk(bad_i - 1, bad_d, vals, bnd)


@pytest.mark.parametrize("n,nq,m,subdim,k", [(3000, 7, 4, 5, 20), (500, 3, 3, 7, 500), (2000, 4, 1, 40, 8)])
def test_host_pq_scan_selects_the_float64_neighbours(lsq, n, nq, m, subdim, k):
    codes, centers, Q = pq_case(n + m, n, nq, m, subdim, m, m * subdim + 1)
    dists, ids = drop_in(lsq, codes, centers, Q, m, subdim, k)
    vals, bnd = R.pq_dist(Q[:, :m * subdim], list(centers), codes)
    R.check_topk(ids, dists, vals, bnd, "host PQ scan")
    if m > 1:
        Qs = Q.copy()
        Qs[:, subdim:m * subdim] = Q[:, subdim + 1:m * subdim + 1]           # every sub-space boundary after the first shifted by one
        ds, i_s = drop_in(lsq, codes, centers, Qs, m, subdim, k)
        with pytest.raises(AssertionError):
            R.check_values(ds, vals[np.arange(nq)[:, None], i_s], bnd[np.arange(nq)[:, None], i_s])


def test_pq_split_follows_splitarray():
    """d = 10 over m = 3 sub-spaces: widths 4, 3, 3; the helper refuses codebooks that do not match the split"""
    assert [(s.start, s.stop) for s in R.splitarray(10, 3)] == [(0, 4), (4, 7), (7, 10)]
    rng = np.random.default_rng(1)
    Q = rng.standard_normal((2, 10)).astype(np.float32)
    C = [rng.standard_normal((H, w)).astype(np.float32) for w in (4, 3, 3)]
    codes = rng.integers(0, H, size=(5, 3))
    v, _ = R.pq_dist(Q, C, codes)
    want = sum(((Q[:, None, s].astype(np.float64) - C[k][codes[:, k]][None].astype(np.float64)) ** 2).sum(2) for k, s in enumerate(R.splitarray(10, 3)))
    assert np.allclose(v, want, rtol=1e-12)
    with pytest.raises(AssertionError):
        R.pq_dist(Q, [C[1], C[0], C[2]], codes)


def _lsqr_problem(rng, d, n, m, noise=0.05, skew=False):
    codes = rng.integers(0, H, size=(n, m))
    if skew:
        codes[rng.random(n) < 0.9, 0] = 7                                   # 90 % of the first codebook's codes are one value
    Ctrue = rng.standard_normal((m * H, d)).astype(np.float32)
    X = (sum(Ctrue[j * H + codes[:, j]] for j in range(m)) + noise * rng.standard_normal((n, d))).astype(np.float32)
    return X, codes


def check_lsqr(K, X, codes, m, cols, method, skewed=False):
    """K (m h, d) f32 codebooks against the float64 least-squares optimum: the residual within (1 + 1e-4) of the optimum's and the
    reconstruction within 2e-4 of the optimum's.  skewed: a code histogram dominated by one value makes S ill-conditioned, and LSQR's stopping rule
    (atol = sqrt(eps_f32), the reference's tolerance) then leaves the reconstruction up to ~9e-4 from the optimum; there the 2e-4 is replaced by
    the stopping rule itself, evaluated in float64 (f64ref.lsqr_stopping_rule), and the residual criterion stays."""
    _, rec_ref = R.lsq_codebooks(X, codes, m, cols=cols, method=method)
    rec = R.reconstruct(K[:, cols], codes, m)
    Xc = X[:, cols].astype(np.float64)
    r, r0 = np.linalg.norm(Xc - rec), np.linalg.norm(Xc - rec_ref)
    assert r <= r0 * (1 + 1e-4), (r, r0)
    if skewed:
        crit = R.lsqr_stopping_rule(X, codes, m, K, cols)
        assert np.all(crit <= np.sqrt(np.finfo(np.float32).eps)), crit
    else:
        assert np.linalg.norm(rec - rec_ref) <= 2e-4 * np.linalg.norm(rec_ref), np.linalg.norm(rec - rec_ref) / np.linalg.norm(rec_ref)


@pytest.mark.parametrize("d,n,m,skew,method", [(6, 20_000, 4, False, "lsqr"), (4, 60_000, 3, True, "normal"), (5, 3000, 1, False, "normal")])
def test_host_lsqr_reaches_the_float64_optimum(lsq, d, n, m, skew, method):
    rng = np.random.default_rng(d * n)
    X, codes = _lsqr_problem(rng, d, n, m, skew=skew)
    C = lsq.update_codebooks(np.ascontiguousarray(X.T), (codes.T + 1).astype(np.int16), H, nthreads=4)
    K = np.ascontiguousarray(np.concatenate(C, axis=1).T)
    check_lsqr(K, X, codes, m, np.arange(d), method, skew)
    Kb = K.copy()
    Kb[:H] = 0                                                              # one codebook's update skipped
    with pytest.raises(AssertionError):
        check_lsqr(Kb, X, codes, m, np.arange(d), method, skew)


def _chain_case(seed, n, d, m):
    rng = np.random.default_rng(seed)
    od = ini.get_cbdims_chain(d, m)
    K = np.zeros((m * H, d), dtype=np.float32)
    for i in range(m):
        K[i * H:(i + 1) * H, od[i]] = rng.standard_normal((H, od[i].stop - od[i].start))
    X = rng.standard_normal((n, d)).astype(np.float32) * 2
    return X, K


@pytest.mark.parametrize("n,d,m", [(40, 32, 4), (16, 24, 8), (6, 12, 3)])
def test_checker_viterbi_is_the_float64_chain_optimum(n, d, m):
    X, K = _chain_case(n + d + m, n, d, m)
    codes = ini.encoding_viterbi_exact(X, K, m, H)
    R.check_chain(X, K, codes, m, what="checker Viterbi")
    if m == 3:
        for i in range(3):
            e, _ = R.chain_exhaustive_m3(X[i], K)
            opt, _ = R.chain_optimum(X[i:i + 1], K, 3)
            assert abs(opt[0] - e) <= 1e-9 * (1 + abs(e))
    # one code moved to its second-best state (the others held): the vector and position with the widest gap, so the move is certain to show
    U, _ = R.unaries(X, K, m)
    T, _ = R.pair_tables(K, m)
    best = (-1.0, 0, 0, 0)
    for i in range(n):
        for j in range(m):
            s = U[j, i].copy()
            if j > 0:
                s += T[j, j - 1, codes[i, j - 1]]
            if j < m - 1:
                s += T[j, j + 1, codes[i, j + 1]]
            o = np.argsort(s)
            if s[o[1]] - s[o[0]] > best[0]:
                best = (s[o[1]] - s[o[0]], i, j, o[1])
    bad = codes.copy()
    bad[best[1], best[2]] = best[3]
    with pytest.raises(AssertionError):
        R.check_chain(X, K, bad, m)


@pytest.mark.parametrize("n,d,m", [(200, 16, 4), (33, 129, 2)])
def test_checker_assignment_is_the_float64_nearest_codeword(n, d, m):
    X, K = _tables_case(n * d, n, d, m)
    sd = R.splitarray(d, m)
    Kp = np.zeros_like(K)
    for j in range(m):
        Kp[j * H:(j + 1) * H, sd[j]] = K[j * H:(j + 1) * H, sd[j]]          # codebook j padded to d rows, zero outside its sub-space
    a, mv = ini.assign_codewords_exact(X, Kp, m, H)
    vals, bnd = R.assign_values(X, Kp, m, sd)
    for j in range(m):
        xs = (X[:, sd[j]].astype(np.float64) ** 2).sum(1)
        R.check_argmin(a[:, j], vals[j], bnd[j], "checker assignment, sub-space %d" % j)
        R.check_values(mv[:, j] + xs, vals[j][np.arange(n), a[:, j]], bnd[j][np.arange(n), a[:, j]], "checker minima")
    second = np.argsort(vals[0], axis=1)[:, 1]
    with pytest.raises(AssertionError):
        R.check_argmin(second, vals[0], bnd[0])


def test_oracle_norm_quantisation_within_the_bound(oracle):
    rng = np.random.default_rng(3)
    d, n, m = 30, 400, 5
    C = [rng.standard_normal((d, H)).astype(np.float32) for _ in range(m)]
    B = rng.integers(1, H + 1, size=(m, n)).astype(np.int16)
    K = np.ascontiguousarray(np.concatenate([c.T for c in C], axis=0))
    codes = B.T.astype(np.int64) - 1
    nrm64, nb = R.norms(K, codes, m)
    cb = np.sort(rng.choice(nrm64, size=64, replace=False)).astype(np.float32)
    idx, nrm = oracle.quantize_norms(B, C, cb, want_norms=True)
    R.check_values(nrm, nrm64, nb, "oracle norms")
    vals, vb = R.norm_centroid_values(nrm64, nb, cb)
    R.check_argmin(idx.astype(np.int64) - 1, vals, vb, "oracle norm centroid")
    with pytest.raises(AssertionError):
        R.check_argmin(np.argsort(vals, axis=1)[:, 1], vals, vb)


def test_selection_window_uses_the_bounds_of_the_swapped_pair():
    """items 1 and 2 (values 1 and 2) may swap at k = 2 only if their f32 errors can close the gap: bound 0.6 each can, 0.4 each cannot"""
    vals = np.array([0.0, 1.0, 2.0, 3.0])
    R.check_selection([0, 2], vals, np.array([0.0, 0.6, 0.6, 0.0]))
    with pytest.raises(AssertionError):
        R.check_selection([0, 2], vals, np.array([0.0, 0.4, 0.4, 0.0]))
    with pytest.raises(AssertionError):                                     # a large bound elsewhere in the row does not widen the window
        R.check_selection([0, 2], vals, np.array([0.0, 0.4, 0.4, 5.0]))
    R.check_argmin(np.array([1]), vals[None, :2], np.array([[0.5, 0.5]]))
    with pytest.raises(AssertionError):
        R.check_argmin(np.array([1]), vals[None, :3], np.array([[0.4, 0.4, 9.0]]))
