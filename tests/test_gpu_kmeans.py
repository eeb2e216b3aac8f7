"""PQ / OPQ training resident on the device (csrc/lsq_kmeans.hip, initializers.kmeans_dev / train_pq_dev / train_opq_dev) against tests/kmeans_check.py.

  * lsq_update_centers[_dev]   BIT-EXACT against centers_exact (the arithmetic of the host trainers' _centers): PQ, dense and chain covers, n = 1, n < h,
                               n = 10^5, one code for every row, empty clusters with and without K_prev; exact counts; exact zeros outside the cover with a
                               NaN-filled `out`; host and device entries agree; a second call returns the same bits.
  * lsq_kmeanspp_seed[_dev]    d2 bit-exact against the direct-form replay from the returned rows; every choice judged independently of the device's order of
                               summation (judge_seeding: the band is the worst-case rounding of two n-term sums, at most 1 % ambiguous steps).
  * train_pq_dev               with the same explicit initial codebooks: the codes and the bits of the host train_pq; with its own seeding: within the host
                               trainer's own seed-to-seed spread.
  * train_opq_dev              the trajectory of train_opq at the same seed within 5e-3, orthogonal R, optimal codes, feeds train_chainq_dev.
"""
import numpy as np
import pytest

import kmeans_check as kc

pytestmark = pytest.mark.gpu
H = 256


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _codes(rng, n, m, kind):
    if kind == "one":
        return np.full((n, m), 200, dtype=np.uint8)
    if kind == "few":
        return rng.integers(3, size=(n, m)).astype(np.uint8) * 100
    if kind == "skew":
        return np.minimum(rng.exponential(25.0, size=(n, m)).astype(np.int64), H - 1).astype(np.uint8)
    return rng.integers(H, size=(n, m)).astype(np.uint8)


MEANS_CASES = [(5000, 128, 8, "pq", "random"), (2000, 960, 8, "pq", "random"), (5000, 64, 16, "pq", "skew"), (5000, 30, 4, "pq", "random"),
               (5000, 24, 1, "pq", "random"), (4000, 33, 5, "chain", "random"), (1, 128, 8, "pq", "random"), (100, 128, 8, "pq", "random"),
               (100_000, 128, 8, "pq", "random"), (3000, 30, 4, "pq", "one"), (3000, 16, 4, "pq", "few"), (70_000, 20, 3, "chain", "skew")]


@pytest.mark.parametrize("n,d,m,cover_kind,code_kind", MEANS_CASES)
@pytest.mark.parametrize("prev", [False, True])
def test_cluster_means_bit_exact(engine, n, d, m, cover_kind, code_kind, prev):
    import torch
    rng = np.random.default_rng(n + d + m)
    X = (rng.standard_normal((n, d)) * 2 + 0.5).astype(np.float32)
    codes = _codes(rng, n, m, code_kind)
    cover = kc.pq_cover(d, m) if cover_kind == "pq" else kc.chain_cover(d, m)
    K_prev = rng.standard_normal((m * H, d)).astype(np.float32) if prev else None
    want, want_cnt = kc.centers_exact(X, codes, cover, H, K_prev)
    Kh, cnt_h = engine.update_centers(X, codes.astype(np.int16) + 1, cover, m, K_prev=K_prev)
    assert np.array_equal(cnt_h, want_cnt)
    assert np.array_equal(_bits(Kh), _bits(want)), "host entry: %d entries differ" % int((_bits(Kh) != _bits(want)).sum())
    dX, dB = torch.from_numpy(X).cuda(), torch.from_numpy(codes).cuda()
    dprev = None if K_prev is None else torch.from_numpy(K_prev).cuda()
    out = torch.full((m * H, d), float("nan"), dtype=torch.float32, device="cuda")
    dK, dcnt = engine.update_centers_dev(dX, dB, cover, m, K_prev=dprev, out=out)
    torch.cuda.synchronize()
    assert dK is out
    Kd = dK.cpu().numpy()
    assert np.array_equal(_bits(Kd), _bits(want)) and np.array_equal(dcnt.cpu().numpy(), want_cnt)
    for j in range(m):                                             # exact +0.0 outside the cover
        blk = Kd[j * H:(j + 1) * H][:, cover[:, j] == 0]
        assert not blk.any() and not np.signbit(blk).any()
    dK2, dcnt2 = engine.update_centers_dev(dX, dB, cover, m, K_prev=dprev)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dK2.cpu().numpy()), _bits(Kd)) and np.array_equal(dcnt2.cpu().numpy(), want_cnt)
    if prev:                                                       # in place: K_prev is the output tensor
        io = dprev.clone()
        engine.update_centers_dev(dX, dB, cover, m, K_prev=io, out=io)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(io.cpu().numpy()), _bits(want))


@pytest.mark.parametrize("d,n,m", kc.SEED_PROBLEMS)
def test_seeding_judged_independently_of_the_summation_order(engine, d, n, m):
    import torch
    X, cover, u = kc.seed_problem(d, n, m)
    dX = torch.from_numpy(X).cuda()
    dK, didx, dd2 = engine.kmeanspp_seed_dev(dX, cover, u, m, want_d2=True)
    torch.cuda.synchronize()
    K, idx, d2 = dK.cpu().numpy(), didx.cpu().numpy(), dd2.cpu().numpy()
    v = kc.judge_seeding(X, cover, u, idx)
    print("d=%d n=%d m=%d: ambiguous %d of %d steps, smallest gap / total %.3g, band / total %.3g" % (d, n, m, v["ambiguous"], v["steps"], v["min_gap"],
                                                                                                       v["max_band"]))
    assert v["bad"] == [], v["bad"][:5]
    assert v["ambiguous"] <= 0.01 * v["steps"] and v["zero_road"] == 0
    assert np.array_equal(_bits(d2), _bits(v["d2"])), "%d distances differ from the direct-form replay" % int((_bits(d2) != _bits(v["d2"])).sum())
    for j in range(m):
        assert idx[j, 0] == kc.uniform_row(u[j, 0], n)
        assert np.unique(idx[j]).size == H
        want = np.zeros((H, d), dtype=np.float32)
        want[:, cover[:, j] == 1] = X[idx[j]][:, cover[:, j] == 1]
        assert np.array_equal(_bits(K[j * H:(j + 1) * H]), _bits(want))
    # the float64 rule itself: the same rows wherever no step is ambiguous
    ref_idx, _ = kc.seed_f64(X, cover, u)
    if v["ambiguous"] == 0:
        assert np.array_equal(idx, ref_idx)
    # a second call, and the host-buffer entry: the same rows and bits
    dK2, didx2, _ = engine.kmeanspp_seed_dev(dX, cover, u, m)
    torch.cuda.synchronize()
    assert np.array_equal(didx2.cpu().numpy(), idx) and np.array_equal(_bits(dK2.cpu().numpy()), _bits(K))
    Kh, idx_h, d2_h = engine.kmeanspp_seed(X, cover, u, m)
    assert np.array_equal(idx_h, idx) and np.array_equal(_bits(Kh), _bits(K)) and np.array_equal(_bits(d2_h), _bits(d2))
    # sub-space j of the m-sub-space call is the m = 1 call on that cover with u[j]
    for j in range(m) if m > 1 else []:
        _, i1, d1 = engine.kmeanspp_seed_dev(dX, cover[:, j:j + 1], u[j:j + 1], 1, want_d2=True)
        torch.cuda.synchronize()
        assert np.array_equal(i1.cpu().numpy()[0], idx[j]) and np.array_equal(_bits(d1.cpu().numpy()[:, 0]), _bits(d2[:, j]))


def test_seeding_with_fewer_distinct_points_than_centres(engine):
    """10 distinct points, 30 copies each: the ten are chosen first (a zero-distance row is never chosen while the total is positive), then the total is 0 and
    the uniform rule takes over; chain (overlapping, non-aligned) covers and a general list cover."""
    rng = np.random.default_rng(3)
    Xd = np.repeat(rng.standard_normal((10, 9)).astype(np.float32), 30, axis=0)[rng.permutation(300)]
    for cover in (np.ones((9, 1), dtype=np.uint8), kc.chain_cover(9, 3), np.array([[1, 0], [0, 1]] * 4 + [[1, 1]], dtype=np.uint8)):
        m = cover.shape[1]
        u = rng.random((m, H))
        K, idx, d2 = engine.kmeanspp_seed(Xd, cover, u, m)
        v = kc.judge_seeding(Xd, cover, u, idx)
        assert v["bad"] == [] and v["zero_road"] >= m * (H - 11) and not d2.any()
        assert np.array_equal(_bits(d2), _bits(v["d2"]))
        for j in range(m):
            sub = Xd[idx[j, :10]][:, cover[:, j] == 1]
            assert np.unique(sub, axis=0).shape[0] == 10


def _list_cover(d, m):
    """codebook j covers the dimensions t with t % m == j: lists that are not contiguous"""
    cover = np.zeros((d, m), dtype=np.uint8)
    cover[np.arange(d), np.arange(d) % m] = 1
    return cover


@pytest.mark.parametrize("d,n,cover_kind,m", [(200, 3000, "pq", 2), (150, 2500, "pq", 1), (130, 2000, "chain", 3), (140, 2000, "list", 2), (960, 400, "dense", 16),
                                              (257, 700, "list", 3)])
def test_seeding_wide_and_irregular_covers(engine, d, n, cover_kind, m):
    """Sub-spaces wider than one staged chunk of the distance pass, d not a multiple of 4, overlapping covers, list covers, and more covered (codebook,
    dimension) pairs than the pass keeps centres for on chip: the same rule, judged the same way."""
    X = np.ascontiguousarray(kc.clustered(d, n, seed=7).T)
    cover = {"pq": kc.pq_cover, "chain": kc.chain_cover, "list": _list_cover, "dense": lambda d_, m_: np.ones((d_, m_), dtype=np.uint8)}[cover_kind](d, m)
    u = np.random.default_rng(d + n).random((m, H))
    K, idx, d2 = engine.kmeanspp_seed(X, cover, u, m)
    v = kc.judge_seeding(X, cover, u, idx)
    assert v["bad"] == [], v["bad"][:5]
    assert v["ambiguous"] <= 0.01 * v["steps"]
    assert np.array_equal(_bits(d2), _bits(v["d2"])), "%d distances differ from the direct-form replay" % int((_bits(d2) != _bits(v["d2"])).sum())
    for j in range(m):
        want = np.zeros((H, d), dtype=np.float32)
        want[:, cover[:, j] == 1] = X[idx[j]][:, cover[:, j] == 1]
        assert np.array_equal(_bits(K[j * H:(j + 1) * H]), _bits(want))


def _sampled_init(X, m, seed):
    """m initial codebooks (subdim x 256): data columns sampled without replacement.  X is d x n."""
    d, n = X.shape
    rng = np.random.default_rng(seed)
    cover = kc.pq_cover(d, m)
    return [np.ascontiguousarray(X[cover[:, j] == 1][:, rng.choice(n, H, replace=False)]) for j in range(m)]


@pytest.mark.parametrize("d,n,m,seed", [(16, 3000, 4, 2), (64, 10_000, 8, 4)])
def test_lloyd_on_the_device_is_the_host_trainer_bit_for_bit(lsq, engine, d, n, m, seed):
    """The same explicit initial codebooks: the assignment kernel is shared and the means are held to the same bits, so train_pq_dev and train_pq(init=...)
    return identical codes and bit-identical codebooks (re-seeded empty clusters included: the same generators in the same order)."""
    import torch
    X = kc.clustered(d, n, seed=seed)
    C0 = _sampled_init(X, m, 11)
    C, B, err = lsq.train_pq(X, m, H, seed=0, engine=engine, init=C0)
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    dK, dB, err_d = lsq.train_pq_dev(dX, m, H, seed=0, engine=engine, init=C0)
    torch.cuda.synchronize()
    assert tuple(dK.shape) == (m * H, d) and tuple(dB.shape) == (n, m) and dB.dtype == torch.uint8
    codes = dB.cpu().numpy().astype(np.int64) + 1
    assert np.array_equal(codes, B.T.astype(np.int64)), "%d codes differ" % int((codes != B.T).sum())
    Cd = lsq.codebooks_from_padded(dK, d, m)
    for j in range(m):
        assert np.array_equal(_bits(Cd[j]), _bits(C[j])), "codebook %d: %d entries differ" % (j, int((_bits(Cd[j]) != _bits(C[j])).sum()))
    cover = kc.pq_cover(d, m)
    Kd = dK.cpu().numpy()
    for j in range(m):
        assert not Kd[j * H:(j + 1) * H][:, cover[:, j] == 0].any()
    assert abs(err_d - err) <= 1e-5 * err
    # the padded layout as `init`, and a tensor: the same result
    dK2, dB2, _ = lsq.train_pq_dev(dX, m, H, seed=0, engine=engine, init=torch.from_numpy(lsq.initializers._padded(C0, d, m, H)).cuda())
    torch.cuda.synchronize()
    assert torch.equal(dB2, dB) and torch.equal(dK2, dK)


def test_train_pq_dev_with_its_own_seeding_reaches_kmeanspp_quality(lsq, engine):
    """The bar comes from the checker's trainer (oracle/init_oracle.py: numpy k-means++ + Lloyd), never from the code under test: its error over seeds
    0 .. 7 gives a range; every device run must end at or below max_host (1 + spread_host), spread_host = (max - min) / min -- a different but equally valid
    seeding stream lands anywhere in that spread."""
    import torch
    import oracle.init_oracle as ini
    X = kc.clustered(16, 3000, seed=2)
    host = np.array([ini.train_pq(X, 4, H, seed=s)[2] for s in range(8)])
    spread = (host.max() - host.min()) / host.min()
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    dev = []
    for s in range(8):
        dK, dB, err = lsq.train_pq_dev(dX, 4, H, seed=s, engine=engine)
        rec = sum(dK.cpu().numpy()[j * H + dB.cpu().numpy()[:, j].astype(np.int64)] for j in range(4))
        assert abs(float(((X.T.astype(np.float64) - rec) ** 2).sum()) / 3000 - err) <= 1e-5 * err      # the returned error is the error of what was returned
        dev.append(err)
    dev = np.array(dev)
    print("host k-means++ + Lloyd: %.5f .. %.5f (spread %.2f %%); device: %.5f .. %.5f" % (host.min(), host.max(), 100 * spread, dev.min(), dev.max()))
    assert np.all(dev <= host.max() * (1 + spread)), (dev, host)


def test_train_opq_dev_follows_train_opq(lsq, engine):
    import torch
    d, n, m, niter = 32, 2500, 4, 3
    X = kc.clustered(d, n, seed=3)
    X = (np.linalg.qr(np.random.default_rng(0).standard_normal((d, d)))[0].astype(np.float32) @ X)      # hide the axis structure
    C, B, R, obj = lsq.train_opq(X, m, H, niter, "natural", seed=1, engine=engine)
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    dK, dB, Rd, obj_d = lsq.train_opq_dev(dX, m, H, niter, "natural", seed=1, engine=engine)
    torch.cuda.synchronize()
    print("train_opq obj %s, train_opq_dev obj %s" % (obj.tolist(), obj_d.tolist()))
    assert obj_d.shape == obj.shape == (niter + 1,) and tuple(dK.shape) == (m * H, d) and tuple(dB.shape) == (n, m) and dB.dtype == torch.uint8
    assert np.all(np.abs(obj_d - obj) <= 5e-3 * np.abs(obj)), (obj_d, obj)
    R64 = Rd.astype(np.float64)
    assert np.abs(R64.T @ R64 - np.eye(d)).max() <= 1e-5
    assert obj_d[-1] <= obj_d[0] and np.all(np.diff(obj_d) <= 1e-3 * obj_d[0])
    # every code is optimal for the returned R and codebooks, re-evaluated in float64
    K, codes = dK.cpu().numpy().astype(np.float64), dB.cpu().numpy().astype(np.int64)
    Xr = X.T.astype(np.float64) @ R64
    cover = kc.pq_cover(d, m)
    for j in range(m):
        dims = cover[:, j] == 1
        Kj = K[j * H:(j + 1) * H]
        assert not Kj[:, ~dims].any()
        e = ((Xr[:, None, dims] - Kj[None, :, dims]) ** 2).sum(axis=2)                                  # (n, 256)
        emin = e.min(axis=1)
        got = e[np.arange(n), codes[:, j]]
        assert np.all(got <= emin + 1e-4 * np.maximum(1.0, np.abs(emin))), "sub-space %d: %d codes are not optimal" % (j, int((got > emin + 1e-4 * np.maximum(1.0, np.abs(emin))).sum()))
    # "random" start: the generator's draw order is train_opq's
    _, _, _, obj_r = lsq.train_opq(X, m, H, 1, "random", seed=5, engine=engine)
    _, _, Rr, obj_rd = lsq.train_opq_dev(dX, m, H, 1, "random", seed=5, engine=engine)
    assert np.all(np.abs(obj_rd - obj_r) <= 5e-3 * np.abs(obj_r)), (obj_rd, obj_r)
    # the output feeds the next stage as it is, and goes back into the host-shaped functions
    dK2, dB2, R2, obj2 = lsq.train_chainq_dev(dX, m, H, Rd, dB, 1, engine=engine)
    torch.cuda.synchronize()
    assert np.isfinite(obj2).all() and obj2[-1] <= obj2[0] * 1.001 and tuple(dK2.shape) == (m * H, d) and tuple(dB2.shape) == (n, m)
    Cl = lsq.codebooks_from_padded(dK, d, m)
    assert len(Cl) == m and Cl[0].shape == (d // m, H)
    dXr = (dX @ torch.from_numpy(Rd).cuda()).contiguous()
    assert np.array_equal(lsq.quantize_pq(np.ascontiguousarray(dXr.cpu().numpy().T), Cl, engine=engine).T.astype(np.int64) - 1, codes)
    Bq = lsq.quantize_opq(X, Rd, Cl, engine=engine)                  # rotates on the host: another BLAS, so a near-tie may fall the other way
    assert Bq.shape == (m, n) and np.mean(Bq.T.astype(np.int64) - 1 != codes) <= 1e-3


def test_rejections(lsq, engine):
    import torch
    LsqError, EINVAL = lsq._lib.LsqError, lsq._lib.LSQ_EINVAL
    rng = np.random.default_rng(1)
    n, d, m = 300, 8, 2
    X = rng.standard_normal((n, d)).astype(np.float32)
    B = rng.integers(1, H + 1, size=(n, m)).astype(np.int16)
    cover = kc.pq_cover(d, m)
    u = rng.random((m, H))
    dX, dB = torch.from_numpy(X).cuda(), torch.from_numpy((B - 1).astype(np.uint8)).cuda()

    def rejected(fn, name=None):
        with pytest.raises(LsqError) as e:
            fn()
        assert e.value.code == EINVAL and (name is None or name in str(e.value)), str(e.value)

    rejected(lambda: engine.update_centers(X, np.minimum(B, 16), cover, m, h=16), "lsq_update_centers")                      # h != 256
    rejected(lambda: engine.kmeanspp_seed(X, cover, rng.random((m, 16)), m, h=16), "lsq_kmeanspp_seed")
    c17 = np.zeros((34, 17), dtype=np.uint8)
    c17[np.arange(34), np.arange(34) // 2] = 1
    X34 = rng.standard_normal((n, 34)).astype(np.float32)
    rejected(lambda: engine.update_centers(X34, np.ones((n, 17), np.int16), c17, 17), "lsq_update_centers")                  # m > 16
    rejected(lambda: engine.kmeanspp_seed(X34, c17, rng.random((17, H)), 17), "lsq_kmeanspp_seed")
    empty = cover.copy()
    empty[:, 1] = 0
    rejected(lambda: engine.update_centers(X, B, empty, m), "covers no dimension")                                            # a codebook with an empty cover
    rejected(lambda: engine.update_centers_dev(dX, dB, empty, m), "lsq_update_centers_dev")
    rejected(lambda: engine.kmeanspp_seed(X, empty, u, m), "covers no dimension")
    rejected(lambda: engine.kmeanspp_seed_dev(dX, empty, u, m), "lsq_kmeanspp_seed_dev")
    two = cover.copy()
    two[0, 0] = 2
    rejected(lambda: engine.update_centers(X, B, two, m))
    for bad in (1.0, -1e-9, np.nan, 1.5):                                                                                    # u outside [0, 1)
        ub = u.copy()
        ub[1, 77] = bad
        rejected(lambda: engine.kmeanspp_seed(X, cover, ub, m), "outside [0, 1)")
        rejected(lambda: engine.kmeanspp_seed_dev(dX, cover, ub, m), "outside [0, 1)")
    with pytest.raises(LsqError) as e:                                                                                        # a code outside 1 .. h
        Bb = B.copy()
        Bb[3, 1] = 257
        engine.update_centers(X, Bb, cover, m)
    assert e.value.code == lsq._lib.LSQ_ECODE
    # the trainers: width-1 sub-spaces, n < h for OPQ's sampled start
    with pytest.raises(ValueError):
        lsq.train_pq_dev(dX, d, H, engine=engine)
    with pytest.raises(ValueError):
        lsq.train_opq_dev(dX, d, H, 1, engine=engine)
    with pytest.raises(ValueError):
        lsq.kmeans_dev(dX, H, engine=engine, dim2C=np.eye(d, dtype=np.uint8))
    with pytest.raises(ValueError):
        lsq.train_opq_dev(dX[:100].contiguous(), m, H, 1, engine=engine)
    with pytest.raises(ValueError):
        lsq.train_opq_dev(dX, m, H, 1, "other", engine=engine)
    # n = 0: empty outputs, no fault
    X0 = np.zeros((0, d), dtype=np.float32)
    K0, cnt0 = engine.update_centers(X0, np.zeros((0, m), np.int16), cover, m)
    assert K0.shape == (m * H, d) and not K0.any() and not cnt0.any()
    Kp = rng.standard_normal((m * H, d)).astype(np.float32)
    K0p, _ = engine.update_centers(X0, np.zeros((0, m), np.int16), cover, m, K_prev=Kp)
    assert np.array_equal(K0p, Kp * cover.T.repeat(H, axis=0))
    Ks, idx0, d20 = engine.kmeanspp_seed(X0, cover, u, m)
    assert d20.shape == (0, m) and not Ks.any() and (idx0 == -1).all()
    dKs, didx0, dd20 = engine.kmeanspp_seed_dev(dX[:0], cover, u, m, want_d2=True)
    torch.cuda.synchronize()
    assert tuple(dd20.shape) == (0, m) and not dKs.cpu().numpy().any() and (didx0.cpu().numpy() == -1).all()
    # and the context still works
    K1, _ = engine.update_centers(X, B, cover, m)
    assert np.array_equal(_bits(K1), _bits(kc.centers_exact(X, B.astype(np.int64) - 1, cover)[0]))
