"""CPU checks of tests/kmeans_check.py, the checker of the device cluster means and k-means++ seeding (csrc/lsq_kmeans.hip): its mean rule is the
shipped host arithmetic (initializers._centers) bit for bit, its seeding judge accepts a plain float64 run of the rule without one ambiguous step, and
the C-ABI lists the four new entries."""
import os
import re

import numpy as np
import pytest

import kmeans_check as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 256


@pytest.mark.parametrize("n,d,m,kind", [(20000, 5, 1, "random"), (3000, 16, 4, "random"), (1, 8, 2, "random"), (500, 7, 3, "one"), (100, 6, 2, "few"),
                                        (4000, 30, 4, "skew")])
@pytest.mark.parametrize("prev", [False, True])
def test_centers_exact_is_the_shipped_host_arithmetic(lsq, n, d, m, kind, prev):
    """centers_exact == initializers._centers(..., old=K_prev) bit for bit, per sub-space: random codes (n = 20 000 over 256 codes, and shapes with many
    empty clusters), one row, every row in one cluster, a skewed distribution.  With old=None the host re-seeds an empty cluster at random -- there the
    comparison covers the non-empty clusters and the checker's rows must be zero."""
    from importlib import import_module
    ini = import_module("local-search-quantization_amd.initializers")
    rng = np.random.default_rng(n + d + m)
    X = (rng.standard_normal((n, d)) * 3).astype(np.float32)
    if kind == "one":
        codes = np.full((n, m), 17, dtype=np.int64)
    elif kind == "few":
        codes = rng.integers(5, size=(n, m))
    elif kind == "skew":
        codes = np.minimum((rng.exponential(20.0, size=(n, m))).astype(np.int64), H - 1)
    else:
        codes = rng.integers(H, size=(n, m))
    cover = kc.pq_cover(d, m)
    K_prev = rng.standard_normal((m * H, d)).astype(np.float32) if prev else None
    K, counts = kc.centers_exact(X, codes, cover, H, K_prev)
    assert K.dtype == np.float32 and counts.dtype == np.int32
    for j in range(m):
        dims = np.nonzero(cover[:, j])[0]
        old = None if K_prev is None else np.ascontiguousarray(K_prev[j * H:(j + 1) * H][:, dims].T)
        want = ini._centers(np.ascontiguousarray(X[:, dims].T), codes[:, j], H, np.random.default_rng(0), old=old)      # (r, h)
        cnt = np.bincount(codes[:, j], minlength=H)
        assert np.array_equal(counts[j * H:(j + 1) * H], cnt)
        got = K[j * H:(j + 1) * H]
        nz = cnt > 0
        assert np.array_equal(got[np.ix_(nz, dims)].view(np.uint32), want.T[nz].view(np.uint32)), "sub-space %d: means differ" % j
        if prev:
            assert np.array_equal(got[np.ix_(~nz, dims)], want.T[~nz])
        else:
            assert not got[~nz].any()
        mask = np.ones(d, dtype=bool)
        mask[dims] = False
        assert not got[:, mask].any() and not np.signbit(got[:, mask]).any()


def test_centers_exact_on_overlapping_covers():
    """a chain cover: a dimension belongs to two codebooks, each averaging its own clusters over it"""
    rng = np.random.default_rng(5)
    n, d, m = 700, 12, 4
    X = rng.standard_normal((n, d)).astype(np.float32)
    codes = rng.integers(H, size=(n, m))
    cover = kc.chain_cover(d, m)
    assert cover.sum(axis=1).max() == 2
    K, counts = kc.centers_exact(X, codes, cover)
    for j in (0, m - 1):
        c = int(codes[0, j])
        rows = np.nonzero(codes[:, j] == c)[0]
        dims = np.nonzero(cover[:, j])[0]
        assert np.allclose(K[j * H + c, dims], X[rows][:, dims].astype(np.float64).mean(axis=0), rtol=1e-5, atol=1e-6)
        assert counts[j * H + c] == rows.size


@pytest.mark.parametrize("d,n,m", kc.SEED_PROBLEMS)
def test_judge_accepts_the_float64_rule_without_an_ambiguous_step(d, n, m):
    """The three seeding problems of the GPU test: a float64 run of the rule is accepted at every step, no target comes within the band of a boundary, and
    the 256 chosen rows are distinct."""
    X, cover, u = kc.seed_problem(d, n, m)
    idx, d2 = kc.seed_f64(X, cover, u)
    v = kc.judge_seeding(X, cover, u, idx)
    print("d=%d n=%d m=%d: smallest gap / total %.3g, band / total %.3g, ambiguous %d of %d" % (d, n, m, v["min_gap"], v["max_band"], v["ambiguous"], v["steps"]))
    assert v["bad"] == [] and v["ambiguous"] == 0 and v["zero_road"] == 0 and v["steps"] == m * (H - 1)
    assert v["min_gap"] > v["max_band"]
    assert np.array_equal(v["d2"], d2)
    for j in range(m):
        assert np.unique(idx[j]).size == H


def test_judge_rejects_a_wrong_row_and_follows_the_zero_road():
    X, cover, u = kc.seed_problem(16, 3000, 4)
    idx, _ = kc.seed_f64(X, cover, u)
    wrong = idx.copy()
    wrong[2, 100] = (wrong[2, 100] + 1500) % 3000
    assert kc.judge_seeding(X, cover, u, wrong)["bad"]
    wrong = idx.copy()
    wrong[1, 7] = wrong[1, 3]                                      # a row already chosen: distance 0
    assert any("distance 0" in b[2] for b in kc.judge_seeding(X, cover, u, wrong)["bad"])
    # fewer distinct points than steps: the total reaches 0 and the uniform rule takes over
    Xd = np.repeat(np.random.default_rng(3).standard_normal((10, 6)).astype(np.float32), 30, axis=0)
    c1 = np.ones((6, 1), dtype=np.uint8)
    u1 = np.random.default_rng(4).random((1, H))
    i1, d2 = kc.seed_f64(Xd, c1, u1)
    v = kc.judge_seeding(Xd, c1, u1, i1)
    assert v["bad"] == [] and v["zero_road"] >= H - 10 - 1 and not d2.any()
    assert np.unique(Xd[i1[0, :10]], axis=0).shape[0] == 10          # the ten distinct points first: no zero-distance row before the total is 0


def test_header_and_signatures_list_the_four_entries(lsq):
    hdr = open(os.path.join(ROOT, "include", "lsq_mi355x.h")).read()
    declared = set(re.findall(r"LSQ_API\s+[\w\s\*]*?\b(lsq_\w+)\s*\(", hdr))
    for name in ("lsq_update_centers", "lsq_update_centers_dev", "lsq_kmeanspp_seed", "lsq_kmeanspp_seed_dev"):
        assert name in declared, "%s is not declared in include/lsq_mi355x.h" % name
        assert name in lsq._lib.SIGNATURES, "%s is not in _lib.SIGNATURES" % name
    assert int(re.search(r"#define\s+LSQ_VERSION\s+(\d+)", hdr).group(1)) >= 1100
    assert lsq._lib.load().lsq_version() >= 1100
    for name in ("kmeans_dev", "train_pq_dev", "train_opq_dev", "codebooks_from_padded"):
        assert hasattr(lsq, name)


def test_host_trainers_take_explicit_initial_codebooks(lsq):
    """the additive `init=` keyword of kmeans / train_pq exists and checks its shape; nothing else about the host trainers changes"""
    import inspect
    ini = lsq.initializers
    assert inspect.signature(ini.kmeans).parameters["init"].default is None
    assert inspect.signature(ini.train_pq).parameters["init"].default is None
    with pytest.raises(ValueError):
        ini.kmeans(np.zeros((4, 300), np.float32), H, init=np.zeros((3, H), np.float32))
    C = [np.arange(2 * H, dtype=np.float32).reshape(2, H)] * 3 + [np.ones((2, H), np.float32)]
    K = ini._padded(C, 8, 4, H)
    back = lsq.codebooks_from_padded(K, 8, 4)
    assert all(np.array_equal(a, b) for a, b in zip(C, back))
