"""The PQ / OPQ scan on the device: lsq_linscan_pq / lsq_linscan_pq_dev (csrc/lsq_adc.hip) must return what the host drop-in lsq_linscan_aqd_query
returns (itself pinned to the reference build in tests/test_linscan_pq.py) -- distances as bits, 0-based ids, tie order -- on every road of the
selection: exhaustive (small databases), thresholded candidate lists, the per-query fallback, and both test hooks; and the stored reference
outputs on the fixture cases."""
import numpy as np
import pytest

from test_linscan_pq import FIXTURE_CASES, assert_same, drop_in, fixture_inputs, pq_case, reference_outputs

pytestmark = pytest.mark.gpu
H = 256


def _check(lsq, codes, centers, Q, m, subdim, K, expect=None, **options):
    dref, iref = drop_in(lsq, codes, centers, Q, m, subdim, K)
    with lsq.Engine(0) as eng:
        for k, v in options.items():
            eng.set_option(k, v)
        d, i = eng.linscan_pq(codes, Q, centers, m, K, subdim)
        st = eng.linscan_stats()
    assert i.dtype == np.uint32 and i.max() < codes.shape[0]
    assert_same(d, i, dref, iref)
    if expect is not None:
        for k, v in expect.items():
            assert st[k] == v, (k, st)
    return st


@pytest.mark.parametrize("name", sorted(FIXTURE_CASES))
def test_fixture_cases_match_the_reference_build(lsq, name):
    n, nq, m, subdim, dc, dq, K, kind = FIXTURE_CASES[name]
    codes, centers, Q = fixture_inputs(name)
    dref, iref = reference_outputs(name)
    with lsq.Engine(0) as eng:
        d, i = eng.linscan_pq(codes, Q, centers, m, K, subdim)
        st = eng.linscan_stats()
    assert_same(d, i, dref, iref)
    assert st["exhaustive"] == 1 and st["queries"] == nq, st


@pytest.mark.parametrize("m", [1, 3, 4, 8, 12, 16])
def test_thresholded_lists_every_code_width(lsq, m):
    """n ~ 3e5: the sampled threshold and candidate lists; m = 4, 8, 12, 16 read codes as dwords, 1 and 3 as bytes"""
    n, nq, subdim, K = 300_000 + 17 * m, 21, 4, 100
    codes, centers, Q = pq_case(900 + m, n, nq, m, subdim, m, m * subdim)
    st = _check(lsq, codes, centers, Q, m, subdim, K, expect={"exhaustive": 0, "queries": nq})
    assert st["fallback_queries"] == 0 and st["candidates"] < 0.25 * n * nq, st


@pytest.mark.parametrize("m,dc,dq_extra", [(8, 11, 3), (4, 8, 0), (3, 3, 9)])
def test_strided_codes_and_queries(lsq, m, dc, dq_extra):
    """dim1codes > m (the byte path, rows dc bytes apart) and dim1queries > m * subdim, on both roads"""
    subdim = 5
    for n, nq, K in ((40_000, 9, 50), (150_001, 13, 30)):
        codes, centers, Q = pq_case(n + dc, n, nq, m, subdim, dc, m * subdim + dq_extra)
        _check(lsq, codes, centers, Q, m, subdim, K, expect={"exhaustive": int(n <= 65536)})


def test_sampled_entries_far_away_fall_back(lsq):
    """every entry the strided sample looks at is far from every query: the thresholds sit above everything unsampled, the lists overflow,
    every query takes the exhaustive road"""
    n, nq, m, subdim, K = 160_000, 12, 8, 4, 200
    codes, centers, Q = pq_case(13, n, nq, m, subdim, m, m * subdim)
    centers[:, 255] += np.float32(1.0e3)
    codes[codes == 255] = 254
    codes[:: n // 16384] = 255
    st = _check(lsq, codes, centers, Q, m, subdim, K)
    assert st["fallback_queries"] == nq, st


def test_clustered_database_is_still_exact(lsq):
    """a database sorted by its first code byte: near neighbours in long runs, the sample is not exchangeable"""
    n, nq, m, subdim, K = 200_000, 10, 4, 6, 500
    codes, centers, Q = pq_case(14, n, nq, m, subdim, m, m * subdim)
    codes = np.ascontiguousarray(codes[np.lexsort(codes.T[::-1])])
    _check(lsq, codes, centers, Q, m, subdim, K, expect={"exhaustive": 0})


def test_massive_ties_fall_back_in_id_order(lsq):
    n, nq, m, subdim, K = 80_000, 9, 8, 2, 30
    codes, centers, Q = pq_case(15, n, nq, m, subdim, m, m * subdim)
    codes[:] = codes[0]
    st = _check(lsq, codes, centers, Q, m, subdim, K, expect={"fallback_queries": nq})
    with lsq.Engine(0) as eng:
        _, i = eng.linscan_pq(codes, Q, centers, m, K, subdim)
    assert np.array_equal(i, np.tile(np.arange(K, dtype=np.uint32), (nq, 1))), st


def test_test_hooks(lsq):
    """linscan_exhaustive = 1 forces the exhaustive road; linscan_rank = 1 (threshold = the sample's minimum) makes every list short -> fallback"""
    n, nq, m, subdim, K = 100_000, 18, 8, 3, 300
    codes, centers, Q = pq_case(16, n, nq, m, subdim, m, m * subdim, kind="dup")
    _check(lsq, codes, centers, Q, m, subdim, K, expect={"exhaustive": 1, "fallback_queries": 0}, linscan_exhaustive=1)
    _check(lsq, codes, centers, Q, m, subdim, K, expect={"exhaustive": 0, "fallback_queries": nq}, linscan_rank=1)
    _check(lsq, codes, centers, Q, m, subdim, K, expect={"exhaustive": 0, "fallback_queries": 0})


def test_device_tensors_on_the_torch_stream_and_stats(lsq):
    import torch
    n, nq, m, subdim, K = 120_000, 40, 8, 16, 100
    codes, centers, Q = pq_case(17, n, nq, m, subdim, m, m * subdim)
    dref, iref = drop_in(lsq, codes, centers, Q, m, subdim, K)
    dev = torch.device("cuda:0")
    dC, dQ, dK = torch.from_numpy(codes).to(dev), torch.from_numpy(Q).to(dev), torch.from_numpy(centers).to(dev)
    side = torch.cuda.Stream(device=dev)
    with lsq.Engine(0, profile=True) as eng:
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            d, i = eng.linscan_pq_dev(dC, dQ, dK, m, K, subdim)
            d2, i2 = eng.linscan_pq_dev(dC[:50_000], dQ, dK, m, K, subdim)
        side.synchronize()
        st = eng.linscan_stats()
        assert_same(d.cpu().numpy(), i.cpu().numpy().view(np.uint32), dref, iref)
        assert_same(d2.cpu().numpy(), i2.cpu().numpy().view(np.uint32), *drop_in(lsq, codes[:50_000], centers, Q, m, subdim, K))
        assert st["queries"] == 2 * nq and st["codes"] == 50_000 and st["exhaustive"] == 1 and st["batches"] >= 2, st
        assert st["scan_ms"] > 0 and st["lut_ms"] > 0 and st["select_ms"] > 0, st
        # Julia shapes through the reference-shaped wrapper, on the device
        C = [np.ascontiguousarray(centers[k].T) for k in range(m)]
        dj, rj = lsq.linscan_pq(codes.T, Q.T, C, 8 * m, K, engine=eng)
    assert np.array_equal(rj.T, iref + 1) and np.array_equal(dj.T.view(np.uint32), dref.view(np.uint32))


def test_more_than_16_subspaces_is_refused(lsq):
    codes, centers, Q = pq_case(18, 1000, 2, 17, 2, 17, 34)
    with lsq.Engine(0) as eng:
        with pytest.raises(lsq._lib.LsqError) as e:
            eng.linscan_pq(codes, Q, centers, 17, 10, 2)
        assert e.value.code == lsq._lib.LSQ_EINVAL and "16" in str(e.value)
        assert eng.linscan_stats()["queries"] == 0


def _clustered(d, n, k, seed, spread=0.35):
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((d, k)).astype(np.float32) * 3.0
    a = rng.integers(k, size=n)
    return (cen[:, a] + spread * rng.standard_normal((d, n))).astype(np.float32)


# recall of the true nearest neighbour on the data below.  First run on an MI355X: PQ r@10 0.150, r@100 1.000; OPQ r@10 0.140, r@100 1.000.
# The clusters are tighter than a sub-space codebook resolves, so a cluster's points share codes and rank among themselves by id: r@1 is chance
# within a cluster, r@10 far above the 10 / 30 000 of a random ranking.  Bounds with room below the measured values:
RECALL_AT_10, RECALL_AT_100 = 0.05, 0.95


@pytest.mark.parametrize("flavour", ["pq", "opq"])
def test_demo_flow_on_synthetic_data(lsq, flavour):
    """demos/demo_pq.jl / demo_opq.jl on seeded clustered data: train -> quantize the base -> linscan -> eval_recall against float64 brute force"""
    d, m, ntrain, nbase, nq, knn = 32, 4, 4000, 30_000, 100, 100
    b = 8 * m
    allx = _clustered(d, ntrain + nbase + nq, k=500, seed=21)
    x_train, x_base, x_query = allx[:, :ntrain], allx[:, ntrain:ntrain + nbase], allx[:, ntrain + nbase:]
    if flavour == "pq":
        C, B, err = lsq.train_pq(x_train, m, H, seed=3)
        B_base = lsq.quantize_pq(x_base, C)
        search = lambda eng: lsq.linscan_pq((B_base - 1).astype(np.uint8), x_query, C, b, knn, engine=eng)        # noqa: E731
    else:
        C, B, R, obj = lsq.train_opq(x_train, m, H, 4, "natural", seed=3)
        B_base = lsq.quantize_opq(x_base, R, C)
        search = lambda eng: lsq.linscan_opq((B_base - 1).astype(np.uint8), x_query, C, b, R, knn, engine=eng)     # noqa: E731
    dists, idx = search(None)
    with lsq.Engine(0) as eng:
        dists_d, idx_d = search(eng)
    assert idx.shape == (knn, nq) and idx.dtype == np.uint32 and idx.min() >= 1 and idx.max() <= nbase
    assert np.array_equal(idx_d, idx) and np.array_equal(dists_d.view(np.uint32), dists.view(np.uint32))
    xb, xq = x_base.astype(np.float64), x_query.astype(np.float64)
    d2 = (xb ** 2).sum(0)[:, None] - 2.0 * xb.T @ xq + (xq ** 2).sum(0)[None, :]
    gt = (d2.argmin(0) + 1).astype(np.uint32)
    rec = lsq.eval_recall(gt, idx, knn)
    print("%s recall@1 %.3f @10 %.3f @100 %.3f" % (flavour, rec[0], rec[9], rec[99]))
    assert rec[99] >= RECALL_AT_100 and rec[9] >= RECALL_AT_10, rec[[0, 9, 99]]
    assert np.all(np.diff(rec) >= 0)
