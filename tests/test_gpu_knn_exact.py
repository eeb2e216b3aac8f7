"""Exact k-NN on the device: lsq_knn_exact / lsq_knn_exact_dev (csrc/lsq_knn.hip under the selection of csrc/lsq_adc.hip) must return what the host
drop-in lsq_knn_exact_cpu and the numpy restatement return (tests/test_knn_exact.py pins those to the contract) -- distances as bits, 0-based ids,
tie and NaN order -- on every road of the selection (exhaustive, thresholded lists, the per-query fallback, both test hooks), at edge widths, with
row views offset by one float, and on the demo's synthetic data against an independent argmin."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import knn_check as KC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(seed, n, nq, d):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)


def _cpu(lsq, Xb, Xq, nn):
    rc, dists, ids = KC.knn_cpu(lsq._lib.load(), Xb, Xq, Xq.shape[1], nn)
    assert rc == 0
    return dists, ids


def _dev(eng, Xb, Xq, nn):
    dd, di = eng.knn_exact_dev(torch.from_numpy(Xb).cuda(), torch.from_numpy(Xq).cuda(), nn)
    torch.cuda.synchronize()
    return dd.cpu().numpy(), di.cpu().numpy().view(np.uint32)


def _same(d1, i1, d2, i2):
    assert np.array_equal(i1, i2), "ids differ at %s" % (np.argwhere(i1 != i2)[:5].tolist(),)
    assert KC.same_bits(d1, d2), "distances differ"


def _search(lsq, Xb, Xq, nn, expect=None, **options):
    with lsq.Engine(0) as eng:
        for k, v in options.items():
            eng.set_option(k, v)
        d, i = eng.knn_exact(Xb, Xq, nn)
        st = eng.linscan_stats()
    assert i.dtype == np.uint32 and i.max() < Xb.shape[0]
    for k, v in (expect or {}).items():
        assert st[k] == v, (k, st)
    return d, i, st


@pytest.mark.parametrize("d", [1, 3, 4, 127, 128, 129, 960, 1000])
def test_widths_match_cpu_and_numpy(lsq, d):
    Xb, Xq = _data(d, 3000, 17, d)
    d1, i1, st = _search(lsq, Xb, Xq, 10, expect=dict(exhaustive=1, queries=17, fallback_queries=0))
    assert st["lut_ms"] == 0.0
    _same(d1, i1, *_cpu(lsq, Xb, Xq, 10))
    _same(d1, i1, *KC.knn_np(Xb, Xq, 10))


@pytest.mark.parametrize("nq", [1, 17, 1000])
def test_query_counts(lsq, nq):
    Xb, Xq = _data(nq, 5000, nq, 32)
    d1, i1, _ = _search(lsq, Xb, Xq, 20)
    _same(d1, i1, *_cpu(lsq, Xb, Xq, 20))


def test_nn_equals_n(lsq):
    Xb, Xq = _data(11, 700, 9, 20)
    d1, i1, _ = _search(lsq, Xb, Xq, 700)
    _same(d1, i1, *KC.knn_np(Xb, Xq, 700))


def test_threshold_road(lsq):
    """10^5 rows: sample thresholds and candidate lists; every query served by its list"""
    Xb, Xq = _data(21, 100_000, 1000, 64)
    d1, i1, st = _search(lsq, Xb, Xq, 100, expect=dict(exhaustive=0, fallback_queries=0, queries=1000, codes=100_000))
    assert 100 * 1000 <= st["candidates"] < 1000 * st["list_capacity"]
    _same(d1, i1, *_cpu(lsq, Xb, Xq, 100))


def test_exhaustive_option(lsq):
    Xb, Xq = _data(22, 100_000, 64, 48)
    d1, i1, st = _search(lsq, Xb, Xq, 30, expect=dict(exhaustive=1, fallback_queries=0), linscan_exhaustive=1)
    assert st["candidates"] == 64 * 100_000
    _same(d1, i1, *_cpu(lsq, Xb, Xq, 30))


def test_rank_option_forces_the_fallback(lsq):
    """threshold rank 1: every list is shorter than nn, so every query is redone by the exhaustive road"""
    Xb, Xq = _data(23, 100_000, 40, 17)
    d1, i1, st = _search(lsq, Xb, Xq, 50, expect=dict(exhaustive=0, fallback_queries=40), linscan_rank=1)
    _same(d1, i1, *_cpu(lsq, Xb, Xq, 50))


@pytest.mark.parametrize("d", [4, 128, 129])
def test_views_offset_by_one_float(lsq, d):
    """rows d + 1 floats apart starting one float into the allocation: the 4-byte paths and the row strides"""
    n, nq, nn = 2000, 33, 25
    Xb, Xq = _data(30 + d, n, nq, d)
    sb = torch.full((1 + n * (d + 1),), float("nan"), device="cuda")
    sq = torch.full((1 + nq * (d + 1),), float("inf"), device="cuda")
    vb = sb[1:].view(n, d + 1)[:, :d]
    vq = sq[1:].view(nq, d + 1)[:, :d]
    vb.copy_(torch.from_numpy(Xb))
    vq.copy_(torch.from_numpy(Xq))
    assert vb.stride() == (d + 1, 1) and vb.data_ptr() % 16 != 0
    with lsq.Engine(0) as eng:
        dd, di = eng.knn_exact_dev(vb, vq, nn)
        torch.cuda.synchronize()
    _same(dd.cpu().numpy(), di.cpu().numpy().view(np.uint32), *_cpu(lsq, Xb, Xq, nn))


def test_ties_nan_and_inf_as_on_the_cpu(lsq):
    rng = np.random.default_rng(5)
    half = rng.integers(-4, 5, size=(500, 6)).astype(np.float32)
    Xb = np.concatenate([half, half, half[:100]])
    Xb[[3, 50]] = np.nan
    Xb[[7, 120], 2] = np.inf
    Xb[9, 0] = -np.inf
    Xq = rng.integers(-4, 5, size=(11, 6)).astype(np.float32)
    for nn in (1, 37, Xb.shape[0]):
        d1, i1, _ = _search(lsq, Xb, Xq, nn)
        _same(d1, i1, *_cpu(lsq, Xb, Xq, nn))
        _same(d1, i1, *KC.knn_np(Xb, Xq, nn))
    same = np.full((300, 4), 2.5, dtype=np.float32)
    _, i1, _ = _search(lsq, same, Xq[:, :4], 120)
    assert all(np.array_equal(i1[q], np.arange(120)) for q in range(Xq.shape[0]))


def test_deterministic_and_host_and_device_forms_agree(lsq):
    Xb, Xq = _data(40, 120_000, 300, 40)
    with lsq.Engine(0) as eng:
        d0, i0 = eng.knn_exact(Xb, Xq, 64)
        for _ in range(2):
            d1, i1 = eng.knn_exact(Xb, Xq, 64)
            _same(d0, i0, d1, i1)
            _same(d0, i0, *_dev(eng, Xb, Xq, 64))


def test_base_rows_find_themselves(lsq):
    Xb, _ = _data(50, 100_000, 1, 24)
    sel = np.random.default_rng(51).choice(Xb.shape[0], 500, replace=False)
    with lsq.Engine(0) as eng:
        dists, ids = _dev(eng, Xb, Xb[sel], 5)
    assert np.array_equal(ids[:, 0], sel.astype(np.uint32)) and (dists[:, 0] == 0).all()
    assert (dists[:, 1] > 0).all()


def test_demo_ground_truth_matches_an_independent_argmin(lsq, monkeypatch):
    """tools/demo_lsq_gpu.py's synthetic stand-in: its ground truth (knn_exact on the device) against a chunked float64 numpy argmin"""
    spec = importlib.util.spec_from_file_location("demo_lsq_gpu", os.path.join(ROOT, "tools", "demo_lsq_gpu.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    monkeypatch.delenv("LSQ_DATA_DIR", raising=False)
    name, _, xb, xq, gt = demo.load(3000, 6000, 200)
    assert name == "synthetic" and gt.dtype == np.uint32 and gt.shape == (200,)
    b64 = xb.T.astype(np.float64)
    want = np.empty(xq.shape[1], dtype=np.int64)
    for q0 in range(0, xq.shape[1], 50):
        q = xq[:, q0:q0 + 50].T.astype(np.float64)
        want[q0:q0 + 50] = ((b64[None, :, :] - q[:, None, :]) ** 2).sum(2).argmin(1)
    assert np.array_equal(gt.astype(np.int64) - 1, want)
