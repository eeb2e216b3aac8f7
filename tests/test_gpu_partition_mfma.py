"""Partition.assign on the matrix cores (option "partition_mfma", csrc/lsq_passign.hip): in every case the option-on call, the option-off call on the same
Partition and partition_check.assign_np agree bit for bit on ids and distances, at the smallest shapes at which the new kernels can go wrong."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import partition_check as pc  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture
def eng(engine):
    yield engine
    engine.set_option("partition_mfma", 0)
    engine.set_option("partition_mfma_cap", 0)


def to_dev(torch, v):
    """a numpy row view -> the torch view of the same geometry on the device"""
    buf = v
    while buf.base is not None:
        buf = buf.base
    first, p = (v.ctypes.data - buf.ctypes.data) // v.itemsize, pc.pitch(v)
    return torch.from_numpy(buf).cuda()[first:first + v.shape[0] * p].view(v.shape[0], p)[:, :v.shape[1]]


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def on_and_off(eng, part, X, cap=0):
    """-> (ids, dist, account) of the option-on assign, held to the option-off assign of the same Partition"""
    eng.set_option("partition_mfma", 0)
    want, wdist = part.assign(X, want_dist=True)
    assert part.mfma_info()["served"] == 0
    eng.set_option("partition_mfma", 1)
    eng.set_option("partition_mfma_cap", cap)
    got, dist = part.assign(X, want_dist=True)
    info = part.mfma_info()
    assert np.array_equal(host(part.assign(X)), host(got))                               # without the distances: the same ids
    eng.set_option("partition_mfma", 0)
    assert np.array_equal(host(got), host(want)) and pc.same(host(dist), host(wdist)), info
    assert info["served"] == 1 and info["rows"] == X.shape[0] and info["nlist"] == part.nlist and info["redo_rows"] <= X.shape[0]
    return host(got), host(dist), info


def problem(nlist, n, d, u8, seed):
    """assign_problem's values (offset data) at any nlist: the last centroid repeats the first (an exact tie), row 0 equals a centroid (distance +0.0)"""
    rng = np.random.default_rng(seed)
    cent = (rng.standard_normal((nlist, d)) * 40 + 128).astype(np.float32)
    X = (rng.standard_normal((n, d)) * 40 + 128).astype(np.float32)
    if u8:
        cent, X = np.floor(np.clip(cent, 0, 254)), np.floor(np.clip(X, 0, 254))
    cent[-1] = cent[0]
    X[0] = cent[nlist // 2]
    X[-1] = cent[0] + np.float32(1)
    return cent, (X.astype(np.uint8) if u8 else X)


def test_the_option_name(eng):
    eng.set_option("partition_mfma", 1)
    eng.set_option("partition_mfma_cap", 7)


@pytest.mark.parametrize("d", [1, 8, 15, 16, 17, 130, 256, 257])
@pytest.mark.parametrize("nlist,n", [(1, 129), (127, 1), (128, 2000), (129, 129), (300, 2000), (300, 1)])
def test_shape_edges(eng, torch, nlist, n, d):
    for u8 in (False, True):
        cent, X = problem(nlist, n, d, u8, 1000 * nlist + 10 * n + d)
        ref, acc = pc.assign_np(X, cent)
        view = pc.row_view(X, 1, offset=3) if u8 else pc.row_view(X, 3, offset=1)          # pitched; uint8 at an odd byte offset
        with eng.partition_dev(torch.from_numpy(cent).cuda()) as part, eng.partition(cent) as hpart:
            for p, rows in ((part, to_dev(torch, X)), (part, to_dev(torch, view)), (hpart, X), (hpart, view)):
                got, dist, info = on_and_off(eng, p, rows)
                assert np.array_equal(got, ref) and pc.same(dist, acc[np.arange(n), ref]), (u8, info)
                assert info["resident"] == int((d + 15) // 16 * 16 <= 256) and info["switched_off"] == 0 and info["pairs"] == n * nlist, info
                assert info["pending"] >= n - info["nonfinite_rows"] and info["nonfinite_rows"] == 0, info


@pytest.mark.parametrize("u8", [False, True])
def test_centroid_split_at_65537_lists(eng, torch, u8):
    n = 200
    cent, X = pc.assign_problem(65537, u8, n=n)
    ref, acc = pc.assign_np(X, cent)
    with eng.partition_dev(torch.from_numpy(cent).cuda()) as part:
        got, dist, info = on_and_off(eng, part, torch.from_numpy(X).cuda())
    assert np.array_equal(got, ref) and pc.same(dist, acc[np.arange(n), ref])
    assert got[n // 2] == pc.TIE[0] and got[7] == 123 and dist[7] == 0 and not np.signbit(dist[7])
    assert info["splits"] > 1 and info["switched_off"] == 0, info


@pytest.mark.parametrize("d", [16, 130])
def test_float64_reference(eng, torch, d):
    """|f - D| <= gamma_{d+3} D for the chain and f_assigned <= f_c for every c:  D64(assigned) <= D64(min) (1 + gamma) / (1 - gamma)"""
    rng = np.random.default_rng(d)
    cent, X = rng.standard_normal((300, d)).astype(np.float32), rng.standard_normal((500, d)).astype(np.float32)
    with eng.partition_dev(torch.from_numpy(cent).cuda()) as part:
        got, _, info = on_and_off(eng, part, torch.from_numpy(X).cuda())
    D = np.stack([((cent.astype(np.float64) - x) ** 2).sum(1) for x in X.astype(np.float64)])
    g = (d + 3) * U / (1 - (d + 3) * U)
    assert np.all(D[np.arange(500), got] <= D.min(1) * (1 + g) / (1 - g) * (1 + 1e-12)) and info["redo_rows"] == 0, info


@pytest.mark.parametrize("special_centroids", [False, True])
def test_non_finite_values(eng, torch, special_centroids):
    cent, X = problem(300, 2000, 4, False, 5)
    pc.special_rows(X, cent if special_centroids else cent.copy(), 9)                   # in place
    ref, acc = pc.assign_np(X, cent)
    with eng.partition_dev(torch.from_numpy(cent).cuda()) as part:
        got, dist, info = on_and_off(eng, part, torch.from_numpy(X).cuda())
    assert np.array_equal(got, ref) and pc.same(dist, acc[np.arange(2000), ref])
    with np.errstate(all="ignore"):
        bad = int((~np.isfinite((X.astype(np.float64) ** 2).sum(1).astype(np.float32))).sum())
    assert 0 < bad < 1000 and info["nonfinite_rows"] == bad, (bad, info)
    if not special_centroids:
        assert info["switched_off"] == 0 and info["redo_rows"] == bad + info["overflow_rows"], info


def test_overflowing_rows_are_redone(eng, torch):
    """40 000 centroids with the same bits tie exactly at the minimum of the first 100 rows: every one of them is a candidate, whatever the capacity"""
    cent, X = pc.duplicated_centroids()
    ref, acc = pc.assign_np(X, cent)
    assert np.all(ref[:100] == 5000) and np.all(pc.keys(acc[:100, 5000:45000]) == pc.keys(acc[np.arange(100), ref[:100]])[:, None])
    with eng.partition_dev(torch.from_numpy(cent).cuda()) as part:
        got, dist, info = on_and_off(eng, part, torch.from_numpy(X).cuda())
    assert np.array_equal(got, ref) and pc.same(dist, acc[np.arange(300), ref])
    assert info["cap"] < 40000 and info["splits"] > 1 and 100 <= info["overflow_rows"] <= info["redo_rows"], info


def test_capacity_one_switches_the_road_off(eng, torch):
    """every part of the centroids holds a candidate of every row -- its own nearest --, so with two parts or more every row exceeds a capacity of one"""
    rng = np.random.default_rng(3)
    cent, X = rng.standard_normal((300, 16)).astype(np.float32), rng.standard_normal((2000, 16)).astype(np.float32)
    with eng.partition_dev(torch.from_numpy(cent).cuda()) as part:
        got, _, info = on_and_off(eng, part, torch.from_numpy(X).cuda(), cap=1)
    assert np.array_equal(got, pc.assign_np(X, cent)[0])
    assert info["splits"] >= 2 and info["cap"] == 1 and info["overflow_rows"] > 1000 and info["switched_off"] == 1, info


def test_a_large_common_offset(eng, torch):
    rng = np.random.default_rng(4)
    cent, X = (rng.standard_normal((300, 128)) + 1000).astype(np.float32), (rng.standard_normal((500, 128)) + 1000).astype(np.float32)
    with eng.partition_dev(torch.from_numpy(cent).cuda()) as part:
        got, _, _ = on_and_off(eng, part, torch.from_numpy(X).cuda())
    assert np.array_equal(got, pc.assign_np(X, cent)[0])


def test_the_followers(lsq, eng, torch):
    dX = torch.from_numpy(np.random.default_rng(6).standard_normal((3000, 16)).astype(np.float32)).cuda()
    out = []
    for on in (0, 1):
        eng.set_option("partition_mfma", on)
        part, dassign = lsq.train_coarse_dev(dX, 40, niter=3, engine=eng)
        with part:
            out.append((part.centroids().cpu().numpy(), dassign.cpu().numpy(), part.mfma_info()["served"]))
            if on:                                                                       # an update between two assigns is seen by the second one
                part.update(dX, torch.zeros(3000, dtype=torch.int32, device="cuda") + 39)
                assert np.array_equal(part.assign(dX).cpu().numpy(), pc.assign_np(dX.cpu().numpy(), part.centroids().cpu().numpy())[0])
    assert pc.same(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and (out[0][2], out[1][2]) == (0, 1)
