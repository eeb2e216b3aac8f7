"""Exact k-NN of 8-bit sets on the i8 matrix cores (option "knn_u8_mfma"; csrc/lsq_knnu.hip): with the option on, Index.knn on uint8 rows and uint8
queries must return the ids and distance bits of exact integer arithmetic -- D = N_x + N_q - 2 X Q^T, ranked by (D, id), dist = float32(D) -- and of the
same call with the option off (the dot4 road), with the SAME number of fallback queries: a kernel that emitted nothing would otherwise hide behind the
fallback.  n = 70 001 is past the exhaustive limit and ragged in 128-row tiles and in the last block range; the widths are the edges of the 16-byte
operand, the 32-byte K step, the 64-byte chunk and the contract's last d."""
import numpy as np
import pytest
import torch

import index_knn_check as IK

pytestmark = pytest.mark.gpu
N = 70001
NOT_ASKED, NOT_INTEGER_ROAD, FILTERED, EXHAUSTIVE = 1, 2, 3, 4


def _reference(Xb, Xq, nn):
    """-> dists (nq, nn) f32, ids (nq, nn) from exact integers: float64 products of bytes summed over d <= 258 are exact; key = D << 17 | id"""
    X, Q = Xb.astype(np.float64), Xq.astype(np.float64)
    D = ((X * X).sum(1)[None, :] + (Q * Q).sum(1)[:, None] - 2.0 * (Q @ X.T)).astype(np.int64)
    key = np.sort(np.partition((D << 17) | np.arange(Xb.shape[0]), nn - 1, axis=1)[:, :nn], axis=1)
    return (key >> 17).astype(np.float32), (key & ((1 << 17) - 1)).astype(np.uint32)


def _both(lsq, Xb, Xq, nn, base=None, Q=None, fallback_cap=None):
    """Index.knn with the option on, checked against the option-off call on the same engine and against the reference"""
    base = torch.tensor(Xb).cuda() if base is None else base
    Q = torch.tensor(Xq).cuda() if Q is None else Q
    n, nq = Xb.shape[0], Xq.shape[0]
    got = []
    with lsq.Engine(0) as eng, eng.index_dev(None, None, None, 0, base=base, d=Xb.shape[1]) as ix:
        for on in (0, 1):
            eng.set_option("knn_u8_mfma", on)
            d, i = ix.knn(Q, nn)
            torch.cuda.synchronize()
            got.append((d.cpu().numpy(), i.cpu().numpy(), ix.knn_info(), ix.knn_mfma_info()))
    (d0, i0, st0, mf0), (d1, i1, st1, mf1) = got
    print("fallback_queries off/on:", st0["fallback_queries"], st1["fallback_queries"], "account:", mf1)
    assert mf0["served"] == 0 and mf0["reason"] == NOT_ASKED and st0["int_road"] == 1 and st1["int_road"] == 1
    assert mf1["served"] == 1 and mf1["pairs"] == n * nq, mf1
    assert st1["fallback_queries"] == st0["fallback_queries"] and st1["exhaustive"] == 0
    assert mf1["kept"] >= (nq - st1["fallback_queries"]) * nn, (mf1, st1)
    if fallback_cap is not None:
        assert st0["fallback_queries"] <= fallback_cap, st0
    IK.same(d1, i1, d0, i0)
    IK.same(d1, i1, *_reference(Xb, Xq, nn))


# a rotation over the widths, not a product: every nq and every nn meets several widths
WIDTHS = [1, 15, 16, 17, 63, 64, 65, 128, 129, 258]
SHAPES = [(d, (1, 127, 129)[k % 3], (1, 50, 1000)[(k + k // 3) % 3]) for k, d in enumerate(WIDTHS)]


@pytest.mark.parametrize("d,nq,nn", SHAPES)
def test_uniform_bytes(lsq, d, nq, nn):
    Xb, Xq = IK.u8_data(2800 + d, N, nq, d)
    _both(lsq, Xb, Xq, nn, fallback_cap=nq // 8 if d >= 3 else None)      # (d < 3: a handful of distinct distances, every list overflows)


@pytest.mark.parametrize("case", ["rows_00", "rows_ff", "rows_80", "duplicates"])
def test_corner_data(lsq, case):
    """rows_00 / rows_ff: 30 constant rows (fewer than nn: all of them are answers) against queries of all 0x00 and of all 0xFF -- D = 0 through the -128 * -128 (127 * 127) products, and the
    largest D of the width; rows_80: rows that are zero after the shift, as the padding is, and the nearest rows of every query; duplicates: ties by id"""
    d, nq, nn = 65, 8, 50
    Xb, Xq = IK.u8_data(77, N, nq, d)
    if case == "duplicates":
        Xb = np.ascontiguousarray(np.resize(Xb[:7001], (N, d)))
    else:
        Xb[np.random.default_rng(3).choice(N, 30, replace=False)] = {"rows_00": 0x00, "rows_ff": 0xFF, "rows_80": 0x80}[case]
    if case in ("rows_00", "rows_ff"):
        Xq[0::2], Xq[1::2] = 0x00, 0xFF
    _both(lsq, Xb, Xq, nn)


@pytest.mark.parametrize("ldb,offb,ldq,offq", [(67, 1, 65, 0), (65, 0, 72, 4), (70, 3, 69, 2)])
def test_pitched_base_and_queries(lsq, ldb, offb, ldq, offq):
    """the byte loader (a pitch that is no multiple of 4, a base pointer at an odd byte) and the dword loader on padded rows; the padding is 255"""
    d, nq = 65, 5
    Xb, Xq = IK.u8_data(5, N, nq, d)
    tb, tq = torch.from_numpy(IK.laid_out(Xb, ldb, offb)[1]).cuda(), torch.from_numpy(IK.laid_out(Xq, ldq, offq)[1]).cuda()
    base, Q = torch.as_strided(tb, Xb.shape, (ldb, 1), storage_offset=offb), torch.as_strided(tq, Xq.shape, (ldq, 1), storage_offset=offq)
    assert base.data_ptr() % 4 == offb % 4
    _both(lsq, Xb, Xq, 10, base=base, Q=Q)


@pytest.mark.parametrize("why", ["d259", "filter", "small_n", "widened"])
def test_roads_not_served(lsq, why):
    d, n, want = (259, 1000, NOT_INTEGER_ROAD) if why == "d259" else (32, 1000, {"filter": FILTERED, "small_n": EXHAUSTIVE, "widened": NOT_INTEGER_ROAD}[why])
    Xb, Xq = IK.u8_data(9, n, 7, d)
    res = []
    with lsq.Engine(0) as eng, eng.index_dev(None, None, None, 0, base=torch.tensor(Xb).cuda()) as ix:
        eng.set_option("knn_u8_int", 0 if why == "widened" else 1)
        if why == "filter":
            ix.set_filter(mask=torch.arange(n).cuda() % 3 != 0, road="dense")
        for on in (0, 1):
            eng.set_option("knn_u8_mfma", on)
            dd, ii = ix.knn(torch.tensor(Xq).cuda(), 10)
            res.append((dd.cpu().numpy(), ii.cpu().numpy()))
            mf = ix.knn_mfma_info()
            assert mf["served"] == 0 and mf["pairs"] == 0 and mf["reason"] == (want if on else NOT_ASKED), mf
        eng.set_option("knn_u8_mfma", 2)                # as "knn_prefilter": any non-zero value asks
        ix.knn(torch.tensor(Xq).cuda(), 10)
        assert ix.knn_mfma_info()["reason"] == want
    IK.same(*res[1], *res[0])


def test_knn_exact_passes_the_option(lsq):
    Xb, Xq = IK.u8_data(11, N, 5, 16)
    want_d, want_i = _reference(Xb, Xq, 10)
    with lsq.Engine(0) as eng:
        dists, ids = lsq.knn_exact(Xb.T, Xq.T, 10, engine=eng, u8_mfma=True)
    IK.same(dists.T, ids.T - np.uint32(1), want_d, want_i)
