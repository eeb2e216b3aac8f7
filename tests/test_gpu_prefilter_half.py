"""The pre-filter of exact k-NN on half-precision rows (options "knn_prefilter" + "knn_prefilter_half"; csrc/lsq_knnh.hip) only decides which pairs deserve
the direct chain: Index.knn with both options on returns the bits, the ids, the tie order and the statistics of the same call with both off, and of the host
checker lsq_knn_exact_cpu on the widened rows -- at the operand, K-step and chunk edges of both formats, where the window is wide or decides nothing, where
lists overflow, on views the 16-byte loader cannot take, and on the roads it does not serve."""
import numpy as np
import pytest
import torch

import knn_check as KC

pytestmark = pytest.mark.gpu
N = 70_001                                   # above the exhaustive limit of 65 536; 547 row tiles, the last one ragged
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "uint8": torch.uint8}


def _gauss(d, n=N, nq=130):
    rng = np.random.default_rng(3100 + d)
    return rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)


def _run(lsq, rows, Q, nn, on, mask=None, only_half=False, **options):
    """Index.knn over device rows -> dists, ids, knn_info, the 4.29 account, the 16-bit tile's account"""
    with lsq.Engine(0) as eng:
        eng.set_option("knn_prefilter", int(on and not only_half))
        eng.set_option("knn_prefilter_half", int(on))
        for k, v in options.items():
            eng.set_option(k, v)
        with eng.index_dev(None, None, None, 0, base=rows) as ix:
            if mask is not None:
                ix.set_filter(mask=torch.from_numpy(mask).cuda(), road="dense")
            d, i = ix.knn(Q, nn)
            out = (d.cpu().numpy(), i.cpu().numpy().view(np.uint32), ix.knn_info(), ix.knn_prefilter_info(), ix.knn_prefilter_half_info())
        torch.cuda.synchronize()
    return out


def _same(a, b):
    assert np.array_equal(a[1], b[1]), "ids differ at %s" % (np.argwhere(a[1] != b[1])[:5].tolist(),)
    assert KC.same_bits(a[0], b[0]), "distances differ"
    assert a[2]["fallback_queries"] == b[2]["fallback_queries"] and a[2]["exhaustive"] == b[2]["exhaustive"]


def _both(lsq, rows, Q, nn, cpu=True, **options):
    """both options off, both on: identical; and (cpu) the host checker on the widened rows"""
    off, on = _run(lsq, rows, Q, nn, 0, **options), _run(lsq, rows, Q, nn, 1, **options)
    _same(off, on)
    if cpu:
        wide, q = rows.float().cpu().numpy(), Q.cpu().numpy()
        rc, cd, ci = KC.knn_cpu(lsq._lib.load(), wide, q, q.shape[1], nn)
        assert rc == 0 and np.array_equal(ci, on[1]) and KC.same_bits(cd, on[0])
    return off, on


@pytest.mark.parametrize("nq,nn", [(37, 1), (37, 100), (130, 1), (130, 100)])
@pytest.mark.parametrize("fmt", ["f16", "bf16"])
@pytest.mark.parametrize("d", [1, 7, 8, 9, 15, 16, 17, 31, 33, 64, 129, 130])
def test_identity_on_gaussian_rows(lsq, d, fmt, nq, nn):
    Xb, Xq = _gauss(d)
    rows, Q = torch.from_numpy(Xb).cuda().to(TORCH[fmt]), torch.from_numpy(Xq[:nq]).cuda()
    off, on = _both(lsq, rows, Q, nn)
    info = on[4]
    print(d, fmt, nq, nn, info)
    assert info["served"] == 1 and info["reason"] == 0 and info["switched_off"] == 0 and info["overflow_queries"] == 0
    assert info["format"] == (lsq._lib.BASE_F16 if fmt == "f16" else lsq._lib.BASE_BF16) and info["pieces"] == (3 if fmt == "f16" else 2)
    assert info["pairs"] == N * nq and info["pending"] >= info["kept"] >= nq * nn
    kappa, eta = lsq.knn_prefilter_half_bound(d, fmt)
    assert info["kappa"] == float(kappa) and info["eta"] == float(eta) and off[4]["served"] == 0
    # `candidates`: what the direct scan appends for the same queries is what the recheck kept (the 4.29 road on the same rows counts it the same way)
    with lsq.Engine(0) as eng:
        eng.set_option("knn_prefilter", 1)
        with eng.index_dev(None, None, None, 0, base=rows) as ix:
            ix.knn(Q, nn)
            assert ix.knn_prefilter_info()["kept"] == info["kept"] and ix.knn_prefilter_half_info()["reason"] == lsq._lib.KNN_PREFILTER_HALF_NOT_ASKED


def _near(Xb, Xq, fmt):                      # queries = stored rows a few f32 ulps away, under large norms: cancellation, and tau at a tie
    Xb *= np.float32(200)
    w = torch.from_numpy(Xb[:130]).to(TORCH[fmt]).float().numpy()
    Xq[:] = w
    for _ in range(3):
        Xq[:, ::2] = np.nextafter(Xq[:, ::2], np.float32(np.inf))
    return Xb, Xq


def _duplicates(Xb, Xq, fmt):
    Xb[5000:7000] = Xq[0] + np.float32(0.01)
    Xb[20_000:20_300] = Xb[3]
    return Xb, Xq


def _wide(Xb, Xq, fmt):                      # components spanning 2^-40 .. 2^20 (f16 rows turn the ends into 0 and inf)
    rng = np.random.default_rng(5)
    return (np.ldexp(Xb, rng.integers(-40, 21, Xb.shape)).astype(np.float32), np.ldexp(Xq, rng.integers(-40, 21, Xq.shape)).astype(np.float32))


def _tiny(Xb, Xq, fmt):
    return Xb * np.float32(1e-20), Xq * np.float32(1e-20)


def _offset(Xb, Xq, fmt):
    return Xb + np.float32(1000), Xq + np.float32(1000)


def _nonfinite(Xb, Xq, fmt):
    Xb[[3, 50, 69_999]] = np.nan
    Xb[[7, 120], 2] = np.inf
    Xb[9, 0] = -np.inf
    Xb[11] = 0.0
    Xb[12] = -0.0
    Xq[5, 1] = np.nan
    Xq[6, 0] = np.inf
    Xq[7, 3] = -np.inf
    Xq[8] = -0.0
    return Xb, Xq


def _f16_edges(Xb, Xq, fmt):                 # the largest f16 and f16 subnormals (bf16 rows round them; the result must still be the direct road's)
    Xb[100:200, ::3] = np.float32(65504)
    Xb[200:300, 1::3] = np.float32(-65504)
    Xb[300:2300] = np.ldexp(Xb[300:2300], -20)
    Xq[1] = np.ldexp(Xq[1], -20)
    Xq[2, ::3] = np.float32(65504)
    return Xb, Xq


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
@pytest.mark.parametrize("case", [_near, _duplicates, _wide, _tiny, _offset, _nonfinite, _f16_edges, "pitched", "odd_view", "cap4"])
def test_where_the_window_or_the_loader_matters(lsq, case, fmt):
    d, nn = 33, 100
    Xb, Xq = _gauss(d)
    options = {}
    if callable(case):
        Xb, Xq = case(Xb, Xq, fmt)
    rows, Q = torch.from_numpy(Xb).cuda().to(TORCH[fmt]), torch.from_numpy(Xq).cuda()
    if case == "pitched":                                     # rows 40 halves apart: 16-byte aligned starts, the vector loader with a ragged tail
        store = torch.full((N, 40), float("nan"), device="cuda", dtype=TORCH[fmt])
        store[:, :d] = rows
        rows = store[:, :d]
    if case == "odd_view":                                    # rows d + 1 halves apart, one half into the allocation: the element loader
        store = torch.full((1 + N * (d + 1),), float("nan"), device="cuda", dtype=TORCH[fmt])
        view = store[1:].view(N, d + 1)[:, :d]
        view.copy_(rows)
        rows = view
        assert rows.data_ptr() % 16 != 0
    if case == "cap4":
        options["knn_prefilter_cap"] = 4
    off, on = _both(lsq, rows, Q, nn, **options)
    info = on[4]
    print(case, fmt, info)
    assert info["served"] == 1 and info["pairs"] > 0
    if case is _offset:                                       # norms of 3.3e7 against distances of 66: the window decides nothing
        assert info["switched_off"] == 1
    if case == "cap4":                                        # every list overflows, every query is redone by the direct scan
        assert info["overflow_queries"] == 130 and info["kept"] == 0 and info["switched_off"] == 1
    if case in ("pitched", "odd_view"):                       # (query 0 of _duplicates has 2000 rows inside tau: more than any list holds, on either road)
        assert info["overflow_queries"] == 0 and info["switched_off"] == 0


@pytest.mark.parametrize("road", ["f32_rows", "u8_rows", "filter", "u8_queries", "small_n", "option_alone"])
def test_roads_not_served_say_so(lsq, road):
    L = lsq._lib
    Xb, Xq = _gauss(24, n=60_000 if road == "small_n" else N)
    rows, Q, kw = torch.from_numpy(Xb).cuda().to(torch.bfloat16), torch.from_numpy(Xq).cuda(), {}
    reason = {"f32_rows": L.KNN_PREFILTER_HALF_ROWS_NOT_HALF, "u8_rows": L.KNN_PREFILTER_HALF_ROWS_NOT_HALF, "filter": L.KNN_PREFILTER_HALF_FILTERED,
              "u8_queries": L.KNN_PREFILTER_HALF_U8_QUERIES, "small_n": L.KNN_PREFILTER_HALF_EXHAUSTIVE, "option_alone": L.KNN_PREFILTER_HALF_PREFILTER_OFF}[road]
    if road == "f32_rows":
        rows = rows.float()
    if road in ("u8_rows", "u8_queries"):
        rows = torch.from_numpy(np.rint(Xb * 40 + 128).clip(0, 255).astype(np.uint8)).cuda()
    if road == "u8_queries":
        Q = torch.from_numpy(np.rint(Xq * 40 + 128).clip(0, 255).astype(np.uint8)).cuda()
    if road == "filter":
        kw["mask"] = np.arange(N) % 3 != 0
    if road == "option_alone":
        kw["only_half"] = True
    off, on = _run(lsq, rows, Q, 50, 0, **{k: v for k, v in kw.items() if k == "mask"}), _run(lsq, rows, Q, 50, 1, **kw)
    _same(off, on)
    assert on[4]["served"] == 0 and on[4]["reason"] == reason and on[4]["pairs"] == 0 and on[4]["kappa"] == 0
    assert off[4]["served"] == 0 and off[4]["reason"] == L.KNN_PREFILTER_HALF_NOT_ASKED
