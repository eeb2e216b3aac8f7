"""The MFMA pre-filter of exact k-NN (option "knn_prefilter"; csrc/lsq_knnm.hip) may only decide which pairs deserve the direct chain: with it on, every
call returns the bits, the ids and the statistic `candidates` of the same call with it off -- on every row type, at ragged shapes, where the window is
wide, where lists overflow, and on the roads it does not serve.  Equal `candidates` is the sharp part: a pair wrongly dropped inside tau changes it."""
import numpy as np
import pytest
import torch

import knn_check as KC

pytestmark = pytest.mark.gpu
N, NQ, NN = 70_001, 130, 50                  # above the exhaustive limit of 65 536, ragged row and query tiles
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "uint8": torch.uint8}


def _gauss(seed, d, n=N, nq=NQ):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)


def _run(lsq, base, Q, pre, nn=NN, index=False, mask=None, **options):
    """one search of device rows `base` -> dists, ids, statistics, the pre-filter's account.  index: through a base-only Index (any row type), whose
    knn_info and knn_prefilter_info are returned; otherwise Engine.knn_exact_dev (f32 rows), whose linscan_stats carry `candidates` -- and no account"""
    with lsq.Engine(0) as eng:
        eng.set_option("knn_prefilter", int(pre))
        for k, v in options.items():
            eng.set_option(k, v)
        if index:
            with eng.index_dev(None, None, None, 0, base=base) as ix:
                if mask is not None:
                    ix.set_filter(mask=torch.from_numpy(mask).cuda(), road="dense")
                d, i = ix.knn(Q, nn)
                st, info = ix.knn_info(), ix.knn_prefilter_info()
        else:
            d, i = eng.knn_exact_dev(base, Q, nn)
            st, info = eng.linscan_stats(), None
        torch.cuda.synchronize()
    return d.cpu().numpy(), i.cpu().numpy().view(np.uint32), st, info


def _identical(a, b, stats=("candidates", "fallback_queries", "exhaustive", "threshold_rank", "list_capacity")):
    assert np.array_equal(a[1], b[1]), "ids differ at %s" % (np.argwhere(a[1] != b[1])[:5].tolist(),)
    assert KC.same_bits(a[0], b[0]), "distances differ"
    for k in stats:
        assert a[2][k] == b[2][k], (k, a[2], b[2])


@pytest.mark.parametrize("tx", ["f32", "f16", "bf16", "uint8"])
@pytest.mark.parametrize("d", [1, 3, 17, 128, 130])
def test_identity(lsq, d, tx):
    Xb, Xq = _gauss(100 + d, d)
    if tx == "uint8":                                         # uniform bytes: at d = 1 a row value is shared by ~273 rows, a list is one such group (< capacity)
        rng = np.random.default_rng(d)
        Xb, Xq = rng.integers(0, 256, (N, d)).astype(np.float32), rng.uniform(0, 255, (NQ, d)).astype(np.float32)
    rows = torch.from_numpy(Xb).cuda().to(TORCH[tx])          # what the pre-filtered call reads ...
    wide, Q = rows.float(), torch.from_numpy(Xq).cuda()       # ... and the same values as f32 rows: the direct call's
    direct = _run(lsq, wide, Q, 0)
    pre = _run(lsq, rows, Q, 1, index=True)
    _identical(direct, pre, stats=())
    if tx == "f32":                                           # the context form: its statistics too
        _identical(direct, _run(lsq, rows, Q, 1))
    info = pre[3]
    print(d, tx, direct[2]["candidates"], info)
    assert info["served"] == 1 and info["reason"] == 0 and info["overflow_queries"] == 0 and info["switched_off"] == 0
    assert info["kept"] == direct[2]["candidates"] and info["pending"] >= info["kept"] and info["pairs"] == N * NQ
    if tx == "f32":
        rc, cd, ci = KC.knn_cpu(lsq._lib.load(), Xb, Xq, d, NN)
        assert rc == 0 and np.array_equal(ci, pre[1]) and KC.same_bits(cd, pre[0])


def _offset(Xb, Xq):
    return Xb + np.float32(1000), Xq + np.float32(1000)


def _tiny(Xb, Xq):
    return Xb * np.float32(1e-20), Xq * np.float32(1e-20)


def _duplicates(Xb, Xq):
    Xb[5000:7000] = Xq[0] + np.float32(0.01)
    return Xb, Xq


def _nonfinite(Xb, Xq):
    Xb[[3, 50, 69_999]] = np.nan
    Xb[[7, 120], 2] = np.inf
    Xb[9, 0] = -np.inf
    Xq[5, 1] = np.nan
    Xq[6, 0] = np.inf
    return Xb, Xq


@pytest.mark.parametrize("case", [_offset, _tiny, _duplicates, _nonfinite, "view"])
def test_where_the_window_matters(lsq, case):
    d = 64
    Xb, Xq = _gauss(7, d)
    if case == "view":                                        # rows d + 1 floats apart, one float into the allocation
        sb = torch.full((1 + N * (d + 1),), float("nan"), device="cuda")
        sq = torch.full((1 + NQ * (d + 1),), float("inf"), device="cuda")
        base, Q = sb[1:].view(N, d + 1)[:, :d], sq[1:].view(NQ, d + 1)[:, :d]
        base.copy_(torch.from_numpy(Xb))
        Q.copy_(torch.from_numpy(Xq))
        assert base.data_ptr() % 16 != 0
    else:
        Xb, Xq = case(Xb, Xq)
        base, Q = torch.from_numpy(Xb).cuda(), torch.from_numpy(Xq).cuda()
    direct, pre = _run(lsq, base, Q, 0), _run(lsq, base, Q, 1)
    _identical(direct, pre)
    ix = _run(lsq, base, Q, 1, index=True)                    # the same call on an index, for its account
    _identical(direct, ix, stats=())
    info = ix[3]
    print(case, info)
    assert info["served"] == 1
    if case is _offset:                                       # norms of 6.4e7 against distances of 128: the window decides nothing
        assert info["switched_off"] + info["overflow_queries"] > 0 or info["pending"] > info["kept"]


def test_overflow_is_redone_directly(lsq):
    Xb, Xq = _gauss(8, 32)
    base, Q = torch.from_numpy(Xb).cuda(), torch.from_numpy(Xq).cuda()
    direct, pre = _run(lsq, base, Q, 0), _run(lsq, base, Q, 1, knn_prefilter_cap=64)
    _identical(direct, pre)
    assert pre[2]["exhaustive"] == 0 and pre[2]["fallback_queries"] == 0
    ix = _run(lsq, base, Q, 1, index=True, knn_prefilter_cap=64)
    _identical(direct, ix, stats=())
    assert ix[3]["overflow_queries"] == NQ and ix[3]["kept"] == 0 and ix[3]["switched_off"] == 1


def test_short_lists_take_the_exhaustive_fallback(lsq):
    Xb, Xq = _gauss(9, 17)
    base, Q = torch.from_numpy(Xb).cuda(), torch.from_numpy(Xq).cuda()
    direct, pre = _run(lsq, base, Q, 0, linscan_rank=1), _run(lsq, base, Q, 1, linscan_rank=1)
    _identical(direct, pre)
    ix = _run(lsq, base, Q, 1, index=True, linscan_rank=1)
    _identical(direct, ix, stats=())
    assert pre[2]["fallback_queries"] == NQ and ix[2]["fallback_queries"] == NQ and ix[3]["served"] == 1


@pytest.mark.parametrize("road", ["small_n", "filter", "u8_queries"])
def test_roads_not_served_say_so(lsq, road):
    L = lsq._lib
    Xb, Xq = _gauss(10, 24, n=60_000 if road == "small_n" else N)
    kw, reason = dict(index=True), L.KNN_PREFILTER_EXHAUSTIVE
    if road == "filter":
        kw, reason = dict(index=True, mask=np.arange(N) % 3 != 0), L.KNN_PREFILTER_FILTERED
    if road == "u8_queries":
        Xb, Xq = np.rint(Xb * 40 + 128).clip(0, 255).astype(np.uint8), np.rint(Xq * 40 + 128).clip(0, 255).astype(np.uint8)
        kw, reason = dict(index=True), L.KNN_PREFILTER_U8_QUERIES
    base, Q = torch.from_numpy(Xb).cuda(), torch.from_numpy(Xq).cuda()
    direct, pre = _run(lsq, base, Q, 0, **kw), _run(lsq, base, Q, 1, **kw)
    _identical(direct, pre, stats=("fallback_queries", "exhaustive"))
    assert pre[3]["served"] == 0 and pre[3]["reason"] == reason and pre[3]["pairs"] == 0
    assert direct[3]["served"] == 0 and direct[3]["reason"] == L.KNN_PREFILTER_NOT_ASKED


@pytest.mark.parametrize("tx", ["f32", "bf16"])
def test_index_knn_before_and_after_an_add(lsq, tx):
    Xb, Xq = _gauss(11, 40, n=N + 300)
    rows, Q = torch.from_numpy(Xb).cuda().to(TORCH[tx]), torch.from_numpy(Xq).cuda()
    with lsq.Engine(0) as eng, eng.index_dev(None, None, None, 0, base=rows[:N].clone()) as ix:
        for grown in (False, True):
            if grown:
                ix.add(base=rows[N:])
            got = []
            for pre in (0, 1):
                eng.set_option("knn_prefilter", pre)
                d, i = ix.knn(Q, NN)
                got.append((d.cpu().numpy(), i.cpu().numpy().view(np.uint32), ix.knn_info(), ix.knn_prefilter_info()))
            _identical(got[0], got[1], stats=("fallback_queries", "exhaustive"))
            assert got[1][3]["served"] == 1 and got[1][3]["pairs"] == (N + 300 * grown) * NQ
