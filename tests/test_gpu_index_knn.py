"""Exact k-NN on an index's resident base rows (lsq_index_knn: csrc/lsq_knn.hip under the selection of csrc/lsq_adc.hip), above all on un-widened uint8
rows: the integer road (v_dot4_u32_u8, d <= 258) and the widened road must both return the bits and ids of the checkers of tests/index_knn_check.py --
lsq_knn_exact_cpu on the widened matrices, and int64 arithmetic for d <= 258 -- at every width around the dword and chunk edges, for bases and queries at
byte offsets with padded pitches (padding of 255), at the tile edges, on every road of the selection, and interleaved with the index's other calls.
knn_info()["int_road"] is asserted everywhere: a build that always widens does not pass."""
import numpy as np
import pytest
import torch

import index_knn_check as IK
import knn_check as KC

pytestmark = pytest.mark.gpu
EINVAL = -1


def _dev_view(M, ld, off):
    """uint8 matrix M on the device with row pitch ld at byte offset off, surrounded by 255s -> (view, storage)"""
    _, buf = IK.laid_out(M, ld, off)
    t = torch.from_numpy(buf).cuda()
    return torch.as_strided(t, M.shape, (ld, 1), storage_offset=off), t


def _knn(ix, Q, nn, int_road, id_base=0, **expect):
    d, i = ix.knn(Q, nn, id_base=id_base)
    info = ix.knn_info()
    assert info["int_road"] == int_road and info["queries"] == Q.shape[0] and info["rows"] == ix.n, info
    for k, v in expect.items():
        assert info[k] == v, (k, info)
    if torch.is_tensor(d):
        torch.cuda.synchronize()
        d, i = d.cpu().numpy(), i.cpu().numpy()
    assert i.dtype == np.int32
    return d, i - id_base


def _both_roads(eng, Xb, Xq, nn, base=None, Q=None, **expect):
    """the device result on the integer road, after checking that the widened road (option knn_u8_int = 0) returns the same bits"""
    base = torch.tensor(Xb).cuda() if base is None else base            # (a copy: the shared reference data is read-only)
    Q = torch.tensor(Xq).cuda() if Q is None else Q
    with eng.index_dev(None, None, None, 0, base=base, d=Xb.shape[1]) as ix:
        d1, i1 = _knn(ix, Q, nn, 1, **expect)
        eng.set_option("knn_u8_int", 0)
        try:
            d0, i0 = _knn(ix, Q, nn, 0, **expect)
        finally:
            eng.set_option("knn_u8_int", 1)
    IK.same(d1, i1, d0, i0)
    return d1, i1


@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 127, 128, 129, 257, 258])
def test_widths_integer_road(lsq, d):
    Xb, Xq = IK.u8_data(d, 1000, 9, d)
    with lsq.Engine(0) as eng:
        got = _both_roads(eng, Xb, Xq, 10, exhaustive=1, fallback_queries=0)
    IK.same(*got, *IK.knn_int64(Xb, Xq, 10))
    IK.same(*got, *IK.knn_widened(lsq._lib.load(), Xb, Xq, 10))


@pytest.mark.parametrize("d", [259, 960])
def test_widths_past_258_take_the_widened_road(lsq, d):
    Xb, Xq = IK.u8_data(d, 1000, 9, d)
    with lsq.Engine(0) as eng, eng.index_dev(None, None, None, 0, base=torch.from_numpy(Xb).cuda()) as ix:
        got = _knn(ix, torch.from_numpy(Xq).cuda(), 10, 0)
    IK.same(*got, *IK.knn_widened(lsq._lib.load(), Xb, Xq, 10))


def test_extreme_distances(lsq):
    with lsq.Engine(0) as eng:
        Xb, Xq = IK.extreme(300, 5, 258)
        got = _both_roads(eng, Xb, Xq, 300)
        IK.same(*got, *IK.knn_int64(Xb, Xq, 300))
        assert got[0][0, got[1][0] == 0][0] == np.float32(16776450.0)      # all 255 against all 0: the largest D the integer road is allowed
        Xb, Xq = IK.extreme(300, 5, 960)                                    # here the chain rounds: the device must return the chain
        with eng.index_dev(None, None, None, 0, base=torch.from_numpy(Xb).cuda()) as ix:
            got = _knn(ix, torch.from_numpy(Xq).cuda(), 300, 0)
        IK.same(*got, *IK.knn_widened(lsq._lib.load(), Xb, Xq, 300))


@pytest.mark.parametrize("d", [5, 13])
def test_loaders_base_and_queries(lsq, d):
    """pointer offset 0-3 x pitch {d, d + 1, next multiple of 4, that + 4}, for the base and for the queries; d = 5 with pitch 8 at offset 0 is the last,
    partial dword of a dword-loaded row"""
    n, nq, nn = 200, 6, 8
    Xb, Xq = IK.u8_data(100 + d, n, nq, d)
    want = IK.knn_int64(Xb, Xq, nn)
    up4 = (d + 3) // 4 * 4
    with lsq.Engine(0) as eng:
        for off in range(4):
            for ld in (d, d + 1, up4, up4 + 4):
                base, keep_b = _dev_view(Xb, ld, off)
                Q, keep_q = _dev_view(Xq, ld, (off + 1) % 4)
                assert base.data_ptr() % 4 == off and base.stride(0) == ld
                IK.same(*_both_roads(eng, Xb, Xq, nn, base=base, Q=Q), *want)
                IK.same(*_both_roads(eng, Xb, Xq, nn, base=base), *want)
        # host queries keep their layout too (the base of a host index is packed by the binding)
        _, qbuf = IK.laid_out(Xq, d + 3, 1)
        Qh = np.lib.stride_tricks.as_strided(qbuf[1:], shape=Xq.shape, strides=(d + 3, 1))
        with eng.index(None, None, None, 0, base=Xb) as ix:
            IK.same(*_knn(ix, Qh, nn, 1), *want)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 3000])
def test_tile_edges_and_nn_equals_n(lsq, n):
    d = 8
    Xb, Xq = IK.u8_data(n, n, 129, d)
    want = IK.knn_int64(Xb, Xq, n)
    with lsq.Engine(0) as eng:
        for nq in (1, 127, 128, 129):
            got = _both_roads(eng, Xb, Xq[:nq], n)
            IK.same(*got, want[0][:nq], want[1][:nq])


@pytest.fixture(scope="module")
def large(lsq):
    """n = 100 000 (past ADC_SMALL_N: thresholded lists), nq = 1000, d = 64, nn = 100, and its reference: computed once, read-only"""
    Xb, Xq = IK.u8_data(77, 100000, 1000, 64)
    want = IK.knn_widened(lsq._lib.load(), Xb, Xq, 100)
    for a in (Xb, Xq) + want:
        a.setflags(write=False)
    IK.same(want[0][:8], want[1][:8], *IK.knn_int64(Xb, Xq[:8], 100))
    return Xb, Xq, want


def test_thresholded_lists(lsq, large):
    Xb, Xq, want = large
    with lsq.Engine(0) as eng:
        IK.same(*_both_roads(eng, Xb, Xq, 100, exhaustive=0, fallback_queries=0), *want)


@pytest.mark.parametrize("option,expect", [("linscan_rank", dict(exhaustive=0, fallback_queries=48)), ("linscan_exhaustive", dict(exhaustive=1, fallback_queries=0))])
def test_selection_hooks(lsq, large, option, expect):
    Xb, Xq, want = large
    with lsq.Engine(0) as eng:
        eng.set_option(option, 1)
        IK.same(*_both_roads(eng, Xb, Xq[:48], 100, **expect), want[0][:48], want[1][:48])


def test_heavy_ties_overflow_to_the_fallback(lsq):
    rng = np.random.default_rng(5)
    Xb = rng.integers(0, 4, (50000, 6), dtype=np.uint8)
    Xb = np.concatenate([Xb, Xb])                                   # every row twice: ties go to the smaller id
    Xq = rng.integers(0, 4, (40, 6), dtype=np.uint8)
    with lsq.Engine(0) as eng:
        got = _both_roads(eng, Xb, Xq, 100, exhaustive=0)
        with eng.index_dev(None, None, None, 0, base=torch.from_numpy(Xb).cuda()) as ix:
            ix.knn(torch.from_numpy(Xq).cuda(), 100)
            assert ix.knn_info()["fallback_queries"] > 0
    IK.same(*got, *IK.knn_widened(lsq._lib.load(), Xb, Xq, 100))
    assert (np.diff(got[1].astype(np.int64), axis=1)[np.diff(got[0], axis=1) == 0] > 0).all()


def test_u8_base_with_fractional_f32_queries(lsq):
    Xb, Xq = IK.u8_data(8, 2000, 33, 50)
    Qf = Xq.astype(np.float32) + np.random.default_rng(9).random((33, 50), dtype=np.float32)
    rc, wd, wi = KC.knn_cpu(lsq._lib.load(), Xb.astype(np.float32), Qf, 50, 20)
    assert rc == 0
    with lsq.Engine(0) as eng, eng.index_dev(None, None, None, 0, base=torch.from_numpy(Xb).cuda()) as ix:
        IK.same(*_knn(ix, torch.from_numpy(Qf).cuda(), 20, 0), wd, wi)
    with lsq.Engine(0) as eng:                                      # the Engine calls accept the uint8 base, host and device forms
        d1, i1 = eng.knn_exact(Xb, Qf, 20)
        assert i1.dtype == np.uint32
        IK.same(d1, i1, wd, wi)
        d2, i2 = eng.knn_exact_dev(torch.from_numpy(Xb).cuda(), torch.from_numpy(Xq).cuda(), 20)
        IK.same(d2.cpu().numpy(), i2.cpu().numpy(), *IK.knn_int64(Xb, Xq, 20))
        d3, i3 = lsq.knn_exact(np.ascontiguousarray(Xb.T), np.ascontiguousarray(Xq.T), 20, engine=eng)
        IK.same(d3.T, i3.T - 1, *IK.knn_int64(Xb, Xq, 20))


@pytest.mark.parametrize("id_base", [0, 1])
def test_f32_index_is_knn_exact_dev(lsq, id_base):
    rng = np.random.default_rng(12)
    Xb, Xq = rng.standard_normal((70000, 24)).astype(np.float32), rng.standard_normal((50, 24)).astype(np.float32)
    dXb, dXq = torch.from_numpy(Xb).cuda(), torch.from_numpy(Xq).cuda()
    with lsq.Engine(0) as eng:
        rd, ri = eng.knn_exact_dev(dXb, dXq, 30)
        with eng.index_dev(None, None, None, 0, base=dXb) as ix:
            d, i = ix.knn(dXq, 30, id_base=id_base)
            assert ix.knn_info()["int_road"] == 0
        assert torch.equal(d.view(torch.int32), rd.view(torch.int32)) and torch.equal(i, ri + id_base)


def test_one_index_many_calls(lsq):
    n, nq, d, m, h, k = 4000, 40, 16, 2, 256, 10
    rng = np.random.default_rng(31)
    Xb, Xq = IK.u8_data(30, n, nq, d)
    Xb2, _ = IK.u8_data(32, n, nq, d)
    K = rng.standard_normal((m * h, d)).astype(np.float32)
    codes = rng.integers(0, h, (n, m)).astype(np.uint8)
    dbn = rng.random(n).astype(np.float32)
    Qf = Xq.astype(np.float32)
    cand = rng.integers(0, n, (nq, 64)).astype(np.int32)
    calls = {
        "knn": lambda ix, ix2: ix.knn(Xq, k),
        "search": lambda ix, ix2: ix.search(Qf, k, shortlist=50),
        "knn1": lambda ix, ix2: ix.knn(Xq, k, id_base=1),
        "rerank": lambda ix, ix2: ix.rerank(Qf, cand, k, id_base=0),
        "knn_f32q": lambda ix, ix2: ix.knn(Qf, k),
        "knn_other": lambda ix, ix2: ix2.knn(Xq, 2 * k),
    }
    fresh = {}
    for name, fn in calls.items():
        with lsq.Engine(0) as eng, eng.index(codes, K, dbn, m, base=Xb) as ix, eng.index(None, None, None, 0, base=Xb2) as ix2:
            fresh[name] = fn(ix, ix2)
    IK.same(fresh["knn"][0], fresh["knn"][1], *IK.knn_int64(Xb, Xq, k))
    IK.same(fresh["knn_f32q"][0], fresh["knn_f32q"][1], *fresh["knn"])
    IK.same(fresh["knn1"][0], fresh["knn1"][1] - 1, *fresh["knn"])
    IK.same(fresh["knn_other"][0], fresh["knn_other"][1], *IK.knn_int64(Xb2, Xq, 2 * k))
    order = ["knn", "search", "knn_other", "knn1", "rerank", "knn", "knn_f32q", "knn_other", "search", "knn"]
    with lsq.Engine(0) as eng, eng.index(codes, K, dbn, m, base=Xb) as ix, eng.index(None, None, None, 0, base=Xb2) as ix2:
        for name in order + order:                                  # two runs are identical
            IK.same(*calls[name](ix, ix2), *fresh[name])
        with eng.index_dev(None, None, None, 0, base=torch.from_numpy(Xb).cuda()) as ixd:      # host and device forms agree
            IK.same(*_knn(ixd, torch.from_numpy(Xq).cuda(), k, 1), *fresh["knn"])


def test_self_match(lsq):
    Xb, _ = IK.u8_data(40, 3000, 1, 32, hi=3)
    Xb[1500:] = Xb[:1500]                                            # duplicates: the first id is the row or an earlier copy of it
    with lsq.Engine(0) as eng, eng.index(None, None, None, 0, base=Xb) as ix:
        d, i = _knn(ix, Xb, 2, 1)
    assert (d[:, 0] == 0).all() and (i[:, 0] <= np.arange(3000)).all() and (Xb[i[:, 0]] == Xb).all()


def test_einval_launches_nothing(lsq):
    L = lsq._lib.load()
    Xb, Xq = IK.u8_data(50, 100, 4, 8)
    dists, ids = np.zeros((4, 100), np.float32), np.zeros((4, 100), np.int32)
    Qf = np.zeros(4 * 8 * 4 + 4, np.uint8)
    with lsq.Engine(0) as eng, eng.index(None, None, None, 0, base=Xb) as ix:
        def call(h=ix._h, dp=dists.ctypes.data, ip=ids.ctypes.data, q=Xq.ctypes.data, q_u8=1, nq=4, ldq=8, nn=5, id_base=0):
            return L.lsq_index_knn(h, dp, ip, q, q_u8, nq, ldq, nn, id_base, 0)
        assert call() == 0
        before = ix.knn_info()
        for bad in (dict(nn=0), dict(nn=101), dict(nq=0), dict(ldq=7), dict(id_base=2), dict(id_base=-1), dict(q=None), dict(dp=None), dict(ip=None),
                    dict(h=None), dict(q=Qf.ctypes.data + 1 + (-Qf.ctypes.data % 4), q_u8=0)):
            assert call(**bad) == EINVAL, bad
            assert b"lsq_index_knn" in L.lsq_last_error()
        assert call(q=Qf.ctypes.data + (-Qf.ctypes.data % 4), q_u8=0) == 0
        assert L.lsq_index_get_knn_info(ix._h, None) == EINVAL
        K = np.zeros((256, 8), np.float32)
        with eng.index(np.zeros((100, 1), np.uint8), K, np.zeros(100, np.float32), 1) as scan_only:      # an index without base rows
            assert call(h=scan_only._h) == EINVAL
        assert ix.knn_info()["queries"] == 4 and before["int_road"] == 1
