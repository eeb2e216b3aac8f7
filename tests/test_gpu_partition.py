"""The coarse partition on the device: every call of lsq_partition_* held bit for bit to its host checker (which tests/test_partition.py holds to the numpy
statement of the contract), host and device forms, at the smallest shapes at which each kernel can go wrong; then the two functions built on them,
train_coarse_dev and build_ivf_residual_index, against the host statement of the same build; and all of it again at 65 536 .. 2^24 lists."""
import contextlib
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivf_check as ic  # noqa: E402
import partition_check as pc  # noqa: E402
from knn_check import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
H = 256


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def root(v):
    while v.base is not None:
        v = v.base
    return v


def to_dev(torch, v):
    """a numpy row view (pc.row_view) -> (the torch view of the same geometry on the device, its whole buffer)"""
    if v.base is None:
        t = torch.from_numpy(v).cuda()
        return t, t
    buf = root(v)
    first = (v.ctypes.data - buf.ctypes.data) // v.itemsize
    n, d = v.shape
    p = pc.pitch(v)
    t = torch.from_numpy(buf).cuda()
    return t[first:first + n * p].view(n, p)[:, :d], t


def loader_of(t):
    """how four components of a row of `t` travel: f32 16 bytes or dwords, uint8 a dword or bytes, by the alignment of the base and of the pitch in bytes"""
    a = t.data_ptr() | ((t.stride(0) if t.shape[0] > 1 else t.shape[1]) * t.element_size())
    return min(16 if a % 16 == 0 else (4 if a % 4 == 0 else 1), 4 * t.element_size())


def lists_for(n, nlist, seed):
    return np.random.default_rng(seed).integers(0, nlist, n).astype(np.int32)


# ---- residuals ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 4, 5, 16, 127, 128, 130])
@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_residuals_equal_the_host_checker(lsq, engine, torch, n, d):
    L = lsq._lib.load()
    rng = np.random.default_rng(1000 * n + d)
    nlist = {1: 1, 255: 2, 257: 300, 1000: 300}[n]
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    Xf = rng.standard_normal((n, d)).astype(np.float32)
    Xf, cent = pc.special_rows(Xf, cent, n + d)
    X8 = rng.integers(0, 256, (n, d)).astype(np.uint8)
    assign = lists_for(n, nlist, d)
    dassign = torch.from_numpy(assign).cuda()
    wantf = pc.residuals_cpu(L, Xf, cent, assign)[1]
    want8 = pc.residuals_cpu(L, X8, cent, assign)[1]
    assert pc.same(wantf, pc.residuals_np(Xf, cent, assign)) and same_bits(want8, pc.residuals_np(X8, cent, assign))
    odd = 1 if d % 2 == 0 else 2                                                      # an odd pitch for the byte rows
    views = [(Xf, wantf), (pc.row_view(Xf, 3, offset=1), wantf), (pc.row_view(Xf, 4 - d % 4, offset=0), wantf), (X8, want8),
             (pc.row_view(X8, (-d) % 4 + 4, offset=0), want8), (pc.row_view(X8, (-d) % 16, offset=0), want8)]
    views += [(pc.row_view(X8, odd, offset=o), want8) for o in range(4)]
    seen = {np.dtype(np.float32): set(), np.dtype(np.uint8): set()}
    with engine.partition_dev(torch.from_numpy(cent).cuda()) as part:
        for k, (v, want) in enumerate(views):
            dv, _ = to_dev(torch, v)
            # R: a row view of its own (ldr > d, 4- but not 16-byte aligned) with a sentinel everywhere else, or a new contiguous tensor
            if k % 2:
                out, obuf = to_dev(torch, pc.row_view(np.full((n, d), 55, np.float32), 3, offset=1))
                R = part.residuals(dv, dassign, out=out)
                assert R is out and pc.untouched_dev(obuf.cpu().numpy(), 1, n, d, d + 3, 77)
            else:
                R = part.residuals(dv, dassign)
            assert pc.same(R.cpu().numpy(), want), (k, v.dtype, v.strides)
            info = part.info()
            assert info["call"] == lsq._lib.PARTITION_RESIDUALS and info["rows"] == n and info["loader_bytes"] == loader_of(dv), (k, info)
            seen[v.dtype].add(info["loader_bytes"])
        assert n == 1 or (seen[np.dtype(np.float32)] == {16, 4} and seen[np.dtype(np.uint8)] == {4, 1})      # all three loader widths ran
    with engine.partition(cent) as part:                                              # the host form: arrays in and out, row views read and written in place
        for v, want in (views[1], views[-1]):
            out = pc.row_view(np.full((n, d), 55, np.float32), 2)
            assert part.residuals(v, assign, out=out) is out and pc.same(out, want) and pc.untouched(out, 77)
        assert pc.same(part.residuals(Xf.astype(np.float64), assign), wantf)          # anything else is converted first


def test_residuals_keep_negative_zero(engine, torch):
    x = torch.full((3, 5), -0.0, device="cuda")
    with engine.partition_dev(torch.zeros(1, 5, device="cuda")) as part:
        R = part.residuals(x, torch.zeros(3, dtype=torch.int32, device="cuda")).cpu().numpy()
    assert np.all(R == 0) and np.all(np.signbit(R))


# ---- update -------------------------------------------------------------------------------------------------------------------------------------------
def _update_both(lsq, engine, torch, cent, X, assign):
    """device form, host form, host checker -> the device form's (centroids, counts) after checking that all three agree"""
    L = lsq._lib.load()
    rc, want, wc = pc.update_cpu(L, cent, X, assign)
    assert rc == 0
    dX, _ = to_dev(torch, X)
    with engine.partition_dev(torch.from_numpy(cent).cuda()) as part:
        counts = part.update(dX, torch.from_numpy(assign).cuda(), want_counts=True)
        got = part.centroids().cpu().numpy()
        info = part.info()
        assert part.update(dX, torch.from_numpy(assign).cuda()) is None
    assert same_bits(got, want) and np.array_equal(counts.cpu().numpy(), wc)
    assert info["call"] == lsq._lib.PARTITION_UPDATE and info["rows"] == X.shape[0] and info["empty_lists"] == int((wc == 0).sum())
    assert info["lists_touched"] == int((wc > 0).sum()) and info["max_list_rows"] == int(wc.max()) and info["loader_bytes"] == X.itemsize
    with engine.partition(cent) as part:
        hc = part.update(X, assign, want_counts=True)
        assert same_bits(part.centroids(), want) and np.array_equal(hc, wc)
    return got, wc


def test_update_is_numpy_add_at_on_decade_spanning_rows(lsq, engine, torch):
    X = pc.decades(5000, 5, 3)
    assign = lists_for(5000, 7, 1)                                                    # lists 7 and 8 stay empty
    cent = np.random.default_rng(2).standard_normal((9, 5)).astype(np.float32)
    got, counts = _update_both(lsq, engine, torch, cent, X, assign)
    want, wc = pc.update_np(cent, X, assign)
    assert same_bits(got, want) and np.array_equal(counts, wc)
    assert same_bits(got[7:], cent[7:])                                               # a list without rows keeps its centroid's bits
    f32 = np.zeros((9, 5), np.float32)
    np.add.at(f32, assign, X)
    assert not same_bits((f32[:7] / wc[:7, None]).astype(np.float32), got[:7])        # a float32 accumulator is another number


@pytest.mark.parametrize("d", [1, 5, 64, 130, 300])
def test_update_walks_lists_of_every_length_around_the_prefetch_depth(lsq, engine, torch, d):
    """lists of 1 .. 2 * prefetch + 1 rows with interleaved row ids and three empty lists; f32 row views and uint8 rows at a byte offset; d = 300: two
    blocks per list"""
    assign, nlist = pc.ladder_lists()
    n = assign.shape[0]
    rng = np.random.default_rng(d)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    for X in (pc.row_view(pc.decades(n, d, d), 3, offset=1), pc.row_view(rng.integers(0, 256, (n, d)).astype(np.uint8), 5, offset=3)):
        got, wc = _update_both(lsq, engine, torch, cent, X, assign)
        assert sorted(wc[wc > 0]) == list(range(1, 2 * pc.PREFETCH + 2))
        assert same_bits(got[wc == 0], cent[wc == 0]) and int((wc == 0).sum()) == 3
        assert same_bits(got, pc.update_np(cent, np.ascontiguousarray(X), assign)[0])


def test_update_with_more_lists_than_rows_and_one_list_for_all(lsq, engine, torch):
    rng = np.random.default_rng(3)
    X = pc.decades(6, 4, 1)
    for lists, nl in ((np.arange(6, dtype=np.int32)[::-1].copy() * 3, 20), (np.full(6, 4, np.int32), 5)):
        _update_both(lsq, engine, torch, rng.standard_normal((nl, 4)).astype(np.float32), X, lists)
    X = pc.decades(3000, 16, 5)                                                       # one list holding every row: one chain of 3000 adds per dimension
    got, wc = _update_both(lsq, engine, torch, np.zeros((3, 16), np.float32), X, np.full(3000, 1, np.int32))
    assert wc.tolist() == [0, 3000, 0]


def test_two_updates_give_the_same_bits(engine, torch):
    X = torch.from_numpy(pc.decades(4000, 33, 9)).cuda()
    assign = torch.from_numpy(lists_for(4000, 50, 2)).cuda()
    cent = torch.zeros(50, 33, device="cuda")
    outs = []
    for _ in range(2):
        with engine.partition_dev(cent) as part:
            part.update(X, assign)
            outs.append(part.centroids().cpu().numpy())
    assert same_bits(outs[0], outs[1])


# ---- code_norms -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 4, 6, 128])
@pytest.mark.parametrize("m", [1, 7, 8, 16])
def test_code_norms_equal_the_host_checker(lsq, engine, torch, m, d):
    L = lsq._lib.load()
    n, nlist = 700, 13
    codes, K, cent, assign = pc.code_problem(n, d, m, nlist, 31 * m + d)
    K[codes[3, 0]] = np.nan                                                           # a NaN reconstruction: its norm byte is the first entry
    s = pc.code_norms_cpu(L, codes, K, cent, assign)[1]
    dcodes, dassign = torch.from_numpy(codes).cuda(), torch.from_numpy(assign).cuda()
    Kbuf = torch.zeros(m * H * d + 1, device="cuda")
    Kbuf[1:] = torch.from_numpy(K).cuda().reshape(-1)
    roads = [torch.from_numpy(K).cuda(), Kbuf[1:].view(m * H, d)]                     # 16-byte aligned (d % 4 == 0: four dimensions per load) and 4-byte aligned only
    assert roads[0].data_ptr() % 16 == 0 and roads[1].data_ptr() % 16 == 4 and roads[1].is_contiguous()
    with engine.partition_dev(torch.from_numpy(cent).cuda()) as part, engine.partition(cent) as hpart:
        for dK in roads:
            assert pc.same(part.code_norms(dcodes, dK, dassign).cpu().numpy(), s)
            for ncb in (1, 37, 256):
                cb = np.sort(np.random.default_rng(ncb).choice(s[np.isfinite(s)], ncb, replace=False)).astype(np.float32)
                if ncb > 2:
                    cb[ncb // 2] = cb[ncb // 2 - 1]                                   # a duplicated entry goes to the first
                rc, ws, wnc, wdb = pc.code_norms_cpu(L, codes, K, cent, assign, cb)
                norms, nc, dbn = part.code_norms(dcodes, dK, dassign, torch.from_numpy(cb).cuda())
                assert rc == 0 and pc.same(norms.cpu().numpy(), ws) and np.array_equal(nc.cpu().numpy(), wnc) and same_bits(dbn.cpu().numpy(), wdb)
                assert wnc[3] == 0 and (ncb <= 2 or not np.any(wnc == ncb // 2))
        hn, hnc, hdb = hpart.code_norms(codes, K, assign, cb)                         # the host form
        assert pc.same(hn, ws) and np.array_equal(hnc, wnc) and same_bits(hdb, wdb)
        assert part.info()["call"] == lsq._lib.PARTITION_CODE_NORMS and part.info()["rows"] == n


def test_code_norms_with_zero_centroids_are_quantize_norms_dev(engine, torch):
    codes, K, cent, assign = pc.code_problem(900, 32, 8, 4, 12)
    dcodes, dK, dassign = torch.from_numpy(codes).cuda(), torch.from_numpy(K).cuda(), torch.from_numpy(assign).cuda()
    dcb = torch.linspace(0, 400, 64, device="cuda")
    idx, dbn, nrm = engine.quantize_norms_dev(dcodes, dK, dcb, 8)
    with engine.partition_dev(torch.zeros(4, 32, device="cuda")) as part:
        norms, nc, db = part.code_norms(dcodes, dK, dassign, dcb)
    assert torch.equal(norms.view(torch.int32), nrm.view(torch.int32)) and torch.equal(nc, idx) and torch.equal(db.view(torch.int32), dbn.view(torch.int32))


def test_code_norms_without_cbnorms_write_norms_only(lsq, engine, torch):
    L = lsq._lib.load()
    codes, K, cent, assign = pc.code_problem(300, 6, 3, 5, 2)
    dcodes, dK, dassign = torch.from_numpy(codes).cuda(), torch.from_numpy(K).cuda(), torch.from_numpy(assign).cuda()
    norms, nc, dbn = torch.full((300,), -7.0, device="cuda"), torch.full((300,), 255, dtype=torch.uint8, device="cuda"), torch.full((300,), -7.0, device="cuda")
    with engine.partition_dev(torch.from_numpy(cent).cuda()) as part:
        torch.cuda.synchronize()                                                      # the raw calls below run on the context's own stream
        args = [dcodes.data_ptr(), dK.data_ptr(), 300, 3, H, dassign.data_ptr(), None, 0]
        assert L.lsq_partition_code_norms(part._h, *args, norms.data_ptr(), nc.data_ptr(), dbn.data_ptr(), 1) == 0
        assert L.lsq_partition_code_norms(part._h, *args, None, nc.data_ptr(), dbn.data_ptr(), 1) == lsq._lib.LSQ_EINVAL
    torch.cuda.synchronize()
    assert same_bits(norms.cpu().numpy(), pc.code_norms_np(codes, K, cent, assign)) and bool((nc == 255).all()) and bool((dbn == -7).all())


# ---- assign ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,nlist", [(1, 3, 1), (700, 16, 9), (2049, 130, 300)])
def test_assign_is_ivf_assign(lsq, engine, torch, n, d, nlist):
    rng = np.random.default_rng(n + d)
    cent = (rng.standard_normal((nlist, d)) * 40 + 128).astype(np.float32)
    if nlist > 4:
        cent[4] = cent[2]                                                             # an exact tie: the smaller list wins
    Xf = (rng.standard_normal((n, d)) * 40 + 128).astype(np.float32)
    Xf[n // 2] = cent[min(2, nlist - 1)]
    X8 = np.clip(Xf, 0, 255).astype(np.uint8)
    with engine.partition_dev(torch.from_numpy(cent).cuda()) as part, engine.partition(cent) as hpart:
        for X in (Xf, X8, pc.row_view(Xf, 3, offset=1), pc.row_view(X8, 1, offset=3)):
            want = lsq.ivf_assign(np.ascontiguousarray(X), cent)                      # the host cores
            ref, acc = pc.assign_np(np.ascontiguousarray(X), cent)
            assert np.array_equal(want, ref)
            got, dist = part.assign(to_dev(torch, X)[0], want_dist=True)
            assert np.array_equal(got.cpu().numpy(), want) and same_bits(dist.cpu().numpy(), acc[np.arange(n), ref]), X.dtype
            assert np.array_equal(part.assign(to_dev(torch, X)[0]).cpu().numpy(), want) and np.array_equal(hpart.assign(X), want)
            assert not np.any(want == 4) or nlist <= 4
        assert part.info()["call"] == lsq._lib.PARTITION_ASSIGN and part.info()["rows"] == n
    assert nlist <= 4 or lsq.ivf_assign(Xf, cent)[n // 2] == 2


# ---- bad lists --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", [-1, 6, 2 ** 31 - 1, -2 ** 31])
def test_a_list_outside_the_range_is_refused_and_never_an_offset(lsq, engine, torch, entry):
    codes, K, cent, assign = pc.code_problem(500, 8, 2, 6, 4)
    assign[123] = entry
    X = torch.from_numpy(np.random.default_rng(0).standard_normal((500, 8)).astype(np.float32)).cuda()
    dassign, dcodes, dK = torch.from_numpy(assign).cuda(), torch.from_numpy(codes).cuda(), torch.from_numpy(K).cuda()
    with engine.partition_dev(torch.from_numpy(cent).cuda()) as part, engine.partition(cent) as hpart:
        for call in (lambda: part.update(X, dassign), lambda: part.residuals(X, dassign), lambda: part.code_norms(dcodes, dK, dassign),
                     lambda: hpart.update(X.cpu().numpy(), assign), lambda: hpart.residuals(X.cpu().numpy(), assign),
                     lambda: hpart.code_norms(codes, K, assign)):
            with pytest.raises(lsq._lib.LsqError, match="list_of_row") as err:
                call()
            assert err.value.code == lsq._lib.LSQ_EINVAL
        assert same_bits(part.centroids().cpu().numpy(), cent) and same_bits(hpart.centroids(), cent)      # unchanged after the failed update
        dassign[123] = 0                                                              # and the handle goes on working
        part.update(X, dassign)
        assign[123] = 0
        assert same_bits(part.centroids().cpu().numpy(), pc.update_np(cent, X.cpu().numpy(), assign)[0])


def test_the_library_refuses_bad_arguments_before_a_launch(lsq, engine, torch):
    L, EINVAL = lsq._lib.load(), lsq._lib.LSQ_EINVAL
    X = torch.zeros(10, 8, device="cuda")
    lists, R = torch.zeros(10, dtype=torch.int32, device="cuda"), torch.zeros(10, 8, device="cuda")
    x, l, r = X.data_ptr(), lists.data_ptr(), R.data_ptr()
    desc, out = lsq._lib.PartitionDesc(), C.c_void_p()
    for nlist, d, cp in ((0, 8, x), ((1 << 24) + 1, 8, x), (4, 0, x), (4, 8, None)):
        desc.nlist, desc.d, desc.centroids, desc.on_device = nlist, d, cp, 1
        assert L.lsq_partition_create(C.byref(out), engine._h, C.byref(desc)) == EINVAL and not out.value
    with engine.partition_dev(torch.zeros(4, 8, device="cuda")) as part:
        h = part._h
        assert L.lsq_partition_assign(h, x, 0, 10, 7, l, None, 1) == EINVAL           # ldx < d
        assert L.lsq_partition_assign(h, x + 2, 0, 9, 8, l, None, 1) == EINVAL        # f32 rows not 4-byte aligned
        assert L.lsq_partition_assign(h, x, 0, -1, 8, l, None, 1) == EINVAL
        assert L.lsq_partition_assign(h, x, 0, 2 ** 31 - 1, 8, l, None, 1) == EINVAL
        assert L.lsq_partition_assign(h, None, 0, 10, 8, l, None, 1) == EINVAL and L.lsq_partition_assign(h, x, 0, 10, 8, None, None, 1) == EINVAL
        assert L.lsq_partition_update(h, x, 0, 10, 7, l, None, 1) == EINVAL and L.lsq_partition_update(h, x, 0, 10, 8, None, None, 1) == EINVAL
        assert L.lsq_partition_residuals(h, x, 0, 10, 8, l, r, 7, 1) == EINVAL        # ldr < d
        assert L.lsq_partition_residuals(h, x, 0, 10, 8, l, None, 8, 1) == EINVAL and L.lsq_partition_residuals(h, x + 1, 0, 9, 8, l, r, 8, 1) == EINVAL
        for m, hh, ncb in ((0, H, 3), (17, H, 3), (2, 128, 3), (2, H, 0), (2, H, 257)):
            assert L.lsq_partition_code_norms(h, l, x, 10, m, hh, l, x, ncb, r, None, None, 1) == EINVAL, (m, hh, ncb)
        assert L.lsq_partition_get_centroids(h, None, 1) == EINVAL and L.lsq_partition_get_info(h, None) == EINVAL
        assert L.lsq_partition_assign(h, x, 0, 0, 8, l, None, 1) == 0 and L.lsq_partition_residuals(h, x, 0, 0, 8, l, r, 8, 1) == 0      # n = 0
        with pytest.raises(ValueError):
            part.residuals(X.t(), lists)                                              # a strided view never reaches the library
        with pytest.raises(TypeError):
            part.assign(X.double())
        with pytest.raises(TypeError):
            part.update(X, lists.long())


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------------------------------
N, D, M, NLIST, ILS = 2000, 16, 4, 8, 2


@pytest.fixture(scope="module")
def build(lsq, engine, torch):
    """the problem of the pipeline tests and the HOST statement of the build, made once: ivf_assign, numpy residuals run through the same encode call,
    code_norms_cpu -- shared and left unchanged"""
    rng = np.random.default_rng(77)
    centres = rng.standard_normal((NLIST, D)).astype(np.float32) * 6
    X = (centres[rng.integers(0, NLIST, N)] + rng.standard_normal((N, D))).astype(np.float32)
    K = (rng.standard_normal((M * H, D)) / M).astype(np.float32)
    Q = (centres[rng.integers(0, NLIST, 37)] + rng.standard_normal((37, D))).astype(np.float32)
    cent, assign = lsq.train_coarse(X, NLIST, 4, 3, engine)
    assert np.array_equal(assign, lsq.ivf_assign(X, cent))
    R = X - cent[assign]
    dK = torch.from_numpy(K).cuda()
    dB0 = engine.randinit_dev(5, N, M)
    dBs, _, _ = engine.encode_icm_dev(torch.from_numpy(R).cuda(), dB0, dK, M, [ILS], 2, 2, True, seed=5)
    codes = dBs[-1].cpu().numpy()
    rc, norms, _, _ = pc.code_norms_cpu(lsq._lib.load(), codes, K, cent, assign)
    assert rc == 0
    cb = np.quantile(norms, np.linspace(0, 1, 256)).astype(np.float32)
    rc, _, nc, dbn = pc.code_norms_cpu(lsq._lib.load(), codes, K, cent, assign, cb)
    assert rc == 0
    return dict(X=X, K=K, Q=Q, cent=cent, assign=assign, codes=codes, norms=norms, cb=cb, nc=nc, dbn=dbn, dK=dK, dB0=dB0)


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_train_coarse_dev_is_train_coarse(lsq, engine, torch, build, u8):
    X = np.clip(build["X"] * 8 + 128, 0, 255).astype(np.uint8) if u8 else build["X"]
    cent, assign = (lsq.train_coarse(X, NLIST, 4, 3, engine) if u8 else (build["cent"], build["assign"]))
    part, dassign = lsq.train_coarse_dev(torch.from_numpy(X).cuda(), NLIST, 4, 3, engine=engine)
    with part:
        assert same_bits(part.centroids().cpu().numpy(), cent) and np.array_equal(dassign.cpu().numpy(), assign)
        assert dassign.dtype == torch.int32 and part.nlist == NLIST and part.d == D


@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
def test_the_device_build_searches_like_the_host_statement(lsq, engine, torch, build, packed):
    b = build
    dX, dQ = torch.from_numpy(b["X"]).cuda(), torch.from_numpy(b["Q"]).cuda()
    with engine.partition_dev(torch.from_numpy(b["cent"]).cuda()) as part:
        ix = lsq.build_ivf_residual_index(dX, part, b["dK"], M, engine=engine, ilsiters=ILS, icmiter=2, npert=2, randord=True, seed=5, dB0=b["dB0"],
                                          cbnorms=b["cb"] if packed else None)
    ref = (engine.index_packed(b["codes"], b["K"], b["nc"], b["cb"], M) if packed else engine.index(b["codes"], b["K"], b["norms"], M))
    ref.set_lists(b["cent"], b["assign"])
    with ix, ref:
        assert ix.nlist == NLIST and bool(ix.packed_info()["row_bytes"]) == packed
        for nprobe in (1, 3, 8):
            dd, di = ix.search_ivf(dQ, 10, nprobe, add_coarse=True)
            rd, ri = ref.search_ivf(b["Q"], 10, nprobe, add_coarse=True)
            assert same_bits(dd.cpu().numpy(), rd) and np.array_equal(di.cpu().numpy(), ri), nprobe
            if packed:
                continue
            # the distances are |q - c_l - r^|^2: float64, the tolerance of the same identity in tests/test_ivf.py
            ids = ri.astype(np.int64) - 1
            recon = sum(b["K"][j * H + b["codes"][:, j].astype(np.int64)] for j in range(M)).astype(np.float64)
            full = b["cent"][b["assign"]].astype(np.float64) + recon
            want = ((b["Q"][:, None, :].astype(np.float64) - full[ids]) ** 2).sum(2)
            print("nprobe", nprobe, "max |dist - f64|", float(np.abs(rd - want).max()))
            assert np.all(ids >= 0) and np.allclose(rd, want, rtol=1e-5, atol=1e-4)


def test_the_device_build_takes_uint8_rows(lsq, engine, torch, build):
    """8-bit rows stay 8-bit: the index built from them is the index built from the widened rows"""
    X8 = np.clip(build["X"] * 8 + 128, 0, 255).astype(np.uint8)
    kw = dict(engine=engine, ilsiters=[ILS], icmiter=2, npert=2, randord=True, seed=9)
    dQ = torch.from_numpy(build["Q"] * 8 + 128).cuda()
    out = []
    for dX in (torch.from_numpy(X8).cuda(), torch.from_numpy(X8.astype(np.float32)).cuda()):
        part, _ = lsq.train_coarse_dev(dX, NLIST, 2, 1, engine=engine)
        with part, lsq.build_ivf_residual_index(dX, part, build["dK"] * 8, M, **kw) as ix:
            out.append([t.cpu().numpy() for t in ix.search_ivf(dQ, 5, 3, add_coarse=True)])
    assert same_bits(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ---- neighbours -----------------------------------------------------------------------------------------------------------------------------------------
def test_partition_calls_leave_the_context_and_its_indexes_alone(lsq, engine, torch, build):
    b = build

    def work(eng, ix):
        dBs, sums, stats = eng.encode_icm_dev(torch.from_numpy(b["X"]).cuda(), b["dB0"], b["dK"], M, [ILS], 2, 2, True, seed=11)
        dd, di = ix.search(torch.from_numpy(b["Q"]).cuda(), 10)
        return dBs.cpu().numpy(), np.asarray(sums), np.asarray(stats), dd.cpu().numpy(), di.cpu().numpy()

    def index_of(eng):
        return eng.index_dev(torch.from_numpy(b["codes"]).cuda(), b["dK"], torch.from_numpy(b["norms"]).cuda(), M)

    with lsq.Engine(0) as fresh, index_of(fresh) as fix:
        want = work(fresh, fix)
    with index_of(engine) as ix, engine.partition_dev(torch.from_numpy(b["cent"]).cuda()) as part:
        before = work(engine, ix)
        dX = torch.from_numpy(b["X"]).cuda()
        dassign = part.assign(dX)
        part.update(dX, dassign)
        part.residuals(dX, dassign)
        part.code_norms(torch.from_numpy(b["codes"]).cuda(), b["dK"], dassign)
        after = work(engine, ix)
    for got in (before, after):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert same_bits(got[3], want[3]) and np.array_equal(got[4], want[4])


# ---- many lists: 2^16 .. 2^24 centroids ---------------------------------------------------------------------------------------------------------------
MANY, BOUND = ic.MANY, ic.BOUND


def _nearest_search(engine, torch, cent, X):
    """the search an assignment borrows, on its own: engine.knn_exact_dev(centroids, rows, 1) -> its statistics, fallback_queries this call's alone"""
    before = engine.linscan_stats()["fallback_queries"]
    engine.knn_exact_dev(torch.from_numpy(cent).cuda(), torch.from_numpy(np.ascontiguousarray(X)).cuda(), 1)
    st = engine.linscan_stats()
    st["fallback_queries"] -= before
    return st


OPTIONS = (None, "linscan_exhaustive", "linscan_rank")      # the context's coarse roads: default, every query exhaustive, every query redone (rank 1)


@contextlib.contextmanager
def _option(engine, option):
    """the shared context under one search option, reset whatever happens"""
    if option:
        engine.set_option(option, 1)
    try:
        yield
    finally:
        engine.set_option("linscan_rank", 0)
        engine.set_option("linscan_exhaustive", 0)


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("nlist", [65536, 65537])
def test_assign_on_either_side_of_the_sampled_search(lsq, engine, torch, nlist, u8):
    """reaches: Partition.assign through the exhaustive road (65 536 centroids) and the sampled one (65 537), and the context's two search options handed
    to it.  Evidence: the direct nearest-centroid search's statistics under the same options"""
    cent, X = pc.assign_problem(nlist, u8)
    n = X.shape[0]
    want = lsq.ivf_assign(X, cent)                                                    # the host cores
    ref, acc = pc.assign_np(X[:200], cent)
    wdist = acc[np.arange(200), ref]
    assert np.array_equal(want[:200], ref) and want[n // 2] == pc.TIE[0] and want[7] == 123
    views = (X, pc.row_view(X, 1, offset=3) if u8 else pc.row_view(X, 3, offset=1))
    with engine.partition_dev(torch.from_numpy(cent).cuda()) as part, engine.partition(cent) as hpart:
        for option in OPTIONS:
            with _option(engine, option):
                for v in views:
                    got, dist = part.assign(to_dev(torch, v)[0], want_dist=True)
                    assert np.array_equal(got.cpu().numpy(), want) and same_bits(dist.cpu().numpy()[:200], wdist), (option, v.strides)
                    hgot, hdist = hpart.assign(v, want_dist=True)
                    assert np.array_equal(hgot, want) and same_bits(hdist[:200], wdist), (option, v.strides)
                assert part.info()["call"] == lsq._lib.PARTITION_ASSIGN and part.info()["rows"] == n
                st = _nearest_search(engine, torch, cent, X.astype(np.float32))
            assert st["exhaustive"] == (1 if option == "linscan_exhaustive" or nlist <= 65536 else 0), (option, st)
            if nlist > 65536 and option is None:
                assert st["threshold_rank"] == 10 and st["list_capacity"] == 320 and st["fallback_queries"] < n      # select_model.plan(65537, 1)
            if nlist > 65536 and option == "linscan_rank":                            # (one neighbour: the sample's minimum serves its query)
                assert st["threshold_rank"] == 1


def test_assign_with_duplicated_centroids(lsq, engine, torch):
    """reaches: an assignment whose coarse batch is mixed -- the rows beside 40 000 equal centroids overflow their candidate lists and are redone, the
    others are served.  Evidence: the direct search's 1 <= fallback_queries < n"""
    cent, X = pc.duplicated_centroids()
    want = lsq.ivf_assign(X, cent)
    ref, acc = pc.assign_np(X, cent)
    assert np.array_equal(want, ref) and np.all(want[:100] == 5000)
    with engine.partition_dev(torch.from_numpy(cent).cuda()) as part, engine.partition(cent) as hpart:
        got, dist = part.assign(torch.from_numpy(X).cuda(), want_dist=True)
        assert np.array_equal(got.cpu().numpy(), want) and same_bits(dist.cpu().numpy(), acc[np.arange(X.shape[0]), ref])
        assert np.array_equal(hpart.assign(X), want)
    st = _nearest_search(engine, torch, cent, X)
    assert st["exhaustive"] == 0 and 1 <= st["fallback_queries"] < X.shape[0], st
    assert st["fallback_queries"] == ic.coarse_stats(cent, X, 1)["fallback_queries"]


def test_update_at_65537_lists(lsq, engine, torch):
    """reaches: update_kernel on 65 537 blocks, about 1200 of which find their list empty; the grouping sort on 49 key bits behind an update.
    Evidence: partition info's empty_lists, lists_touched and max_list_rows, exact (_update_both)"""
    X = pc.decades(262148, 5, 6)
    assign = lists_for(262148, MANY, 5)
    cent = np.random.default_rng(2).standard_normal((MANY, 5)).astype(np.float32)
    got, counts = _update_both(lsq, engine, torch, cent, X, assign)
    want, wc = pc.update_np(cent, X, assign)
    assert same_bits(got, want) and np.array_equal(counts, wc) and 500 < int((wc == 0).sum()) < 2000
    assert same_bits(got[wc == 0], cent[wc == 0])                                     # empty lists keep their centroid's bits
    _timed_update(engine, torch, cent, X, assign)


def _timed_update(engine, torch, cent, X, assign):
    """one device-form update on resident tensors, its wall time printed -> the handle's info"""
    with engine.partition_dev(torch.from_numpy(cent).cuda()) as part:
        dX, dassign = torch.from_numpy(X).cuda(), torch.from_numpy(assign).cuda()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        part.update(dX, dassign)
        torch.cuda.synchronize()
        print("update at nlist = %d, n = %d, d = %d, device form: %.4f s" % (cent.shape[0], X.shape[0], X.shape[1], time.perf_counter() - t0))
        return part.info()


def test_update_at_the_contracts_bound(lsq, engine, torch):
    """reaches: update_kernel on 2^24 blocks of which 950 have rows (2^24 - 950 atomic adds on one word), ivf_offsets_kernel's threads opening runs of
    tens of thousands of empty lists, counts of 2^24 entries.  Evidence: partition info's empty_lists = 2^24 - 950, exact"""
    (_, _, _, cent, assign, _, _), _, _ = ic.bound_problem()
    X = pc.decades(assign.shape[0], 2, 8)
    got, counts = _update_both(lsq, engine, torch, cent, X, assign)
    want, wc = pc.update_np(cent, X, assign)
    assert same_bits(got, want) and np.array_equal(counts, wc) and int((wc == 0).sum()) == BOUND - 950 and int(wc.max()) == 26
    info = _timed_update(engine, torch, cent, X, assign)
    assert (info["empty_lists"], info["lists_touched"], info["max_list_rows"]) == (BOUND - 950, 950, 26)


def _residuals_and_code_norms(lsq, engine, torch, nlist, d, lists, n=257, m=3):
    L = lsq._lib.load()
    codes, K, cent, _ = pc.code_problem(n, d, m, nlist, d + nlist % 1000)
    assign = np.resize(np.asarray(lists, dtype=np.int32), n)
    X = np.random.default_rng(d).standard_normal((n, d)).astype(np.float32)
    rc, wantR = pc.residuals_cpu(L, X, cent, assign)
    rc2, ws, _, _ = pc.code_norms_cpu(L, codes, K, cent, assign)
    assert rc == 0 and rc2 == 0 and not same_bits(wantR, X)
    with engine.partition_dev(torch.from_numpy(cent).cuda()) as part, engine.partition(cent) as hpart:
        dassign = torch.from_numpy(assign).cuda()
        assert pc.same(part.residuals(torch.from_numpy(X).cuda(), dassign).cpu().numpy(), wantR) and pc.same(hpart.residuals(X, assign), wantR)
        assert part.info()["call"] == lsq._lib.PARTITION_RESIDUALS and part.info()["rows"] == n
        assert pc.same(part.code_norms(torch.from_numpy(codes).cuda(), torch.from_numpy(K).cuda(), dassign).cpu().numpy(), ws)
        assert pc.same(hpart.code_norms(codes, K, assign), ws)
        assert part.nlist == nlist and int(assign.max()) == nlist - 1


@pytest.mark.parametrize("d", [5, 128])
def test_residuals_and_code_norms_read_the_last_centroids_of_65537(lsq, engine, torch, d):
    """reaches: residual_kernel / code_norms_kernel at centroid offsets l * d for l = 0, 65 535, 65 536 = nlist - 1 (the first l past 16 bits).
    Evidence: the rows' lists and the handle's nlist"""
    _residuals_and_code_norms(lsq, engine, torch, MANY, d, [0, 65535, 65536, MANY - 1])


def test_residuals_and_code_norms_read_the_last_centroid_of_the_bound(lsq, engine, torch):
    """reaches: the same kernels at l = 2^24 - 1, d = 2: the last centroid row the contract allows"""
    _residuals_and_code_norms(lsq, engine, torch, BOUND, 2, [BOUND - 1, 0, BOUND - 1, 65536])


def test_train_coarse_dev_is_train_coarse_at_65537_lists(lsq, engine, torch):
    """reaches: assign and update alternated on 65 537 centroids (the sampled search with 70 000 queries, most lists of one row); the baseline runs the
    context's exact search through host buffers, another caller of the same selection.  Evidence: bit-equal centroids, 500 rows held to the host cores"""
    X = np.random.default_rng(21).standard_normal((70000, 4)).astype(np.float32)
    cent, assign = lsq.train_coarse(X, MANY, 2, 3, engine)
    part, dassign = lsq.train_coarse_dev(torch.from_numpy(X).cuda(), MANY, 2, 3, engine=engine)
    with part:
        assert part.nlist == MANY and same_bits(part.centroids().cpu().numpy(), cent) and np.array_equal(dassign.cpu().numpy(), assign)
    rows = np.arange(0, 70000, 140)
    assert np.array_equal(assign[rows], lsq.ivf_assign(X[rows], cent))                # the host cores
    assert _nearest_search(engine, torch, cent, X[rows])["exhaustive"] == 0


BN, BD, BM = 70000, 16, 4


@pytest.fixture(scope="module")
def big_build(lsq, engine, torch):
    """`build` at 65 537 lists: the centroids are 65 537 rows of X (train_coarse without a Lloyd step: every list holds its own seed row, none is empty),
    and the HOST statement of the build on them, made once"""
    rng = np.random.default_rng(78)
    X = rng.standard_normal((BN, BD)).astype(np.float32)
    K = (rng.standard_normal((BM * H, BD)) / BM).astype(np.float32)
    Q = (X[rng.integers(0, BN, 37)] + np.float32(0.05) * rng.standard_normal((37, BD))).astype(np.float32)
    cent, assign = lsq.train_coarse(X, MANY, 0, 3, engine)
    rows = np.arange(0, BN, 140)
    assert np.array_equal(assign[rows], lsq.ivf_assign(X[rows], cent)) and np.bincount(assign, minlength=MANY).min() >= 1
    R = X - cent[assign]
    dK = torch.from_numpy(K).cuda()
    dB0 = engine.randinit_dev(5, BN, BM)
    dBs, _, _ = engine.encode_icm_dev(torch.from_numpy(R).cuda(), dB0, dK, BM, [ILS], 2, 2, True, seed=5)
    codes = dBs[-1].cpu().numpy()
    rc, norms, _, _ = pc.code_norms_cpu(lsq._lib.load(), codes, K, cent, assign)
    assert rc == 0
    cb = np.quantile(norms, np.linspace(0, 1, 256)).astype(np.float32)
    rc, _, nc, dbn = pc.code_norms_cpu(lsq._lib.load(), codes, K, cent, assign, cb)
    assert rc == 0
    return dict(X=X, K=K, Q=Q, cent=cent, assign=assign, codes=codes, norms=norms, cb=cb, nc=nc, dbn=dbn, dK=dK, dB0=dB0)


@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
def test_the_device_build_at_65537_lists_searches_like_the_host_statement(lsq, engine, torch, big_build, packed):
    """reaches: build_ivf_residual_index on 65 537 lists -- assign, residuals, code_norms and set_lists at that nlist in one chain -- and its search at
    nprobe = 1 (one list of one or two rows) and 64.  Evidence: Index.nlist, no padding in the reference's ids"""
    b = big_build
    dX, dQ = torch.from_numpy(b["X"]).cuda(), torch.from_numpy(b["Q"]).cuda()
    with engine.partition_dev(torch.from_numpy(b["cent"]).cuda()) as part:
        ix = lsq.build_ivf_residual_index(dX, part, b["dK"], BM, engine=engine, ilsiters=ILS, icmiter=2, npert=2, randord=True, seed=5, dB0=b["dB0"],
                                          cbnorms=b["cb"] if packed else None)
    ref = (engine.index_packed(b["codes"], b["K"], b["nc"], b["cb"], BM) if packed else engine.index(b["codes"], b["K"], b["norms"], BM))
    ref.set_lists(b["cent"], b["assign"])
    with ix, ref:
        assert ix.nlist == MANY and bool(ix.packed_info()["row_bytes"]) == packed
        for nprobe, nn in ((1, 1), (64, 10)):
            dd, di = ix.search_ivf(dQ, nn, nprobe, add_coarse=True)
            rd, ri = ref.search_ivf(b["Q"], nn, nprobe, add_coarse=True)
            assert ic.padding_ok(ri) and np.all(ri > 0)
            assert same_bits(dd.cpu().numpy(), rd) and np.array_equal(di.cpu().numpy(), ri), nprobe
            if packed:
                continue
            # the distances are |q - c_l - r^|^2: float64, the tolerance of the same identity in tests/test_ivf.py
            ids = ri.astype(np.int64) - 1
            recon = sum(b["K"][j * H + b["codes"][:, j].astype(np.int64)] for j in range(BM)).astype(np.float64)
            full = b["cent"][b["assign"]].astype(np.float64) + recon
            want = ((b["Q"][:, None, :].astype(np.float64) - full[ids]) ** 2).sum(2)
            print("nlist 65537 nprobe", nprobe, "max |dist - f64|", float(np.abs(rd - want).max()))
            assert np.allclose(rd, want, rtol=1e-5, atol=1e-4)


# ---- small routes --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_counts", [False, True], ids=["no-counts", "counts"])
def test_update_without_rows_keeps_the_centroids(lsq, engine, torch, want_counts):
    """n = 0 has a branch of its own: the centroids keep their bits, the counts are zeroed on either side, info = (UPDATE, rows 0, empty_lists nlist)"""
    cent = np.random.default_rng(1).standard_normal((9, 5)).astype(np.float32)
    with engine.partition_dev(torch.from_numpy(cent).cuda()) as part, engine.partition(cent) as hpart:
        for p, X, lists in ((part, torch.zeros(0, 5, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")),
                            (hpart, np.zeros((0, 5), np.float32), np.zeros(0, np.int32)),
                            (hpart, np.zeros((0, 5), np.uint8), np.zeros(0, np.int32))):
            if want_counts and p._dev:                                                # (the wrapper hands over zeroed counts: fill the raw call's by hand)
                counts = torch.full((9,), -7, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                assert lsq._lib.load().lsq_partition_update(p._h, None, 0, 0, 5, None, counts.data_ptr(), 1) == 0
                assert bool((counts == 0).all())
            elif want_counts:
                counts = np.full(9, -7, np.int32)
                assert lsq._lib.load().lsq_partition_update(p._h, None, int(X.dtype == np.uint8), 0, 5, None, counts.ctypes.data, 0) == 0
                assert not counts.any()
            got = p.update(X, lists, want_counts=want_counts)
            assert (got is None) == (not want_counts) and (got is None or not np.asarray(got.cpu() if p._dev else got).any())
            info = p.info()
            assert (info["call"], info["rows"], info["empty_lists"], info["lists_touched"]) == (lsq._lib.PARTITION_UPDATE, 0, 9, 0)
            after = p.centroids()
            assert same_bits(after.cpu().numpy() if p._dev else after, cent)


def test_host_forms_without_rows_write_nothing(lsq, engine):
    """n = 0 through the raw symbols (the wrapper returns before the library for an empty array): success, nothing written, null pointers allowed"""
    L = lsq._lib.load()
    cent = np.random.default_rng(2).standard_normal((4, 8)).astype(np.float32)
    lists, dist, R, norms = np.full(3, -7, np.int32), np.full(3, -7, np.float32), np.full((3, 8), -7, np.float32), np.full(3, -7, np.float32)
    K, codes = np.zeros((2 * H, 8), np.float32), np.zeros((3, 2), np.uint8)
    with engine.partition(cent) as part:
        h, x = part._h, R.ctypes.data
        assert L.lsq_partition_assign(h, x, 0, 0, 8, lists.ctypes.data, dist.ctypes.data, 0) == 0 and L.lsq_partition_assign(h, None, 0, 0, 8, None, None, 0) == 0
        assert L.lsq_partition_residuals(h, x, 0, 0, 8, lists.ctypes.data, R.ctypes.data, 8, 0) == 0
        assert L.lsq_partition_residuals(h, None, 1, 0, 8, None, None, 8, 0) == 0
        assert L.lsq_partition_code_norms(h, codes.ctypes.data, K.ctypes.data, 0, 2, H, lists.ctypes.data, None, 0, norms.ctypes.data, None, None, 0) == 0
        assert L.lsq_partition_code_norms(h, None, K.ctypes.data, 0, 2, H, None, None, 0, norms.ctypes.data, None, None, 0) == 0
        assert np.all(lists == -7) and np.all(dist == -7) and np.all(R == -7) and np.all(norms == -7)
        assert part.assign(np.zeros((0, 8), np.float32)).shape == (0,) and part.residuals(np.zeros((0, 8), np.float32), np.zeros(0, np.int32)).shape == (0, 8)
        assert part.code_norms(np.zeros((0, 2), np.uint8), K, np.zeros(0, np.int32)).shape == (0,)
        assert same_bits(part.centroids(), cent)


def test_a_closed_engine_closes_its_partitions(lsq):
    cent = np.random.default_rng(3).standard_normal((5, 4)).astype(np.float32)
    X = np.random.default_rng(4).standard_normal((50, 4)).astype(np.float32)
    eng = lsq.Engine(0)
    part = eng.partition(cent)
    want = part.assign(X)
    eng.close()
    assert part._h is None
    part.close()                                                                      # and closing it again is harmless
    with lsq.Engine(0) as eng2, eng2.partition(cent) as part2:
        assert np.array_equal(part2.assign(X), want) and np.array_equal(want, lsq.ivf_assign(X, cent))
