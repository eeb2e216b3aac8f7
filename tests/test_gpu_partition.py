"""The coarse partition on the device: every call of lsq_partition_* held bit for bit to its host checker (which tests/test_partition.py holds to the numpy
statement of the contract), host and device forms, at the smallest shapes at which each kernel can go wrong; then the two functions built on them,
train_coarse_dev and build_ivf_residual_index, against the host statement of the same build."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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
