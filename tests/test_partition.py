"""The coarse partition without a GPU: the three host checkers against the numpy statement of their contracts (tests/partition_check.py), the boundary
(header, both libraries, binding, version) and every argument the library refuses before it needs a device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import partition_check as pc  # noqa: E402
from knn_check import same_bits  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 256
HANDLE = ("lsq_partition_create", "lsq_partition_destroy", "lsq_partition_get_centroids", "lsq_partition_get_info", "lsq_partition_assign",
          "lsq_partition_update", "lsq_partition_residuals", "lsq_partition_code_norms")
CHECKERS = ("lsq_partition_update_cpu", "lsq_partition_residuals_cpu", "lsq_partition_code_norms_cpu")


def test_boundary_declares_exports_and_binds_the_eleven_symbols(lsq):
    hdr = open(os.path.join(ROOT, "include", "lsq_mi355x.h")).read()
    assert int(re.search(r"#define LSQ_VERSION (\d+)", hdr).group(1)) >= 1900
    L, tun = lsq._lib.load(), lsq._lib.load(tuning=True)
    assert L.lsq_version() >= 1900 and tun.lsq_version() >= 1900
    for s in HANDLE + CHECKERS:
        assert re.search(r"LSQ_API int %s\(" % s, hdr), s
        assert s in lsq._lib.SIGNATURES and hasattr(L, s) and hasattr(tun, s)
    # no new symbol takes the context first: the closed catalogues of the context walks stay closed
    first = set(re.findall(r"\b(lsq_\w+)\s*\(\s*(?:struct\s+)?lsq_ctx\s*\*", hdr))
    assert not any(s.startswith("lsq_partition") for s in first)
    assert re.search(r"lsq_partition_create\(lsq_partition \*\*out, lsq_ctx \*ctx, const lsq_partition_desc \*desc\)", hdr)
    for s in HANDLE[1:]:
        assert re.search(r"LSQ_API int %s\(lsq_partition \*p\b" % s, hdr), "%s does not take the handle first" % s
    for name, struct in (("lsq_partition_info", lsq._lib.PartitionInfo), ("lsq_partition_desc", lsq._lib.PartitionDesc)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S).group(1)
        fields = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert fields == [f for f, _ in struct._fields_], name
    assert "(3i)" in hdr and re.search(r"NO COUNTERPART", hdr)
    for name in ("train_coarse_dev", "build_ivf_residual_index", "Partition"):
        assert callable(getattr(lsq, name))
    assert all(hasattr(lsq.Partition, f) for f in ("assign", "update", "residuals", "code_norms", "centroids", "info"))
    assert all(hasattr(lsq.Engine, f) for f in ("partition", "partition_dev"))


def test_handle_symbols_refuse_a_null_handle(lsq):
    L, EINVAL = lsq._lib.load(), lsq._lib.LSQ_EINVAL
    buf, ibuf, info, desc = np.zeros(64, np.float32), np.zeros(64, np.int32), lsq._lib.PartitionInfo(), lsq._lib.PartitionDesc()
    b, i = buf.ctypes.data, ibuf.ctypes.data
    out = C.c_void_p()
    desc.nlist, desc.d, desc.centroids = 2, 4, b
    assert L.lsq_partition_create(C.byref(out), None, C.byref(desc)) == EINVAL and not out.value      # a null context
    assert L.lsq_partition_create(None, None, C.byref(desc)) == EINVAL
    assert L.lsq_partition_destroy(None) == 0                                                          # like every destroy here
    assert L.lsq_partition_get_centroids(None, b, 0) == EINVAL
    assert L.lsq_partition_get_info(None, C.byref(info)) == EINVAL
    assert L.lsq_partition_assign(None, b, 0, 4, 4, i, None, 0) == EINVAL
    assert L.lsq_partition_update(None, b, 0, 4, 4, i, None, 0) == EINVAL
    assert L.lsq_partition_residuals(None, b, 0, 4, 4, i, b, 4, 0) == EINVAL
    assert L.lsq_partition_code_norms(None, i, b, 4, 1, H, i, None, 0, b, None, None, 0) == EINVAL
    assert b"null partition" in L.lsq_last_error()


# ---- update -------------------------------------------------------------------------------------------------------------------------------------------
def test_np_add_at_is_the_sequential_float64_loop():
    """the identity the contract rests on, on the decade-spanning data"""
    X = pc.decades(5000, 5, 3)
    assign = np.random.default_rng(1).integers(0, 7, 5000).astype(np.int32)
    cent = np.zeros((9, 5), np.float32)
    a, ca = pc.update_np(cent, X, assign)
    b, cb = pc.update_loop(cent, X, assign)
    assert same_bits(a, b) and np.array_equal(ca, cb)
    # and a float32 sum is another number: the data can tell the accumulators apart
    f32 = np.zeros((9, 5), np.float32)
    np.add.at(f32, assign, X)
    live = ca > 0
    assert not same_bits((f32[live] / ca[live, None]).astype(np.float32), a[live])


@pytest.mark.parametrize("threads", [0, 1, 3])
def test_update_cpu_is_the_numpy_statement_on_decade_spanning_rows(lsq, threads):
    L = lsq._lib.load()
    X = pc.decades(5000, 5, 3)
    assign = np.random.default_rng(1).integers(0, 7, 5000).astype(np.int32)          # lists 7 and 8 stay empty
    cent = np.random.default_rng(2).standard_normal((9, 5)).astype(np.float32)
    rc, got, counts = pc.update_cpu(L, cent, X, assign, threads)
    want, wc = pc.update_np(cent, X, assign)
    assert rc == 0 and same_bits(got, want) and np.array_equal(counts, wc)
    assert same_bits(got[7:], cent[7:]) and not counts[7:].any()                      # a list without rows keeps its centroid's bits
    # a float32 accumulation would differ
    f32 = np.zeros((9, 5), np.float32)
    np.add.at(f32, assign, X)
    assert not same_bits((f32[:7] / wc[:7, None]).astype(np.float32), want[:7])


def test_update_cpu_on_row_views_uint8_rows_and_the_list_ladder(lsq):
    L = lsq._lib.load()
    assign, nlist = pc.ladder_lists()
    n = assign.shape[0]
    rng = np.random.default_rng(8)
    for d in (1, 5, 130):
        cent = rng.standard_normal((nlist, d)).astype(np.float32)
        Xf = pc.row_view(pc.decades(n, d, d), 3, offset=1)
        X8 = pc.row_view(rng.integers(0, 256, (n, d)).astype(np.uint8), 5, offset=3)
        for X in (Xf, X8):
            rc, got, counts = pc.update_cpu(L, cent, X, assign)
            want, wc = pc.update_np(cent, np.ascontiguousarray(X), assign)
            assert rc == 0 and same_bits(got, want) and np.array_equal(counts, wc), (d, X.dtype)
            assert sorted(wc[wc > 0]) == list(range(1, 2 * pc.PREFETCH + 2))
    # nlist > n, one-row lists, one list holding every row
    X = pc.decades(6, 4, 1)
    for lists, nl in ((np.arange(6, dtype=np.int32)[::-1] * 3, 20), (np.full(6, 4, np.int32), 5)):
        cent = rng.standard_normal((nl, 4)).astype(np.float32)
        rc, got, counts = pc.update_cpu(L, cent, X, lists)
        want, wc = pc.update_np(cent, X, lists)
        assert rc == 0 and same_bits(got, want) and np.array_equal(counts, wc)


# ---- many lists: the problems of tests/test_gpu_partition.py above 65 536 lists, from the host alone ----------------------------------------------------
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("nlist", [65536, 65537])
def test_assign_problem_has_its_tie_and_its_zero_distance(lsq, nlist, u8):
    """the host cores (ivf_assign) against the numpy statement on the rows the device's distances are held to"""
    cent, X = pc.assign_problem(nlist, u8)
    rows = np.r_[0:198, 7, X.shape[0] // 2]
    want = lsq.ivf_assign(X[rows], cent)
    ref, acc = pc.assign_np(X[rows], cent)
    assert np.array_equal(want, ref) and X.dtype == (np.uint8 if u8 else np.float32) and cent.shape == (nlist, 8)
    assert want[-1] == pc.TIE[0] and 7.9 < acc[-1, pc.TIE[0]] == acc[-1, pc.TIE[1]] < 8.1 and want[-2] == 123 and acc[-2, 123] == 0
    assert len(set(want.tolist())) > 150                                              # the rows spread over the lists


def test_duplicated_centroids_split_the_rows_of_a_coarse_search():
    """by the model of the selection: the rows beside the 40 000 equal centroids overflow their candidate lists, and not every row does"""
    import ivf_check as ic
    cent, X = pc.duplicated_centroids()
    st = ic.coarse_stats(cent, X, 1)
    assert st["exhaustive"] == 0 and 100 <= st["fallback_queries"] < X.shape[0]
    assert np.all(pc.assign_np(X[:100], cent)[0] == 5000)


def test_update_cpu_is_the_numpy_statement_at_65537_lists(lsq):
    X = pc.decades(262148, 5, 6)
    assign = np.random.default_rng(5).integers(0, 65537, 262148).astype(np.int32)
    cent = np.random.default_rng(2).standard_normal((65537, 5)).astype(np.float32)
    rc, got, counts = pc.update_cpu(lsq._lib.load(), cent, X, assign)
    want, wc = pc.update_np(cent, X, assign)
    assert rc == 0 and same_bits(got, want) and np.array_equal(counts, wc) and 500 < (wc == 0).sum() < 2000
    assert same_bits(got[wc == 0], cent[wc == 0])


# ---- residuals ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 4, 5, 16, 127, 128, 130])
def test_residuals_cpu_is_the_numpy_statement(lsq, d):
    L = lsq._lib.load()
    rng = np.random.default_rng(d)
    n, nlist = 257, 300
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    assign = rng.integers(0, nlist, n).astype(np.int32)
    Xf = rng.standard_normal((n, d)).astype(np.float32)
    Xf, cent = pc.special_rows(Xf, cent, d)
    X8 = rng.integers(0, 256, (n, d)).astype(np.uint8)
    for X in (pc.row_view(Xf, 3, offset=1), pc.row_view(X8, 1, offset=3), Xf, X8):
        out = pc.row_view(np.full((n, d), 55, np.float32), 2)
        rc, R = pc.residuals_cpu(L, X, cent, assign, out=out)
        assert rc == 0 and pc.same(R, pc.residuals_np(np.ascontiguousarray(X), cent, assign)), X.dtype
        assert pc.untouched(out, 77)                                                  # nothing between or past the rows is touched
    R0 = pc.residuals_np(Xf, cent, assign)
    assert np.isnan(R0).any() and np.isinf(R0).any()
    neg0 = np.zeros((1, d), np.float32)
    neg0[:] = -0.0
    rc, R = pc.residuals_cpu(L, neg0, np.zeros((1, d), np.float32), np.zeros(1, np.int32))
    assert rc == 0 and np.all(np.signbit(R))                                          # -0.0 - +0.0 = -0.0


# ---- code_norms ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,d", [(1, 1), (7, 4), (8, 6), (16, 128)])
@pytest.mark.parametrize("ncb", [1, 37, 256])
def test_code_norms_cpu_is_the_numpy_statement(lsq, m, d, ncb):
    L = lsq._lib.load()
    codes, K, cent, assign = pc.code_problem(300, d, m, 11, 7 * m + d)
    s = pc.code_norms_np(codes, K, cent, assign)
    rng = np.random.default_rng(ncb)
    cb = np.sort(rng.choice(s, ncb, replace=ncb > s.shape[0])).astype(np.float32)
    if ncb > 2:
        cb[ncb // 2] = cb[ncb // 2 - 1]                                               # a duplicated entry: the first one wins
    rc, norms, nc, dbn = pc.code_norms_cpu(L, codes, K, cent, assign, cb)
    ws, wnc, wdb = pc.code_norms_np(codes, K, cent, assign, cb)
    assert rc == 0 and same_bits(norms, ws) and np.array_equal(nc, wnc) and same_bits(dbn, wdb)
    if ncb > 2:
        assert not np.any(nc == ncb // 2)
    rc, norms1, nc1, dbn1 = pc.code_norms_cpu(L, codes, K, cent, assign, cb, nthreads=1)
    assert rc == 0 and same_bits(norms1, norms) and np.array_equal(nc1, nc)
    # without cbnorms only norms is written
    rc, norms2, nc2, dbn2 = pc.code_norms_cpu(L, codes, K, cent, assign, None)
    assert rc == 0 and same_bits(norms2, ws) and np.all(nc2 == 255) and np.all(dbn2 == -7)


def test_code_norms_cpu_with_nan_rows(lsq):
    L = lsq._lib.load()
    codes, K, cent, assign = pc.code_problem(200, 6, 3, 5, 2)
    K[codes[3, 0]] = np.nan
    cent[assign[9], 2] = np.nan
    cb = np.linspace(-5, 50, 19).astype(np.float32)
    rc, norms, nc, dbn = pc.code_norms_cpu(L, codes, K, cent, assign, cb)
    ws, wnc, wdb = pc.code_norms_np(codes, K, cent, assign, cb)
    assert rc == 0 and np.isnan(ws[3]) and np.isnan(ws[9]) and pc.same(norms, ws) and np.array_equal(nc, wnc) and pc.same(dbn, wdb)
    assert nc[3] == 0 and nc[9] == 0                                                  # a NaN norm is never nearer: the first entry stays


def test_code_norms_with_zero_centroids_are_quantize_norms(lsq):
    """a = the chain of lsq_quantize_norms, and with c = 0 the second chain stays +0.0: s has quantize_norms' bits, the codes its indices"""
    L = lsq._lib.load()
    codes, K, cent, assign = pc.code_problem(400, 32, 8, 4, 12)
    cb = np.linspace(0, 400, 64).astype(np.float32)
    rc, norms, nc, dbn = pc.code_norms_cpu(L, codes, K, np.zeros_like(cent), assign, cb)
    B = codes.astype(np.int16).T + 1                                                  # the reference layout: m x n, 1-based
    idx = lsq.quantize_norms(B, [np.ascontiguousarray(K[j * H:(j + 1) * H].T) for j in range(8)], cb)      # the mirror of lsq_quantize_norms, bit for bit
    assert rc == 0 and np.array_equal(nc.astype(np.int64) + 1, np.asarray(idx).reshape(-1)) and same_bits(dbn, cb[nc])
    recon = sum(K[j * H + codes[:, j].astype(np.int64)] for j in range(8))
    acc = np.zeros(400, np.float32)
    for t in range(32):
        acc = acc + recon[:, t] * recon[:, t]
    assert same_bits(norms, acc)


def test_code_norms_cpu_agrees_with_the_float64_residual_norms(lsq):
    L = lsq._lib.load()
    codes, K, cent, assign = pc.code_problem(600, 8, 2, 6, 5)
    rc, norms, _, _ = pc.code_norms_cpu(L, codes, K, cent, assign)
    assert rc == 0 and np.allclose(norms, lsq.ivf_residual_norms(codes, K, cent, assign), rtol=1e-5, atol=1e-4)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_host_checkers_refuse_bad_arguments(lsq):
    L, EINVAL = lsq._lib.load(), lsq._lib.LSQ_EINVAL
    n, d, nlist, m = 50, 6, 4, 2
    codes, K, cent, assign = pc.code_problem(n, d, m, nlist, 1)
    X = np.random.default_rng(0).standard_normal((n, d)).astype(np.float32)
    R, counts, norms = np.zeros((n, d), np.float32), np.zeros(nlist, np.int32), np.zeros(n, np.float32)
    cb = np.ones(3, np.float32)
    p = lambda a: a.ctypes.data      # noqa: E731
    upd = lambda **k: L.lsq_partition_update_cpu(*[k.get(a, v) for a, v in (("cent", p(cent)), ("counts", p(counts)), ("X", p(X)), ("u8", 0), ("n", n), ("d", d),      # noqa: E731
                                                                               ("ldx", d), ("lor", p(assign)), ("nlist", nlist), ("nt", 0))])
    res = lambda **k: L.lsq_partition_residuals_cpu(*[k.get(a, v) for a, v in (("R", p(R)), ("ldr", d), ("X", p(X)), ("u8", 0), ("n", n), ("d", d), ("ldx", d),      # noqa: E731
                                                                                  ("cent", p(cent)), ("lor", p(assign)), ("nlist", nlist), ("nt", 0))])
    cn = lambda **k: L.lsq_partition_code_norms_cpu(*[k.get(a, v) for a, v in (("norms", p(norms)), ("nc", None), ("dbn", None), ("codes", p(codes)), ("K", p(K)),      # noqa: E731
                                                                                 ("cent", p(cent)), ("lor", p(assign)), ("n", n), ("m", m), ("h", H), ("d", d),
                                                                                 ("nlist", nlist), ("cb", p(cb)), ("ncb", 3), ("nt", 0))])
    keep = cent.copy()
    assert upd() == 0 and res() == 0 and cn() == 0
    cent[:] = keep
    for call, bads in ((upd, [("cent", None), ("X", None), ("lor", None), ("n", -1), ("n", 2 ** 31 - 1), ("d", 0), ("ldx", d - 1), ("nlist", 0),
                              ("nlist", (1 << 24) + 1), ("X", p(X) + 1)]),
                       (res, [("R", None), ("X", None), ("cent", None), ("lor", None), ("n", -1), ("n", 2 ** 31 - 1), ("d", 0), ("ldx", d - 1), ("ldr", d - 1),
                              ("nlist", 0), ("nlist", (1 << 24) + 1), ("X", p(X) + 2)]),
                       (cn, [("codes", None), ("K", None), ("cent", None), ("lor", None), ("n", -1), ("m", 0), ("m", 17), ("h", 128), ("d", 0), ("nlist", 0),
                             ("ncb", 0), ("ncb", 257), ("n", 2 ** 31 - 1)])):
        for name, value in bads:
            assert call(**{name: value}) == EINVAL, (call, name, value)
    assert cn(cb=None, norms=None) == EINVAL                                          # without cbnorms the call needs norms
    assert upd(u8=1, X=p(X) + 1, ldx=4 * d) == 0                                      # uint8 rows at any byte offset
    cent[:] = keep
    for entry in (-1, nlist):                                                         # an entry outside [0, nlist): found before anything is written
        assign[17] = entry
        R[:] = 5
        assert upd() == EINVAL and b"list_of_row" in L.lsq_last_error() and np.array_equal(cent, keep)
        assert res() == EINVAL and np.all(R == 5)
        assert cn() == EINVAL
    assign[17] = 0
    assert upd(n=0) == 0 and res(n=0) == 0 and cn(n=0) == 0 and np.array_equal(cent, keep) and not counts.any()


def test_partition_device_forms_refuse_cpu_tensors(lsq):
    """before the library is reached: no Engine is needed to be refused"""
    import torch

    class NoEngine:
        _L = None
    part = object.__new__(lsq.Partition)
    part._bind(NoEngine(), True)
    part.nlist, part.d = 4, 8
    X, lists = torch.zeros(10, 8), torch.zeros(10, dtype=torch.int32)
    for call in (lambda: part.assign(X), lambda: part.update(X, lists), lambda: part.residuals(X, lists),
                 lambda: part.code_norms(torch.zeros(10, 2, dtype=torch.uint8), torch.zeros(2 * H, 8), lists)):
        with pytest.raises(TypeError, match="device tensor"):
            call()
    with pytest.raises(TypeError, match="device tensor"):
        lsq.Partition(NoEngine(), torch.zeros(4, 8), True)
    with pytest.raises(TypeError, match="int8"):
        hp = object.__new__(lsq.Partition)
        hp._bind(NoEngine(), False)
        hp.nlist, hp.d = 4, 8
        hp.assign(np.zeros((10, 8), np.int8))
