"""Half-precision base rows on the device, against the numpy contract of tests/half_check.py.

  Identity N   lsq_index_narrow_base stores the bits of half_check.narrow -- read back through lsq_index_get_base -- and counts what narrowing destroyed.
  Identity W   an index over halves H answers every call that reads base rows (rerank, knn on its three filter roads, search / search_ivf with a
               shortlist) and every life-cycle step (add, remove, compact, add) as the index over the float32 matrix widen(H) on the same engine.

Every comparison is bit for bit, NaN for NaN.  Shapes are the smallest that reach each road of the kernels."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import half_check as HC  # noqa: E402
from rerank_check import rerank_cpu  # noqa: E402

pytestmark = pytest.mark.gpu
H = 256
FMTS = ["f16", "bf16"]
NAN_HALF = {"f16": 0x7E00, "bf16": 0x7FC0}


def _torch():
    import torch
    return torch


def _dev(a):
    """a host array as a device tensor; bf16 bits (uint16) travel as int16 and are viewed as bfloat16"""
    torch = _torch()
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.bfloat16)
    return torch.from_numpy(a).cuda()


def _view(rows, ldb, offset, fill):
    """rows (n, d) on the device as a view of pitch ldb elements, `offset` elements into a larger buffer whose other elements are `fill` -> (tensor view, keep)"""
    n, d = rows.shape
    big = np.full(offset + n * ldb + 64, fill, dtype=rows.dtype)
    body = big[offset:offset + n * ldb].reshape(n, ldb)
    body[:, :d] = rows
    flat = _dev(big)
    return flat[offset:offset + n * ldb].view(n, ldb)[:, :d], flat


def _call(ix, method, *arrays, **kw):
    """a method of an index on host arrays, whichever way the index was made -> numpy results"""
    if ix._dev:
        arrays = [_dev(a) if isinstance(a, np.ndarray) else a for a in arrays]
        kw = {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    out = getattr(ix, method)(*arrays, **kw)
    conv = lambda o: o.cpu().numpy() if hasattr(o, "cpu") else o             # noqa: E731
    return tuple(conv(o) for o in out) if isinstance(out, tuple) else conv(out)


def _same(a, b):
    return HC.same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])


def _counts(d):
    """a statistics dict without its times"""
    return {k: v for k, v in d.items() if not k.endswith("_ms")}


def _halves(X, fmt):
    """narrow(X) and its widening: (H as the host dtype of the format, W float32)"""
    Hh = HC.narrow(X, fmt)
    return Hh, HC.widen(Hh, fmt)


def _fill(fmt):
    return np.array([NAN_HALF[fmt]], np.uint16).view(HC.HOST_DTYPE[fmt])[0]


# ---- Identity N: narrowing on the device ----------------------------------------------------------------------------------------------------------------
def _narrow_problem(d, seed):
    rng = np.random.default_rng(seed)
    n = 300
    X = (rng.standard_normal((n, d)) * 100).astype(np.float32)
    e = np.concatenate([HC.edge_values(), HC.random_floats(rng, 200)])
    at = rng.choice(n * d, min(len(e), n * d), replace=False)
    X.reshape(-1)[at] = e[:len(at)]
    return X


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("d", [1, 7, 8, 9, 40])
def test_device_narrowing_stores_the_contracts_bits(lsq, engine, fmt, d):
    B = lsq._lib
    X = _narrow_problem(d, 10 * d + HC.FORMATS[fmt])
    n = X.shape[0]
    want = HC.widen(HC.narrow(X, fmt), fmt)
    cnt = HC.counts(X, fmt)
    assert cnt[2] > 0 and (d == 1 or (cnt[0] > 0 and cnt[1] > 0))
    nan32 = np.float32(np.nan)
    # (pitch, offset in floats): a 16-byte-aligned view whose pitch is a multiple of four floats (the 16-byte loads), and a view one float into the buffer
    # with an odd pitch (the dword loads); NaN between the rows
    for ldb, off in (((d + 4) // 4 * 4, 0), (d + 1 + (d % 2), 1), (d, 0)):
        view, keep = _view(X, ldb, off, nan32)
        with engine.index_dev(None, None, None, 0, base=view, base_format=fmt) as ix:      # create over f32, narrow on the device, let go of the tensor
            info = ix.base_info()
            assert (info["format"], info["elem_bytes"], info["ldb"], info["owned"], info["resident_bytes"]) == (HC.FORMATS[fmt], 2, d, 1, 2 * n * d)
            assert (info["to_inf"], info["to_zero"], info["nans"]) == cnt, (ldb, off)
            assert HC.same_bits(_call(ix, "base_rows"), want), (ldb, off)
        assert HC.same_bits(keep[off:off + n * ldb].view(n, ldb)[:, :d].cpu().numpy(), X)      # the borrowed rows are untouched
    # a host index: uploaded as f32 at its pitch, then narrowed
    big = np.full((n, d + 3), nan32)
    big[:, :d] = X
    with engine.index(None, None, None, 0, base=big, d=d) as ix:
        assert ix.base_info()["format"] == B.BASE_F32 and ix.base_info()["ldb"] == d + 3 and HC.same_bits(ix.base_rows(), X)
        ix.narrow_base(fmt)
        info = ix.base_info()
        assert (info["format"], info["ldb"], info["resident_bytes"]) == (HC.FORMATS[fmt], d, 2 * n * d) and (info["to_inf"], info["to_zero"], info["nans"]) == cnt
        assert HC.same_bits(ix.base_rows(), want)
    # ... and it is the index created over the host narrowing (Identity N: device and host give the same bits)
    with engine.index(None, None, None, 0, base=big[:, :d], base_format=fmt) as ix:
        assert ix.base_info()["format"] == HC.FORMATS[fmt] and HC.same_bits(ix.base_rows(), want)


def test_a_refused_narrowing_changes_nothing(lsq, engine):
    rng = np.random.default_rng(1)
    n, d, m = 200, 9, 2
    X = HC.matrix(rng, n, d)
    Q = rng.standard_normal((3, d)).astype(np.float32)
    codes, K, dbn = rng.integers(0, H, (n, m), dtype=np.uint8), rng.standard_normal((m * H, d)).astype(np.float32), rng.random(n).astype(np.float32)
    L = lsq._lib.load()
    with engine.index(codes, K, dbn, m) as ix:                               # no base rows
        with pytest.raises(lsq._lib.LsqError):
            ix.narrow_base("f16")
        with pytest.raises(lsq._lib.LsqError):
            ix.base_rows()
        assert ix.base_info()["format"] == 0 and ix.base_info()["resident_bytes"] == 0
    X8 = rng.integers(0, 256, (n, d), dtype=np.uint8)
    with engine.index(None, None, None, 0, base=X8) as ix:                   # a uint8 base
        before = ix.knn(Q, 5)
        with pytest.raises(lsq._lib.LsqError):
            ix.narrow_base("bf16")
        assert ix.base_info()["format"] == 1 and HC.same_bits(ix.base_rows(), X8.astype(np.float32)) and _same(ix.knn(Q, 5), before)
    with engine.index(None, None, None, 0, base=X) as ix:
        assert L.lsq_index_narrow_base(ix._h, 7) == -1 and L.lsq_index_narrow_base(ix._h, 0) == -1 and L.lsq_index_narrow_base(ix._h, 1) == -1      # format 7
        assert ix.base_info()["format"] == 0 and HC.same_bits(ix.base_rows(), X)
        ix.narrow_base("f16")
        rows, before, info = ix.base_rows(), ix.knn(Q, 5), ix.base_info()
        for again in ("f16", "bf16"):                                        # a second call: the base is no longer f32
            with pytest.raises(lsq._lib.LsqError):
                ix.narrow_base(again)
        assert ix.base_info() == info and HC.same_bits(ix.base_rows(), rows) and _same(ix.knn(Q, 5), before)


# ---- lsq_index_get_base ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "u8", "f16", "bf16"])
def test_get_base_returns_the_stored_rows(lsq, engine, kind):
    torch = _torch()
    rng = np.random.default_rng(5)
    n, d = 150, 19
    X = HC.matrix(rng, n, d)
    HC.special_rows(X, rng)
    if kind == "u8":
        rows = rng.integers(0, 256, (n, d), dtype=np.uint8)
        want, fill, kw = rows.astype(np.float32), np.uint8(255), {}
    elif kind == "f32":
        rows, want, fill, kw = X, X, np.float32(np.nan), {}
    else:
        rows, want = _halves(X, kind)
        fill, kw = _fill(kind), {"base_format": kind}
    padded = np.full((n, d + 2), fill, dtype=rows.dtype)
    padded[:, :d] = rows
    view, keep = _view(rows, d + 3, 1, fill)                                 # an odd pitch, one element into the buffer: nothing is aligned
    with engine.index(None, None, None, 0, base=padded[:, :d], **kw) as hix, engine.index_dev(None, None, None, 0, base=view) as dix:
        assert dix.base_info()["owned"] == 0 and hix.base_info()["owned"] == 1 and dix.base_info()["ldb"] == d + 3
        for ix in (hix, dix):
            assert HC.same_bits(_call(ix, "base_rows"), want)
            for start, count in ((0, 1), (n - 1, 1), (7, 64), (n, 0), (3, n - 3)):      # sub-ranges, the empty range at n included
                got = _call(ix, "base_rows", start=start, count=count)
                assert got.shape == (count, d) and HC.same_bits(got, want[start:start + count]), (start, count)
            assert _call(ix, "base_rows", start=n).shape == (0, d)
            for start, count in ((n + 1, 0), (-1, 1), (n - 1, 2), (0, n + 1)):      # refused before anything is written
                with pytest.raises(lsq._lib.LsqError):
                    ix.base_rows(start=start, count=count)
            with pytest.raises(ValueError):
                ix.base_rows(out=(torch.zeros((n, d - 1), device="cuda") if ix._dev else np.zeros((n, d - 1), np.float32)))      # ldo < d
        # a padded output pitch: the gaps are not written
        out = np.full((40, d + 5), np.float32(7.0))
        got = hix.base_rows(start=10, count=40, out=out[:, 2:2 + d + 1])
        assert HC.same_bits(got[:, :d], want[10:50]) and np.all(out[:, :2] == 7.0) and np.all(out[:, 2 + d:] == 7.0)
        tout = torch.full((40, d + 5), 7.0, device="cuda")
        dix.base_rows(start=10, count=40, out=tout[:, 1:1 + d])
        tout = tout.cpu().numpy()
        assert HC.same_bits(tout[:, 1:1 + d], want[10:50]) and np.all(tout[:, :1] == 7.0) and np.all(tout[:, 1 + d:] == 7.0)
        # the host form in staging chunks (the test hook of lsq_index_reconstruct): the same rows
        engine.set_option("recon_chunk", 7)
        try:
            assert HC.same_bits(hix.base_rows(start=2, count=n - 2), want[2:])
        finally:
            engine.set_option("recon_chunk", 0)
        # a filter changes nothing
        hix.set_filter(ids=np.arange(0, n, 3, dtype=np.int32))
        assert HC.same_bits(hix.base_rows(), want)


# ---- Identity W: the re-rank ------------------------------------------------------------------------------------------------------------------------------
RR_N, RR_NQ = 600, 4
RR_LISTS = [1, 255, 256, 257, 600]


def _rerank_layouts(d):
    """(name, pitch in elements, offset in elements): the 16-byte road, the dword road, the 2-byte road; every pitch leaves at least one padding column"""
    even = d + 2 if d % 2 == 0 else d + 1
    if even % 8 == 0:
        even += 2
    odd = d + 1 if d % 2 == 0 else d + 2
    return [("vec16", (d + 8) // 8 * 8, 0), ("dword", even, 2), ("half", odd, 1)]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("d", [1, 2, 3, 7, 8, 9, 63, 64, 65, 127, 128, 129, 200])
def test_rerank_on_half_rows_equals_the_widened_index(lsq, engine, fmt, d):
    lib = lsq._lib.load()
    rng = np.random.default_rng(1000 * d + HC.FORMATS[fmt])
    X = HC.matrix(rng, RR_N, d)
    special = HC.special_rows(X, rng)
    Hh, W = _halves(X, fmt)
    assert np.isnan(W[special[0]]).all() and np.isinf(W[special[1]]).all() and (W[special[3]] != 0).all()      # subnormals survive the widening
    Xq = rng.standard_normal((RR_NQ, d)).astype(np.float32)
    cands = {}
    for Lc in RR_LISTS:
        for id_base in (0, 1):
            c = rng.integers(id_base, RR_N + id_base, (RR_NQ, Lc)).astype(np.int32)
            c[0, 0] = RR_N + id_base                                         # ids outside the base, at both ends
            c[-1, -1] = id_base - 1
            if Lc >= 255:
                c[1, :5] = special + id_base
            cands[(Lc, id_base)] = c
    # the f32 index over widen(H), NaN in its padding columns, held to the host checker
    Wp = np.full((RR_N, d + 1), np.float32(np.nan))
    Wp[:, :d] = W
    roads = set()
    with engine.index(None, None, None, 0, base=Wp, d=d) as wix:
        ref = {}
        for (Lc, id_base), c in cands.items():
            rc, rd, ri = rerank_cpu(lib, Wp, Xq, c, d, Lc, id_base)
            assert rc == 0
            got = wix.rerank(Xq, c, Lc, id_base=id_base)
            assert _same(got, (rd, ri)), ("f32", Lc, id_base)
            ref[(Lc, id_base)] = got
        wstats = wix.stats()
        for name, ldb, off in _rerank_layouts(d):
            view, keep = _view(Hh, ldb, off, _fill(fmt))                     # NaN halves between the rows: a component consumed past d poisons a distance
            addr = view.data_ptr() | (2 * ldb)
            roads.add(16 if addr % 16 == 0 else 4 if addr % 4 == 0 else 2)
            with engine.index_dev(None, None, None, 0, base=view, d=d) as hix:
                assert hix.base_info()["format"] == HC.FORMATS[fmt] and hix.base_info()["owned"] == 0
                for (Lc, id_base), c in cands.items():
                    assert _same(_call(hix, "rerank", Xq, c, Lc, id_base=id_base), ref[(Lc, id_base)]), (name, Lc, id_base)
                assert _same(_call(hix, "rerank", Xq, cands[(257, 1)], 1, id_base=1), (ref[(257, 1)][0][:, :1], ref[(257, 1)][1][:, :1]))      # k = 1 < L
                st = hix.stats()                                             # the same calls and one more, of 257 candidates with two outside the base
                assert (st["invalid"], st["rows"], st["batches"]) == (wstats["invalid"] + 2, wstats["rows"] + RR_NQ * 257 - 2, wstats["batches"] + 1)
        # a host index over the same halves (rows in the format, taken as they are, at an odd pitch)
        Hp = np.full((RR_N, d + 1 + d % 2), _fill(fmt), dtype=Hh.dtype)
        Hp[:, :d] = Hh
        with engine.index(None, None, None, 0, base=Hp[:, :d], base_format=fmt) as hix:
            for key in ((600, 0), (255, 1)):
                assert _same(hix.rerank(Xq, cands[key], key[0], id_base=key[1]), ref[key]), key
    assert roads == {16, 4, 2}


# ---- Identity W: exact k-NN -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("d", [1, 15, 16, 17, 40])
def test_knn_on_half_rows_equals_the_widened_index(lsq, engine, fmt, d):
    lib = lsq._lib.load()
    rng = np.random.default_rng(77 * d + HC.FORMATS[fmt])
    for n in (1, 63, 64, 65, 200):
        X = HC.matrix(rng, n, d, edges=n > 1)
        if n >= 63:
            HC.special_rows(X, rng)
            X[3] = np.float32(777.0) + rng.integers(0, 8, d).astype(np.float32)      # ties: duplicate rows (exact in both formats, unlike any other row), ordered by id
            X[10] = X[3]
            X[40] = X[3]
        Hh, W = _halves(X, fmt)
        ldb = d + 1 + (n % 2)                                                # odd and even pitches
        Hp = np.full((n, ldb), _fill(fmt), dtype=Hh.dtype)
        Hp[:, :d] = Hh
        Wp = np.full((n, ldb), np.float32(np.nan))
        Wp[:, :d] = W
        mask = rng.random(n) < 0.6
        mask[:min(n, 4)] = True
        with engine.index(None, None, None, 0, base=Hp[:, :d], base_format=fmt) as hix, engine.index(None, None, None, 0, base=Wp[:, :d]) as wix:
            for nq in (1, 127, 128, 129):
                Q = rng.standard_normal((nq, d)).astype(np.float32)
                if n >= 63:
                    Q[0] = W[3]                                              # distance 0 to the three duplicates
                for road in (None, "dense", "compact"):
                    for ix in (hix, wix):
                        if road is None:
                            ix.clear_filter()
                        else:
                            ix.set_filter(mask=mask, road=road)
                    live = n if road is None else int(mask.sum())
                    for k in sorted({1, min(10, n), n}):
                        got, want = hix.knn(Q, k), wix.knn(Q, k)
                        assert _same(got, want), (n, nq, road, k)
                        assert _counts(hix.knn_info()) == _counts(wix.knn_info()) and hix.filter_info()["road"] == wix.filter_info()["road"]
                        if n >= 63 and k >= 3 and road is None:
                            assert list(got[1][0, :3]) == [3, 10, 40] and np.all(got[0][0, :3] == 0)
                        if k > live:
                            assert np.all(got[1][:, live:] == -1)            # past the allowed rows: (+inf, id_base - 1)
            for ix in (hix, wix):                                            # the widened call is the host checker's (unfiltered road)
                ix.clear_filter()
            got = hix.knn(Q, n)
            dd, ii = np.zeros((129, n), np.float32), np.zeros((129, n), np.uint32)
            assert lib.lsq_knn_exact_u8_cpu(dd.ctypes.data, ii.ctypes.data, Wp.ctypes.data, 0, Q.ctypes.data, 0, n, 129, d, ldb, d, n, 0) == 0
            assert HC.same_bits(got[0], dd) and np.array_equal(got[1], ii.astype(np.int32))
            # uint8 queries against a half base: the same template, no road of its own
            Q8 = rng.integers(0, 256, (5, d), dtype=np.uint8)
            for road in (None, "dense", "compact"):
                for ix in (hix, wix):
                    ix.clear_filter() if road is None else ix.set_filter(mask=mask, road=road)
                k = min(10, n)
                assert _same(hix.knn(Q8, k), wix.knn(Q8, k)) and _same(hix.knn(Q8, k), wix.knn(Q8.astype(np.float32), k))
                assert hix.knn_info()["int_road"] == 0


@pytest.mark.parametrize("fmt", FMTS)
def test_knn_exact_dev_takes_half_tensors(lsq, engine, fmt):
    rng = np.random.default_rng(9)
    n, d, nq, k = 300, 24, 7, 10
    X = HC.matrix(rng, n, d)
    Hh, W = _halves(X, fmt)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    view, keep = _view(Hh, d + 3, 1, _fill(fmt))
    dd, di = engine.knn_exact_dev(view, _dev(Q), k)
    wd, wi = engine.knn_exact_dev(_dev(W), _dev(Q), k)
    assert HC.same_bits(dd.cpu().numpy(), wd.cpu().numpy()) and np.array_equal(di.cpu().numpy(), wi.cpu().numpy())
    with pytest.raises(TypeError):
        engine.index_dev(None, None, None, 0, base=view, base_format="bf16" if fmt == "f16" else "f16")      # the dtype decides: a contradiction is refused


# ---- Identity W: the two-stage calls ------------------------------------------------------------------------------------------------------------------------
def _database(rng, n, d, m):
    K = (rng.standard_normal((m * H, d)) / np.sqrt(m)).astype(np.float32)
    codes = rng.integers(0, H, (n, m)).astype(np.uint8)
    recon = sum(K[j * H + codes[:, j].astype(np.int64)] for j in range(m))
    dbn = (recon.astype(np.float64) ** 2).sum(1).astype(np.float32)
    Xb = (recon + 0.35 * rng.standard_normal((n, d))).astype(np.float32)
    return codes, K, dbn, Xb


def _make(engine, packed, dev, codes, K, dbn, nc, cb, m, base, fmt=None):
    """a plain or packed index, of host arrays or of device tensors, over `base` rows"""
    kw = {"base_format": fmt} if fmt and not dev else {}
    t = _dev if dev else (lambda a: a)
    if packed:
        return (engine.index_packed_dev if dev else engine.index_packed)(t(codes), t(K), t(nc), t(cb), m, base=t(base), **kw)
    return (engine.index_dev if dev else engine.index)(t(codes), t(K), t(dbn), m, base=t(base), **kw)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("fmt", FMTS)
def test_two_stage_calls_on_half_rows(lsq, engine, fmt, packed):
    rng = np.random.default_rng(31 + HC.FORMATS[fmt])
    n, m, d, nlist, nq, k, L = 2000, 4, 16, 8, 33, 10, 100
    codes, K, dbn, Xb = _database(rng, n, d, m)
    Hh, W = _halves(Xb, fmt)
    ncb = 16
    nc, cb = rng.integers(0, ncb, n, dtype=np.uint8), np.sort(rng.random(ncb).astype(np.float32) * 8 + 1)
    if packed:
        dbn = cb[nc]
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    assign = rng.integers(0, nlist, n).astype(np.int32)
    Q = (Xb[rng.integers(0, n, nq)] + 0.25 * rng.standard_normal((nq, d))).astype(np.float32)
    for dev in (False, True):
        with _make(engine, packed, dev, codes, K, dbn, nc, cb, m, Hh, fmt) as hix, _make(engine, packed, dev, codes, K, dbn, nc, cb, m, W) as wix:
            assert hix.base_info()["format"] == HC.FORMATS[fmt] and wix.base_info()["format"] == 0
            assert hix.base_info()["resident_bytes"] * 2 == wix.base_info()["resident_bytes"]
            for ix in (hix, wix):
                _call(ix, "set_lists", cent, assign)
            got, want = _call(hix, "search", Q, k, shortlist=L), _call(wix, "search", Q, k, shortlist=L)
            assert _same(got, want) and np.isfinite(got[0]).all()
            assert _same(_call(hix, "search", Q, k), _call(wix, "search", Q, k))      # no shortlist: the scan alone
            got, want = _call(hix, "search_ivf", Q, k, 3, shortlist=L), _call(wix, "search_ivf", Q, k, 3, shortlist=L)
            assert _same(got, want)
            assert _counts(hix.stats()) == _counts(wix.stats()) and _counts(hix.ivf_info()) == _counts(wix.ivf_info())
            # and the re-ranked distances are lsq_rerank_cpu's on the widened rows
            if not dev:
                sd, si = hix.search(Q, L)
                rc, rd, ri = rerank_cpu(lsq._lib.load(), W, Q, si, d, k, 1)
                assert rc == 0 and _same(hix.search(Q, k, shortlist=L), (rd, ri))


# ---- Identity W through the life cycle: add, remove, compact, add --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("fmt", FMTS)
def test_life_cycle_on_half_rows(lsq, engine, fmt, dev):
    rng = np.random.default_rng(50 + HC.FORMATS[fmt] + 10 * dev)
    n, m, d, nlist, nq, k, L = 700, 4, 12, 5, 9, 8, 40
    total = n + 90 + 60
    codes, K, dbn, Xb = _database(rng, total, d, m)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    assign = rng.integers(0, nlist, total).astype(np.int32)
    Q = (Xb[rng.integers(0, n, nq)] + 0.25 * rng.standard_normal((nq, d))).astype(np.float32)
    Hh, W = _halves(Xb, fmt)
    model = W[:n].copy()                                                     # the rows the index must hold, as float32

    def compare(hix, wix, what):
        assert hix.n == wix.n == model.shape[0], what
        assert HC.same_bits(_call(hix, "base_rows"), model) and HC.same_bits(_call(wix, "base_rows"), model), what
        assert _same(_call(hix, "search", Q, k, shortlist=L), _call(wix, "search", Q, k, shortlist=L)), what
        assert _same(_call(hix, "search_ivf", Q, k, 2, shortlist=L), _call(wix, "search_ivf", Q, k, 2, shortlist=L)), what
        assert _same(_call(hix, "knn", Q, k), _call(wix, "knn", Q, k)), what
        assert hix.base_info()["format"] == HC.FORMATS[fmt] and hix.base_info()["elem_bytes"] == 2 and wix.base_info()["format"] == 0, what

    if dev:                                                                  # a borrowed half tensor at an odd pitch, one element into its buffer
        hview, keep = _view(Hh[:n], d + 1, 1, _fill(fmt))
        hix = engine.index_dev(_dev(codes[:n]), _dev(K), _dev(dbn[:n]), m, base=hview)
        wix = engine.index_dev(_dev(codes[:n]), _dev(K), _dev(dbn[:n]), m, base=_dev(W[:n]))
    else:
        hix = engine.index(codes[:n], K, dbn[:n], m, base=Xb[:n], base_format=fmt)      # narrowed by the binding
        wix = engine.index(codes[:n], K, dbn[:n], m, base=W[:n])
    with hix, wix:
        mask = rng.random(n) < 0.7
        for ix in (hix, wix):
            _call(ix, "set_lists", cent, assign[:n])
            _call(ix, "set_filter", mask=mask)
        compare(hix, wix, "created")
        assert hix.base_info()["owned"] == (0 if dev else 1)
        # add 1: host rows -- float32, narrowed by the binding -- to either kind of index
        a, b = n, n + 90
        hix.add(codes=codes[a:b], dbnorms=dbn[a:b], base=Xb[a:b], assign=assign[a:b])
        wix.add(codes=codes[a:b], dbnorms=dbn[a:b], base=W[a:b], assign=assign[a:b])
        model = np.concatenate([model, W[a:b]])
        compare(hix, wix, "add f32 rows")
        assert hix.base_info()["owned"] == 1 and (not dev or hix.growth_info()["adopted"] == 1)      # the borrowed half tensor was adopted
        # remove
        gone = rng.choice(b, 120, replace=False).astype(np.int32)
        for ix in (hix, wix):
            ix.remove(gone)
        compare(hix, wix, "remove")
        # compact: the rows outside the filter leave
        old = _call(hix, "compact")
        assert np.array_equal(old, _call(wix, "compact"))
        model = model[old]
        compare(hix, wix, "compact")
        # add 2: rows already narrow (float16 rows / the uint16 bits), at a padded pitch
        a, b = n + 90, total
        narrow = np.full((b - a, d + 3), _fill(fmt), dtype=Hh.dtype)
        narrow[:, :d] = Hh[a:b]
        hix.add(codes=codes[a:b], dbnorms=dbn[a:b], base=narrow[:, :d], assign=assign[a:b])
        wix.add(codes=codes[a:b], dbnorms=dbn[a:b], base=W[a:b], assign=assign[a:b])
        model = np.concatenate([model, W[a:b]])
        compare(hix, wix, "add narrow rows")
        # reserve moves the rows again
        for ix in (hix, wix):
            ix.reserve(4 * total)
        compare(hix, wix, "reserve")
        if dev:                                                              # device rows must have the index's dtype
            with pytest.raises(TypeError):
                hix.add(codes=_dev(codes[:2]), dbnorms=_dev(dbn[:2]), base=_dev(W[:2]), assign=_dev(assign[:2]))
            hix.add(codes=_dev(codes[:2]), dbnorms=_dev(dbn[:2]), base=_dev(Hh[:2]), assign=_dev(assign[:2]))
            wix.add(codes=_dev(codes[:2]), dbnorms=_dev(dbn[:2]), base=_dev(W[:2]), assign=_dev(assign[:2]))
            model = np.concatenate([model, W[:2]])
            compare(hix, wix, "add device rows")
