"""Decode on the device (lsq_index_reconstruct) and search by stored row (lsq_index_search_rows).  Every decode is held to the
contract of tests/recon_check.py (decode: from +0.0, codebooks ascending, every add rounded) AND to lsq_reconstruct_cpu, under same_bits: bit identity,
any NaN where the contract's value is a NaN.  Every case runs on a host-buffer index and on a device-tensor index; the output lies inside a buffer of
sentinels, which the rows' gaps and the zones around them must keep.  search_rows is held to the identity it states: search(reconstruct(rows))."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_add_check as IA  # noqa: E402
import index_compact_check as IC  # noqa: E402
import recon_check as RC  # noqa: E402

pytestmark = pytest.mark.gpu
H = 256
SENTINEL = 0xDEADBEEF                                                        # as a float: a finite negative number, never a decode's NaN pad
GUARD = 64                                                                   # floats of sentinel before and after the rows


# ---- the pieces ----------------------------------------------------------------------------------------------------------------------------------------
def _index(engine, codes, K, m, dev, packed, dbn=None):
    """an index over codes [n][m]: plain (rows of m bytes) or packed (rows of m + 1 bytes); host arrays or device tensors"""
    n = codes.shape[0]
    conv = IA.t if dev else np.ascontiguousarray
    if packed:
        make = engine.index_packed_dev if dev else engine.index_packed
        return make(conv(codes), conv(K), conv(np.zeros(n, np.uint8)), conv(np.ones(1, np.float32)), m)
    make = engine.index_dev if dev else engine.index
    return make(conv(codes), conv(K), conv(np.zeros(n, np.float32) if dbn is None else dbn), m)


class Guarded:
    """`count` output rows of d floats, ldo apart, inside a buffer of sentinels that starts `shift` floats past a 16-byte boundary -- a numpy array or a
    device tensor.  rows(): what Index.reconstruct is given; check(): the rows as numpy, after asserting that nothing else was written"""

    def __init__(self, count, d, ldo, shift, dev):
        self.count, self.d, self.ldo, self.dev = count, d, ldo, dev
        self.lo = GUARD + shift
        total = self.lo + count * ldo + GUARD
        if dev:
            import torch
            self.flat = torch.full((total,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda").view(torch.float32)
            assert self.flat.data_ptr() % 16 == 0
        else:
            raw = np.full(total + 4, SENTINEL, dtype=np.uint32).view(np.float32)
            self.flat = raw[(-(raw.ctypes.data // 4)) % 4:][:total]
            assert self.flat.ctypes.data % 16 == 0

    def rows(self):
        body = self.flat[self.lo:self.lo + self.count * self.ldo]
        return (body.view(self.count, self.ldo) if self.dev else body.reshape(self.count, self.ldo))[:, :self.d]

    def check(self):
        flat = IA.to_np(self.flat).view(np.uint32)
        body = flat[self.lo:self.lo + self.count * self.ldo].reshape(self.count, self.ldo)
        assert np.all(flat[:self.lo] == SENTINEL) and np.all(flat[self.lo + self.count * self.ldo:] == SENTINEL), "a guard zone was written"
        assert np.all(body[:, self.d:] == SENTINEL), "the gap between two rows was written"
        return np.ascontiguousarray(body[:, :self.d]).view(np.float32)

    def untouched(self):
        return bool(np.all(IA.to_np(self.flat).view(np.uint32) == SENTINEL))


LAYOUTS = {"tight": (0, 0), "pitch+1": (1, 0), "shift4": (0, 1)}              # name -> (ldo - d, floats past the 16-byte boundary)


def _recon(ix, layout="tight", **kw):
    """Index.reconstruct into a guarded buffer -> the rows as numpy (guards checked)"""
    ids = kw.get("ids")
    count = len(ids) if ids is not None else kw.get("count", ix.n - kw.get("start", 0))
    extra, shift = LAYOUTS[layout]
    g = Guarded(count, ix.d, ix.d + extra, shift, ix._dev)
    if ids is not None:
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        kw["ids"] = IA.t(ids) if ix._dev else ids
    got = ix.reconstruct(out=g.rows(), **kw)
    assert got.shape == (count, ix.d)
    return g.check()


# ---- 1. loader edges -----------------------------------------------------------------------------------------------------------------------------------
DS = [1, 3, 4, 5, 16, 64, 127, 128, 129, 132, 260, 960]
MS = [1, 2, 7, 8, 15, 16]
NS = [1, 63, 64, 65, 1000, 9000]


@pytest.mark.parametrize("d", DS)
def test_loader_edges(lsq, engine, d):
    """per d every m; n, the row format (plain / packed: ldc = m, m + 1 -- whole dwords at m = 8, 16 and packed 7, 15, bytes otherwise) and the output
    layout rotate so that over the twelve d every m meets every n, both formats and every layout.  d: the dword road (1, 3, 5, 127, 129), the 16-byte road
    with a lane group below a wave (4, 16, 64), of one wave (128 .. 256) and looping over it (260: a second trip for one lane group; 960), and tails"""
    lib, B = lsq._lib.load(), lsq._lib
    di = DS.index(d)
    for i, m in enumerate(MS):
        n, packed, layout = NS[(i + di) % 6], bool((i + di // 6) % 2), list(LAYOUTS)[(i + di) % 3]
        if d == 960 and n == 9000:
            n = 2500                                                         # (still several grid strides: one row per wave-step, 2048 blocks of 4)
        rng = np.random.default_rng(100 * d + m)
        K = (rng.standard_normal((m * H, d)) / np.sqrt(m)).astype(np.float32)
        codes = rng.integers(0, H, (n, m)).astype(np.uint8)
        want = RC.decode(codes, K, m)
        rc, cpu = RC.reconstruct_cpu(lib, codes, K, m)
        assert rc == 0 and RC.same_bits(cpu, want)
        for dev in (False, True):
            with _index(engine, codes, K, m, dev, packed) as ix:
                got = _recon(ix, layout)
                assert RC.same_bits(got, want), (d, m, n, packed, layout, dev)
                info = ix.recon_info()
                vec = d % 4 == 0 and layout == "tight"                       # a device call decodes in place; a host call into its own tight staging
                if dev:
                    assert info["road"] & 3 == (B.RECON_ROAD_VEC16 if vec else B.RECON_ROAD_DWORD), (d, layout, info)
                else:
                    assert info["road"] & 3 == (B.RECON_ROAD_VEC16 if d % 4 == 0 else B.RECON_ROAD_DWORD), (d, info)
                assert bool(info["road"] & B.RECON_ROAD_CODE_DWORDS) == ((m + packed) % 4 == 0) and info["rows"] == n and info["invalid"] == 0
                if n > 6:                                                    # a range inside: the first and the last rows stay out
                    assert RC.same_bits(_recon(ix, layout, start=3, count=n - 5), want[3:n - 2])


# ---- 2. the id form ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m,packed", [(20, 8, False), (5, 7, True)])
def test_id_form(lsq, engine, d, m, packed):
    lib, n = lsq._lib.load(), 3000
    rng = np.random.default_rng(d)
    K = (rng.standard_normal((m * H, d)) / np.sqrt(m)).astype(np.float32)
    codes = rng.integers(0, H, (n, m)).astype(np.uint8)
    patterns = {"ascending": lambda c: np.arange(c) % n, "descending": lambda c: (n - 1 - np.arange(c)) % n, "equal": lambda c: np.full(c, n - 1),
                "random": lambda c: rng.integers(0, n, c)}
    for dev in (False, True):
        with _index(engine, codes, K, m, dev, packed) as ix:
            for k, count in enumerate([0, 1, 64, 65, 5000]):
                for j, (name, make) in enumerate(patterns.items()):
                    ids, base, layout = make(count), (k + j) % 2, list(LAYOUTS)[(k + j) % 3]
                    if name == "random" and count > n:
                        assert len(np.unique(ids)) < count                   # repeats
                    want = RC.decode_ids(codes, K, m, ids)
                    got = _recon(ix, layout, ids=ids + base, id_base=base)
                    assert RC.same_bits(got, want), (name, count, base, dev)
                    rc, cpu = RC.reconstruct_cpu(lib, codes, K, m, ids=ids + base, id_base=base)
                    assert rc == 0 and RC.same_bits(cpu, want)
                    if count:
                        assert ix.recon_info()["rows"] == count
            # bad ids at either end
            for base in (0, 1):
                ids = rng.integers(0, n, 200) + base
                bad_at = [0, 77, 199, 13]
                ids[bad_at] = [base - 1, base + n, -2 ** 31, 2 ** 31 - 1]
                assert ids.min() < base and ids.max() >= base + n            # non-vacuity: invalid ids at both ends
                g = Guarded(200, d, d + 1, 0, dev)
                arg = IA.t(ids.astype(np.int32)) if dev else ids.astype(np.int32)
                with pytest.raises(lsq._lib.LsqError):
                    ix.reconstruct(ids=arg, id_base=base, out=g.rows())
                assert g.untouched()                                         # refused before anything was written
                got = _recon(ix, "pitch+1", ids=ids, id_base=base, pad_nan=True)
                want = RC.decode_ids(codes, K, m, ids, id_base=base, pad_nan=True)
                assert RC.same_bits(got, want) and np.all(got.view(np.uint32)[bad_at] == RC.NAN_BITS)
                assert not np.isnan(got[np.setdiff1d(np.arange(200), bad_at)]).any()
                info = ix.recon_info()
                assert info["invalid"] == 4 and info["rows"] == 196
                rc, cpu = RC.reconstruct_cpu(lib, codes, K, m, ids=ids, id_base=base, flags=lsq._lib.RECON_PAD_NAN)
                assert rc == 0 and RC.same_bits(cpu, want)


def test_refusals_launch_nothing(lsq, engine):
    rng = np.random.default_rng(1)
    K, codes = rng.standard_normal((2 * H, 8)).astype(np.float32), rng.integers(0, H, (50, 2)).astype(np.uint8)
    for dev in (False, True):
        with _index(engine, codes, K, 2, dev, False) as ix, (engine.index_dev if dev else engine.index)(None, None, None, 0, base=(IA.t if dev else np.asarray)(
                rng.standard_normal((50, 8)).astype(np.float32))) as bare:
            calls_before = ix.recon_info()["calls"]
            for kw in (dict(count=-1), dict(start=49, count=2), dict(start=51, count=0), dict(start=-1, count=1), dict(id_base=2), dict(add_coarse=True)):
                g = Guarded(max(kw.get("count", 50), 0), 8, 8, 0, dev)
                with pytest.raises(lsq._lib.LsqError):
                    ix.reconstruct(out=g.rows(), **kw)
                assert g.untouched(), kw
            side, p = ix._side, ix._side.ptr
            g = Guarded(50, 8, 8, 0, dev)
            for args in ((p(g.rows()), 7, None, 0, 50, 0, 0), (p(g.rows()), 8, None, 0, 50, 0, 4), (None, 8, None, 0, 50, 0, 0)):      # ldo < d; a flag; null out
                with pytest.raises(lsq._lib.LsqError):
                    engine._call(side, "lsq_index_reconstruct", *args, int(dev), h=ix._h)
            with pytest.raises(lsq._lib.LsqError):
                engine._call(side, "lsq_index_reconstruct", p(g.rows()), 8, None, 0, 50, 0, 0, int(dev), h=bare._h)      # an index without codes
            assert g.untouched() and ix.recon_info()["calls"] == calls_before
            assert ix.reconstruct(count=0).shape == (0, 8)                   # count == 0: LSQ_OK


# ---- 3. special values and the order of the sum ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m", [(4, 8), (7, 2), (8, 1), (129, 16)])
def test_special_values(lsq, engine, d, m):
    rng = np.random.default_rng(7 * d + m)
    K = RC.special_codebooks(rng, m, d)
    codes = rng.integers(0, H, (300, m)).astype(np.uint8)
    want = RC.decode(codes, K, m)
    # non-vacuity, on the host arrays: +0.0 where starting from the first codeword gives -0.0; NaNs from inf - inf and from the table; denormals
    assert np.all(RC.bits(want[:, 0]) == 0x00000000) and np.all(RC.bits(K[codes[:, 0].astype(np.int64), 0]) == 0x80000000)
    if m > 1:
        assert np.isnan(want[:, 1]).all()
    assert d < 3 or np.isnan(want[:, 2]).any()
    if m == 1 and d > 3:
        assert np.all((RC.bits(want[:, 3]) >> 23) == 0) and np.all(RC.bits(want[:, 3]) != 0)      # a denormal survives the add of +0.0
    for dev in (False, True):
        for packed in (False, True):
            with _index(engine, codes, K, m, dev, packed) as ix:
                assert RC.same_bits(_recon(ix, "shift4"), want)
                got = _recon(ix, ids=np.arange(299, -1, -1))
                assert RC.same_bits(got, want[::-1]) and np.all(RC.bits(got[:, 0]) == 0)


@pytest.mark.parametrize("d,m", [(16, 8), (5, 16), (128, 7)])
def test_order_and_width_sensitivity(lsq, engine, d, m):
    codes, K = RC.order_sensitive(500, m, d, seed=d + m)                     # asserts, on the host, that another order or a wider sum shows
    want = RC.decode(codes, K, m)
    for dev in (False, True):
        with _index(engine, codes, K, m, dev, False) as ix:
            assert RC.same_bits(_recon(ix), want)


# ---- 4. the coarse add -----------------------------------------------------------------------------------------------------------------------------------
def _coarse_problem(n, m, d, nlist, seed, packed=False):
    P = IA.problem(n, m, d, 70, seed, nlist=nlist, packed=packed)
    lor = P["lor"].copy()
    if nlist >= 7:
        lor[np.flatnonzero(lor != 0)[:5]] = 0                                # list 0: MORE than half of the rows
        counts = np.bincount(lor, minlength=nlist)
        assert (counts == 0).any() and (counts == 1).any() and counts.max() > n // 2 + 1      # non-vacuity: empty, one-row and over-half lists
    P["lor"] = lor
    return P


@pytest.mark.parametrize("nlist", [1, 7, 300])
def test_coarse_add(lsq, engine, nlist):
    lib, n, m, d = lsq._lib.load(), 2000, 8, 24
    P = _coarse_problem(n, m, d, nlist, 40 + nlist)
    codes, K, cent, lor = P["codes"], P["K"], P["cent"], P["lor"]
    plain = RC.decode(codes, K, m)
    want = RC.add_coarse(plain, cent, lor)
    assert (RC.bits(want) != RC.bits(plain)).any()
    rc, cpu = RC.reconstruct_cpu(lib, codes, K, m, cent=cent, lor=lor, flags=lsq._lib.RECON_ADD_COARSE)
    assert rc == 0 and RC.same_bits(cpu, want)
    ids = np.random.default_rng(nlist).integers(0, n, 333)
    for dev in (False, True):
        with IA.fresh(engine, P, n, dev=dev, lists=False) as ix:
            with pytest.raises(lsq._lib.LsqError):                         # refused without lists
                ix.reconstruct(add_coarse=True)
            conv = IA.t if dev else np.ascontiguousarray
            ix.set_lists(conv(cent), conv(lor))
            assert RC.same_bits(_recon(ix, "pitch+1", add_coarse=True), want) and ix.recon_info()["map_rebuilt"] == 1
            assert RC.same_bits(_recon(ix, ids=ids, add_coarse=True), want[ids]) and ix.recon_info()["map_rebuilt"] == 0      # the map is kept
            assert RC.same_bits(_recon(ix), plain) and ix.recon_info()["map_rebuilt"] == 0
            # other lists: the map follows
            lor2, cent2 = ((lor.astype(np.int64) * 5 + np.arange(n)) % nlist).astype(np.int32), cent[::-1].copy()
            ix.set_lists(conv(cent2), conv(lor2))
            assert RC.same_bits(_recon(ix, add_coarse=True), RC.add_coarse(plain, cent2, lor2)) and ix.recon_info()["map_rebuilt"] == 1
            assert ix.recon_info()["map_rebuilds"] == 2
            # add: 150 rows more; compact after a removal: the map is rebuilt each time
            rng = np.random.default_rng(5)
            more, more_lor = rng.integers(0, H, (150, m)).astype(np.uint8), rng.integers(0, nlist, 150).astype(np.int32)
            ix.add(codes=conv(more), dbnorms=conv(np.zeros(150, np.float32)), assign=conv(more_lor))
            all_codes, all_lor = np.concatenate([codes, more]), np.concatenate([lor2, more_lor])
            full = RC.add_coarse(RC.decode(all_codes, K, m), cent2, all_lor)
            assert RC.same_bits(_recon(ix, add_coarse=True), full) and ix.recon_info()["map_rebuilt"] == 1
            gone = np.arange(0, n + 150, 3)
            ix.remove(gone.astype(np.int32) if not dev else IA.t(gone.astype(np.int32)))
            assert RC.same_bits(_recon(ix, add_coarse=True), full) and ix.recon_info()["map_rebuilt"] == 0      # tombstones: every row still addressable
            keep = IA.to_np(ix.compact()).astype(np.int64)
            assert RC.same_bits(_recon(ix, add_coarse=True), full[keep]) and ix.recon_info()["map_rebuilt"] == 1


# ---- 5. the index identities -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
def test_index_identities(lsq, engine, packed):
    """after add -> remove -> compact -> add an index reconstructs as a FRESH index over the same rows; a filter, tombstones, a held range result and the
    searches around a reconstruct are undisturbed"""
    m, d, nlist = 8, 24, 7
    P = _coarse_problem(1200, m, d, nlist, 77, packed=packed)
    for dev in (False, True):
        with IA.fresh(engine, P, 700, dev=dev) as ix:
            IA.grow(ix, P, 700, 1000, dev=dev)
            gone = np.arange(5, 1000, 4).astype(np.int32)
            ix.remove(IA.t(gone) if dev else gone)
            before = IA.call(ix, "search", P["Q"], 10)
            lims, rd, ri = ix.range_search((IA.t if dev else np.asarray)(P["Q"][:9]), 40.0)
            total = int(ix.range_info()["results"])
            assert total > 0
            tomb = _recon(ix, add_coarse=True)                               # tombstoned rows decode as before: the filter changes nothing
            assert RC.same_bits(tomb, RC.add_coarse(RC.decode(P["codes"][:1000], P["K"], m), P["cent"], P["lor"][:1000]))
            assert IA.same(IA.call(ix, "search", P["Q"], 10), before)        # a search before and after a reconstruct: the same bits
            side = ix._side
            d2, i2 = side.new((total,), np.float32, rd), side.new((total,), np.int32, rd)
            engine._call(side, "lsq_index_range_fetch", side.ptr(d2), side.ptr(i2), total, int(dev), h=ix._h)      # the held result is still there
            assert IA.same((d2, i2), (rd, ri))
            keep = IA.to_np(ix.compact())
            S = IC.sub({k: (v[:1000] if k in IC.PER_ROW else v) for k, v in P.items()}, keep)
            IA.grow(ix, {**P, **{k: np.concatenate([S[k], P[k][1000:]]) for k in IC.PER_ROW if k in P}}, S["n"], S["n"] + 200, dev=dev)
            F = {**P, **{k: np.concatenate([S[k], P[k][1000:]]) for k in IC.PER_ROW if k in P}}
            F["n"] = S["n"] + 200
            assert ix.n == F["n"]
            ids = np.random.default_rng(3).integers(0, F["n"], 400)
            with IA.fresh(engine, F, F["n"], dev=dev) as fx:
                for kw in (dict(), dict(add_coarse=True), dict(ids=ids), dict(ids=ids + 1, id_base=1, add_coarse=True), dict(start=F["n"] - 7, count=7)):
                    a, b = _recon(ix, **kw), _recon(fx, **kw)
                    assert RC.same_bits(a, b), kw
                want = RC.add_coarse(RC.decode(F["codes"], F["K"], m), F["cent"], F["lor"])
                assert RC.same_bits(_recon(fx, add_coarse=True), want)      # the yardstick itself against the contract
            # under a filter (both roads) the decode is the same
            mask = np.arange(F["n"]) % 3 == 0
            for road in ("dense", "compact"):
                ix.set_filter(mask=IA.t(mask) if dev else mask, road=road)
                assert RC.same_bits(_recon(ix, add_coarse=True), want)
            ix.clear_filter()


# ---- 6. search by stored row -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
def test_search_rows_is_search_of_reconstruct(lsq, engine, packed):
    m, d, nlist, n = 8, 24, 7, 2000
    P = _coarse_problem(n, m, d, nlist, 90 + packed, packed=packed)
    rows = np.random.default_rng(2).integers(0, n, 70).astype(np.int32)      # 70 rows as queries, some repeated
    rows[:2] = [0, n - 1]
    for dev in (False, True):
        conv = IA.t if dev else np.ascontiguousarray
        with IA.fresh(engine, P, n, dev=dev) as ix:
            for filt in (None, "dense", "compact"):
                if filt:
                    mask = np.arange(n) % 5 != 1
                    ix.set_filter(mask=conv(mask), road=filt)
                q_plain, q_coarse = ix.reconstruct(ids=conv(rows)), ix.reconstruct(ids=conv(rows), add_coarse=True)
                for base in (0, 1):
                    got = ix.search_rows(conv(rows + base), 10, id_base=base)
                    stats = ix.scan_stats()
                    want = ix.search(q_plain, 10)
                    assert IA.same(got, want) and IA.pick(stats, IA.STATS_SCAN) == IA.pick(ix.scan_stats(), IA.STATS_SCAN), (filt, base)
                for nprobe in (1, 4, nlist):
                    for add in (False, True):
                        got = ix.search_rows(conv(rows), 10, nprobe=nprobe, add_coarse=add)
                        stats = ix.ivf_info()
                        q = q_coarse if add else q_plain
                        want = ix.search_ivf(q, 10, nprobe, add_coarse=add)
                        assert IA.same(got, want) and IA.pick(stats, IA.STATS_IVF) == IA.pick(ix.ivf_info(), IA.STATS_IVF), (filt, nprobe, add)
                if not filt:                                                 # no self-exclusion: the row itself is a candidate like any other
                    d0, i0 = (IA.to_np(a) for a in ix.search_rows(conv(rows), n))
                    assert all(rows[q] + 1 in i0[q] for q in range(70))
            ix.clear_filter()
            # refusals leave dists / ids untouched
            side, p = ix._side, ix._side.ptr
            dd, ii = side.new((70, 10), np.float32, "cuda" if dev else None), side.new((70, 10), np.int32, "cuda" if dev else None)
            dd[...] = 7.0
            ii[...] = -5
            bad_rows = rows.copy()
            bad_rows[33] = n
            for args in ((conv(bad_rows), 70, 0, 10, 0, 0), (conv(rows), 70, 0, 10, nlist + 1, 0), (conv(rows), 70, 0, n + 1, 0, 0), (conv(rows), 70, 2, 10, 0, 0),
                         (conv(rows), 70, 0, 10, 0, 1), (conv(rows), 70, 0, 10, 2, 64), (conv(rows), 70, 0, 0, 0, 0)):
                with pytest.raises(lsq._lib.LsqError):
                    engine._call(side, "lsq_index_search_rows", p(dd), p(ii), p(args[0]), *args[1:], int(dev), h=ix._h)
                assert np.all(IA.to_np(dd) == 7.0) and np.all(IA.to_np(ii) == -5), args[1:]
        with IA.fresh(engine, P, n, dev=dev, lists=False) as ix:             # nprobe >= 1 before set_lists
            with pytest.raises(lsq._lib.LsqError):
                ix.search_rows(conv(rows), 10, nprobe=1)
            assert IA.same(ix.search_rows(conv(rows), 10), ix.search(ix.reconstruct(ids=conv(rows)), 10))


# ---- 7. a host-buffer call in several staging chunks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m,packed", [(24, 8, False), (5, 7, True)])
def test_host_call_in_several_chunks(lsq, engine, d, m, packed):
    """option "recon_chunk" cuts a host-buffer call into chunks whose size does not divide the count: the later chunks start inside the ids / the range
    and reuse the index's staging; the range form, the id form with the NaN pad, the coarse add, an output with a pitch.  The same bits for every value"""
    n, nlist = 1000, 7
    P = _coarse_problem(n, m, d, nlist, 300 + d, packed=packed)
    codes, K, cent, lor = P["codes"], P["K"], P["cent"], P["lor"]
    plain = RC.decode(codes, K, m)
    rng = np.random.default_rng(d)
    ids = rng.integers(0, n, 517)
    ids[[0, 300, 516]] = [-1, n, n + 5]                                      # invalid ids in the first, a middle and the last chunk
    want_ids = RC.decode_ids(codes, K, m, ids, pad_nan=True, cent=cent, lor=lor)
    try:
        with IA.fresh(engine, P, n, dev=False) as ix:
            for chunk in (0, 37, 1000, 999, 64, 1):
                engine.set_option("recon_chunk", chunk)
                assert RC.same_bits(_recon(ix, "pitch+1"), plain), chunk
                assert RC.same_bits(_recon(ix, "shift4", start=3, count=n - 5, add_coarse=True), RC.add_coarse(plain, cent, lor)[3:n - 2]), chunk
                if chunk != 1:
                    assert RC.same_bits(_recon(ix, "pitch+1", ids=ids + 1, id_base=1, pad_nan=True, add_coarse=True), want_ids), chunk
                    assert ix.recon_info()["invalid"] == 3 and ix.recon_info()["rows"] == 514
                bad = Guarded(517, d, d, 0, False)
                with pytest.raises(lsq._lib.LsqError):                       # an id in the LAST chunk refuses the whole call: no earlier chunk was written
                    ix.reconstruct(ids=np.where(np.arange(517) == 516, n, np.clip(ids, 0, n - 1)).astype(np.int32), out=bad.rows())
                assert bad.untouched(), chunk
    finally:
        engine.set_option("recon_chunk", 0)
