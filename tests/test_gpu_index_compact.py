"""Removing rows from the resident index on the device (lsq_index_remove, lsq_index_compact).  At every step:

  Identity C  the compacted index answers every call -- search, search_ivf on both roads, rerank, knn, stage two -- and reports every deterministic
              statistic as a FRESH index over the surviving rows does, bit for bit (tests/index_compact_check.py over tests/index_add_check.py);
  Identity M  the filtered answer before the compact and the answer after it have the same distance bits, ids mapped by new_of_old.

The fresh index is itself held to the host checkers once per family (and the model behind both identities in tests/test_index_compact.py), so the
yardstick is not the code under test.  Identity R (remove = set_filter of the difference) and the refusals have tests of their own."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_check as FC  # noqa: E402
import index_add_check as IA  # noqa: E402
import index_compact_check as IC  # noqa: E402
import ivf_check as ic  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL = -1


def _step(ix, P, removed, dev_ids=False, shrink=False, **kw):
    """remove `removed` (0-based rows of the index as it is), compact, and assert both identities -> (the survivors' problem, old_of_new, new_of_old)"""
    n = ix.n
    old_of_new, new_of_old = IC.maps(n, removed)
    ids = np.ascontiguousarray(removed, dtype=np.int32)
    ix.remove(IA.t(ids) if dev_ids and ids.shape[0] else ids)
    assert ix.n == n
    before = IA.answers(ix, P, **kw)
    got = ix.compact(shrink=shrink)
    assert bool(getattr(got, "is_cuda", False)) == ix._dev and np.array_equal(IA.to_np(got), old_of_new)
    S = IC.sub(P, old_of_new)
    assert ix.n == S["n"] == ix.growth_info()["n"]
    after = IA.answers(ix, S, **kw)
    with IA.fresh(ix._eng, S, S["n"], codes=ix._has_codes, base=ix._has_base, lists=bool(getattr(ix, "nlist", 0))) as fx:
        assert IA.equal_answers(after, IA.answers(fx, S, **kw)) == [], "Identity C"
    assert IC.held_M(before, after, new_of_old) == [], "Identity M"
    f = ix.filter_info()
    assert (f["active"], f["n"], f["allowed"]) == (0, S["n"], 0)
    return S, old_of_new, new_of_old


# ---- 1. the gather's roads: rows of 1, 5, 8, 9, 16 and 17 bytes, 2065 rows (not a multiple of 32: the bitmap's last word is partial) ---------------------
FORMATS = {"m1": (1, False), "m5": (5, False), "m8": (8, False), "m16": (16, False), "packed-m7": (7, True), "packed-m8": (8, True), "packed-m16": (16, True)}
N1 = 2065


def _patterns(n):
    """name -> the rows removed.  Which road of compact_gather_kernel each forces is asserted below from the kernel's branch conditions (IC.gather_roads):
    alternate   no two survivors were neighbours: a 16-byte chunk that holds bytes of two rows is put together byte by byte -- every chunk for rows
                shorter than 16 bytes; 16-byte rows are one aligned load each
    runs23      survivors in runs of exactly 2 and 3 rows between single removed rows (period 7 against 16-byte chunks: the runs' edges fall at every
                offset of a chunk): chunks inside a run take a load, chunks across an edge the byte road
    head1/2/3   one long run behind 1, 2, 3 removed rows: every source is k * rowb bytes past its destination -- for odd rowb the funnel at shift
                k mod 4 = 1, 2, 3, for 8-byte rows whole dwords, for 16-byte rows the aligned load
    last        only the last row leaves: source = destination, aligned loads, a shorter stream
    keep-first / keep-last   n' = 1: one short chunk (one whole chunk for 16- and 17-byte rows)
    word        a whole bitmap word (rows 64 .. 95) leaves: its prefix entry repeats
    nothing     a filter that allows every row: the identity gather"""
    period = np.arange(n) % 7
    return {"alternate": np.arange(1, n, 2), "runs23": np.flatnonzero((period == 2) | (period == 6)), "head1": np.arange(1), "head2": np.arange(2),
            "head3": np.arange(3), "last": np.array([n - 1]), "keep-first": np.arange(1, n), "keep-last": np.arange(n - 1), "word": np.arange(64, 96),
            "nothing": np.zeros(0, dtype=np.int64)}


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_gather_roads(lsq, engine, fmt):
    m, packed = FORMATS[fmt]
    rowb = m + packed
    P = IA.problem(N1, m, 24, 11, 800 + rowb, packed=packed)
    seen = {}
    for k, (name, removed) in enumerate(_patterns(N1).items()):
        seen[name] = IC.gather_roads(IC.maps(N1, removed)[0], rowb)
        dev = bool(k % 2)
        with IA.fresh(engine, P, N1, dev=dev) as ix:                         # host and device indexes, host and device ids in turn
            if name == "nothing":
                FC.set_filter(ix, mask=np.ones(N1, dtype=bool))              # an active filter that drops nothing
            _step(ix, P, removed, dev_ids=bool((k // 2) % 2), nns=(1, 10))
            c = ix.compact_info()
            assert (c["n_before"], c["n_after"], c["compactions"], c["rows_dropped"]) == (N1, N1 - len(removed), 1, len(removed))
            assert c["moved_bytes"] == (N1 - len(removed)) * (rowb + (0 if packed else 4))
    # the roads, from the kernel's own conditions
    if rowb < 16:
        assert seen["alternate"] - {"tail"} == {"bytes"}
        assert "bytes" in seen["runs23"]
    if rowb == 16:
        assert seen["alternate"] | seen["head1"] | seen["runs23"] == {"aligned"}
    if rowb == 17:
        assert "bytes" in seen["alternate"] and "bytes" in seen["runs23"]
    if rowb % 2:
        assert {"funnel1"} <= seen["head1"] and {"funnel2"} <= seen["head2"] and {"funnel3"} <= seen["head3"]
        assert not (seen["head1"] | seen["head2"] | seen["head3"]) & {"bytes"}
    if rowb == 8:
        assert seen["head1"] - {"tail"} == {"dwords"} and seen["head2"] - {"tail"} == {"aligned"}
    assert seen["last"] - {"tail"} == {"aligned"} and seen["nothing"] - {"tail"} == {"aligned"}
    assert seen["keep-first"] == seen["keep-last"] == ({"tail"} if rowb < 16 else {"aligned"} if rowb == 16 else {"aligned", "tail"})
    if fmt == "m8":                                                          # the yardstick against the untouched host scan
        full = FC.full_scan(lsq._lib.load(), P["codes"], P["K"], P["dbn"], P["Q"])
        with IA.fresh(engine, P, N1) as fx:
            assert IA.same(fx.search(P["Q"], 100), (full[0][:, :100], full[1][:, :100]))


# ---- 2. base rows: f32 d = 24 at pitch 24 and 25 (100 bytes: rows never 16-byte aligned twice running), uint8 d = 37 at pitch 37 and 40; a base-only index
BASES = {"f32-24": ("f32", 24, 24), "f32-25": ("f32", 24, 25), "u8-37": ("u8", 37, 37), "u8-40": ("u8", 37, 40)}


@pytest.mark.parametrize("case", list(BASES))
def test_base_rows(lsq, engine, case):
    import torch
    kind, d, pitch = BASES[case]
    n = 1033
    P = IA.problem(n, 4, d, 7, 77 + pitch, base=kind)
    rng = np.random.default_rng(pitch)
    patterns = {"alternate": np.arange(1, n, 2), "head1": np.arange(1), "third": rng.permutation(n)[: n // 3], "keep-last": np.arange(n - 1)}
    for name, removed in patterns.items():
        wide = torch.zeros((n, pitch), dtype=torch.uint8 if kind == "u8" else torch.float32, device="cuda")
        wide[:, :d] = IA.t(P["base"])
        image = wide.clone()
        with engine.index_dev(None, None, None, 0, base=wide[:, :d], d=d) as ix:      # a borrowing index at this pitch
            old_of_new, new_of_old = IC.maps(n, removed)
            # rerank ignores the filter: the same candidates before and after, renumbered; ids outside the base on both sides
            keep = old_of_new[rng.integers(0, old_of_new.shape[0], (7, 12))].astype(np.int32)
            keep[:, ::5] = n + 2
            after_cand = np.where(keep >= n, old_of_new.shape[0] + 2, new_of_old[np.minimum(keep, n - 1)]).astype(np.int32)
            k = min(5, old_of_new.shape[0])
            rb = IA.call(ix, "rerank", P["Q"], cand=keep, k=k, id_base=0)
            S, _, _ = _step(ix, P, removed, dev_ids=True, nns=(k,), knn=True)
            ra = IA.call(ix, "rerank", P["Q"], cand=after_cand, k=k, id_base=0)
            assert np.array_equal(IA.bits(rb[0]), IA.bits(ra[0])) and np.array_equal(IC.map_ids(rb[1], new_of_old, 0), ra[1]), (case, name)
            assert ix.growth_info()["adopted"] == 1
            assert torch.equal(wide, image)                                  # the caller's rows were never written
    if case == "f32-24":                                                     # the yardstick: the fresh index against the host exact search
        with IA.fresh(engine, P, n, codes=False) as fx:
            fd, fi = FC.full_knn(lsq._lib.load(), P["base"], P["Q"])
            assert IA.same(fx.knn(P["Q"], 5), (fd[:, :5], fi[:, :5].astype(np.int32)))


# ---- 3. inverted lists -----------------------------------------------------------------------------------------------------------------------------------
def _lists_problem(nlist, packed):
    """3000 skewed rows (ivf_check.skewed_lists: list 0 half of the rows, lists 1 and 2 empty, lists 3 and 4 one row each) with five rows on the last list"""
    P = IA.problem(3000, 7 if packed else 8, 16, 37, 600 + nlist + packed, nlist=nlist, packed=packed)
    rng = np.random.default_rng(nlist)
    P["lor"][:] = ic.skewed_lists(rng, 3000, nlist)
    if nlist >= 7:
        P["lor"][rng.permutation(3000)[:5]] = nlist - 1
    return P


def _list_removals(nlist):
    """the removals, applied one after another to the index as it then is: lor -> the rows removed"""
    first_of_each = lambda lor: np.array([np.flatnonzero(lor == l)[0] for l in np.unique(lor)])      # noqa: E731
    out = [("one-from-each", first_of_each), ("half-of-the-giant", lambda lor: np.flatnonzero(lor == 0)[::2])]
    if nlist > 1:
        out += [("last-list", lambda lor: np.flatnonzero(lor == nlist - 1)), ("list-0", lambda lor: np.flatnonzero(lor == 0)),
                ("all-but-one-list", lambda lor: np.flatnonzero(lor != np.bincount(lor[lor != 0]).argmax()))]
    return out


@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
@pytest.mark.parametrize("nlist", [1, 7, 300])
def test_inverted_lists(lsq, engine, nlist, packed):
    P = _lists_problem(nlist, packed)
    nprobes = sorted({1, min(3, nlist), nlist})
    if nlist == 7 and not packed:                                            # the yardstick against the host checker
        rc, hd, hi = ic.ivf_cpu(lsq._lib.load(), P["codes"], P["K"], P["dbn"], P["cent"], P["lor"], P["Q"], P["Qc"], 3, 10)
        with IA.fresh(engine, P, 3000) as fx:
            assert rc == 0 and IA.same(fx.search_ivf(P["Q"], 10, 3, Q_coarse=P["Qc"]), (hd, hi))
    with IA.fresh(engine, P, 3000, dev=packed) as ix:
        for k, (name, rows_of) in enumerate(_list_removals(nlist)):
            removed = rows_of(P["lor"])
            if len(removed) == 0:                                            # (seven lists: by now a single list holds every row)
                continue
            assert len(removed) < ix.n, name
            P, _, _ = _step(ix, P, removed, dev_ids=bool(k % 2), nns=(10,) if ix.n - len(removed) >= 10 else (1,), nprobes=nprobes)
            if name == "list-0":
                assert not (P["lor"] == 0).any()
            # every list probed: the scan's own result
            nn = min(10, ix.n)
            assert IA.same(IA.call(ix, "search_ivf", P["Q"], nn, nlist, Q_coarse=P["Qc"]), IA.call(ix, "search", P["Q"], nn))
            if nlist == 7 and k < 2:
                assert IC.held_C(ix, P, nns=(10,), nprobes=(3,), flags=ic.TEST_BATCH) == []
        # the lists replaced after the compactions
        P2 = dict(P, lor=P["lor"][::-1].copy(), cent=P["cent"][::-1].copy())
        conv = IA.t if ix._dev else (lambda a: a)
        ix.set_lists(conv(P2["cent"]), conv(P2["lor"]))
        assert IC.held_C(ix, P2, nns=(min(10, ix.n),), nprobes=nprobes) == []


# ---- 4. crossing 65 536 rows downwards: the selection returns to the every-distance road exactly as a fresh index of that size is on it -------------------
def test_crossing_the_small_n_limit_downwards(lsq, engine):
    P = IA.problem(70000, 8, 16, 5, 43)
    removed = np.random.default_rng(4).permutation(70000)[:10000]
    with IA.fresh(engine, P, 70000) as ix:
        ix.search(P["Q"], 50)
        assert ix.scan_stats()["exhaustive"] == 0
        S, _, _ = _step(ix, P, removed, nns=(50,))
        ix.search(S["Q"], 50)
        assert ix.n == 60000 and ix.scan_stats()["exhaustive"] == 1
        full = FC.full_scan(lsq._lib.load(), S["codes"], S["K"], S["dbn"], S["Q"])
        assert IA.same(ix.search(S["Q"], 50), (full[0][:, :50], full[1][:, :50]))


# ---- 5. the lifecycle --------------------------------------------------------------------------------------------------------------------------------------
def _prefix(P, n):
    return dict({k: v for k, v in P.items()}, n=n, **{k: P[k][:n] for k in IC.PER_ROW if k in P})


def _concat(S, P, lo, hi):
    return dict(S, n=S["n"] + hi - lo, **{k: np.concatenate([S[k], P[k][lo:hi]]) for k in IC.PER_ROW if k in S})


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_remove_compact_add_remove_compact(lsq, engine, dev):
    P = IA.problem(2300, 8, 16, 9, 55, nlist=7, base="f32")
    rng = np.random.default_rng(6)
    kw = dict(nns=(10,), nprobes=(1, 3, 7), shortlist=40, knn=True)
    with IA.fresh(engine, P, 2000, dev=dev) as ix:
        S, _, _ = _step(ix, _prefix(P, 2000), rng.permutation(2000)[:400], dev_ids=not dev, **kw)
        g = ix.growth_info()
        assert (g["n"], g["capacity_rows"], g["adopted"]) == (1600, 2000, int(dev))      # the capacity is kept; a borrowing index was adopted by the gather
        IA.grow(ix, P, 2000, 2300, dev=dev)                                  # into the freed rows: nothing is re-allocated
        S = _concat(S, P, 2000, 2300)
        assert ix.n == 1900 and ix.growth_info()["reallocations"] == g["reallocations"] and ix.growth_info()["capacity_rows"] == 2000
        assert IC.held_C(ix, S, **kw) == [], "Identity G on the compacted index"
        S, _, _ = _step(ix, S, rng.permutation(1900)[:700], dev_ids=dev, shrink=True, **kw)
        assert ix.growth_info()["capacity_rows"] == 1200 == ix.n
        c = ix.compact_info()
        assert (c["removes"], c["rows_tombstoned"], c["compactions"], c["rows_dropped"], c["shrunk"]) == (2, 1100, 2, 1100, 1)
        assert (c["n_before"], c["n_after"]) == (1900, 1200)
        # without a filter nothing leaves, the map is the identity and SHRINK still acts on reserved capacity
        ix.reserve(3000)
        assert ix.growth_info()["capacity_rows"] == 3000
        assert np.array_equal(IA.to_np(ix.compact()), np.arange(1200)) and ix.growth_info()["capacity_rows"] == 3000
        assert np.array_equal(IA.to_np(ix.compact(shrink=True)), np.arange(1200)) and ix.growth_info()["capacity_rows"] == 1200
        assert ix.compact_info()["rows_dropped"] == 1100 and ix.compact_info()["compactions"] == 4
        assert IC.held_C(ix, S, **kw) == []


def test_a_borrowing_index_leaves_the_callers_tensors_alone(lsq, engine):
    import torch
    P = IA.problem(2065, 8, 16, 9, 57, nlist=7, base="f32")
    tens = {k: IA.t(P[k]) for k in ("codes", "K", "dbn", "base", "cent", "lor")}
    image = {k: v.clone() for k, v in tens.items()}
    with engine.index_dev(tens["codes"], tens["K"], tens["dbn"], 8, base=tens["base"]) as ix:
        ix.set_lists(tens["cent"], tens["lor"])
        assert ix.growth_info()["adopted"] == 0
        _step(ix, P, np.arange(0, 2065, 3), dev_ids=True, nns=(10,), nprobes=(3,), knn=True)
        assert ix.growth_info()["adopted"] == 1
        torch.cuda.synchronize()
        assert all(torch.equal(tens[k], image[k]) for k in tens)


# ---- 6. Identity R: remove in instalments = one set_filter of the difference ----------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["no-filter", "mask", "force-compact"])
def test_remove_equals_set_filter_of_the_difference(lsq, engine, start):
    n = 2065
    P = IA.problem(n, 8, 16, 9, 61, nlist=7, base="f32")
    rng = np.random.default_rng(8)
    allowed = np.ones(n, dtype=bool) if start == "no-filter" else rng.random(n) < 0.6
    road = "compact" if start == "force-compact" else None
    parts = [rng.permutation(n)[:300], np.concatenate([rng.permutation(n)[:200]] * 2), np.array([n - 1, 0, 0, 64])]      # duplicates inside a call
    parts[2] = np.concatenate([parts[2], parts[0][:50], np.flatnonzero(~allowed)[:5]])      # rows removed before, rows the mask had excluded already
    kw = dict(nns=(10,), nprobes=(1, 7), knn=True)
    for dev in (False, True):
        with IA.fresh(engine, P, n, dev=dev) as ix, IA.fresh(engine, P, n, dev=dev) as want:
            if start != "no-filter":
                FC.set_filter(ix, road=road, mask=allowed)
            ix.remove(np.zeros(0, np.int32))                                 # a no-op: it creates no filter
            assert ix.filter_info()["active"] == int(start != "no-filter")
            left, cleared = allowed.copy(), 0
            for k, part in enumerate(parts):
                ids = (part + k % 2).astype(np.int32)                        # id_base 0, 1, 0
                ix.remove(IA.t(ids) if (k + dev) % 2 else ids, id_base=k % 2)
                cleared += int(left[np.unique(part)].sum())                  # the bits this call newly clears
                left[part] = False
                FC.set_filter(want, road=road, bits=FC.to_bits(left))
                assert IA.equal_answers(IA.answers(ix, P, **kw), IA.answers(want, P, **kw)) == [], (start, dev, k)
                got, exp = ix.filter_info(), want.filter_info()
                assert {f: v for f, v in got.items() if f != "road"} == {f: v for f, v in exp.items() if f != "road"}
            if start == "force-compact":                                     # the force is kept: the scan walks the row list
                IA.call(ix, "search", P["Q"], 10)
                assert ix.filter_info()["road"] == 2
            c = ix.compact_info()
            assert (c["removes"], c["rows_tombstoned"]) == (3, cleared) and cleared == int(allowed.sum()) - int(left.sum())


# ---- 7. refusals change nothing --------------------------------------------------------------------------------------------------------------------------
def _snapshot(ix, P):
    a = IA.answers(ix, P, nns=(10,), nprobes=(1, 7), knn=True)
    return a, ix.growth_info(), ix.filter_info(), ix.compact_info(), ix.ivf_info(), ix.n


def _unchanged(a, b):
    return IA.equal_answers(a[0], b[0]) == [] and a[1:] == b[1:]


@pytest.mark.parametrize("filtered", [False, True], ids=["no-filter", "filter"])
def test_refusals_change_nothing(lsq, engine, filtered):
    n = 2065
    P = IA.problem(n, 8, 16, 9, 63, nlist=7, base="f32")
    L = lsq._lib.load()
    ok = np.array([5, 6, 7], dtype=np.int32)
    with IA.fresh(engine, P, n) as ix:
        if filtered:
            ix.remove(np.arange(100, 400, dtype=np.int32))
        snap = _snapshot(ix, P)

        def remove(ids, count, id_base):
            return L.lsq_index_remove(ix._h, None if ids is None else ids.ctypes.data, count, id_base, 0)

        def compact(**fields):
            desc = lsq._lib.IndexCompactDesc()
            for f, v in fields.items():
                setattr(desc, f, v)
            return L.lsq_index_compact(ix._h, C.byref(desc))

        refused = [("id_base - 1", lambda: remove(np.array([5, -1, 6], dtype=np.int32), 3, 0)),
                   ("id_base - 1, 1-based", lambda: remove(np.array([5, 0, 6], dtype=np.int32), 3, 1)),
                   ("id_base + n", lambda: remove(np.array([5, n, 6], dtype=np.int32), 3, 0)),
                   ("id_base + n, 1-based", lambda: remove(np.array([5, n + 1, 6], dtype=np.int32), 3, 1)),
                   ("id_base = 2", lambda: remove(ok, 3, 2)), ("count < 0", lambda: remove(ok, -1, 0)), ("null ids", lambda: remove(None, 3, 0)),
                   ("unknown flag", lambda: compact(flags=2)), ("bad id_base", lambda: compact(id_base=2))]
        for name, call in refused:
            assert call() == EINVAL and L.lsq_last_error(), name
            assert _unchanged(_snapshot(ix, P), snap), name
        # no allowed row: an index holds at least one
        FC.set_filter(ix, mask=np.zeros(n, dtype=bool))
        snap = _snapshot(ix, P)
        assert compact() == EINVAL and b"allowed" in L.lsq_last_error()
        assert L.lsq_index_compact(ix._h, None) == EINVAL
        assert _unchanged(_snapshot(ix, P), snap)
