"""Helpers of tests/test_index_compact.py and tests/test_gpu_index_compact.py: the sub-problem over the rows that survive a removal, the two maps in
numpy, and the two yardsticks of lsq_index_compact --

  Identity C  held_C: the compacted index answers every call as a FRESH index over the surviving rows does, bit for bit (tests/index_add_check.py:
              fresh / answers / equal_answers, unchanged);
  Identity M  held_M: the filtered answer before the call and the answer after it have the same distance bits, and id_after = new_of_old[id_before]
              (padding records stay padding).

A problem is index_add_check's dict of numpy arrays over all rows."""
import numpy as np

import index_add_check as IA

PER_ROW = ("codes", "dbn", "nc", "base", "lor")


def maps(n, removed):
    """rows `removed` (any iterable of 0-based ids, duplicates legal) leave an index of n rows -> old_of_new (n',), new_of_old (n,) with -1, int32 0-based"""
    keep = np.ones(n, dtype=bool)
    keep[np.asarray(list(removed), dtype=np.int64)] = False
    old_of_new = np.flatnonzero(keep).astype(np.int32)
    new_of_old = np.full(n, -1, dtype=np.int32)
    new_of_old[old_of_new] = np.arange(old_of_new.shape[0], dtype=np.int32)
    return old_of_new, new_of_old


def sub(P, old_of_new):
    """the problem over the survivors, in their order: every per-row array gathered, everything else shared"""
    Q = dict(P)
    for k in PER_ROW:
        if k in P:
            Q[k] = np.ascontiguousarray(P[k][old_of_new])
    Q["n"] = int(old_of_new.shape[0])
    return Q


def gather_roads(sel, rowb):
    """the roads compact_gather_kernel takes over a stream of len(sel) rows of rowb bytes (csrc/lsq_compact.hip; source and destination arrays start at
    16-byte boundaries), by its own branch conditions: per 16-byte destination chunk "aligned" (a run of survivors, source 16-byte aligned: one dwordx4
    load), "dwords" (a run, source 4-byte aligned), "funnel1" .. "funnel3" (a run, source at byte 1 .. 3 of a dword: the alignbyte funnel at that shift),
    "bytes" (the chunk straddles survivors that were not neighbours), "tail" (the stream's last, short chunk)"""
    sel = np.asarray(sel, dtype=np.int64)
    total, roads = sel.shape[0] * rowb, set()
    for D in range(0, total, 16):
        ln = min(16, total - D)
        p, pe = D // rowb, (D + ln - 1) // rowb
        if ln < 16:
            roads.add("tail")
        elif sel[pe] - sel[p] != pe - p:
            roads.add("bytes")
        else:
            a = sel[p] * rowb + D - p * rowb
            roads.add("aligned" if a % 16 == 0 else "dwords" if a % 4 == 0 else "funnel%d" % (a % 4))
    return roads


def held_C(ix, Ps, **kw):
    """Identity C at the index's current size: the labels at which it differs from the fresh index over the survivors' problem Ps (lists included, no
    filter)"""
    assert ix.n == Ps["n"]
    with IA.fresh(ix._eng, Ps, ix.n, dev=False, codes=ix._has_codes, base=ix._has_base, lists=bool(getattr(ix, "nlist", 0))) as fx:
        return IA.equal_answers(IA.answers(ix, Ps, **kw), IA.answers(fx, Ps, **kw))


def map_ids(ids, new_of_old, id_base):
    """ids in id_base through the map; a padding record (id_base - 1) stays one"""
    ids = np.asarray(ids).astype(np.int64) - id_base
    out = np.where(ids < 0, -1, new_of_old[np.clip(ids, 0, new_of_old.shape[0] - 1)]).astype(np.int64)
    assert not np.any((ids >= 0) & (out < 0)), "an answer names a removed row"
    return (out + id_base).astype(np.int32)


ID_BASE = {"search": 1, "search-shortlist": 1, "ivf": 1, "knn-f32": 0, "knn-u8": 0}      # the id base of each call of IA.answers that a filter restricts


def held_M(before, after, new_of_old):
    """-> the labels of two IA.answers() (before: under the filter; after: compacted) at which Identity M fails.  rerank ignores the filter and its
    candidates are ids, so it is compared by the tests that map the candidates; statistics are not compared here (the roads differ)"""
    bad = []
    for k, ((bd, bi), _) in before.items():
        name = k[0] if isinstance(k, tuple) else k
        if name not in ID_BASE or k not in after:                             # (a search for more than n' neighbours: outside Identity M)
            continue
        (ad, ai), _ = after[k]
        if not (np.array_equal(IA.bits(bd), IA.bits(ad)) and np.array_equal(map_ids(bi, new_of_old, ID_BASE[name]), np.asarray(ai))):
            bad.append(k)
    return bad
