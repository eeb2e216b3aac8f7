"""The contract of a row filter on the resident index (lsq_index_set_filter), stated in numpy: the checker of tests/test_filter.py and
tests/test_gpu_filter.py.

    While a filter is set, search / search_ivf / knn return, per query, the result the same call would return for nn = (all candidate rows), with every
    row outside the allowed set removed, truncated to nn and padded with (+inf, id_base - 1).

filtered() is that sentence: a stable removal from a full ranking, then padding.  The full rankings come from the checkers the project already has, called
with nn = the number of candidate rows: the untouched host scan (search), lsq_ivf_search_cpu (search_ivf), lsq_knn_exact_u8_cpu (knn), lsq_rerank_cpu on
the filtered stage-one ids (shortlist).  Everything is compared bit for bit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivf_check as ic  # noqa: E402
from knn_check import same_bits  # noqa: E402
from packed_check import host_scan  # noqa: E402
from rerank_check import rerank_cpu  # noqa: E402

BITS, BYTES, IDS = 0, 1, 2
DENY, FORCE_DENSE, FORCE_COMPACT = 1, 2, 4


def filtered(full_d, full_ids, allowed, nn, pad_id):
    """full_d, full_ids (nq, N): a full ranking, ids in the id base pad_id + 1 (an entry with id pad_id is the ranking's own padding and is dropped);
    allowed (n,) bool by 0-based row -> the first nn entries of every row whose id is allowed, in the ranking's order, then (+inf, pad_id)"""
    full_d = np.asarray(full_d, dtype=np.float32)
    full_ids = np.asarray(full_ids).astype(np.int64)
    allowed = np.asarray(allowed, dtype=bool)
    nq = full_d.shape[0]
    out_d = np.full((nq, nn), np.float32(np.inf), dtype=np.float32)
    out_i = np.full((nq, nn), pad_id, dtype=np.int32)
    for q in range(nq):
        row = full_ids[q] - (pad_id + 1)
        keep = np.flatnonzero((row >= 0) & allowed[np.clip(row, 0, allowed.shape[0] - 1)])[:nn]
        out_d[q, :keep.shape[0]] = full_d[q, keep]
        out_i[q, :keep.shape[0]] = full_ids[q, keep]
    return out_d, out_i


def same(got, want):
    """(dists, ids) pairs equal bit for bit"""
    return same_bits(np.asarray(got[0]), want[0]) and np.array_equal(np.asarray(got[1]).astype(np.int64), np.asarray(want[1]).astype(np.int64))


# ---- the full rankings ----------------------------------------------------------------------------------------------------------------------------
def full_scan(lib, codes, K, dbn, Q):
    """the host scan's ranking of every row: ids 1-based"""
    return host_scan(lib, codes, K, dbn, Q, codes.shape[0])


def full_ivf(lib, p, nprobe, flags=0):
    """lsq_ivf_search_cpu with nn = n: every probed row in order, then its own (+inf, 0) padding; ids 1-based"""
    rc, d, i = ic.ivf_cpu(lib, *p, nprobe, p[0].shape[0], flags=flags)
    assert rc == 0
    return d, i


def full_knn(lib, base, Q):
    """lsq_knn_exact_u8_cpu with nn = n on f32 or uint8 rows / queries: ids 0-based"""
    base = np.ascontiguousarray(base)
    Q = np.ascontiguousarray(Q)
    (n, d), nq = base.shape, Q.shape[0]
    dists, ids = np.zeros((nq, n), dtype=np.float32), np.zeros((nq, n), dtype=np.uint32)
    rc = lib.lsq_knn_exact_u8_cpu(dists.ctypes.data, ids.ctypes.data, base.ctypes.data, int(base.dtype == np.uint8), Q.ctypes.data,
                                  int(Q.dtype == np.uint8), n, nq, d, d, d, n, 0)
    assert rc == 0
    return dists, ids.astype(np.int64)


def two_stage(lib, stage1_ids, base, Q_exact, nn):
    """stage two on the filtered stage-one ids (1-based; the padding id 0 lies outside the base and stays last)"""
    rc, d, i = rerank_cpu(lib, base, Q_exact, stage1_ids, Q_exact.shape[1], nn, 1)
    assert rc == 0
    return d, i


# ---- filters over n rows ----------------------------------------------------------------------------------------------------------------------------
def masks(n, seed=5):
    """name -> allowed (n,) bool: the cases of the issue, at any n >= 64"""
    rng = np.random.default_rng(seed)
    out = {"all": np.ones(n, dtype=bool), "none": np.zeros(n, dtype=bool)}
    one = np.zeros(n, dtype=bool)
    one[n // 3] = True
    out["one"] = one
    out["even"] = np.arange(n) % 2 == 0
    out["word0"] = np.arange(n) < 32
    out["last-word"] = np.arange(n) >= (n - 1) // 32 * 32                   # the partial last word where n % 32 != 0
    for name, frac in (("half", 2), ("tenth", 10), ("hundredth", 100)):
        out[name] = rng.random(n) < 1.0 / frac
    seven = np.zeros(n, dtype=bool)
    seven[rng.permutation(n)[:7]] = True
    out["seven"] = seven
    return out


def to_bits(allowed, garbage_tail=False):
    """the uint32 words of a mask; garbage_tail: the bits at and past n set (they must be ignored)"""
    n = allowed.shape[0]
    padded = np.zeros((n + 31) // 32 * 32, dtype=bool)
    padded[:n] = allowed
    if garbage_tail:
        padded[n:] = True
    return np.packbits(padded.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1).copy()


def forms(allowed, seed=9):
    """the same set four ways -> [(label, set_filter keyword arguments)]: the mask, the bits (with garbage past n), the ids 1-based in random order with
    duplicates, and the complement's ids 0-based as a DENY list"""
    rng = np.random.default_rng(seed)
    rows = np.flatnonzero(allowed).astype(np.int32)
    dup = np.concatenate([rows, rows[: (rows.shape[0] + 1) // 2]])
    dup = dup[rng.permutation(dup.shape[0])] + 1
    return [("mask", dict(mask=allowed.copy())), ("bits", dict(bits=to_bits(allowed, garbage_tail=True))),
            ("ids", dict(ids=dup.astype(np.int32), id_base=1)), ("deny", dict(ids=np.flatnonzero(~allowed).astype(np.int32), deny=True, id_base=0))]


def set_filter(ix, road=None, **kw):
    """Index.set_filter with numpy arguments on either kind of index (a device index gets torch tensors; torch has no uint32 arithmetic: the words go
    as int32, the same bits)"""
    if ix._dev:
        import torch
        for k in ("mask", "bits", "ids"):
            if k in kw:
                a = kw[k]
                kw[k] = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    ix.set_filter(road=road, **kw)


def lists_without_allowed(lor, allowed, nlist):
    return int(nlist - np.unique(np.asarray(lor)[np.asarray(allowed, dtype=bool)]).shape[0])
