"""The contract of range search (lsq_index_range_search, lsq_range_search_cpu), stated in numpy: the checker of tests/test_range.py and
tests/test_gpu_range.py.

    The result of query q is the longest prefix with dist <= r_q of the full ranking the existing call returns for nn = (all candidate rows), with that
    ranking's own (+inf, pad) padding dropped.

range_of() is that sentence.  The full rankings come from the checkers the project already has -- filter_check.full_scan (the untouched host scan),
filter_check.full_ivf (lsq_ivf_search_cpu) and, under a filter, filter_check.filtered over either -- never from the code under test.  Everything is compared
bit for bit: lims, distances, ids."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from knn_check import same_bits  # noqa: E402

RADII = ("-inf", "+inf", "nan", "min", "10th", "half", "mid-10-11", "below-min")


def range_of(full_d, full_ids, radius, pad_id):
    """full_d, full_ids (nq, N): a full ranking (an entry with id pad_id is the ranking's own padding and is dropped); radius (nq,) or a scalar
    -> lims (nq + 1,) int64, dists (lims[-1],) f32, ids (lims[-1],) int32: per query the longest prefix with dist <= radius (IEEE: a NaN on either side
    ends it)"""
    full_d = np.asarray(full_d, dtype=np.float32)
    full_ids = np.asarray(full_ids).astype(np.int64)
    nq = full_d.shape[0]
    radius = np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,))
    lims = np.zeros(nq + 1, dtype=np.int64)
    parts_d, parts_i = [], []
    for q in range(nq):
        real = full_ids[q] != pad_id
        d, i = full_d[q][real], full_ids[q][real]
        with np.errstate(invalid="ignore"):
            inside = d <= radius[q]
        stop = int(np.argmin(inside)) if not inside.all() else inside.shape[0]      # the first entry outside the radius
        parts_d.append(d[:stop])
        parts_i.append(i[:stop])
        lims[q + 1] = lims[q] + stop
    dists = np.concatenate(parts_d).astype(np.float32) if parts_d else np.zeros(0, np.float32)
    ids = np.concatenate(parts_i).astype(np.int32) if parts_i else np.zeros(0, np.int32)
    return lims, dists, ids


def radii(full_d):
    """full_d (nq, N): a host ranking, ascending per query -> {name: (nq,) f32}, one radius per query and case, every case of RADII: -inf and +inf, NaN, the
    query's smallest distance exactly, its 10th and its ceil(N / 2)-th distance exactly (a tie group is then cut at one of its members), the midpoint
    between its 10th and 11th, and the float just below its smallest.  Positions past the row's end are clipped to it"""
    full_d = np.asarray(full_d, dtype=np.float32)
    nq, N = full_d.shape
    at = lambda k: full_d[:, min(max(k, 1), N) - 1].copy()      # noqa: E731  the k-th distance, 1-based
    with np.errstate(invalid="ignore", over="ignore"):
        mid = ((at(10).astype(np.float64) + at(11).astype(np.float64)) / 2).astype(np.float32)
        below = np.nextafter(at(1), np.float32(-np.inf)).astype(np.float32)
    out = {"-inf": np.full(nq, -np.inf, np.float32), "+inf": np.full(nq, np.inf, np.float32), "nan": np.full(nq, np.nan, np.float32),
           "min": at(1), "10th": at(10), "half": at(-(-N // 2)), "mid-10-11": mid, "below-min": below}
    assert tuple(out) == RADII
    return out


def same(got, want):
    """(lims, dists, ids) triples equal bit for bit"""
    gl, gd, gi = (np.asarray(a) for a in got)
    wl, wd, wi = want
    return (gl.dtype == np.int64 and np.array_equal(gl, wl) and gd.shape == wd.shape and same_bits(np.asarray(gd, dtype=np.float32), wd)
            and np.array_equal(gi.astype(np.int64), wi.astype(np.int64)))


def tie_cut_at_last_member(full_d, full_ids, radius, pad_id):
    """queries whose radius equals a distance that at least two candidate rows share: the result then ends exactly at the tie group's last member"""
    full_d = np.asarray(full_d, dtype=np.float32)
    radius = np.broadcast_to(np.asarray(radius, dtype=np.float32), (full_d.shape[0],))
    real = np.asarray(full_ids) != pad_id
    return int(sum(int(((full_d[q] == radius[q]) & real[q]).sum() >= 2) for q in range(full_d.shape[0])))


def range_cpu(lib, codes, K, dbn, Q, radius, cent=None, lor=None, nprobe=0, flags=0, Qc=None, allowed=None, capacity=None, nthreads=0, poison=None):
    """lsq_range_search_cpu on row arrays -> (rc, lims, dists, ids).  capacity None: the two-call protocol (count, then arrays of exactly that size);
    else one call with arrays of max(capacity, 0) entries pre-filled with `poison`"""
    codes, K, dbn = np.ascontiguousarray(codes, dtype=np.uint8), np.ascontiguousarray(K, dtype=np.float32), np.ascontiguousarray(dbn, dtype=np.float32)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    (n, m), (nq, d) = codes.shape, Q.shape
    radius = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,)))
    cent = None if cent is None else np.ascontiguousarray(cent, dtype=np.float32)
    lor = None if lor is None else np.ascontiguousarray(lor, dtype=np.int32)
    Qc = None if Qc is None else np.ascontiguousarray(Qc, dtype=np.float32)
    mask = None if allowed is None else np.ascontiguousarray(np.asarray(allowed, dtype=bool)).view(np.uint8)
    ptr = lambda a: None if a is None else a.ctypes.data      # noqa: E731
    lims = np.full(nq + 1, -7, dtype=np.int64)

    def call(dists, ids, cap):
        return lib.lsq_range_search_cpu(lims.ctypes.data, ptr(dists), ptr(ids), cap, codes.ctypes.data, K.ctypes.data, dbn.ctypes.data, ptr(cent), ptr(lor),
                                        0 if cent is None else cent.shape[0], nprobe, flags, ptr(mask), Q.ctypes.data, ptr(Qc), radius.ctypes.data,
                                        n, m, K.shape[0] // m, d, nq, d, nthreads)

    if capacity is None:
        rc = call(None, None, 0)
        if rc != 0:
            return rc, lims, None, None
        capacity = int(lims[-1])
    dists = np.full(max(capacity, 0), np.float32(0 if poison is None else poison), dtype=np.float32)
    ids = np.full(max(capacity, 0), 0 if poison is None else int(poison), dtype=np.int32)
    rc = call(dists, ids, capacity)
    return rc, lims, dists, ids
