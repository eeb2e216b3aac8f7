"""Helpers of tests/test_packed.py and tests/test_gpu_packed.py: the packed index (rows of m code bytes and one norm byte, lsq_index_create_packed) is
held to ONE identity -- every call returns the bits of the same call on a plain index with dbnorms[i] = cbnorms[c_i] -- so what is needed here is only
the inputs: norm tables with their bytes, the untouched host scan as the outside reference, and the raw C call for the refusals.  numpy only."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 256
# what a scan reports about its selection: only these can see a sample that read other rows (the fallback road repairs the results)
STAT_KEYS = ("exhaustive", "threshold_rank", "list_capacity", "candidates", "fallback_queries", "batches")
IVF_KEYS = ("queries", "probed_rows", "records", "threshold_queries", "fallback_queries", "batches", "batch_queries", "tail_capacity")


def header():
    with open(os.path.join(ROOT, "include", "lsq_mi355x.h")) as f:
        return f.read()


def header_struct_fields(name):
    """the field names of `typedef struct name { ... } name;` in the header, in order"""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        for piece in decl.split(","):
            ids = re.findall(r"[A-Za-z_]\w*", piece)
            if ids:
                fields.append(ids[-1])
    return fields


def table(rng, ncb, special=False):
    """cbnorms (ncb,) f32: positive norms in random order; special: NaN, +inf, -inf and -0.0 among them (as many as fit)"""
    cb = (rng.random(ncb) * 8 + 0.5).astype(np.float32)
    if special:
        for at, v in zip(rng.permutation(ncb)[:4], (np.nan, np.inf, -0.0, -np.inf)):
            cb[at] = np.float32(v)
    return cb


def problem(rng, n, m, d, nq, ncb=256, special=False, zero_K=False):
    """codes (n,m), K (m*256,d), norm bytes (n,) that use every entry of the table where n allows (the last one at row n - 1), cbnorms (ncb,), Q (nq,d)"""
    K = np.zeros((m * H, d), dtype=np.float32) if zero_K else (rng.standard_normal((m * H, d)) / np.sqrt(m)).astype(np.float32)
    codes = rng.integers(0, H, (n, m)).astype(np.uint8)
    nc = rng.integers(0, ncb, n).astype(np.uint8)
    k = min(n, ncb)
    nc[:k] = np.arange(ncb - k, ncb)                                          # the table's last entry is always in use
    nc[n - 1] = ncb - 1
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    return codes, K, nc, table(rng, ncb, special), Q


def quantize(dbn, ncb=256):
    """a float norm per row -> (cbnorms, norm bytes) with at most ncb entries: NaN, +inf and -inf keep entries of their own, the finite values are kept
    exactly when few enough and snapped to the nearest of evenly ranked ones otherwise.  cbnorms[bytes] is then the problem's dbnorms: equal rows stay equal"""
    dbn = np.asarray(dbn, dtype=np.float32)
    cb, nc = [], np.zeros(dbn.shape[0], dtype=np.int64)
    for pick in (np.isnan(dbn), np.isposinf(dbn), np.isneginf(dbn)):
        if pick.any():
            nc[pick] = len(cb)
            cb.append(dbn[pick][0])
    fin = np.isfinite(dbn)
    vals = np.unique(dbn[fin])
    room = ncb - len(cb)
    if len(vals) > room:
        vals = vals[np.linspace(0, len(vals) - 1, room).round().astype(np.int64)]
    if fin.any():
        at = np.clip(np.searchsorted(vals, dbn[fin]), 1, max(len(vals) - 1, 1)) if len(vals) > 1 else np.zeros(int(fin.sum()), dtype=np.int64)
        if len(vals) > 1:
            at = np.where(np.abs(dbn[fin] - vals[at - 1]) <= np.abs(vals[at] - dbn[fin]), at - 1, at)
        nc[fin] = len(cb) + at
        cb.extend(vals.tolist())
    cb = np.asarray(cb, dtype=np.float32)
    return cb, nc.astype(np.uint8)


def host_scan(lib, codes, K, dbn, Q, nn, nthreads=0):
    """lsq_linscan_aqd_query_extra_byte, the untouched host scan -> dists (nq,nn) f32, ids (nq,nn) int32 1-based"""
    codes, K = np.ascontiguousarray(codes, dtype=np.uint8), np.ascontiguousarray(K, dtype=np.float32)
    dbn, Q = np.ascontiguousarray(dbn, dtype=np.float32), np.ascontiguousarray(Q, dtype=np.float32)
    (n, m), (nq, d) = codes.shape, Q.shape
    dists, ids = np.zeros((nq, nn), dtype=np.float32), np.zeros((nq, nn), dtype=np.int32)
    rc = lib.lsq_linscan_aqd_query_extra_byte(dists.ctypes.data, ids.ctypes.data, codes.ctypes.data, Q.ctypes.data, K.ctypes.data, dbn.ctypes.data, nq, n, m,
                                              K.shape[0] // m, d, nn, nthreads)
    assert rc == 0
    return dists, ids


def raw_create(lsq, engine, codes, norm_codes, cbnorms, K, on_device):
    """lsq_index_create_packed itself -> (return code, the handle's value: None while it is NULL).  codes .. K: numpy arrays (on_device = 0) or torch
    device tensors; a handle that was made is destroyed here"""
    ptr = (lambda t: t.data_ptr()) if on_device else (lambda a: a.ctypes.data)
    desc = lsq._lib.IndexPackedDesc()
    n, m = codes.shape
    desc.n, desc.d, desc.m, desc.h = n, K.shape[1], m, H
    desc.codes, desc.norm_codes, desc.cbnorms, desc.ncb, desc.codebooks = ptr(codes), ptr(norm_codes), ptr(cbnorms), cbnorms.shape[0], ptr(K)
    desc.base, desc.base_u8, desc.ldb, desc.on_device = None, 0, 0, int(on_device)
    handle = C.c_void_p()
    rc = engine._L.lsq_index_create_packed(C.byref(handle), engine._h, C.byref(desc))
    value = handle.value
    if value:
        engine._L.lsq_index_destroy(handle)
    return rc, value
