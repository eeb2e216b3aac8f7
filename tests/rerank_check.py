"""numpy restatement of the exact re-rank (lsq_rerank_cpu, lsq_index_rerank): the checker of tests/test_rerank.py and tests/test_gpu_rerank.py.

    dist   = knn_check.knn_dists' rule (f32, s ascending, every op rounded) between a query and each of ITS candidates
    result = the nn smallest (dist, id) pairs among the query's L candidates, lexicographic, NaN after every number; a duplicated id comes twice; an id
             outside [id_base, id_base + n) comes after everything, NaN included, as (+inf, id_base - 1)"""
import numpy as np

from knn_check import knn_dists, order_keys


def rerank_np(Xb, Xq, cand, nn, id_base):
    """Xb (n, >= d) f32 or uint8, Xq (nq, d), cand (nq, L) int -> dists (nq, nn) f32, ids (nq, nn) int32"""
    n = Xb.shape[0]
    D = knn_dists(np.asarray(Xb, dtype=np.float32), Xq)                     # (nq, n): uint8 -> f32 is exact
    r = np.asarray(cand, dtype=np.int64) - id_base
    ok = (r >= 0) & (r < n)
    dist = np.where(ok, np.take_along_axis(D, np.clip(r, 0, n - 1), axis=1), np.float32(np.inf)).astype(np.float32)
    hi = order_keys(dist).astype(np.uint64) | ((~ok).astype(np.uint64) << np.uint64(32))
    field = np.where(ok, r + 1, 0)
    order = np.stack([np.lexsort((field[q], hi[q])) for q in range(r.shape[0])])[:, :nn]
    out_d = np.take_along_axis(dist, order, axis=1)
    out_d[np.isnan(out_d)] = np.float32(np.nan)                             # the library hands out one NaN (0x7fc00000) whatever the payload
    out_i = (np.take_along_axis(field, order, axis=1) - 1 + id_base).astype(np.int32)
    return out_d, out_i


def rerank_cpu(lib, Xb, Xq, cand, d, nn, id_base, nthreads=0):
    """lsq_rerank_cpu on row arrays Xb (n, ldb) f32 / uint8, Xq (nq, ldq), cand (nq, L), reading d components of each row -> (rc, dists, ids)"""
    u8 = Xb.dtype == np.uint8
    Xb = np.ascontiguousarray(Xb, dtype=np.uint8 if u8 else np.float32)
    Xq = np.ascontiguousarray(Xq, dtype=np.float32)
    cand = np.ascontiguousarray(cand, dtype=np.int32)
    nq, L = cand.shape
    dists = np.zeros((nq, nn), dtype=np.float32)
    ids = np.zeros((nq, nn), dtype=np.int32)
    rc = lib.lsq_rerank_cpu(dists.ctypes.data, ids.ctypes.data, Xb.ctypes.data, int(u8), Xq.ctypes.data, cand.ctypes.data, Xb.shape[0], nq, d,
                            Xb.shape[1], Xq.shape[1], L, nn, id_base, nthreads)
    return rc, dists, ids


def padded(X, pad, fill):
    """rows of X with `pad` extra columns of `fill` (never to be read): ldb = d + pad"""
    if pad == 0:
        return np.ascontiguousarray(X)
    out = np.full((X.shape[0], X.shape[1] + pad), fill, dtype=X.dtype)
    out[:, :X.shape[1]] = X
    return out


# the shapes both test files walk: every d at which the kernel takes another road (a single component, less than one 16-byte piece, one piece, one piece
# and a tail, whole 128-byte lines of f32 and one of uint8, lines and a tail), each with rows d and d + 3 elements apart
DIMS = [1, 3, 16, 17, 128, 130]
LISTS = [1, 63, 64, 65, 1000]               # one lane, a wave less one, a wave, a wave and one, four tiles with a ragged last one


def base_and_queries(d, n, nq, seed, u8=False):
    rng = np.random.default_rng(seed)
    if u8:
        Xb = rng.integers(0, 256, (n, d), dtype=np.uint8)
        Xq = rng.integers(0, 256, (nq, d)).astype(np.float32) + rng.random((nq, d), dtype=np.float32)
    else:
        Xb = rng.standard_normal((n, d)).astype(np.float32)
        Xq = rng.standard_normal((nq, d)).astype(np.float32)
    return Xb, Xq
