"""numpy restatement of exact k-NN (lsq_knn_exact*): the checker of tests/test_knn_exact.py and tests/test_gpu_knn_exact.py.

    dist(q, i) = ((0 + e_0 e_0) + e_1 e_1) + ... + e_{d-1} e_{d-1},   e_s = x_i[s] - q[s]     f32, s ascending, every op rounded
    result     = the nn smallest (dist, id) pairs in lexicographic order, ids 0-based uint32, NaN last

numpy's f32 array ops round each subtract, multiply and add separately, so the loop over s below reproduces the contract bit for bit."""
import numpy as np


def order_keys(dist):
    """Order-preserving u32 keys of f32 distances (a < b <=> key(a) < key(b)), NaN last: the library's record keys."""
    b = np.ascontiguousarray(dist, dtype=np.float32).view(np.uint32)
    k = np.where(b >> 31 == 1, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(dist), np.uint32(0xFFFFFFFF), k)


def knn_dists(Xb, Xq, chunk=1 << 22):
    """(nq, n) f32 distances by the contract; Xb (n, >= d) and Xq (nq, >= d) with d = Xq's width used of both."""
    Xb = np.asarray(Xb, dtype=np.float32)
    Xq = np.asarray(Xq, dtype=np.float32)
    n, nq, d = Xb.shape[0], Xq.shape[0], Xq.shape[1]
    out = np.empty((nq, n), dtype=np.float32)
    step = max(1, chunk // max(n, 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for q0 in range(0, nq, step):
            q = Xq[q0:q0 + step]
            acc = np.zeros((q.shape[0], n), dtype=np.float32)
            for s in range(d):
                e = Xb[None, :, s] - q[:, s, None]
                acc = acc + e * e
            out[q0:q0 + step] = acc
    return out


def knn_select(D, nn):
    """-> dists (nq, nn) f32, ids (nq, nn) uint32: the nn smallest (dist, id) pairs of each row of D, lexicographic, NaN last."""
    nq, n = D.shape
    keys = (order_keys(D).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]
    top = np.sort(keys, axis=1)[:, :nn]
    ids = (top & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    dists = np.take_along_axis(D, ids.astype(np.int64), axis=1)
    dists[np.isnan(dists)] = np.float32(np.nan)                     # the library hands out one NaN (0x7fc00000) whatever the payload
    return dists, ids


def knn_np(Xb, Xq, nn):
    return knn_select(knn_dists(Xb, Xq), nn)


def knn_cpu(lib, Xb, Xq, d, nn, nthreads=0):
    """lsq_knn_exact_cpu on row arrays Xb (n, ldb), Xq (nq, ldq) reading d floats of each row -> (rc, dists, ids)."""
    Xb = np.ascontiguousarray(Xb, dtype=np.float32)
    Xq = np.ascontiguousarray(Xq, dtype=np.float32)
    nq = Xq.shape[0]
    dists = np.zeros((nq, nn), dtype=np.float32)
    ids = np.zeros((nq, nn), dtype=np.uint32)
    rc = lib.lsq_knn_exact_cpu(dists.ctypes.data, ids.ctypes.data, Xb.ctypes.data, Xq.ctypes.data, Xb.shape[0], nq, d, Xb.shape[1], Xq.shape[1],
                               nn, nthreads)
    return rc, dists, ids


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))
