"""Shared pieces of tests/test_index_knn.py and tests/test_gpu_index_knn.py: data, matrices laid out at byte offsets with padded pitches, and the two
checkers of exact k-NN on 8-bit sets -- neither calls the code under test:

    widened   lsq_knn_exact_cpu (tests/knn_check.py, tests/test_knn_exact.py) on astype(float32): the contract at every d
    int64     float32(SUM (x - q)^2) in int64 with a (dist, id) lexsort: equals the contract while the sum stays <= 2^24, i.e. for d <= 258"""
import numpy as np

import knn_check as KC

PAD = 255          # what padding columns and the bytes around a matrix are filled with: a loader that reads them changes a distance


def u8_data(seed, n, nq, d, hi=256):
    rng = np.random.default_rng(seed)
    return rng.integers(0, hi, (n, d), dtype=np.uint8), rng.integers(0, hi, (nq, d), dtype=np.uint8)


def extreme(n, nq, d, seed=0):
    """rows of mostly 255 against queries of mostly 0 (a few entries random): the largest distances d allows; row 0 / query 0 are all 255 / all 0"""
    rng = np.random.default_rng(seed)
    Xb = np.full((n, d), 255, dtype=np.uint8)
    Xq = np.zeros((nq, d), dtype=np.uint8)
    for M in (Xb, Xq):
        for r in range(1, M.shape[0]):
            c = rng.integers(0, d, max(1, d // 16))
            M[r, c] = rng.integers(0, 256, c.size)
    return Xb, Xq


def laid_out(M, ld, offset, dtype=None):
    """M (rows, d) as a view with row pitch ld ELEMENTS starting `offset` BYTES into a buffer filled with PAD -> (view (rows, d), buffer); the buffer ends
    with the d-th element of the last row, so a read past it leaves the allocation"""
    M = np.ascontiguousarray(M if dtype is None else M.astype(dtype))
    rows, d = M.shape
    es = M.itemsize
    buf = np.full(offset + ((rows - 1) * ld + d) * es, PAD, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[offset:].view(np.uint8), shape=(rows, d * es), strides=(ld * es, 1))
    view[:, :] = M.view(np.uint8).reshape(rows, d * es)
    out = np.ndarray((rows, d), dtype=M.dtype, buffer=buf, offset=offset, strides=(ld * es, es)) if offset % es == 0 else None
    return out, buf


def knn_int64(Xb, Xq, nn):
    """-> dists (nq, nn) f32, ids (nq, nn) uint32 0-based, from int64 arithmetic (valid while every distance <= 2^24)"""
    D = ((Xb.astype(np.int64)[None, :, :] - Xq.astype(np.int64)[:, None, :]) ** 2).sum(2)
    assert D.max() <= 1 << 24
    ids = np.lexsort((np.broadcast_to(np.arange(D.shape[1]), D.shape), D), axis=1)[:, :nn]
    return np.take_along_axis(D, ids, axis=1).astype(np.float32), ids.astype(np.uint32)


def knn_widened(lib, Xb, Xq, nn):
    rc, dists, ids = KC.knn_cpu(lib, Xb.astype(np.float32), Xq.astype(np.float32), Xq.shape[1], nn)
    assert rc == 0
    return dists, ids


def knn_u8_cpu(lib, bptr, base_u8, qptr, q_u8, n, nq, d, ldb, ldq, nn, nthreads=2):
    """lsq_knn_exact_u8_cpu on raw addresses -> (rc, dists, ids)"""
    dists = np.zeros((nq, max(nn, 1)), dtype=np.float32)
    ids = np.zeros((nq, max(nn, 1)), dtype=np.uint32)
    rc = lib.lsq_knn_exact_u8_cpu(dists.ctypes.data, ids.ctypes.data, bptr, int(base_u8), qptr, int(q_u8), n, nq, d, ldb, ldq, nn, nthreads)
    return rc, dists, ids


def same(d1, i1, d2, i2):
    assert np.array_equal(np.asarray(i1).view(np.uint32), np.asarray(i2).view(np.uint32)), "ids differ at %s" % (np.argwhere(np.asarray(i1).view(np.uint32) != np.asarray(i2).view(np.uint32))[:5].tolist(),)
    assert KC.same_bits(d1, d2), "distances differ"
