"""numpy restatement of the inverted-list search (lsq_ivf_search_cpu, lsq_index_search_ivf): the checker of tests/test_ivf.py and tests/test_gpu_ivf.py.

    probed lists  the nprobe smallest (coarse, list) pairs, coarse = knn_check.knn_dists' distance of the query's coarse row to the centroid
    table[e]      ((0 - (2 q_0) c_e0) - (2 q_1) c_e1) - ...        f32, k ascending, every op rounded
    dist(i)       (((0 + table[0 h + b_i0]) + table[1 h + b_i1]) + ...) + dbnorms[i]   [then + coarse(q, list of i) with add_coarse]
    result        the nn smallest (dist, id) pairs over the rows of the probed lists, ids 1-based original rows, NaN after every number, then (+inf, 0)"""
import numpy as np

from knn_check import knn_dists, order_keys

H = 256
ADD_COARSE, EVERY_RECORD, TEST_BATCH = 1, 2, 4


def adc_dists(codes, K, dbn, Qs):
    """(nq, n) f32 ADC distances by the scans' rule"""
    (n, m), (nq, d) = codes.shape, Qs.shape
    with np.errstate(invalid="ignore", over="ignore"):
        T = np.zeros((nq, K.shape[0]), dtype=np.float32)
        for k in range(d):
            T = T - (np.float32(2) * Qs[:, k, None]) * K[None, :, k]
        acc = np.zeros((nq, n), dtype=np.float32)
        for j in range(m):
            acc = acc + T[:, j * (K.shape[0] // m) + codes[:, j].astype(np.int64)]
        return acc + dbn[None, :]


def probes_np(cent, Qc, nprobe):
    """-> coarse (nq, nlist) f32, probes (nq, nprobe) list ids in rank order"""
    Dc = knn_dists(cent, Qc)
    keys = (order_keys(Dc).astype(np.uint64) << np.uint64(32)) | np.arange(cent.shape[0], dtype=np.uint64)[None, :]
    return Dc, (np.sort(keys, axis=1)[:, :nprobe] & np.uint64(0xFFFFFFFF)).astype(np.int64)


def ivf_np(codes, K, dbn, cent, lor, Qs, Qc, nprobe, nn, add_coarse=False):
    """-> dists (nq, nn) f32, ids (nq, nn) int32"""
    n, nq = codes.shape[0], Qs.shape[0]
    Dc, probes = probes_np(cent, Qc, nprobe)
    dist = adc_dists(codes, K, dbn, Qs)
    if add_coarse:
        with np.errstate(invalid="ignore", over="ignore"):
            dist = dist + Dc[:, lor]
    probed = np.zeros(Dc.shape, dtype=bool)
    probed[np.arange(nq)[:, None], probes] = True
    width = max(n, nn)                                                       # columns past n: the padding entries
    ok = np.zeros((nq, width), dtype=bool)
    ok[:, :n] = probed[:, lor]
    full = np.full((nq, width), np.float32(np.inf), dtype=np.float32)
    full[:, :n] = dist
    full = np.where(ok, full, np.float32(np.inf)).astype(np.float32)
    hi = order_keys(full).astype(np.uint64) | ((~ok).astype(np.uint64) << np.uint64(32))
    field = np.where(ok, np.arange(width)[None, :] + 1, 0)
    order = np.stack([np.lexsort((field[q], hi[q])) for q in range(nq)])[:, :nn]
    out_d = np.take_along_axis(full, order, axis=1)
    out_d[np.isnan(out_d)] = np.float32(np.nan)                              # the library hands out one NaN (0x7fc00000) whatever the payload
    return out_d, np.take_along_axis(field, order, axis=1).astype(np.int32)


def tail_hits_np(codes, K, dbn, cent, lor, Qs, Qc, nprobe, nn, add_coarse=False):
    """per query (rows of the head, rows of the tail, tail rows with !(dist > tau)): what the thresholded road appends, by the contract's definition
    of the head (the first probed lists, in rank order, that hold nn rows together) and of tau (the head's nn-th smallest distance)"""
    Dc, probes = probes_np(cent, Qc, nprobe)
    dist = adc_dists(codes, K, dbn, Qs)
    if add_coarse:
        dist = dist + Dc[:, lor]
    out = []
    for q in range(Qs.shape[0]):
        head, rows = [], 0
        for l in probes[q]:
            if rows >= nn:
                break
            head.append(l)
            rows += int((lor == l).sum())
        in_head = np.isin(lor, head)
        in_tail = np.isin(lor, probes[q][len(head):])
        if rows < nn:
            out.append((rows, 0, 0))
            continue
        tau = np.sort(order_keys(dist[q, in_head]))[nn - 1]
        out.append((rows, int(in_tail.sum()), int((order_keys(dist[q, in_tail]) <= tau).sum()) if tau != 0xFFFFFFFF else int(in_tail.sum())))
    return out


def ivf_cpu(lib, codes, K, dbn, cent, lor, Qs, Qc, nprobe, nn, flags=0, nthreads=0):
    """lsq_ivf_search_cpu on row arrays -> (rc, dists, ids)"""
    codes, K, dbn = np.ascontiguousarray(codes, dtype=np.uint8), np.ascontiguousarray(K, dtype=np.float32), np.ascontiguousarray(dbn, dtype=np.float32)
    cent, lor = np.ascontiguousarray(cent, dtype=np.float32), np.ascontiguousarray(lor, dtype=np.int32)
    Qs = np.ascontiguousarray(Qs, dtype=np.float32)
    Qc = None if Qc is None else np.ascontiguousarray(Qc, dtype=np.float32)
    (n, m), (nq, d) = codes.shape, Qs.shape
    dists, ids = np.zeros((nq, nn), dtype=np.float32), np.zeros((nq, nn), dtype=np.int32)
    rc = lib.lsq_ivf_search_cpu(dists.ctypes.data, ids.ctypes.data, codes.ctypes.data, K.ctypes.data, dbn.ctypes.data, cent.ctypes.data, lor.ctypes.data,
                                Qs.ctypes.data, None if Qc is None else Qc.ctypes.data, n, m, K.shape[0] // m, d, cent.shape[0], nq, d, nprobe, nn,
                                flags, nthreads)
    return rc, dists, ids


def skewed_lists(rng, n, nlist):
    """lists 1, 2 (and the last) empty, lists 3, 4 one row each, list 0 half of the rows (longer than one block pass), the others random"""
    if nlist < 7:
        return rng.integers(0, nlist, n).astype(np.int32) if nlist > 1 else np.zeros(n, dtype=np.int32)
    lor = rng.integers(5, nlist - 1, n).astype(np.int32)
    perm = rng.permutation(n)
    lor[perm[:n // 2]] = 0
    lor[perm[n // 2]], lor[perm[n // 2 + 1]] = 3, 4
    return lor


def problem(n, d, m, nlist, nq, seed, small_int=False, lists="skewed"):
    """codes, K, dbnorms, centroids, list_of_row, Q_scan, Q_coarse of a quantised base with a coarse partition laid over it"""
    rng = np.random.default_rng(seed)
    if small_int:                                                            # exact ties: every table entry and every norm is a small integer
        K = rng.integers(-2, 3, (m * H, d)).astype(np.float32)
        Qs = rng.integers(-2, 3, (nq, d)).astype(np.float32)
        cent = rng.integers(-2, 3, (nlist, d)).astype(np.float32)
    else:
        K = (rng.standard_normal((m * H, d)) / np.sqrt(m)).astype(np.float32)
        Qs = rng.standard_normal((nq, d)).astype(np.float32)
        cent = rng.standard_normal((nlist, d)).astype(np.float32)
    codes = rng.integers(0, H, (n, m)).astype(np.uint8)
    recon = sum(K[j * H + codes[:, j].astype(np.int64)] for j in range(m))
    dbn = (recon.astype(np.float64) ** 2).sum(1).astype(np.float32)
    lor = skewed_lists(rng, n, nlist) if lists == "skewed" else (np.arange(n) % nlist).astype(np.int32) if lists == "even" else \
        rng.integers(0, nlist, n).astype(np.int32)
    Qc = (Qs + np.float32(0.25) * rng.standard_normal((nq, d)).astype(np.float32)) if not small_int else Qs.copy()
    return codes, K, dbn, cent, lor, Qs, Qc


# (d, m, nlist, nprobe, nn, nq): every value of the issue's grid at least once; m = 8, 16 take the dword loader, 1 and 7 the byte loader
SHAPES = [(5, 1, 1, 1, 1, 1), (32, 7, 7, 3, 10, 37), (32, 8, 40, 3, 300, 37), (5, 16, 40, 40, 10, 37), (32, 8, 7, 7, 300, 1), (5, 7, 40, 1, 1, 37),
          (32, 16, 7, 1, 300, 37), (32, 8, 40, 40, 1, 37), (5, 8, 7, 3, 10, 1), (32, 1, 40, 3, 10, 37), (5, 16, 1, 1, 300, 37), (32, 7, 40, 40, 300, 1)]
N = 3000
