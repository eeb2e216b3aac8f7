"""The numpy statement of the four contracts of the coarse partition (include/lsq_mi355x.h, section 3i), the ctypes wrappers of its three host checkers
and the problems both test files share.  Nothing here needs a GPU.

    assign_np      the first of the (dist, list) pairs of the exact search: f32 direct form, dimensions ascending, ties to the smaller list, NaN last
    update_np      train_coarse's means: np.add.at on float64 sums (= the sequential row-order loop), sums / counts, .astype(float32); empty lists kept
    residuals_np   X.astype(float32) - centroids[assign]: one rounded subtraction
    code_norms_np  a = chain of a + r^ r^, b = chain of b + c r^, s = a + (b + b), float32 throughout; first minimum of (s - cb[j])^2

Every float32 operation below is a separate numpy ufunc call on float32 arrays: each one rounds, none is fused.
"""
import numpy as np

H = 256
PREFETCH = 32        # UPD_PREFETCH of csrc/lsq_partition.hip: rows in flight ahead of the update kernel's chain


def same(a, b):
    """bit for bit, a NaN of any payload equal to a NaN at the same place (IEEE leaves the payload open; host and device propagate different ones)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def keys(v):
    """lsq_adc_key: order-preserving uint32 keys of float32 values, NaN last"""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    k = np.where(b >> 31 == 1, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(v), np.uint32(0xFFFFFFFF), k)


def assign_np(X, cent):
    X, cent = np.asarray(X).astype(np.float32), np.asarray(cent, dtype=np.float32)
    acc = np.zeros((X.shape[0], cent.shape[0]), dtype=np.float32)
    for s in range(X.shape[1]):
        e = cent[None, :, s] - X[:, None, s]
        acc = acc + e * e
    return np.argmin(keys(acc), axis=1).astype(np.int32), acc        # argmin: the first minimum, i.e. the smaller list


def update_np(cent, X, assign):
    """-> (new centroids, counts): the lines of reference_api.train_coarse"""
    cent = np.array(cent, dtype=np.float32)
    X = np.asarray(X).astype(np.float32)
    nlist = cent.shape[0]
    sums = np.zeros(cent.shape, dtype=np.float64)
    np.add.at(sums, assign, X)
    counts = np.bincount(assign, minlength=nlist)
    live = counts > 0
    cent[live] = (sums[live] / counts[live, None]).astype(np.float32)
    return cent, counts.astype(np.int32)


def update_loop(cent, X, assign):
    """the same, as the contract words it: one float64 add after another in ascending row id"""
    cent = np.array(cent, dtype=np.float32)
    X = np.asarray(X).astype(np.float32)
    sums, counts = np.zeros(cent.shape, dtype=np.float64), np.zeros(cent.shape[0], dtype=np.int64)
    for i in range(X.shape[0]):
        sums[assign[i]] = sums[assign[i]] + X[i].astype(np.float64)
        counts[assign[i]] += 1
    for l in np.nonzero(counts)[0]:
        cent[l] = (sums[l] / np.float64(counts[l])).astype(np.float32)
    return cent, counts.astype(np.int32)


def residuals_np(X, cent, assign):
    with np.errstate(invalid="ignore"):
        return np.asarray(X).astype(np.float32) - np.asarray(cent, dtype=np.float32)[assign]


def code_norms_np(codes, K, cent, assign, cb=None):
    """-> norms [, norm_codes, dbnorms]"""
    codes, K, cent = np.asarray(codes), np.asarray(K, dtype=np.float32), np.asarray(cent, dtype=np.float32)
    n, m = codes.shape
    with np.errstate(invalid="ignore", over="ignore"):
        rec = K[codes[:, 0].astype(np.int64)].copy()
        for j in range(1, m):
            rec = rec + K[j * H + codes[:, j].astype(np.int64)]
        c = cent[assign]
        a, b = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        for t in range(K.shape[1]):
            a = a + rec[:, t] * rec[:, t]
            b = b + c[:, t] * rec[:, t]
        s = a + (b + b)
        if cb is None:
            return s
        cb = np.asarray(cb, dtype=np.float32)
        best = np.zeros(n, dtype=np.int64)
        df = s - cb[0]
        bd = df * df
        for j in range(1, cb.shape[0]):
            df = s - cb[j]
            dd = df * df
            take = dd < bd                                       # strict <: the first minimum; a NaN never wins
            best[take] = j
            bd = np.where(take, dd, bd)
    return s, best.astype(np.uint8), cb[best]


# ---- the host checkers through ctypes -----------------------------------------------------------------------------------------------------------------
def pitch(a):
    return a.shape[1] if a.shape[0] <= 1 else a.strides[0] // a.itemsize


def update_cpu(L, cent, X, assign, nthreads=0):
    """-> (rc, new centroids, counts); X: a float32 or uint8 row view"""
    cent = np.array(cent, dtype=np.float32, order="C")
    counts = np.full(cent.shape[0], -7, dtype=np.int32)
    assign = np.ascontiguousarray(assign, dtype=np.int32)
    rc = L.lsq_partition_update_cpu(cent.ctypes.data, counts.ctypes.data, X.ctypes.data, int(X.dtype == np.uint8), X.shape[0], cent.shape[1], pitch(X),
                                    assign.ctypes.data, cent.shape[0], nthreads)
    return rc, cent, counts


def residuals_cpu(L, X, cent, assign, nthreads=0, out=None):
    cent, assign = np.ascontiguousarray(cent, dtype=np.float32), np.ascontiguousarray(assign, dtype=np.int32)
    R = np.zeros((X.shape[0], cent.shape[1]), dtype=np.float32) if out is None else out
    rc = L.lsq_partition_residuals_cpu(R.ctypes.data, pitch(R), X.ctypes.data, int(X.dtype == np.uint8), X.shape[0], cent.shape[1], pitch(X),
                                       cent.ctypes.data, assign.ctypes.data, cent.shape[0], nthreads)
    return rc, R


def code_norms_cpu(L, codes, K, cent, assign, cb=None, nthreads=0):
    """-> (rc, norms, norm_codes, dbnorms); the last two stay at their fill values (255, -7) when cb is None"""
    codes, K = np.ascontiguousarray(codes, dtype=np.uint8), np.ascontiguousarray(K, dtype=np.float32)
    cent, assign = np.ascontiguousarray(cent, dtype=np.float32), np.ascontiguousarray(assign, dtype=np.int32)
    n, m = codes.shape
    norms, nc, dbn = np.full(n, -7, np.float32), np.full(n, 255, np.uint8), np.full(n, -7, np.float32)
    cbp = None if cb is None else np.ascontiguousarray(cb, dtype=np.float32)
    rc = L.lsq_partition_code_norms_cpu(norms.ctypes.data, nc.ctypes.data, dbn.ctypes.data, codes.ctypes.data, K.ctypes.data, cent.ctypes.data,
                                        assign.ctypes.data, n, m, H, K.shape[1], cent.shape[0], None if cbp is None else cbp.ctypes.data,
                                        0 if cbp is None else cbp.shape[0], nthreads)
    return rc, norms, nc, dbn


# ---- problems ----------------------------------------------------------------------------------------------------------------------------------------
def decades(n, d, seed):
    """float32 values spread over twelve decades, both signs: a float32 sum differs from the float64 one in most entries"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, d)) * 10.0 ** rng.uniform(-6, 6, (n, d))).astype(np.float32)


def row_view(a, extra, offset=0):
    """a copy of the 2-d array `a` as a row view: `extra` more elements between the rows, the first row `offset` elements into its buffer"""
    n, d = a.shape
    buf = np.full(offset + n * (d + extra) + 3, 77, dtype=a.dtype)
    v = buf[offset:offset + n * (d + extra)].reshape(n, d + extra)[:, :d]
    v[:] = a
    return v


def untouched_dev(buf, first, n, d, ld, fill):
    """every element of the flat buffer `buf` outside the n rows of d elements that start at `first` and lie `ld` apart still holds `fill`"""
    mask = np.ones(buf.shape[0], dtype=bool)
    mask[(first + np.arange(n)[:, None] * ld + np.arange(d)[None, :]).reshape(-1)] = False
    return bool(np.all(buf[mask] == fill))


def untouched(v, fill):
    """the same for the buffer under the numpy row view `v`"""
    buf = v
    while buf.base is not None:
        buf = buf.base
    return untouched_dev(buf, (v.ctypes.data - buf.ctypes.data) // v.itemsize, v.shape[0], v.shape[1], pitch(v), fill)


def special_rows(X, cent, seed):
    """NaN, +-inf and -0.0 sprinkled over float32 rows and centroids, in place"""
    rng = np.random.default_rng(seed)
    for arr in (X, cent):
        flat = arr.reshape(-1)
        for v in (np.nan, np.inf, -np.inf, -0.0):
            flat[rng.integers(0, flat.shape[0], max(1, flat.shape[0] // 50))] = np.float32(v)
    return X, cent


def ladder_lists(nlist_extra=3):
    """lists of 1, 2, ... 2 * PREFETCH + 1 rows, their row ids interleaved, plus `nlist_extra` lists without rows (first, middle, last)
    -> (assign (n,) int32, nlist)"""
    sizes = list(range(1, 2 * PREFETCH + 2))
    lists = np.concatenate([np.full(s, k + 1, dtype=np.int32) for k, s in enumerate(sizes)])      # list 0 stays empty
    lists[lists > len(sizes) // 2] += 1                                                            # one in the middle too
    np.random.default_rng(4).shuffle(lists)
    return lists, int(lists.max()) + 2                                                             # and the last one


TIE = (70, 60000)      # assign_problem: two centroids with the same bits


def assign_problem(nlist, u8=False, n=2000, d=8, seed=0):
    """-> (centroids (nlist, d) f32, X (n, d) f32 or uint8), values * 40 + 128 (uint8: both clipped to 0 .. 254 and floored).  Centroids TIE[0] and TIE[1]
    are equal and row n // 2 lies one step beside them in every dimension: an exact tie, the smaller list wins.  Row 7 equals centroid 123: distance +0.0"""
    rng = np.random.default_rng(seed + nlist)
    cent = (rng.standard_normal((nlist, d)) * 40 + 128).astype(np.float32)
    X = (rng.standard_normal((n, d)) * 40 + 128).astype(np.float32)
    if u8:
        cent, X = np.floor(np.clip(cent, 0, 254)), np.floor(np.clip(X, 0, 254))
    cent[TIE[1]] = cent[TIE[0]]
    X[n // 2] = cent[TIE[0]] + np.float32(1)
    X[7] = cent[123]
    return cent, (X.astype(np.uint8) if u8 else X)


def duplicated_centroids(n=300, d=8, nlist=65537, seed=12):
    """-> (centroids, X): centroids 5000 .. 44 999 are one point v, the first 100 rows lie beside v (40 000 lists tie at the threshold of their coarse
    search, the smallest wins), the other rows are anywhere"""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    X = rng.standard_normal((n, d)).astype(np.float32)
    v = np.float32(0.5) * X[0]
    cent[5000:45000] = v
    X[:100] = v + np.float32(0.01) * rng.standard_normal((100, d)).astype(np.float32)
    return cent, X


def code_problem(n, d, m, nlist, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    K = (rng.standard_normal((m * H, d)) * scale).astype(np.float32)
    codes = rng.integers(0, H, (n, m)).astype(np.uint8)
    cent = (rng.standard_normal((nlist, d)) * 3).astype(np.float32)
    assign = rng.integers(0, nlist, n).astype(np.int32)
    return codes, K, cent, assign
