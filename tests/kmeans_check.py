"""Numpy checker of the two device steps of resident PQ / OPQ training (csrc/lsq_kmeans.hip): cluster means and k-means++ seeding.

Written from the rules of include/lsq_mi355x.h alone, as explicit loops over the order of the arithmetic -- nothing here calls the code under test.

  centers_exact    per codebook, code and covered dimension: the rows holding the code added in ascending row order with plain f32 adds, divided by the
                   count in double, rounded to f32; an empty cluster takes its row of K_prev (None: zero); +0.0 outside the cover.
  seed_f64         the seeding rule with the prefix sums taken by numpy in float64 (cumsum, row by row).
  judge_seeding    judges the rows a seeding call chose INDEPENDENTLY of the order in which it summed: d2 is replayed exactly from the call's own earlier
                   choices, P = float64 cumsum(d2), target = u P[-1]; row i is accepted iff d2[i] > 0 and P[i-1] - band <= target <= P[i] + band with
                   band = 2 n 2^-53 P[-1] -- the worst-case rounding of two n-term sums of non-negative doubles (the call's prefix and its total), derived,
                   not tuned.  A step whose target lies within band of a boundary of P is counted as ambiguous (either neighbour is accepted there).
"""
import numpy as np

H = 256


def clustered(d, n, k=40, seed=0, spread=0.2):
    """The generator of tests/test_gpu_initializers.py (_clustered): 40 Gaussian blobs -> d x n f32."""
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((d, k)).astype(np.float32) * 2.0
    a = rng.integers(k, size=n)
    return (cen[:, a] + spread * rng.standard_normal((d, n))).astype(np.float32)


def pq_cover(d, m):
    """dim2C (d, m) of PQ / OPQ: codebook j covers splitarray(1:d, m)[j] (src/utils.jl:152-177: the first d mod m parts get one more)."""
    cover = np.zeros((d, m), dtype=np.uint8)
    base, extra, lo = d // m, d % m, 0
    for j in range(m):
        w = base + (1 if j < extra else 0)
        cover[lo:lo + w, j] = 1
        lo += w
    return cover


def chain_cover(d, m):
    """dim2C of a chain (src/codebook_update.jl:88-102): m - 1 blocks, codebook j covers blocks j - 1 and j -- overlapping codebooks."""
    blocks = pq_cover(d, m - 1)
    cover = np.zeros((d, m), dtype=np.uint8)
    for j in range(m):
        if j > 0:
            cover[:, j] |= blocks[:, j - 1]
        if j < m - 1:
            cover[:, j] |= blocks[:, j]
    return cover


def centers_exact(X, codes, dim2C, h=H, K_prev=None):
    """X (n, d) f32, codes (n, m) 0-based, dim2C (d, m) -> (K (m h, d) f32, counts (m h,) int32).  The loop runs over the RANK of a row inside its cluster:
    step r adds the r-th row (ascending) of every cluster that has one -- one f32 add per entry and step, clusters side by side."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    codes = np.asarray(codes, dtype=np.int64)
    n, d = X.shape
    m = codes.shape[1]
    K = np.zeros((m * h, d), dtype=np.float32)
    counts = np.zeros(m * h, dtype=np.int32)
    for j in range(m):
        dims = np.nonzero(np.asarray(dim2C)[:, j])[0]
        a = codes[:, j]
        cnt = np.bincount(a, minlength=h)[:h]
        order = np.argsort(a, kind="stable")                      # grouped by code, ascending row inside a group
        start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        Xs = X[:, dims]
        acc = np.zeros((h, dims.size), dtype=np.float32)
        for r in range(int(cnt.max()) if n else 0):
            cl = np.nonzero(cnt > r)[0]
            acc[cl] = acc[cl] + Xs[order[start[cl] + r]]
        nz = cnt > 0
        block = np.zeros((h, d), dtype=np.float32)
        block[np.ix_(nz, dims)] = (acc[nz].astype(np.float64) / cnt[nz].astype(np.float64)[:, None]).astype(np.float32)
        if K_prev is not None:
            block[np.ix_(~nz, dims)] = np.asarray(K_prev, dtype=np.float32)[j * h:(j + 1) * h][np.ix_(~nz, dims)]
        K[j * h:(j + 1) * h] = block
        counts[j * h:(j + 1) * h] = cnt
    return K, counts


def d2_direct(X, row, dims):
    """||x_i - x_row||^2 over `dims` ascending: f32, direct form, one rounded multiply and one rounded add per dimension (no FMA)."""
    s = np.zeros(X.shape[0], dtype=np.float32)
    for t in dims:
        e = X[:, t] - X[row, t]
        s = s + e * e
    return s


def uniform_row(u, n):
    return min(n - 1, int(np.floor(u * n)))


def seed_f64(X, dim2C, u, h=H):
    """The seeding rule with numpy's float64 cumsum as the prefix sum -> (idx (m, h) int64, d2 (n, m) f32 to the nearest of all h chosen rows)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    n, m = X.shape[0], np.asarray(dim2C).shape[1]
    idx = np.zeros((m, h), dtype=np.int64)
    d2_all = np.zeros((n, m), dtype=np.float32)
    for j in range(m):
        dims = np.nonzero(np.asarray(dim2C)[:, j])[0]
        idx[j, 0] = uniform_row(u[j, 0], n)
        d2 = d2_direct(X, idx[j, 0], dims)
        for k in range(1, h):
            P = np.cumsum(d2.astype(np.float64))
            if P[-1] > 0:
                idx[j, k] = min(n - 1, int(np.searchsorted(P, u[j, k] * P[-1], side="right")))      # the first i with P[i] > target
            else:
                idx[j, k] = uniform_row(u[j, k], n)
            d2 = np.minimum(d2, d2_direct(X, idx[j, k], dims))
        d2_all[:, j] = d2
    return idx, d2_all


def judge_seeding(X, dim2C, u, idx, h=H):
    """-> dict: steps, ambiguous (count), bad (list of (j, k, why)), zero_road (steps that took the tot == 0 rule), min_gap (smallest distance of a target
    to a boundary, relative to the total), max_band (largest band / total), d2 (n, m): the exact replay from idx, to the nearest of all h rows."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    n, m = X.shape[0], np.asarray(dim2C).shape[1]
    idx = np.asarray(idx, dtype=np.int64)
    out = {"steps": 0, "ambiguous": 0, "bad": [], "zero_road": 0, "min_gap": np.inf, "max_band": 0.0, "d2": np.zeros((n, m), dtype=np.float32)}
    if idx.shape != (m, h) or idx.min() < 0 or idx.max() >= n:
        out["bad"].append((-1, -1, "indices out of range or of the wrong shape"))
        return out
    for j in range(m):
        dims = np.nonzero(np.asarray(dim2C)[:, j])[0]
        if idx[j, 0] != uniform_row(u[j, 0], n):
            out["bad"].append((j, 0, "step 0 is row %d, the rule gives %d" % (idx[j, 0], uniform_row(u[j, 0], n))))
        d2 = d2_direct(X, idx[j, 0], dims)
        for k in range(1, h):
            out["steps"] += 1
            i = int(idx[j, k])
            P = np.cumsum(d2.astype(np.float64))
            tot = P[-1]
            if tot > 0:
                target = u[j, k] * tot
                band = 2.0 * n * 2.0 ** -53 * tot
                before = P[i - 1] if i > 0 else 0.0
                if not d2[i] > 0:
                    out["bad"].append((j, k, "row %d at distance 0 chosen while the total is %g" % (i, tot)))
                elif not (before - band <= target <= P[i] + band):
                    out["bad"].append((j, k, "row %d: target %.17g outside [%.17g, %.17g] +- %.3g" % (i, target, before, P[i], band)))
                q = int(np.searchsorted(P, target))
                gap = min(abs(P[min(q, n - 1)] - target), abs((P[q - 1] if q > 0 else 0.0) - target))
                out["min_gap"] = min(out["min_gap"], gap / tot)
                out["max_band"] = max(out["max_band"], band / tot)
                if gap <= band:
                    out["ambiguous"] += 1
            else:
                out["zero_road"] += 1
                if i != uniform_row(u[j, k], n):
                    out["bad"].append((j, k, "total 0: row %d, the rule gives %d" % (i, uniform_row(u[j, k], n))))
            d2 = np.minimum(d2, d2_direct(X, i, dims))
        out["d2"][:, j] = d2
    return out


# the three seeding problems of the tests: (d, n, m) on clustered(d, n, seed=2); m = 1 is plain k-means
SEED_PROBLEMS = [(16, 3000, 4), (4, 20000, 1), (32, 100000, 4)]


def seed_problem(d, n, m):
    X = np.ascontiguousarray(clustered(d, n, seed=2).T)
    u = np.random.default_rng(1000 + d + m).random((m, H))
    return X, pq_cover(d, m), u
