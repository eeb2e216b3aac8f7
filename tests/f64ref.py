"""Float64 references for every quantity the kernels compute, each with a rigorous bound on its f32 evaluation, and the comparators that use them.

Written from the formulas of the method (LSQ / PQ / ChainQ), not from oracle/ or the product: the point is to check both from outside.  Every value
is computed in float64 from the f32 inputs, so its own rounding is some 2^-29 of the f32 bound below and is ignored.

Bounds (Higham, "Accuracy and Stability of Numerical Algorithms", 3.1): a sum of k rounded products, added in ANY order and with or without fused
multiply-adds, is within  gamma_k * sum_i |a_i b_i|  of the exact sum, gamma_k = k u / (1 - k u), u = 2^-24.  Scalings by 2 are exact.  A bound
stated for a formula therefore holds for every evaluation order and every blocking a kernel may choose.

Comparators:
  * check_values:     |got - ref64| <= bound, elementwise.
  * check_selection:  a top-k list / an argmin is accepted iff every chosen item's float64 value is at most the true k-th plus its own bound and
                      the bound of the item it may have displaced, and every item not chosen is at least the true k-th minus its own bound and that
                      of the item that may have displaced it (swaps inside the rounding window and nothing else); the returned distances are within
                      their bound and non-decreasing.
  * check_chain:      Viterbi codes: their float64 chain energy is within the bound of the optimum of an independent min-sum DP.
"""
import numpy as np

U32 = 2.0 ** -24
H = 256


def gamma(k):
    """gamma_k = k u / (1 - k u), u = 2^-24"""
    k = np.asarray(k, dtype=np.float64)
    assert np.all(k * U32 < 0.5)
    return k * U32 / (1.0 - k * U32)


def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def splitarray(n, nparts):
    """Split 0..n-1 into nparts contiguous ranges, the first n mod nparts of them one longer -> list of 0-based slices."""
    per, extra = divmod(n, nparts)
    out, lo = [], 0
    for p in range(nparts):
        hi = lo + per + (1 if p < extra else 0)
        out.append(slice(lo, hi))
        lo = hi
    return out


# ---- the encoder's tables ------------------------------------------------------------------------------------------------------------------

def unaries(X, K, m, h=H):
    """U[j, i, a] = -2 <c_ja, x_i> + ||c_ja||^2 -> (U64 (m, n, h), bound (m, n, h))."""
    X, K = _f64(X), _f64(K)
    d = X.shape[1]
    nrm = (K * K).sum(1)
    U = (nrm[None, :] - 2.0 * (X @ K.T)).reshape(X.shape[0], m, h).transpose(1, 0, 2)
    mag = (nrm[None, :] + 2.0 * (np.abs(X) @ np.abs(K).T)).reshape(X.shape[0], m, h).transpose(1, 0, 2)
    # 2d products (d of 2 x c, d of c c) summed in any tree, plus at most two roundings where partial sums meet: gamma_{2d+2} (2 sum|x c| + sum c^2)
    return U, gamma(2 * d + 2) * mag


def pair_tables(K, m, h=H):
    """T[j, k, b, a] = 2 <c_kb, c_ja> (the column added to node j when codebook k holds b) -> (T64 (m, m, h, h), bound)."""
    K = _f64(K)
    d = K.shape[1]
    G = K @ K.T
    A = np.abs(K) @ np.abs(K).T
    T = 2.0 * G.reshape(m, h, m, h).transpose(2, 0, 1, 3)          # [j, k, b, a] = G[k h + b, j h + a]
    # d products: gamma_d * 2 sum |c c|
    return T, gamma(d) * 2.0 * A.reshape(m, h, m, h).transpose(2, 0, 1, 3)


def _codewords(K, codes, m, h=H):
    codes = np.asarray(codes, dtype=np.int64)
    return [K[j * h + codes[:, j]] for j in range(m)]


def reconstruct(K, codes, m, h=H):
    """x_hat_i = sum_j c_j[b_ij] in float64 -> (n, d)"""
    cw = _codewords(_f64(K), codes, m, h)
    return sum(cw)


def veccost(X, K, codes, m, h=H):
    """||x - sum_j c_j[b_j]||^2 -> (cost64 (n,), bound (n,)); codes (n, m) 0-based."""
    X = _f64(X)
    cw = _codewords(_f64(K), codes, m, h)
    r = X - sum(cw)
    A = np.abs(X) + sum(np.abs(c) for c in cw)
    # every evaluation -- direct (residual of m + 1 terms, squared, d of them summed) or expanded (||x||^2 + unaries + pair terms: at most
    # 2d + (m + 1)^2 rounded terms deep) -- sums products whose magnitudes add up to at most sum_t A_t^2, A_t = |x_t| + sum_j |c_jt|:
    # gamma_{2d + (m+1)^2 + 2} sum_t A_t^2
    d = X.shape[1]
    return (r * r).sum(1), gamma(2 * d + (m + 1) ** 2 + 2) * (A * A).sum(1)


def mean_bound(bounds, values):
    """The mean of n f32 costs: the per-item bounds averaged, plus gamma_n of the mean of |value| for an f32 (or better) accumulation."""
    n = len(values)
    return float(np.mean(bounds)) + float(gamma(n)) * float(np.mean(np.abs(values) + bounds))


def norms(K, codes, m, h=H):
    """||x_hat||^2 -> (norm64 (n,), bound (n,))."""
    cw = _codewords(_f64(K), codes, m, h)
    xh = sum(cw)
    A = sum(np.abs(c) for c in cw)
    d = xh.shape[1]
    # x_hat_t carries at most gamma_{m-1} A_t, A_t = sum_j |c_jt|; squaring doubles that (gamma_{2m}), then the square and d-term sum: gamma_{2m+d+1} sum_t A_t^2
    return (xh * xh).sum(1), gamma(2 * m + d + 1) * (A * A).sum(1)


def norm_centroid_values(nrm64, nrm_bound, cbnorms):
    """(n - cb_c)^2 per centroid -> (values (n, ncb), bound): n carries E = nrm_bound, the difference and the square one rounding each:
    |(D + E)^2 (1 + gamma_2) - D^2| <= 2 D E + E^2 + gamma_2 (D + E)^2, D = |n - cb_c|"""
    cb = _f64(cbnorms).reshape(-1)
    D = np.abs(np.asarray(nrm64)[:, None] - cb[None, :])
    E = np.asarray(nrm_bound)[:, None]
    return D * D, 2 * D * E + E * E + gamma(2) * (D + E) ** 2


# ---- the scans -----------------------------------------------------------------------------------------------------------------------------

def lsq_adc(Q, K, codes, dbnorms, m, h=H):
    """LSQ ADC distance -2 <q, x_hat> + dbnorm -> (dist64 (nq, n), bound (nq, n))."""
    Q, K = _f64(Q), _f64(K)
    cw = _codewords(K, codes, m, h)
    xh = sum(cw)
    A = sum(np.abs(c) for c in cw)
    dbn = _f64(dbnorms)
    d = Q.shape[1]
    # d products per table entry, then m entries and the norm summed: gamma_{d+m+1} (2 sum_j sum_t |q_t c_jt| + |dbnorm|)
    return dbn[None, :] - 2.0 * (Q @ xh.T), gamma(d + m + 1) * (2.0 * (np.abs(Q) @ A.T) + np.abs(dbn)[None, :])


def pq_dist(Q, C, codes, dims=None):
    """PQ distance sum_k ||q_k - C_k[b_k]||^2 over the sub-spaces dims (default: splitarray(d, m)); C: list of (h, width_k) or an (m, h, w) array.
    -> (dist64 (nq, n), bound (nq, n))."""
    Q = _f64(Q)
    m = len(C)
    dims = splitarray(Q.shape[1], m) if dims is None else dims
    codes = np.asarray(codes, dtype=np.int64)
    out = np.zeros((Q.shape[0], codes.shape[0]))
    for k in range(m):
        Ck = _f64(C[k])
        assert Ck.shape[1] == dims[k].stop - dims[k].start, "codebook %d does not match its sub-space" % k
        qk = Q[:, dims[k]]
        if Ck.shape[1] <= 64:                                      # squares of differences where it is cheap (no cancellation at all)
            tab = ((qk[:, None, :] - Ck[None, :, :]) ** 2).sum(2)
        else:                                                      # wide sub-spaces: expanded, its float64 cancellation far below the f32 bound
            tab = np.maximum((qk * qk).sum(1)[:, None] + (Ck * Ck).sum(1)[None, :] - 2.0 * qk @ Ck.T, 0.0)
        out += tab[:, codes[:, k]]
    w = max(s.stop - s.start for s in dims)
    # every term (c - q) rounded, squared and rounded, then m * w non-negative terms summed: gamma_{m w + 2} * dist
    return out, gamma(m * w + 2) * out


# ---- the initialisers ----------------------------------------------------------------------------------------------------------------------

def chain_energy(X, K, codes, m, h=H):
    """sum_j U_j[b_j] + sum_{j<m-1} 2 <c_j[b_j], c_{j+1}[b_{j+1}]> (= ||x - x_hat||^2 - ||x||^2 for chain neighbours) -> (E64 (n,), bound (n,))."""
    X, K = _f64(X), _f64(K)
    cw = _codewords(K, codes, m, h)
    d = X.shape[1]
    e = np.zeros(X.shape[0])
    mag = np.zeros(X.shape[0])
    for j in range(m):
        e += (cw[j] * cw[j]).sum(1) - 2.0 * (X * cw[j]).sum(1)
        mag += (cw[j] * cw[j]).sum(1) + 2.0 * np.abs(X * cw[j]).sum(1)
    for j in range(m - 1):
        e += 2.0 * (cw[j] * cw[j + 1]).sum(1)
        mag += 2.0 * np.abs(cw[j] * cw[j + 1]).sum(1)
    # m unaries (gamma_{2d+2}) and m - 1 pair entries (gamma_d), then 2m - 1 table entries summed: gamma_{2d + 2m + 2} * magnitude
    return e, gamma(2 * d + 2 * m + 2) * mag


def chain_optimum(X, K, m, h=H, chunk=16):
    """Independent float64 min-sum DP over the chain -> (optimal energy (n,), optimal codes (n, m) 0-based)."""
    U, _ = unaries(X, K, m, h)
    T, _ = pair_tables(K, m, h)
    n = U.shape[1]
    best = np.zeros(n)
    codes = np.zeros((n, m), dtype=np.int64)
    for lo in range(0, n, chunk):
        sl = slice(lo, min(n, lo + chunk))
        acc = U[0, sl]
        back = []
        for j in range(1, m):
            tot = acc[:, :, None] + T[j, j - 1][None, :, :]          # [i, b (codebook j-1), a (codebook j)] = acc + 2 <c_{j-1,b}, c_{j,a}>
            arg = tot.argmin(1)
            back.append(arg)
            acc = np.take_along_axis(tot, arg[:, None, :], 1)[:, 0, :] + U[j, sl]
        last = acc.argmin(1)
        best[sl] = acc[np.arange(acc.shape[0]), last]
        codes[sl, m - 1] = last
        for j in range(m - 1, 0, -1):
            last = back[j - 1][np.arange(acc.shape[0]), last]
            codes[sl, j - 1] = last
    return best, codes


def chain_exhaustive_m3(x, K, h=H):
    """The minimum of the chain energy over all h^3 codes of one vector (m = 3), float64 -> (energy, codes)."""
    U, _ = unaries(np.asarray(x)[None, :], K, 3, h)
    T, _ = pair_tables(K, 3, h)
    tot = U[0, 0][:, None, None] + T[1, 0][:, :, None] + U[1, 0][None, :, None] + T[2, 1][None, :, :] + U[2, 0][None, None, :]
    i = int(tot.argmin())
    return float(tot.reshape(-1)[i]), np.unravel_index(i, tot.shape)


def assign_values(X, K, m, dims=None, h=H):
    """Per codebook j the squared distance ||x_s - c_s||^2 over its sub-space s = dims[j] (default: every dimension) to every codeword
    -> (values (m, n, h), bound (m, n, h)).  The kernels return the unary -2 <x, c> + ||c||^2 of codewords that are zero outside s; that plus
    ||x_s||^2 (added in float64) carries the unary's bound."""
    X, K = _f64(X), _f64(K)
    n, d = X.shape
    dims = [slice(0, d)] * m if dims is None else dims
    _, b = unaries(X, K, m, h)
    V = np.empty((m, n, h))
    for j in range(m):
        xs, cs = X[:, dims[j]], K[j * h:(j + 1) * h, dims[j]]
        V[j] = np.maximum((xs * xs).sum(1)[:, None] + (cs * cs).sum(1)[None, :] - 2.0 * xs @ cs.T, 0.0)
    return V, b


# ---- the codebook update -------------------------------------------------------------------------------------------------------------------

def lsq_codebooks(X, codes, m, h=H, cols=None, method="lsqr"):
    """The least-squares codebooks  argmin_K ||X - S K||  (S the n x m h one-hot code matrix) per dimension in float64.
    X (n, d), codes (n, m) 0-based; cols: the dimensions to solve (default all).  method "lsqr": scipy LSQR with atol = btol = 1e-12;
    "normal": the normal equations S'S K = S'X (dense, m h <= 2048), solved by least squares (S'S is singular: shifts between codebooks, unused codes).
    -> (K64 (m h, len(cols)), reconstruction S K (n, len(cols)))."""
    X = _f64(X)
    n, d = X.shape
    cols = np.arange(d) if cols is None else np.asarray(cols)
    codes = np.asarray(codes, dtype=np.int64)
    idx = codes + (np.arange(m) * h)[None, :]
    if method == "normal":
        G = gram(codes, m, h)
        R = np.stack([np.bincount(idx.reshape(-1), weights=np.repeat(X[:, t], m), minlength=m * h) for t in cols], 1)
        Kt = np.linalg.lstsq(G, R, rcond=1e-13)[0]
    else:
        import scipy.sparse as sp
        from scipy.sparse.linalg import lsqr
        S = sp.csr_matrix((np.ones(n * m), (np.repeat(np.arange(n), m), idx.reshape(-1))), shape=(n, m * h))
        Kt = np.stack([lsqr(S, X[:, t], atol=1e-12, btol=1e-12, iter_lim=20000)[0] for t in cols], 1)
    rec = sum(Kt[idx[:, j]] for j in range(m))
    return Kt, rec


def gram(codes, m, h=H):
    """S'S of the one-hot code matrix, dense float64 (m h, m h): pair counts of the codes."""
    codes = np.asarray(codes, dtype=np.int64)
    G = np.zeros((m * h, m * h))
    for i in range(m):
        for j in range(m):
            G[i * h:(i + 1) * h, j * h:(j + 1) * h] = np.bincount(codes[:, i] * h + codes[:, j], minlength=h * h).reshape(h, h)
    return G


def lsqr_stopping_rule(X, codes, m, K, cols, h=H):
    """LSQR's stopping rule ||S'r|| <= atol ||S|| ||r||, evaluated in float64 for the codebooks K with ||S|| <= ||S||_F = sqrt(n m): per dimension
    ||S'r|| / (||S||_F ||r||), r = x - S K.  A solver that stopped on this rule with atol = sqrt(eps_f32) (the reference's tolerance) returns at
    most atol here; codebooks far from the optimum leave a large ||S'r|| and fail it."""
    X = _f64(X)
    n = X.shape[0]
    codes = np.asarray(codes, dtype=np.int64)
    idx = codes + (np.arange(m) * h)[None, :]
    Kc = _f64(K)[:, cols]
    r = X[:, cols] - sum(Kc[idx[:, j]] for j in range(m))
    Str = np.stack([np.bincount(idx.reshape(-1), weights=np.repeat(r[:, c], m), minlength=m * h) for c in range(len(cols))], 1)
    return np.linalg.norm(Str, axis=0) / (np.sqrt(n * m) * np.linalg.norm(r, axis=0))


# ---- comparators ---------------------------------------------------------------------------------------------------------------------------

def check_values(got, ref, bound, what="value"):
    """|got - ref64| <= bound, elementwise."""
    got = np.asarray(got, dtype=np.float64)
    ref, bound = np.broadcast_to(ref, got.shape), np.broadcast_to(bound, got.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0))), got.shape)
        raise AssertionError("%s: %d of %d entries outside the f32 bound; worst at %s: got %r, float64 %r, |diff| %g > bound %g"
                             % (what, int(bad.sum()), got.size, i, got[i], ref[i], err[i], bound[i]))


def check_selection(ids, vals, bound, dists=None, what="selection"):
    """One selection of k = len(ids) items out of vals (N,) float64 with bound (N,) (or a scalar): see the module docstring.
    dists (k,), when given: the returned distances, within their bound of the float64 value of their id, non-decreasing."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    vals = np.asarray(vals, dtype=np.float64)
    N, k = vals.shape[0], ids.shape[0]
    if ids.min() < 0 or ids.max() >= N:
        raise AssertionError("%s: ids out of range 0..%d" % (what, N - 1))
    if np.unique(ids).shape[0] != k:
        raise AssertionError("%s: repeated ids" % what)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), vals.shape)
    t = np.partition(vals, k - 1)[k - 1]                           # the true k-th smallest value
    chosen = np.zeros(N, dtype=bool)
    chosen[ids] = True
    # The kernel returns the k smallest f32 values f, |f - vals| <= bound.  A chosen c above t displaced an unchosen o with vals[o] <= t, and
    # f[c] <= f[o] gives vals[c] <= t + bound[c] + bound[o]; an unchosen o below t was displaced by a chosen c with vals[c] >= t, so
    # vals[o] >= t - bound[o] - bound[c].  The partner's bound is taken as the largest among the items that can be that partner.
    top_out = ~chosen & (vals <= t)
    b_top = float(bound[top_out].max()) if top_out.any() else 0.0
    ch_hi = chosen & (vals >= t)
    b_ch = float(bound[ch_hi].max()) if ch_hi.any() else 0.0
    over = vals[ids] - (t + bound[ids] + b_top)
    if (over > 0).any():
        j = int(np.argmax(over))
        raise AssertionError("%s: chosen item %d has float64 value %r > k-th %r + bound %g + %g" % (what, ids[j], vals[ids[j]], t, bound[ids[j]], b_top))
    under = (t - bound - b_ch - vals)[~chosen]
    if (under > 0).any():
        j = np.nonzero(~chosen)[0][int(np.argmax(under))]
        raise AssertionError("%s: item %d with float64 value %r < k-th %r - bound %g - %g was not chosen" % (what, j, vals[j], t, bound[j], b_ch))
    if dists is not None:
        dists = np.asarray(dists, dtype=np.float64).reshape(-1)
        check_values(dists, vals[ids], bound[ids], what + " (returned distances)")
        if (np.diff(dists) < 0).any():
            raise AssertionError("%s: returned distances decrease" % what)


def check_topk(ids, dists, vals, bound, what="top-k"):
    """Row by row: ids / dists (nq, k), vals / bound (nq, N)."""
    bound = np.broadcast_to(bound, vals.shape)
    for q in range(vals.shape[0]):
        check_selection(ids[q], vals[q], bound[q], None if dists is None else dists[q], "%s, query %d" % (what, q))


def check_argmin(idx, vals, bound, what="argmin"):
    """idx (n,) against vals / bound (n, N), vectorised: check_selection with k = 1 -- the chosen item c is within bound[c] plus the largest
    bound among the row's minimisers of the row's minimum."""
    idx = np.asarray(idx, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.float64)
    bound = np.broadcast_to(bound, vals.shape)
    rows = np.arange(vals.shape[0])
    mn = vals.min(1)
    b_top = np.where(vals <= mn[:, None], bound, 0.0).max(1)
    got = vals[rows, idx]
    bad = got > mn + bound[rows, idx] + b_top
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError("%s: %d of %d rows chose a worse item; row %d chose %d (%r), the minimum is %r, bounds %g + %g"
                             % (what, int(bad.sum()), bad.size, i, idx[i], got[i], mn[i], bound[i, idx[i]], b_top[i]))


def check_chain(X, K, codes, m, h=H, what="chain"):
    """Viterbi codes (n, m) 0-based: their float64 energy is at most the independent DP's optimum plus the f32 bounds of both paths
    (the f32 DP returns a path whose f32 energy is no larger than the f32 energy of the true optimum, rounding being monotone)."""
    e, b = chain_energy(X, K, codes, m, h)
    opt, ocodes = chain_optimum(X, K, m, h)
    _, ob = chain_energy(X, K, ocodes, m, h)
    bad = e > opt + b + ob
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError("%s: %d of %d vectors are not chain optima; vector %d: energy %r, optimum %r, bound %g"
                             % (what, int(bad.sum()), bad.size, i, e[i], opt[i], b[i] + ob[i]))
    return e, opt
