"""Float64 checker of the sparse codebook step (the tests' yardstick, not the product).

The problem (src/codebook_update_sparse.jl, matlab/sparse_lsq_fun.m):

    minimise 0.5 ||A k - b||^2   subject to   ||k||_1 <= tau,      A = I_d (x) S,  b = vec(X'),

with S the n x (m h) code indicator matrix.  Here K is held as the project's [m h][d] matrix, so A k is the
reconstruction matrix R[i][t] = SUM_j K[j h + code_ij][t] and A'r is the per-codeword sum of residual rows.

- `certificate`: the LASSO duality gap.  For a feasible K with residual r = b - A K, y = r is dual feasible up to the
  scaling built into the gap, and f(K) - f* <= gap(K) = r'(r - b) + tau ||A'r||_inf exactly.
- `project_l1`: Euclidean projection onto the l1 ball by sorting (van den Berg & Friedlander's oneProjector).
- `spg`: a plain restatement of SPGL1's single-tau spectral projected gradient (curvilinear nonmonotone search, the
  feasible-direction fallback, Barzilai-Borwein steps), the same rules as csrc/lsq_spgl1.hip.
- `threshold`: keep the S entries largest in |K|, ties to the lower flat index (Julia's sortperm(abs(K[:]), rev=true)).
"""
import numpy as np

try:
    import scipy.sparse as _sp
except ImportError:      # pragma: no cover - the checker works without scipy, only slower
    _sp = None

H = 256


class Problem:
    """X (n, d) f32 data, codes (n, m) 0-based: the operator A and the right-hand side b in float64."""

    def __init__(self, X, codes, m, h=H):
        self.X = np.asarray(X, dtype=np.float64)
        self.codes = np.asarray(codes, dtype=np.int64)
        self.n, self.d = self.X.shape
        self.m, self.h = m, h
        self.cols = self.codes + (np.arange(m, dtype=np.int64) * h)[None, :]
        if _sp is not None:
            rows = np.repeat(np.arange(self.n), m)
            self.S = _sp.csr_matrix((np.ones(self.n * m), (rows, self.cols.ravel())), shape=(self.n, m * h))
            self.St = self.S.T.tocsr()
        else:
            self.S = None

    def A(self, K):
        K = np.asarray(K, dtype=np.float64)
        if self.S is not None:
            return np.asarray(self.S @ K)
        out = np.zeros((self.n, self.d))
        for j in range(self.m):
            out += K[self.cols[:, j]]
        return out

    def At(self, R):
        if self.S is not None:
            return np.asarray(self.St @ R)
        out = np.zeros((self.m * self.h, self.d))
        for j in range(self.m):
            np.add.at(out, self.cols[:, j], R)
        return out

    def dense(self):
        """The explicit n d x (m h d) matrix A, for tiny problems: column (c, t) of K's flat [m h][d] layout."""
        S = np.zeros((self.n, self.m * self.h))
        for j in range(self.m):
            S[np.arange(self.n), self.cols[:, j]] += 1.0
        A = np.zeros((self.n, self.d, self.m * self.h, self.d))
        for t in range(self.d):
            A[:, t, :, t] = S
        return A.reshape(self.n * self.d, self.m * self.h * self.d)


def certificate(P, K, tau):
    """-> dict(f, gap, rel_gap, gnorm, l1, rnorm, bnorm) of K (any dtype, evaluated in float64)."""
    K = np.asarray(K, dtype=np.float64)
    r = P.X - P.A(K)
    f = 0.5 * float(np.sum(r * r))
    gnorm = float(np.max(np.abs(P.At(r)))) if r.size else 0.0
    gap = float(np.sum(r * (r - P.X))) + tau * gnorm
    return dict(f=f, gap=gap, rel_gap=abs(gap) / max(1.0, f), gnorm=gnorm, l1=float(np.sum(np.abs(K))),
                rnorm=float(np.sqrt(2 * f)), bnorm=float(np.sqrt(np.sum(P.X * P.X))))


def rounding_allowance(P, K32, tau):
    """Bound on |gap(x) - gap(fl32(x))| for any x that rounds to K32, plus the float64 error of evaluating the gap.

    |x - K32| <= u |K32| + 2^-149 elementwise (u = 2^-24, round to nearest).  With D that bound and dr = A (x - K32):
      |(2r - b)'dr| <= |A'(2r - b)|' D,  ||dr||^2 <= ||A D||^2,  tau | ||A'(r + dr)||_inf - ||A'r||_inf | <= tau ||A'A D||_inf
    (A is non-negative).  The evaluation itself: n d m terms of size ||b||^2-ish, each with a relative error of a few eps."""
    K = np.asarray(K32, dtype=np.float64)
    D = np.abs(K) * 2.0 ** -24 + 2.0 ** -149
    r = P.X - P.A(K)
    AD = P.A(D)
    term = float(np.sum(np.abs(P.At(2 * r - P.X)) * D)) + float(np.sum(AD * AD)) + tau * float(np.max(P.At(AD)))
    scale = float(np.sum(P.X * P.X)) + float(np.sum(r * r)) + tau * float(np.max(np.abs(P.At(r))))
    return term + 64 * np.finfo(np.float64).eps * (P.m + 2) * scale


def project_l1(v, tau):
    """Euclidean projection of v onto {x : ||x||_1 <= tau} (sort-based, SPGL1's oneProjector)."""
    v = np.asarray(v, dtype=np.float64)
    if tau <= 0:
        return np.zeros_like(v)
    a = np.abs(v).ravel()
    if a.sum() <= tau:
        return v.copy()
    u = np.sort(a)[::-1]
    cs = np.cumsum(u)
    k = np.arange(1, u.size + 1)
    ok = u > (cs - tau) / k
    kstar = int(np.nonzero(ok)[0].max()) + 1
    theta = (cs[kstar - 1] - tau) / kstar
    return np.sign(v) * np.maximum(np.abs(v) - theta, 0.0)


OPTIMAL, ITERATIONS, LINE_ERROR = 0, 1, 2


def spg(P, tau, K0=None, opt_tol=1e-4, max_iter=None, n_prev=3, step_min=1e-16, step_max=1e5, max_line_errors=10):
    """SPGL1's LASSO mode in float64.  -> (K [m h][d] float64, info dict)."""
    b = P.X
    project = lambda v: project_l1(v, tau)
    x = project(np.zeros((P.m * P.h, P.d)) if K0 is None else np.asarray(K0, dtype=np.float64))
    if max_iter is None:
        max_iter = 10 * P.n * P.d
    r = b - P.A(x)
    g = -P.At(r)
    f = 0.5 * float(np.sum(r * r))
    bnorm = float(np.sqrt(np.sum(b * b)))
    last = [-np.inf] * n_prev
    last[0] = f
    f_best, x_best = f, x.copy()
    dxn = float(np.max(np.abs(project(x - g) - x))) if x.size else 0.0
    g_step = step_max if dxn < 1.0 / step_max else min(step_max, max(step_min, 1.0 / dxn))
    it = trials = 0
    stat = None
    while True:
        gnorm = float(np.max(np.abs(g)))
        rnorm = float(np.sqrt(np.sum(r * r)))
        gap = float(np.sum(r * (r - b))) + tau * gnorm
        rgap = abs(gap) / max(1.0, f)
        if rgap <= opt_tol or rnorm < opt_tol * bnorm:
            stat = OPTIMAL
        elif it >= max_iter:
            stat = ITERATIONS
        if stat is not None:
            break
        it += 1
        x_old, f_old, g_old = x, f, g
        fmax = max(last)
        # spgLineCurvy
        step, scale, s_norm, n_safe, k, err = 1.0, 1.0, 0.0, 0, 0, None
        G = g_step * g
        while True:
            trials += 1
            xn = project(x - step * scale * G)
            rn = b - P.A(xn)
            fn = 0.5 * float(np.sum(rn * rn))
            s = xn - x
            gts = scale * float(np.sum(G * s))
            if gts >= 0:
                err = 2
                break
            if fn < fmax + 1e-4 * step * gts:
                err = 0
                break
            if k >= 10:
                err = 1
                break
            k += 1
            step /= 2
            s_old, s_norm = s_norm, float(np.sqrt(np.sum(s * s))) / np.sqrt(s.size)
            if abs(s_norm - s_old) <= 1e-6 * s_norm:
                gn = float(np.sqrt(np.sum(G * G))) / np.sqrt(G.size)
                scale = s_norm / gn / (2.0 ** n_safe)
                n_safe += 1
        if err:
            # spgLine: feasible direction
            dx = project(x - g_step * g) - x
            gtd = -abs(float(np.sum(g * dx)))
            step, k = 1.0, 0
            while True:
                trials += 1
                xn = x + step * dx
                rn = b - P.A(xn)
                fn = 0.5 * float(np.sum(rn * rn))
                if fn < fmax + 1e-4 * step * gtd:
                    err = 0
                    break
                if k >= 10:
                    err = 1
                    break
                k += 1
                if step <= 0.1:
                    step /= 2
                else:
                    tmp = (-gtd * step * step) / (2 * (fn - f - step * gtd))
                    if not (tmp >= 0.1 and tmp <= 0.9 * step):
                        tmp = step / 2
                    step = tmp
        if err:
            x, f = x_old, f_old
            if max_line_errors <= 0:
                stat = LINE_ERROR
                break
            step_max /= 10
            max_line_errors -= 1
            g_step = min(step_max, g_step)
        else:
            x, r, f = xn, rn, fn
            g = -P.At(r)
            s = x - x_old
            y = g - g_old
            sts, sty = float(np.sum(s * s)), float(np.sum(s * y))
            g_step = step_max if sty <= 0 else min(step_max, max(step_min, sts / sty))
        last[it % n_prev] = f
        if f < f_best:
            f_best, x_best = f, x.copy()
    if stat != OPTIMAL and f > f_best:
        x = x_best
    c = certificate(P, x, tau)
    return x, dict(status=stat, iterations=it, line_search_trials=trials, **c)


def threshold(K, S):
    """Keep the S entries of K largest in |K| (ties: lower flat index first), +0.0 elsewhere.  S < 0: unchanged."""
    K = np.array(K, dtype=np.float32, copy=True)
    if S < 0:
        return K
    flat = K.ravel()
    order = np.lexsort((np.arange(flat.size), -np.abs(flat).astype(np.float64)))
    flat[order[S:]] = np.float32(0.0)
    return flat.reshape(K.shape)
