"""Initialisers of the LSQ training pipeline: PQ, OPQ and ChainQ.

Mirrors of the reference's trainers with the reference's names, argument order and Julia shapes, so that
`demos/demo_lsq_gpu.jl` reads the same against this package:

    C, B, R, err = train_opq(x_train, m, h, niter, "natural")        # src/opq/OPQ.jl:21-101
    C, B, R, err = train_chainq(x_train, m, h, R, B, C, niter)       # src/chainq/chainq.jl:10-58
    C, B, cbnorms, B_norms, obj = train_lsq(x_train, m, h, R, B, C, ...)   # reference_api.train_lsq (GPU encoder)

The two data-parallel steps run ON THE DEVICE through the C-ABI (csrc/lsq_init.hip; round 6): the nearest-codeword assignment of PQ / OPQ and of
their k-means (`lsq_assign_codewords`: every sub-space of a vector set in one call, codebooks padded to d rows) and ChainQ's Viterbi encoder
(`lsq_encode_viterbi`).  Like the rest of the engine they need h == 256 and a gfx950 device -- there is no CPU fallback; the numpy restatement of
these steps lives in oracle/init_oracle.py as the checker (tests only).  What stays on the host in train_pq / train_opq is the glue around them: k-means++
seeding, cluster means, the Procrustes SVD, and the scalar k-means of the norm codebook (an O(n log h) sorted search).  kmeans_dev / train_pq_dev /
train_opq_dev are the resident forms: seeding and cluster means on the device too (lsq_kmeanspp_seed_dev, lsq_update_centers_dev: csrc/lsq_kmeans.hip), X,
codes and codebooks in HBM throughout; only the d x d Procrustes SVD stays on the host.  The chain's structured LSQR codebook update runs
by default in scipy (float64, a Python loop over the dimensions: the checker's own path); `solver="host"` selects the C-ABI host solver
(lsq_update_codebooks_struct) and `engine=<Engine>` the device solver (lsq_update_codebooks_struct_gpu / _dev), which train_chainq_dev uses with X,
codes and codebooks resident in HBM.
PARITY UNPINNED: the reference delegates to Clustering.jl k-means, StatsBase sampling and IterativeSolvers LSQR,
none vendored or version-pinned, and has no tests for them; what is mirrored is the algorithm and the interfaces.
Shapes follow Julia: X is d x n, codes B are m x n Int16 **1-based**, codebooks are lists of (rows x h) matrices.
"""
import numpy as np

from .engine import splitarray

__all__ = ["train_pq", "quantize_pq", "qerror_pq", "train_opq", "quantize_opq", "get_cbdims_chain", "update_codebooks_generic",
           "update_codebooks_chain", "encoding_viterbi", "train_chainq", "train_chainq_dev", "kmeans", "kmeans_dev", "train_pq_dev", "train_opq_dev",
           "codebooks_from_padded"]


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _eng(engine=None):
    """The C-ABI context the device steps run on (the package's default one unless the caller brings its own)."""
    if engine is not None:
        return engine
    from .reference_api import default_engine
    return default_engine()


def _subdims(d, m):
    """splitarray(1:d, m) as 0-based slices (src/utils.jl:152-177)."""
    return [slice(lo, hi) for lo, hi in splitarray(d, m)]


def _assign_scalar(c, x):
    """r = 1 (the norm codebook of train_lsq: n scalars, h centres): argmin_k (x - c_k)^2 evaluated in f32, lowest index on ties -- the result of the
    brute-force h x n scan, in O(n log h): the f32 distance is monotone in |x - c_k|, so the minimisers form a contiguous run of the SORTED centres
    around x; the run is found from the two neighbours of x and widened while the distance stays equal.  (The pairwise expansion of _sqdist
    cancels catastrophically for scalars of the size of squared norms; this is also the better-conditioned formula.)
    Behaviour note: EVERY width-1 k-means goes through here, i.e. also a PQ / OPQ sub-space of width 1 (d == m) -- its assignments are those of
    (x - c)^2, which can differ from the expanded-distance scan of wider sub-spaces on near-ties; the reference (Clustering.jl) is unpinned either way."""
    c = np.asarray(c, dtype=np.float32).reshape(-1)
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    h, n = c.shape[0], x.shape[0]
    order = np.argsort(c, kind="stable")
    cs = c[order]
    pos = np.searchsorted(cs, x)                                   # cs[pos - 1] < x <= cs[pos]
    L = np.clip(pos - 1, 0, h - 1)
    R = np.clip(pos, 0, h - 1)
    dL = (x - cs[L]) ** 2
    dR = (x - cs[R]) ** 2
    best = np.minimum(dL, dR)
    lo = np.where(dL <= dR, L, R)                                  # one member of the run of minimisers
    hi = lo.copy()
    idx = order[lo].copy()                                         # lowest ORIGINAL index seen in the run so far
    other = np.where(dL <= dR, R, L)
    tie = (dL == dR) & (L != R)
    idx[tie] = np.minimum(idx[tie], order[other[tie]])
    lo = np.where(tie, np.minimum(lo, other), lo)
    hi = np.where(tie, np.maximum(hi, other), hi)
    live = np.arange(n)
    while live.size:                                               # widen the run while the next centre on either side is exactly as far (duplicates, rounding)
        l2, h2 = lo[live] - 1, hi[live] + 1
        okl = l2 >= 0
        okh = h2 < h
        el = np.zeros(live.size, dtype=bool)
        eh = np.zeros(live.size, dtype=bool)
        el[okl] = (x[live[okl]] - cs[l2[okl]]) ** 2 == best[live[okl]]
        eh[okh] = (x[live[okh]] - cs[h2[okh]]) ** 2 == best[live[okh]]
        if el.any():
            t = live[el]
            lo[t] -= 1
            idx[t] = np.minimum(idx[t], order[lo[t]])
        if eh.any():
            t = live[eh]
            hi[t] += 1
            idx[t] = np.minimum(idx[t], order[hi[t]])
        live = live[el | eh]
    return idx.astype(np.int64), best.astype(np.float32)


def _assign(C, X, engine=None):
    """Nearest codeword per column of X (r x n) among the columns of C (r x h), lowest index on ties (update_assignments!, src/opq/kmeans.jl:6-75)
    -> (assignments (n,) 0-based, squared distances (n,) f32).  r >= 2: on the device (lsq_assign_codewords, h == 256)."""
    if X.shape[0] == 1:
        return _assign_scalar(C, X)
    Xr = np.ascontiguousarray(_f32(X).T)
    B, mv = _eng(engine).assign_codewords(Xr, np.ascontiguousarray(_f32(C).T), 1, h=C.shape[1], want_min=True)
    return B[:, 0].astype(np.int64) - 1, np.maximum(mv[:, 0] + np.einsum("ij,ij->i", Xr, Xr), 0.0).astype(np.float32)


def _assign_subspaces(C, X, sd, engine=None):
    """All m sub-spaces of the vector set in ONE device call: codebook i padded to the d rows of X, zero outside sd[i] (quantize_pq, src/pq/PQ.jl:12-41;
    OPQ's assignment step, src/opq/OPQ.jl:60-66,88-91) -> B (m, n) int64 0-based."""
    X = _f32(X)
    d, m, h = X.shape[0], len(C), C[0].shape[1]
    K = np.zeros((m * h, d), dtype=np.float32)
    for i in range(m):
        K[i * h:(i + 1) * h, sd[i]] = _f32(C[i]).T
    B = _eng(engine).assign_codewords(np.ascontiguousarray(X.T), K, m, h=h)
    return B.T.astype(np.int64) - 1


def _centers(X, a, h, rng, old=None):
    """Cluster means (update_centers!, src/opq/kmeans.jl:77-123); an empty cluster is re-seeded with a random point."""
    r, n = X.shape
    C = np.zeros((r, h), dtype=np.float32)
    cnt = np.bincount(a, minlength=h)
    nz = cnt > 0
    if r == 1:                                           # n scalars (the norm codebook): one weighted bincount, sums in f64
        C[0] = np.bincount(a, weights=X[0].astype(np.float64), minlength=h).astype(np.float64)[:h] / np.maximum(cnt, 1)
    else:
        np.add.at(C.T, a, X.T)
        C[:, nz] /= cnt[nz]
    for k in np.nonzero(~nz)[0]:
        C[:, k] = X[:, rng.integers(n)] if old is None else old[:, k]
    return C


def kmeans(X, h, niter=25, seed=0, engine=None, init=None):
    """Lloyd k-means with k-means++ seeding on the columns of X (r x n) -> centers (r x h), assignments (n,) 0-based, total cost.
    Stands in for Clustering.jl's `kmeans(X, h, init=:kmpp)` (src/pq/PQ.jl:60).  init: explicit initial centers (r x h); the seeding is skipped."""
    X = _f32(X)
    r, n = X.shape
    rng = np.random.default_rng(seed)
    if init is not None:
        C = _f32(init).copy()
        if C.shape != (r, h):
            raise ValueError("init must be (r, h) = (%d, %d), got %s" % (r, h, C.shape))
    else:
        C = np.empty((r, h), dtype=np.float32)
        C[:, 0] = X[:, rng.integers(n)]
        d2 = ((X - C[:, :1]) ** 2).sum(axis=0)
        for k in range(1, h):
            tot = float(d2.sum())
            idx = rng.integers(n) if tot <= 0 else int(np.searchsorted(np.cumsum(d2), rng.random() * tot))
            C[:, k] = X[:, min(idx, n - 1)]
            d2 = np.minimum(d2, ((X - C[:, k:k + 1]) ** 2).sum(axis=0))
    a, cost = _assign(C, X, engine)
    for _ in range(niter):
        C = _centers(X, a, h, rng)
        a2, cost = _assign(C, X, engine)
        if np.array_equal(a2, a):
            break
        a = a2
    return C, a, float(cost.sum())


# ---- PQ (src/pq/PQ.jl) ---------------------------------------------------------------------------------------
def quantize_pq(X, C, V=False, *, engine=None):
    """quantize_pq(X, C) -> B (m x n Int16, 1-based).  src/pq/PQ.jl:12-41 -- one device call for all sub-spaces."""
    X = _f32(X)
    sd = _subdims(X.shape[0], len(C))
    if any(s_.stop - s_.start < 2 for s_ in sd):          # width-1 sub-spaces (d == m): the scalar search, as in kmeans()
        return np.stack([_assign(_f32(C[i]), X[sd[i]], engine)[0] + 1 for i in range(len(C))]).astype(np.int16)
    return (_assign_subspaces(C, X, sd, engine) + 1).astype(np.int16)


def qerror_pq(X, B, C):
    """Mean squared reconstruction error of PQ codes (codebooks hold sub-vectors)."""
    X = _f32(X)
    sd = _subdims(X.shape[0], len(C))
    err = 0.0
    for i in range(len(C)):
        err += float(((X[sd[i]] - _f32(C[i])[:, np.asarray(B[i], dtype=np.int64) - 1]) ** 2).sum())
    return err / X.shape[1]


def train_pq(X, m, h, V=False, *, seed=0, engine=None, init=None):
    """train_pq(X, m, h) -> C, B, error.  src/pq/PQ.jl:44-76 (k-means per subspace).  init: m explicit initial codebooks (subdim x h); no seeding then."""
    X = _f32(X)
    sd = _subdims(X.shape[0], m)
    C, B = [], []
    for i in range(m):
        c, a, cost = kmeans(X[sd[i]], h, seed=seed + i, engine=engine, init=None if init is None else init[i])
        C.append(c)
        B.append(a + 1)
        if V:
            print("codebook %d / %d: error in subspace %e" % (i + 1, m, cost / X.shape[1]))
    B = np.stack(B).astype(np.int16)
    return C, B, qerror_pq(X, B, C)


# ---- OPQ (src/opq/OPQ.jl) ------------------------------------------------------------------------------------
def quantize_opq(X, R, C, V=False, *, engine=None):
    """quantize_opq(X, R, C) = quantize_pq(R'X, C).  src/opq/OPQ.jl:10-19"""
    return quantize_pq(_f32(R).T @ _f32(X), C, V, engine=engine)


def _procrustes(X, CB):
    """R = U V' with U S V' = svd(X CB')  (src/opq/OPQ.jl:78-79, src/chainq/chainq.jl:44-45)."""
    U, _, Vt = np.linalg.svd(X.astype(np.float64) @ CB.astype(np.float64).T, full_matrices=False)
    return (U @ Vt).astype(np.float32)


def train_opq(X, m, h, niter, init="natural", V=False, *, seed=0, engine=None):
    """train_opq(X, m, h, niter, init) -> C, B, R, obj.  src/opq/OPQ.jl:21-101
    C[i]: (subdim x h) codebooks of the rotated space, B: m x n Int16 1-based, R: d x d, obj: niter+1 errors."""
    X = _f32(X)
    d, n = X.shape
    rng = np.random.default_rng(seed)
    if init == "natural":
        R = np.eye(d, dtype=np.float32)
    elif init == "random":
        R = np.linalg.svd(rng.standard_normal((d, d)))[0].astype(np.float32)
    else:
        raise ValueError("Intialization %s unknown" % init)
    RX = R.T @ X
    sd = _subdims(d, m)
    C = [RX[sd[i]][:, rng.choice(n, h, replace=False)].copy() for i in range(m)]     # :46-50
    wide = all(s_.stop - s_.start >= 2 for s_ in sd)

    def assign_all(RX_):
        if wide:
            return _assign_subspaces(C, RX_, sd, engine)
        return np.stack([_assign(C[i], RX_[sd[i]], engine)[0] for i in range(m)])

    CB = np.zeros_like(X)
    B = assign_all(RX)
    for i in range(m):
        CB[sd[i]] = C[i][:, B[i]]
    obj = np.zeros(niter + 1, dtype=np.float32)
    for it in range(niter + 1):
        obj[it] = float(((R @ CB - X) ** 2).sum()) / n
        if V:
            print("%3d %e" % (it, obj[it]))
        R = _procrustes(X, CB)
        RX = R.T @ X
        for i in range(m):                                   # update C (:85-86); the sub-spaces are independent, so all centres first ...
            C[i] = _centers(RX[sd[i]], B[i], h, rng, old=C[i])
        B = assign_all(RX)                                   # ... then update B for every sub-space in one device call (:88-91)
        for i in range(m):
            CB[sd[i]] = C[i][:, B[i]]
    return C, (B + 1).astype(np.int16), R, obj


# ---- ChainQ (src/chainq/chainq.jl, src/encodings/encode_chain.jl, src/codebook_update.jl:88-169) -------------------
def get_cbdims_chain(d, m):
    """Dimensions each codebook of a chain covers: consecutive codebooks overlap on one of the m-1 blocks.
    src/codebook_update.jl:88-102.  Returns m 0-based slices.  A chain needs m >= 2 codebooks and one dimension per block, d >= m - 1."""
    if m < 2 or d < m - 1:
        from ._lib import LSQ_EINVAL, LsqError
        raise LsqError(LSQ_EINVAL, "get_cbdims_chain: a chain needs m >= 2 and d >= m - 1, got d=%d m=%d" % (d, m))
    sub = splitarray(d, m - 1)
    od = [slice(sub[0][0], sub[0][1])]
    for i in range(1, m - 1):
        od.append(slice(sub[i - 1][0], sub[i][1]))
    od.append(slice(sub[-1][0], sub[-1][1]))
    return od


def _cover_map(odims, d, m):
    """dim2C of the reference (codebook_update.jl:134-136): (d, m) uint8, 1 where codebook i covers dimension t.  odims: per codebook a slice or an index list."""
    dim2C = np.zeros((d, m), dtype=np.uint8)
    for i in range(m):
        dim2C[odims[i], i] = 1
    return dim2C


def update_codebooks_generic(X, B, h, odimsfunc, V=False, *, nthreads=0, engine=None, solver=None):
    """Least-squares codebooks under a dimension structure: odimsfunc(d, m) says which dimensions each codebook has, and for every dimension t only
    the codebooks that cover t are fitted (LSQR on the corresponding columns of the one-hot code matrix); the others stay zero there.
    src/codebook_update.jl:104-158.  Three solvers of the same systems (atol = btol = sqrt(eps_f32), conlim = 1e8):
      solver=None, engine=None   scipy's LSQR in float64, a Python loop over the dimensions (the default);
      solver="host"              the C-ABI host solver, f32 LSQR on `nthreads` cores (lsq_update_codebooks_struct);
      engine=<Engine>            the device solver, all dimensions at once (lsq_update_codebooks_struct_gpu)."""
    if solver not in (None, "host"):
        raise ValueError("solver must be None or 'host', got %r" % (solver,))
    X = _f32(X)
    d, n = X.shape
    m = np.shape(B)[0]
    od = odimsfunc(d, m)
    if solver == "host" or engine is not None:
        from . import _lib
        Xr = np.ascontiguousarray(X.T)
        Br = np.ascontiguousarray(np.asarray(B, dtype=np.int16).T)
        dim2C = _cover_map(od, d, m)
        if solver == "host":
            K = np.empty((m * h, d), dtype=np.float32)
            cover = np.ascontiguousarray(dim2C.T)
            _lib.check(_lib.load().lsq_update_codebooks_struct(Xr.ctypes.data, Br.ctypes.data, cover.ctypes.data, d, n, m, h, int(nthreads), K.ctypes.data))
        else:
            K, _ = engine.update_codebooks_struct(Xr, Br, dim2C, m, h=h)
        return [np.ascontiguousarray(K[i * h:(i + 1) * h].T) for i in range(m)]
    from scipy.sparse import csr_matrix
    from scipy.sparse.linalg import lsqr
    B = np.asarray(B, dtype=np.int64)
    covers = _cover_map(od, d, m)
    cols = (B - 1 + (np.arange(m) * h)[:, None]).T.reshape(-1)                     # sparsify_codes, src/utils.jl:50-69
    S = csr_matrix((np.ones(n * m, dtype=np.float32), (np.repeat(np.arange(n), m), cols)), shape=(n, m * h)).tocsc()
    K = np.zeros((d, m * h), dtype=np.float32)
    tol = float(np.sqrt(np.finfo(np.float32).eps))
    cache = {}
    for t in range(d):
        cbs = tuple(int(i) for i in np.nonzero(covers[t])[0])
        if not cbs:
            continue
        if cbs not in cache:
            idx = np.concatenate([np.arange(i * h, (i + 1) * h) for i in cbs])
            cache[cbs] = (idx, S[:, idx])
        idx, St = cache[cbs]
        K[t, idx] = lsqr(St, X[t].astype(np.float64), atol=tol, btol=tol, conlim=1e8)[0].astype(np.float32)
    return [np.ascontiguousarray(K[:, i * h:(i + 1) * h]) for i in range(m)]


def update_codebooks_chain(X, B, h, V=False, *, nthreads=0, engine=None, solver=None):
    """update_codebooks_generic with the chain's structure (get_cbdims_chain).  src/codebook_update.jl:160-169"""
    return update_codebooks_generic(X, B, h, get_cbdims_chain, V, nthreads=nthreads, engine=engine, solver=solver)


def encoding_viterbi(X, C, V=False, *, engine=None):
    """Exact MAP codes of a chain (unaries + binaries between consecutive codebooks only) by dynamic programming ON THE DEVICE
    (lsq_encode_viterbi, csrc/lsq_init.hip).  src/encodings/encode_chain.jl:1-123; min / argmin take the lowest index on ties as the reference's scans do."""
    X = _f32(X)
    m, h = len(C), np.asarray(C[0]).shape[1]
    K = np.ascontiguousarray(np.concatenate([_f32(c).T for c in C], axis=0))          # hcat(C...) as (m h, d)
    return np.ascontiguousarray(_eng(engine).encode_viterbi(np.ascontiguousarray(X.T), K, m, h=h).T)


def _qerror_full(X, B, C):
    rec = np.zeros_like(X)
    for i in range(len(C)):
        rec += C[i][:, np.asarray(B[i], dtype=np.int64) - 1]
    return float(((X - rec) ** 2).sum()) / X.shape[1]


def train_chainq(X, m, h, R, B, C, niter, V=False, *, engine=None, device_update=False):
    """train_chainq(X, m, h, R, B, C, niter) -> C, B, R, obj.  src/chainq/chainq.jl:10-58
    B: initial codes (e.g. OPQ's); the incoming C is only a placeholder, as in the reference (re-fitted at :27).
    device_update: the structured LSQR codebook update on the device too (needs `engine`), as train_lsq's keyword."""
    X = _f32(X)
    R = _f32(R)
    B = np.asarray(B, dtype=np.int16)
    RX = R.T @ X
    if device_update and engine is None:
        raise ValueError("device_update=True needs engine=<Engine>")
    upd = {"engine": engine} if device_update else {}           # default: update_codebooks_chain(X, B, h, V), the scipy path
    C = update_codebooks_chain(RX, B, h, V, **upd)                     # :27
    B = encoding_viterbi(RX, C, V, engine=engine)                # :31
    obj = np.zeros(niter + 1, dtype=np.float32)
    for it in range(niter + 1):
        obj[it] = _qerror_full(RX, B, C)
        if V:
            print("%3d %e" % (it, obj[it]))
        CB = np.zeros_like(X)
        for i in range(m):
            CB += C[i][:, B[i].astype(np.int64) - 1]
        R = _procrustes(X, CB)                                   # :44-45
        RX = R.T @ X
        C = update_codebooks_chain(RX, B, h, V, **upd)
        B = encoding_viterbi(RX, C, V, engine=engine)
    return C, B, R, obj


def train_chainq_dev(dX, m, h, R, dB, niter, *, engine):
    """src/chainq/chainq.jl:10-58 with X, the codes and the codebooks resident in HBM: the structured LSQR codebook update (lsq_update_codebooks_struct_dev)
    and the Viterbi encode (lsq_encode_viterbi_dev) on device tensors.  dX (n, d) f32, dB (n, m) uint8 0-BASED: CUDA/HIP torch tensors; R (d, d) host.
    -> (dK (m*h, d) tensor: the codebooks of the rotated space, zero outside the chain's dimensions; dB (n, m) uint8 tensor; R (d, d) f32 host; obj (niter + 1,) f32).
    torch is the glue around the two steps, on the device: the rotation R'X, the reconstruction, the objective and the d x d product X CB' (float64).  Per
    iteration only that d x d matrix, R and the scalar objective cross to the host, where the Procrustes SVD runs in float64 as in train_chainq."""
    import torch
    n, d = dX.shape
    dev = dX.device
    dcover = torch.from_numpy(_cover_map(get_cbdims_chain(d, m), d, m)).to(dev)
    offs = (torch.arange(m, device=dev, dtype=torch.int64) * h)[None, :]
    dX64 = None

    def rotate(Rm):
        return (dX @ torch.as_tensor(np.ascontiguousarray(Rm, dtype=np.float32), device=dev)).contiguous()       # rows of (R'X)'

    R = _f32(R)
    dXr = rotate(R)
    dB = dB.contiguous()
    dK, _ = engine.update_codebooks_struct_dev(dXr, dB, dcover, m, h=h)          # :27
    dB = engine.encode_viterbi_dev(dXr, dK, m, h=h)                               # :31
    obj = np.zeros(niter + 1, dtype=np.float32)
    for it in range(niter + 1):
        dCB = dK[dB.to(torch.int64) + offs].sum(dim=1)                            # (n, d): the reconstructions
        obj[it] = float(((dXr - dCB).double() ** 2).sum().item()) / n
        if dX64 is None:
            dX64 = dX.double()
        M = (dX64.T @ dCB.double()).cpu().numpy()                                 # X CB' (d x d), float64
        U, _, Vt = np.linalg.svd(M, full_matrices=False)                          # :44-45
        R = (U @ Vt).astype(np.float32)
        dXr = rotate(R)
        dK, _ = engine.update_codebooks_struct_dev(dXr, dB, dcover, m, h=h, out=dK)
        dB = engine.encode_viterbi_dev(dXr, dK, m, h=h)
    return dK, dB, R, obj


# ---- PQ / OPQ resident on the device (csrc/lsq_kmeans.hip) -----------------------------------------------------------------------------
def codebooks_from_padded(K, d, m):
    """The padded (m h, d) codebook layout of the resident trainers (array or tensor) -> the list of (subdim x h) codebooks train_pq / train_opq return."""
    if hasattr(K, "detach"):
        K = K.detach().cpu().numpy()
    K = _f32(K)
    h = K.shape[0] // m
    if K.shape != (m * h, d):
        raise ValueError("K must be (m*h, d) with d = %d, got %s" % (d, K.shape))
    sd = _subdims(d, m)
    return [np.ascontiguousarray(K[i * h:(i + 1) * h, sd[i]].T) for i in range(m)]


def _padded(C, d, m, h):
    """list of (subdim x h) codebooks, or an (m h, d) array -> (m h, d) f32, zero outside each sub-space"""
    if isinstance(C, (list, tuple)):
        sd = _subdims(d, m)
        K = np.zeros((m * h, d), dtype=np.float32)
        for i in range(m):
            K[i * h:(i + 1) * h, sd[i]] = _f32(C[i]).T
        return K
    K = _f32(C)
    if K.shape != (m * h, d):
        raise ValueError("initial codebooks must be (m*h, d) = (%d, %d), got %s" % (m * h, d, K.shape))
    return K


def _check_wide(cover, what):
    if cover.sum(axis=0).min() < 2:
        raise ValueError("%s: a sub-space of width < 2 (d == m) is not served on the device; use the host trainers (train_pq / train_opq / kmeans) there" % what)


def kmeans_dev(dX, h, niter=25, seed=0, *, engine, dim2C=None, init=None):
    """Lloyd k-means of all sub-spaces of a device tensor in lock-step: dX (n, d) f32 CUDA/HIP tensor, dim2C (d, m) 0/1 host array (None: plain k-means,
    m = 1) -> (dK (m*h, d) tensor, zero outside each sub-space; dB (n, m) uint8 0-based tensor; total cost).
    Seeding by lsq_kmeanspp_seed_dev with u = default_rng(seed).random((m, h)), or the given `init` codebooks ((m*h, d) array or tensor); assignment by
    lsq_assign_codewords_dev; means by lsq_update_centers_dev.  A sub-space whose codes did not change has converged and is frozen (centres, codes, no more
    re-seeds): the state the host kmeans() leaves at its `break`.  An empty cluster is re-seeded with a random data row drawn from default_rng(seed + j) for
    sub-space j in ascending cluster order, as kmeans() of train_pq's i-th sub-space does; the counts cross the bus only when some cluster is empty."""
    import torch
    n, d = dX.shape
    dev = dX.device
    cover = np.ones((d, 1), dtype=np.uint8) if dim2C is None else np.ascontiguousarray(np.asarray(dim2C).astype(np.uint8))
    if cover.ndim != 2 or cover.shape[0] != d:
        raise ValueError("dim2C must be (d, m) with d = %d, got %s" % (d, cover.shape))
    m = cover.shape[1]
    _check_wide(cover, "kmeans_dev")
    if n < 1:
        raise ValueError("kmeans_dev: no data")
    if init is None:
        u = np.random.default_rng(seed).random((m, h))
        dK, _, _ = engine.kmeanspp_seed_dev(dX, cover, u, m, h=h, want_idx=False)
    elif hasattr(init, "detach"):
        dK = init.detach().to(device=dev, dtype=torch.float32).clone().contiguous()
        if tuple(dK.shape) != (m * h, d):
            raise ValueError("init must be (m*h, d) = (%d, %d), got %s" % (m * h, d, tuple(dK.shape)))
    else:
        dK = torch.from_numpy(_padded(init, d, m, h).copy()).to(dev)
    dims = [torch.from_numpy(np.nonzero(cover[:, j])[0]).to(dev) for j in range(m)]
    rngs = [np.random.default_rng(seed + j) for j in range(m)]
    dB, dmin = engine.assign_codewords_dev(dX, dK, m, h=h, want_min=True)
    active = np.ones(m, dtype=bool)
    dKn = torch.empty_like(dK)
    dcnt = torch.empty(m * h, dtype=torch.int32, device=dev)
    for _ in range(niter):
        engine.update_centers_dev(dX, dB, cover, m, h=h, out=dKn, counts=dcnt)
        nempty = (dcnt.view(m, h) == 0).sum(dim=1).cpu().numpy()
        cnt = dcnt.view(m, h).cpu().numpy() if nempty[active].any() else None
        for j in np.nonzero(active)[0]:
            dK[j * h:(j + 1) * h] = dKn[j * h:(j + 1) * h]
            if cnt is not None and nempty[j]:
                ks = np.nonzero(cnt[j] == 0)[0]
                rows = torch.as_tensor(np.array([rngs[j].integers(n) for _k in ks], dtype=np.int64), device=dev)
                dK[(torch.as_tensor(ks + j * h, device=dev))[:, None], dims[j][None, :]] = dX[rows[:, None], dims[j][None, :]]
        dB2, dmin = engine.assign_codewords_dev(dX, dK, m, h=h, want_min=True)
        changed = (dB2 != dB).any(dim=0).cpu().numpy()
        dB = dB2                                                 # a frozen sub-space's centres did not move: its codes are the same bits
        active &= changed
        if not active.any():
            break
    xsq = (dX.double() ** 2) @ torch.from_numpy(cover.astype(np.float64)).to(dev)      # (n, m): ||x_sub||^2
    cost = float((dmin.double() + xsq).clamp_min(0).sum().item())
    return dK, dB, cost


def train_pq_dev(dX, m, h, *, seed=0, engine, init=None):
    """train_pq on a device tensor (src/pq/PQ.jl:44-76): dX (n, d) f32 -> (dK (m*h, d) padded codebooks, dB (n, m) uint8 0-based, error).
    init: m explicit initial codebooks (a list of (subdim x h), as train_pq's, or the padded (m*h, d) layout); no seeding then."""
    import torch
    n, d = dX.shape
    if d < m:
        raise ValueError("train_pq_dev: d = %d < m = %d" % (d, m))
    cover = _cover_map(_subdims(d, m), d, m)
    _check_wide(cover, "train_pq_dev")
    if init is not None and not hasattr(init, "detach"):
        init = _padded(init, d, m, h)
    dK, dB, _ = kmeans_dev(dX, h, seed=seed, engine=engine, dim2C=cover, init=init)
    offs = (torch.arange(m, device=dX.device, dtype=torch.int64) * h)[None, :]
    err = float(((dX - dK[dB.to(torch.int64) + offs].sum(dim=1)).double() ** 2).sum().item()) / n
    return dK, dB, err


def train_opq_dev(dX, m, h, niter, init="natural", *, seed=0, engine):
    """train_opq on a device tensor (src/opq/OPQ.jl:21-101): dX (n, d) f32 -> (dK (m*h, d): the codebooks of the rotated space, padded; dB (n, m) uint8
    0-based (feeds train_chainq_dev); R (d, d) f32 host; obj (niter + 1,) f32).  The generator, its draw order (the "random" rotation, then h sampled rows per
    sub-space) and the empty-cluster rule (the old codeword stays) are train_opq's; only the sampled indices are uploaded.  torch is the glue on the device:
    the rotation X R, the reconstruction, the objective and the d x d product X CB' (float64); per iteration that matrix, R and the objective cross the bus
    and the Procrustes SVD runs on the host in float64."""
    import torch
    n, d = dX.shape
    dev = dX.device
    if d < m:
        raise ValueError("train_opq_dev: d = %d < m = %d" % (d, m))
    sd = _subdims(d, m)
    cover = _cover_map(sd, d, m)
    _check_wide(cover, "train_opq_dev")
    if n < h:
        raise ValueError("train_opq_dev: n = %d < h = %d: the initial codebooks are h rows sampled without replacement" % (n, h))
    rng = np.random.default_rng(seed)
    if init == "natural":
        R = np.eye(d, dtype=np.float32)
    elif init == "random":
        R = np.linalg.svd(rng.standard_normal((d, d)))[0].astype(np.float32)
    else:
        raise ValueError("Intialization %s unknown" % init)

    def rotate(Rm):
        return (dX @ torch.as_tensor(np.ascontiguousarray(Rm, dtype=np.float32), device=dev)).contiguous()       # rows of (R'X)'

    dXr = rotate(R)
    dK = torch.zeros((m * h, d), dtype=torch.float32, device=dev)
    for i in range(m):                                                          # :46-50
        rows = torch.from_numpy(rng.choice(n, h, replace=False).astype(np.int64)).to(dev)
        dK[i * h:(i + 1) * h, sd[i]] = dXr[rows, sd[i]]
    offs = (torch.arange(m, device=dev, dtype=torch.int64) * h)[None, :]
    dB = engine.assign_codewords_dev(dXr, dK, m, h=h)
    dX64 = dX.double()
    obj = np.zeros(niter + 1, dtype=np.float32)
    for it in range(niter + 1):
        dCB = dK[dB.to(torch.int64) + offs].sum(dim=1)                          # (n, d): the reconstructions in the rotated space
        dR = torch.as_tensor(R, device=dev)
        obj[it] = float(((dCB @ dR.T - dX).double() ** 2).sum().item()) / n
        M = (dX64.T @ dCB.double()).cpu().numpy()                               # X CB' (d x d), float64
        U, _, Vt = np.linalg.svd(M, full_matrices=False)                        # :78-79
        R = (U @ Vt).astype(np.float32)
        dXr = rotate(R)
        engine.update_centers_dev(dXr, dB, cover, m, K_prev=dK, h=h, out=dK)    # :85-86
        dB = engine.assign_codewords_dev(dXr, dK, m, h=h)                       # :88-91
    return dK, dB, R, obj
