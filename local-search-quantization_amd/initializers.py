"""Initialisers of the LSQ training pipeline: PQ, OPQ and ChainQ.

Mirrors of the reference's trainers with the reference's names, argument order and Julia shapes, so that
`demos/demo_lsq_gpu.jl` reads the same against this package:

    C, B, R, err = train_opq(x_train, m, h, niter, "natural")        # src/opq/OPQ.jl:21-101
    C, B, R, err = train_chainq(x_train, m, h, R, B, C, niter)       # src/chainq/chainq.jl:10-58
    C, B, cbnorms, B_norms, obj = train_lsq(x_train, m, h, R, B, C, ...)   # reference_api.train_lsq (GPU encoder)

The two data-parallel steps run ON THE DEVICE through the C-ABI (csrc/lsq_init.hip; round 6): the nearest-codeword assignment of PQ / OPQ and of
their k-means (`lsq_assign_codewords`: every sub-space of a vector set in one call, codebooks padded to d rows) and ChainQ's Viterbi encoder
(`lsq_encode_viterbi`).  Like the rest of the engine they need h == 256 and a gfx950 device -- there is no CPU fallback; the numpy restatement of
these steps lives in oracle/init_oracle.py as the checker (tests only).  What stays on the host is the glue around them: k-means++ seeding, cluster
means, the Procrustes SVD, and the scalar k-means of the norm codebook (an O(n log h) sorted search).  The chain's structured LSQR codebook update runs
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
           "update_codebooks_chain", "encoding_viterbi", "train_chainq", "train_chainq_dev", "kmeans"]


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


def kmeans(X, h, niter=25, seed=0, engine=None):
    """Lloyd k-means with k-means++ seeding on the columns of X (r x n) -> centers (r x h), assignments (n,) 0-based, total cost.
    Stands in for Clustering.jl's `kmeans(X, h, init=:kmpp)` (src/pq/PQ.jl:60)."""
    X = _f32(X)
    r, n = X.shape
    rng = np.random.default_rng(seed)
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


def train_pq(X, m, h, V=False, *, seed=0, engine=None):
    """train_pq(X, m, h) -> C, B, error.  src/pq/PQ.jl:44-76 (k-means per subspace)."""
    X = _f32(X)
    sd = _subdims(X.shape[0], m)
    C, B = [], []
    for i in range(m):
        c, a, cost = kmeans(X[sd[i]], h, seed=seed + i, engine=engine)
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
