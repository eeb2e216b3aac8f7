"""Host-side mirror of the reference's operator interface for the encoding path.

Same function names, positional arguments, array shapes (Julia d x n / m x n / list of d x h) and
1-based Int16 codes as the reference, so parity tests read like calls into the reference:

    encode_icm_cuda(RX, B, C, ilsiters, icmiter, npert, randord, nsplits=2, V=False) -> (Bs, objs)
        src/encodings/encode_icm_cuda.jl:253-262   (call site demos/demo_lsq_gpu.jl:50)
    encoding_icm(X, oldB, C, niter, randord, npert, V=False) -> B
        src/encodings/encode_icm.jl:131-189
    encode_icm_fully(B, X, C, binaries, cbi, niter, randord, npert, IDX, V)   (in place)
        src/encodings/encode_icm.jl:4-127
    get_unaries, get_binaries, veccost, qerror, splitarray   src/utils.jl
    randinit                                                  src/initializations.jl

Extra keyword-only arguments (`seed`, `it`, `engine`) expose what the reference leaves to global
RNG state.  Everything runs in liblsq_mi355x.so on the GPU; there is no CPU fallback here.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from . import engine as _engine

_default_engine = None


def default_engine():
    global _default_engine
    if _default_engine is None:
        _default_engine = _engine.Engine(0)
    return _default_engine


def _K_of(C):
    """hcat(C...) as the (m*h, d) row-major buffer (== Julia d x (m*h) column-major)."""
    return np.ascontiguousarray(np.concatenate([np.asarray(Cj, dtype=np.float32).T for Cj in C], axis=0))


def _dims(C):
    d, h = np.asarray(C[0]).shape
    return len(C), d, h


def _X_of(X):
    return np.ascontiguousarray(np.asarray(X, dtype=np.float32).T)       # (d, n) -> (n, d)


def _X8_of(X):
    """encode_icm_cuda's data matrix: a uint8 (d, n) matrix -- what bvecs_read returns -- stays uint8 ((n, d), the 8-bit entry points); int8 is refused
    by the engine; everything else is float32 as before."""
    if getattr(X, "dtype", None) in (np.dtype(np.uint8), np.dtype(np.int8)):
        return np.ascontiguousarray(np.asarray(X).T)
    return _X_of(X)


def _B_of(B):
    return np.ascontiguousarray(np.asarray(B, dtype=np.int16).T)         # (m, n) -> (n, m)


def encode_icm_cuda(RX, B, C, ilsiters, icmiter, npert, randord, nsplits=2, V=False, *, seed=0, engine=None):
    """-> (Bs, objs): Bs = list of (m, n) int16 1-based matrices, objs = float32 vector.
    RX may be the UInt8 matrix bvecs_read returns: it is handed over un-widened (lsq_encode_icm_u8) and gives what Float32.(RX) gives."""
    eng = engine or default_engine()
    m, d, h = _dims(C)
    Bs, objs = eng.encode_icm(_X8_of(RX), _B_of(B), _K_of(C), m, list(ilsiters), icmiter, npert, randord,
                              seed=seed, nsplits=nsplits, verbose=V, h=h)
    return [Bs[r].T for r in range(Bs.shape[0])], objs


def encoding_icm(X, oldB, C, niter, randord, npert, V=False, *, seed=0, it=None, engine=None):
    """One ILS iteration (encode_icm.jl:131-189).  With the reference's own argument list (no `it`) the engine counts the calls, so the
    demo loop `for i = 1:ilsiter; B = encoding_icm(...); end` (demos/demo_lsq.jl:48-51) perturbs differently every time -- and equals
    encode_icm_cuda(..., [ilsiter], ...) on a fresh engine (or after engine.set_option("ils_counter", 0))."""
    eng = engine or default_engine()
    m, d, h = _dims(C)
    return eng.encoding_icm(_X_of(X), _B_of(oldB), _K_of(C), m, niter, randord, npert, seed=seed, it=it, h=h).T


def encode_icm_fully(B, X, C, binaries, cbi, niter, randord, npert, IDX, V=False, *, seed=0, it=None, engine=None):
    """In place on B (m, n) int16.  `binaries`/`cbi` are accepted for signature parity and ignored
    (rebuilt on the device from C).  IDX = (first, last) 1-based or a range."""
    eng = engine or default_engine()
    m, d, h = _dims(C)
    first = IDX[0] if not isinstance(IDX, range) else IDX.start
    Bt = _B_of(B)
    eng.encode_icm_fully(Bt, _X_of(X), _K_of(C), m, niter, randord, npert, idx_first=int(first), seed=seed, it=it, h=h)
    B[...] = Bt.T
    return B


def get_unaries(X, C, V=False, *, engine=None):
    """-> list of m (h, n) matrices (unaries[j][a, i])."""
    eng = engine or default_engine()
    m, d, h = _dims(C)
    U = eng.get_unaries(_X_of(X), _K_of(C), m, h=h)
    return [U[j].T for j in range(m)]


def get_binaries(C, *, engine=None):
    """-> (binaries, cbi): binaries[idx] is (h, h) with [a, b] = 2<c_i[a], c_j[b]>, cbi (2, ncbi) 1-based, i<j i-major."""
    eng = engine or default_engine()
    m, d, h = _dims(C)
    T = eng.get_binaries(_K_of(C), m, h=h)
    binaries, cbi = [], []
    for i in range(m):
        for j in range(i + 1, m):
            binaries.append(T[i, j].T)        # T[i][j][b][a] -> [a, b]
            cbi.append((i + 1, j + 1))
    return binaries, np.asarray(cbi, dtype=np.int32).T.reshape(2, -1)


def veccost(X, B, C, *, engine=None):
    eng = engine or default_engine()
    m, d, h = _dims(C)
    return eng.veccost(_X_of(X), _B_of(B), _K_of(C), m, h=h)


def qerror(X, B, C, *, engine=None):
    eng = engine or default_engine()
    m, d, h = _dims(C)
    return eng.qerror(_X_of(X), _B_of(B), _K_of(C), m, h=h)


def beam_order(C):
    """The visiting order of encode_beam that starts with the codebooks that carry the most energy: 0-based codebook indices by descending mean
    ||c||^2 (float64 means; equal means keep their ascending order)."""
    e = [float((np.asarray(Cj, dtype=np.float64) ** 2).sum(axis=0).mean()) for Cj in C]
    return np.argsort(-np.asarray(e), kind="stable").astype(np.int32)


def encode_beam(X, C, L, order=None, *, engine=None):
    """Beam search of width L over the full pair tables (no counterpart in the reference; a deterministic start that can stand in for randinit).
    X d x n Float32 (or the UInt8 matrix bvecs_read returns), C the m codebooks (d x h), order: 0-based visiting order (None: ascending; beam_order(C):
    by energy) -> B m x n Int16 1-based."""
    eng = engine or default_engine()
    m, d, h = _dims(C)
    with eng.encoder(_K_of(C), m, h=h) as enc:
        return enc.beam(_X8_of(X), L, order=order).T


def linscan_lsq(B, X, C, dbnorms, R, k=10000, *, nthreads=0, engine=None):
    """Linear scan with LSQ codes + separately stored norms  (src/linscan/Linscan.jl:46-73).
    B (m, n) uint8 0-based; X (d, nq) queries; C list of (d, h); dbnorms (n,); R (d, d) rotation.
    -> dists (k, nq) float32 ascending, res (k, nq) int32 1-based ids.
    engine=None: the host scan (lsq_linscan_aqd_query_extra_byte, the reference's own division of labour);
    engine=<Engine>: the device scan (lsq_linscan) -- same results bit for bit."""
    from . import _lib
    B = np.ascontiguousarray(np.asarray(B, dtype=np.uint8).T)                   # (n, m)
    RX = np.ascontiguousarray((np.asarray(R, dtype=np.float32).T @ np.asarray(X, dtype=np.float32)).T)   # (nq, d)
    K = _K_of(C)
    dbn = np.ascontiguousarray(dbnorms, dtype=np.float32)
    n, m = B.shape
    nq, d = RX.shape
    h = np.asarray(C[0]).shape[1]
    if engine is not None:
        dists, res = engine.linscan(B, RX, K, dbn, m, k, h=h)
        return dists.T, res.T
    dists = np.zeros((nq, k), dtype=np.float32)
    res = np.zeros((nq, k), dtype=np.int32)
    _lib.check(_lib.load().lsq_linscan_aqd_query_extra_byte(dists.ctypes.data, res.ctypes.data, B.ctypes.data, RX.ctypes.data,
                                                            K.ctypes.data, dbn.ctypes.data, nq, n, m, h, d, k, int(nthreads)))
    return dists.T, res.T


def range_search_lsq(B, X, C, dbnorms, R, radius, *, centroids=None, assign=None, nprobe=0, add_coarse=False, X_coarse=None, allowed=None, nthreads=0):
    """Range search with LSQ codes on the host, for callers without an engine (lsq_range_search_cpu; the reference has no counterpart): every code
    whose ADC distance -- linscan_lsq's, bit for bit -- to a query is <= that query's radius.
    B (m, n) uint8 0-based; X (d, nq) queries; C list of (d, h); dbnorms (n,); R (d, d) rotation; radius a scalar or (nq,).  nprobe >= 1 with centroids
    (d, nlist) and assign (n,) 0-based lists: only the codes of each query's nprobe nearest lists (X_coarse (d, nq): what is compared with the centroids,
    default the rotated queries; add_coarse: the coarse distance added, for residual codes).  allowed (n,) bool: only those codes.
    -> lims (nq+1,) int64, dists (lims[-1],) float32, ids (lims[-1],) int32 1-based: query q's results are entries lims[q] .. lims[q+1]-1, ascending by
    (dist, id).  An engine's resident index answers the same question on the device: Index.range_search."""
    from . import _lib
    codes = np.ascontiguousarray(np.asarray(B, dtype=np.uint8).T)                # (n, m)
    RX = np.ascontiguousarray((np.asarray(R, dtype=np.float32).T @ np.asarray(X, dtype=np.float32)).T)   # (nq, d)
    K = _K_of(C)
    dbn = np.ascontiguousarray(dbnorms, dtype=np.float32)
    (n, m), (nq, d) = codes.shape, RX.shape
    h = np.asarray(C[0]).shape[1]
    rad = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,)))
    cent = lor = qc = None
    nlist = 0
    if int(nprobe) >= 1:
        if centroids is None or assign is None:
            raise ValueError("nprobe >= 1 needs centroids and assign")
        cent = np.ascontiguousarray(np.asarray(centroids, dtype=np.float32).T)   # (nlist, d)
        lor = np.ascontiguousarray(assign, dtype=np.int32)
        nlist = cent.shape[0]
        if cent.shape[1] != d or lor.shape != (n,):
            raise ValueError("shape mismatch: centroids %s, expected (%d, nlist); assign %s, expected (%d,)" % (np.asarray(centroids).shape, d, lor.shape, n))
        if X_coarse is not None:
            qc = np.ascontiguousarray(np.asarray(X_coarse, dtype=np.float32).T)
            if qc.shape != (nq, d):
                raise ValueError("shape mismatch: X_coarse %s, expected (%d, %d)" % (np.asarray(X_coarse).shape, d, nq))
    mask = None
    if allowed is not None:
        mask = np.ascontiguousarray(np.asarray(allowed) != 0).view(np.uint8)
        if mask.shape != (n,):
            raise ValueError("shape mismatch: allowed %s, expected (%d,)" % (mask.shape, n))
    ptr = lambda a: None if a is None else a.ctypes.data      # noqa: E731
    lims = np.zeros(nq + 1, dtype=np.int64)

    def call(dists, ids, capacity):
        _lib.check(_lib.load().lsq_range_search_cpu(lims.ctypes.data, ptr(dists), ptr(ids), capacity, codes.ctypes.data, K.ctypes.data, dbn.ctypes.data,
                                                    ptr(cent), ptr(lor), nlist, int(nprobe), _lib.IVF_ADD_COARSE if add_coarse else 0, ptr(mask),
                                                    RX.ctypes.data, ptr(qc), rad.ctypes.data, n, m, h, d, nq, d, int(nthreads)))

    call(None, None, 0)                                 # the two-call protocol: the counts, then arrays of exactly that size
    total = int(lims[-1])
    dists, ids = np.zeros(total, dtype=np.float32), np.zeros(total, dtype=np.int32)
    if total:
        call(dists, ids, total)
    return lims, dists, ids


def linscan_lsq_bytes(B, X, C, cbnorms, B_norms, R, k=10000, *, engine=None, nthreads=0):
    """linscan_lsq on the codes as train_lsq and quantize_norms leave them: the norm of a vector is ONE BYTE, an index into cbnorms, and is never widened
    to a float per vector (the reference does that one line before its scan, demos/demo_lsq_gpu.jl:57-60).
    B (m, n) uint8 0-based; X (d, nq); C list of (d, h); cbnorms (ncb <= 256,) float32; B_norms (n,) integers 1-BASED as quantize_norms returns them.
    -> linscan_lsq(B, X, C, cbnorms[B_norms - 1], R, k)'s arrays exactly.
    engine=<Engine>: a packed index (Engine.index_packed) of m + 1 bytes per vector; engine=None: the norms widened in numpy, the host scan."""
    cb = np.asarray(cbnorms)
    bn = np.asarray(B_norms)
    Bm = np.asarray(B)
    if cb.dtype != np.float32:
        raise TypeError("cbnorms must be float32, got %s" % cb.dtype)
    if bn.dtype.kind not in "iu":
        raise TypeError("B_norms must be an integer array (1-based indexes into cbnorms), got %s" % bn.dtype)
    if Bm.dtype != np.uint8:
        raise TypeError("B must be uint8 (0-based codes), got %s" % Bm.dtype)
    if cb.ndim != 1 or not 1 <= cb.shape[0] <= 256:
        raise ValueError("cbnorms must be a vector of 1 .. 256 entries, got shape %s" % (cb.shape,))
    if Bm.ndim != 2 or bn.ndim != 1 or bn.shape[0] != Bm.shape[1]:
        raise ValueError("B_norms must hold one entry per code: B %s, B_norms %s" % (Bm.shape, bn.shape))
    if bn.size and (int(bn.min()) < 1 or int(bn.max()) > cb.shape[0]):
        raise ValueError("B_norms must lie in 1 .. %d (got %d .. %d)" % (cb.shape[0], int(bn.min()), int(bn.max())))
    if engine is None:
        return linscan_lsq(Bm, X, C, cb[bn.astype(np.int64) - 1], R, k, nthreads=nthreads)
    codes = np.ascontiguousarray(Bm.T)
    RX = np.ascontiguousarray((np.asarray(R, dtype=np.float32).T @ np.asarray(X, dtype=np.float32)).T)
    h = np.asarray(C[0]).shape[1]
    with engine.index_packed(codes, _K_of(C), (bn.astype(np.int64) - 1).astype(np.uint8), np.ascontiguousarray(cb), codes.shape[1], h=h) as ix:
        dists, res = ix.search(RX, k)
    return dists.T, res.T


def linscan_pq(B, X, C, b, k=10000, *, engine=None):
    """Linear scan with PQ codes  (src/linscan/Linscan.jl:5-26 -> linscan_aqd_query, src/linscan/cpp/linscan_aqd.cpp:37-114).
    B (m, n) uint8 0-based; X (d, nq) queries; C list of (subdim, h) centre matrices; b bits per code (8 m); d % m == 0 (Cint(d/m)).
    -> dists (k, nq) float32 ascending, res (k, nq) uint32 1-based ids.
    engine=None: the host scan (lsq_linscan_aqd_query, the reference's own division of labour);
    engine=<Engine>: the device scan (lsq_linscan_pq) -- same results bit for bit."""
    from . import _lib
    codes = np.ascontiguousarray(np.asarray(B, dtype=np.uint8).T)              # (n, m): dim1codes = m
    Q = _X_of(X)                                                                # (nq, d): dim1queries = d
    n, m = codes.shape
    nq, d = Q.shape
    if d % m != 0:
        raise ValueError("linscan_pq: d=%d is not a multiple of m=%d (the reference passes Cint(d/m))" % (d, m))
    subdim = d // m
    centers = np.ascontiguousarray(np.stack([np.asarray(Ck, dtype=np.float32).T for Ck in C]))      # cat(3, C...) -> [len(C)][h][subdim]
    dists = np.zeros((nq, k), dtype=np.float32)
    res = np.zeros((nq, k), dtype=np.uint32)
    args = (dists.ctypes.data, res.ctypes.data, codes.ctypes.data, centers.ctypes.data, Q.ctypes.data, n, nq, int(b), int(k), m, d, subdim)
    if engine is not None:
        engine._check(engine._L.lsq_linscan_pq(engine._h, *args))
    else:
        _lib.check(_lib.load().lsq_linscan_aqd_query(*args))
    return dists.T, res.T + np.uint32(1)                                        # Linscan.jl:25: res .+= 1


def linscan_opq(B, X, C, b, R, k=10000, *, engine=None):
    """Linear scan with OPQ codes  (src/linscan/Linscan.jl:29-43): linscan_pq(B, R'X, C, b, k)."""
    RX = np.asarray(R, dtype=np.float32).T @ np.asarray(X, dtype=np.float32)
    return linscan_pq(B, RX, C, b, k, engine=engine)


def knn_exact(X_base, X_query, k, *, engine=None, nthreads=0):
    """Exact k-NN, the ground truth of a recall figure (what the reference reads from sift_groundtruth.ivecs, for any base).
    X_base (d, n), X_query (d, nq) Float32 in Julia shapes, or the UInt8 matrices of bvecs_read, which are handed through un-widened (same results as
    after astype(float32), by contract).  -> dists (k, nq) float32 ascending, ids (k, nq) uint32 1-BASED, so that eval_recall(ids[0, :], idx, knn) works
    directly.  dist = ((0 + e_0^2) + e_1^2) + ..., e_s = x[s] - q[s] in f32; ties by smaller id, NaN last.
    engine=None: the host cores (lsq_knn_exact_cpu / lsq_knn_exact_u8_cpu, nthreads 0 = all); engine=<Engine>: the device -- same results bit for bit."""
    from . import _lib
    Xb, Xq = _base_rows(X_base), _base_rows(X_query)
    if Xb.shape[1] != Xq.shape[1]:
        raise ValueError("knn_exact: base d=%d, queries d=%d" % (Xb.shape[1], Xq.shape[1]))
    b8, q8 = Xb.dtype == np.uint8, Xq.dtype == np.uint8
    if q8 and not b8:
        Xq, q8 = Xq.astype(np.float32), False
    if engine is not None:
        dists, ids = engine.knn_exact(Xb, Xq, k)
    else:
        (n, d), nq = Xb.shape, Xq.shape[0]
        dists = np.zeros((nq, k), dtype=np.float32)
        ids = np.zeros((nq, k), dtype=np.uint32)
        if b8:
            _lib.check(_lib.load().lsq_knn_exact_u8_cpu(dists.ctypes.data, ids.ctypes.data, Xb.ctypes.data, 1, Xq.ctypes.data, int(q8), n, nq, d, d, d,
                                                        int(k), int(nthreads)))
        else:
            _lib.check(_lib.load().lsq_knn_exact_cpu(dists.ctypes.data, ids.ctypes.data, Xb.ctypes.data, Xq.ctypes.data, n, nq, d, d, d, int(k),
                                                     int(nthreads)))
    return dists.T, ids.T + np.uint32(1)


def _base_rows(X_base):
    """(d, n) base set -> (n, d) rows; the uint8 matrix bvecs_read returns stays uint8 (the 8-bit road), everything else is float32"""
    if getattr(X_base, "dtype", None) == np.dtype(np.uint8):
        return np.ascontiguousarray(np.asarray(X_base).T)
    return _X_of(X_base)


def rerank(X_base, X_query, ids, k, *, engine=None, nthreads=0):
    """Stage two of a two-stage search -- no counterpart in the reference, which reports the recall of the ADC order: every query's candidates
    re-ordered by the exact distance of knn_exact.  X_base (d, n) Float32 or the UInt8 matrix of bvecs_read, X_query (d, nq), ids (L, nq) 1-based (what
    linscan_lsq / linscan_pq / linscan_opq return).  -> dists (k, nq) float32 ascending, ids (k, nq) int32 1-based; ties by smaller id, NaN last, an id
    outside 1..n last of all as (+inf, 0).  engine=None: the host cores (lsq_rerank_cpu); engine=<Engine>: the device -- same results bit for bit."""
    from . import _lib
    Xb, Xq = _base_rows(X_base), _X_of(X_query)
    cand = np.ascontiguousarray(np.asarray(ids).astype(np.int64).T.astype(np.int32))      # (nq, L)
    if Xb.shape[1] != Xq.shape[1] or cand.shape[0] != Xq.shape[0]:
        raise ValueError("rerank: base %s, queries %s, ids %s" % (Xb.shape, Xq.shape, cand.shape))
    if engine is not None:
        with engine.index(None, None, None, 0, base=Xb) as ix:
            dists, out = ix.rerank(Xq, cand, k, id_base=1)
    else:
        (n, d), (nq, L) = Xb.shape, cand.shape
        dists = np.zeros((nq, k), dtype=np.float32)
        out = np.zeros((nq, k), dtype=np.int32)
        _lib.check(_lib.load().lsq_rerank_cpu(dists.ctypes.data, out.ctypes.data, Xb.ctypes.data, int(Xb.dtype == np.uint8), Xq.ctypes.data,
                                              cand.ctypes.data, n, nq, d, d, d, L, int(k), 1, int(nthreads)))
    return dists.T, out.T


def narrow_rows(X, fmt, *, nthreads=0):
    """Rows of float32 narrowed to half precision on the host (lsq_narrow_rows_cpu), round to nearest even: fmt "f16" -> a float16 array (the bits of
    X.astype(np.float16)), "bf16" -> a uint16 array holding the upper 16 bits of the rounded float32 (numpy has no bfloat16).  X (n, d) rows with unit
    column stride (a row view is read in place).  What Engine.index(base=..., base_format=fmt) uploads."""
    from . import _lib
    from .engine import base_format_code
    code = base_format_code(fmt)
    if code is None:
        raise ValueError("narrow_rows needs a format: \"f16\" or \"bf16\"")
    X = np.asarray(X, dtype=np.float32)
    if X.ndim != 2 or X.strides[1] != 4 or X.strides[0] % 4 or (X.shape[0] > 1 and X.strides[0] < X.shape[1] * 4):
        X = np.ascontiguousarray(X)
    n, d = X.shape
    out = np.zeros((n, d), dtype=np.uint16)
    lds = int(X.strides[0] // 4) if n > 1 else d
    _lib.check(_lib.load().lsq_narrow_rows_cpu(out.ctypes.data if n else None, X.ctypes.data if n else None, n, d, max(lds, d), d, code, int(nthreads)))
    return out.view(np.float16) if code == _lib.BASE_F16 else out


def linscan_lsq_rerank(B, X, C, dbnorms, R, X_base, shortlist, k, *, engine=None, nthreads=0, base_format=None):
    """linscan_lsq for `shortlist` neighbours, then rerank to k: the scan reads R'X, the re-rank X against X_base (both in the base set's own frame).
    -> dists (k, nq) exact float32, ids (k, nq) int32 1-based.  engine=<Engine>: one resident index does both stages on the device (lsq_index_search).
    base_format="f16" / "bf16" (with an engine): the index keeps its base rows in half precision (Engine.index's base_format)."""
    if engine is None:
        if base_format is not None:
            raise ValueError("base_format needs an engine: the host road keeps no resident base")
        _, res = linscan_lsq(B, X, C, dbnorms, R, shortlist, nthreads=nthreads)
        return rerank(X_base, X, res, k, nthreads=nthreads)
    codes = np.ascontiguousarray(np.asarray(B, dtype=np.uint8).T)
    RX = np.ascontiguousarray((np.asarray(R, dtype=np.float32).T @ np.asarray(X, dtype=np.float32)).T)
    m, _, h = _dims(C)
    with engine.index(codes, _K_of(C), np.ascontiguousarray(dbnorms, dtype=np.float32), m, base=_base_rows(X_base), h=h, base_format=base_format) as ix:
        dists, ids = ix.search(RX, k, shortlist=shortlist, Q_exact=_X_of(X))
    return dists.T, ids.T


# -- the coarse partition of an inverted-list search (Index.set_lists / Index.search_ivf).  No counterpart in the reference; ROW arrays, as Engine and Index
# take them: X (n, d), centroids (nlist, d), codes (n, m) uint8 0-based, K (m*h, d) --------------------------------------------------------------------------

def ivf_assign(X, centroids, engine=None, *, nthreads=0):
    """The nearest centroid of every row: exact k-NN with one neighbour and the centroids as base (ties to the smaller list, NaN last) -- the rule by which
    Index.search_ivf picks a query's lists.  -> (n,) int32 0-based.  engine=None: the host cores; engine=<Engine>: the device, the same ids."""
    from . import _lib
    X, cent = np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(centroids, dtype=np.float32)
    if X.ndim != 2 or cent.ndim != 2 or X.shape[1] != cent.shape[1]:
        raise ValueError("ivf_assign: X %s, centroids %s" % (X.shape, cent.shape))
    if engine is not None:
        _, ids = engine.knn_exact(cent, X, 1)
    else:
        (n, d), nlist = X.shape, cent.shape[0]
        dists, ids = np.zeros((n, 1), dtype=np.float32), np.zeros((n, 1), dtype=np.uint32)
        _lib.check(_lib.load().lsq_knn_exact_cpu(dists.ctypes.data, ids.ctypes.data, cent.ctypes.data, X.ctypes.data, nlist, n, d, d, d, 1, int(nthreads)))
    return np.ascontiguousarray(ids[:, 0]).astype(np.int32)


def train_coarse(X, nlist, niter=10, seed=0, engine=None):
    """Seeded Lloyd iterations for the coarse centroids: nlist distinct rows of X to start (numpy's default_rng(seed)), assignment by ivf_assign, means in
    numpy (float64 sums, rounded to float32); an empty cluster keeps its centroid.  -> (centroids (nlist, d) float32, assign (n,) int32), assign being
    ivf_assign's of the returned centroids."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    n, d = X.shape
    if not 1 <= nlist <= n:
        raise ValueError("train_coarse: needs 1 <= nlist <= n (got nlist=%d n=%d)" % (nlist, n))
    cent = X[np.sort(np.random.default_rng(seed).choice(n, nlist, replace=False))].copy()
    assign = ivf_assign(X, cent, engine)
    for _ in range(niter):
        sums = np.zeros((nlist, d), dtype=np.float64)
        np.add.at(sums, assign, X)
        counts = np.bincount(assign, minlength=nlist)
        live = counts > 0
        cent[live] = (sums[live] / counts[live, None]).astype(np.float32)
        assign = ivf_assign(X, cent, engine)
    return cent, assign


def ivf_residual_norms(codes, K, centroids, assign):
    """The scalar a residual index stores as dbnorms: with r^ the reconstruction of a row's codes (of x - c_l) and c_l its list's centroid,
    |r^|^2 + 2 <c_l, r^> (float64, rounded to float32), so that the scan's sum plus the coarse distance (add_coarse=True) is |q - c_l - r^|^2."""
    codes, K = np.asarray(codes), np.asarray(K, dtype=np.float32)
    m = codes.shape[1]
    h = K.shape[0] // m
    recon = sum(K[j * h + codes[:, j].astype(np.int64)] for j in range(m)).astype(np.float64)
    c = np.asarray(centroids, dtype=np.float64)[np.asarray(assign, dtype=np.int64)]
    return ((recon * recon).sum(1) + 2.0 * (c * recon).sum(1)).astype(np.float32)


def train_coarse_dev(dX, nlist, niter=10, seed=0, *, engine):
    """train_coarse with everything resident in HBM: dX (n, d) float32 or uint8 device tensor (8-bit rows are never widened).  The same start rows
    (numpy's default_rng(seed).choice, gathered on the device), then Partition.assign and Partition.update alternated.
    -> (Partition, dassign (n,) int32 tensor); its centroids and assignment are bit-identical to train_coarse(X, nlist, niter, seed, engine)."""
    import torch
    n = int(dX.shape[0])
    if not 1 <= nlist <= n:
        raise ValueError("train_coarse_dev: needs 1 <= nlist <= n (got nlist=%d n=%d)" % (nlist, n))
    rows = torch.from_numpy(np.sort(np.random.default_rng(seed).choice(n, nlist, replace=False)).astype(np.int64)).to(dX.device)
    part = engine.partition_dev(dX[rows].to(torch.float32).contiguous())      # (uint8 -> float32 is exact)
    dassign = part.assign(dX)
    for _ in range(niter):
        part.update(dX, dassign)
        dassign = part.assign(dX)
    return part, dassign


def build_ivf_residual_index(dX, partition, dK, m, *, engine, ilsiters, icmiter, npert, randord, seed=0, dB0=None, cbnorms=None, base=None, report=None):
    """A residual inverted-list index built on the device: assign -> residuals -> encode_icm_dev on the residuals -> code_norms -> index_dev (cbnorms=None:
    float norms) or index_packed_dev (cbnorms (<= 256,): norm bytes) -> set_lists.  dX (n, d) float32 or uint8 device tensor, never widened: its
    residuals are the only float32 copy and are dropped after the encode.  partition: a device Partition (train_coarse_dev); dK (m*256, d): codebooks
    trained on residuals (train_lsq_dev on a training set's residuals); ilsiters: the ILS iterations (an int, or a list whose last entry counts); dB0:
    the start codes (default randinit_dev(seed)); base: the rows a shortlist is re-ranked on, or None; report: a dict that receives what the build made on
    the way (assign, codes: device tensors; obj: the mean squared error |x - c_l - r^|^2 the encode reports), or None.
    ONE FRAME: the rotation stays with the caller.  Codebooks in a rotated frame mean a partition trained on R'X; queries then go in as
    Q_scan = Q_coarse = R'q with add_coarse=True, Q_exact in the base's own frame.  -> the Index, lists set."""
    import torch
    dassign = partition.assign(dX)
    dR = partition.residuals(dX, dassign)
    n = int(dX.shape[0])
    if dB0 is None:
        dB0 = engine.randinit_dev(seed, n, m, device=dX.device)
    ils = [int(ilsiters)] if np.isscalar(ilsiters) else list(ilsiters)
    dBs, sums, _ = engine.encode_icm_dev(dR, dB0, dK, m, ils, icmiter, npert, randord, seed=seed)
    del dR
    dcodes = dBs[-1]
    if report is not None:
        report.update(assign=dassign, codes=dcodes, obj=float(sums[-1]) / max(n, 1))
    if cbnorms is None:
        ix = engine.index_dev(dcodes, dK, partition.code_norms(dcodes, dK, dassign), m, base=base)
    else:
        dcb = torch.as_tensor(np.asarray(cbnorms, dtype=np.float32) if not hasattr(cbnorms, "is_cuda") else cbnorms).to(dX.device).contiguous()
        _, dnc, _ = partition.code_norms(dcodes, dK, dassign, dcb)
        ix = engine.index_packed_dev(dcodes, dK, dnc, dcb, m, base=base)
    ix.set_lists(partition.centroids(), dassign)
    return ix


def eval_recall(ids_gnd, ids_predicted, k, V=False):
    """recall@N curve (src/linscan/Linscan.jl:76-117): ids_gnd (nq,), ids_predicted (k, nq), same id base.
    -> recall_at_i (k,) with recall_at_i[i-1] = fraction of queries whose true neighbour ranks <= i."""
    ids_gnd = np.asarray(ids_gnd)
    P = np.asarray(ids_predicted)
    nq = P.shape[1]
    assert nq == ids_gnd.shape[0]
    ranks = np.full(nq, k + 1, dtype=np.int64)
    for i in range(nq):
        pos = np.nonzero(P[:k, i] == ids_gnd[i])[0]
        if pos.size == 1:                                   # the reference requires exactly one hit (:94-98)
            ranks[i] = pos[0] + 1
    rec = np.array([(ranks <= i).sum() / nq for i in range(1, k + 1)], dtype=np.float64)
    if V:
        for i in (1, 2, 5, 10, 20, 50, 100, 200, 500, 1000, 2000, 5000, 10000):
            if i <= k:
                print("r@%d = %s" % (i, 100.0 * rec[i - 1]))
    return rec


def update_codebooks(X, B, h, V=False, codebook_upd_method="lsqr", *, nthreads=0, engine=None):
    """src/codebook_update.jl:52-86 -> list of m (d, h) codebooks minimising ||X - sum_j C_j[:, B_j]||^2 (LSQR, or LSMR with codebook_upd_method="lsmr": host only).
    engine=None: the host solver (std::thread workers over the dimensions, the reference's own division of labour);
    engine=<Engine>: the device solver (lsq_update_codebooks_gpu: all dimensions at once) -- the same result on every tested problem (required: 1e-5)."""
    from . import _lib
    if codebook_upd_method not in ("lsqr", "lsmr"):
        raise ValueError("Codebook update method unknown: %r" % (codebook_upd_method,))      # codebook_update.jl:22-23,60
    if codebook_upd_method == "lsmr" and engine is not None:
        raise ValueError("the device solver is LSQR (the reference's default); 'lsmr' runs on the host: pass engine=None")
    Xr, Br = _X_of(X), _B_of(B)
    n, d = Xr.shape
    m = Br.shape[1]
    if engine is not None:
        K, _ = engine.update_codebooks(Xr, Br, m, h=h)
        return [np.ascontiguousarray(K[j * h:(j + 1) * h].T) for j in range(m)]
    K = np.zeros((m * h, d), dtype=np.float32)
    fn = _lib.load().lsq_update_codebooks_lsmr if codebook_upd_method == "lsmr" else _lib.load().lsq_update_codebooks
    _lib.check(fn(Xr.ctypes.data, Br.ctypes.data, d, n, m, h, int(nthreads), K.ctypes.data))
    return [np.ascontiguousarray(K[j * h:(j + 1) * h].T) for j in range(m)]


def train_lsq(X, m, h, R, B, C, niter, ilsiter, icmiter, randord, npert, V=False, *, seed=0, engine=None, device_update=False):
    """src/lsq/LSQ.jl:10-88: alternate codebook update (host LSQR) and ILS/ICM encoding (GPU).
    -> (C, B, cbnorms, B_norms, obj).  The final norm codebook is the reference's plain k-means on the squared
    norms of the reconstructions (Clustering.kmeans there; initializers.kmeans here: k-means++ seeding + Lloyd, <= 100 sweeps, seeded -- unpinned)."""
    X = np.asarray(X, dtype=np.float32)
    R = np.asarray(R, dtype=np.float32)
    d, n = X.shape
    RX = R.T @ X
    upd_engine = engine if device_update else None          # device_update: the LSQR codebook update on the device too (needs `engine`)
    C = update_codebooks(RX, B, h, V, engine=upd_engine)
    C = [R @ Ci for Ci in C]
    it = 0

    def encode(Bc, it):
        Bs, _ = encode_icm_cuda(X, Bc, C, [ilsiter], icmiter, npert, randord, 1, V, seed=seed + it, engine=engine)
        return Bs[-1]

    B = encode(np.asarray(B, dtype=np.int16), it)
    obj = np.zeros(niter, dtype=np.float32)
    for iter_ in range(niter):
        obj[iter_] = qerror(X, B, C, engine=engine)
        if V:
            print("%3d %e" % (iter_ + 1, obj[iter_]))
        C = update_codebooks(X, B, h, V, engine=upd_engine)
        it += 1
        B = encode(B, it)
    # the codebook for norms (LSQ.jl:67-84): squared norms of the reconstructions (f32, dimensions ascending), then "plain-old k-means" with h centres.
    # The reference calls Clustering.jl's kmeans(dbnorms, h) -- k-means++ seeding, Lloyd until the assignments settle (at most 100 sweeps by default); un-vendored
    # and seeded from Julia's global RNG, so the centres are unpinned: the package's own kmeans() (initializers.py) is the same algorithm under `seed`.
    from .initializers import kmeans
    CB = reconstruct(B, C)
    dbnorms = np.zeros(n, dtype=np.float32)
    for j in range(CB.shape[0]):
        dbnorms += CB[j] * CB[j]
    centers, assign, _ = kmeans(dbnorms.reshape(1, n), min(h, n), niter=100, seed=seed)
    cb = centers.reshape(-1).astype(np.float32)
    B_norms = (assign + 1).reshape(1, n).astype(np.int16)
    return C, B, cb, B_norms, obj


def train_lsq_dev(dX, m, h, dB, niter, ilsiter, icmiter, randord, npert, *, seed=0, engine, R=None, norm_codebook=True):
    """src/lsq/LSQ.jl:10-88 with everything resident in HBM: the same alternation as train_lsq -- LSQR codebook update (lsq_update_codebooks_dev),
    ILS/ICM encode (lsq_encode_icm_dev, seed + call index), objective -- on device tensors, no host copy of X, the codes or the codebooks between the
    steps.  dX (n, d) f32, dB (n, m) uint8 0-BASED: CUDA/HIP torch tensors (the layouts of Engine.encode_icm_dev); R (d, d) rotation or None (identity).
    -> (dK (m*h, d) tensor, dB (n, m) uint8 tensor, cbnorms (<= h,) f32, B_norms (1, n) int16 1-based, obj (niter,) f32).  Same codebooks, codes and
    objective as train_lsq(..., engine=engine, device_update=True) on the same inputs (tests/test_pipeline_gpu.py).  torch is used for the two
    rotations only (RX = X R once; K R' once): glue, not the path."""
    import torch
    n, d = dX.shape
    dXr = dX if R is None else (dX @ torch.as_tensor(np.asarray(R, dtype=np.float32), device=dX.device)).contiguous()      # rows of RX' = (R' x)'
    dK, _ = engine.update_codebooks_dev(dXr, dB.contiguous(), m, h=h)
    if R is not None:
        dK = (dK @ torch.as_tensor(np.asarray(R, dtype=np.float32), device=dX.device).T).contiguous()                       # C = R C: rows of K are codewords
    del dXr
    it = 0

    def encode(dBc, it):
        dBs, sums, _ = engine.encode_icm_dev(dX, dBc, dK, m, [ilsiter], icmiter, npert, randord, seed=seed + it, h=h)
        return dBs[-1], float(sums[-1])

    dB, s = encode(dB.contiguous(), it)
    obj = np.zeros(niter, dtype=np.float32)
    for iter_ in range(niter):
        obj[iter_] = s / n                                                   # qerror(X, B, C): the mean cost of the codes the encode just returned
        dK, _ = engine.update_codebooks_dev(dX, dB, m, h=h)
        it += 1
        dB, s = encode(dB, it)
    if not norm_codebook:
        return dK, dB, None, None, obj
    # the codebook for norms (LSQ.jl:67-84): squared norms of the reconstructions on the device, the reference's plain k-means on the host (n scalars)
    from .initializers import kmeans
    _, _, nrm = engine.quantize_norms_dev(dB, dK, torch.zeros(1, dtype=torch.float32, device=dX.device), m, h=h)
    dbnorms = nrm.cpu().numpy()
    centers, assign, _ = kmeans(dbnorms.reshape(1, n), min(h, n), niter=100, seed=seed)
    return dK, dB, centers.reshape(-1).astype(np.float32), (assign + 1).reshape(1, n).astype(np.int16), obj      # B_norms 1 x n like train_lsq (LSQ.jl:84)


def _spgl1_inputs(X, B, h, tau, prevC, S):
    """Julia-layout arguments of the sparse codebook step -> (Xr (n, d), Br (n, m), K0 (m h, d) or None, m), checked before any device is touched."""
    X = np.asarray(X, dtype=np.float32)
    B = np.asarray(B)
    if X.ndim != 2 or B.ndim != 2:
        raise ValueError("X must be d x n and B m x n, got %s and %s" % (X.shape, B.shape))
    d, n = X.shape
    m = B.shape[0]
    K0 = None
    if prevC is not None:
        if len(prevC) != m or any(np.shape(Cj) != (d, h) for Cj in prevC):
            raise ValueError("prevC must hold m = %d matrices of d x h = %d x %d" % (m, d, h))
        K0 = _K_of(prevC)
    _engine.check_spgl1_args((n, d), (B.shape[1], m), m, h, tau, S, None if K0 is None else K0.shape)
    if B.size and (B.min() < 1 or B.max() > h):
        raise ValueError("codes must lie in 1..%d" % h)
    return _X_of(X), _B_of(B.astype(np.int16)), K0, m


def _spgl1(X, B, h, tau, prevC, S, engine, opt_tol, max_iter):
    Xr, Br, K0, m = _spgl1_inputs(X, B, h, tau, prevC, S)
    eng = engine or default_engine()
    K, info = eng.update_codebooks_spgl1(Xr, Br, m, float(tau), K_init=K0, S=int(S), h=h, opt_tol=opt_tol, max_iter=max_iter)
    return [np.ascontiguousarray(K[j * h:(j + 1) * h].T) for j in range(m)], info


def update_codebooks_spgl1(X, B, h, tau, prevC, spgl1_path=None, V=False, *, engine=None, opt_tol=None, max_iter=None, return_info=False):
    """src/codebook_update_sparse.jl:9-73: min 1/2 ||A k - vec(X')||^2 s.t. ||k||_1 <= tau over all d dimensions at once (A = I_d (x) sparsify_codes(B, h)),
    warm-started from prevC, on the device (csrc/lsq_spgl1.hip: SPGL1's LASSO mode restated; the reference calls MATLAB's SPGL1).  X d x n, B m x n Int16
    1-based, prevC m matrices d x h.  -> new C (m matrices d x h, f32) [, info dict].  `spgl1_path` is accepted and ignored: nothing calls MATLAB here."""
    C, info = _spgl1(X, B, h, tau, prevC, -1, engine, opt_tol, max_iter)
    if V:
        print("SPGL1 codebook update: %d iterations, f = %e, relative gap %.2e" % (info["iterations"], info["f"], info["rel_gap"]))
    return (C, info) if return_info else C


def update_codebooks_spgl1_threshold(X, B, h, tau, prevC, S, spgl1_path=None, V=False, *, engine=None, opt_tol=None, max_iter=None, return_info=False):
    """src/codebook_update_sparse.jl:75-106: update_codebooks_spgl1, then keep the S entries of K = hcat(C...) largest in |K| (ties: the lower linear
    index -- sortperm(abs(K[:]), rev=true)) and set the others to 0.  -> C [, info]."""
    C, info = _spgl1(X, B, h, tau, prevC, S, engine, opt_tol, max_iter)
    if V:
        print("%d non-zero elements after update" % info["nnz_before_threshold"])
    return (C, info) if return_info else C


def train_lsq_sparse(X, m, h, niter, ilsiter, icmiter, randord, npert, S, tau, B, Cinit, R, spgl1_path=None, V=True, *, seed=0, engine=None,
                     infos=None, opt_tol=None, max_iter=None):
    """src/lsq_sparse/LSQ_SPGL1.jl:6-120 (SLSQ): PQ codebooks Cinit (m matrices len(subdim) x h) padded to full dimension, then on RX = R'X alternate
    {SPGL1 codebook update + top-S threshold, ilsiter x encoding_icm} niter times, recording qerror before every update; the norm codebook is k-means on
    the squared norms of the reconstructions.  -> (C, B, R, obj, cbnorms, objs) like the reference: C in the rotated space (not rotated back).
    `infos` (optional list) receives the info dict of every codebook update.  encoding_icm's ILS iteration counter runs from `seed`'s call 0."""
    X = np.asarray(X, dtype=np.float32)
    R = np.asarray(R, dtype=np.float32)
    if X.ndim != 2:
        raise ValueError("X must be d x n")
    d, n = X.shape
    if R.shape != (d, d):
        raise ValueError("R must be d x d = %d x %d, got %s" % (d, d, R.shape))
    if len(Cinit) != m:
        raise ValueError("Cinit must hold m = %d codebooks" % m)
    subdims = [slice(lo, hi) for lo, hi in _engine.splitarray(d, m)]
    C = []
    for i in range(m):
        Ci = np.zeros((d, h), dtype=np.float32)
        Ci[subdims[i], :] = np.asarray(Cinit[i], dtype=np.float32)
        C.append(Ci)
    B = np.asarray(B, dtype=np.int16)
    _spgl1_inputs(X, B, h, tau, C, S)                                   # every argument checked before the device is touched
    if int(niter) < 0 or int(ilsiter) < 0:
        raise ValueError("niter and ilsiter must be >= 0")
    eng = engine or default_engine()
    RX = np.ascontiguousarray(R.T @ X)
    if V:
        print("Warm start error: %e" % qerror(RX, B, C, engine=eng))
    it = 0

    def update(C):
        C, info = _spgl1(RX, B, h, tau, C, S, eng, opt_tol, max_iter)
        if infos is not None:
            infos.append(info)
        if V:
            print("%d non-zero elements. l1 norm is %e" % (info["nnz"], sum(float(np.abs(Cj).sum(dtype=np.float64)) for Cj in C)))
        return C

    def encode(B, it):
        for _ in range(ilsiter):
            B = encoding_icm(RX, B, C, icmiter, randord, npert, V, seed=seed, it=it, engine=eng)
            it += 1
        return B, it

    C = update(C)
    B, it = encode(B, it)
    objs = np.zeros(niter, dtype=np.float32)
    for iter_ in range(niter):
        obj = qerror(RX, B, C, engine=eng)
        if V:
            print("%3d %e" % (iter_ + 1, obj))
        C = update(C)
        B, it = encode(B, it)
        objs[iter_] = obj
    from .initializers import kmeans
    CB = reconstruct(B, C)
    dbnorms = np.zeros(n, dtype=np.float32)
    for j in range(CB.shape[0]):
        dbnorms += CB[j] * CB[j]
    centers, _, _ = kmeans(dbnorms.reshape(1, n), min(h, n), niter=100, seed=seed)
    cbnorms = centers.reshape(-1).astype(np.float32)
    obj = qerror(RX, B, C, engine=eng)
    if V:
        print("%3d %e" % (niter + 1, obj))
    return C, B, R, obj, cbnorms, objs


def reconstruct(B, C):
    """src/utils.jl:203-223: CB = sum_i C[i][:, B[i, :]] accumulated in codebook order from zero (f32). -> (d, n)"""
    B = np.asarray(B)
    d = np.asarray(C[0]).shape[0]
    CB = np.zeros((d, B.shape[1]), dtype=np.float32)
    for i, Ci in enumerate(C):
        CB += np.asarray(Ci, dtype=np.float32)[:, B[i].astype(np.int64) - 1]
    return CB


def reconstruct_cpu(codes, K, m, *, ids=None, id_base=0, out=None, centroids=None, assign=None, add_coarse=False, pad_nan=False, h=256, nthreads=0):
    """The decode on the host, for callers without an engine and as the device's checker (lsq_reconstruct_cpu): codes (n, >=m) uint8 0-based rows with
    unit column stride (any row pitch), K (m*h, d) -> (count, d) float32: rows 0 .. n-1, or rows ids (count,) int32 in id_base.  add_coarse: plus
    centroids[assign[row]] (centroids (nlist, d), assign (n,) int32); pad_nan: an id outside the rows gives a row of NaN.  out: (count, >=d) float32
    rows to write into."""
    from . import _lib
    codes = np.asarray(codes, dtype=np.uint8)
    if codes.ndim != 2 or codes.strides[1] != 1:
        codes = np.ascontiguousarray(codes)
    K = np.ascontiguousarray(K, dtype=np.float32)
    n, d = int(codes.shape[0]), int(K.shape[1])
    ldc = int(codes.strides[0]) if n > 1 else int(codes.shape[1])
    if ids is not None:
        ids = np.ascontiguousarray(ids, dtype=np.int32)
    count = n if ids is None else int(ids.shape[0])
    if out is None:
        out = np.zeros((count, d), dtype=np.float32)
    if out.dtype != np.float32 or out.ndim != 2 or out.shape[0] != count or out.shape[1] < d or out.strides[1] != 4 or out.strides[0] % 4:
        raise ValueError("out must be (count, >=d) float32 rows with unit column stride")
    ldo = int(out.strides[0] // 4) if count > 1 else int(out.shape[1])
    cent = None if centroids is None else np.ascontiguousarray(centroids, dtype=np.float32)
    lor = None if assign is None else np.ascontiguousarray(assign, dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data      # noqa: E731
    fl = (_lib.RECON_ADD_COARSE if add_coarse else 0) | (_lib.RECON_PAD_NAN if pad_nan else 0)
    _lib.check(_lib.load().lsq_reconstruct_cpu(ptr(out), ldo, ptr(codes), ldc, ptr(K), ptr(ids), count, int(id_base), n, int(m), int(h), d, ptr(cent),
                                               ptr(lor), fl, int(nthreads)))
    return out


def quantize_norms(B, C, cbnorms, *, engine=None):
    """src/utils.jl:6-31: squared norm of every reconstruction (f32, dimensions ascending), then the index
    (1-based Int16) of the nearest scalar centroid in `cbnorms`; ties -> lowest index (findmin).
    engine=<Engine>: the device kernel (lsq_quantize_norms) -- the same numbers bit for bit."""
    if engine is not None:
        idx, _, _ = engine.quantize_norms(np.ascontiguousarray(np.asarray(B, dtype=np.int16).T), _K_of(C), cbnorms, len(C), h=np.asarray(C[0]).shape[1])
        return idx
    CB = reconstruct(B, C)
    norms = np.zeros(CB.shape[1], dtype=np.float32)
    for j in range(CB.shape[0]):                      # sequential f32 accumulation, j ascending
        norms += CB[j] * CB[j]
    cb = np.asarray(cbnorms, dtype=np.float32)
    d2 = (norms[None, :] - cb[:, None]) ** 2          # (h, n) f32
    return (np.argmin(d2, axis=0) + 1).astype(np.int16)


def _vecs_read(filename, bounds, dtype, item):
    """TEXMEX .fvecs/.ivecs/.bvecs (src/read/*vecs_read.jl): records [int32 d][d x item]; bounds = (a, b) 1-based
    inclusive, an int n (first n vectors) or None (all).  -> (d, n) column-per-vector like the reference."""
    with open(filename, "rb") as f:
        d = int(np.frombuffer(f.read(4), dtype=np.int32)[0])
        rec = 4 + d * item
        f.seek(0, 2)
        total = f.tell() // rec
        if bounds is None:
            a, b = 1, total
        elif isinstance(bounds, (int, np.integer)):
            a, b = 1, int(bounds)
        else:
            a, b = int(bounds[0]), int(bounds[-1])
        assert a >= 1 and b <= total
        f.seek((a - 1) * rec)
        raw = np.frombuffer(f.read((b - a + 1) * rec), dtype=np.uint8).reshape(b - a + 1, rec)
    dims = raw[:, :4].copy().view(np.int32).ravel()
    assert np.all(dims == d), "inconsistent dimension headers"
    return np.ascontiguousarray(raw[:, 4:]).view(dtype).reshape(b - a + 1, d).T


def fvecs_read(bounds, filename):
    return _vecs_read(filename, bounds, np.float32, 4)


def ivecs_read(bounds, filename):
    return _vecs_read(filename, bounds, np.int32, 4)


def bvecs_read(bounds, filename):
    return _vecs_read(filename, bounds, np.uint8, 1)


def randinit(n, m, h, *, seed=0):
    return _engine.randinit(n, m, h, seed=seed).T


def splitarray(x, nparts):
    """x: a range (1-based like Julia's 1:n) -> list of ranges."""
    n = len(x)
    return [x[s:e] for s, e in _engine.splitarray(n, nparts)]


# ---- snapshots without an engine: the host-only writer, reader, inspector and digest (lsq_snapshot_*_cpu) ---------------------------------------------
_SNAP_DTYPES = {"codebooks": np.float32, "codes": np.uint8, "dbnorms": np.float32, "norm_codes": np.uint8, "cbnorms": np.float32, "centroids": np.float32,
                "list_of_row": np.int32, "filter_bits": np.uint32}
_SNAP_BASE = {_lib.BASE_F32: np.float32, _lib.BASE_U8: np.uint8, _lib.BASE_F16: np.float16, _lib.BASE_BF16: np.uint16}


def snapshot_digest(data, first_word=0):
    """The digest of the bytes of `data` (anything numpy can view as bytes) taken as the words first_word, first_word + 1, ... of a snapshot section
    (include/lsq_mi355x.h (3p)); the digests of pieces cut at multiples of 4 bytes add up, mod 2^64, to the digest of the whole   [lsq_snapshot_digest_cpu]"""
    buf = np.frombuffer(np.ascontiguousarray(data).tobytes(), dtype=np.uint8)
    out = C.c_uint64()
    _lib.check(_lib.load().lsq_snapshot_digest_cpu(buf.ctypes.data if buf.size else None, int(buf.size), int(first_word), C.byref(out)))
    return int(out.value)


def snapshot_info(path, verify=False):
    """Header and section table of a snapshot file: n, d, m, h, packed, ncb, base_format, nlist, has_codes, has_base, filter_active, filter_force, allowed,
    file_bytes, header_digest and sections = [{name, kind, elem_bytes, offset, bytes, digest}].  verify: every section is read, its digest and the
    padding before it checked.  No engine, no device   [lsq_snapshot_inspect_cpu]"""
    info = _lib.SnapshotInfo()
    _lib.check(_lib.load().lsq_snapshot_inspect_cpu(os.fsencode(path), C.byref(info), int(bool(verify))))
    return info.as_dict()


def snapshot_write(path, *, codebooks=None, codes=None, dbnorms=None, norm_codes=None, cbnorms=None, base=None, base_format=None, centroids=None,
                   list_of_row=None, filter_bits=None, filter_force=0):
    """Write a snapshot from host arrays -- the keys of Index.export() -- without an engine: the bytes Index.save() writes for the index built over
    them.  A plain index gives dbnorms, a packed one norm_codes and cbnorms; base: float32, uint8, float16 rows, or uint16 bfloat16 bits with
    base_format="bf16"; filter_bits: uint32 words, bits at or past n are dropped   [lsq_snapshot_write_cpu]"""
    a, keep = _lib.SnapshotArrays(), []
    given = {"codebooks": codebooks, "codes": codes, "dbnorms": dbnorms, "norm_codes": norm_codes, "cbnorms": cbnorms, "centroids": centroids,
             "list_of_row": list_of_row, "filter_bits": filter_bits}
    for key, arr in given.items():
        if arr is not None:
            arr = np.ascontiguousarray(arr, dtype=_SNAP_DTYPES[key])
            keep.append(arr)
            setattr(a, key, arr.ctypes.data)
    if codes is None and base is None:
        raise ValueError("a snapshot needs codes, base rows or both")
    if codes is not None:
        if codebooks is None or (dbnorms is None) == (norm_codes is None) or (norm_codes is None) != (cbnorms is None):
            raise ValueError("codes need codebooks and either dbnorms or norm_codes + cbnorms")
        a.n, a.m, a.h, a.d = int(keep[1].shape[0]), int(np.asarray(codes).shape[1]), 256, int(np.asarray(codebooks).shape[1])
        a.packed, a.ncb = int(norm_codes is not None), 0 if cbnorms is None else int(np.asarray(cbnorms).shape[0])
    if base is not None:
        base = np.asarray(base)
        fmt = {"float32": _lib.BASE_F32, "uint8": _lib.BASE_U8, "float16": _lib.BASE_F16}.get(base.dtype.name)
        if base_format == "bf16" and base.dtype == np.uint16:
            fmt = _lib.BASE_BF16
        if fmt is None or (base_format is not None and base_format != {_lib.BASE_F16: "f16", _lib.BASE_BF16: "bf16"}.get(fmt)):
            raise TypeError("base rows of dtype %s with base_format=%r" % (base.dtype, base_format))
        base = np.ascontiguousarray(base)
        keep.append(base)
        a.base, a.base_format = base.ctypes.data, fmt
        if codes is None:
            a.n, a.d = int(base.shape[0]), int(base.shape[1])
    a.nlist = 0 if centroids is None else int(np.asarray(centroids).shape[0])
    a.filter_active, a.filter_force = int(filter_bits is not None), int(filter_force)
    sizes = {"codebooks": a.m * 256 * a.d, "codes": a.n * a.m, "dbnorms": a.n, "norm_codes": a.n, "cbnorms": a.ncb, "centroids": a.nlist * a.d,
             "list_of_row": a.n, "filter_bits": (a.n + 31) // 32}
    for key, arr in given.items():
        if arr is not None and np.asarray(arr).size != sizes[key]:
            raise ValueError("%s holds %d elements, the shapes ask for %d" % (key, np.asarray(arr).size, sizes[key]))
    if base is not None and base.shape != (a.n, a.d):
        raise ValueError("base must be (%d, %d), got %s" % (a.n, a.d, base.shape))
    _lib.check(_lib.load().lsq_snapshot_write_cpu(os.fsencode(path), C.byref(a)))


def snapshot_read(path):
    """The arrays of a snapshot file as a dict with the keys of Index.export() (only those present; filter_force beside filter_bits), every digest
    verified.  No engine, no device   [lsq_snapshot_inspect_cpu, lsq_snapshot_read_cpu]"""
    info = snapshot_info(path)
    n, d, m = info["n"], info["d"], info["m"]
    shapes = {"codebooks": (m * 256, d), "codes": (n, m), "dbnorms": (n,), "norm_codes": (n,), "cbnorms": (info["ncb"],), "base": (n, d),
              "centroids": (info["nlist"], d), "list_of_row": (n,), "filter_bits": ((n + 31) // 32,)}
    a, out = _lib.SnapshotArrays(), {}
    for sec in info["sections"]:
        key = sec["name"]
        out[key] = np.zeros(shapes[key], dtype=_SNAP_BASE[info["base_format"]] if key == "base" else _SNAP_DTYPES[key])
        setattr(a, key, out[key].ctypes.data)
    _lib.check(_lib.load().lsq_snapshot_read_cpu(os.fsencode(path), C.byref(a)))
    if info["filter_active"]:
        out["filter_force"] = int(a.filter_force)
    return out
