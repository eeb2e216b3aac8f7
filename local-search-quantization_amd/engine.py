"""Engine: thin, typed Python handle on the C-ABI context (one per process / per GPU).

Row-major conventions (the Julia buffers seen from numpy, see include/lsq_mi355x.h):
    X (n, d) float32 | K (m*h, d) float32 | B (n, m) int16 1-based (host) / uint8 0-based (device)
    X (n, d) uint8 (the encode calls only: .bvecs base sets stay 8-bit end to end, the lsq_*_u8 entry points)
torch is used only as the owner of device memory and streams; every computation happens inside
liblsq_mi355x.so.
"""
import contextlib
import ctypes as C
import weakref

import numpy as np

from . import _lib

H = 256
IT_AUTO = 0xFFFFFFFF      # LSQ_IT_AUTO: the context counts the ILS iterations of the CPU-shaped entry points


def _np(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a


def _x_host(X):
    """The data matrix of an encode call as a C-contiguous host array -> (array, is_u8).  uint8 (numpy, or a CPU torch tensor) stays uint8 and takes
    the 8-bit entry points; int8 is refused (bytes of a .bvecs file are unsigned: a signed view would encode other vectors); anything else is
    converted to float32 as it always was.  A non-contiguous array is copied, whatever its type."""
    dt = getattr(X, "dtype", None)
    name = str(dt).replace("torch.", "") if dt is not None else ""
    if name == "int8":
        raise TypeError("int8 data is not accepted: 8-bit base sets are unsigned (uint8); view or convert the array explicitly")
    if name == "uint8":
        return np.ascontiguousarray(X, dtype=np.uint8), True
    return _np(X, np.float32), False


def _is_u8(a):
    return str(getattr(a, "dtype", "")).replace("torch.", "") == "uint8"


class Engine:
    def __init__(self, device=0, chunk=None, profile=False, schedule=None, skip=None, tuning=False):
        """tuning=True loads liblsq_mi355x_tuning.so (same ABI + option "ablation", environment knobs, clock stamps)."""
        self._L = _lib.load(tuning=tuning)
        h = C.c_void_p()
        self._check(self._L.lsq_create(C.byref(h), int(device)))
        self._h = h
        self._indexes = weakref.WeakSet()             # the Index objects made on this context: closed before it
        self.device = int(device)
        if chunk is not None:
            self.set_option("chunk", int(chunk))
        if schedule is not None:
            self.set_option("schedule", int(schedule))
        if skip is not None:
            self.set_option("skip", int(bool(skip)))
        if profile:
            self.set_option("profile", 1)

    def _check(self, rc):
        return _lib.check(rc, self._L)

    # -- lifetime -------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            for ix in list(getattr(self, "_indexes", ())):      # an index needs its context to free what it holds on the device
                ix.close()
            self._L.lsq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- options / timing -----------------------------------------------------------------
    def set_option(self, key, value):
        self._check(self._L.lsq_set_option(self._h, key.encode(), int(value)))

    def set_stream(self, hip_stream_ptr):
        self._check(self._L.lsq_set_stream(self._h, C.c_void_p(hip_stream_ptr or 0)))

    @contextlib.contextmanager
    def _on_torch_stream(self):
        """Bind the context to torch's CURRENT stream for the duration of one call, then return to the context's own stream.
        The torch stream object is held for as long as its raw handle is bound, so a temporary stream
        (`with torch.cuda.stream(torch.cuda.Stream())`) can never leave a dangling hipStream_t behind."""
        import torch
        stream = torch.cuda.current_stream(self.device)
        self.set_stream(stream.cuda_stream)
        try:
            yield stream
        finally:
            self.set_option("own_stream", 1)

    def synchronize(self):
        self._check(self._L.lsq_synchronize(self._h))

    def timings(self):
        t = _lib.Timings()
        self._check(self._L.lsq_get_timings_sized(self._h, C.addressof(t), C.sizeof(t)))      # size-checked: this binding and the library may be of different versions
        return t.as_dict()

    def walk_trace(self, count=64):
        """recomputed node updates per position (sweep * m + rank in the visiting order) since reset_timings  [lsq_get_walk_trace]"""
        out = np.zeros(count, dtype=np.int64)
        self._check(self._L.lsq_get_walk_trace(self._h, out.ctypes.data, int(count)))
        return out

    def reset_timings(self):
        self._check(self._L.lsq_reset_timings(self._h))

    def q16_snapshot(self):
        """What the last resident chunk of the last encode call left behind for the 16-bit filtered walk: the inputs of the inequality its window rests on
        (csrc/lsq_icmq.hip, BOUND), read-only   [lsq_get_q16_snapshot].  Raises LsqError (LSQ_EINVAL) when no filtered chunk is resident.
        -> dict: rows (cn), row0 (the chunk's first row within the call), m, slq / slf (candidates per 16-bit / f32 slice), filtered (the chunk stayed on the
           filtered walk to its end), params {ok, oor, nflag, loU, invD, D, hiq (f32 arrays [m]), window (int [m]), slack (f64 [m])}, and device tensors
           Uq u16 [m][256/slq][cn][slq], Tq u16 [m][256/slq][(m-1)*256][slq], qflag u16 [cn], U f32 [m][256/slf][cn][slf], T f32 [m][m][256][256]
           (torch has no uint16 arithmetic: the u16 items come as int16 tensors holding the same bits)."""
        import torch
        P = _lib.Q16SnapshotParams()
        info = np.zeros(6, dtype=np.int64)
        torch.cuda.current_stream(self.device).synchronize()      # the tensors below are written on the context's stream, not on torch's
        self._check(self._L.lsq_get_q16_snapshot(self._h, _lib.SNAP_PARAMS, C.addressof(P), C.sizeof(P), info.ctypes.data))
        cn, row0, m, slq, slf, filtered = (int(v) for v in info)
        dev = torch.device("cuda", self.device)
        shapes = {"Uq": (_lib.SNAP_UQ, torch.int16, (m, H // slq, cn, slq)), "Tq": (_lib.SNAP_TQ, torch.int16, (m, H // slq, (m - 1) * H, slq)),
                  "qflag": (_lib.SNAP_QFLAG, torch.int16, (cn,)), "U": (_lib.SNAP_U, torch.float32, (m, H // slf, cn, slf)),
                  "T": (_lib.SNAP_T, torch.float32, (m, m, H, H))}
        out = {"rows": cn, "row0": row0, "m": m, "slq": slq, "slf": slf, "filtered": bool(filtered)}
        for name, (what, dtype, shape) in shapes.items():
            t = torch.empty(shape, dtype=dtype, device=dev)
            self._check(self._L.lsq_get_q16_snapshot(self._h, what, t.data_ptr(), t.numel() * t.element_size(), None))
            out[name] = t
        self.synchronize()
        nodes = [P.node[j] for j in range(m)]
        out["params"] = {"ok": int(P.ok), "oor": int(P.oor), "nflag": int(P.nflag),
                         "loU": np.array([q.loU for q in nodes], dtype=np.float32), "invD": np.array([q.invD for q in nodes], dtype=np.float32),
                         "D": np.array([q.D for q in nodes], dtype=np.float32), "hiq": np.array([q.hiq for q in nodes], dtype=np.float32),
                         "window": np.array([q.window for q in nodes], dtype=np.int64), "slack": np.array([q.slack for q in nodes], dtype=np.float64)}
        return out

    # -- (1) whole call, host buffers -------------------------------------------------------
    def encode_icm(self, X, B, K, m, ilsiters, icmiter, npert, randord, seed=0, nsplits=1, global_offset=0,
                   verbose=False, h=H):
        """-> Bs (nr, n, m) int16 1-based, objs (nr,) float32   [lsq_encode_icm; uint8 X: lsq_encode_icm_u8, the rows stay 8-bit]"""
        X, u8 = _x_host(X)
        K, B = _np(K, np.float32), _np(B, np.int16)
        n, d = X.shape
        self._check_shapes(X, K, B, m, h)
        ils = _np(ilsiters, np.int64).reshape(-1)
        nr = ils.shape[0]
        Bs = np.empty((nr, n, m), dtype=np.int16)
        objs = np.zeros(nr, dtype=np.float32)
        call = self._L.lsq_encode_icm_u8 if u8 else self._L.lsq_encode_icm
        self._check(call(self._h, X.ctypes.data, B.ctypes.data, K.ctypes.data, d, n, m, h,
                                          ils.ctypes.data, nr, int(icmiter), int(npert), int(bool(randord)),
                                          int(nsplits), int(seed), int(global_offset), int(bool(verbose)),
                                          Bs.ctypes.data, objs.ctypes.data))
        return Bs, objs

    # -- (1b) whole call, device-resident torch tensors -------------------------------------
    def encode_icm_dev(self, dX, dB0, dK, m, ilsiters, icmiter, npert, randord, seed=0, global_offset=0,
                       out=None, h=H, nonblocking=False):
        """dX (n,d) f32 or uint8 (8-bit rows: lsq_encode_icm_u8_dev, any byte offset into a larger buffer), dB0 (n,m) u8 0-based, dK (m*h,d) f32:
        CUDA/HIP torch tensors.
        -> dBs (nr, n, m) uint8 tensor, obj_sums (nr,) float64 numpy (SUM of costs), stats (I, 2) int64.
        nonblocking=True (option "async"): nothing in the call waits for the device; obj_sums and stats come back as DEVICE tensors, valid after the
        caller has synchronised torch's current stream (the call can be captured into a graph from its second use on a shape on)."""
        import torch
        assert dX.is_cuda and dB0.is_cuda and dK.is_cuda, "device tensors required"
        if dX.dtype == torch.int8:
            raise TypeError("int8 data is not accepted: 8-bit base sets are unsigned (uint8)")
        assert dX.dtype in (torch.float32, torch.uint8) and dK.dtype == torch.float32 and dB0.dtype == torch.uint8
        assert dX.is_contiguous() and dB0.is_contiguous() and dK.is_contiguous()
        call = self._L.lsq_encode_icm_u8_dev if dX.dtype == torch.uint8 else self._L.lsq_encode_icm_dev
        n, d = dX.shape
        if dB0.shape != (n, m) or dK.shape != (m * h, d):
            raise ValueError("shape mismatch: X %s B %s K %s m=%d h=%d" % (tuple(dX.shape), tuple(dB0.shape), tuple(dK.shape), m, h))
        ils = _np(ilsiters, np.int64).reshape(-1)
        nr = ils.shape[0]
        I = int(ils.max())
        dBs = out if out is not None else torch.empty((nr, n, m), dtype=torch.uint8, device=dX.device)
        if nonblocking:
            obj_t = torch.zeros(nr, dtype=torch.float64, device=dX.device)
            stats_t = torch.zeros((I, 2), dtype=torch.int64, device=dX.device)
            with self._on_torch_stream():
                self.set_option("async", 1)
                try:
                    self._check(call(self._h, dX.data_ptr(), dB0.data_ptr(), dK.data_ptr(), d, n, m, h,
                                                           ils.ctypes.data, nr, int(icmiter), int(npert), int(bool(randord)),
                                                           int(seed), int(global_offset), dBs.data_ptr(), obj_t.data_ptr(), stats_t.data_ptr()))
                finally:
                    self.set_option("async", 0)
            return dBs, obj_t, stats_t
        obj = np.zeros(nr, dtype=np.float64)
        stats = np.zeros((I, 2), dtype=np.int64)
        with self._on_torch_stream():
            self._check(call(self._h, dX.data_ptr(), dB0.data_ptr(), dK.data_ptr(), d, n, m, h,
                                                   ils.ctypes.data, nr, int(icmiter), int(npert), int(bool(randord)),
                                                   int(seed), int(global_offset), dBs.data_ptr(), obj.ctypes.data,
                                                   stats.ctypes.data))
        return dBs, obj, stats

    # -- (1c) the search step after the path: ADC linear scan on the device ------------------
    def linscan(self, codes, Q, K, dbnorms, m, k, h=H):
        """codes (n,m) uint8 0-based, Q (nq,d), K (m*h,d), dbnorms (n,): host arrays.
        -> dists (nq,k) float32 ascending, ids (nq,k) int32 1-BASED   [lsq_linscan]"""
        codes, Q, K, dbn = _np(codes, np.uint8), _np(Q, np.float32), _np(K, np.float32), _np(dbnorms, np.float32)
        n, nq, d = codes.shape[0], Q.shape[0], Q.shape[1]
        if codes.shape != (n, m) or K.shape != (m * h, d) or dbn.shape != (n,):
            raise ValueError("shape mismatch: codes %s Q %s K %s dbnorms %s m=%d h=%d" % (codes.shape, Q.shape, K.shape, dbn.shape, m, h))
        dists = np.zeros((nq, k), dtype=np.float32)
        ids = np.zeros((nq, k), dtype=np.int32)
        self._check(self._L.lsq_linscan(self._h, dists.ctypes.data, ids.ctypes.data, codes.ctypes.data, Q.ctypes.data, K.ctypes.data,
                                        dbn.ctypes.data, nq, n, m, h, d, int(k)))
        return dists, ids

    def linscan_dev(self, dcodes, dQ, dK, dnorms, m, k, h=H):
        """The same on device-resident torch tensors -> (dists (nq,k) f32, ids (nq,k) int32 1-based) tensors   [lsq_linscan_dev]"""
        import torch
        assert dcodes.is_cuda and dQ.is_cuda and dK.is_cuda and dnorms.is_cuda, "device tensors required"
        assert dcodes.dtype == torch.uint8 and dQ.dtype == torch.float32 and dK.dtype == torch.float32 and dnorms.dtype == torch.float32
        assert dcodes.is_contiguous() and dQ.is_contiguous() and dK.is_contiguous() and dnorms.is_contiguous()
        n, (nq, d) = dcodes.shape[0], dQ.shape
        if dcodes.shape != (n, m) or dK.shape != (m * h, d) or dnorms.shape != (n,):
            raise ValueError("shape mismatch")
        dists = torch.empty((nq, k), dtype=torch.float32, device=dQ.device)
        ids = torch.empty((nq, k), dtype=torch.int32, device=dQ.device)
        with self._on_torch_stream():
            self._check(self._L.lsq_linscan_dev(self._h, dists.data_ptr(), ids.data_ptr(), dcodes.data_ptr(), dQ.data_ptr(), dK.data_ptr(),
                                                dnorms.data_ptr(), nq, n, m, h, d, int(k)))
        return dists, ids

    def linscan_pq(self, codes, Q, C3, m, k, subdim):
        """PQ / OPQ codes, no norm term.  codes (n, dim1codes) uint8 0-based (the first m bytes of a row used), Q (nq, dim1queries),
        C3 (m, 256, subdim) centres (any shape holding m*256*subdim floats): host arrays.
        -> dists (nq,k) float32 ascending, ids (nq,k) uint32 0-BASED   [lsq_linscan_pq]"""
        codes, Q, C3 = _np(codes, np.uint8), _np(Q, np.float32), _np(C3, np.float32)
        if codes.ndim != 2 or Q.ndim != 2 or C3.size != m * H * subdim:
            raise ValueError("shape mismatch: codes %s Q %s C3 %s m=%d subdim=%d" % (codes.shape, Q.shape, C3.shape, m, subdim))
        (n, dc), (nq, dq) = codes.shape, Q.shape
        dists = np.zeros((nq, k), dtype=np.float32)
        ids = np.zeros((nq, k), dtype=np.uint32)
        self._check(self._L.lsq_linscan_pq(self._h, dists.ctypes.data, ids.ctypes.data, codes.ctypes.data, C3.ctypes.data, Q.ctypes.data,
                                           n, nq, 8 * m, int(k), dc, dq, int(subdim)))
        return dists, ids

    def linscan_pq_dev(self, dcodes, dQ, dC3, m, k, subdim):
        """The same on device-resident torch tensors -> (dists (nq,k) f32, ids (nq,k) 0-based) tensors; torch has no uint32 arithmetic, so the
        ids tensor is int32 holding the uint32 bits (every id is below 2^31)   [lsq_linscan_pq_dev]"""
        import torch
        assert dcodes.is_cuda and dQ.is_cuda and dC3.is_cuda, "device tensors required"
        assert dcodes.dtype == torch.uint8 and dQ.dtype == torch.float32 and dC3.dtype == torch.float32
        assert dcodes.is_contiguous() and dQ.is_contiguous() and dC3.is_contiguous()
        if dcodes.dim() != 2 or dQ.dim() != 2 or dC3.numel() != m * H * subdim:
            raise ValueError("shape mismatch")
        (n, dc), (nq, dq) = dcodes.shape, dQ.shape
        dists = torch.empty((nq, k), dtype=torch.float32, device=dQ.device)
        ids = torch.empty((nq, k), dtype=torch.int32, device=dQ.device)
        with self._on_torch_stream():
            self._check(self._L.lsq_linscan_pq_dev(self._h, dists.data_ptr(), ids.data_ptr(), dcodes.data_ptr(), dC3.data_ptr(), dQ.data_ptr(),
                                                   n, nq, 8 * m, int(k), dc, dq, int(subdim)))
        return dists, ids

    def knn_exact(self, Xb, Xq, k):
        """Exact k-NN (the ground truth of a recall figure).  Xb (n, d) base rows, Xq (nq, d) queries: host arrays, float32 -- or a uint8 base (the
        un-widened rows of a .bvecs set) with uint8 or float queries, which goes through a temporary base-only Index and is never widened.
        -> dists (nq,k) float32 ascending, ids (nq,k) uint32 0-BASED; ties by smaller id, NaN last   [lsq_knn_exact / lsq_index_knn]"""
        if _is_u8(Xb):
            if Xb.ndim != 2 or Xq.ndim != 2 or Xb.shape[1] != Xq.shape[1]:
                raise ValueError("shape mismatch: base %s queries %s" % (tuple(Xb.shape), tuple(Xq.shape)))
            with self.index(None, None, None, 0, base=Xb) as ix:
                dists, ids = ix.knn(Xq, k)
            return dists, ids.view(np.uint32)
        Xb, Xq = _np(Xb, np.float32), _np(Xq, np.float32)
        if Xb.ndim != 2 or Xq.ndim != 2 or Xb.shape[1] != Xq.shape[1]:
            raise ValueError("shape mismatch: base %s queries %s" % (Xb.shape, Xq.shape))
        (n, d), nq = Xb.shape, Xq.shape[0]
        dists = np.zeros((nq, k), dtype=np.float32)
        ids = np.zeros((nq, k), dtype=np.uint32)
        self._check(self._L.lsq_knn_exact(self._h, dists.ctypes.data, ids.ctypes.data, Xb.ctypes.data, Xq.ctypes.data, n, nq, d, d, d, int(k)))
        return dists, ids

    def knn_exact_dev(self, dXb, dXq, k):
        """The same on device-resident torch tensors (n, d) / (nq, d), f32 -- or a uint8 base with uint8 or f32 queries (a temporary Index that borrows
        the base); row views with unit column stride are read in place.
        -> (dists (nq,k) f32, ids (nq,k) 0-based) tensors; the ids tensor is int32 holding the uint32 bits   [lsq_knn_exact_dev / lsq_index_knn]"""
        import torch
        if dXb.dtype == torch.uint8:
            if dXb.dim() != 2 or dXq.dim() != 2 or dXb.shape[1] != dXq.shape[1]:
                raise ValueError("shape mismatch: base %s queries %s" % (tuple(dXb.shape), tuple(dXq.shape)))
            with self.index_dev(None, None, None, 0, base=dXb) as ix:
                return ix.knn(dXq, k)
        assert dXb.is_cuda and dXq.is_cuda and dXb.dtype == torch.float32 and dXq.dtype == torch.float32, "device f32 tensors required"
        if dXb.dim() != 2 or dXq.dim() != 2 or dXb.shape[1] != dXq.shape[1]:
            raise ValueError("shape mismatch: base %s queries %s" % (tuple(dXb.shape), tuple(dXq.shape)))
        (n, d), nq = dXb.shape, dXq.shape[0]
        for t in (dXb, dXq):
            if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < d):
                raise ValueError("rows must be unit-stride and at least d floats apart (got strides %s)" % (t.stride(),))
        ldb = dXb.stride(0) if n > 1 else d
        ldq = dXq.stride(0) if nq > 1 else d
        dists = torch.empty((nq, k), dtype=torch.float32, device=dXq.device)
        ids = torch.empty((nq, k), dtype=torch.int32, device=dXq.device)
        with self._on_torch_stream():
            self._check(self._L.lsq_knn_exact_dev(self._h, dists.data_ptr(), ids.data_ptr(), dXb.data_ptr(), dXq.data_ptr(), n, nq, d, ldb, ldq, int(k)))
        return dists, ids

    # -- (1d) two-stage search on a resident index ------------------------------------------
    def index(self, codes, K, dbnorms, m, base=None, h=H, d=None):
        """An Index of HOST arrays, copied once and owned by the index: codes (n,m) uint8 0-based, K (m*h,d), dbnorms (n,), base (n,ldb) float32 or
        uint8 (the un-widened rows of a .bvecs set) or None (scan only).  codes=None: a base-only index (re-rank only), which reads the first d
        components of a base row (default: all of them)   [lsq_index_create]"""
        return Index(self, codes, K, dbnorms, m, base, h, d, on_device=False)

    def index_dev(self, dcodes, dK, dnorms, m, base=None, h=H, d=None):
        """The same on device-resident torch tensors, BORROWED: the index keeps references to them; searches take and return tensors.  base: a 2-d
        tensor or a view of one with unit column stride, at any byte offset."""
        return Index(self, dcodes, dK, dnorms, m, base, h, d, on_device=True)

    def quantize_norms(self, B, K, cbnorms, m, h=H):
        """B (n,m) int16 1-based, K (m*h,d), cbnorms (<= 256,): host arrays.
        -> idx (n,) int16 1-based index of the nearest norm centroid, dbnorms (n,) = cbnorms[idx-1], norms (n,) unquantised   [lsq_quantize_norms]"""
        B, K, cb = _np(B, np.int16), _np(K, np.float32), _np(cbnorms, np.float32).reshape(-1)
        n, d = B.shape[0], K.shape[1]
        if B.shape != (n, m) or K.shape != (m * h, d):
            raise ValueError("shape mismatch: B %s K %s m=%d h=%d" % (B.shape, K.shape, m, h))
        idx = np.zeros(n, dtype=np.int16)
        dbn = np.zeros(n, dtype=np.float32)
        nrm = np.zeros(n, dtype=np.float32)
        self._check(self._L.lsq_quantize_norms(self._h, B.ctypes.data, K.ctypes.data, cb.ctypes.data, cb.shape[0], d, n, m, h,
                                               idx.ctypes.data, dbn.ctypes.data, nrm.ctypes.data))
        return idx, dbn, nrm

    def quantize_norms_dev(self, dcodes, dK, dcb, m, h=H):
        """device tensors: codes (n,m) uint8 0-based, K (m*h,d) f32, cbnorms (<= 256,) f32 -> idx (n,) uint8 0-BASED, dbnorms (n,), norms (n,)   [lsq_quantize_norms_dev]"""
        import torch
        assert dcodes.is_cuda and dK.is_cuda and dcb.is_cuda and dcodes.dtype == torch.uint8 and dK.dtype == torch.float32 and dcb.dtype == torch.float32
        assert dcodes.is_contiguous() and dK.is_contiguous() and dcb.is_contiguous()
        n, d = dcodes.shape[0], dK.shape[1]
        if dcodes.shape != (n, m) or dK.shape != (m * h, d):
            raise ValueError("shape mismatch")
        idx = torch.empty(n, dtype=torch.uint8, device=dK.device)
        dbn = torch.empty(n, dtype=torch.float32, device=dK.device)
        nrm = torch.empty(n, dtype=torch.float32, device=dK.device)
        with self._on_torch_stream():
            self._check(self._L.lsq_quantize_norms_dev(self._h, dcodes.data_ptr(), dK.data_ptr(), dcb.data_ptr(), int(dcb.numel()), d, n, m, h,
                                                       idx.data_ptr(), dbn.data_ptr(), nrm.data_ptr()))
        return idx, dbn, nrm

    def update_codebooks(self, X, B, m, h=H):
        """X (n,d) f32, B (n,m) int16 1-based: host arrays -> K (m*h,d) least-squares codebooks, LSQR iterations   [lsq_update_codebooks_gpu]"""
        X, B = _np(X, np.float32), _np(B, np.int16)
        n, d = X.shape
        if B.shape != (n, m):
            raise ValueError("shape mismatch: X %s B %s m=%d" % (X.shape, B.shape, m))
        K = np.zeros((m * h, d), dtype=np.float32)
        it = C.c_int(0)
        self._check(self._L.lsq_update_codebooks_gpu(self._h, X.ctypes.data, B.ctypes.data, d, n, m, h, K.ctypes.data, C.byref(it)))
        return K, int(it.value)

    def update_codebooks_dev(self, dX, dcodes, m, h=H, out=None):
        """device tensors: X (n,d) f32, codes (n,m) uint8 0-based -> K (m*h,d) f32 tensor, LSQR iterations   [lsq_update_codebooks_dev]"""
        import torch
        assert dX.is_cuda and dcodes.is_cuda and dX.dtype == torch.float32 and dcodes.dtype == torch.uint8 and dX.is_contiguous() and dcodes.is_contiguous()
        n, d = dX.shape
        if dcodes.shape != (n, m):
            raise ValueError("shape mismatch")
        dK = out if out is not None else torch.empty((m * h, d), dtype=torch.float32, device=dX.device)
        it = C.c_int(0)
        with self._on_torch_stream():
            self._check(self._L.lsq_update_codebooks_dev(self._h, dX.data_ptr(), dcodes.data_ptr(), d, n, m, h, dK.data_ptr(), C.byref(it)))
        return dK, int(it.value)

    # -- the structured codebook update: update_codebooks_generic / update_codebooks_chain (codebook_update.jl:104-158) ------------------
    def update_codebooks_struct(self, X, B, dim2C, m, h=H):
        """X (n,d) f32, B (n,m) int16 1-based, dim2C (d,m) 0/1 (codebook j covers dimension t) or None (every codebook covers everything): host arrays
        -> K (m*h,d) least-squares codebooks over the covering codebooks only, exactly zero elsewhere; LSQR iterations   [lsq_update_codebooks_struct_gpu]"""
        X, B = _np(X, np.float32), _np(B, np.int16)
        n, d = X.shape
        if B.shape != (n, m):
            raise ValueError("shape mismatch: X %s B %s m=%d" % (X.shape, B.shape, m))
        cover = None if dim2C is None else cover_bytes(dim2C, d, m)
        K = np.empty((m * h, d), dtype=np.float32)
        it = C.c_int(0)
        self._check(self._L.lsq_update_codebooks_struct_gpu(self._h, X.ctypes.data, B.ctypes.data, None if cover is None else cover.ctypes.data, d, n, m, h,
                                                            K.ctypes.data, C.byref(it)))
        return K, int(it.value)

    def update_codebooks_struct_dev(self, dX, dcodes, ddim2C, m, h=H, out=None):
        """device tensors: X (n,d) f32, codes (n,m) uint8 0-based; dim2C (d,m) 0/1 as a device tensor (uint8 or bool), a host array, or None
        -> K (m*h,d) f32 tensor (`out` when given: it may hold anything), LSQR iterations   [lsq_update_codebooks_struct_dev]"""
        import torch
        assert dX.is_cuda and dcodes.is_cuda and dX.dtype == torch.float32 and dcodes.dtype == torch.uint8 and dX.is_contiguous() and dcodes.is_contiguous()
        n, d = dX.shape
        if dcodes.shape != (n, m):
            raise ValueError("shape mismatch")
        if ddim2C is None:
            dcover = None
        elif isinstance(ddim2C, torch.Tensor):
            if tuple(ddim2C.shape) != (d, m):
                raise ValueError("dim2C must be (d, m) = (%d, %d), got %s" % (d, m, tuple(ddim2C.shape)))
            dcover = ddim2C.to(device=dX.device, dtype=torch.uint8).t().contiguous()          # Julia's d x m in memory: [m][d]
        else:
            dcover = torch.from_numpy(cover_bytes(ddim2C, d, m)).to(dX.device)
        dK = out if out is not None else torch.empty((m * h, d), dtype=torch.float32, device=dX.device)
        if tuple(dK.shape) != (m * h, d) or dK.dtype != torch.float32 or not dK.is_cuda or not dK.is_contiguous():
            raise ValueError("out must be a contiguous (m*h, d) = (%d, %d) f32 device tensor" % (m * h, d))
        it = C.c_int(0)
        with self._on_torch_stream():
            self._check(self._L.lsq_update_codebooks_struct_dev(self._h, dX.data_ptr(), dcodes.data_ptr(), None if dcover is None else dcover.data_ptr(),
                                                                d, n, m, h, dK.data_ptr(), C.byref(it)))
        return dK, int(it.value)

    # -- the sparse codebook update: SPGL1's LASSO mode (csrc/lsq_spgl1.hip) ---------------------------------
    @staticmethod
    def _spgl1_params(opt_tol, max_iter):
        if opt_tol is None and max_iter is None:
            return None
        return _lib.Spgl1Params(float(opt_tol or 0.0), int(max_iter or 0))

    def update_codebooks_spgl1(self, X, B, m, tau, K_init=None, S=-1, h=H, opt_tol=None, max_iter=None):
        """X (n,d) f32, B (n,m) int16 1-based: host arrays -> (K (m*h,d) f32, info dict): min 1/2||A k - b||^2 s.t. ||k||_1 <= tau warm-started
        from K_init, then only the S largest |K| kept (S < 0: all)   [lsq_update_codebooks_spgl1]"""
        X, B = _np(X, np.float32), _np(B, np.int16)
        n, d = X.shape if X.ndim == 2 else (-1, -1)
        check_spgl1_args(X.shape, B.shape, m, h, tau, S, None if K_init is None else np.shape(K_init), opt_tol, max_iter)
        K0 = None if K_init is None else _np(K_init, np.float32)
        K = np.zeros((m * h, d), dtype=np.float32)
        info = _lib.Spgl1Info()
        p = self._spgl1_params(opt_tol, max_iter)
        self._check(self._L.lsq_update_codebooks_spgl1(self._h, X.ctypes.data, B.ctypes.data, d, n, m, h, float(tau),
                                                       None if K0 is None else K0.ctypes.data, int(S), None if p is None else C.byref(p),
                                                       K.ctypes.data, C.byref(info)))
        return K, info.as_dict()

    def update_codebooks_spgl1_dev(self, dX, dcodes, m, tau, dK_init=None, S=-1, h=H, opt_tol=None, max_iter=None, out=None):
        """device tensors: X (n,d) f32, codes (n,m) uint8 0-based, K_init (m*h,d) f32 or None -> (K (m*h,d) f32 tensor, info dict)
        [lsq_update_codebooks_spgl1_dev]"""
        import torch
        check_spgl1_args(tuple(dX.shape), tuple(dcodes.shape), m, h, tau, S, None if dK_init is None else tuple(dK_init.shape), opt_tol, max_iter)
        for name, t, dt in (("X", dX, torch.float32), ("codes", dcodes, torch.uint8), ("K_init", dK_init, torch.float32), ("out", out, torch.float32)):
            if t is None:
                continue
            if not t.is_cuda or t.dtype != dt:
                raise ValueError("%s must be a %s device tensor" % (name, dt))
            if not t.is_contiguous():
                raise ValueError("%s must be contiguous" % name)
        n, d = dX.shape
        dK = out if out is not None else torch.empty((m * h, d), dtype=torch.float32, device=dX.device)
        if tuple(dK.shape) != (m * h, d):
            raise ValueError("out must be (m*h, d) = (%d, %d)" % (m * h, d))
        info = _lib.Spgl1Info()
        p = self._spgl1_params(opt_tol, max_iter)
        with self._on_torch_stream():
            self._check(self._L.lsq_update_codebooks_spgl1_dev(self._h, dX.data_ptr(), dcodes.data_ptr(), d, n, m, h, float(tau),
                                                               None if dK_init is None else dK_init.data_ptr(), int(S),
                                                               None if p is None else C.byref(p), dK.data_ptr(), C.byref(info)))
        return dK, info.as_dict()

    # -- the initialisers' data-parallel steps (csrc/lsq_init.hip) ----------------------------------
    def encode_viterbi(self, X, K, m, h=H):
        """X (n,d) f32, K (m*h,d) f32 (chain codebooks, zero outside their dimensions) -> B (n,m) int16 1-based: the exact chain optimum
        (encode_chain.jl:92-123)   [lsq_encode_viterbi]"""
        X, K = _np(X, np.float32), _np(K, np.float32)
        n, d = X.shape
        if K.shape != (m * h, d):
            raise ValueError("K must be (m*h, d) = (%d, %d), got %s" % (m * h, d, K.shape))
        B = np.empty((n, m), dtype=np.int16)
        self._check(self._L.lsq_encode_viterbi(self._h, X.ctypes.data, K.ctypes.data, d, n, m, h, B.ctypes.data))
        return B

    def encode_viterbi_dev(self, dX, dK, m, h=H):
        """device tensors -> codes (n,m) uint8 0-based   [lsq_encode_viterbi_dev]"""
        import torch
        assert dX.is_cuda and dK.is_cuda and dX.dtype == torch.float32 and dK.dtype == torch.float32 and dX.is_contiguous() and dK.is_contiguous()
        n, d = dX.shape
        if dK.shape != (m * h, d):
            raise ValueError("shape mismatch")
        dB = torch.empty((n, m), dtype=torch.uint8, device=dX.device)
        with self._on_torch_stream():
            self._check(self._L.lsq_encode_viterbi_dev(self._h, dX.data_ptr(), dK.data_ptr(), d, n, m, h, dB.data_ptr()))
        return dB

    def assign_codewords(self, X, K, m, h=H, want_min=False):
        """Per codebook independently the first argmin_a ||c||^2 - 2<x,c> (quantize_pq / the k-means assignment step; PQ.jl:12-41, kmeans.jl:6-75).
        X (n,d), K (m*h,d) -> B (n,m) int16 1-based [, the minima (n,m) f32]   [lsq_assign_codewords]"""
        X, K = _np(X, np.float32), _np(K, np.float32)
        n, d = X.shape
        if K.shape != (m * h, d):
            raise ValueError("K must be (m*h, d) = (%d, %d), got %s" % (m * h, d, K.shape))
        B = np.empty((n, m), dtype=np.int16)
        mv = np.empty((n, m), dtype=np.float32) if want_min else None
        self._check(self._L.lsq_assign_codewords(self._h, X.ctypes.data, K.ctypes.data, d, n, m, h, B.ctypes.data, mv.ctypes.data if want_min else None))
        return (B, mv) if want_min else B

    def assign_codewords_dev(self, dX, dK, m, h=H, want_min=False):
        """device tensors -> codes (n,m) uint8 0-based [, minima (n,m) f32]   [lsq_assign_codewords_dev]"""
        import torch
        assert dX.is_cuda and dK.is_cuda and dX.dtype == torch.float32 and dK.dtype == torch.float32 and dX.is_contiguous() and dK.is_contiguous()
        n, d = dX.shape
        if dK.shape != (m * h, d):
            raise ValueError("shape mismatch")
        dB = torch.empty((n, m), dtype=torch.uint8, device=dX.device)
        dmin = torch.empty((n, m), dtype=torch.float32, device=dX.device) if want_min else None
        with self._on_torch_stream():
            self._check(self._L.lsq_assign_codewords_dev(self._h, dX.data_ptr(), dK.data_ptr(), d, n, m, h, dB.data_ptr(), dmin.data_ptr() if want_min else None))
        return (dB, dmin) if want_min else dB

    # -- PQ / OPQ training resident on the device: cluster means and k-means++ seeding (csrc/lsq_kmeans.hip) ----------------
    @staticmethod
    def _host_cover(dim2C, d, m):
        """dim2C (d, m) 0/1 as a host array or a tensor (copied to the host: the library checks the map before it launches anything) -> (m, d) bytes"""
        if hasattr(dim2C, "detach"):
            dim2C = dim2C.detach().cpu().numpy()
        return cover_bytes(dim2C, d, m)

    def update_centers(self, X, B, dim2C, m, K_prev=None, h=H):
        """X (n,d) f32, B (n,m) int16 1-based, dim2C (d,m) 0/1, K_prev (m*h,d) or None: host arrays -> (K (m*h,d): per codebook and code the mean of its
        rows over the covered dimensions, rows added in ascending order in f32; an empty cluster keeps its row of K_prev (None: zero); exact zeros outside
        the cover.  counts (m*h,) int32)   [lsq_update_centers]"""
        X, B = _np(X, np.float32), _np(B, np.int16)
        n, d = X.shape
        if B.shape != (n, m):
            raise ValueError("shape mismatch: X %s B %s m=%d" % (X.shape, B.shape, m))
        cover = self._host_cover(dim2C, d, m)
        Kp = None if K_prev is None else _np(K_prev, np.float32)
        if Kp is not None and Kp.shape != (m * h, d):
            raise ValueError("K_prev must be (m*h, d) = (%d, %d), got %s" % (m * h, d, Kp.shape))
        K = np.empty((m * h, d), dtype=np.float32)
        counts = np.zeros(m * h, dtype=np.int32)
        self._check(self._L.lsq_update_centers(self._h, X.ctypes.data, B.ctypes.data, cover.ctypes.data, None if Kp is None else Kp.ctypes.data, d, n, m, h,
                                               K.ctypes.data, counts.ctypes.data))
        return K, counts

    def update_centers_dev(self, dX, dcodes, dim2C, m, K_prev=None, h=H, out=None, counts=None):
        """device tensors: X (n,d) f32, codes (n,m) uint8 0-based, K_prev (m*h,d) f32 or None (it may be `out`); dim2C (d,m) 0/1 on the HOST
        -> (K (m*h,d) f32 tensor (`out` when given: it may hold anything), counts (m*h,) int32 tensor).  Nothing waits for the device   [lsq_update_centers_dev]"""
        import torch
        assert dX.is_cuda and dcodes.is_cuda and dX.dtype == torch.float32 and dcodes.dtype == torch.uint8 and dX.is_contiguous() and dcodes.is_contiguous()
        n, d = dX.shape
        if dcodes.shape != (n, m):
            raise ValueError("shape mismatch")
        cover = self._host_cover(dim2C, d, m)
        dK = out if out is not None else torch.empty((m * h, d), dtype=torch.float32, device=dX.device)
        for name, t in (("out", dK), ("K_prev", K_prev)):
            if t is not None and (tuple(t.shape) != (m * h, d) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous()):
                raise ValueError("%s must be a contiguous (m*h, d) = (%d, %d) f32 device tensor" % (name, m * h, d))
        dcnt = counts if counts is not None else torch.empty(m * h, dtype=torch.int32, device=dX.device)
        if tuple(dcnt.shape) != (m * h,) or dcnt.dtype != torch.int32 or not dcnt.is_cuda or not dcnt.is_contiguous():
            raise ValueError("counts must be a contiguous (m*h,) int32 device tensor")
        with self._on_torch_stream():
            self._check(self._L.lsq_update_centers_dev(self._h, dX.data_ptr(), dcodes.data_ptr(), cover.ctypes.data, None if K_prev is None else K_prev.data_ptr(),
                                                       d, n, m, h, dK.data_ptr(), dcnt.data_ptr()))
        return dK, dcnt

    @staticmethod
    def _seed_u(u, m, h):
        u = _np(u, np.float64)
        if u.shape != (m, h):
            raise ValueError("u must be (m, h) = (%d, %d) doubles in [0, 1), got %s" % (m, h, u.shape))
        return u

    def kmeanspp_seed(self, X, dim2C, u, m, h=H):
        """k-means++ (D^2) seeding of all m sub-spaces.  X (n,d) f32, dim2C (d,m) 0/1, u (m,h) doubles in [0,1) drawn by the caller: host arrays
        -> (K (m*h,d): the chosen rows restricted to the cover, idx (m,h) int64 0-based row indices, d2 (n,m) f32 squared distance to the nearest chosen row)
        [lsq_kmeanspp_seed]"""
        X = _np(X, np.float32)
        n, d = X.shape
        cover, u = self._host_cover(dim2C, d, m), self._seed_u(u, m, h)
        K = np.empty((m * h, d), dtype=np.float32)
        idx = np.empty((m, h), dtype=np.int64)
        d2 = np.empty((n, m), dtype=np.float32)
        self._check(self._L.lsq_kmeanspp_seed(self._h, X.ctypes.data, cover.ctypes.data, u.ctypes.data, d, n, m, h, K.ctypes.data, idx.ctypes.data, d2.ctypes.data))
        return K, idx, d2

    def kmeanspp_seed_dev(self, dX, dim2C, u, m, h=H, want_idx=True, want_d2=False, out=None):
        """The same on a device tensor X (n,d) f32; dim2C and u on the HOST -> (K (m*h,d) f32 tensor, idx (m,h) int64 tensor or None, d2 (n,m) f32 tensor or
        None).  2 h - 1 launches in stream order, nothing waits for the device   [lsq_kmeanspp_seed_dev]"""
        import torch
        assert dX.is_cuda and dX.dtype == torch.float32 and dX.is_contiguous()
        n, d = dX.shape
        cover, u = self._host_cover(dim2C, d, m), self._seed_u(u, m, h)
        dK = out if out is not None else torch.empty((m * h, d), dtype=torch.float32, device=dX.device)
        if tuple(dK.shape) != (m * h, d) or dK.dtype != torch.float32 or not dK.is_cuda or not dK.is_contiguous():
            raise ValueError("out must be a contiguous (m*h, d) = (%d, %d) f32 device tensor" % (m * h, d))
        didx = torch.empty((m, h), dtype=torch.int64, device=dX.device) if want_idx else None
        dd2 = torch.empty((n, m), dtype=torch.float32, device=dX.device) if want_d2 else None
        with self._on_torch_stream():
            self._check(self._L.lsq_kmeanspp_seed_dev(self._h, dX.data_ptr(), cover.ctypes.data, u.ctypes.data, d, n, m, h, dK.data_ptr(),
                                                      didx.data_ptr() if want_idx else None, dd2.data_ptr() if want_d2 and n > 0 else None))
        return dK, didx, dd2

    def linscan_stats(self):
        t = _lib.LinscanStats()
        self._check(self._L.lsq_get_linscan_stats(self._h, C.byref(t)))
        return t.as_dict()

    # -- (2) CPU-path shaped ---------------------------------------------------------------
    def encoding_icm(self, X, oldB, K, m, niter, randord, npert, seed=0, it=None, global_offset=0, h=H):
        """ONE ILS iteration with the accept rule.  it=None (default): the context's own counter (LSQ_IT_AUTO) -- the k-th call uses it = k-1."""
        it = IT_AUTO if it is None else it
        X, K, oldB = _np(X, np.float32), _np(K, np.float32), _np(oldB, np.int16)
        n, d = X.shape
        self._check_shapes(X, K, oldB, m, h)
        out = np.empty((n, m), dtype=np.int16)
        self._check(self._L.lsq_encoding_icm(self._h, X.ctypes.data, oldB.ctypes.data, K.ctypes.data, d, n, m, h,
                                            int(niter), int(bool(randord)), int(npert), int(seed), int(it),
                                            int(global_offset), out.ctypes.data))
        return out

    def encode_icm_fully(self, B, X, K, m, niter, randord, npert, idx_first=1, seed=0, it=None, h=H):
        """In place on B (n, m) int16 (must be C-contiguous int16).  it=None: the context's counter, as in encoding_icm."""
        it = IT_AUTO if it is None else it
        X, K = _np(X, np.float32), _np(K, np.float32)
        if B.dtype != np.int16 or not B.flags["C_CONTIGUOUS"]:
            raise ValueError("B must be a C-contiguous int16 (n, m) array (it is updated in place)")
        n, d = X.shape
        self._check_shapes(X, K, B, m, h)
        self._check(self._L.lsq_encode_icm_fully(self._h, B.ctypes.data, X.ctypes.data, K.ctypes.data, d, n, m, h,
                                                int(niter), int(bool(randord)), int(npert), int(idx_first), int(seed), int(it)))
        return B

    # -- (3) helpers -----------------------------------------------------------------------
    def get_unaries(self, X, K, m, h=H):
        X, K = _np(X, np.float32), _np(K, np.float32)
        n, d = X.shape
        U = np.empty((m, n, h), dtype=np.float32)
        self._check(self._L.lsq_get_unaries(self._h, X.ctypes.data, K.ctypes.data, d, n, m, h, U.ctypes.data))
        return U

    def get_binaries(self, K, m, h=H):
        K = _np(K, np.float32)
        d = K.shape[1]
        T = np.empty((m, m, h, h), dtype=np.float32)
        self._check(self._L.lsq_get_binaries(self._h, K.ctypes.data, d, m, h, T.ctypes.data))
        return T

    def veccost(self, X, B, K, m, h=H):
        X, K, B = _np(X, np.float32), _np(K, np.float32), _np(B, np.int16)
        n, d = X.shape
        self._check_shapes(X, K, B, m, h)
        out = np.empty(n, dtype=np.float32)
        self._check(self._L.lsq_veccost(self._h, X.ctypes.data, B.ctypes.data, K.ctypes.data, d, n, m, h, out.ctypes.data))
        return out

    def qerror(self, X, B, K, m, h=H):
        X, K, B = _np(X, np.float32), _np(K, np.float32), _np(B, np.int16)
        n, d = X.shape
        self._check_shapes(X, K, B, m, h)
        out = C.c_double(0.0)
        self._check(self._L.lsq_qerror(self._h, X.ctypes.data, B.ctypes.data, K.ctypes.data, d, n, m, h, C.byref(out)))
        return float(out.value)

    def perturb(self, B, npert, seed=0, it=0, global_offset=0, h=H):
        B = _np(B, np.int16).copy()
        n, m = B.shape
        self._check(self._L.lsq_perturb(self._h, B.ctypes.data, n, m, h, int(npert), int(seed), int(it), int(global_offset)))
        return B

    # -- (4) device generators -------------------------------------------------------------
    def synth_data_u8_dev(self, seed, n, d, device=None, global_offset=0):
        import torch
        X = torch.empty((n, d), dtype=torch.float32, device=device or ("cuda:%d" % self.device))
        with self._on_torch_stream():
            self._check(self._L.lsq_synth_data_u8_dev(self._h, int(seed), int(global_offset), n, d, X.data_ptr()))
        return X

    def randinit_dev(self, seed, n, m, device=None, global_offset=0, h=H):
        import torch
        B = torch.empty((n, m), dtype=torch.uint8, device=device or ("cuda:%d" % self.device))
        with self._on_torch_stream():
            self._check(self._L.lsq_randinit_dev(self._h, int(seed), int(global_offset), n, m, h, B.data_ptr()))
        return B

    def synth_codebooks_dev(self, seed, m, d, device=None, h=H):
        import torch
        K = torch.empty((m * h, d), dtype=torch.float32, device=device or ("cuda:%d" % self.device))
        with self._on_torch_stream():
            self._check(self._L.lsq_synth_codebooks_dev(self._h, int(seed), m, h, d, K.data_ptr()))
        return K

    @staticmethod
    def _check_shapes(X, K, B, m, h):
        n, d = X.shape
        if K.shape != (m * h, d):
            raise ValueError("K must be (m*h, d) = (%d, %d), got %s" % (m * h, d, K.shape))
        if B.shape != (n, m):
            raise ValueError("B must be (n, m) = (%d, %d), got %s" % (n, m, B.shape))


# -- the resident index (made by Engine.index / Engine.index_dev) --------------------------------

class Index:
    """A resident database on an Engine's device: the ADC scan (stage one) and the exact re-rank of its shortlists (stage two)   [lsq_index_*].
    Made by Engine.index (host arrays in and out) or Engine.index_dev (torch tensors in and out, on torch's current stream)."""

    def __init__(self, engine, codes, K, dbnorms, m, base, h, d, on_device):
        self._eng, self._L, self._dev, self._h = engine, engine._L, bool(on_device), None
        desc = _lib.IndexDesc()
        if self._dev:
            import torch
            for t, dt in ((codes, torch.uint8), (K, torch.float32), (dbnorms, torch.float32)):
                if t is not None:
                    assert t.is_cuda and t.dtype == dt and t.is_contiguous(), "contiguous device tensors required"
            if base is not None:
                assert base.is_cuda and base.dtype in (torch.float32, torch.uint8) and base.dim() == 2 and base.stride(1) == 1
            ptr = lambda t: t.data_ptr()      # noqa: E731
            u8 = base is not None and base.dtype == torch.uint8
            ldb = 0 if base is None else (base.stride(0) if base.shape[0] > 1 else base.shape[1])
        else:
            codes = None if codes is None else _np(codes, np.uint8)
            K = None if K is None else _np(K, np.float32)
            dbnorms = None if dbnorms is None else _np(dbnorms, np.float32)
            if base is not None:
                base, u8 = _x_host(base)
            else:
                u8 = False
            ptr = lambda a: a.ctypes.data      # noqa: E731
            ldb = 0 if base is None else base.shape[1]
        if codes is None and base is None:
            raise ValueError("an index needs codes, base rows or both")
        n = int(codes.shape[0] if codes is not None else base.shape[0])
        d = int(K.shape[1] if codes is not None else (d or base.shape[1]))
        if codes is not None and (tuple(codes.shape) != (n, m) or tuple(K.shape) != (m * h, d) or tuple(dbnorms.shape) != (n,)):
            raise ValueError("shape mismatch: codes %s K %s dbnorms %s m=%d h=%d" % (tuple(codes.shape), tuple(K.shape), tuple(dbnorms.shape), m, h))
        if base is not None and (base.shape[0] != n or base.shape[1] < d):
            raise ValueError("shape mismatch: base %s for n=%d d=%d" % (tuple(base.shape), n, d))
        desc.n, desc.d, desc.m, desc.h = n, d, int(m), int(h)
        desc.codes = ptr(codes) if codes is not None else None
        desc.codebooks = ptr(K) if codes is not None else None
        desc.dbnorms = ptr(dbnorms) if codes is not None else None
        desc.base = ptr(base) if base is not None else None
        desc.base_u8, desc.ldb, desc.on_device = int(u8), int(ldb), int(self._dev)
        self._keep = (codes, K, dbnorms, base)      # borrowed device tensors stay alive with the index
        self.n, self.d, self.m = n, d, int(m)
        handle = C.c_void_p()
        with self._stream():
            engine._check(self._L.lsq_index_create(C.byref(handle), engine._h, C.byref(desc)))
        self._h = handle
        engine._indexes.add(self)

    def _stream(self):
        return self._eng._on_torch_stream() if self._dev else contextlib.nullcontext()

    def _queries(self, Q):
        if self._dev:
            import torch
            assert Q.is_cuda and Q.dtype == torch.float32 and Q.dim() == 2 and Q.is_contiguous(), "contiguous device f32 queries required"
            return Q, Q.data_ptr()
        Q = _np(Q, np.float32)
        return Q, Q.ctypes.data

    def _outputs(self, nq, k, like):
        if self._dev:
            import torch
            dists = torch.empty((nq, k), dtype=torch.float32, device=like.device)
            ids = torch.empty((nq, k), dtype=torch.int32, device=like.device)
            return dists, ids, dists.data_ptr(), ids.data_ptr()
        dists, ids = np.zeros((nq, k), dtype=np.float32), np.zeros((nq, k), dtype=np.int32)
        return dists, ids, dists.ctypes.data, ids.ctypes.data

    def search(self, Q_scan, k, shortlist=0, Q_exact=None):
        """Q_scan (nq,d): what the scan reads (the rotated queries of linscan_lsq); Q_exact (nq,d): the queries in the base set's own frame (default:
        Q_scan).  shortlist=0: the ADC scan alone, Engine.linscan's results; shortlist=L>=k: scan for L, re-rank to k by exact distance.
        -> dists (nq,k) float32 ascending, ids (nq,k) int32 1-BASED   [lsq_index_search]"""
        Qs, ps = self._queries(Q_scan)
        Qe, pe = self._queries(Q_exact) if Q_exact is not None else (Qs, ps)
        if tuple(Qe.shape) != tuple(Qs.shape) or Qs.shape[1] != self.d:
            raise ValueError("shape mismatch: Q_scan %s Q_exact %s d=%d" % (tuple(Qs.shape), tuple(Qe.shape), self.d))
        nq = Qs.shape[0]
        dists, ids, pd, pi = self._outputs(nq, int(k), Qs)
        with self._stream():
            self._eng._check(self._L.lsq_index_search(self._h, pd, pi, ps, pe, nq, self.d, int(shortlist), int(k), int(self._dev)))
        return dists, ids

    def rerank(self, Q, cand, k, id_base=1):
        """Stage two alone: cand (nq,L) int32 ids in id_base (the 0-based shortlists of linscan_pq: id_base=0).
        -> dists (nq,k) float32 exact, ascending, ids (nq,k) int32 in id_base; an id outside the base comes last as (+inf, id_base-1)   [lsq_index_rerank]"""
        Q, pq = self._queries(Q)
        if self._dev:
            import torch
            assert cand.is_cuda and cand.dtype == torch.int32 and cand.dim() == 2 and cand.is_contiguous(), "contiguous device int32 candidates required"
            pc = cand.data_ptr()
        else:
            cand = _np(cand, np.int32)
            pc = cand.ctypes.data
        if cand.ndim != 2 or cand.shape[0] != Q.shape[0] or Q.shape[1] != self.d:
            raise ValueError("shape mismatch: Q %s cand %s d=%d" % (tuple(Q.shape), tuple(cand.shape), self.d))
        nq, L = cand.shape
        dists, ids, pd, pi = self._outputs(nq, int(k), Q)
        with self._stream():
            self._eng._check(self._L.lsq_index_rerank(self._h, pd, pi, pq, pc, nq, self.d, int(L), int(k), int(id_base), int(self._dev)))
        return dists, ids

    def knn(self, Q, k, id_base=0):
        """Exact k-NN over the resident base rows (f32, or uint8 never widened): the ground truth of a recall figure.  Q (nq,>=d) float32 or uint8 rows
        with unit column stride, any row pitch and byte offset (numpy on an Engine.index, torch on an Engine.index_dev); the first d columns are read.
        -> dists (nq,k) float32 ascending with lsq_knn_exact's bits, ids (nq,k) int32 in id_base; ties by smaller id   [lsq_index_knn]"""
        u8 = _is_u8(Q)
        if self._dev:
            import torch
            assert Q.is_cuda and Q.dtype in (torch.float32, torch.uint8) and Q.dim() == 2 and Q.stride(1) == 1, "device f32 / uint8 query rows required"
            ldq, pq = (Q.stride(0) if Q.shape[0] > 1 else Q.shape[1]), Q.data_ptr()
        else:
            Q = np.asarray(Q)
            if Q.dtype != np.uint8:
                Q = np.asarray(Q, dtype=np.float32)
            if Q.ndim != 2 or Q.strides[1] != Q.itemsize or Q.strides[0] % Q.itemsize or (Q.shape[0] > 1 and Q.strides[0] < Q.shape[1] * Q.itemsize):
                Q = np.ascontiguousarray(Q)
            ldq, pq = (Q.strides[0] // Q.itemsize if Q.shape[0] > 1 else Q.shape[1]), Q.ctypes.data
        if Q.ndim != 2 or Q.shape[1] < self.d:
            raise ValueError("shape mismatch: Q %s d=%d" % (tuple(Q.shape), self.d))
        nq = Q.shape[0]
        dists, ids, pd, pi = self._outputs(nq, int(k), Q)
        with self._stream():
            self._eng._check(self._L.lsq_index_knn(self._h, pd, pi, pq, int(u8), nq, int(ldq), int(k), int(id_base), int(self._dev)))
        return dists, ids

    def knn_info(self):
        """what the last knn call did: queries, rows, batches, fallback_queries, exhaustive, int_road, norms_ms / scan_ms / select_ms (with profile=True)"""
        st = _lib.IndexKnnInfo()
        self._eng._check(self._L.lsq_index_get_knn_info(self._h, C.byref(st)))
        return st.as_dict()

    def stats(self):
        st = _lib.IndexStats()
        self._eng._check(self._L.lsq_index_get_stats(self._h, C.byref(st)))
        return st.as_dict()

    def close(self):
        # Engine.close closes its indexes first.  Should the context be gone all the same, the handle is dropped, not destroyed: lsq_index_destroy would
        # reach through the freed context, and lsq_destroy knows nothing of the index's buffers, which then stay allocated until the process ends.
        if getattr(self, "_h", None) and getattr(self._eng, "_h", None):
            self._L.lsq_index_destroy(self._h)
        self._h = None
        self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# -- host-only pieces of the path (no GPU needed) ---------------------------------------------

def cover_bytes(dim2C, d, m):
    """A cover map given as a (d, m) array of 0 / 1 (the reference's dim2C, codebook_update.jl:134-136) -> the bytes the C-ABI reads: Julia's column-major
    d x m, i.e. a contiguous (m, d) uint8 array.  Values are passed on as they are (the library rejects anything but 0 and 1)."""
    a = np.asarray(dim2C)
    if a.shape != (d, m):
        raise ValueError("dim2C must be (d, m) = (%d, %d), got %s" % (d, m, a.shape))
    return np.ascontiguousarray(a.T.astype(np.uint8))


def check_spgl1_args(xshape, bshape, m, h, tau, S, kshape=None, opt_tol=None, max_iter=None):
    """The argument rules of lsq_update_codebooks_spgl1, checked before any device is touched: X (n, d), codes (n, m), K_init (m h, d)."""
    import math
    if len(xshape) != 2 or xshape[0] < 1 or xshape[1] < 1:
        raise ValueError("X must be (n, d) with n, d >= 1, got %s" % (tuple(xshape),))
    n, d = xshape
    if not (isinstance(m, (int, np.integer)) and 1 <= m <= 16):
        raise ValueError("m=%r must be an integer in 1..16" % (m,))
    if h != H:
        raise ValueError("h=%r unsupported: h must be 256" % (h,))
    if tuple(bshape) != (n, m):
        raise ValueError("codes must be (n, m) = (%d, %d), got %s" % (n, m, tuple(bshape)))
    try:
        t = float(tau)
    except (TypeError, ValueError):
        raise ValueError("tau=%r must be a number" % (tau,))
    if math.isnan(t) or t < 0:
        raise ValueError("tau=%r must be a number >= 0" % (tau,))
    if not isinstance(S, (int, np.integer)) or isinstance(S, bool):
        raise ValueError("S=%r must be an integer (< 0: no threshold)" % (S,))
    if kshape is not None and tuple(kshape) != (m * h, d):
        raise ValueError("K_init must be (m*h, d) = (%d, %d), got %s" % (m * h, d, tuple(kshape)))
    if opt_tol is not None and not (0 < float(opt_tol) < 1):
        raise ValueError("opt_tol=%r must lie in (0, 1)" % (opt_tol,))
    if max_iter is not None and int(max_iter) < 1:
        raise ValueError("max_iter=%r must be >= 1" % (max_iter,))


def randinit(n, m, h=H, seed=0, global_offset=0):
    """initializations.jl:2-8 -> (n, m) int16 1-based (Philox-keyed, shard-invariant)."""
    B = np.empty((n, m), dtype=np.int16)
    _lib.check(_lib.load().lsq_randinit(int(seed), int(global_offset), n, m, h, B.ctypes.data))
    return B


def node_order(seed, it, m, randord=True):
    o = np.empty(m, dtype=np.int32)
    _lib.check(_lib.load().lsq_node_order(int(seed), int(it), m, int(bool(randord)), o.ctypes.data))
    return o


class MultiEngine:
    """Single-process multi-GPU handle (lsq_multi_*): one context + host thread per listed device, `splitarray` shards,
    results identical to the one-device call.  `encode_icm` has Engine.encode_icm's signature, so the reference-shaped
    functions accept it as `engine=`:  encode_icm_cuda(RX, B, C, ..., engine=MultiEngine([0, 1, 2, 3]))."""

    def __init__(self, devices, **options):
        self._L = _lib.load()
        devs = np.ascontiguousarray(list(devices), dtype=np.int32)
        h = C.c_void_p()
        _lib.check(self._L.lsq_multi_create(C.byref(h), devs.ctypes.data, int(devs.shape[0])))
        self._h = h
        self.devices = [int(x) for x in devs]
        for k, v in options.items():
            self.set_option(k, v)

    def set_option(self, key, value):
        _lib.check(self._L.lsq_multi_set_option(self._h, key.encode(), int(value)))

    def encode_icm(self, X, B, K, m, ilsiters, icmiter, npert, randord, seed=0, nsplits=1, global_offset=0,
                   verbose=False, h=H):
        """-> Bs (nr, n, m) int16 1-based, objs (nr,) float32   [lsq_multi_encode_icm; uint8 X: lsq_multi_encode_icm_u8]"""
        X, u8 = _x_host(X)
        K, B = _np(K, np.float32), _np(B, np.int16)
        n, d = X.shape
        if B.shape != (n, m) or K.shape != (m * h, d):
            raise ValueError("shape mismatch: X %s B %s K %s m=%d h=%d" % (X.shape, B.shape, K.shape, m, h))
        ils = _np(ilsiters, np.int64).reshape(-1)
        nr = ils.shape[0]
        Bs = np.empty((nr, n, m), dtype=np.int16)
        objs = np.zeros(nr, dtype=np.float32)
        call = self._L.lsq_multi_encode_icm_u8 if u8 else self._L.lsq_multi_encode_icm
        _lib.check(call(self._h, X.ctypes.data, B.ctypes.data, K.ctypes.data, d, n, m, h,
                                                ils.ctypes.data, nr, int(icmiter), int(npert), int(bool(randord)),
                                                int(seed), int(global_offset), int(bool(verbose)), Bs.ctypes.data, objs.ctypes.data))
        return Bs, objs

    def linscan(self, codes, Q, K, dbnorms, m, k, h=H):
        """the ADC scan over a database sharded across the devices; Engine.linscan's signature and results   [lsq_multi_linscan]"""
        codes, Q, K, dbn = _np(codes, np.uint8), _np(Q, np.float32), _np(K, np.float32), _np(dbnorms, np.float32)
        n, nq, d = codes.shape[0], Q.shape[0], Q.shape[1]
        if codes.shape != (n, m) or K.shape != (m * h, d) or dbn.shape != (n,):
            raise ValueError("shape mismatch: codes %s Q %s K %s dbnorms %s m=%d h=%d" % (codes.shape, Q.shape, K.shape, dbn.shape, m, h))
        dists = np.zeros((nq, k), dtype=np.float32)
        ids = np.zeros((nq, k), dtype=np.int32)
        _lib.check(self._L.lsq_multi_linscan(self._h, dists.ctypes.data, ids.ctypes.data, codes.ctypes.data, Q.ctypes.data, K.ctypes.data,
                                             dbn.ctypes.data, nq, n, m, h, d, int(k)))
        return dists, ids

    def close(self):
        if self._h is not None and self._h.value:
            self._L.lsq_multi_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def splitarray(n, nparts):
    """utils.jl:152-177 -> list of (start, stop) 0-based half-open ranges."""
    L = _lib.load()
    out = []
    for p in range(nparts):
        s, ln = C.c_int64(), C.c_int64()
        _lib.check(L.lsq_splitarray(n, nparts, p, C.byref(s), C.byref(ln)))
        out.append((s.value, s.value + ln.value))
    return out


def device_count():
    c = C.c_int(0)
    rc = _lib.load().lsq_device_count(C.byref(c))
    return c.value if rc == 0 else 0
