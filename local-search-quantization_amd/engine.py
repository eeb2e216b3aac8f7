"""Engine: thin, typed Python handle on the C-ABI context (one per process / per GPU).

Row-major conventions (the Julia buffers seen from numpy, see include/lsq_mi355x.h):
    X (n, d) float32 | K (m*h, d) float32 | B (n, m) int16 1-based (host) / uint8 0-based (device)
    X (n, d) uint8 (the encode calls only: .bvecs base sets stay 8-bit end to end, the lsq_*_u8 entry points)
torch is used only as the owner of device memory and streams; every computation happens inside
liblsq_mi355x.so.
"""
import contextlib
import ctypes as C
import os
import weakref

import numpy as np

from . import _lib

H = 256
IT_AUTO = 0xFFFFFFFF      # LSQ_IT_AUTO: the context counts the ILS iterations of the CPU-shaped entry points
_F32, _U8, _I16, _I32, _I64 = np.float32, np.uint8, np.int16, np.int32, np.int64
_NOTHING = contextlib.nullcontext()


def _dtname(a):
    """the element type of a numpy array or a torch tensor by name ("uint8", "float32", ...); "" for anything else"""
    return str(getattr(a, "dtype", "")).replace("torch.", "")


def _array_address(a):
    return None if a is None else a.ctypes.data


def _tensor_address(t):
    return None if t is None else t.data_ptr()


class _Side:
    """One side of a host / _dev pair of entry points: how an argument is taken, where an output is made, which address the library gets and what the
    call runs under.  _HOST converts (numpy, C-contiguous, the element type asked for); _DEVICE reads the caller's torch tensors in place, so it
    verifies and raises -- it never converts, and what it refuses never reaches a kernel as an address."""

    def __init__(self, dev):
        self.dev, self.suffix = dev, "_dev" if dev else ""
        self.codes = _U8 if dev else _I16          # B: 0-based bytes on the device, 1-based int16 on the host
        self.ptr = _tensor_address if dev else _array_address      # the address the library gets; None stays None

    def take(self, a, dtype, name, rows=False):
        """an input.  rows=True: a device form that reads row views in place asks only for 2-d with unit column stride, not for contiguity"""
        if not self.dev:
            return np.ascontiguousarray(a, dtype=dtype)
        if not getattr(a, "is_cuda", False):
            raise TypeError("%s must be a device tensor, got %s" % (name, "a CPU tensor" if hasattr(a, "is_cuda") else type(a).__name__))
        if _dtname(a) != dtype.__name__:
            raise TypeError("%s must be %s, got %s" % (name, dtype.__name__, _dtname(a)))
        if rows and (a.dim() != 2 or a.stride(1) != 1):
            raise ValueError("%s must be 2-d rows with unit column stride, got shape %s strides %s" % (name, tuple(a.shape), a.stride()))
        if not rows and not a.is_contiguous():
            raise ValueError("%s must be contiguous, got shape %s strides %s" % (name, tuple(a.shape), a.stride()))
        return a

    def maybe(self, a, dtype, name):
        return None if a is None else self.take(a, dtype, name)

    def take_x(self, X, name, rows=False):
        """rows of data -> (array, is_u8).  uint8 (the bytes of a .bvecs set) stays uint8 and takes the 8-bit entry points; int8 is refused (those bytes
        are unsigned: a signed view would encode other vectors); anything else is float32 -- converted on the host, required on the device."""
        dt = _dtname(X)
        if dt == "int8":
            raise TypeError("int8 data is not accepted: 8-bit base sets are unsigned (uint8); view or convert the array explicitly")
        return self.take(X, _U8 if dt == "uint8" else _F32, name, rows), dt == "uint8"

    def new(self, shape, dtype, like=None, zero=False):
        """an output, on the device of the tensor (or the device) `like`.  zero: a host output starts at zero; a device output is never cleared here"""
        if not self.dev:
            return (np.zeros if zero else np.empty)(shape, dtype=dtype)
        import torch
        return torch.empty(shape, dtype=getattr(torch, dtype.__name__), device=getattr(like, "device", like))

    def out(self, out, shape, dtype, like, name="out", zero=False):
        """the caller's `out` (device forms only), verified like an input, or a new output; its shape is the caller's line in _shapes"""
        return self.new(shape, dtype, like, zero) if out is None else self.take(out, dtype, name)

    def topk(self, nq, k, like, ids=_I32):
        """(dists, ids) of a search: (nq, k) float32 and int32 (uint32 where a host form says so)"""
        return self.new((nq, k), _F32, like, zero=True), self.new((nq, k), ids, like, zero=True)

    def pitch(self, a):
        """elements between the rows of a 2-d array (a single row: its width)"""
        if a.shape[0] <= 1:
            return a.shape[1]
        return a.stride(0) if self.dev else a.strides[0] // a.itemsize

    def stream(self, engine):
        return engine._on_torch_stream() if self.dev else _NOTHING


_HOST, _DEVICE = _Side(False), _Side(True)

# half-precision base rows (Engine.index(..., base_format=), Index.narrow_base): name -> (the library's format, the dtype a host array of such rows has --
# bfloat16 travels as the uint16 BITS, numpy has no such type --, the dtype of a device tensor)
_HALF = {"f16": (_lib.BASE_F16, np.float16, "float16"), "bf16": (_lib.BASE_BF16, np.uint16, "bfloat16")}
_HALF_BY_CODE = {v[0]: (k,) + v[1:] for k, v in _HALF.items()}
_FORMAT_NAMES = {_lib.BASE_F32: "float32", _lib.BASE_U8: "uint8", _lib.BASE_F16: "float16", _lib.BASE_BF16: "bfloat16"}


def base_format_code(fmt):
    """None -> None, "f16" / "bf16" -> LSQ_BASE_F16 / LSQ_BASE_BF16; anything else is a ValueError (raised before any library call)"""
    if fmt is None:
        return None
    if not isinstance(fmt, str) or fmt not in _HALF:
        raise ValueError("base_format must be None, \"f16\" or \"bf16\", got %r" % (fmt,))
    return _HALF[fmt][0]


def _row_view(a, dtype):
    """a 2-d host array as rows with unit column stride and a pitch of whole elements, read in place where it already is that"""
    a = np.asarray(a, dtype=dtype)
    if a.ndim != 2 or a.strides[1] != a.itemsize or a.strides[0] % a.itemsize or (a.shape[0] > 1 and a.strides[0] < a.shape[1] * a.itemsize):
        a = np.ascontiguousarray(a)
    return a


def _host_half_rows(L, check, base, code):
    """host rows for a half-precision base of format `code`: rows already in the format are taken as they are (float16 for "f16", the uint16 bits for
    "bf16"), float rows are narrowed by lsq_narrow_rows_cpu (round to nearest even); any other dtype is a TypeError, raised before any library call"""
    name, np_dtype, _ = _HALF_BY_CODE[code]
    dt = _dtname(base)
    if dt == np.dtype(np_dtype).name:
        return _row_view(base, np_dtype)
    if dt == "int8":
        raise TypeError("int8 data is not accepted: 8-bit base sets are unsigned (uint8); view or convert the array explicitly")
    if not (dt.startswith("float") or dt == ""):
        raise TypeError("base rows for base_format=%r must be float rows to narrow or %s rows%s, got %s" % (
            name, np.dtype(np_dtype).name, " holding the bfloat16 bits" if code == _lib.BASE_BF16 else "", dt))
    X = _row_view(base, _F32)
    n, d = X.shape
    out = np.zeros((n, d), dtype=np.uint16)
    check(L.lsq_narrow_rows_cpu(out.ctypes.data, X.ctypes.data, n, d, int(_HOST.pitch(X)), d, code, 0))
    return out.view(np_dtype)


def _device_half_rows(base, code, name="base"):
    """a device tensor of base rows under base_format `code` (None: the dtype alone decides) -> (tensor, its format, the format to narrow to afterwards or
    None).  float16 / bfloat16 tensors are borrowed as they are and a contradicting base_format is a TypeError; a float32 tensor with a format is taken as
    float32 and narrowed on the device once the index exists"""
    if not getattr(base, "is_cuda", False):
        raise TypeError("%s must be a device tensor, got %s" % (name, "a CPU tensor" if hasattr(base, "is_cuda") else type(base).__name__))
    dt = _dtname(base)
    have = {"float16": _lib.BASE_F16, "bfloat16": _lib.BASE_BF16}.get(dt)
    if have is not None:
        if code is not None and code != have:
            raise TypeError("%s is a %s tensor, which contradicts base_format=%r" % (name, dt, _HALF_BY_CODE[code][0]))
        if base.dim() != 2 or base.stride(1) != 1:
            raise ValueError("%s must be 2-d rows with unit column stride, got shape %s strides %s" % (name, tuple(base.shape), base.stride()))
        return base, have, None
    if code is not None and dt != "float32":
        raise TypeError("%s must be float32 (narrowed on the device), float16 or bfloat16 for base_format=%r, got %s" % (name, _HALF_BY_CODE[code][0], dt))
    base, u8 = _DEVICE.take_x(base, name, rows=True)
    return base, _lib.BASE_U8 if u8 else _lib.BASE_F32, code


def _fits(shape, want):
    return len(shape) == len(want) and all(w is None or w == s for s, w in zip(shape, want))


def _shapes(*items):
    """items (name, array or None, expected shape; None: any extent).  One mismatch -> ValueError naming every argument, the shape it has and the one it should have"""
    for _, a, want in items:
        if a is not None and tuple(a.shape) != want and not _fits(tuple(a.shape), want):
            raise ValueError("shape mismatch: " + ", ".join("%s %s, expected %s" % (nm, tuple(b.shape), tuple("*" if w is None else w for w in sh))
                                                            for nm, b, sh in items if b is not None))


def _encode_args(side, X, B, K, m, h, ilsiters):
    """what every whole-call encode reads -> X, is_u8, B, K, n, d, the ILS iteration counts as int64"""
    X, u8 = side.take_x(X, "X")
    B, K = side.take(B, side.codes, "B"), side.take(K, _F32, "K")
    n, d = X.shape
    _shapes(("X", X, (n, d)), ("B", B, (n, m)), ("K", K, (m * h, d)))
    return X, u8, B, K, n, d, _HOST.take(ilsiters, _I64, "ilsiters").reshape(-1)


def _linscan_args(side, codes, Q, K, dbnorms, m, k, h):
    """the ADC scan's arguments -> (dists, ids), the argument list after the handle (Engine's two forms and MultiEngine's differ in the symbol alone)"""
    codes, Q, K, dbn = side.take(codes, _U8, "codes"), side.take(Q, _F32, "Q"), side.take(K, _F32, "K"), side.take(dbnorms, _F32, "dbnorms")
    n, nq, d = codes.shape[0], Q.shape[0], Q.shape[1]
    _shapes(("codes", codes, (n, m)), ("Q", Q, (nq, d)), ("K", K, (m * h, d)), ("dbnorms", dbn, (n,)))
    dists, ids = side.topk(nq, k, Q)
    p = side.ptr
    return (dists, ids), (p(dists), p(ids), p(codes), p(Q), p(K), p(dbn), nq, n, m, h, d, int(k))


class Engine:
    def __init__(self, device=0, chunk=None, profile=False, schedule=None, skip=None, tuning=False):
        """tuning=True loads liblsq_mi355x_tuning.so (same ABI + option "ablation", environment knobs, clock stamps)."""
        self._L = _lib.load(tuning=tuning)
        h = C.c_void_p()
        self._check(self._L.lsq_create(C.byref(h), int(device)))
        self._h = h
        self._indexes = weakref.WeakSet()             # the handles made on this context (Index, Encoder objects): closed before it
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
            for ix in list(getattr(self, "_indexes", ())):      # an index or encoder needs its context to free what it holds on the device
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
        self._call(_HOST, "lsq_get_timings_sized", C.addressof(t), C.sizeof(t))      # size-checked: this binding and the library may be of different versions
        return t.as_dict()

    def walk_trace(self, count=64):
        """recomputed node updates per position (sweep * m + rank in the visiting order) since reset_timings  [lsq_get_walk_trace]"""
        out = np.zeros(count, dtype=np.int64)
        self._call(_HOST, "lsq_get_walk_trace", out.ctypes.data, int(count))
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
        self._call(_HOST, "lsq_get_q16_snapshot", _lib.SNAP_PARAMS, C.addressof(P), C.sizeof(P), info.ctypes.data)
        cn, row0, m, slq, slf, filtered = (int(v) for v in info)
        shapes = {"Uq": (_lib.SNAP_UQ, torch.int16, (m, H // slq, cn, slq)), "Tq": (_lib.SNAP_TQ, torch.int16, (m, H // slq, (m - 1) * H, slq)),
                  "qflag": (_lib.SNAP_QFLAG, torch.int16, (cn,)), "U": (_lib.SNAP_U, torch.float32, (m, H // slf, cn, slf)),
                  "T": (_lib.SNAP_T, torch.float32, (m, m, H, H))}
        out = {"rows": cn, "row0": row0, "m": m, "slq": slq, "slf": slf, "filtered": bool(filtered)}
        for name, (what, dtype, shape) in shapes.items():
            t = torch.empty(shape, dtype=dtype, device=self._device())
            self._call(_HOST, "lsq_get_q16_snapshot", what, t.data_ptr(), t.numel() * t.element_size(), None)
            out[name] = t
        self.synchronize()
        nodes = [P.node[j] for j in range(m)]
        out["params"] = {"ok": int(P.ok), "oor": int(P.oor), "nflag": int(P.nflag),
                         "loU": np.array([q.loU for q in nodes], dtype=np.float32), "invD": np.array([q.invD for q in nodes], dtype=np.float32),
                         "D": np.array([q.D for q in nodes], dtype=np.float32), "hiq": np.array([q.hiq for q in nodes], dtype=np.float32),
                         "window": np.array([q.window for q in nodes], dtype=np.int64), "slack": np.array([q.slack for q in nodes], dtype=np.float64)}
        return out

    # -- one call path: every entry point below is `_call(side, symbol, arguments after the handle)` ------------------------------
    def _call(self, side, sym, *args, h=None, under=None):
        """The one way into the library: under the side's context (nothing on the host; torch's current stream bound for the call's duration on the
        device; `under`: a wrapper of it) call `sym` with the handle first (h: an index's; default the context's) and raise LsqError on a non-zero
        return code."""
        with under or side.stream(self):
            return self._check(getattr(self._L, sym)(self._h if h is None else h, *args))

    @contextlib.contextmanager
    def _nonblocking(self):
        """the device side's context with option "async" set for the one call inside it"""
        with self._on_torch_stream():
            self.set_option("async", 1)
            try:
                yield
            finally:
                self.set_option("async", 0)

    def _device(self, device=None):
        return device or ("cuda:%d" % self.device)

    # -- (1) whole call, host buffers -------------------------------------------------------
    def encode_icm(self, X, B, K, m, ilsiters, icmiter, npert, randord, seed=0, nsplits=1, global_offset=0,
                   verbose=False, h=H):
        """-> Bs (nr, n, m) int16 1-based, objs (nr,) float32   [lsq_encode_icm; uint8 X: lsq_encode_icm_u8, the rows stay 8-bit]"""
        X, u8, B, K, n, d, ils = _encode_args(_HOST, X, B, K, m, h, ilsiters)
        nr, p = ils.shape[0], _HOST.ptr
        Bs, objs = _HOST.new((nr, n, m), _I16), _HOST.new(nr, _F32, zero=True)
        self._call(_HOST, "lsq_encode_icm_u8" if u8 else "lsq_encode_icm", p(X), p(B), p(K), d, n, m, h, p(ils), nr, int(icmiter), int(npert),
                   int(bool(randord)), int(nsplits), int(seed), int(global_offset), int(bool(verbose)), p(Bs), p(objs))
        return Bs, objs

    # -- (1b) whole call, device-resident torch tensors -------------------------------------
    def encode_icm_dev(self, dX, dB0, dK, m, ilsiters, icmiter, npert, randord, seed=0, global_offset=0,
                       out=None, h=H, nonblocking=False):
        """dX (n,d) f32 or uint8 (8-bit rows: lsq_encode_icm_u8_dev, any byte offset into a larger buffer), dB0 (n,m) u8 0-based, dK (m*h,d) f32:
        CUDA/HIP torch tensors.
        -> dBs (nr, n, m) uint8 tensor, obj_sums (nr,) float64 numpy (SUM of costs), stats (I, 2) int64.
        nonblocking=True (option "async"): nothing in the call waits for the device; obj_sums and stats come back as DEVICE tensors, valid after the
        caller has synchronised torch's current stream (the call can be captured into a graph from its second use on a shape on)."""
        dX, u8, dB0, dK, n, d, ils = _encode_args(_DEVICE, dX, dB0, dK, m, h, ilsiters)
        nr, I, p = ils.shape[0], int(ils.max()), _DEVICE.ptr
        dBs = _DEVICE.out(out, (nr, n, m), _U8, dX)
        if out is not None:                               # any shape that holds the nr * n * m bytes, as ever
            _shapes(("out (flat)", out.reshape(-1), (nr * n * m,)))
        sums = _DEVICE if nonblocking else _HOST          # the sums and the statistics: where nothing may wait, they stay on the device
        obj, stats = sums.new(nr, np.float64, dX, zero=True), sums.new((I, 2), _I64, dX, zero=True)
        if nonblocking:
            obj.zero_()
            stats.zero_()
        self._call(_DEVICE, "lsq_encode_icm_u8_dev" if u8 else "lsq_encode_icm_dev", p(dX), p(dB0), p(dK), d, n, m, h, ils.ctypes.data, nr,
                   int(icmiter), int(npert), int(bool(randord)), int(seed), int(global_offset), p(dBs), sums.ptr(obj), sums.ptr(stats),
                   under=self._nonblocking() if nonblocking else None)
        return dBs, obj, stats

    # -- (1c) the search step after the path: ADC linear scan on the device ------------------
    def linscan(self, codes, Q, K, dbnorms, m, k, h=H):
        """codes (n,m) uint8 0-based, Q (nq,d), K (m*h,d), dbnorms (n,): host arrays.
        -> dists (nq,k) float32 ascending, ids (nq,k) int32 1-BASED   [lsq_linscan]"""
        return self._linscan(_HOST, codes, Q, K, dbnorms, m, k, h)

    def linscan_dev(self, dcodes, dQ, dK, dnorms, m, k, h=H):
        """The same on device-resident torch tensors -> (dists (nq,k) f32, ids (nq,k) int32 1-based) tensors   [lsq_linscan_dev]"""
        return self._linscan(_DEVICE, dcodes, dQ, dK, dnorms, m, k, h)

    def _linscan(self, side, *args):
        result, cargs = _linscan_args(side, *args)
        self._call(side, "lsq_linscan" + side.suffix, *cargs)
        return result

    def linscan_pq(self, codes, Q, C3, m, k, subdim):
        """PQ / OPQ codes, no norm term.  codes (n, dim1codes) uint8 0-based (the first m bytes of a row used), Q (nq, dim1queries),
        C3 (m, 256, subdim) centres (any shape holding m*256*subdim floats): host arrays.
        -> dists (nq,k) float32 ascending, ids (nq,k) uint32 0-BASED   [lsq_linscan_pq]"""
        return self._linscan_pq(_HOST, codes, Q, C3, m, k, subdim)

    def linscan_pq_dev(self, dcodes, dQ, dC3, m, k, subdim):
        """The same on device-resident torch tensors -> (dists (nq,k) f32, ids (nq,k) 0-based) tensors; torch has no uint32 arithmetic, so the
        ids tensor is int32 holding the uint32 bits (every id is below 2^31)   [lsq_linscan_pq_dev]"""
        return self._linscan_pq(_DEVICE, dcodes, dQ, dC3, m, k, subdim)

    def _linscan_pq(self, side, codes, Q, C3, m, k, subdim):
        codes, Q, C3 = side.take(codes, _U8, "codes"), side.take(Q, _F32, "Q"), side.take(C3, _F32, "C3")
        _shapes(("codes", codes, (None, None)), ("Q", Q, (None, None)), ("C3 (flat)", C3.reshape(-1), (m * H * subdim,)))
        (n, dc), (nq, dq), p = codes.shape, Q.shape, side.ptr
        dists, ids = side.topk(nq, k, Q, ids=_I32 if side.dev else np.uint32)
        self._call(side, "lsq_linscan_pq" + side.suffix, p(dists), p(ids), p(codes), p(C3), p(Q), n, nq, 8 * m, int(k), dc, dq, int(subdim))
        return dists, ids

    def knn_exact(self, Xb, Xq, k):
        """Exact k-NN (the ground truth of a recall figure).  Xb (n, d) base rows, Xq (nq, d) queries: host arrays, float32 -- or a uint8 base (the
        un-widened rows of a .bvecs set) with uint8 or float queries, which goes through a temporary base-only Index and is never widened.
        -> dists (nq,k) float32 ascending, ids (nq,k) uint32 0-BASED; ties by smaller id, NaN last   [lsq_knn_exact / lsq_index_knn]"""
        return self._knn_exact(_HOST, Xb, Xq, k)

    def knn_exact_dev(self, dXb, dXq, k):
        """The same on device-resident torch tensors (n, d) / (nq, d), f32 -- or a uint8, float16 or bfloat16 base with uint8 or f32 queries (a temporary
        Index that borrows the base: the bits of the call on the widened base); row views with unit column stride are read in place.
        -> (dists (nq,k) f32, ids (nq,k) 0-based) tensors; the ids tensor is int32 holding the uint32 bits   [lsq_knn_exact_dev / lsq_index_knn]"""
        return self._knn_exact(_DEVICE, dXb, dXq, k)

    def _knn_exact(self, side, Xb, Xq, k):
        u8 = _dtname(Xb) == "uint8" or (side.dev and _dtname(Xb) in ("float16", "bfloat16"))      # never widened: the temporary base-only Index
        if not u8:
            Xb, Xq = side.take(Xb, _F32, "base", rows=True), side.take(Xq, _F32, "queries", rows=True)
        _shapes(("base", Xb, (None, None)), ("queries", Xq, (None, Xb.shape[-1])))
        if u8:                                           # the base is never widened: a temporary base-only Index (it takes its own arguments)
            if side.dev:
                side.take_x(Xq, "queries", rows=True)    # refused before the index is made, not after
            with Index(self, None, None, None, 0, Xb, H, None, on_device=side.dev) as ix:
                dists, ids = ix.knn(Xq, k)
            return dists, ids if side.dev else ids.view(np.uint32)
        (n, d), nq, p = Xb.shape, Xq.shape[0], side.ptr
        if side.dev:                                     # row views are read in place, each at its own pitch
            for t in (Xb, Xq):
                if t.shape[0] > 1 and t.stride(0) < d:
                    raise ValueError("rows must be unit-stride and at least d floats apart (got strides %s)" % (t.stride(),))
        dists, ids = side.topk(nq, k, Xq, ids=_I32 if side.dev else np.uint32)
        self._call(side, "lsq_knn_exact" + side.suffix, p(dists), p(ids), p(Xb), p(Xq), n, nq, d, side.pitch(Xb), side.pitch(Xq), int(k))
        return dists, ids

    # -- (1d) two-stage search on a resident index ------------------------------------------
    def index(self, codes, K, dbnorms, m, base=None, h=H, d=None, base_format=None):
        """An Index of HOST arrays, copied once and owned by the index: codes (n,m) uint8 0-based, K (m*h,d), dbnorms (n,), base (n,ldb) float32 or
        uint8 (the un-widened rows of a .bvecs set) or None (scan only).  codes=None: a base-only index (re-rank only), which reads the first d
        components of a base row (default: all of them).  base_format="f16" / "bf16": the index keeps HALF-PRECISION base rows (2 d bytes per row): float
        rows are narrowed on the host, round to nearest even (narrow_rows); a float16 array ("f16") or a uint16 array of bfloat16 bits ("bf16") is taken
        as it is.  Every call that reads base rows then returns what the index over the widened rows returns.  base_format=None: as ever -- a float16 array
        is widened to float32   [lsq_index_create]"""
        return Index(self, codes, K, dbnorms, m, base, h, d, on_device=False, base_format=base_format)

    def index_dev(self, dcodes, dK, dnorms, m, base=None, h=H, d=None, base_format=None):
        """The same on device-resident torch tensors, BORROWED: the index keeps references to them; searches take and return tensors.  base: a 2-d
        tensor or a view of one with unit column stride, at any byte offset.  A torch.float16 or torch.bfloat16 base is borrowed as it is (the dtype
        decides; a contradicting base_format is a TypeError); a float32 base with base_format="f16" / "bf16" is narrowed on the device into rows the index
        owns (Index.narrow_base) and is not kept."""
        return Index(self, dcodes, dK, dnorms, m, base, h, d, on_device=True, base_format=base_format)

    def index_packed(self, codes, K, norm_codes, cbnorms, m, base=None, h=H, base_format=None):
        """An Index that keeps the norm BYTE: codes (n,m) uint8 0-based, norm_codes (n,) uint8 0-based indexes into cbnorms (<= 256,) float32 -- what
        quantize_norms computes -- packed into rows of m + 1 bytes that the index owns.  Every search returns the bits of Engine.index(codes, K,
        cbnorms[norm_codes], m, base)   [lsq_index_create_packed]"""
        return Index(self, codes, K, None, m, base, h, None, on_device=False, packed=(norm_codes, cbnorms), base_format=base_format)

    def index_packed_dev(self, dcodes, dK, dnorm_codes, dcbnorms, m, base=None, h=H, base_format=None):
        """The same from device tensors (quantize_norms_dev's idx as it is).  dcodes, dnorm_codes and dcbnorms are read once, before this returns: they
        may be freed or overwritten afterwards; dK and base are borrowed as in index_dev."""
        return Index(self, dcodes, dK, None, m, base, h, None, on_device=True, packed=(dnorm_codes, dcbnorms), base_format=base_format)

    def load_index(self, path, dev=False):
        """The Index a snapshot file holds (Index.save): header and table are validated before anything is allocated, the sections stream into device
        arrays the index owns, and what arrived on the device is digested there and compared with the file's table.  It answers every call bit for bit
        like the index that was saved.  dev: its calls take and return torch tensors (as Engine.index_dev's) instead of numpy arrays   [lsq_index_load]"""
        return Index._loaded(self, path, dev)

    # -- (1e) the beam-search encoder on resident codebooks ----------------------------------
    def encoder(self, K, m, chunk=0, h=H):
        """An Encoder of HOST codebooks K (m*h,d), copied once: ||c||^2 and the pair tables are built here, not per call.  Its beam() takes and returns
        host arrays.  chunk: vectors per pass (0 = the library's default)   [lsq_encoder_create]"""
        return Encoder(self, K, m, chunk, h, on_device=False)

    def encoder_dev(self, dK, m, chunk=0, h=H):
        """The same from a device tensor dK (copied as well); its beam() takes and returns torch tensors, on torch's current stream."""
        return Encoder(self, dK, m, chunk, h, on_device=True)

    # -- (1f) the coarse partition of a residual inverted-list index --------------------------
    def partition(self, centroids):
        """A Partition of HOST centroids (nlist,d) float32, copied once (update() replaces the copy): nearest-centroid assignment, cluster means,
        residuals and the scalar a residual index stores, on host arrays   [lsq_partition_create]"""
        return Partition(self, centroids, on_device=False)

    def partition_dev(self, dcentroids):
        """The same from a device tensor (copied as well); its methods take and return torch tensors, on torch's current stream."""
        return Partition(self, dcentroids, on_device=True)

    def quantize_norms(self, B, K, cbnorms, m, h=H):
        """B (n,m) int16 1-based, K (m*h,d), cbnorms (<= 256,): host arrays.
        -> idx (n,) int16 1-based index of the nearest norm centroid, dbnorms (n,) = cbnorms[idx-1], norms (n,) unquantised   [lsq_quantize_norms]"""
        return self._quantize_norms(_HOST, B, K, cbnorms, m, h)

    def quantize_norms_dev(self, dcodes, dK, dcb, m, h=H):
        """device tensors: codes (n,m) uint8 0-based, K (m*h,d) f32, cbnorms (<= 256,) f32 -> idx (n,) uint8 0-BASED, dbnorms (n,), norms (n,)   [lsq_quantize_norms_dev]"""
        return self._quantize_norms(_DEVICE, dcodes, dK, dcb, m, h)

    def _quantize_norms(self, side, B, K, cbnorms, m, h):
        B, K, cb = side.take(B, side.codes, "B"), side.take(K, _F32, "K"), side.take(cbnorms, _F32, "cbnorms").reshape(-1)
        n, d, p = B.shape[0], K.shape[1], side.ptr
        _shapes(("B", B, (n, m)), ("K", K, (m * h, d)))
        idx, dbn, nrm = side.new(n, side.codes, K, zero=True), side.new(n, _F32, K, zero=True), side.new(n, _F32, K, zero=True)
        self._call(side, "lsq_quantize_norms" + side.suffix, p(B), p(K), p(cb), int(cb.shape[0]), d, n, m, h, p(idx), p(dbn), p(nrm))
        return idx, dbn, nrm

    def update_codebooks(self, X, B, m, h=H):
        """X (n,d) f32, B (n,m) int16 1-based: host arrays -> K (m*h,d) least-squares codebooks, LSQR iterations   [lsq_update_codebooks_gpu]"""
        return self._update_codebooks(_HOST, X, B, m, h, None)

    def update_codebooks_dev(self, dX, dcodes, m, h=H, out=None):
        """device tensors: X (n,d) f32, codes (n,m) uint8 0-based -> K (m*h,d) f32 tensor, LSQR iterations   [lsq_update_codebooks_dev]"""
        return self._update_codebooks(_DEVICE, dX, dcodes, m, h, out)

    def _update_codebooks(self, side, X, B, m, h, out):
        X, B = side.take(X, _F32, "X"), side.take(B, side.codes, "B")
        (n, d), p = X.shape, side.ptr
        K = side.out(out, (m * h, d), _F32, X, zero=True)
        _shapes(("X", X, (n, d)), ("B", B, (n, m)), ("out", K, (m * h, d)))
        it = C.c_int(0)
        self._call(side, "lsq_update_codebooks" + (side.suffix or "_gpu"), p(X), p(B), d, n, m, h, p(K), C.byref(it))
        return K, int(it.value)

    # -- the structured codebook update: update_codebooks_generic / update_codebooks_chain (codebook_update.jl:104-158) ------------------
    def update_codebooks_struct(self, X, B, dim2C, m, h=H):
        """X (n,d) f32, B (n,m) int16 1-based, dim2C (d,m) 0/1 (codebook j covers dimension t) or None (every codebook covers everything): host arrays
        -> K (m*h,d) least-squares codebooks over the covering codebooks only, exactly zero elsewhere; LSQR iterations   [lsq_update_codebooks_struct_gpu]"""
        return self._update_codebooks_struct(_HOST, X, B, dim2C, m, h, None)

    def update_codebooks_struct_dev(self, dX, dcodes, ddim2C, m, h=H, out=None):
        """device tensors: X (n,d) f32, codes (n,m) uint8 0-based; dim2C (d,m) 0/1 as a device tensor (uint8 or bool), a host array, or None
        -> K (m*h,d) f32 tensor (`out` when given: it may hold anything), LSQR iterations   [lsq_update_codebooks_struct_dev]"""
        return self._update_codebooks_struct(_DEVICE, dX, dcodes, ddim2C, m, h, out)

    def _update_codebooks_struct(self, side, X, B, dim2C, m, h, out):
        X, B = side.take(X, _F32, "X"), side.take(B, side.codes, "B")
        (n, d), p = X.shape, side.ptr
        K = side.out(out, (m * h, d), _F32, X)
        _shapes(("X", X, (n, d)), ("B", B, (n, m)), ("out", K, (m * h, d)))
        if dim2C is None:
            cover = None
        elif side.dev and hasattr(dim2C, "is_cuda"):           # a tensor, wherever it lives.  Julia's d x m in memory: [m][d]
            import torch
            _shapes(("dim2C", dim2C, (d, m)))
            cover = dim2C.to(device=X.device, dtype=torch.uint8).t().contiguous()
        else:                                                  # a host array; the device form reads it from the device all the same
            cover = cover_bytes(dim2C, d, m)
            if side.dev:
                import torch
                cover = torch.from_numpy(cover).to(X.device)
        it = C.c_int(0)
        self._call(side, "lsq_update_codebooks_struct" + (side.suffix or "_gpu"), p(X), p(B), p(cover), d, n, m, h, p(K), C.byref(it))
        return K, int(it.value)

    # -- the sparse codebook update: SPGL1's LASSO mode (csrc/lsq_spgl1.hip) ---------------------------------
    def update_codebooks_spgl1(self, X, B, m, tau, K_init=None, S=-1, h=H, opt_tol=None, max_iter=None):
        """X (n,d) f32, B (n,m) int16 1-based: host arrays -> (K (m*h,d) f32, info dict): min 1/2||A k - b||^2 s.t. ||k||_1 <= tau warm-started
        from K_init, then only the S largest |K| kept (S < 0: all)   [lsq_update_codebooks_spgl1]"""
        return self._update_codebooks_spgl1(_HOST, X, B, m, tau, K_init, S, h, opt_tol, max_iter, None)

    def update_codebooks_spgl1_dev(self, dX, dcodes, m, tau, dK_init=None, S=-1, h=H, opt_tol=None, max_iter=None, out=None):
        """device tensors: X (n,d) f32, codes (n,m) uint8 0-based, K_init (m*h,d) f32 or None -> (K (m*h,d) f32 tensor, info dict)
        [lsq_update_codebooks_spgl1_dev]"""
        return self._update_codebooks_spgl1(_DEVICE, dX, dcodes, m, tau, dK_init, S, h, opt_tol, max_iter, out)

    def _update_codebooks_spgl1(self, side, X, B, m, tau, K_init, S, h, opt_tol, max_iter, out):
        X, B, K0 = side.take(X, _F32, "X"), side.take(B, side.codes, "codes"), side.maybe(K_init, _F32, "K_init")
        check_spgl1_args(tuple(X.shape), tuple(B.shape), m, h, tau, S, None if K0 is None else tuple(K0.shape), opt_tol, max_iter)
        (n, d), p = X.shape, side.ptr
        K = side.out(out, (m * h, d), _F32, X, zero=True)
        _shapes(("out", K, (m * h, d)))
        info = _lib.Spgl1Info()
        params = None if opt_tol is None and max_iter is None else C.byref(_lib.Spgl1Params(float(opt_tol or 0.0), int(max_iter or 0)))
        self._call(side, "lsq_update_codebooks_spgl1" + side.suffix, p(X), p(B), d, n, m, h, float(tau), p(K0), int(S), params, p(K), C.byref(info))
        return K, info.as_dict()

    # -- the initialisers' data-parallel steps (csrc/lsq_init.hip) ----------------------------------
    def encode_viterbi(self, X, K, m, h=H):
        """X (n,d) f32, K (m*h,d) f32 (chain codebooks, zero outside their dimensions) -> B (n,m) int16 1-based: the exact chain optimum
        (encode_chain.jl:92-123)   [lsq_encode_viterbi]"""
        return self._assign(_HOST, "lsq_encode_viterbi", X, K, m, h)[0]

    def encode_viterbi_dev(self, dX, dK, m, h=H):
        """device tensors -> codes (n,m) uint8 0-based   [lsq_encode_viterbi_dev]"""
        return self._assign(_DEVICE, "lsq_encode_viterbi", dX, dK, m, h)[0]

    def assign_codewords(self, X, K, m, h=H, want_min=False):
        """Per codebook independently the first argmin_a ||c||^2 - 2<x,c> (quantize_pq / the k-means assignment step; PQ.jl:12-41, kmeans.jl:6-75).
        X (n,d), K (m*h,d) -> B (n,m) int16 1-based [, the minima (n,m) f32]   [lsq_assign_codewords]"""
        B, mv = self._assign(_HOST, "lsq_assign_codewords", X, K, m, h, bool(want_min))
        return (B, mv) if want_min else B

    def assign_codewords_dev(self, dX, dK, m, h=H, want_min=False):
        """device tensors -> codes (n,m) uint8 0-based [, minima (n,m) f32]   [lsq_assign_codewords_dev]"""
        dB, dmin = self._assign(_DEVICE, "lsq_assign_codewords", dX, dK, m, h, bool(want_min))
        return (dB, dmin) if want_min else dB

    def _assign(self, side, sym, X, K, m, h, want_min=None):
        """the two calls that give every row one code per codebook; want_min: None where the symbol has no argument for the minima"""
        X, K = side.take(X, _F32, "X"), side.take(K, _F32, "K")
        (n, d), p = X.shape, side.ptr
        _shapes(("X", X, (n, d)), ("K", K, (m * h, d)))
        B = side.new((n, m), side.codes, X)
        mv = side.new((n, m), _F32, X) if want_min else None
        self._call(side, sym + side.suffix, p(X), p(K), d, n, m, h, p(B), *(() if want_min is None else (p(mv),)))
        return B, mv

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
        return self._update_centers(_HOST, X, B, dim2C, m, K_prev, h, None, None)

    def update_centers_dev(self, dX, dcodes, dim2C, m, K_prev=None, h=H, out=None, counts=None):
        """device tensors: X (n,d) f32, codes (n,m) uint8 0-based, K_prev (m*h,d) f32 or None (it may be `out`); dim2C (d,m) 0/1 on the HOST
        -> (K (m*h,d) f32 tensor (`out` when given: it may hold anything), counts (m*h,) int32 tensor).  Nothing waits for the device   [lsq_update_centers_dev]"""
        return self._update_centers(_DEVICE, dX, dcodes, dim2C, m, K_prev, h, out, counts)

    def _update_centers(self, side, X, B, dim2C, m, K_prev, h, out, counts):
        X, B, Kp = side.take(X, _F32, "X"), side.take(B, side.codes, "B"), side.maybe(K_prev, _F32, "K_prev")
        (n, d), p = X.shape, side.ptr
        K, cnt = side.out(out, (m * h, d), _F32, X), side.out(counts, (m * h,), _I32, X, "counts", zero=True)
        _shapes(("X", X, (n, d)), ("B", B, (n, m)), ("K_prev", Kp, (m * h, d)), ("out", K, (m * h, d)), ("counts", cnt, (m * h,)))
        cover = self._host_cover(dim2C, d, m)
        self._call(side, "lsq_update_centers" + side.suffix, p(X), p(B), cover.ctypes.data, p(Kp), d, n, m, h, p(K), p(cnt))
        return K, cnt

    def kmeanspp_seed(self, X, dim2C, u, m, h=H):
        """k-means++ (D^2) seeding of all m sub-spaces.  X (n,d) f32, dim2C (d,m) 0/1, u (m,h) doubles in [0,1) drawn by the caller: host arrays
        -> (K (m*h,d): the chosen rows restricted to the cover, idx (m,h) int64 0-based row indices, d2 (n,m) f32 squared distance to the nearest chosen row)
        [lsq_kmeanspp_seed]"""
        return self._kmeanspp_seed(_HOST, X, dim2C, u, m, h, True, True, None)

    def kmeanspp_seed_dev(self, dX, dim2C, u, m, h=H, want_idx=True, want_d2=False, out=None):
        """The same on a device tensor X (n,d) f32; dim2C and u on the HOST -> (K (m*h,d) f32 tensor, idx (m,h) int64 tensor or None, d2 (n,m) f32 tensor or
        None).  2 h - 1 launches in stream order, nothing waits for the device   [lsq_kmeanspp_seed_dev]"""
        return self._kmeanspp_seed(_DEVICE, dX, dim2C, u, m, h, want_idx, want_d2, out)

    def _kmeanspp_seed(self, side, X, dim2C, u, m, h, want_idx, want_d2, out):
        X, u = side.take(X, _F32, "X"), _HOST.take(u, np.float64, "u")
        (n, d), p = X.shape, side.ptr
        cover = self._host_cover(dim2C, d, m)
        K = side.out(out, (m * h, d), _F32, X)
        _shapes(("X", X, (n, d)), ("u", u, (m, h)), ("out", K, (m * h, d)))
        idx = side.new((m, h), _I64, X) if want_idx else None
        d2 = side.new((n, m), _F32, X) if want_d2 else None
        self._call(side, "lsq_kmeanspp_seed" + side.suffix, p(X), cover.ctypes.data, u.ctypes.data, d, n, m, h, p(K), p(idx),
                   None if side.dev and n == 0 else p(d2))          # the device form takes no pointer to an empty tensor
        return K, idx, d2

    def linscan_stats(self):
        t = _lib.LinscanStats()
        self._call(_HOST, "lsq_get_linscan_stats", C.byref(t))
        return t.as_dict()

    # -- (2) CPU-path shaped ---------------------------------------------------------------
    @staticmethod
    def _xkb(X, K, B, m, h):
        """the data, the codebooks and (or None) the codes of the CPU-shaped calls -> X, K, B, n, d"""
        X, K, B = _HOST.take(X, _F32, "X"), _HOST.take(K, _F32, "K"), _HOST.maybe(B, _I16, "B")
        n, d = X.shape
        _shapes(("X", X, (n, d)), ("K", K, (m * h, d)), ("B", B, (n, m)))
        return X, K, B, n, d

    def encoding_icm(self, X, oldB, K, m, niter, randord, npert, seed=0, it=None, global_offset=0, h=H):
        """ONE ILS iteration with the accept rule.  it=None (default): the context's own counter (LSQ_IT_AUTO) -- the k-th call uses it = k-1."""
        X, K, oldB, n, d = self._xkb(X, K, oldB, m, h)
        out, p = _HOST.new((n, m), _I16), _HOST.ptr
        self._call(_HOST, "lsq_encoding_icm", p(X), p(oldB), p(K), d, n, m, h, int(niter), int(bool(randord)), int(npert), int(seed),
                   int(IT_AUTO if it is None else it), int(global_offset), p(out))
        return out

    def encode_icm_fully(self, B, X, K, m, niter, randord, npert, idx_first=1, seed=0, it=None, h=H):
        """In place on B (n, m) int16 (must be C-contiguous int16).  it=None: the context's counter, as in encoding_icm."""
        if B.dtype != np.int16 or not B.flags["C_CONTIGUOUS"]:
            raise ValueError("B must be a C-contiguous int16 (n, m) array (it is updated in place)")
        X, K, B, n, d = self._xkb(X, K, B, m, h)
        p = _HOST.ptr
        self._call(_HOST, "lsq_encode_icm_fully", p(B), p(X), p(K), d, n, m, h, int(niter), int(bool(randord)), int(npert), int(idx_first), int(seed),
                   int(IT_AUTO if it is None else it))
        return B

    # -- (3) helpers -----------------------------------------------------------------------
    def get_unaries(self, X, K, m, h=H):
        X, K = _HOST.take(X, _F32, "X"), _HOST.take(K, _F32, "K")
        (n, d), p = X.shape, _HOST.ptr
        U = _HOST.new((m, n, h), _F32)
        self._call(_HOST, "lsq_get_unaries", p(X), p(K), d, n, m, h, p(U))
        return U

    def get_binaries(self, K, m, h=H):
        K = _HOST.take(K, _F32, "K")
        T = _HOST.new((m, m, h, h), _F32)
        self._call(_HOST, "lsq_get_binaries", K.ctypes.data, K.shape[1], m, h, T.ctypes.data)
        return T

    def veccost(self, X, B, K, m, h=H):
        X, K, B, n, d = self._xkb(X, K, B, m, h)
        out, p = _HOST.new(n, _F32), _HOST.ptr
        self._call(_HOST, "lsq_veccost", p(X), p(B), p(K), d, n, m, h, p(out))
        return out

    def qerror(self, X, B, K, m, h=H):
        X, K, B, n, d = self._xkb(X, K, B, m, h)
        out, p = C.c_double(0.0), _HOST.ptr
        self._call(_HOST, "lsq_qerror", p(X), p(B), p(K), d, n, m, h, C.byref(out))
        return float(out.value)

    def perturb(self, B, npert, seed=0, it=0, global_offset=0, h=H):
        B = _HOST.take(B, _I16, "B").copy()
        n, m = B.shape
        self._call(_HOST, "lsq_perturb", B.ctypes.data, n, m, h, int(npert), int(seed), int(it), int(global_offset))
        return B

    # -- (4) device generators -------------------------------------------------------------
    def synth_data_u8_dev(self, seed, n, d, device=None, global_offset=0):
        X = _DEVICE.new((n, d), _F32, self._device(device))
        self._call(_DEVICE, "lsq_synth_data_u8_dev", int(seed), int(global_offset), n, d, X.data_ptr())
        return X

    def randinit_dev(self, seed, n, m, device=None, global_offset=0, h=H):
        B = _DEVICE.new((n, m), _U8, self._device(device))
        self._call(_DEVICE, "lsq_randinit_dev", int(seed), int(global_offset), n, m, h, B.data_ptr())
        return B

    def synth_codebooks_dev(self, seed, m, d, device=None, h=H):
        K = _DEVICE.new((m * h, d), _F32, self._device(device))
        self._call(_DEVICE, "lsq_synth_codebooks_dev", int(seed), m, h, d, K.data_ptr())
        return K


# -- the resident index (made by Engine.index / Engine.index_dev) --------------------------------

class _Handle:
    """The life of a handle made on an Engine's context (Index, Encoder): the side its calls take, how it is made and freed, how its info structs are read."""

    _destroy = None                                   # the symbol that frees the handle
    _side = property(lambda self: _DEVICE if self._dev else _HOST)

    def _bind(self, engine, on_device):
        self._eng, self._L, self._dev, self._h, self._keep = engine, engine._L, bool(on_device), None, None
        return self._side

    def _create(self, sym, desc):
        handle = C.c_void_p()
        self._eng._call(self._side, sym, self._eng._h, C.byref(desc), h=C.byref(handle))
        self._h = handle
        self._eng._indexes.add(self)

    def _info(self, sym, struct):
        st = struct()
        self._eng._call(_HOST, sym, C.byref(st), h=self._h)
        return st.as_dict()

    def close(self):
        # Engine.close closes its handles first.  Should the context be gone all the same, the handle is dropped, not destroyed: its destroy call would
        # reach through the freed context, and lsq_destroy knows nothing of the handle's buffers, which then stay allocated until the process ends.
        if getattr(self, "_h", None) and getattr(self._eng, "_h", None):
            getattr(self._L, self._destroy)(self._h)
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


class Index(_Handle):
    """A resident database on an Engine's device: the ADC scan (stage one) and the exact re-rank of its shortlists (stage two)   [lsq_index_*].
    Made by Engine.index (host arrays in and out) or Engine.index_dev (torch tensors in and out, on torch's current stream)."""

    _destroy = "lsq_index_destroy"

    def __init__(self, engine, codes, K, dbnorms, m, base, h, d, on_device, packed=None, base_format=None):
        side = self._bind(engine, on_device)
        code = base_format_code(base_format)           # an unknown format is refused here, before anything is taken
        codes, K, dbnorms = side.maybe(codes, _U8, "codes"), side.maybe(K, _F32, "K"), side.maybe(dbnorms, _F32, "dbnorms")
        u8, narrow_to = False, None                      # u8: what the description's base_u8 field carries -- the FORMAT of the base rows
        if base is None:
            if code is not None:
                raise ValueError("base_format=%r needs base rows" % (base_format,))
        elif side.dev:
            base, u8, narrow_to = _device_half_rows(base, code)
        elif code is not None:
            base, u8 = _host_half_rows(self._L, engine._check, base, code), code
        else:
            base, u8 = side.take_x(base, "base", rows=True)
        self._u8, self._fmt, self._has_codes, self._has_base, self._packed = int(u8) == _lib.BASE_U8, int(u8), codes is not None, base is not None, packed is not None
        if packed is not None:
            self._init_packed(side, codes, K, packed, m, base, u8, h)
            return self._narrow_after(narrow_to)
        if codes is None and base is None:
            raise ValueError("an index needs codes, base rows or both")
        n = int(codes.shape[0] if codes is not None else base.shape[0])
        d = int(K.shape[1] if codes is not None else (d or base.shape[1]))
        if codes is not None:
            _shapes(("codes", codes, (n, m)), ("K", K, (m * h, d)), ("dbnorms", dbnorms, (n,)))
        if base is not None:
            _shapes(("base", base, (n, max(d, base.shape[1]))))       # at least d columns
        desc, p = _lib.IndexDesc(), side.ptr
        desc.n, desc.d, desc.m, desc.h = n, d, int(m), int(h)
        if codes is not None:
            desc.codes, desc.codebooks, desc.dbnorms = p(codes), p(K), p(dbnorms)
        desc.base, desc.base_u8, desc.ldb, desc.on_device = p(base), int(u8), 0 if base is None else int(side.pitch(base)), int(self._dev)
        self._keep = (codes, K, dbnorms, base)      # borrowed device tensors stay alive with the index
        self.n, self.d, self.m = n, d, int(m)
        self._create("lsq_index_create", desc)
        self._narrow_after(narrow_to)

    def _narrow_after(self, code):
        """a device index made from a float32 tensor with a base_format: narrowed now, the borrowed float32 rows let go"""
        if code is None:
            return
        try:
            self.narrow_base(_HALF_BY_CODE[code][0])
        except Exception:
            self.close()
            raise
        self._keep = tuple(None if i == len(self._keep) - 1 else a for i, a in enumerate(self._keep))      # base is the last of what is kept

    def _init_packed(self, side, codes, K, packed, m, base, u8, h):
        """the packed form (Engine.index_packed): the norm bytes and their table instead of dbnorms; checked here, refused before any library call"""
        if codes is None or K is None:
            raise ValueError("a packed index needs codes and codebooks")
        if not side.dev and np.asarray(packed[0]).dtype != _U8:      # the host side converts values, but a norm byte is an index: never narrowed silently
            raise TypeError("norm_codes must be uint8, got %s" % np.asarray(packed[0]).dtype)
        nc, cb = side.take(packed[0], _U8, "norm_codes"), side.take(packed[1], _F32, "cbnorms")
        n, d = int(codes.shape[0]), int(K.shape[1])
        _shapes(("codes", codes, (n, m)), ("K", K, (m * h, d)), ("norm_codes", nc, (n,)), ("cbnorms", cb, (None,)))
        if not 1 <= int(cb.shape[0]) <= 256:
            raise ValueError("cbnorms must hold 1 .. 256 entries, got %d" % int(cb.shape[0]))
        if base is not None:
            _shapes(("base", base, (n, max(d, base.shape[1]))))
        desc, p = _lib.IndexPackedDesc(), side.ptr
        desc.n, desc.d, desc.m, desc.h = n, d, int(m), int(h)
        desc.codes, desc.norm_codes, desc.cbnorms, desc.ncb, desc.codebooks = p(codes), p(nc), p(cb), int(cb.shape[0]), p(K)
        desc.base, desc.base_u8, desc.ldb, desc.on_device = p(base), int(u8), 0 if base is None else int(side.pitch(base)), int(self._dev)
        self._keep = (K, base)                      # what a device index borrows; codes, norm bytes and table were copied
        self.n, self.d, self.m = n, d, int(m)
        self._create("lsq_index_create_packed", desc)

    def _search_args(self, Q_scan, k, **others):
        """the queries of a two-stage search, each of the others (name=array or None) defaulting to Q_scan -> Qs, the others in order, dists, ids"""
        side = self._side
        Qs = side.take(Q_scan, _F32, "Q_scan")
        Qo = [Qs if a is None else side.take(a, _F32, name) for name, a in others.items()]
        _shapes(("Q_scan", Qs, (None, self.d)), *((name, a, tuple(Qs.shape)) for name, a in zip(others, Qo)))
        return (Qs, *Qo, *side.topk(Qs.shape[0], int(k), Qs))

    def search(self, Q_scan, k, shortlist=0, Q_exact=None):
        """Q_scan (nq,d): what the scan reads (the rotated queries of linscan_lsq); Q_exact (nq,d): the queries in the base set's own frame (default:
        Q_scan).  shortlist=0: the ADC scan alone, Engine.linscan's results; shortlist=L>=k: scan for L, re-rank to k by exact distance.
        -> dists (nq,k) float32 ascending, ids (nq,k) int32 1-BASED   [lsq_index_search]"""
        Qs, Qe, dists, ids = self._search_args(Q_scan, k, Q_exact=Q_exact)
        side, p = self._side, self._side.ptr
        self._eng._call(side, "lsq_index_search", p(dists), p(ids), p(Qs), p(Qe), Qs.shape[0], self.d, int(shortlist), int(k), int(self._dev), h=self._h)
        return dists, ids

    def rerank(self, Q, cand, k, id_base=1):
        """Stage two alone: cand (nq,L) int32 ids in id_base (the 0-based shortlists of linscan_pq: id_base=0).
        -> dists (nq,k) float32 exact, ascending, ids (nq,k) int32 in id_base; an id outside the base comes last as (+inf, id_base-1)   [lsq_index_rerank]"""
        side = self._side
        Q, cand = side.take(Q, _F32, "Q"), side.take(cand, _I32, "cand")
        _shapes(("Q", Q, (None, self.d)), ("cand", cand, (Q.shape[0], None)))
        (nq, L), p = cand.shape, side.ptr
        dists, ids = side.topk(nq, int(k), Q)
        self._eng._call(side, "lsq_index_rerank", p(dists), p(ids), p(Q), p(cand), nq, self.d, int(L), int(k), int(id_base), int(self._dev), h=self._h)
        return dists, ids

    def knn(self, Q, k, id_base=0):
        """Exact k-NN over the resident base rows (f32; uint8, float16 and bfloat16 rows are widened in registers, never in memory): the ground truth of a recall figure.  Q (nq,>=d) float32 or uint8 rows
        with unit column stride, any row pitch and byte offset (numpy on an Engine.index, torch on an Engine.index_dev); the first d columns are read.
        -> dists (nq,k) float32 ascending with lsq_knn_exact's bits, ids (nq,k) int32 in id_base; ties by smaller id   [lsq_index_knn]"""
        side = self._side
        if side.dev:
            Q, u8 = side.take_x(Q, "Q", rows=True)
        else:                                           # the host form converts, but a row view of the right type is read in place here as well
            u8 = _dtname(Q) == "uint8"
            Q = np.asarray(Q, dtype=_U8 if u8 else _F32)
            if Q.ndim != 2 or Q.strides[1] != Q.itemsize or Q.strides[0] % Q.itemsize or (Q.shape[0] > 1 and Q.strides[0] < Q.shape[1] * Q.itemsize):
                Q = np.ascontiguousarray(Q)
        _shapes(("Q", Q, (None, max(self.d, Q.shape[-1]))))           # at least d columns
        nq, p = Q.shape[0], side.ptr
        dists, ids = side.topk(nq, int(k), Q)
        self._eng._call(side, "lsq_index_knn", p(dists), p(ids), p(Q), int(u8), nq, int(side.pitch(Q)), int(k), int(id_base), int(self._dev), h=self._h)
        return dists, ids

    def set_lists(self, centroids, assign):
        """Lay inverted lists over the index's codes: centroids (nlist,d) float32, assign (n,) int32 0-based list of every row (train_coarse and
        ivf_assign make them).  The index copies what it needs; calling it again replaces the lists   [lsq_index_set_lists]"""
        side = self._side
        cent, lor = side.take(centroids, _F32, "centroids"), side.take(assign, _I32, "assign")
        _shapes(("centroids", cent, (None, self.d)), ("assign", lor, (self.n,)))
        desc, p = _lib.IvfDesc(), side.ptr
        desc.nlist, desc.centroids, desc.list_of_row, desc.on_device = int(cent.shape[0]), p(cent), p(lor), int(self._dev)
        self._eng._call(side, "lsq_index_set_lists", C.byref(desc), h=self._h)
        self.nlist = int(cent.shape[0])

    def search_ivf(self, Q_scan, k, nprobe, shortlist=0, Q_coarse=None, Q_exact=None, add_coarse=False, every_record=False, flags=0):
        """search() over the rows of each query's nprobe nearest lists alone.  Q_coarse (nq,d): what is compared with the centroids (default: Q_scan);
        add_coarse: one more rounded add of the coarse distance (residual codes); every_record: the road that writes and sorts every probed row.
        -> dists (nq,k) float32 ascending, ids (nq,k) int32 1-BASED original row ids; (+inf, 0) where the probed lists hold fewer than k rows
        [lsq_index_search_ivf]"""
        Qs, Qc, Qe, dists, ids = self._search_args(Q_scan, k, Q_coarse=Q_coarse, Q_exact=Q_exact)
        side, p = self._side, self._side.ptr
        fl = int(flags) | (_lib.IVF_ADD_COARSE if add_coarse else 0) | (_lib.IVF_EVERY_RECORD if every_record else 0)
        self._eng._call(side, "lsq_index_search_ivf", p(dists), p(ids), p(Qs), p(Qc), p(Qe), Qs.shape[0], self.d, int(nprobe), int(shortlist), int(k), fl,
                        int(self._dev), h=self._h)
        return dists, ids

    def range_search(self, Q_scan, radius, nprobe=0, Q_coarse=None, add_coarse=False):
        """Every candidate row within `radius` of each query: radius a scalar or (nq,) float32, compared as dist <= radius (a NaN on either side returns
        nothing).  nprobe=0: every row; nprobe>=1: the rows of the query's nprobe nearest lists, chosen and (add_coarse) measured as search_ivf does.
        Under a filter: the allowed rows alone.  The distances are search()'s / search_ivf()'s own bits, so a query's result is the longest prefix
        within the radius of the ranking those return for k = all candidate rows.
        -> lims (nq+1,) int64, dists (lims[-1],) float32, ids (lims[-1],) int32 1-BASED: query q's results are entries lims[q] .. lims[q+1]-1, ascending by
        (dist, id); numpy on an Engine.index, torch tensors on an Engine.index_dev   [lsq_index_range_search, lsq_index_range_fetch]"""
        side, p = self._side, self._side.ptr
        Qs = side.take(Q_scan, _F32, "Q_scan")
        Qc = Qs if Q_coarse is None else side.take(Q_coarse, _F32, "Q_coarse")
        nq = int(Qs.shape[0])
        if np.ndim(radius) == 0 and not hasattr(radius, "is_cuda"):      # one radius for every query
            rad = side.new((nq,), _F32, Qs)
            rad[...] = float(radius)
        else:
            rad = side.take(radius, _F32, "radius")
        _shapes(("Q_scan", Qs, (None, self.d)), ("Q_coarse", Qc, tuple(Qs.shape)), ("radius", rad, (nq,)))
        lims = side.new((nq + 1,), _I64, Qs, zero=True)
        spare = side.new((1,), _F32, Qs)                # nq == 0: an empty array still names one
        qs, qc, rd = (p(a) if nq else p(spare) for a in (Qs, Qc, rad))
        fl = _lib.IVF_ADD_COARSE if add_coarse else 0
        self._eng._call(side, "lsq_index_range_search", p(lims), qs, qc if int(nprobe) else None, rd, nq, self.d, int(nprobe), fl, int(self._dev), h=self._h)
        total = int(self.range_info()["results"])
        dists, ids = side.new((total,), _F32, Qs), side.new((total,), _I32, Qs)
        self._eng._call(side, "lsq_index_range_fetch", p(dists) if total else None, p(ids) if total else None, total, int(self._dev), h=self._h)
        return lims, dists, ids

    def range_info(self):
        """what the last range_search call did: queries, rows_walked, results, max_per_query, batches, road (0 unfiltered, 1 dense, 2 compact), held_bytes,
        coarse_ms / lut_ms / count_ms / fill_ms / sort_ms (with profile=True)"""
        return self._info("lsq_index_get_range_info", _lib.RangeInfo)

    def ivf_info(self):
        """what the last search_ivf call did: queries, probed_rows, records, threshold_queries, fallback_queries, batches, batch_queries,
        tail_capacity, coarse_ms / lut_ms / scan_ms / select_ms (with profile=True)"""
        return self._info("lsq_index_get_ivf_info", _lib.IvfInfo)

    def knn_info(self):
        """what the last knn call did: queries, rows, batches, fallback_queries, exhaustive, int_road, norms_ms / scan_ms / select_ms (with profile=True)"""
        return self._info("lsq_index_get_knn_info", _lib.IndexKnnInfo)

    def stats(self):
        return self._info("lsq_index_get_stats", _lib.IndexStats)

    def packed_info(self):
        """row_bytes (m + 1), ivf_row_bytes (m + 5 once lists are set), ncb, dword_rows, resident_bytes; all zero on an index that is not packed"""
        return self._info("lsq_index_get_packed_info", _lib.IndexPackedInfo)

    def scan_stats(self):
        """the selection statistics of the last search()'s scan: Engine.linscan_stats' fields, this call's figures alone"""
        return self._info("lsq_index_get_scan_stats", _lib.LinscanStats)

    _ROADS = {None: 0, "dense": _lib.FILTER_FORCE_DENSE, "compact": _lib.FILTER_FORCE_COMPACT}

    def set_filter(self, mask=None, bits=None, ids=None, deny=False, id_base=0, road=None):
        """Restrict search, search_ivf and knn to a set of allowed rows, given in exactly one of three forms (numpy on an Engine.index, torch tensors on an
        Engine.index_dev): mask (n,) bool / uint8, non-zero = set; bits (ceil(n/32),) uint32 (a device tensor may be int32: the same bits), bit i & 31 of
        word i >> 5 = row i; ids (count,) int32 row ids in id_base, duplicates legal.  deny: the set rows are the EXCLUDED ones.  Each call then returns what
        it would return for every candidate row with the rows outside the set removed, truncated to k and padded with (+inf, id_base - 1); rerank ignores the
        filter.  The index keeps a copy.  road: None (by the number of allowed rows), "dense" or "compact" -- test hooks, the same results
        [lsq_index_set_filter]"""
        given = [(name, a) for name, a in (("mask", mask), ("bits", bits), ("ids", ids)) if a is not None]
        if len(given) != 1:
            raise ValueError("set_filter needs exactly one of mask, bits, ids (got %s)" % (", ".join(nm for nm, _ in given) or "none"))
        if road not in self._ROADS:
            raise ValueError("road must be None, 'dense' or 'compact', got %r" % (road,))
        side, (name, a) = self._side, given[0]
        desc = _lib.FilterDesc()
        if name == "mask":
            if _dtname(a) not in ("bool", "uint8"):
                raise TypeError("mask must be bool or uint8, got %s" % (_dtname(a) or type(a).__name__))
            if side.dev:
                import torch
                a = side.take(a.view(torch.uint8) if _dtname(a) == "bool" and getattr(a, "is_cuda", False) else a, _U8, "mask")
            else:
                a = np.ascontiguousarray(a).view(_U8)
            _shapes(("mask", a, (self.n,)))
            desc.form = _lib.FILTER_BYTES
        elif name == "bits":
            if side.dev:
                a = side.take(a, np.int32 if _dtname(a) == "int32" else np.uint32, "bits")
            else:
                a = np.ascontiguousarray(a, dtype=np.uint32)
            _shapes(("bits", a, ((self.n + 31) // 32,)))
            desc.form = _lib.FILTER_BITS
        else:
            a = side.take(a, _I32, "ids")
            _shapes(("ids", a, (None,)))
            desc.form, desc.count, desc.id_base = _lib.FILTER_IDS, int(a.shape[0]), int(id_base)
        desc.data = side.ptr(a) if a.shape[0] > 0 else side.ptr(side.new((1,), _I32, a))      # an empty id list still names an array
        desc.flags, desc.on_device = (_lib.FILTER_DENY if deny else 0) | self._ROADS[road], int(self._dev)
        self._eng._call(side, "lsq_index_set_filter", C.byref(desc), h=self._h)

    def clear_filter(self):
        """drop the filter: every call answers over all rows again, bit for bit as before   [lsq_index_set_filter(NULL)]"""
        self._eng._call(self._side, "lsq_index_set_filter", None, h=self._h)

    def filter_info(self):
        """active, n, allowed, lists / lists_without_allowed (0 without inverted lists), road of the last search / search_ivf / knn call (0 unfiltered,
        1 dense, 2 compact), crossover_rows (compact by default when allowed <= this, outside the band the header describes)"""
        return self._info("lsq_index_get_filter_info", _lib.FilterInfo)

    def add(self, codes=None, dbnorms=None, norm_codes=None, base=None, assign=None):
        """Append rows: they become rows n .. n + count - 1 (0-based), and every call then answers as on an index built over the concatenation, with the
        concatenated lists and a filter that allows the new rows too.  What the index holds is what must be given: codes (count,m) uint8 0-based with
        dbnorms (count,) float32 -- a packed index: norm_codes (count,) uint8 instead --, base (count,>=d) rows of the index's own type with unit column
        stride and any pitch (a half-precision index: host float rows are narrowed, float16 rows / uint16 bfloat16 bits are taken as they are; device
        tensors must have the index's dtype), assign (count,) int32 0-based lists once lists are set.  All numpy arrays or all torch device tensors, whichever way the
        index was made; they are read before the call returns.  A device index that borrowed its arrays copies them once, at the first add or reserve
        [lsq_index_add]"""
        given = [(nm, a) for nm, a in (("codes", codes), ("dbnorms", dbnorms), ("norm_codes", norm_codes), ("base", base), ("assign", assign)) if a is not None]
        if not given:
            raise ValueError("add needs the arrays of the new rows")
        on_dev = [bool(getattr(a, "is_cuda", False)) for _, a in given]
        if any(on_dev) != all(on_dev):
            raise TypeError("add takes numpy arrays or torch device tensors, not both: %s" % ", ".join("%s %s" % (nm, "device" if v else "host") for (nm, _), v in zip(given, on_dev)))
        side = _DEVICE if on_dev[0] else _HOST
        if not side.dev and norm_codes is not None and np.asarray(norm_codes).dtype != _U8:      # a norm byte is an index: never narrowed silently
            raise TypeError("norm_codes must be uint8, got %s" % np.asarray(norm_codes).dtype)
        codes, dbnorms, nc, lor = side.maybe(codes, _U8, "codes"), side.maybe(dbnorms, _F32, "dbnorms"), side.maybe(norm_codes, _U8, "norm_codes"), side.maybe(assign, _I32, "assign")
        fmt = self._format()
        if base is not None and fmt in _HALF_BY_CODE:      # a half index: host float rows are narrowed, rows already in the format are taken as they are
            if side.dev:
                base, have, _ = _device_half_rows(base, None)
                if have != fmt:
                    raise TypeError("base rows must have the index's own type (%s), got %s" % (_FORMAT_NAMES[fmt], _dtname(base)))
            else:
                base = _host_half_rows(self._L, self._eng._check, base, fmt)
        elif base is not None:
            u8 = _dtname(base) == "uint8"
            if u8 != self._u8:
                raise TypeError("base rows must have the index's own type (%s), got %s" % ("uint8" if self._u8 else "float32", _dtname(base)))
            if side.dev:
                base, _ = side.take_x(base, "base", rows=True)
            else:                                       # a row view of the right type is read in place: any pitch and byte offset
                base = np.asarray(base, dtype=_U8 if u8 else _F32)
                if base.ndim != 2 or base.strides[1] != base.itemsize or base.strides[0] % base.itemsize or (base.shape[0] > 1 and base.strides[0] < base.shape[1] * base.itemsize):
                    base = np.ascontiguousarray(base)
        count = int(next(a for a in (codes, dbnorms, nc, base, lor) if a is not None).shape[0])
        _shapes(("codes", codes, (count, self.m)), ("dbnorms", dbnorms, (count,)), ("norm_codes", nc, (count,)), ("assign", lor, (count,)),
                ("base", base, (count, max(self.d, base.shape[-1] if base is not None else 0))))
        desc, p = _lib.IndexAddDesc(), side.ptr
        desc.count, desc.codes, desc.dbnorms, desc.norm_codes, desc.list_of_row = count, p(codes), p(dbnorms), p(nc), p(lor)
        desc.base, desc.ldb, desc.on_device = p(base), 0 if base is None else int(side.pitch(base)), int(side.dev)
        try:
            self._eng._call(side, "lsq_index_add", C.byref(desc), h=self._h)
        finally:
            self.n = int(self.growth_info()["n"])

    def reserve(self, rows):
        """capacity for at least `rows` rows in all: the adds up to there re-allocate nothing (a device index adopts its borrowed arrays now)   [lsq_index_reserve]"""
        self._eng._call(self._side, "lsq_index_reserve", int(rows), h=self._h)

    def growth_info(self):
        """n, capacity_rows, adds, rows_added, reallocations, adopted, merged_rows (last add), append_ms / merge_ms / filter_ms (last add, with profile=True)"""
        return self._info("lsq_index_get_growth_info", _lib.IndexGrowthInfo)

    def remove(self, ids, id_base=0):
        """Hide rows for good: ids (count,) int32 row ids in id_base, a numpy array or a torch device tensor on either kind of index; duplicates and rows
        already removed are legal.  Every call then answers as after set_filter(the allowed rows in force, or all rows, minus these); a forced road of
        the filter in force stays.  An id outside the index refuses the call and changes nothing.  The rows still occupy memory and scan time until
        compact()   [lsq_index_remove]"""
        side = _DEVICE if getattr(ids, "is_cuda", False) else _HOST
        ids = side.take(ids, _I32, "ids")
        _shapes(("ids", ids, (None,)))
        count = int(ids.shape[0])
        self._eng._call(side, "lsq_index_remove", side.ptr(ids) if count else None, count, int(id_base), int(side.dev), h=self._h)

    def compact(self, shrink=False, want_map=True):
        """The rows outside the filter in force LEAVE the index (no filter: none does): the survivors keep their order and become rows 0 .. n' - 1, every
        call then answers bit for bit as on an index freshly built over them, and the filter is gone.  shrink: the storage is sized to n' rows instead of
        keeping its capacity for later adds.  -> old_of_new (n',) int32 0-based, the former row of every row (numpy on a host index, a device tensor on a
        device index); None with want_map=False.  Index.n follows   [lsq_index_compact]"""
        side = self._side
        desc = _lib.IndexCompactDesc()
        desc.flags, desc.id_base, desc.on_device = (_lib.COMPACT_SHRINK if shrink else 0), 0, int(side.dev)
        out = None
        if want_map:
            info = self.filter_info()
            out = side.new((int(info["allowed"] if info["active"] else info["n"]),), _I32, self._eng._device() if side.dev else None)
            desc.old_of_new = side.ptr(out) if out.shape[0] else None
        try:
            self._eng._call(side, "lsq_index_compact", C.byref(desc), h=self._h)
        finally:
            self.n = int(self.growth_info()["n"])
        return out

    def compact_info(self):
        """n_before / n_after / moved_bytes / shrunk (last compact), removes, rows_tombstoned, compactions, rows_dropped (since creation), tombstone_ms (last
        remove) and gather_ms / layout_ms (last compact) with profile=True"""
        return self._info("lsq_index_get_compact_info", _lib.IndexCompactInfo)

    def reconstruct(self, ids=None, start=0, count=None, add_coarse=False, pad_nan=False, id_base=0, out=None):
        """The vectors the index's codes stand for.  ids=None: rows start .. start + count - 1 (count=None: to the last row); else ids (count,) int32 in
        id_base, any order, repeats allowed -- numpy on an Engine.index, a device tensor on an Engine.index_dev.  add_coarse: plus the centroid of the
        row's list (a residual index; needs set_lists).  pad_nan: an id outside the index gives a row of NaN and is counted in recon_info()["invalid"]
        -- this decodes search results, whose padding ids lie outside; without it such an id refuses the call and nothing is written.  A filter
        changes nothing: a removed row is addressable until compact().  out: (count, >=d) float32 rows to write into (the same kind of array)
        -> (count, d) float32   [lsq_index_reconstruct]"""
        side, p = self._side, self._side.ptr
        if ids is not None:
            ids = side.take(ids, _I32, "ids")
            _shapes(("ids", ids, (None,)))
            count, start = int(ids.shape[0]), 0
        elif count is None:
            count = self.n - int(start)
        count = int(count)
        if out is None:
            out = side.new((max(count, 0), self.d), _F32, self._eng._device() if side.dev else None, zero=True)
        elif side.dev:
            out = side.take(out, _F32, "out", rows=True)
        elif not (isinstance(out, np.ndarray) and out.dtype == _F32 and out.ndim == 2 and out.strides[1] == 4 and out.strides[0] % 4 == 0):
            raise ValueError("out must be a 2-d float32 numpy array of rows with unit column stride")
        _shapes(("out", out, (max(count, 0), max(self.d, out.shape[1]))))
        fl = (_lib.RECON_ADD_COARSE if add_coarse else 0) | (_lib.RECON_PAD_NAN if pad_nan else 0)
        ldo = int(side.pitch(out)) if out.shape[0] > 1 else int(out.shape[1])
        self._eng._call(side, "lsq_index_reconstruct", p(out) if count > 0 else None, ldo, p(ids) if ids is not None and count > 0 else None, int(start), count,
                        int(id_base), fl, int(self._dev), h=self._h)
        return out

    def search_rows(self, rows, k, nprobe=0, add_coarse=False, id_base=0):
        """Neighbours of STORED rows: rows (nq,) int32 in id_base (numpy / device tensor as the index).  The rows are decoded on the device (with the
        centroid of their list when add_coarse) and searched: nprobe=0 is search(reconstruct(rows), k), nprobe>=1 is search_ivf(reconstruct(rows,
        add_coarse), k, nprobe, add_coarse=add_coarse) -- bit for bit, the filter in force included.  No self-exclusion: a row is returned like any
        other, and with quantised norms it need not come first.
        -> dists (nq,k) float32 ascending, ids (nq,k) int32 1-BASED   [lsq_index_search_rows]"""
        side, p = self._side, self._side.ptr
        rows = side.take(rows, _I32, "rows")
        _shapes(("rows", rows, (None,)))
        nq = int(rows.shape[0])
        dists, ids = side.topk(nq, int(k), self._eng._device() if side.dev else None)
        fl = _lib.IVF_ADD_COARSE if add_coarse else 0
        self._eng._call(side, "lsq_index_search_rows", p(dists), p(ids), p(rows) if nq else None, nq, int(id_base), int(k), int(nprobe), fl, int(self._dev),
                        h=self._h)
        return dists, ids

    def recon_info(self):
        """the last reconstruct / search_rows call: rows decoded, invalid ids, map_rebuilt (the row -> list map was built by it), map_rebuilds and calls
        (since creation), road (_lib.RECON_ROAD_*), map_ms / decode_ms (with profile=True)"""
        return self._info("lsq_index_get_recon_info", _lib.IndexReconInfo)

    def _format(self):
        """the format of the base rows (_lib.BASE_*)"""
        return getattr(self, "_fmt", _lib.BASE_U8 if self._u8 else _lib.BASE_F32)

    def narrow_base(self, fmt):
        """Convert the index's resident FLOAT32 base rows, on the device, into half-precision rows the index owns ("f16" / "bf16", round to nearest
        even; dense rows).  Afterwards the index is the index created over the narrowed rows: 2 d bytes per row instead of 4 d.  A borrowed float32
        tensor is left untouched and no longer used.  Both copies exist until the call returns.  base_info() reports what narrowing cost: values that
        became inf or zero   [lsq_index_narrow_base]"""
        code = base_format_code(fmt)
        if code is None:
            raise ValueError("narrow_base needs a format: \"f16\" or \"bf16\"")
        self._eng._call(self._side, "lsq_index_narrow_base", code, h=self._h)
        self._fmt, self._u8 = code, False

    def base_info(self):
        """format (_lib.BASE_*), elem_bytes, ldb, owned, resident_bytes of the base rows (all zero without any); to_inf / to_zero / nans and narrow_ms
        (with profile=True) of the last narrow_base"""
        return self._info("lsq_index_get_base_info", _lib.IndexBaseInfo)

    def base_rows(self, start=0, count=None, out=None):
        """The STORED base rows start .. start + count - 1 (count=None: to the last row), widened to float32 whatever their format -- reconstruct()
        returns what the codes stand for, this what the re-rank reads.  A filter changes nothing.  out: (count, >=d) float32 rows to write into (numpy
        on an Engine.index, a device tensor on an Engine.index_dev)
        -> (count, d) float32   [lsq_index_get_base]"""
        side, p = self._side, self._side.ptr
        count = self.n - int(start) if count is None else int(count)
        if out is None:
            out = side.new((max(count, 0), self.d), _F32, self._eng._device() if side.dev else None, zero=True)
        elif side.dev:
            out = side.take(out, _F32, "out", rows=True)
        elif not (isinstance(out, np.ndarray) and out.dtype == _F32 and out.ndim == 2 and out.strides[1] == 4 and out.strides[0] % 4 == 0):
            raise ValueError("out must be a 2-d float32 numpy array of rows with unit column stride")
        _shapes(("out", out, (max(count, 0), max(self.d, out.shape[1]))))
        ldo = int(side.pitch(out)) if out.shape[0] > 1 else int(out.shape[1])
        self._eng._call(side, "lsq_index_get_base", p(out) if count > 0 else None, int(start), count, ldo, int(self._dev), h=self._h)
        return out

    # -- snapshots: the logical state saved, loaded, exported, digested ------------------------
    @classmethod
    def _loaded(cls, engine, path, dev):
        self = cls.__new__(cls)
        self._bind(engine, dev)
        handle = C.c_void_p()
        engine._call(self._side, "lsq_index_load", engine._h, os.fsencode(path), 0, h=C.byref(handle))
        self._h = handle
        engine._indexes.add(self)
        self._keep = ()
        sc = self._snapshot_scalars()
        self.n, self.d, self.m = int(sc.n), int(sc.d), int(sc.m)
        self._fmt, self._u8 = int(sc.base_format), int(sc.base_format) == _lib.BASE_U8
        if sc.nlist:
            self.nlist = int(sc.nlist)
        return self

    def _snapshot_scalars(self):
        """the scalars of the logical state (an export that asks for no array); what the index has follows from them"""
        a = _lib.SnapshotArrays()
        self._eng._call(_HOST, "lsq_index_export", C.byref(a), 0, h=self._h)
        self._has_codes, self._has_base, self._packed = a.m > 0, self._has_base_rows(), bool(a.packed)
        return a

    def _has_base_rows(self):
        return bool(self.base_info()["elem_bytes"])

    def save(self, path):
        """Write the index's logical state -- the arrays a caller would pass to build it fresh, after every add / remove / compact -- to the snapshot
        file `path` (a temporary beside it, renamed on success).  The file is a function of that state alone: equal indexes save equal bytes
        [lsq_index_save]"""
        self._eng._call(self._side, "lsq_index_save", os.fsencode(path), 0, h=self._h)

    def export(self, dev=False):
        """The logical state as arrays: a dict with only the keys the index has -- codebooks (m*256,d), codes (n,m), dbnorms (n,) or norm_codes (n,) +
        cbnorms (ncb,), base (n,d) in the stored format (bfloat16 rows: uint16 bits on the host), centroids (nlist,d) + list_of_row (n,), filter_bits
        (ceil(n/32),) uint32 + filter_force -- numpy arrays, or torch device tensors with dev=True   [lsq_index_export]"""
        sc = self._snapshot_scalars()
        side = _DEVICE if dev else _HOST
        n, d, m = int(sc.n), int(sc.d), int(sc.m)
        like = self._eng._device() if dev else None
        want = {}
        if m:
            want["codebooks"], want["codes"] = ((m * H, d), _F32), ((n, m), _U8)
            if sc.packed:
                want["norm_codes"], want["cbnorms"] = ((n,), _U8), ((int(sc.ncb),), _F32)
            else:
                want["dbnorms"] = ((n,), _F32)
        if self._has_base:
            fmt = int(sc.base_format)
            host_dt = {_lib.BASE_F32: _F32, _lib.BASE_U8: _U8, _lib.BASE_F16: np.float16, _lib.BASE_BF16: np.uint16}[fmt]
            want["base"] = ((n, d), host_dt)
        if sc.nlist:
            want["centroids"], want["list_of_row"] = ((int(sc.nlist), d), _F32), ((n,), _I32)
        if sc.filter_active:
            want["filter_bits"] = (((n + 31) // 32,), np.uint32)
        out, a = {}, _lib.SnapshotArrays()
        for key, (shape, dt) in want.items():
            if not dev:
                out[key] = np.zeros(shape, dtype=dt)
            else:
                import torch
                tdt = {"uint32": torch.int32, "uint16": torch.bfloat16}.get(np.dtype(dt).name) or getattr(torch, np.dtype(dt).name)
                out[key] = torch.empty(shape, dtype=tdt, device=like)      # (filter_bits: the uint32 words as int32; bfloat16 rows as torch.bfloat16)
            setattr(a, key, side.ptr(out[key]))
        self._eng._call(side, "lsq_index_export", C.byref(a), int(dev), h=self._h)
        if sc.filter_active:
            out["filter_force"] = int(a.filter_force)
        return out

    def digest(self):
        """Scalars and per-section digests of the logical state, computed on the device; equal to snapshot_info() of the file save() would write: n, d, m,
        ..., file_bytes, header_digest, sections = [{name, kind, elem_bytes, offset, bytes, digest}]   [lsq_index_digest]"""
        return self._info("lsq_index_digest", _lib.SnapshotInfo)

    def snapshot_info(self):
        """the last save() of this index, or the load that made it: op (1 save, 2 load), bytes, chunks, chunk_bytes, sections, host_staging_bytes, file_ms,
        total_ms and, with profile=True, derive_ms / digest_ms / copy_ms   [lsq_index_get_snapshot_info]"""
        return self._info("lsq_index_get_snapshot_info", _lib.SnapshotIoInfo)



# -- the beam-search encoder (made by Engine.encoder / Engine.encoder_dev) ------------------------

class Encoder(_Handle):
    """Beam search over the full pair tables on codebooks resident on an Engine's device   [lsq_encoder_*]: deterministic codes that can replace the
    random start of an ILS encode.  Made by Engine.encoder (host arrays in and out) or Engine.encoder_dev (torch tensors in and out)."""

    _destroy = "lsq_encoder_destroy"

    def __init__(self, engine, K, m, chunk, h, on_device):
        side = self._bind(engine, on_device)
        K = side.take(K, _F32, "K")
        _shapes(("K", K, (int(m) * h, None)))
        desc = _lib.EncoderDesc()
        desc.d, desc.m, desc.h, desc.codebooks, desc.on_device, desc.chunk = int(K.shape[1]), int(m), int(h), side.ptr(K), int(self._dev), int(chunk)
        self.d, self.m = int(K.shape[1]), int(m)
        self._create("lsq_encoder_create", desc)      # the codebooks are copied: K is not kept

    def beam(self, X, L, order=None, want_score=False):
        """X (n,d) float32 or uint8 rows (the un-widened bytes of a .bvecs set: the bits of the float32 call), beam width 1 <= L <= 32, order: the
        codebooks' visiting order (a permutation of range(m), host integers; None: ascending).
        -> codes (n,m): int16 1-based (host) / uint8 0-based (device: the B0 of encode_icm_dev) [, score (n,) float32: ||x||^2 + score is the
        vector's veccost]   [lsq_encoder_beam]"""
        side = self._side
        X, u8 = side.take_x(X, "X")
        _shapes(("X", X, (None, self.d)))
        n, p = X.shape[0], side.ptr
        o = None if order is None else _HOST.take(order, _I32, "order").reshape(-1)
        if o is not None:
            _shapes(("order", o, (self.m,)))
        codes = side.new((n, self.m), side.codes, X)
        score = side.new(n, _F32, X) if want_score else None
        self._eng._call(side, "lsq_encoder_beam", p(X), int(u8), n, int(L), _array_address(o), p(codes), p(score), int(self._dev), h=self._h)
        return (codes, score) if want_score else codes

    def info(self):
        """the last beam call: vectors, chunks, beam, unaries_ms / beam_ms (with profile=True)"""
        return self._info("lsq_encoder_get_info", _lib.EncoderInfo)


# -- the coarse partition (made by Engine.partition / Engine.partition_dev) -----------------------

class Partition(_Handle):
    """nlist coarse centroids resident on an Engine's device and the four steps that build a residual inverted-list index on them   [lsq_partition_*]:
    assign (the nearest centroid, Index.search_ivf's own rule), update (one Lloyd half-step, numpy's float64 bits), residuals (x - c) and code_norms
    (|r^|^2 + 2 <c, r^>, the dbnorms or norm bytes of a residual index).  Rows X (n,d) are float32 or uint8 (the un-widened bytes of a .bvecs set) and
    may be row views: unit column stride, any pitch, uint8 at any byte offset.  Made by Engine.partition (host arrays in and out) or
    Engine.partition_dev (torch tensors in and out)."""

    _destroy = "lsq_partition_destroy"

    def __init__(self, engine, centroids, on_device):
        side = self._bind(engine, on_device)
        cent = side.take(centroids, _F32, "centroids")
        _shapes(("centroids", cent, (None, None)))
        desc = _lib.PartitionDesc()
        desc.nlist, desc.d, desc.centroids, desc.on_device = int(cent.shape[0]), int(cent.shape[1]), side.ptr(cent), int(self._dev)
        self.nlist, self.d = int(cent.shape[0]), int(cent.shape[1])
        self._create("lsq_partition_create", desc)    # the centroids are copied: cent is not kept

    def _rows(self, X, name, dtype=None):
        """rows read (or, with dtype, written) in place -> (array, is_u8).  The device side verifies; the host side converts what is not already a row
        view of the right type"""
        side = self._side
        if side.dev:
            X, u8 = (side.take(X, dtype, name, rows=True), False) if dtype else side.take_x(X, name, rows=True)
            if X.shape[0] > 1 and X.stride(0) < X.shape[1]:
                raise ValueError("%s: rows must be at least d elements apart (got strides %s)" % (name, X.stride()))
        else:
            if _dtname(X) == "int8":
                raise TypeError("int8 data is not accepted: 8-bit base sets are unsigned (uint8); view or convert the array explicitly")
            u8 = dtype is None and _dtname(X) == "uint8"
            want = dtype or (_U8 if u8 else _F32)
            if dtype is not None and (not isinstance(X, np.ndarray) or X.dtype != dtype):
                raise TypeError("%s must be a %s array (it is written in place)" % (name, dtype.__name__))
            X = np.asarray(X, dtype=want)
            if X.ndim != 2 or X.strides[1] != X.itemsize or X.strides[0] % X.itemsize or (X.shape[0] > 1 and X.strides[0] < X.shape[1] * X.itemsize):
                if dtype is not None:
                    raise ValueError("%s must be 2-d rows with unit column stride (it is written in place)" % name)
                X = np.ascontiguousarray(X)
        _shapes((name, X, (None, self.d)))
        return X, u8

    def _lists(self, assign, n):
        lor = self._side.take(assign, _I32, "assign")
        _shapes(("assign", lor, (n,)))
        return lor

    def assign(self, X, want_dist=False):
        """-> assign (n,) int32 0-based: the nearest centroid of every row by the exact search's rule (ties to the smaller list, NaN last) -- ivf_assign's
        ids [, dist (n,) float32: the distance]   [lsq_partition_assign]"""
        side = self._side
        X, u8 = self._rows(X, "X")
        n, p = X.shape[0], side.ptr
        lor = side.new(n, _I32, X, zero=True)
        dist = side.new(n, _F32, X, zero=True) if want_dist else None
        if n:
            self._eng._call(side, "lsq_partition_assign", p(X), int(u8), n, int(side.pitch(X)), p(lor), p(dist), int(self._dev), h=self._h)
        return (lor, dist) if want_dist else lor

    def update(self, X, assign, want_counts=False):
        """One Lloyd half-step: every list with rows gets the mean of its rows -- float64 sums in ascending row id, divided by the count, rounded to
        float32 (train_coarse's numpy bits) --, a list without rows keeps its centroid.  -> counts (nlist,) int32 or None   [lsq_partition_update]"""
        side = self._side
        X, u8 = self._rows(X, "X")
        n, p = X.shape[0], side.ptr
        lor = self._lists(assign, n)
        counts = side.new(self.nlist, _I32, X, zero=True) if want_counts else None
        self._eng._call(side, "lsq_partition_update", p(X) if n else None, int(u8), n, int(side.pitch(X)), p(lor) if n else None, p(counts),
                        int(self._dev), h=self._h)
        return counts

    def residuals(self, X, assign, out=None):
        """-> R (n,d) float32, R[i] = X[i] - centroid[assign[i]] (one rounded subtraction; uint8 rows widened first).  out: float32 rows written in
        place (a row view with a pitch of its own is allowed: nothing between the rows is touched)   [lsq_partition_residuals]"""
        side = self._side
        X, u8 = self._rows(X, "X")
        n, p = X.shape[0], side.ptr
        lor = self._lists(assign, n)
        R = side.new((n, self.d), _F32, X) if out is None else self._rows(out, "out", _F32)[0]
        _shapes(("out", R, (n, self.d)))
        if n:
            self._eng._call(side, "lsq_partition_residuals", p(X), int(u8), n, int(side.pitch(X)), p(lor), p(R), int(side.pitch(R)), int(self._dev), h=self._h)
        return R

    def code_norms(self, codes, K, assign, cbnorms=None, h=H):
        """The scalar a residual row stores: s = |r^|^2 + 2 <c, r^> in float32 chains (r^: the reconstruction of the row's codes, c: its list's centroid).
        codes (n,m) uint8 0-based, K (m*h,d).  cbnorms=None -> norms (n,) float32 (the input of the norm k-means).  cbnorms (<= 256,) -> (norms, norm_codes
        (n,) uint8: the first nearest entry, dbnorms (n,) = cbnorms[norm_codes]): what Engine.index / index_packed take   [lsq_partition_code_norms]"""
        side = self._side
        codes, K = side.take(codes, _U8, "codes"), side.take(K, _F32, "K")
        cb = None if cbnorms is None else side.take(cbnorms, _F32, "cbnorms").reshape(-1)
        _shapes(("codes", codes, (None, None)), ("K", K, (None, self.d)))
        (n, m), p = codes.shape, side.ptr
        _shapes(("K", K, (m * h, self.d)))
        lor = self._lists(assign, n)
        norms = side.new(n, _F32, K, zero=True)
        nc, dbn = (None, None) if cb is None else (side.new(n, _U8, K, zero=True), side.new(n, _F32, K, zero=True))
        self._eng._call(side, "lsq_partition_code_norms", p(codes) if n else None, p(K), n, int(m), int(h), p(lor) if n else None, p(cb),
                        0 if cb is None else int(cb.shape[0]), p(norms), p(nc), p(dbn), int(self._dev), h=self._h)
        return norms if cb is None else (norms, nc, dbn)

    def centroids(self):
        """-> the current centroids (nlist,d) float32: a copy   [lsq_partition_get_centroids]"""
        side = self._side
        out = side.new((self.nlist, self.d), _F32, self._eng._device())
        self._eng._call(side, "lsq_partition_get_centroids", side.ptr(out), int(self._dev), h=self._h)
        return out

    def info(self):
        """the last call: call (1 assign, 2 update, 3 residuals, 4 code_norms), rows, lists_touched / empty_lists / max_list_rows (update), loader_bytes
        (residuals: 16, 4 or 1), group_ms / kernel_ms (with profile=True)"""
        return self._info("lsq_partition_get_info", _lib.PartitionInfo)


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
        X, u8, B, K, n, d, ils = _encode_args(_HOST, X, B, K, m, h, ilsiters)
        nr, p = ils.shape[0], _HOST.ptr
        Bs, objs = _HOST.new((nr, n, m), _I16), _HOST.new(nr, _F32, zero=True)
        call = self._L.lsq_multi_encode_icm_u8 if u8 else self._L.lsq_multi_encode_icm      # the devices split the rows: no nsplits
        _lib.check(call(self._h, p(X), p(B), p(K), d, n, m, h, p(ils), nr, int(icmiter), int(npert), int(bool(randord)), int(seed), int(global_offset),
                        int(bool(verbose)), p(Bs), p(objs)))
        return Bs, objs

    def linscan(self, codes, Q, K, dbnorms, m, k, h=H):
        """the ADC scan over a database sharded across the devices; Engine.linscan's signature and results   [lsq_multi_linscan]"""
        result, args = _linscan_args(_HOST, codes, Q, K, dbnorms, m, k, h)
        _lib.check(self._L.lsq_multi_linscan(self._h, *args))
        return result

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
