"""CPU tests of the 8-bit encode interface (no GPU needed): the header declares lsq_encode_icm_u8 / lsq_encode_icm_u8_dev / lsq_multi_encode_icm_u8,
the library exports them, _lib.py binds them with the argument lists of the calls they stand in for, and the Python layers hand a uint8 matrix to the
new symbols as it is -- no silent astype(float32) on the way.  The calls are recorded by a stand-in for the ctypes library, so no device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from engine_calls import _Recorder, _offline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 256
U8 = {"lsq_encode_icm_u8": "lsq_encode_icm", "lsq_encode_icm_u8_dev": "lsq_encode_icm_dev", "lsq_multi_encode_icm_u8": "lsq_multi_encode_icm"}


def _header():
    return open(os.path.join(ROOT, "include", "lsq_mi355x.h")).read()


def _prototype(hdr, name):
    m = re.search(r"LSQ_API\s+int\s+%s\s*\((.*?)\);" % name, hdr, flags=re.S)
    assert m, "%s is not declared in include/lsq_mi355x.h" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_u8_entry_points_with_their_counterparts_argument_lists():
    hdr = _header()
    assert int(re.search(r"#define\s+LSQ_VERSION\s+(\d+)", hdr).group(1)) >= 1300
    for new, old in U8.items():
        a, b = _prototype(hdr, new), _prototype(hdr, old)
        assert len(a) == len(b), (new, a, b)
        assert a[1].startswith("const uint8_t *") and b[1].startswith("const float *"), (a[1], b[1])      # the data matrix: the one argument that differs
        strip = lambda s: re.sub(r"\w+$", "", s).replace("struct lsq_ctx", "lsq_ctx")                    # types only (the tag spelling names the same type)
        assert [strip(x) for x in a[:1] + a[2:]] == [strip(x) for x in b[:1] + b[2:]], (new, a, b)
        assert old in hdr[hdr.index("(1b) the whole call on 8-bit data"):], "the header does not say what %s stands in for" % new


def test_library_exports_and_binds_the_u8_entry_points(lsq):
    raw = C.CDLL(lsq._lib.LIB_PATH)
    for new, old in U8.items():
        assert hasattr(raw, new), "liblsq_mi355x.so does not export %s" % new
        assert lsq._lib.SIGNATURES[new] == lsq._lib.SIGNATURES[old]
        assert getattr(lsq._lib.load(), new).argtypes == lsq._lib.SIGNATURES[new][1]
    assert lsq._lib.load().lsq_version() >= 1300
    assert lsq._lib.load(tuning=True).lsq_version() == lsq._lib.load().lsq_version()


def test_null_context_is_einval(lsq):
    """the first check of every entry point needs no device: a null context / null lsq_multi"""
    L = lsq._lib.load()
    ils = np.array([1], dtype=np.int64)
    assert L.lsq_encode_icm_u8(None, None, None, None, 8, 4, 2, H, ils.ctypes.data, 1, 1, 1, 1, 1, 0, 0, 0, None, None) == lsq._lib.LSQ_EINVAL
    assert L.lsq_encode_icm_u8_dev(None, None, None, None, 8, 4, 2, H, ils.ctypes.data, 1, 1, 1, 1, 0, 0, None, None, None) == lsq._lib.LSQ_EINVAL
    assert L.lsq_multi_encode_icm_u8(None, None, None, None, 8, 4, 2, H, ils.ctypes.data, 1, 1, 1, 1, 0, 0, 0, None, None) == lsq._lib.LSQ_EINVAL
    assert b"null" in L.lsq_last_error()


def _problem(n=6, d=8, m=2, seed=0):
    rng = np.random.default_rng(seed)
    X8 = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
    K = rng.standard_normal((m * H, d)).astype(np.float32)
    B = rng.integers(1, H + 1, size=(n, m)).astype(np.int16)
    return X8, K, B


def _encode_calls(obj):
    return [c for c in obj._L.calls if "encode_icm" in c[0]]


@pytest.mark.parametrize("cls, u8_symbol, f32_symbol", [("Engine", "lsq_encode_icm_u8", "lsq_encode_icm"),
                                                        ("MultiEngine", "lsq_multi_encode_icm_u8", "lsq_multi_encode_icm")])
def test_uint8_reaches_the_u8_symbol_unwidened(lsq, cls, u8_symbol, f32_symbol):
    X8, K, B = _problem()
    eng = _offline(getattr(lsq, cls))
    eng.encode_icm(X8, B, K, 2, [1], 1, 1, True)
    (name, args), = _encode_calls(eng)
    assert name == u8_symbol
    assert args[1] == X8.ctypes.data, "the uint8 matrix was copied or converted on its way to the library"
    assert (args[4], args[5], args[6]) == (8, 6, 2)
    # float32, float64 and lists behave as they always did
    for X in (X8.astype(np.float32), X8.astype(np.float64), X8.astype(np.float32).tolist()):
        eng._L.calls.clear()
        eng.encode_icm(X, B, K, 2, [1], 1, 1, True)
        assert [c[0] for c in _encode_calls(eng)] == [f32_symbol]


def test_non_contiguous_uint8_is_copied_as_f32_is(lsq):
    big = np.random.default_rng(1).integers(0, 256, size=(6, 16), dtype=np.uint8)
    view = big[:, ::2]                                     # (6, 8), strides (16, 2)
    assert not view.flags["C_CONTIGUOUS"]
    _, K, B = _problem()
    seen = {}

    class Peek(_Recorder):
        def __getattr__(self, name):
            def fn(*args):
                if name == "lsq_encode_icm_u8":            # the bytes the library would read: 6 x 8 contiguous uint8
                    seen["rows"] = np.ctypeslib.as_array(C.cast(args[1], C.POINTER(C.c_uint8)), shape=(6, 8)).copy()
                self.calls.append((name, args))
                return 0
            return fn

    eng = _offline(lsq.Engine)
    eng._L = Peek()
    eng.encode_icm(view, B, K, 2, [1], 1, 1, True)
    assert [c[0] for c in _encode_calls(eng)] == ["lsq_encode_icm_u8"]
    assert np.array_equal(seen["rows"], view)


def test_int8_is_refused(lsq):
    X8, K, B = _problem()
    for cls in (lsq.Engine, lsq.MultiEngine):
        eng = _offline(cls)
        with pytest.raises(TypeError, match="int8"):
            eng.encode_icm(X8.view(np.int8), B, K, 2, [1], 1, 1, True)
        assert _encode_calls(eng) == []
    eng = _offline(lsq.Engine)
    with pytest.raises(TypeError, match="int8"):
        lsq.encode_icm_cuda(X8.view(np.int8).T, B.T, [K[j * H:(j + 1) * H].T for j in range(2)], [1], 1, 1, True, engine=eng)


def test_encode_icm_cuda_takes_what_bvecs_read_returns(lsq, tmp_path):
    X8, K, B = _problem(n=5, d=12)
    path = tmp_path / "base.bvecs"
    with open(path, "wb") as f:
        for row in X8:
            f.write(np.int32(12).tobytes())
            f.write(row.tobytes())
    RX = lsq.bvecs_read(None, str(path))
    assert RX.dtype == np.uint8 and RX.shape == (12, 5) and np.array_equal(RX.T, X8)
    eng = _offline(lsq.Engine)
    Cs = [np.ascontiguousarray(K[j * H:(j + 1) * H].T) for j in range(2)]      # the reference's list of d x h codebooks
    Bs, objs = lsq.encode_icm_cuda(RX, B.T, Cs, [1, 2], 1, 1, True, engine=eng)
    (name, args), = _encode_calls(eng)
    assert name == "lsq_encode_icm_u8" and (args[4], args[5], args[6]) == (12, 5, 2)
    got = np.ctypeslib.as_array(C.cast(args[1], C.POINTER(C.c_uint8)), shape=(5, 12))
    assert np.array_equal(got, X8)
    assert len(Bs) == 2 and Bs[0].shape == (2, 5) and objs.shape == (2,)
    # and a float matrix still takes the f32 call
    eng._L.calls.clear()
    lsq.encode_icm_cuda(RX.astype(np.float32), B.T, Cs, [1], 1, 1, True, engine=eng)
    assert [c[0] for c in _encode_calls(eng)] == ["lsq_encode_icm"]
