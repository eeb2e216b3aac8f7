"""The boundary of exact k-NN on the i8 matrix cores (option "knn_u8_mfma"; csrc/lsq_knnu.hip) without a GPU: the header, the library and the ctypes table
agree on the one new symbol and on its account struct, and the getter refuses null arguments on the host."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_struct_and_version(lsq):
    hdr = open(os.path.join(ROOT, "include", "lsq_mi355x.h")).read()
    assert re.search(r"LSQ_API int lsq_index_get_knn_mfma_info\(lsq_index \*ix, lsq_knn_mfma_info \*out\);", hdr)
    assert int(re.search(r"#define LSQ_VERSION (\d+)", hdr).group(1)) >= 2800 and lsq._lib.load().lsq_version() >= 2800
    res, args = lsq._lib.SIGNATURES["lsq_index_get_knn_mfma_info"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(lsq._lib.KnnMfmaInfo)]
    body = re.search(r"typedef struct lsq_knn_mfma_info \{(.*?)\} lsq_knn_mfma_info;", hdr, flags=re.S).group(1)
    fields = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [name for name, _ in lsq._lib.KnnMfmaInfo._fields_] == ["served", "reason", "pairs", "kept", "norms_ms", "scan_ms"]
    assert C.sizeof(lsq._lib.KnnMfmaInfo) == 48
    for name, value in (("NOT_ASKED", 1), ("NOT_INTEGER_ROAD", 2), ("FILTERED", 3), ("EXHAUSTIVE", 4)):
        assert getattr(lsq._lib, "KNN_MFMA_" + name) == value and re.search(r"LSQ_KNN_MFMA_%s = %d\b" % (name, value), hdr)


def test_getter_refuses_null(lsq):
    L = lsq._lib.load()
    assert L.lsq_index_get_knn_mfma_info(None, C.byref(lsq._lib.KnnMfmaInfo())) == lsq._lib.LSQ_EINVAL
    assert b"lsq_index_get_knn_mfma_info" in L.lsq_last_error()
