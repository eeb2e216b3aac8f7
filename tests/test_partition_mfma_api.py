"""The boundary of Partition.assign on the matrix cores (option "partition_mfma"; csrc/lsq_passign.hip) without a GPU: the header, both libraries and the
ctypes table agree on the one new symbol and on its account struct, and the getter refuses null arguments on the host."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_struct_and_version(lsq):
    B = lsq._lib
    hdr = open(os.path.join(ROOT, "include", "lsq_mi355x.h")).read()
    assert re.search(r"LSQ_API int lsq_partition_get_mfma_info\(lsq_partition \*p, lsq_partition_mfma_info \*out\);", hdr)
    assert int(re.search(r"#define LSQ_VERSION (\d+)", hdr).group(1)) >= 3300 and B.load().lsq_version() >= 3300
    assert B.SIGNATURES["lsq_partition_get_mfma_info"] == (C.c_int, [C.c_void_p, C.POINTER(B.PartitionMfmaInfo)])
    assert hasattr(C.CDLL(B.LIB_PATH), "lsq_partition_get_mfma_info") and hasattr(C.CDLL(B.TUNING_LIB_PATH), "lsq_partition_get_mfma_info")
    body = re.search(r"typedef struct lsq_partition_mfma_info \{(.*?)\} lsq_partition_mfma_info;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(\w+)\s*[,;]", body)
    kinds = [C.c_int64 if kind == "int64_t" else C.c_double for kind, names in re.findall(r"(int64_t|double)\s+([^;]+);", body) for _ in names.split(",")]
    assert fields == [name for name, _ in B.PartitionMfmaInfo._fields_] and kinds == [t for _, t in B.PartitionMfmaInfo._fields_]
    assert kinds == [C.c_int64] * 13 + [C.c_double] * 6 and C.sizeof(B.PartitionMfmaInfo) == 19 * 8      # sizeof as the header lays it out: no padding
    for name, value in (("NOT_ASKED", 1), ("WIDE", 2)):
        assert getattr(B, "PARTITION_MFMA_" + name) == value and re.search(r"LSQ_PARTITION_MFMA_%s = %d\b" % (name, value), hdr)


def test_getter_refuses_null(lsq):
    L = lsq._lib.load()
    assert L.lsq_partition_get_mfma_info(None, C.byref(lsq._lib.PartitionMfmaInfo())) == lsq._lib.LSQ_EINVAL
    assert b"lsq_partition_get_mfma_info" in L.lsq_last_error()
