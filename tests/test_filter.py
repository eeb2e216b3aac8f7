"""Row filters on the resident index, the parts that need no GPU: the C ABI of lsq_index_set_filter / lsq_index_get_filter_info (v2000), the binding's
structs against the header's, the refusals that need no device, and the numpy statement of the contract (tests/filter_check.py: filtered) against a
brute-force restatement on a small example with ties, a NaN and nn > |A|."""
import ctypes as C
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_check as FC  # noqa: E402
from knn_check import order_keys  # noqa: E402
from packed_check import header, header_struct_fields  # noqa: E402

NEW = ("lsq_index_set_filter", "lsq_index_get_filter_info")
EINVAL = -1


def test_header_declares_the_symbols_and_structs(lsq):
    hdr = header()
    assert int(re.search(r"#define LSQ_VERSION (\d+)", hdr).group(1)) >= 2000
    declared = set(re.findall(r"LSQ_API\s+[\w\s\*]*?\b(lsq_\w+)\s*\(", hdr))
    assert set(NEW) <= declared
    first = set(re.findall(r"\b(lsq_\w+)\s*\(\s*(?:struct\s+)?lsq_ctx\s*\*", hdr))      # neither takes the context first: the context walks stay closed
    assert not first & set(NEW)
    assert header_struct_fields("lsq_filter_desc") == ["form", "data", "count", "id_base", "flags", "on_device"]
    assert header_struct_fields("lsq_filter_info") == ["active", "n", "allowed", "lists", "lists_without_allowed", "road", "crossover_rows"]
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, value in (("LSQ_FILTER_BITS", 0), ("LSQ_FILTER_BYTES", 1), ("LSQ_FILTER_IDS", 2), ("LSQ_FILTER_DENY", 1), ("LSQ_FILTER_FORCE_DENSE", 2),
                        ("LSQ_FILTER_FORCE_COMPACT", 4)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), code), name


def test_both_libraries_export_them_at_v2000(lsq):
    for tuning in (False, True):
        L = lsq._lib.load(tuning=tuning)
        assert L.lsq_version() >= 2000
        raw = C.CDLL(lsq._lib.TUNING_LIB_PATH if tuning else lsq._lib.LIB_PATH)
        for name in NEW:
            assert hasattr(raw, name), name


def test_binding_structs_equal_the_headers(lsq):
    B = lsq._lib
    assert [f for f, _ in B.FilterDesc._fields_] == header_struct_fields("lsq_filter_desc")
    assert [f for f, _ in B.FilterInfo._fields_] == header_struct_fields("lsq_filter_info")
    assert [t for _, t in B.FilterDesc._fields_] == [C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int]
    assert all(t is C.c_int64 for _, t in B.FilterInfo._fields_) and C.sizeof(B.FilterInfo) == 56
    assert C.sizeof(B.FilterDesc) == 40                                    # int, pad, pointer, int64, three ints, pad
    assert (B.FILTER_BITS, B.FILTER_BYTES, B.FILTER_IDS) == (0, 1, 2) and (B.FILTER_DENY, B.FILTER_FORCE_DENSE, B.FILTER_FORCE_COMPACT) == (1, 2, 4)
    assert set(NEW) <= set(B.SIGNATURES)


def test_null_handles_are_refused_without_a_device(lsq):
    L = lsq._lib.load()
    desc, info = lsq._lib.FilterDesc(), lsq._lib.FilterInfo()
    assert L.lsq_index_set_filter(None, C.byref(desc)) == EINVAL and b"lsq_index_set_filter" in L.lsq_last_error()
    assert L.lsq_index_set_filter(None, None) == EINVAL                    # clearing needs a handle too
    assert L.lsq_index_get_filter_info(None, C.byref(info)) == EINVAL and b"lsq_index_get_filter_info" in L.lsq_last_error()


def _brute(full_d, full_ids, allowed, nn, pad_id):
    """the contract said the long way: the (dist, id) pairs of the allowed rows, sorted by (key of dist, id), cut to nn, padded"""
    out_d, out_i = [], []
    for q in range(full_d.shape[0]):
        pairs = [(int(order_keys(full_d[q, j:j + 1])[0]), int(full_ids[q, j]), full_d[q, j]) for j in range(full_d.shape[1])
                 if full_ids[q, j] != pad_id and allowed[int(full_ids[q, j]) - (pad_id + 1)]]
        pairs.sort(key=lambda t: (t[0], t[1]))
        pairs = pairs[:nn]
        out_d.append([p[2] for p in pairs] + [np.float32(np.inf)] * (nn - len(pairs)))
        out_i.append([p[1] for p in pairs] + [pad_id] * (nn - len(pairs)))
    return np.asarray(out_d, dtype=np.float32), np.asarray(out_i, dtype=np.int32)


def test_filtered_is_the_contract_on_a_small_example():
    """12 rows, two queries: ties (rows 2, 5, 9 at distance 1), a real +inf, a NaN (after every number, before the padding), nn above |A|"""
    dist = np.array([[3, 0.5, 1, 7, np.inf, 1, -2, np.nan, 4, 1, 6, 2],
                     [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]], dtype=np.float32)
    n = dist.shape[1]
    for id_base in (0, 1):
        pad_id = id_base - 1
        keys = (order_keys(dist).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]
        order = np.argsort(keys, axis=1, kind="stable")
        full_d, full_ids = np.take_along_axis(dist, order, axis=1), order + id_base
        for allowed in (np.ones(n, bool), np.zeros(n, bool), np.arange(n) % 2 == 1, np.isin(np.arange(n), [2, 4, 7, 9]), np.isin(np.arange(n), [7])):
            for nn in (1, 3, 5, 12):
                d, i = FC.filtered(full_d, full_ids, allowed, nn, pad_id)
                bd, bi = _brute(full_d, full_ids, allowed, nn, pad_id)
                assert FC.same((d, i), (bd, bi)), (id_base, allowed.tolist(), nn)
                k = min(nn, int(allowed.sum()))
                assert np.all(i[:, k:] == pad_id) and np.all(np.isposinf(d[:, k:])) and np.all(i[:, :k] != pad_id)
        d, i = FC.filtered(full_d, full_ids, np.isin(np.arange(n), [2, 4, 7, 9]), 5, pad_id)
        assert i[0].tolist() == [2 + id_base, 9 + id_base, 4 + id_base, 7 + id_base, pad_id]      # tie by id, +inf, NaN, padding
        assert np.isnan(d[0, 3]) and np.isposinf(d[0, 2]) and np.isposinf(d[0, 4])
    # a ranking that carries padding of its own (search_ivf's (+inf, 0) past the probed rows): dropped, never returned as a row
    d, i = FC.filtered(np.array([[1, 2, np.inf, np.inf]], np.float32), np.array([[3, 1, 0, 0]]), np.array([True, False, True]), 3, 0)
    assert i.tolist() == [[3, 1, 0]] and np.isposinf(d[0, 2])


def test_mask_helpers_agree():
    for n in (64, 1000, 1024):
        for name, allowed in FC.masks(n).items():
            bits = FC.to_bits(allowed)
            back = np.unpackbits(bits.view(np.uint8), bitorder="little")[:n].astype(bool)
            assert np.array_equal(back, allowed), (n, name)
            for label, kw in FC.forms(allowed):
                if "ids" in kw:
                    rows = np.unique(kw["ids"] - kw["id_base"])
                    want = np.flatnonzero(~allowed if kw.get("deny") else allowed)
                    assert np.array_equal(rows, want), (n, name, label)
    assert int(FC.masks(1000)["seven"].sum()) == 7 and FC.masks(1000)["last-word"].sum() == 8
