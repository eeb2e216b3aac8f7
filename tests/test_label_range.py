"""Labelled range search without a GPU: the two symbols of v3400 in the header and the binding, and the routing of Index.range_search."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_calls as ec  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols(lsq):
    """both take the index handle first (the catalogue of context symbols does not grow); the argument types are the header's"""
    B = lsq._lib
    hdr = open(os.path.join(ROOT, "include", "lsq_mi355x.h")).read()
    assert int(re.search(r"#define LSQ_VERSION (\d+)", hdr).group(1)) >= 3400 and B.load().lsq_version() >= 3400 and B.load(tuning=True).lsq_version() >= 3400
    for name in ("lsq_index_range_search_labelled", "lsq_index_get_label_range_info"):
        assert re.search(r"LSQ_API int %s\(lsq_index \*ix" % name, hdr), name
    vp, i = C.c_void_p, C.c_int
    assert B.SIGNATURES["lsq_index_range_search_labelled"] == (i, [vp] * 7 + [i] * 6)
    assert B.SIGNATURES["lsq_index_get_label_range_info"] == (i, [vp, C.POINTER(B.LabelRangeInfo)])
    fields = [f for f, _ in B.LabelRangeInfo._fields_]
    body = re.search(r"typedef struct lsq_label_range_info \{(.*?)\} lsq_label_range_info;", hdr, re.S).group(1)
    assert fields == re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_where_routes_the_call(lsq):
    """where=None reaches lsq_index_range_search with the arguments it always had; a predicate reaches the labelled symbol with the words and the rule"""
    eng = ec.offline_engine(lsq)
    ix = ec.offline_index(lsq, eng, False)
    Q, rad, words = np.zeros((ec.NQ, ec.D), np.float32), np.ones(ec.NQ, np.float32), np.arange(ec.NQ, dtype=np.uint32)
    ix.range_search(Q, rad)
    ix.range_search(Q, rad, nprobe=3, add_coarse=True, where=(words, words), any_of=True)
    ix.range_search(Q, rad, where=(words, words))
    calls = [c for c in eng._L.calls if c[0].startswith("lsq_index_range_search")]
    assert [c[0] for c in calls] == ["lsq_index_range_search", "lsq_index_range_search_labelled", "lsq_index_range_search_labelled"]
    assert len(calls[0][1]) == 10 and calls[0][1][5:] == (ec.NQ, ec.D, 0, 0, 0)
    assert calls[1][1][5] == words.ctypes.data and calls[1][1][7:] == (ec.NQ, ec.D, 3, lsq._lib.IVF_ADD_COARSE, lsq._lib.LABEL_ANY, 0)
    assert calls[2][1][3] is None and calls[2][1][7:] == (ec.NQ, ec.D, 0, 0, 0, 0)
    with pytest.raises(ValueError):
        ix.range_search(Q, rad, any_of=True)                 # the rule without a predicate
    with pytest.raises(ValueError):
        ix.range_search(Q, rad, where=(words[:2], words))    # a mask of the wrong length never reaches the library
