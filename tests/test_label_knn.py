"""Labelled exact k-NN without a GPU: the header's declarations, the geometry rule the launch runs on (lsq_label_knn_geometry: host only), and the binding's
routing of Index.knn."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QB = {1: 8, 100: 8, 256: 8, 257: 4, 512: 4, 513: 2, 1024: 2, 1025: 1, 2048: 1}


def _geometry(B, n, d, nn, nq, flags=0, tuning=False):
    g = B.LabelGeometryInfo()
    rc = B.load(tuning=tuning).lsq_label_knn_geometry(n, d, nn, nq, flags, g)
    return rc, g.as_dict()


def test_header_and_library(lsq):
    hdr = open(os.path.join(ROOT, "include", "lsq_mi355x.h")).read()
    assert int(re.search(r"#define LSQ_VERSION (\d+)", hdr).group(1)) >= 3200
    for name in ("lsq_index_knn_labelled", "lsq_index_get_label_knn_info"):
        assert re.search(r"LSQ_API int %s\(lsq_index \*ix" % name, hdr), name
    assert re.search(r"LSQ_API int lsq_label_knn_geometry\(", hdr)
    for tuning in (False, True):
        assert lsq._lib.load(tuning=tuning).lsq_version() >= 3200


@pytest.mark.parametrize("nn", sorted(QB))
def test_queries_per_block(lsq, nn):
    """QB = 4096 / P, P = 2 pow2ceil(max(nn, 256)): the pools take 32 KiB at every nn, the block stays under 64 KiB"""
    P = 2 * max(256, 1 << (nn - 1).bit_length())
    for tuning in (False, True):
        rc, g = _geometry(lsq._lib, 5003, 19, nn, 13, tuning=tuning)
        assert rc == 0 and (g["queries_per_block"], g["pool_records"], g["query_groups"]) == (QB[nn], P, -(-13 // QB[nn])) and QB[nn] * P == 4096
        assert 32768 + 16 * 256 * 4 < g["lds_bytes"] <= 65536


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5003, 10 ** 6, 2 ** 31 - 1])
@pytest.mark.parametrize("nq,nn", [(1, 100), (13, 2048), (10 ** 4, 100), (10 ** 4, 1000)])
def test_row_ranges(lsq, n, nq, nn):
    """ranges of a multiple of 256 rows that cover 0 .. n - 1, none empty, by the labelled scan's rule over the groups of QB queries; the test hook: one range"""
    rc, g = _geometry(lsq._lib, n, 128, nn, nq)
    per, splits, groups = g["rows_per_block"], g["blocks_per_query"], g["query_groups"]
    assert rc == 0 and per % 256 == 0 and per <= 2 ** 28 and (splits - 1) * per < n <= splits * per
    steps = -(-n // 256)
    assert splits == -(-steps // -(-steps // min(max(-(-2048 // groups), -(-n // 2 ** 28)), steps, 65535)))
    rc, g = _geometry(lsq._lib, n, 128, nn, nq, flags=lsq._lib.LABEL_TEST_ONE_SPLIT)
    assert rc == 0 and g["blocks_per_query"] == 1 and g["rows_per_block"] == steps * 256


def test_geometry_refusals(lsq):
    B = lsq._lib
    for args in ((0, 8, 100, 1), (100, 0, 100, 1), (100, 8, 0, 1), (100, 8, 2049, 1), (100, 8, 100, 0)):
        assert _geometry(B, *args)[0] == B.LSQ_EINVAL, args
    assert _geometry(B, 100, 8, 100, 1, flags=4)[0] == B.LSQ_EINVAL
    assert B.load().lsq_label_knn_geometry(100, 8, 100, 1, 0, None) == B.LSQ_EINVAL


def test_where_routes_the_call(lsq):
    """where=None reaches lsq_index_knn with the arguments it always had; a predicate reaches lsq_index_knn_labelled with the words and the flags"""
    E = importlib_engine(lsq)
    calls = []

    class Eng:
        def _call(self, side, sym, *args, h=None):
            calls.append((sym, args))

    ix = object.__new__(E.Index)
    ix._eng, ix._dev, ix._h, ix.d = Eng(), False, None, 4
    Q, words = np.zeros((3, 4), np.float32), np.arange(3, dtype=np.uint32)
    ix.knn(Q, 2, id_base=1)
    ix.knn(Q, 2, where=(words, words), any_of=True, flags=lsq._lib.LABEL_TEST_ONE_SPLIT)
    assert [c[0] for c in calls] == ["lsq_index_knn", "lsq_index_knn_labelled"]
    assert calls[0][1][3:] == (0, 3, 4, 2, 1, 0) and len(calls[0][1]) == 9
    assert calls[1][1][3] == 0 and calls[1][1][6:] == (3, 4, 2, 0, lsq._lib.LABEL_ANY | lsq._lib.LABEL_TEST_ONE_SPLIT, 0)
    with pytest.raises(ValueError):
        ix.knn(Q, 2, where=(words[:2], words))          # a mask of the wrong length never reaches the library


def importlib_engine(lsq):
    import importlib
    return importlib.import_module(lsq.__name__ + ".engine")
