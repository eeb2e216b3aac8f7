"""Labelled search without a GPU: the header's declarations, and the geometry rule the device code runs on (lsq_label_geometry: host only)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lsq_index_set_labels", "lsq_index_search_labelled", "lsq_index_search_ivf_labelled", "lsq_index_get_label_info", "lsq_label_geometry")


def _geometry(B, n, m, packed, nn, nq, flags=0, tuning=False):
    g = B.LabelGeometryInfo()
    rc = B.load(tuning=tuning).lsq_label_geometry(n, m, packed, nn, nq, flags, g)
    return rc, g.as_dict()


def test_header_and_library(lsq):
    hdr = open(os.path.join(ROOT, "include", "lsq_mi355x.h")).read()
    assert int(re.search(r"#define LSQ_VERSION (\d+)", hdr).group(1)) >= 3100
    for name in NEW:
        assert re.search(r"LSQ_API int %s\(%s" % (name, "" if name == "lsq_label_geometry" else r"lsq_index \*ix"), hdr), name
    for tuning in (False, True):
        assert lsq._lib.load(tuning=tuning).lsq_version() >= 3100


@pytest.mark.parametrize("m,packed,nn,qb", [(8, 0, 1, 4), (8, 0, 256, 4), (8, 1, 256, 4), (8, 0, 257, 4), (8, 1, 257, 2), (4, 0, 1024, 2), (16, 0, 100, 2),
                                            (16, 0, 512, 2), (16, 1, 512, 2), (8, 0, 513, 2), (8, 0, 1025, 1), (1, 0, 2048, 1), (16, 1, 2048, 1)])
def test_queries_per_block(lsq, m, packed, nn, qb):
    """QB = the largest of 4, 2, 1 with QB (m KiB of table + 8 P bytes of pool + 1 KiB of norm table when packed) <= 64 KiB, P = 2 pow2ceil(max(nn, 256))"""
    P = 2 * max(256, 1 << (nn - 1).bit_length())
    per_query = 1024 * m + 8 * P + (1024 if packed else 0)
    assert qb == max(q for q in (4, 2, 1) if q == 1 or q * per_query <= 65536)
    for tuning in (False, True):
        rc, g = _geometry(lsq._lib, 10 ** 6, m, packed, nn, 100, tuning=tuning)
        assert rc == 0 and (g["queries_per_block"], g["pool_records"], g["query_groups"]) == (qb, P, -(-100 // qb))
        assert g["lds_bytes"] == qb * (1024 * m + 8 * P) + (1024 if packed else 0) <= 65536      # what a block allocates: ONE norm table


@pytest.mark.parametrize("n", [1, 255, 256, 257, 20011, 10 ** 6, 2 ** 31 - 1])
@pytest.mark.parametrize("nq", [1, 9, 100, 10 ** 4])
def test_row_ranges(lsq, n, nq):
    """ranges of a multiple of 256 rows that cover 0 .. n - 1, none empty; about 2048 blocks while the groups are few, one range per group from 2048 groups on,
    never more than 2^28 rows to a range; the test hook: one range"""
    rc, g = _geometry(lsq._lib, n, 8, 0, 100, nq)
    per, splits, groups = g["rows_per_block"], g["blocks_per_query"], g["query_groups"]
    assert rc == 0 and per % 256 == 0 and per <= 2 ** 28 and (splits - 1) * per < n <= splits * per
    steps = -(-n // 256)
    assert splits == -(-steps // -(-steps // min(max(-(-2048 // groups), -(-n // 2 ** 28)), steps, 65535)))
    rc, g = _geometry(lsq._lib, n, 8, 0, 100, nq, flags=lsq._lib.LABEL_TEST_ONE_SPLIT)
    assert rc == 0 and g["blocks_per_query"] == 1 and g["rows_per_block"] == steps * 256


def test_geometry_refusals(lsq):
    B = lsq._lib
    for args in ((0, 8, 0, 100, 1), (100, 0, 0, 100, 1), (100, 17, 0, 100, 1), (100, 8, 0, 0, 1), (100, 8, 0, 2049, 1), (100, 8, 0, 100, 0)):
        assert _geometry(B, *args)[0] == B.LSQ_EINVAL, args
    assert _geometry(B, 100, 8, 0, 100, 1, flags=4)[0] == B.LSQ_EINVAL
    assert B.load().lsq_label_geometry(100, 8, 0, 100, 1, 0, None) == B.LSQ_EINVAL
