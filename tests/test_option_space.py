"""The covering-array generator of tests/option_space.py (no GPU): the array the GPU test is parametrised over really covers every pair of option
values, stays small, and is the same on every run and every machine."""
from collections import OrderedDict
from itertools import combinations

import pytest

import option_space as S


def test_every_pair_of_values_is_in_some_row_or_excluded():
    rows = S.covering_array()
    seen = set()
    for r in rows:
        assert list(r) == list(S.FACTORS) and all(r[f] in S.FACTORS[f] for f in r), r
        seen |= S.row_pairs(r)
    excluded = {S._norm(p) for p in S.EXCLUSIONS}
    want = 0
    for fa, fb in combinations(S.FACTORS, 2):                 # counted here, independently of all_pairs()
        for va in S.FACTORS[fa]:
            for vb in S.FACTORS[fb]:
                want += 1
                p = S._norm(((fa, va), (fb, vb)))
                assert (p in seen) != (p in excluded), "pair %r: in a row %s, excluded %s" % (p, p in seen, p in excluded)
    assert want == len(S.all_pairs()) + len(excluded) == 525


def test_the_array_is_small():
    rows = S.covering_array()
    biggest = max(len(a) * len(b) for a, b in combinations(S.FACTORS.values(), 2))
    assert biggest == 20 <= len(rows) <= S.MAX_ROWS == 60, len(rows)      # no pairwise array is smaller than the two largest factors' product
    assert len({S.row_id(r) for r in rows}) == len(rows)                  # no row twice, ids unique


def test_the_array_is_reproducible():
    a, b = S.covering_array(), S.covering_array()
    assert a == b and [S.row_id(r) for r in a] == [S.row_id(r) for r in b]
    assert a[0] == OrderedDict((f, v[0]) for f, v in S.FACTORS.items())   # row 0: what a caller gets without setting anything
    shuffled = OrderedDict((f, S.FACTORS[f]) for f in S.FACTORS)          # an equal table built afresh gives the same array (no dependence on identity / hashing)
    assert S.covering_array(shuffled) == a


def test_the_exclusion_list_is_the_documented_one():
    """lsq_set_option rejects no combination of the table's values (each key is range-checked on its own): the list is empty, and the table's defaults are the
    library's (csrc/lsq_api.hip, lsq_ctx; README "Options and tuning knobs")."""
    assert S.EXCLUSIONS == ()
    assert [v[0] for v in S.FACTORS.values()] == [6, 1, 1, -1, 64, 65536, "default", 0, 8, 64, 0, "host_f32"]
    assert {f: len(v) for f, v in S.FACTORS.items()} == {"schedule": 3, "skip": 2, "fallback": 2, "light": 4, "wave_max": 3, "q16_min": 3, "chunk": 2,
                                                        "per_node": 2, "filter_probe_div": 3, "filter_fallback_div": 3, "profile": 2, "entry": 5}


def test_the_generator_honours_an_exclusion_list():
    factors = OrderedDict([("a", (0, 1, 2)), ("b", ("x", "y")), ("c", (False, True)), ("d", (7, 8, 9))])
    excl = ((("a", 2), ("b", "y")), (("d", 9), ("c", True)))
    rows = S.covering_array(factors, excl)
    seen = set().union(*(S.row_pairs(r) for r in rows))
    assert not seen & {S._norm(p) for p in excl}
    assert seen == S.all_pairs(factors, excl) and len(S.all_pairs(factors, excl)) == 37 - 2
    assert rows == S.covering_array(factors, excl)
    with pytest.raises(ValueError):                            # a factor none of whose values may stand next to the seed pair
        S.covering_array(OrderedDict([("a", (0,)), ("b", (0, 1)), ("c", (0,))]), ((("a", 0), ("c", 0)),))


def test_resolve_and_the_road_predicates():
    n = 256 * 280
    row = OrderedDict((f, v[0]) for f, v in S.FACTORS.items())
    opts, entry = S.resolve(row, n)
    assert entry == "host_f32" and opts["chunk"] == 256 * 3968 and opts["q16_min"] == 65536 and "entry" not in opts
    assert S.takes_filtered_walk(row, n) and not S.takes_wave_kernel(row, n, 280)
    third = OrderedDict(row, chunk="third")
    assert S.resolve(third, n)[0]["chunk"] == n // 3 + 1 and not S.takes_filtered_walk(third, n)      # chunks of 23 894 < q16_min: the f32 walk
    assert S.takes_filtered_walk(OrderedDict(third, q16_min=0), n)
    assert not S.takes_filtered_walk(OrderedDict(row, q16_min="above_n"), n) and S.resolve(OrderedDict(row, q16_min="above_n"), n)[0]["q16_min"] == n + 1
    assert not S.takes_wave_kernel(third, n, 94)                                                       # 94 vectors per block > wave_max = 64
    assert S.takes_wave_kernel(OrderedDict(third, wave_max=280), n, 94)                                # light = -1 stands for 256
    assert not S.takes_wave_kernel(OrderedDict(third, wave_max=280, light=64), n, 94)
    assert not S.takes_wave_kernel(OrderedDict(third, wave_max=280, schedule=3), n, 94)
    s4 = OrderedDict(row, schedule=4, wave_max=280)
    assert not S.takes_wave_kernel(s4, n, 280) and S.takes_wave_kernel(OrderedDict(s4, light=280), n, 280)
