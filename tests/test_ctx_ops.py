"""The driver of the context walk (tests/ctx_ops.py, tests/ctx_mutants.py) without a GPU: the circuit covers every ordered pair and the variants rotate,
no context symbol can be added to the library without joining the walk, and every mutant is one unambiguous replacement."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctx_mutants  # noqa: E402
import ctx_ops as ops  # noqa: E402

API = os.path.join(ops.ROOT, "local-search-quantization_amd", "csrc", "lsq_api.hip")


@pytest.mark.parametrize("k,seed", [(1, 0), (2, 1), (5, 2), (len(ops.alphabet()), 20261016), (len(ops.alphabet()), 7)])
def test_circuit_visits_every_ordered_pair_once(k, seed):
    c = ops.eulerian_circuit(k, seed)
    assert len(c) == k * k + 1 and c[0] == c[-1] and set(c) == set(range(k))
    pairs = list(zip(c, c[1:]))
    assert len(set(pairs)) == k * k == len(pairs)                              # all k^2 ordered pairs, self-pairs included, each exactly once
    assert ops.eulerian_circuit(k, seed) == c                                  # seeded
    if k > 2:
        assert ops.eulerian_circuit(k, seed + 1) != c


def test_variants_rotate_and_differ_in_every_dimension():
    al = {o.name: o for o in ops.alphabet()}
    names = list(al)
    circuit = [names[i] for i in ops.eulerian_circuit(len(names), 3)]
    seen = {}
    for name, v in ops.plan(circuit, al):
        if al[name].kind == "move":
            assert v is None
            continue
        assert v == len(seen.setdefault(name, [])) % 3                          # the entry's next variant, in rotation
        seen[name].append(v)
    for name, o in al.items():
        if o.kind == "op":
            assert len(seen[name]) >= len(names) and set(seen[name]) == {0, 1, 2}
            for axis in range(3):                                              # n, d and m all change between an entry's visits
                assert len({s[axis] for s in o.shapes}) == 3, (name, o.shapes)
            if o.encode:
                assert max(s[0] for s in o.shapes) >= 65536, name              # one variant passes q16_min on default options


def test_every_context_symbol_is_walked_or_excluded_with_a_reason(lsq):
    sig = lsq._lib.SIGNATURES
    ctx = ops.context_symbols()
    assert len(ctx) >= 40 and set(ctx) <= set(sig), sorted(set(ctx) - set(sig))
    assert {"lsq_create", "lsq_destroy", "lsq_encode_icm", "lsq_kmeanspp_seed_dev", "lsq_set_option"} <= set(ctx)
    walked = {s for o in ops.alphabet() for s in o.symbols}
    assert walked <= set(ctx), sorted(walked - set(ctx))
    for s in ctx:
        assert (s in walked) != (s in ops.EXCLUDED), "%s must be in the catalogue or (with a reason) in EXCLUDED, and not in both" % s
    assert set(ops.EXCLUDED) <= set(ctx) and all(len(r) > 10 for r in ops.EXCLUDED.values())
    # the exclusions are the constructor, the destructor and the getters -- nothing that computes
    assert all(s in ("lsq_create", "lsq_destroy") or s.startswith("lsq_get_") for s in ops.EXCLUDED)
    assert not any(s.startswith("lsq_get_") and s not in ("lsq_get_unaries", "lsq_get_binaries") for s in walked)


def test_rejected_calls_cover_every_entry_point(lsq):
    sig = lsq._lib.SIGNATURES
    calls = ops.rejected_calls()
    entry_symbols = {s for o in ops.catalogue() for s in o.symbols} - {"lsq_synchronize"}      # (lsq_synchronize has nothing to reject but a null context)
    assert {c[0] for c in calls} == entry_symbols
    for sym, what, args in calls:
        types = sig[sym][1][1:]
        assert len(args) == len(types)
        names = ops.ARG_NAMES[sym].split()
        for a, ty, name in zip(args, types, names):
            if a is None:
                continue                                                       # a null pointer
            assert isinstance(a, (int, float)) and name[0].islower() or name in ("S",), (sym, name, a)
        if what == "m = 17":
            assert 17 in args or 8 * 17 in args, (sym, args)
        if what == "h = 128":
            assert args[names.index("h")] == 128 and args[names.index("m")] == 8


def test_every_mutant_is_one_unambiguous_stale_value_slip():
    with open(API) as f:
        src = f.read()
    fixed = {o.name for o in ops.catalogue(fixed=True)} | {"opt:" + p for p in ops.MUTANT_PHASES}
    seq = ops.mutant_sequence()
    pairs = set()
    prof = None
    for a, b in zip(seq, seq[1:]):
        prof = a[4:] if a.startswith("opt:") else prof
        pairs.add((a, b, prof))
    assert len(ctx_mutants.MUTANTS) >= 5 and len(set(ctx_mutants.NAMES)) == len(ctx_mutants.NAMES)
    for name, old, new, profile, pair in ctx_mutants.MUTANTS:
        assert src.count(old) == 1, name
        out = ctx_mutants.mutate(src, name)
        assert out != src and out.count("\n") <= src.count("\n")
        # a slip removes or changes an assignment of a flag / counter: no allocation, size, bound, pointer or launch is named in what it touches
        touched = old.replace(new, "") if new in old else old + new
        touched = touched.replace("LSQ_TRY(c->sci.ensure(sizeof(float) * (size_t)m * LSQ_H));", "")      # (context of one replacement: in `old` and `new` alike)
        for word in ("ensure", "hipMalloc", "hipMemcpy", "hipMemset", "launch", "<<<", "sizeof"):
            assert word not in touched, (name, word)
        assert not re.search(r"(->|\.)p\b", touched), name                     # no DevBuf pointer
        assert set(pair) <= fixed and (pair[0], pair[1], profile) in pairs, (name, pair, profile)
    assert len({o.shapes[0] for o in ops.catalogue(fixed=True)}) == 1 and all(len(set(o.shapes)) == 1 for o in ops.catalogue(fixed=True))


def test_first_difference_names_the_element():
    a = (np.arange(6, dtype=np.float32).reshape(2, 3), np.zeros(len(ops.COUNTERS), dtype=np.int64))
    b = (a[0].copy(), a[1].copy())
    assert ops.first_difference(a, b) is None
    b[0][1, 2] = 9
    assert "(1, 2)" in ops.first_difference(a, b) and "output 0" in ops.first_difference(a, b)
    b[0][1, 2] = 5
    b[1][4] = 3
    assert "filtered_blocks" in ops.first_difference(a, b)
    n1, n2 = (np.array([np.nan, 1.0]),), (np.array([np.nan, 1.0]),)
    assert ops.first_difference(n1, n2) is None                                # NaN equals NaN at the same position
    assert ops.first_difference((np.array([np.nan, 1.0]),), (np.array([1.0, np.nan]),)) is not None
    err = (np.array([(-1,)], dtype=ops.ERR), a[1])
    assert ops.is_error(err) and ops.first_difference(err, err) is None and ops.first_difference(err, a) is not None
