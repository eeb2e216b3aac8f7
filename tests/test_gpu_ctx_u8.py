"""Every ordered pair of the 8-bit encode entry points, their f32 counterparts and the option moves on ONE long-lived context (the alphabet of
tests/ctx_ops_u8.py, the driver of tests/ctx_ops.py): each step must equal, bit for bit and counter for counter, the same entry and variant on a fresh
Engine with the same options, and the fresh result its oracle."""
import os
import re
import sys
import time

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctx_ops as ops  # noqa: E402
import ctx_ops_u8 as u8  # noqa: E402

WALK_SEED = 20261017


def test_every_8bit_context_symbol_is_walked():
    """CPU: the header's entry points that take a context and 8-bit data are exactly the symbols this alphabet walks"""
    with open(os.path.join(ops.ROOT, "include", "lsq_mi355x.h")) as f:
        hdr = f.read()
    declared = set(re.findall(r"\b(lsq_\w+)\s*\(\s*struct\s+lsq_ctx\s*\*", hdr))
    walked = {s for o in u8.u8_ops() for s in o.symbols}
    assert declared == walked == set(u8.U8_SYMBOLS), (declared, walked)
    names = [o.name for o in u8.alphabet()]
    assert len(names) == len(set(names)) == 8
    for o in u8.u8_ops():
        assert o.encode and max(s[0] for s in o.shapes) >= 65536      # one variant passes q16_min on default options


@pytest.fixture(scope="module")
def walk(lsq, oracle):
    w = ops.Walk(ops=u8.alphabet(), seed=WALK_SEED)
    yield w
    w.close()


@pytest.mark.gpu
def test_8bit_entries_are_reproducible_on_two_fresh_contexts(walk):
    for o in u8.u8_ops():
        for v in range(len(o.shapes)):
            walk.determinism(o.name, v)
    assert walk.demoted == {}, "not bit-reproducible on two fresh contexts: %r" % walk.demoted


@pytest.mark.gpu
def test_every_ordered_pair_on_one_context(walk):
    names = list(walk.ops)
    k = len(names)
    circuit = [names[i] for i in ops.eulerian_circuit(k, WALK_SEED)]
    assert len(circuit) == k * k + 1
    t = time.time()
    walk.open()
    try:
        bad = walk.run(circuit)
    finally:
        walk.close()
    print("8-bit pair walk: k = %d entries, %d steps, %d fresh contexts so far, %.1f s" % (k, walk.index, walk.fresh_runs, time.time() - t))
    assert bad == [], bad[0][4]
