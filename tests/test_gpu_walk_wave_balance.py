"""The filtered walk hands a node update's items (16 vectors x one slice at m <= 8, 32 vectors above) to its 16 waves round-robin, and inside a slice
step each wave sets its own scheduling priority from how far along its items it is.  Priority changes WHEN an item is served, never
which wave owns it or what it computes -- integer level sums, per-vector ds_min keys -- so a result can only change if a wave skips or repeats an
item.  The cases are therefore the sizes at which the item counts of the waves differ: n = 1 (one wave with one item, fifteen with none), 15 and
17 (a last item with fewer than 16 vectors; at m <= 8 a second wave with a single vector), 255 / 257 (every wave one item, the last one short /
wave 0 a second item of one vector), 4095 (a block just under a full pass: 15 or 16 items per wave at m <= 8, two passes at m = 16).  m = 3, 8, 16:
one table group, two groups with the short second one, and the 16-candidate slices of m > 8.  The filter is forced onto every block (no light
blocks, no probe, no hand-over to the f32 walk), with the memoisation (`skip`) on and off; every code against the oracle bit for bit, the
objective to 1e-6, and a second call on the same context must return the same bytes."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
H = 256
D, ILS, J, NPERT, SEED = 16, [2], 4, 2, 17


@functools.lru_cache(maxsize=None)
def _case(m, n):
    """inputs and the oracle's answer, computed once per (m, n) and shared by the skip-on / skip-off cases (read-only)"""
    import oracle as O
    from conftest import make_problem
    O.build()
    X, K, B0 = make_problem(D, n, m, seed=300 + m, kind="gauss")
    ref, objs_ref = O.encode_icm(X, B0, K, m, H, ILS, J, NPERT, True, SEED)
    for a in (X, K, B0, ref, objs_ref):
        a.setflags(write=False)
    return X, K, B0, ref, objs_ref


@pytest.mark.parametrize("skip", [1, 0], ids=["skip", "noskip"])
@pytest.mark.parametrize("n", [1, 15, 17, 255, 257, 4095])
@pytest.mark.parametrize("m", [3, 8, 16])
def test_every_wave_item_count_through_the_filtered_walk(lsq, m, n, skip):
    X, K, B0, ref, objs_ref = _case(m, n)
    with lsq.Engine(0) as eng:
        for k, v in (("q16_min", 0), ("light", 0), ("filter_probe_div", 0), ("filter_fallback_div", 0), ("skip", skip)):
            eng.set_option(k, v)
        Bs, objs = eng.encode_icm(X, B0, K, m, ILS, J, NPERT, True, seed=SEED)
        tm = eng.timings()
        Bs2, objs2 = eng.encode_icm(X, B0, K, m, ILS, J, NPERT, True, seed=SEED)
    rel = float(np.max(np.abs(objs.astype(np.float64) - objs_ref) / np.abs(objs_ref)))
    print("m %d n %d skip %d: %d codes differ, objective rel. diff %.3g, filtered_blocks %d light_blocks %d fallback chunks %d" %
          (m, n, skip, int((Bs != ref).sum()), rel, tm["filtered_blocks"], tm["light_blocks"], tm["filter_fallback_chunks"]))
    assert tm["filtered_blocks"] > 0 and tm["light_blocks"] == 0 and tm["filter_fallback_chunks"] == 0, tm      # the kernel under test produced every code
    assert np.array_equal(Bs, ref), "%d codes differ from the oracle" % (Bs != ref).sum()
    assert np.allclose(objs, objs_ref, rtol=1e-6, atol=0), (objs, objs_ref)
    assert Bs.tobytes() == Bs2.tobytes() and objs.tobytes() == objs2.tobytes(), "two calls on one context differ"
