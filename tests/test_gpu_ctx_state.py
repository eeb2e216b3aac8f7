"""The layer between the kernels: `lsq_ctx` is one mutable object that every device entry point shares (work buffers with several owners, flags one call
sets and another consumes, the bound stream, a dozen options).  Here ONE long-lived Engine visits every ordered pair of the alphabet of tests/ctx_ops.py
-- the entry points, host-buffer and _dev forms apart, and the moves that change only the state -- along a seeded Eulerian circuit, and every step must
equal, bit for bit and counter for counter, the same entry and variant on a FRESH Engine that carries the option profile the driver believes is active.
The fresh result itself is held to the entry point's existing checker, so the baseline is never the code agreeing with itself.

Then the sequences that pairs alone do not reach, and the proof that the walk can fail: seven one-slip copies of lsq_api.hip (tests/ctx_mutants.py), each
loaded in a child process of its own, each of which the walk must report at the pair the slip breaks.

Concurrency is out of scope: the header allows one host thread per context and asks the caller to await the old stream before lsq_set_stream binds
another; the driver synchronises before every switch."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctx_mutants  # noqa: E402
import ctx_ops as ops  # noqa: E402

pytestmark = pytest.mark.gpu
H = 256
ROOT = ops.ROOT
WALK_SEED = 20261016


@pytest.fixture(scope="module")
def walk(lsq, oracle):
    w = ops.Walk(seed=WALK_SEED)
    yield w
    w.close()


def _entries(w):
    return [o for o in w.ops.values() if o.kind == "op"]


def test_every_entry_is_reproducible_on_two_fresh_contexts(walk):
    """Determinism first: an entry that is not bit-reproducible on two fresh contexts cannot be held to equality in the walk (it is then held to its checker
    there, and reported here).  None is expected: fixed-order sums, no atomics in any solver, the scan's candidates sorted before they leave."""
    t = time.time()
    for o in _entries(walk):
        for v in range(len(o.shapes)):
            walk.determinism(o.name, v)
    print("determinism: %d entries x 3 variants on two fresh contexts each in %.1f s; not reproducible: %r" % (len(_entries(walk)), time.time() - t, walk.demoted))
    assert walk.demoted == {}, "not bit-reproducible on two fresh contexts (held to their checkers in the walk): %r" % walk.demoted


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
    print("pair walk: k = %d entries, %d steps, %d fresh contexts so far, %.1f s" % (k, walk.index, walk.fresh_runs, time.time() - t))
    assert bad == [], bad[0][4]


# ---- the sequences pairs do not reach ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [2, 3])
def test_consecutive_nonblocking_encodes_fold_the_sum_of_their_counters(walk, count):
    import torch
    op, dev = walk.ops["encode_icm_dev_nb"], walk.ops["encode_icm_dev"]
    order = [1, 0, 2][:count]                                                  # the 70 001-vector variant first: the filtered walk leaves counters on the device
    with walk.lsq.Engine(0) as eng:
        t0 = eng.timings()
        outs = []
        for v in order:
            outs.append(tuple(np.asarray(o) for o in op._call(eng, walk.inputs_for(op.name, v))))      # no timings() in between: nothing folds
        torch.cuda.synchronize()
        t1 = eng.timings()
        got = np.array([t1[c] - t0[c] for c in ops.COUNTERS], dtype=np.int64)
        want = sum(walk.baseline(op.name, v)[-1] for v in order)
        assert np.array_equal(got, want), "folded counters %r, the sum of the fresh calls' %r (%r)" % (got, want, ops.COUNTERS)
        assert want[ops.COUNTERS.index("filtered_blocks")] > 0
        for v, out in zip(order, outs):
            assert ops.first_difference(out, walk.baseline(op.name, v)[:-1]) is None, "nonblocking call on variant %d" % v
        diff = ops.first_difference(dev.run(eng, walk.inputs_for(dev.name, 1)), walk.baseline(dev.name, 1))
        assert diff is None, "blocking encode after %d nonblocking ones: %s" % (count, diff)


def test_no_entry_moves_the_ils_counter(walk, oracle):
    """encoding_icm with it = None three times, one of every other kind of entry between the calls: the oracle's chain at it = 0, 1, 2."""
    inp = walk.inputs_for("encoding_icm_auto", 2)
    n, d, m = inp["shape"]
    others = [nm for nm, o in walk.ops.items() if not o.auto]
    walk.open()
    try:
        B, Bref = inp["B0"], inp["B0"]
        for it in range(3):
            B = walk.eng.encoding_icm(inp["X"], B, inp["K"], m, inp["J"], True, inp["npert"], seed=inp["seed"])
            Bref = oracle.encoding_icm_faithful(inp["X"], Bref, inp["K"], m, H, inp["J"], True, inp["npert"], inp["seed"], it)
            assert np.array_equal(B, Bref), "call %d of the chain differs from the oracle's iteration %d" % (it + 1, it)
            if it < 2:
                bad = walk.run(others + ["opt:default"])
                assert bad == [], bad[0][4]
    finally:
        walk.close()


class Injecting:
    """an Engine that runs one catalogue entry on the same context before each of its method calls"""

    def __init__(self, walk, names):
        self._walk, self._names, self._at, self.injected = walk, names, 0, 0

    def __getattr__(self, attr):
        v = getattr(self._walk.eng, attr)
        if not callable(v) or attr.startswith("_") or attr in ("close", "timings", "set_option"):
            return v

        def call(*a, **k):
            bad = self._walk.run([self._names[self._at % len(self._names)]])
            assert bad == [], "injected before %s: %s" % (attr, bad[0][4])
            self._at += 1
            self.injected += 1
            return v(*a, **k)
        return call


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("trainer", ["train_lsq", "train_chainq", "train_pq"])
def test_trainers_with_a_foreign_call_before_every_step(walk, trainer):
    """The host trainers interleaved with foreign calls on the same context return what they return alone (same seeds)."""
    lsq = walk.lsq
    rng = np.random.default_rng(8)
    d, n, m = 16, 4000, 4
    X = (rng.standard_normal((d, n)) * np.linspace(3, 0.5, d)[:, None]).astype(np.float32)
    B0 = rng.integers(1, H + 1, (m, n)).astype(np.int16)
    R = np.eye(d, dtype=np.float32)

    def train(engine):
        if trainer == "train_lsq":
            return lsq.train_lsq(X, m, H, R, B0, None, 2, 2, 3, True, 3, False, seed=5, engine=engine, device_update=True)
        if trainer == "train_chainq":
            return lsq.train_chainq(X, m, H, R, B0, None, 2, False, engine=engine, device_update=True)
        return lsq.train_pq(X, m, H, False, seed=5, engine=engine)

    with lsq.Engine(0) as alone:
        want = train(alone)
    foreign = [nm for nm, o in walk.ops.items() if o.kind == "op" and not o.auto]
    walk.open()
    try:
        inj = Injecting(walk, foreign)
        got = train(inj)
    finally:
        walk.close()
    assert inj.injected >= 4, inj.injected
    assert _same(got, want), "%s interleaved with %d foreign calls differs from the run alone" % (trainer, inj.injected)


@pytest.mark.parametrize("order", ["short_then_600", "600_other_m_short"])
def test_short_and_600_iteration_encodes_in_the_other_orders(lsq, oracle, order):
    """tests/test_gpu_depth.py runs a short call after a 600-iteration one (the counters outgrow the per-call block for good); here the reverse order, and
    the pair with a call of another m between the two."""
    from conftest import make_problem
    d, n, m, J, npert, seed = 16, 300, 4, 2, 2, 9
    X, K, B0 = make_problem(d, n, m, seed=21, kind="gauss")
    X7, K7, B7 = make_problem(24, 500, 7, seed=22, kind="gauss")
    calls = {"short_then_600": [("a", [3]), ("a", [600]), ("a", [3])], "600_other_m_short": [("a", [600]), ("b", [2]), ("a", [3])]}[order]
    with lsq.Engine(0) as eng:
        for which, ils in calls:
            x, k, b, mm = (X, K, B0, m) if which == "a" else (X7, K7, B7, 7)
            ref, objs_ref = oracle.encode_icm(x, b, k, mm, H, ils, J, npert, True, seed)
            t0 = eng.timings()
            Bs, objs = eng.encode_icm(x, b, k, mm, ils, J, npert, True, seed=seed)
            t1 = eng.timings()
            assert np.array_equal(Bs, ref), "%s, ils = %s: %d codes differ" % (order, ils, (Bs != ref).sum())
            assert np.allclose(objs, objs_ref, rtol=1e-5, atol=0)
            with lsq.Engine(0) as fresh:
                f0 = fresh.timings()
                fresh.encode_icm(x, b, k, mm, ils, J, npert, True, seed=seed)
                f1 = fresh.timings()
            assert [t1[c] - t0[c] for c in ops.COUNTERS] == [f1[c] - f0[c] for c in ops.COUNTERS], (order, ils)


def test_panel_upload_pipeline_then_the_one_piece_upload_on_one_context(walk):
    """A host-buffer encode through the panel upload pipeline, then the same call with the pipeline off on the same context: both equal the oracle (the
    baseline's check) and the fresh context's counters.  (The level parameters the pipeline leaves behind are held to their bound by
    tests/test_gpu_q16_bound.py, case host_sample, through lsq_get_q16_snapshot.)"""
    op = walk.ops["encode_icm"]
    inp = walk.inputs_for(op.name, 1)
    n, d, m = inp["shape"]

    def options(eng, min_bytes):
        eng.set_option("upload_pipeline_min_bytes", min_bytes)
        eng.set_option("upload_panel_bytes", 4 * d * 128 * 37)                    # 37 tiles per panel: several panels, the last one ragged

    want = {}
    for min_bytes in (1, 0):
        with walk.lsq.Engine(0) as fresh:
            options(fresh, min_bytes)
            want[min_bytes] = op.run(fresh, inp)
        op.check(inp, want[min_bytes])
    assert ops.first_difference(want[1][:-1], want[0][:-1]) is None                # the same codes and objectives on both roads
    with walk.lsq.Engine(0) as eng:
        for min_bytes in (1, 0, 1):
            options(eng, min_bytes)
            diff = ops.first_difference(op.run(eng, inp), want[min_bytes])
            assert diff is None, "upload_pipeline_min_bytes = %d: %s" % (min_bytes, diff)


# ---- the proof that the walk can fail ---------------------------------------------------------------------------------------------------------------------

def _child(lib_path, timeout=600):
    env = dict(os.environ, LSQ_LIB_PATH=lib_path)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ctx_ops.py"), "--mutant-sequence"], env=env, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("CTX_MUTANT_RESULT ")]
    if p.returncode != 0 or len(lines) != 1:
        pytest.fail("the child on %s ended abnormally (exit status %d); nothing is retried\n%s" % (lib_path, p.returncode, (p.stdout + p.stderr)[-3000:]), pytrace=False)
    return json.loads(lines[0][len("CTX_MUTANT_RESULT "):])


def test_every_mutant_is_reported_at_its_pair(lsq):
    """Each one-slip copy of lsq_api.hip in a child process of its own, one after another, each once; the shipped library passes the same sequence."""
    shipped = _child(lsq._lib.LIB_PATH)
    assert shipped["mismatches"] == [], "the shipped library on the mutant sequence: %r" % (shipped["mismatches"][0],)
    mdir = os.path.join(os.path.dirname(lsq._lib.LIB_PATH), "csrc", "build", "mutants")
    report = []
    for name, _, _, profile, pair in ctx_mutants.MUTANTS:
        path = os.path.join(mdir, "liblsq_%s.so" % name)
        assert os.path.exists(path), "%s is not built (make -C local-search-quantization_amd/csrc)" % path
        res = _child(path)
        assert res["steps"] == shipped["steps"]
        hits = [(p, c, prof) for _, p, c, prof, _ in res["mismatches"]]
        report.append((name, len(hits), (pair[0], pair[1], profile) in hits))
        assert (pair[0], pair[1], profile) in hits, "mutant %s is not reported at %s -> %s under %s; reported: %r" % (name, pair[0], pair[1], profile, hits[:8])
    print("mutants (name, mismatching steps, reported at its pair): %r" % report)
