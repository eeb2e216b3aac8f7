"""The float64 ILS / ICM replay of tests/icm_replay.py on the CPU.

  * Its own checks: the node values' decomposition equals the direct ||x - sum c||^2 up to a constant in the candidate; the bounds hold for
    the values evaluated in f32 the way the walk evaluates them (fmaf-chain tables, f32 adds in ascending k) and in the reverse order; in
    the exact regime every bound is 0 and every f32 value equals the float64 one.  Its RNG restatement draws the oracle's words.
  * It judges the CPU oracle (oracle/lsq_oracle.c), pinning it against an independent float64 definition without a GPU: bit for bit in the
    exact regime (the lowest index among exact ties, strict-< rejection of equal costs, the ==/< counters), zero wrong decisions and at least
    90 % verified vector-iterations in the bounded one.
  * It accepts the golden fixtures' stored codes.
  * Sensitivity: scratch builds of the oracle, each with one slip, must each fail it.
"""
import ctypes as C
import glob
import importlib
import os
import subprocess

import numpy as np
import pytest

import icm_replay as IR
from conftest import ROOT, make_problem

H = 256


@pytest.fixture(scope="module")
def node_order():
    return importlib.import_module("local-search-quantization_amd").node_order


def _problem(kind, n, d, m, seed):
    if kind == "exact":
        return IR.exact_problem(n, d, m, seed)
    return make_problem(d, n, m, seed=seed, kind=kind)


def judge(node_order, X, K, B0, m, outs, J, npert, randord, seed, stats=None):
    """outs: per ILS iteration the codes (n, m) 1-based, or None -> Report"""
    orders = [node_order(seed, it, m, randord) for it in range(len(outs))]
    outs0 = [None if o is None else np.asarray(o, np.int64) - 1 for o in outs]
    return IR.replay(IR.Case(X, K, m), np.asarray(B0, np.int64) - 1, outs0, lambda c, it: IR.perturb(c, npert, seed, it), orders, J, npert, stats)


# ---- the replay's own checks ---------------------------------------------------------------------------------------------------------

def test_rng_restatement_draws_the_builds_words(oracle):
    for ctr, key in (([0, 0, 0, 0], [0, 0]), ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2), ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0])):
        got = IR.philox4x32_10(*[np.array([c], np.uint64) for c in ctr], *key)
        assert [int(g[0]) for g in got] == oracle.philox4x32_10(ctr, key).tolist()
    idx = np.arange(5, 900, 7) + (1 << 33)
    for w in (0, 3, 17, 31):
        assert IR.rng_word(0x123456789, idx, 4, 1, w).tolist() == [oracle.rng_word(0x123456789, int(i), 4, 1, w) for i in idx]
    codes = np.random.default_rng(0).integers(0, H, (200, 16))
    for m in (1, 3, 8, 16):
        for npert in (0, 1, 4, m):
            got = IR.perturb(codes[:, :m], npert, 77, 3, global_offset=1000)
            ref = np.stack([oracle.perturb(77, 1000 + i, 3, codes[i, :m].astype(np.uint8), H, npert) for i in range(200)])
            assert np.array_equal(got, ref), (m, npert)
            assert ((got != codes[:, :m]).sum(1) <= npert).all()


@pytest.mark.parametrize("kind,d,m", [("gauss", 33, 7), ("sift", 128, 8), ("exact", 30, 16), ("gauss", 1, 3), ("exact", 64, 1)])
def test_decomposition_equals_the_direct_form(kind, d, m):
    X, K, B0 = _problem(kind, 40, d, m, 3)
    IR.check_decomposition(IR.Case(X, K, m), B0.astype(np.int64) - 1, np.arange(0, 40, 5))


@pytest.mark.parametrize("kind,d,m,offset", [("gauss", 32, 8, 0.0), ("sift", 128, 8, 0.0), ("gauss", 30, 16, 300.0), ("gauss", 3, 4, 0.0),
                                             ("gauss", 960, 2, 0.0), ("exact", 64, 16, 0.0), ("exact", 1, 5, 0.0)])
def test_bounds_hold_for_f32_evaluations(oracle, kind, d, m, offset):
    """The oracle's f32 tables (k-ascending fmaf chains) summed in f32 over the conditioning codebooks in ascending and in descending k:
    within the bound of the float64 value every time; in the exact regime bound 0 and equal.  The same for the f32 cost."""
    n = 24
    X, K, B0 = _problem(kind, n, d, m, 5)
    if offset:
        u = np.random.default_rng(1).standard_normal(d).astype(np.float32)
        X, K = (X + np.float32(offset) * u).astype(np.float32), (K + np.float32(offset / m) * u).astype(np.float32)
    case = IR.Case(X, K, m)
    U, T = oracle.unaries(X, K, m, H), oracle.tables(K, m, H)
    codes = B0.astype(np.int64) - 1
    S, A = case.gather(codes)
    rows = np.arange(n)
    for j in range(m):
        E, b = case.node(rows, S, A, codes[:, j], j)
        others = [k for k in range(m) if k != j]
        for ks in (others, others[::-1]):
            s = U[j].copy()
            for k in ks:
                s = (s + T[j, k, codes[:, k]]).astype(np.float32)
            err = np.abs(s.astype(np.float64) - E)
            assert (err <= b).all(), "node %d: f32 value off by %g > bound %g" % (j, err.max(), b[np.unravel_index(np.argmax(err - b), b.shape)])
            if kind == "exact":
                assert not b.any() and not err.any()
    c64, cb = case.cost(rows, codes)
    cost = oracle.veccost(X, K, codes.astype(np.uint8), H).astype(np.float64)
    assert (np.abs(cost - c64) <= cb).all()
    if kind == "exact":
        assert not cb.any() and np.array_equal(cost, c64)


# ---- the replay judges the oracle ----------------------------------------------------------------------------------------------------

ORACLE_CASES = [
    # kind, d, m, npert, icmiter, randord
    ("exact", 16, 1, 1, 4, True), ("exact", 24, 2, 0, 4, True), ("exact", 32, 3, 3, 1, False), ("exact", 48, 7, 1, 4, True),
    ("exact", 64, 8, 8, 1, True), ("exact", 32, 8, 0, 1, False), ("exact", 30, 16, 16, 4, True), ("exact", 17, 16, 1, 1, True),
    ("exact", 3, 8, 4, 4, True), ("exact", 1, 4, 2, 4, False), ("exact", 40, 7, 7, 4, False), ("exact", 8, 2, 2, 1, True),
    ("gauss", 32, 1, 1, 1, True), ("gauss", 33, 2, 2, 4, False), ("sift", 64, 3, 0, 4, True), ("gauss", 30, 7, 7, 1, True),
    ("sift", 128, 8, 1, 4, True), ("gauss", 16, 16, 16, 4, False), ("gauss", 24, 16, 0, 1, True), ("sift", 32, 8, 8, 1, False),
]


@pytest.mark.parametrize("kind,d,m,npert,J,randord", ORACLE_CASES)
def test_replay_judges_the_oracle(oracle, node_order, kind, d, m, npert, J, randord):
    n, I, seed = 400, 3, d * 31 + m
    X, K, B0 = _problem(kind, n, d, m, seed)
    Bs, _, stats = oracle.encode_icm(X, B0, K, m, H, list(range(1, I + 1)), J, npert, randord, seed, want_stats=True)
    rep = judge(node_order, X, K, B0, m, list(Bs), J, npert, randord, seed, stats.astype(np.int64))
    rep.assert_no_wrong("oracle, %s d=%d m=%d npert=%d J=%d" % (kind, d, m, npert, J))
    if kind == "exact":
        assert rep.counts()["verified"] == I * n, rep.message()
        assert all(e is not None for e in rep.equal)                   # every ==/< counter predicted and matched
    else:
        assert rep.fraction_verified() >= 0.9, rep.message()


FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "g*.npz")))


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_replay_accepts_the_golden_fixtures(node_order, path):
    """Only the checkpoints in `ilsiters` are stored: the iterations between them are followed where every decision is forced."""
    z = np.load(path)
    d, n, m, h, J, npert, randord, seed = [int(v) for v in z["params"]]
    X, K = z["X8"].astype(np.float32), z["P8"].astype(np.float32) / np.float32(m)
    outs = [None] * int(z["ilsiters"].max())
    for r, t in enumerate(z["ilsiters"]):
        outs[int(t) - 1] = z["Bs"][r]
    rep = judge(node_order, X, K, z["B0"], m, outs, J, npert, bool(randord), seed, z["stats"])
    rep.assert_no_wrong(os.path.basename(path))
    assert rep.counts()["verified"] > 0, rep.message()


# ---- sensitivity: the slips bit-parity between two restatements cannot see ----------------------------------------------------------

MUTATIONS = {
    "highest_index_on_ties": ("if (s[a] < minv) { minv = s[a]; mini = a; }", "if (s[a] <= minv) { minv = s[a]; mini = a; }"),
    "accept_on_le": ("if (nc < prev) {", "if (nc <= prev) {"),
    "transposed_pair_table": ("const float *col = T + (((size_t)j * m + k) * h + code[k]) * h;",
                              "const float *col = T + (((size_t)k * m + j) * h + code[k]) * h;"),
    "conditioning_term_skipped": ("        if (k == j) continue;\n        const float *col = T",
                                  "        if (k == j || k == (j + 1) % m) continue;\n        const float *col = T"),
    "perturbs_the_last_sweep": ("memcpy(nw, cur, (size_t)m);\n                orc_perturb(", "if (it == 0) memcpy(nw, cur, (size_t)m);\n                orc_perturb("),
}
SENSITIVITY_CASES = [("exact", 16, 8, 2, 4, True), ("exact", 24, 4, 4, 1, True), ("gauss", 32, 8, 4, 4, True)]


def _scratch_oracle(tmp_path, name):
    """oracle/lsq_oracle.c with one mutation applied, compiled with the oracle's flags into tmp_path -> ctypes handle"""
    src = open(os.path.join(ROOT, "oracle", "lsq_oracle.c")).read()
    if name != "none":
        old, new = MUTATIONS[name]
        assert src.count(old) == 1, "mutation %s no longer applies to oracle/lsq_oracle.c" % name
        src = src.replace(old, new)
    c, so = tmp_path / ("orc_%s.c" % name), tmp_path / ("liborc_%s.so" % name)
    c.write_text(src)
    subprocess.check_call(["gcc", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-fno-math-errno", "-fopenmp", "-fPIC", "-shared",
                           "-std=gnu11", "-o", str(so), str(c), "-lm"])
    L = C.CDLL(str(so))
    p = C.c_void_p
    L.orc_encode_icm.argtypes = [p, p, p, C.c_int, C.c_long, C.c_int, C.c_int, p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, p, p, p]
    return L


def _scratch_encode(L, X, B0, K, m, I, J, npert, randord, seed):
    n, d = X.shape
    ils = np.arange(1, I + 1, dtype=np.int64)
    Bs = np.zeros((I, n, m), np.int16)
    objs = np.zeros(I, np.float32)
    stats = np.zeros((I, 2), np.float64)
    B0 = np.ascontiguousarray(B0, np.int16)
    assert L.orc_encode_icm(X.ctypes.data, B0.ctypes.data, K.ctypes.data, d, n, m, H, ils.ctypes.data, I, J, npert, int(randord), seed, 0,
                            Bs.ctypes.data, objs.ctypes.data, stats.ctypes.data) == 0
    return Bs, stats.astype(np.int64)


@pytest.mark.parametrize("name", ["none"] + sorted(MUTATIONS))
def test_replay_catches_each_mutation_of_the_oracle(tmp_path, node_order, name):
    L = _scratch_oracle(tmp_path, name)
    failures = []
    for kind, d, m, npert, J, randord in SENSITIVITY_CASES:
        n, I, seed = 300, 3, 40 + d
        X, K, B0 = _problem(kind, n, d, m, seed)
        Bs, stats = _scratch_encode(L, X, B0, K, m, I, J, npert, randord, seed)
        try:
            rep = judge(node_order, X, K, B0, m, list(Bs), J, npert, randord, seed, stats)
            rep.assert_no_wrong()
            if kind == "exact":
                assert rep.counts()["verified"] == I * n, rep.message()
        except AssertionError as e:
            failures.append("%s d=%d m=%d npert=%d J=%d: %s" % (kind, d, m, npert, J, str(e).strip().splitlines()[0]))
    print("\n".join(["mutation %s:" % name] + failures))
    if name == "none":
        assert not failures, failures                                    # the scratch build itself is judged correct
    else:
        assert failures, "the replay did not notice mutation %s" % name
