"""The beam-search encoder without a device: its four symbols in the header, the binding and both libraries; the numpy checker (tests/beam_check.py)
against things it shares no code with -- brute force, an explicit greedy loop, the nearest-codeword checker, the oracle's veccost --; and what the Python
layers hand to the library (the recorder of tests/engine_calls.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import engine_calls as ec
import oracle.init_oracle as ini
from beam_check import beam_exact, cost_and_score_bound
from conftest import make_problem
from engine_calls import D, H, M, N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lsq_encoder_create", "lsq_encoder_destroy", "lsq_encoder_beam", "lsq_encoder_get_info")
ENCODER = 7777                                # the handle the stand-in's lsq_encoder_create hands out: no extent or argument of the cases below


# ---- header and ABI ---------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_encoder_behind_its_own_handle(lsq):
    hdr = open(os.path.join(ROOT, "include", "lsq_mi355x.h")).read()
    assert int(re.search(r"#define\s+LSQ_VERSION\s+(\d+)", hdr).group(1)) >= 1600
    for sym in SYMBOLS:
        decl = re.search(r"LSQ_API\s+int\s+%s\s*(\([^;]*\));" % sym, hdr)
        assert decl, "%s is not declared" % sym
        assert not re.match(r"\(\s*(?:struct\s+)?lsq_ctx\s*\*", decl.group(1)), "%s takes the context first: the context catalogues are closed" % sym
        assert sym in lsq._lib.SIGNATURES
    for path in (lsq._lib.LIB_PATH, lsq._lib.TUNING_LIB_PATH):
        lib = C.CDLL(path)
        for sym in SYMBOLS:
            assert hasattr(lib, sym), "%s does not export %s" % (os.path.basename(path), sym)
    assert lsq._lib.load().lsq_version() >= 1600
    for cite in ("encode_icm.jl:55-70", "encode_chain.jl:2-89", "NO COUNTERPART"):
        assert cite in hdr


def test_null_handles_are_refused_without_a_device(lsq):
    L, EINVAL = lsq._lib.load(), lsq._lib.LSQ_EINVAL
    x = np.zeros((2, 4), np.float32)
    out = np.zeros((2, 1), np.int16)
    assert L.lsq_encoder_beam(None, x.ctypes.data, 0, 2, 1, None, out.ctypes.data, None, 0) == EINVAL
    assert b"lsq_encoder_beam" in L.lsq_last_error()
    assert L.lsq_encoder_get_info(None, C.byref(lsq._lib.EncoderInfo())) == EINVAL
    h, desc = C.c_void_p(), lsq._lib.EncoderDesc()
    assert L.lsq_encoder_create(C.byref(h), None, C.byref(desc)) == EINVAL and not h.value
    assert L.lsq_encoder_create(None, None, C.byref(desc)) == EINVAL
    assert L.lsq_encoder_destroy(None) == lsq._lib.LSQ_OK


# ---- the checker against what it shares no code with --------------------------------------------------------------------------------------------------------
def _gauss(seed, d, n, m):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((m * H, d)).astype(np.float32)


def test_two_codebooks_and_a_full_beam_is_brute_force(oracle):
    """m = 2, L = 256: stage 0 keeps every code, so the result is the first minimum over all 65 536 pairs of the same f32 sums, the parents ranked by
    their unary (equal unaries: the smaller code first)"""
    X, K = _gauss(1, 16, 30, 2)
    K[5] = K[3]                                                    # two equal stage-0 candidates: the rank rule shows
    codes, score = beam_exact(X, K, 2, 256)
    U, T = oracle.unaries(X, K, 2, H), oracle.tables(K, 2, H)
    for i in range(X.shape[0]):
        rank = sorted(range(H), key=lambda b: (U[0, i, b], b))
        best = None
        for p, b in enumerate(rank):
            for a in range(H):
                v = np.float32(U[0, i, b] + np.float32(U[1, i, a] + T[1, 0, b, a]))
                if best is None or v < best[0]:
                    best = (v, b, a)
        assert (codes[i, 0], codes[i, 1]) == (best[1], best[2]) and score[i].tobytes() == np.float32(best[0]).tobytes()


def _greedy_loop_agrees(oracle, X, K, m, order):
    codes, score = beam_exact(X, K, m, 1, order)
    U, T = oracle.unaries(X, K, m, H), oracle.tables(K, m, H)
    o = list(range(m)) if order is None else order
    for i in range(X.shape[0]):
        b, S = {}, None
        for t, j in enumerate(o):
            s = U[j, i].copy()
            for r in range(t):
                s = s + T[j, o[r], b[o[r]]]
            v = s if t == 0 else np.float32(S) + s
            b[j] = int(np.argmin(v))
            S = v[b[j]]
        assert [b[j] for j in range(m)] == codes[i].tolist() and np.float32(S).tobytes() == score[i].tobytes()


@pytest.mark.parametrize("order", [None, [2, 0, 3, 1]])
def test_beam_of_one_is_the_greedy_loop(oracle, order):
    m = 4
    X, K = _gauss(2, 12, 25, m)
    _greedy_loop_agrees(oracle, X, K, m, order)


@pytest.mark.parametrize("kind", ["gauss", "int"])
def test_beam_of_one_is_the_greedy_loop_past_eight_codebooks(oracle, kind):
    """what tests/test_gpu_beam.py holds the greedy kernel's second code word to: m = 11, ascending and the high-first order; small integers: exact ties"""
    m = 11
    X, K = _gauss(6, 12, 25, m)
    if kind == "int":
        rng = np.random.default_rng(6)
        X, K = rng.integers(-3, 4, X.shape).astype(np.float32), rng.integers(-2, 3, K.shape).astype(np.float32)
    for order in (None, [10, 0, 9, 1, 8, 2, 7, 3, 6, 4, 5]):
        _greedy_loop_agrees(oracle, X, K, m, order)


def test_all_equal_candidates_resolve_by_position():
    """one codeword everywhere and rows of zeros: every candidate of every stage ties, and the (v, p, a) rule leaves code 0 in every codebook"""
    m, d = 4, 16
    c = np.random.default_rng(7).integers(-2, 3, size=d).astype(np.float32)
    X, K = np.zeros((9, d), np.float32), np.tile(c, (m * H, 1))
    for L in (1, 4, 32):
        codes, score = beam_exact(X, K, m, L)
        assert not codes.any() and np.all(score == np.float32(m * m * (c * c).sum()))


def test_one_codebook_is_the_nearest_codeword():
    X, K = _gauss(3, 24, 77, 1)
    K[1::2] = K[0::2]                                              # duplicates: the first copy wins
    want, want_min = ini.assign_codewords_exact(X, K, 1, H)
    for L in (1, 7):
        codes, score = beam_exact(X, K, 1, L)
        assert np.array_equal(codes, want) and np.array_equal(score, want_min[:, 0])


def test_score_is_the_cost_minus_the_norm(oracle):
    m = 5
    X, K = _gauss(4, 32, 120, m)
    K /= np.float32(m)
    for L, order in ((1, None), (6, [4, 1, 0, 3, 2])):
        codes, score = beam_exact(X, K, m, L, order)
        cost = oracle.veccost(X, K, codes.astype(np.uint8), H).astype(np.float64)
        got = (X.astype(np.float64) ** 2).sum(1) + score
        rel = np.abs(got - cost) / cost
        print("L=%d: max relative difference %.3g" % (L, rel.max()))
        assert rel.max() <= 1e-5


def test_score_is_the_float64_reconstruction_error_within_the_derived_bound():
    """the checker's own f32 score at the shape tests/test_gpu_beam.py holds the device's to: the bound of cost_and_score_bound is derived, not measured,
    and a correct f32 evaluation stays far inside it (largest ratio here: 0.00647 at L = 1, 0.0049 at L = 16); a score off by one table entry is far outside"""
    d, n, m = 128, 300, 8
    rng = np.random.default_rng(100 + d + n + m)
    X = rng.standard_normal((n, d)).astype(np.float32)
    K = (rng.standard_normal((m * H, d)) / m).astype(np.float32)
    for L in (1, 16):
        codes, score = beam_exact(X, K, m, L)
        cost, bound = cost_and_score_bound(X, K, m, codes)
        err = np.abs((X.astype(np.float64) ** 2).sum(1) + score.astype(np.float64) - cost)
        print("L=%d: max |error| / bound %.3g (max bound / cost %.3g)" % (L, (err / bound).max(), (bound / cost).max()))
        assert np.all(err <= bound)
        entry = 2 * (K[codes[:, 0]].astype(np.float64) * K[H + codes[:, 1]]).sum(1)          # T[1][0][b_0][b_1], left out of the score
        assert np.mean(np.abs(entry) - err > bound) > 0.9                                     # |error without it| >= |entry| - |error with it|


def test_a_wider_beam_finds_a_lower_score():
    X, K, _ = make_problem(128, 1024, 8, seed=0, kind="gauss")
    s1, s16 = beam_exact(X, K, 8, 1)[1], beam_exact(X, K, 8, 16)[1]
    norm = float((X.astype(np.float64) ** 2).sum(1).mean())
    print("objective: L = 1 %.2f, L = 16 %.2f" % (norm + s1.mean(dtype=np.float64), norm + s16.mean(dtype=np.float64)))
    assert s16.mean(dtype=np.float64) < s1.mean(dtype=np.float64)


def test_uint8_rows_are_the_widened_rows():
    rng = np.random.default_rng(5)
    X8 = rng.integers(0, 256, size=(40, 16), dtype=np.uint8)
    K = (rng.integers(0, 256, size=(3 * H, 16)) / 3.0).astype(np.float32)
    a, b = beam_exact(X8, K, 3, 4), beam_exact(X8.astype(np.float32), K, 3, 4)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


# ---- the Python layers hand arrays on as given --------------------------------------------------------------------------------------------------------------
class _EncoderTracer(ec.Tracer):
    """the stand-in library, handing out an encoder handle as it does an index handle"""

    def __getattr__(self, name):
        fn = super().__getattr__(name)
        if name != "lsq_encoder_create":
            return fn

        def create(*args):
            rc = fn(*args)
            args[0]._obj.value = ENCODER
            return rc
        return create


def _offline(lsq):
    eng = ec.offline_engine(lsq)
    eng._L = _EncoderTracer()
    return eng


def test_encoder_passes_what_it_was_given(lsq):
    P, eng = ec.Problem(), _offline(lsq)
    order = np.array([2, 0, 1], dtype=np.int32)
    more = lambda _: {"encoder": ENCODER, "order": order}      # noqa: E731
    enc = ec.run_case(eng, P, lambda e, P: e.encoder(P.K, M, chunk=50), (None,),
                      [("lsq_encoder_create", ["encoder", "ctx", dict(d=D, m=M, h=H, codebooks="K", on_device=0, chunk=50)])], extra=more)
    assert (enc.d, enc.m) == (D, M) and enc in eng._indexes
    codes, score = ec.run_case(eng, P, lambda e, P: enc.beam(P.X, 5, order=order, want_score=True), ("codes", "score"),
                               [("lsq_encoder_beam", ["encoder", "X", 0, N, 5, "order", "codes", "score", 0])], extra=more)
    assert codes.dtype == np.int16 and codes.shape == (N, M) and score.dtype == np.float32 and score.shape == (N,)
    codes = ec.run_case(eng, P, lambda e, P: enc.beam(P.X8, 32), ("codes",),
                        [("lsq_encoder_beam", ["encoder", "X8", 1, N, 32, None, "codes", None, 0])], extra=more)
    assert codes.dtype == np.int16
    ec.run_case(eng, P, lambda e, P: enc.info(), (None,), [("lsq_encoder_get_info", ["encoder", ec.zeros_of(lsq._lib.EncoderInfo)])], extra=more)
    with pytest.raises(ValueError):
        enc.beam(P.X[:, :D - 1], 4)                                # another d than the codebooks'
    with pytest.raises(ValueError):
        enc.beam(P.X, 4, order=[0, 1])                             # an order of another length
    with pytest.raises(TypeError):
        enc.beam(P.X8.view(np.int8), 4)
    ec.run_case(eng, P, lambda e, P: enc.close(), (None,), [("lsq_encoder_destroy", ["encoder"])], extra=more)
    ec.run_case(eng, P, lambda e, P: enc.close(), (None,), [], extra=more)              # once


def test_a_closed_engine_closes_its_encoders_first(lsq):
    P, eng = ec.Problem(), _offline(lsq)
    enc, ix = eng.encoder(P.K, M), eng.index(P.codes, P.K, P.dbnorms, M)
    tracer = eng._L
    tracer.calls.clear()
    eng.close()
    names = [s for s, _ in tracer.calls]
    assert sorted(names[:2]) == ["lsq_encoder_destroy", "lsq_index_destroy"] and names[2:] == ["lsq_destroy"]
    assert enc._h is None and ix._h is None


def test_reference_shaped_call_goes_through_an_encoder(lsq):
    P, eng = ec.Problem(), _offline(lsq)
    eng._L = _EncoderTracer(peek={("lsq_encoder_beam", 5): 4 * M})                          # the order is a temporary of the binding's
    Cs = [np.ascontiguousarray(P.K[j * H:(j + 1) * H].T) for j in range(M)]                 # Julia shapes: d x h
    B = lsq.encode_beam(P.X.T, Cs, 8, order=[1, 2, 0], engine=eng)
    assert B.shape == (M, N) and B.dtype == np.int16
    calls = eng._L.calls
    assert [s for s, _ in calls] == ["lsq_encoder_create", "lsq_encoder_beam", "lsq_encoder_destroy"]
    assert calls[1][1][2:5] == (0, N, 8) and calls[1][1][8] == 0
    assert eng._L.peeked[(1, 5)] == np.array([1, 2, 0], np.int32).tobytes()
    # beam_order: descending mean squared norm, equal means in ascending order
    Cs2 = [np.full((4, H), v, np.float32) for v in (1.0, 3.0, 1.0, 2.0)]
    assert lsq.beam_order(Cs2).tolist() == [1, 3, 0, 2] and lsq.beam_order(Cs2).dtype == np.int32


def test_device_form_refuses_host_arrays(lsq):
    import torch
    P, eng = ec.Problem(), _offline(lsq)
    with pytest.raises(TypeError):
        eng.encoder_dev(P.K, M)
    with pytest.raises(TypeError):
        eng.encoder_dev(torch.from_numpy(P.K), M)                   # a CPU tensor
    enc = lsq.Encoder.__new__(lsq.Encoder)
    enc._eng, enc._L, enc._dev, enc._h, enc.d, enc.m = eng, eng._L, True, C.c_void_p(ENCODER), D, M
    eng._L.calls.clear()
    for bad in (P.X, torch.from_numpy(P.X), torch.from_numpy(P.X).double()):
        with pytest.raises(TypeError):
            enc.beam(bad, 4)
    assert eng._L.calls == []
    enc._h = None
