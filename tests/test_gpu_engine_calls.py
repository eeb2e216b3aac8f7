"""What the device forms of the binding pass to the library: tests/test_engine_calls.py's comparison on real device tensors, still around the stand-in
library (tests/engine_calls.py) -- no kernel runs, only torch allocations.  The expected entry of a device form is the whole sequence: lsq_set_stream
with the handle of torch's CURRENT stream (every call runs under a non-default torch.cuda.stream, so the default stream's handle would show), the call
itself, lsq_set_option("own_stream", 1).  Views are passed in place: the base of pitch 40 and the query rows of pitch 32 arrive as ldb = 40, ldq = 32."""
import numpy as np
import pytest

import engine_calls as ec
from engine_calls import D, DC, H, KK, L, LDB, LDQ, M, N, NCB, NQ, SUBDIM, Temp

pytestmark = pytest.mark.gpu

COVER = ec.cover_bytes(ec.Problem())
NCOVER = len(COVER)
BIND, UNBIND = ("lsq_set_stream", ["ctx", "stream"]), ("lsq_set_option", ["ctx", b"own_stream", 1])
ASYNC1, ASYNC0 = ("lsq_set_option", ["ctx", b"async", 1]), ("lsq_set_option", ["ctx", b"async", 0])


def on_stream(*calls):
    return [BIND, *calls, UNBIND]


def desc(**kw):
    return dict(dict(n=N, d=D, m=M, h=H, codes="codes", codebooks="K", dbnorms="dbnorms", base=None, base_u8=0, ldb=0, on_device=1), **kw)


BASE_ONLY = dict(m=0, codes=None, codebooks=None, dbnorms=None)

# name -> (call, names of what it returns, the expected calls[, {(symbol, position): bytes to copy from behind a HOST temporary}])
DEVICE = {
    "encode_icm_dev": (lambda e, P: e.encode_icm_dev(P.X, P.codes, P.K, M, P.ils, 6, 7, True, seed=11, global_offset=13), ("Bs", "obj", "stats"),
                       on_stream(("lsq_encode_icm_dev", ["ctx", "X", "codes", "K", D, N, M, H, "ils", 2, 6, 7, 1, 11, 13, "Bs", "obj", "stats"]))),
    "encode_icm_dev[u8, out]": (lambda e, P: e.encode_icm_dev(P.X8, P.codes, P.K, M, P.ils, 6, 7, False, seed=11, out=P.outbuf), ("outbuf", "obj", "stats"),
                                on_stream(("lsq_encode_icm_u8_dev", ["ctx", "X8", "codes", "K", D, N, M, H, "ils", 2, 6, 7, 0, 11, 0, "outbuf", "obj", "stats"]))),
    "encode_icm_dev[nonblocking]": (lambda e, P: e.encode_icm_dev(P.X, P.codes, P.K, M, P.ils, 6, 7, True, seed=11, nonblocking=True), ("Bs", "obj", "stats"),
                                    [BIND, ASYNC1, ("lsq_encode_icm_dev", ["ctx", "X", "codes", "K", D, N, M, H, "ils", 2, 6, 7, 1, 11, 0, "Bs", "obj", "stats"]),
                                     ASYNC0, UNBIND]),
    "linscan_dev": (lambda e, P: e.linscan_dev(P.codes, P.Q, P.K, P.dbnorms, M, KK), ("dists", "ids"),
                    on_stream(("lsq_linscan_dev", ["ctx", "dists", "ids", "codes", "Q", "K", "dbnorms", NQ, N, M, H, D, KK]))),
    "linscan_pq_dev": (lambda e, P: e.linscan_pq_dev(P.codes_pq, P.Q, P.C3, M, KK, SUBDIM), ("dists", "ids"),
                       on_stream(("lsq_linscan_pq_dev", ["ctx", "dists", "ids", "codes_pq", "C3", "Q", N, NQ, 8 * M, KK, DC, D, SUBDIM]))),
    "knn_exact_dev": (lambda e, P: e.knn_exact_dev(P.base, P.Qrows, KK), ("dists", "ids"),
                      on_stream(("lsq_knn_exact_dev", ["ctx", "dists", "ids", "base", "Qrows", N, NQ, D, LDB, LDQ, KK]))),
    "knn_exact_dev[u8]": (lambda e, P: e.knn_exact_dev(P.base8, P.Qrows8, KK), ("dists", "ids"),
                          on_stream(("lsq_index_create", ["index", "ctx", desc(base="base8", base_u8=1, ldb=LDB, **BASE_ONLY)]))
                          + on_stream(("lsq_index_knn", ["index", "dists", "ids", "Qrows8", 1, NQ, LDQ, KK, 0, 1])) + [("lsq_index_destroy", ["index"])]),
    "quantize_norms_dev": (lambda e, P: e.quantize_norms_dev(P.codes, P.K, P.cb, M), ("idx", "dbn", "nrm"),
                           on_stream(("lsq_quantize_norms_dev", ["ctx", "codes", "K", "cb", NCB, D, N, M, H, "idx", "dbn", "nrm"]))),
    "update_codebooks_dev": (lambda e, P: e.update_codebooks_dev(P.X, P.codes, M), ("Kout", None),
                             on_stream(("lsq_update_codebooks_dev", ["ctx", "X", "codes", D, N, M, H, "Kout", 0]))),
    "update_codebooks_dev[out]": (lambda e, P: e.update_codebooks_dev(P.X, P.codes, M, out=P.Kbuf), ("Kbuf", None),
                                  on_stream(("lsq_update_codebooks_dev", ["ctx", "X", "codes", D, N, M, H, "Kbuf", 0]))),
    "update_codebooks_struct_dev[device cover]": (lambda e, P: e.update_codebooks_struct_dev(P.X, P.codes, P.cover, M, out=P.Kbuf), ("Kbuf", None),
                                                  on_stream(("lsq_update_codebooks_struct_dev", ["ctx", "X", "codes", Temp(), D, N, M, H, "Kbuf", 0]))),
    "update_codebooks_struct_dev[host cover]": (lambda e, P: e.update_codebooks_struct_dev(P.X, P.codes, P.cover_host, M), ("Kout", None),
                                                on_stream(("lsq_update_codebooks_struct_dev", ["ctx", "X", "codes", Temp(), D, N, M, H, "Kout", 0]))),
    "update_codebooks_struct_dev[no cover]": (lambda e, P: e.update_codebooks_struct_dev(P.X, P.codes, None, M), ("Kout", None),
                                              on_stream(("lsq_update_codebooks_struct_dev", ["ctx", "X", "codes", None, D, N, M, H, "Kout", 0]))),
    "update_codebooks_spgl1_dev": (lambda e, P: e.update_codebooks_spgl1_dev(P.X, P.codes, M, 2.5, dK_init=P.K, S=9, opt_tol=0.5, max_iter=7, out=P.Kbuf),
                                   ("Kbuf", None),
                                   on_stream(("lsq_update_codebooks_spgl1_dev",
                                              ["ctx", "X", "codes", D, N, M, H, 2.5, "K", 9, dict(opt_tol=0.5, max_iter=7), "Kbuf", "INFO"]))),
    "update_codebooks_spgl1_dev[defaults]": (lambda e, P: e.update_codebooks_spgl1_dev(P.X, P.codes, M, 2.5), ("Kout", None),
                                             on_stream(("lsq_update_codebooks_spgl1_dev", ["ctx", "X", "codes", D, N, M, H, 2.5, None, -1, None, "Kout", "INFO"]))),
    "encode_viterbi_dev": (lambda e, P: e.encode_viterbi_dev(P.X, P.K, M), ("Bout",),
                           on_stream(("lsq_encode_viterbi_dev", ["ctx", "X", "K", D, N, M, H, "Bout"]))),
    "assign_codewords_dev": (lambda e, P: e.assign_codewords_dev(P.X, P.K, M), ("Bout",),
                             on_stream(("lsq_assign_codewords_dev", ["ctx", "X", "K", D, N, M, H, "Bout", None]))),
    "assign_codewords_dev[min]": (lambda e, P: e.assign_codewords_dev(P.X, P.K, M, want_min=True), ("Bout", "mv"),
                                  on_stream(("lsq_assign_codewords_dev", ["ctx", "X", "K", D, N, M, H, "Bout", "mv"]))),
    "update_centers_dev": (lambda e, P: e.update_centers_dev(P.X, P.codes, P.cover_host, M, K_prev=P.K), ("Kout", "counts"),
                           on_stream(("lsq_update_centers_dev", ["ctx", "X", "codes", Temp(COVER), "K", D, N, M, H, "Kout", "counts"])),
                           {("lsq_update_centers_dev", 3): NCOVER}),
    "update_centers_dev[out, counts, device cover]": (lambda e, P: e.update_centers_dev(P.X, P.codes, P.cover, M, out=P.Kbuf, counts=P.cntbuf),
                                                      ("Kbuf", "cntbuf"),
                                                      on_stream(("lsq_update_centers_dev", ["ctx", "X", "codes", Temp(COVER), None, D, N, M, H, "Kbuf", "cntbuf"])),
                                                      {("lsq_update_centers_dev", 3): NCOVER}),
    "kmeanspp_seed_dev": (lambda e, P: e.kmeanspp_seed_dev(P.X, P.cover_host, P.u, M), ("Kout", "idx", None),
                          on_stream(("lsq_kmeanspp_seed_dev", ["ctx", "X", Temp(COVER), "u", D, N, M, H, "Kout", "idx", None])),
                          {("lsq_kmeanspp_seed_dev", 2): NCOVER}),
    "kmeanspp_seed_dev[d2, out]": (lambda e, P: e.kmeanspp_seed_dev(P.X, P.cover_host, P.u, M, want_idx=False, want_d2=True, out=P.Kbuf), ("Kbuf", None, "d2"),
                                   on_stream(("lsq_kmeanspp_seed_dev", ["ctx", "X", Temp(COVER), "u", D, N, M, H, "Kbuf", None, "d2"])),
                                   {("lsq_kmeanspp_seed_dev", 2): NCOVER}),
    "kmeanspp_seed_dev[n = 0]": (lambda e, P: e.kmeanspp_seed_dev(P.X[:0], P.cover_host, P.u, M, want_d2=True), ("Kout", "idx", None),
                                 on_stream(("lsq_kmeanspp_seed_dev", ["ctx", 0, Temp(COVER), "u", D, 0, M, H, "Kout", "idx", None])),      # no rows: torch's null
                                 {("lsq_kmeanspp_seed_dev", 2): NCOVER}),
    "synth_data_u8_dev": (lambda e, P: e.synth_data_u8_dev(11, N, D, global_offset=13), ("Xout",),
                          on_stream(("lsq_synth_data_u8_dev", ["ctx", 11, 13, N, D, "Xout"]))),
    "randinit_dev": (lambda e, P: e.randinit_dev(11, N, M, global_offset=13), ("Bout",), on_stream(("lsq_randinit_dev", ["ctx", 11, 13, N, M, H, "Bout"]))),
    "synth_codebooks_dev": (lambda e, P: e.synth_codebooks_dev(11, M, D), ("Kout",), on_stream(("lsq_synth_codebooks_dev", ["ctx", 11, M, H, D, "Kout"]))),
}


@pytest.fixture(scope="module")
def problem():
    import torch
    P = ec.Problem().to_device("cuda:0")
    P.outbuf = torch.empty((2, N, M), dtype=torch.uint8, device="cuda:0")
    P.Kbuf = torch.empty((M * H, D), dtype=torch.float32, device="cuda:0")
    P.cntbuf = torch.empty(M * H, dtype=torch.int32, device="cuda:0")
    return P


def _on_side_stream(lsq, P, call, outputs, expected, peek=None, eng=None):
    """the case under a non-default stream: the handle the binding binds must be that stream's"""
    import torch
    info = ec.zeros_of(lsq._lib.Spgl1Info)
    expected = [(s, [info if isinstance(a, str) and a == "INFO" else a for a in args]) for s, args in expected]
    eng = eng or ec.offline_engine(lsq, peek=peek)
    side = torch.cuda.Stream(device=0)
    assert side.cuda_stream != torch.cuda.default_stream(0).cuda_stream
    with torch.cuda.stream(side):
        result = ec.run_case(eng, P, call, outputs, expected, extra=lambda r: {"stream": side.cuda_stream})
    torch.cuda.synchronize()
    return result


@pytest.mark.parametrize("name", list(DEVICE))
def test_device_form_passes_what_it_was_given(lsq, problem, name):
    result = _on_side_stream(lsq, problem, *DEVICE[name])
    if name == "kmeanspp_seed_dev[n = 0]":
        assert tuple(result[2].shape) == (0, M)      # the empty d2 is made and returned; the library gets a null pointer for it


def test_nonblocking_results_are_zeroed_device_tensors_and_blocking_ones_host_arrays(lsq, problem):
    _, obj, stats = _on_side_stream(lsq, problem, *DEVICE["encode_icm_dev[nonblocking]"])
    assert obj.is_cuda and stats.is_cuda and tuple(obj.shape) == (2,) and tuple(stats.shape) == (2, 2) and not obj.any() and not stats.any()
    _, obj, stats = _on_side_stream(lsq, problem, *DEVICE["encode_icm_dev"])
    assert isinstance(obj, np.ndarray) and obj.dtype == np.float64 and isinstance(stats, np.ndarray) and stats.dtype == np.int64 and stats.shape == (2, 2)


@pytest.mark.parametrize("u8", [False, True], ids=["f32 base", "uint8 base"])
def test_device_index_borrows_views_in_place(lsq, problem, u8):
    P, eng = problem, ec.offline_engine(lsq)
    base, rows = ("base8", "Qrows8") if u8 else ("base", "Qrows")
    ix = _on_side_stream(lsq, P, lambda e, P: e.index_dev(P.codes, P.K, P.dbnorms, M, base=getattr(P, base)), (None,),
                         on_stream(("lsq_index_create", ["index", "ctx", desc(base=base, base_u8=int(u8), ldb=LDB)])), eng=eng)
    assert ix._keep[0] is P.codes and ix._keep[3] is getattr(P, base) and (ix.n, ix.d, ix.m) == (N, D, M)
    _on_side_stream(lsq, P, lambda e, P: ix.search(P.Q, KK, L, P.Q2), ("dists", "ids"),
                    on_stream(("lsq_index_search", ["index", "dists", "ids", "Q", "Q2", NQ, D, L, KK, 1])), eng=eng)
    _on_side_stream(lsq, P, lambda e, P: ix.rerank(P.Q, P.cand, KK, id_base=0), ("dists", "ids"),
                    on_stream(("lsq_index_rerank", ["index", "dists", "ids", "Q", "cand", NQ, D, L, KK, 0, 1])), eng=eng)
    _on_side_stream(lsq, P, lambda e, P: ix.knn(getattr(P, rows), KK, id_base=1), ("dists", "ids"),
                    on_stream(("lsq_index_knn", ["index", "dists", "ids", rows, int(u8), NQ, LDQ, KK, 1, 1])), eng=eng)
    _on_side_stream(lsq, P, lambda e, P: ix.close(), (None,), [("lsq_index_destroy", ["index"])], eng=eng)


@pytest.mark.parametrize("nonblocking", [False, True], ids=["blocking", "nonblocking"])
def test_a_failed_call_still_unbinds_the_stream(lsq, problem, nonblocking):
    """the entry point returns LSQ_EINVAL: LsqError with the library's message, and the tail of the sequence (async 0, own_stream 1) is still recorded"""
    import torch
    P, eng = problem, ec.offline_engine(lsq, fail="lsq_encode_icm_dev")
    side = torch.cuda.Stream(device=0)
    with torch.cuda.stream(side), pytest.raises(lsq._lib.LsqError, match="stand-in failure") as e:
        eng.encode_icm_dev(P.X, P.codes, P.K, M, P.ils, 6, 7, True, nonblocking=nonblocking)
    assert e.value.code == lsq._lib.LSQ_EINVAL
    got = [(s, a) for s, a in ec.trace(eng._L, {"stream": side.cuda_stream}) if s != "lsq_encode_icm_dev"]
    error = ("lsq_last_error", [])
    assert [s for s, _ in eng._L.calls].count("lsq_encode_icm_dev") == 1
    assert got == ([BIND, ASYNC1, error, ASYNC0, UNBIND] if nonblocking else [BIND, error, UNBIND])


def test_device_forms_refuse_wrong_types_and_strided_views_of_device_tensors(lsq):
    """on a device the refusal is about the tensor itself: the wrong element type is a TypeError, a strided view where contiguity is needed a ValueError"""
    report = ec.refusals("cuda:0")
    assert len(report) > 60
    for case, raised, reached in report:
        want = "ValueError" if case.endswith("strided") else "TypeError"
        assert raised == want and reached == [], "%s: raised %s, reached %s" % (case, raised, reached)

