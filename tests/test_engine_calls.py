"""What the host forms of the binding pass to the library, and what its device forms refuse (no GPU needed: tests/engine_calls.py stands in for the
library).  No test looks at what a call computes -- tests/test_gpu_host_forms.py, ctx_ops.py and the parity tests do -- only at the symbol and the
argument list: an expected entry is written out per method, integers and floats as values, every pointer as the name of the array it addresses (inputs by
their own address: an array already of the right type and layout is passed WITHOUT a copy; outputs by the address of what the method returns), structs
by their field values.  A pointer to no known array stays a number and fails the comparison."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import engine_calls as ec
from engine_calls import D, DC, H, KK, L, LDQ, M, N, NCB, NQ, SUBDIM, Temp

IT_AUTO = 0xFFFFFFFF
COVER = ec.cover_bytes(ec.Problem())
NCOVER = len(COVER)

# name -> (call, names of what it returns, the expected calls[, {(symbol, position): bytes to copy from behind a temporary}])
HOST = {
    "encode_icm": (lambda e, P: e.encode_icm(P.X, P.B, P.K, M, P.ils, 6, 7, True, seed=11, nsplits=2, global_offset=13), ("Bs", "objs"),
                   [("lsq_encode_icm", ["ctx", "X", "B", "K", D, N, M, H, "ils", 2, 6, 7, 1, 2, 11, 13, 0, "Bs", "objs"])]),
    "encode_icm[u8]": (lambda e, P: e.encode_icm(P.X8, P.B, P.K, M, P.ils, 6, 7, False, seed=11, nsplits=2, global_offset=13, verbose=True), ("Bs", "objs"),
                       [("lsq_encode_icm_u8", ["ctx", "X8", "B", "K", D, N, M, H, "ils", 2, 6, 7, 0, 2, 11, 13, 1, "Bs", "objs"])]),
    "linscan": (lambda e, P: e.linscan(P.codes, P.Q, P.K, P.dbnorms, M, KK), ("dists", "ids"),
                [("lsq_linscan", ["ctx", "dists", "ids", "codes", "Q", "K", "dbnorms", NQ, N, M, H, D, KK])]),
    "linscan_pq": (lambda e, P: e.linscan_pq(P.codes_pq, P.Q, P.C3, M, KK, SUBDIM), ("dists", "ids"),
                   [("lsq_linscan_pq", ["ctx", "dists", "ids", "codes_pq", "C3", "Q", N, NQ, 8 * M, KK, DC, D, SUBDIM])]),
    "knn_exact": (lambda e, P: e.knn_exact(P.X, P.Q, KK), ("dists", "ids"),
                  [("lsq_knn_exact", ["ctx", "dists", "ids", "X", "Q", N, NQ, D, D, D, KK])]),
    "knn_exact[u8]": (lambda e, P: e.knn_exact(P.X8, P.Qrows8, KK), ("dists", "ids"),
                      [("lsq_index_create", ["index", "ctx", dict(n=N, d=D, m=0, h=H, codes=None, codebooks=None, dbnorms=None, base="X8", base_u8=1, ldb=D,
                                                                  on_device=0)]),
                       ("lsq_index_knn", ["index", "dists", "ids", "Qrows8", 1, NQ, LDQ, KK, 0, 0]),
                       ("lsq_index_destroy", ["index"])]),
    "quantize_norms": (lambda e, P: e.quantize_norms(P.B, P.K, P.cb, M), ("idx", "dbn", "nrm"),
                       [("lsq_quantize_norms", ["ctx", "B", "K", "cb", NCB, D, N, M, H, "idx", "dbn", "nrm"])]),
    "update_codebooks": (lambda e, P: e.update_codebooks(P.X, P.B, M), ("Kout", None),
                         [("lsq_update_codebooks_gpu", ["ctx", "X", "B", D, N, M, H, "Kout", 0])]),
    "update_codebooks_struct": (lambda e, P: e.update_codebooks_struct(P.X, P.B, P.cover, M), ("Kout", None),
                                [("lsq_update_codebooks_struct_gpu", ["ctx", "X", "B", Temp(COVER), D, N, M, H, "Kout", 0])],
                                {("lsq_update_codebooks_struct_gpu", 3): NCOVER}),
    "update_codebooks_struct[no cover]": (lambda e, P: e.update_codebooks_struct(P.X, P.B, None, M), ("Kout", None),
                                          [("lsq_update_codebooks_struct_gpu", ["ctx", "X", "B", None, D, N, M, H, "Kout", 0])]),
    "update_codebooks_spgl1": (lambda e, P: e.update_codebooks_spgl1(P.X, P.B, M, 2.5, K_init=P.K, S=9, opt_tol=0.5, max_iter=7), ("Kout", None),
                               [("lsq_update_codebooks_spgl1", ["ctx", "X", "B", D, N, M, H, 2.5, "K", 9, dict(opt_tol=0.5, max_iter=7), "Kout", "INFO"])]),
    "update_codebooks_spgl1[defaults]": (lambda e, P: e.update_codebooks_spgl1(P.X, P.B, M, 2.5), ("Kout", None),
                                         [("lsq_update_codebooks_spgl1", ["ctx", "X", "B", D, N, M, H, 2.5, None, -1, None, "Kout", "INFO"])]),
    "encode_viterbi": (lambda e, P: e.encode_viterbi(P.X, P.K, M), ("Bout",),
                       [("lsq_encode_viterbi", ["ctx", "X", "K", D, N, M, H, "Bout"])]),
    "assign_codewords": (lambda e, P: e.assign_codewords(P.X, P.K, M), ("Bout",),
                         [("lsq_assign_codewords", ["ctx", "X", "K", D, N, M, H, "Bout", None])]),
    "assign_codewords[min]": (lambda e, P: e.assign_codewords(P.X, P.K, M, want_min=True), ("Bout", "mv"),
                              [("lsq_assign_codewords", ["ctx", "X", "K", D, N, M, H, "Bout", "mv"])]),
    "update_centers": (lambda e, P: e.update_centers(P.X, P.B, P.cover, M, K_prev=P.K), ("Kout", "counts"),
                       [("lsq_update_centers", ["ctx", "X", "B", Temp(COVER), "K", D, N, M, H, "Kout", "counts"])], {("lsq_update_centers", 3): NCOVER}),
    "update_centers[no K_prev]": (lambda e, P: e.update_centers(P.X, P.B, P.cover, M), ("Kout", "counts"),
                                  [("lsq_update_centers", ["ctx", "X", "B", Temp(COVER), None, D, N, M, H, "Kout", "counts"])],
                                  {("lsq_update_centers", 3): NCOVER}),
    "kmeanspp_seed": (lambda e, P: e.kmeanspp_seed(P.X, P.cover, P.u, M), ("Kout", "idx", "d2"),
                      [("lsq_kmeanspp_seed", ["ctx", "X", Temp(COVER), "u", D, N, M, H, "Kout", "idx", "d2"])], {("lsq_kmeanspp_seed", 2): NCOVER}),
    "encoding_icm": (lambda e, P: e.encoding_icm(P.X, P.B, P.K, M, 6, True, 7, seed=11, global_offset=13), ("out",),
                     [("lsq_encoding_icm", ["ctx", "X", "B", "K", D, N, M, H, 6, 1, 7, 11, IT_AUTO, 13, "out"])]),
    "encoding_icm[it]": (lambda e, P: e.encoding_icm(P.X, P.B, P.K, M, 6, False, 7, seed=11, it=5), ("out",),
                         [("lsq_encoding_icm", ["ctx", "X", "B", "K", D, N, M, H, 6, 0, 7, 11, 5, 0, "out"])]),
    "encode_icm_fully": (lambda e, P: e.encode_icm_fully(P.B, P.X, P.K, M, 6, True, 7, idx_first=2, seed=11), ("B",),
                         [("lsq_encode_icm_fully", ["ctx", "B", "X", "K", D, N, M, H, 6, 1, 7, 2, 11, IT_AUTO])]),
    "get_unaries": (lambda e, P: e.get_unaries(P.X, P.K, M), ("U",), [("lsq_get_unaries", ["ctx", "X", "K", D, N, M, H, "U"])]),
    "get_binaries": (lambda e, P: e.get_binaries(P.K, M), ("T",), [("lsq_get_binaries", ["ctx", "K", D, M, H, "T"])]),
    "veccost": (lambda e, P: e.veccost(P.X, P.B, P.K, M), ("out",), [("lsq_veccost", ["ctx", "X", "B", "K", D, N, M, H, "out"])]),
    "qerror": (lambda e, P: e.qerror(P.X, P.B, P.K, M), (None,), [("lsq_qerror", ["ctx", "X", "B", "K", D, N, M, H, 0.0])]),
    "perturb": (lambda e, P: e.perturb(P.B, 7, seed=11, it=5, global_offset=13), ("Bout",), [("lsq_perturb", ["ctx", "Bout", N, M, H, 7, 11, 5, 13])]),
}

MULTI = {
    "encode_icm": (lambda e, P: e.encode_icm(P.X, P.B, P.K, M, P.ils, 6, 7, True, seed=11, nsplits=2, global_offset=13), ("Bs", "objs"),
                   [("lsq_multi_encode_icm", ["ctx", "X", "B", "K", D, N, M, H, "ils", 2, 6, 7, 1, 11, 13, 0, "Bs", "objs"])]),
    "encode_icm[u8]": (lambda e, P: e.encode_icm(P.X8, P.B, P.K, M, P.ils, 6, 7, True, seed=11, verbose=True), ("Bs", "objs"),
                       [("lsq_multi_encode_icm_u8", ["ctx", "X8", "B", "K", D, N, M, H, "ils", 2, 6, 7, 1, 11, 0, 1, "Bs", "objs"])]),
    "linscan": (lambda e, P: e.linscan(P.codes, P.Q, P.K, P.dbnorms, M, KK), ("dists", "ids"),
                [("lsq_multi_linscan", ["ctx", "dists", "ids", "codes", "Q", "K", "dbnorms", NQ, N, M, H, D, KK])]),
}


@pytest.fixture(scope="module")
def problem():
    return ec.Problem()


def _run(lsq, cls, problem, call, outputs, expected, peek=None):
    info = ec.zeros_of(lsq._lib.Spgl1Info)
    expected = [(s, [info if a == "INFO" and isinstance(a, str) else a for a in args]) for s, args in expected]
    ec.run_case(ec.offline_engine(lsq, cls, peek=peek), problem, call, outputs, expected)


@pytest.mark.parametrize("name", list(HOST))
def test_host_form_passes_what_it_was_given(lsq, problem, name):
    _run(lsq, "Engine", problem, *HOST[name])


@pytest.mark.parametrize("name", list(MULTI))
def test_multi_engine_passes_what_it_was_given(lsq, problem, name):
    _run(lsq, "MultiEngine", problem, *MULTI[name])


@pytest.mark.parametrize("u8", [False, True], ids=["f32 base", "uint8 base"])
def test_host_index_passes_what_it_was_given(lsq, problem, u8):
    """index() copies what it is given once (the index owns it): arrays already right are kept as they are, the base view becomes 70 tight rows"""
    P, eng = problem, ec.offline_engine(lsq)
    base, rows = ("base8", "Qrows8") if u8 else ("base", "Qrows")
    desc = dict(n=N, d=D, m=M, h=H, codes="codes", codebooks="K", dbnorms="dbnorms", base="base_copy", base_u8=int(u8), ldb=D, on_device=0)
    ix = ec.run_case(eng, P, lambda e, P: e.index(P.codes, P.K, P.dbnorms, M, base=getattr(P, base)), (None,),
                     [("lsq_index_create", ["index", "ctx", desc])], extra=lambda ix: {"base_copy": ix._keep[3]})
    assert ix._keep[3].flags["C_CONTIGUOUS"] and np.array_equal(ix._keep[3], getattr(P, base)) and (ix.n, ix.d, ix.m) == (N, D, M)
    ec.run_case(eng, P, lambda e, P: ix.search(P.Q, KK, L, P.Q2), ("dists", "ids"),
                [("lsq_index_search", ["index", "dists", "ids", "Q", "Q2", NQ, D, L, KK, 0])])
    ec.run_case(eng, P, lambda e, P: ix.search(P.Q, KK), ("dists", "ids"),
                [("lsq_index_search", ["index", "dists", "ids", "Q", "Q", NQ, D, 0, KK, 0])])
    ec.run_case(eng, P, lambda e, P: ix.rerank(P.Q, P.cand, KK, id_base=0), ("dists", "ids"),
                [("lsq_index_rerank", ["index", "dists", "ids", "Q", "cand", NQ, D, L, KK, 0, 0])])
    ec.run_case(eng, P, lambda e, P: ix.knn(getattr(P, rows), KK, id_base=1), ("dists", "ids"),       # row views are read in place
                [("lsq_index_knn", ["index", "dists", "ids", rows, int(u8), NQ, LDQ, KK, 1, 0])])
    ec.run_case(eng, P, lambda e, P: ix.close(), (None,), [("lsq_index_destroy", ["index"])])


# ---- the device forms refuse what they cannot read in place -----------------------------------------------------------------------------------------------
REFUSED_WITH = ("TypeError", "ValueError")


def _assert_refused(report):
    assert len(report) > 60
    for case, raised, reached in report:
        assert raised in REFUSED_WITH, "%s: %s" % (case, "accepted" if raised is None else "raised " + raised)
        assert reached == [], "%s reached the library: %s" % (case, reached)


def test_device_forms_refuse_cpu_tensors_wrong_types_and_strided_views(lsq):
    _assert_refused(ec.refusals())


def test_device_forms_refuse_the_same_under_python_O(lsq):
    """an `assert` vanishes under -O; a refusal must not"""
    p = subprocess.run([sys.executable, "-O", os.path.join(ec.ROOT, "tests", "engine_calls.py"), "--refusals"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["optimized"] is True
    _assert_refused(out["report"])
