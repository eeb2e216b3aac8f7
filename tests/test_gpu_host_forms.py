"""Three contracts of the host-buffer entry points that are neither the pipelined encode nor a search (csrc/lsq_api.hip, "host-buffer calls"): each of
them is stage -> its pair's core -> fetch -> one wait, and what the staging promises is pinned here per entry:

  1. a bad code (0, or h + 1) is found while the codes are staged: LSQ_ECODE, no output touched, and the same context then computes what a fresh one does;
  2. n == 0 returns what it always returned and leaves the outputs as it always left them;
  3. a host form and its _dev twin agree bit for bit, on a context of chunk 64 (the initialisers walk three chunks, the last of one row) and on a default one.

The shapes are the smallest at which the staging can go wrong: n = 129 (one row past two 64-lane waves and past a 128-row tile), d = 7 (odd), m = 3
(record stride 8, five padding bytes) and m = 9 (record stride 16); the codebook updates run at the smallest shapes of their own solvers' catalogue
entries (ctx_ops.SPG_SHAPES[0], ctx_ops.CHAIN_SHAPES[1])."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctx_ops as ops  # noqa: E402

pytestmark = pytest.mark.gpu
H = 256
N, D = 129, 7
OK, EINVAL, ECODE = 0, -1, -4


def _p(a):
    return None if a is None else a.ctypes.data


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, want, what):
    assert len(got) == len(want), what
    for q, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, "%s: output %d is %s%s vs %s%s" % (what, q, a.dtype, a.shape, b.dtype, b.shape)
        assert np.array_equal(_bits(a), _bits(b)), "%s: output %d differs in %d of %d elements" % (what, q, int((_bits(a) != _bits(b)).sum()), a.size)


def _cover(d, m):
    """(d, m) 0/1: codebook j covers the two adjacent dimensions from j mod (d - 1) on -- contiguous, overlapping, valid for m > d"""
    cover = np.zeros((d, m), dtype=np.uint8)
    for j in range(m):
        cover[j % (d - 1):j % (d - 1) + 2, j] = 1
    return cover


@functools.lru_cache(maxsize=None)
def _inputs(kind, m):
    lsq = ops.lsq_pkg()
    if kind == "piece":
        rng = np.random.default_rng(100 + m)
        n, d = N, D
        K = (rng.standard_normal((m * H, d)) / m).astype(np.float32)
        codes = rng.integers(0, H, size=(n, m)).astype(np.uint8)
        rec = sum(K[j * H + codes[:, j].astype(np.int64)] for j in range(m))
        inp = {"X": rng.standard_normal((n, d)).astype(np.float32), "K": K, "codes": codes,
               "cb": np.sort((rec.astype(np.float64) ** 2).sum(1))[::2].astype(np.float32), "cover": _cover(d, m),
               "K_prev": rng.standard_normal((m * H, d)).astype(np.float32), "u": rng.random((m, H))}
    elif kind == "chain":
        import chain_cases as cc
        n, d, m = ops.CHAIN_SHAPES[1]
        X, codes, od = cc.chain_problem(d, n, m)
        inp = {"X": X, "codes": codes.astype(np.uint8), "cover": cc.cover_of(od, d, m)}
    else:
        inp = dict(ops._spg_make(*ops.SPG_SHAPES[0], seed=7))
        n, d, m = ops.SPG_SHAPES[0]
        inp["K_init"] = (np.random.default_rng(3).standard_normal((m * H, d)) * 0.01).astype(np.float32)
    inp.update(n=n, d=d, m=m, B=inp["codes"].astype(np.int16) + 1)
    if "cover" in inp:
        inp["cover_bytes"] = lsq.engine.cover_bytes(inp["cover"], d, m)
    return inp


# ---- the raw symbols: call(eng, inp, B, n) -> (return code, the output buffers as they are after the call); every buffer starts as a sentinel ---------------
def _f32(shape, v=1234.5):
    return np.full(shape, v, dtype=np.float32)


def _fully(e, i, B, n):
    out = B.copy()
    return e._L.lsq_encode_icm_fully(e._h, _p(out), _p(i["X"]), _p(i["K"]), i["d"], n, i["m"], H, 2, 1, 2, 5, 11, 3), [out]


def _get_unaries(e, i, B, n):
    U = _f32((i["m"], i["n"], H))
    return e._L.lsq_get_unaries(e._h, _p(i["X"]), _p(i["K"]), i["d"], n, i["m"], H, _p(U)), [U]


def _veccost(e, i, B, n):
    out = _f32(i["n"])
    return e._L.lsq_veccost(e._h, _p(i["X"]), _p(B), _p(i["K"]), i["d"], n, i["m"], H, _p(out)), [out]


def _qerror(e, i, B, n):
    out = C.c_double(7.0)
    rc = e._L.lsq_qerror(e._h, _p(i["X"]), _p(B), _p(i["K"]), i["d"], n, i["m"], H, C.byref(out))
    return rc, [np.array([out.value])]


def _perturb(e, i, B, n):
    out = B.copy()
    return e._L.lsq_perturb(e._h, _p(out), n, i["m"], H, 2, 11, 3, 1000), [out]


def _quantize_norms(e, i, B, n):
    idx, dbn, nrm = np.full(i["n"], -77, dtype=np.int16), _f32(i["n"]), _f32(i["n"])
    rc = e._L.lsq_quantize_norms(e._h, _p(B), _p(i["K"]), _p(i["cb"]), i["cb"].shape[0], i["d"], n, i["m"], H, _p(idx), _p(dbn), _p(nrm))
    return rc, [idx, dbn, nrm]


def _update_gpu(e, i, B, n):
    K, it = _f32((i["m"] * H, i["d"])), C.c_int(-9)
    rc = e._L.lsq_update_codebooks_gpu(e._h, _p(i["X"]), _p(B), i["d"], n, i["m"], H, _p(K), C.byref(it))
    return rc, [K, np.array([it.value])]


def _update_struct(e, i, B, n):
    K, it = _f32((i["m"] * H, i["d"])), C.c_int(-9)
    rc = e._L.lsq_update_codebooks_struct_gpu(e._h, _p(i["X"]), _p(B), _p(i["cover_bytes"]), i["d"], n, i["m"], H, _p(K), C.byref(it))
    return rc, [K, np.array([it.value])]


def _info(info):
    return [np.array([getattr(info, k) for k in ops.INFO_INT], dtype=np.int64), np.array([getattr(info, k) for k in ops.INFO_F64], dtype=np.float64)]


def _update_spgl1(e, i, B, n):
    lib = ops.lsq_pkg()._lib
    K, info, p = _f32((i["m"] * H, i["d"])), lib.Spgl1Info(), lib.Spgl1Params(0.0, ops.SPG_MAXIT)
    info.status, info.iterations, info.f = -9, -9, 1234.5
    rc = e._L.lsq_update_codebooks_spgl1(e._h, _p(i["X"]), _p(B), i["d"], n, i["m"], H, float(i["tau"]), _p(i["K_init"]), -1, C.byref(p), _p(K), C.byref(info))
    return rc, [K] + _info(info)


def _viterbi(e, i, B, n):
    out = np.full((i["n"], i["m"]), -77, dtype=np.int16)
    return e._L.lsq_encode_viterbi(e._h, _p(i["X"]), _p(i["K"]), i["d"], n, i["m"], H, _p(out)), [out]


def _assign(e, i, B, n):
    out, mv = np.full((i["n"], i["m"]), -77, dtype=np.int16), _f32((i["n"], i["m"]))
    return e._L.lsq_assign_codewords(e._h, _p(i["X"]), _p(i["K"]), i["d"], n, i["m"], H, _p(out), _p(mv)), [out, mv]


def _centers(e, i, B, n):
    K, cnt = _f32((i["m"] * H, i["d"])), np.full(i["m"] * H, -77, dtype=np.int32)
    rc = e._L.lsq_update_centers(e._h, _p(i["X"]), _p(B), _p(i["cover_bytes"]), _p(i["K_prev"]), i["d"], n, i["m"], H, _p(K), _p(cnt))
    return rc, [K, cnt]


def _seed(e, i, B, n):
    K, idx, d2 = _f32((i["m"] * H, i["d"])), np.full((i["m"], H), -77, dtype=np.int64), _f32((i["n"], i["m"]))
    rc = e._L.lsq_kmeanspp_seed(e._h, _p(i["X"]), _p(i["cover_bytes"]), _p(i["u"]), i["d"], n, i["m"], H, _p(K), _p(idx), _p(d2))
    return rc, [K, idx, d2]


def _sentinels(call, inp):
    """the output buffers of `call` as they stand before it runs"""
    class Nothing:
        def __getattr__(self, name):
            return lambda *a: OK
    e = type("E", (), {"_L": Nothing(), "_h": None})()
    return call(e, inp, inp["B"], inp["n"])[1]


def _err(eng):
    return eng._L.lsq_last_error().decode()


TAKES_CODES = [("encode_icm_fully", _fully, "piece"), ("veccost", _veccost, "piece"), ("qerror", _qerror, "piece"), ("perturb", _perturb, "piece"),
               ("quantize_norms", _quantize_norms, "piece"), ("update_centers", _centers, "piece"), ("update_codebooks_gpu", _update_gpu, "chain"),
               ("update_codebooks_struct_gpu", _update_struct, "chain"), ("update_codebooks_spgl1", _update_spgl1, "spg")]
NO_CODES = [("get_unaries", _get_unaries, "piece"), ("encode_viterbi", _viterbi, "piece"), ("assign_codewords", _assign, "piece"),
            ("kmeanspp_seed", _seed, "piece")]


def _cases(entries):
    return [pytest.param(call, kind, m, id="%s-m%d" % (name, m)) for name, call, kind in entries for m in ((3, 9) if kind == "piece" else (0,))]


@pytest.fixture(scope="module")
def engines(lsq):
    """the two long-lived contexts every case of this file shares: whatever a case leaves in the staging buffers, the next one finds"""
    with lsq.Engine(0, chunk=64) as small, lsq.Engine(0) as default:
        yield {"chunk64": small, "default": default}


_fresh = {}


def _fresh_result(lsq, call, kind, m):
    if (call, m) not in _fresh:
        inp = _inputs(kind, m)
        with lsq.Engine(0) as e:
            _fresh[(call, m)] = call(e, inp, inp["B"], inp["n"])
        assert _fresh[(call, m)][0] == OK, _err(e)
    return _fresh[(call, m)]


# ---- 1. a bad code never touches an output ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["zero_in_first_row", "h_plus_1_in_last_row"])
@pytest.mark.parametrize("call,kind,m", _cases(TAKES_CODES))
def test_a_bad_code_touches_no_output_and_leaves_nothing_behind(lsq, engines, call, kind, m, where):
    inp, eng = _inputs(kind, m), engines["default"]
    bad = inp["B"].copy()
    if where == "zero_in_first_row":
        bad[0, inp["m"] - 1] = 0
    else:
        bad[-1, 0] = H + 1
    want = _sentinels(call, inp)
    if call in (_fully, _perturb):
        want = [bad.copy()]                                # in place: B itself is unchanged
    if call is _qerror:
        want = [np.array([0.0])]                           # zeroed before anything is staged
    rc, outs = call(eng, inp, bad, inp["n"])
    assert rc == ECODE and "1..256" in _err(eng), (rc, _err(eng))
    _same(outs, want, "outputs after the rejected call")
    rc, outs = call(eng, inp, inp["B"], inp["n"])
    assert rc == OK, _err(eng)
    _same(outs, _fresh_result(lsq, call, kind, m)[1], "valid call after the rejected one vs a fresh context")


# ---- 2. n == 0 -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call,kind,m", _cases(TAKES_CODES + NO_CODES))
def test_an_empty_call_returns_and_leaves_what_it_always_did(engines, call, kind, m):
    inp = _inputs(kind, m)
    want_rc, want = OK, _sentinels(call, inp)
    if call is _qerror:
        want = [np.array([0.0])]
    elif call in (_update_gpu, _update_struct, _update_spgl1):
        want_rc = EINVAL
    elif call is _seed:                                    # no row to choose: zero codebooks, indices -1, d2 empty
        want = [np.zeros_like(want[0]), np.full_like(want[1], -1), want[2]]
    elif call is _centers:                                 # every cluster is empty: it keeps its row of K_prev inside the cover, exact zeros outside
        keep = np.repeat(inp["cover"].T.astype(bool), H, axis=0)
        want = [np.where(keep, inp["K_prev"], np.float32(0)), np.zeros_like(want[1])]
    for name, eng in engines.items():
        rc, outs = call(eng, inp, inp["B"], 0)
        assert rc == want_rc, (name, rc, _err(eng))
        _same(outs, want, "outputs of the empty call on the %s context" % name)


# ---- 3. a host form equals its _dev twin ---------------------------------------------------------------------------------------------------------------------
def _np_dev(ts):
    import torch
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in ts]


def _pair_norms(e, i):
    dev = _np_dev(e.quantize_norms_dev(ops.dev(i["codes"]), ops.dev(i["K"]), ops.dev(i["cb"]), i["m"]))
    return list(e.quantize_norms(i["B"], i["K"], i["cb"], i["m"])), [dev[0].astype(np.int16) + 1, dev[1], dev[2]]


def _pair_update(e, i):
    K, it = e.update_codebooks(i["X"], i["B"], i["m"])
    dK, dit = e.update_codebooks_dev(ops.dev(i["X"]), ops.dev(i["codes"]), i["m"])
    return [K, np.array([it])], _np_dev([dK]) + [np.array([dit])]


def _pair_struct(e, i):
    K, it = e.update_codebooks_struct(i["X"], i["B"], i["cover"], i["m"])
    dK, dit = e.update_codebooks_struct_dev(ops.dev(i["X"]), ops.dev(i["codes"]), ops.dev(i["cover"]), i["m"])
    return [K, np.array([it])], _np_dev([dK]) + [np.array([dit])]


def _pair_spgl1(e, i):
    K, info = e.update_codebooks_spgl1(i["X"], i["B"], i["m"], i["tau"], K_init=i["K_init"], max_iter=ops.SPG_MAXIT)
    dK, dinfo = e.update_codebooks_spgl1_dev(ops.dev(i["X"]), ops.dev(i["codes"]), i["m"], i["tau"], dK_init=ops.dev(i["K_init"]), max_iter=ops.SPG_MAXIT)
    return [K] + list(ops._info_arrays(info)), _np_dev([dK]) + list(ops._info_arrays(dinfo))


def _pair_viterbi(e, i):
    return [e.encode_viterbi(i["X"], i["K"], i["m"])], [_np_dev([e.encode_viterbi_dev(ops.dev(i["X"]), ops.dev(i["K"]), i["m"])])[0].astype(np.int16) + 1]


def _pair_assign(e, i):
    dB, dmin = _np_dev(e.assign_codewords_dev(ops.dev(i["X"]), ops.dev(i["K"]), i["m"], want_min=True))
    return list(e.assign_codewords(i["X"], i["K"], i["m"], want_min=True)), [dB.astype(np.int16) + 1, dmin]


def _pair_centers(with_prev):
    def pair(e, i):
        Kp = i["K_prev"] if with_prev else None
        dev = _np_dev(e.update_centers_dev(ops.dev(i["X"]), ops.dev(i["codes"]), i["cover"], i["m"], K_prev=None if Kp is None else ops.dev(Kp)))
        return list(e.update_centers(i["X"], i["B"], i["cover"], i["m"], K_prev=Kp)), dev
    return pair


def _pair_seed(e, i):
    dev = _np_dev(e.kmeanspp_seed_dev(ops.dev(i["X"]), i["cover"], i["u"], i["m"], want_idx=True, want_d2=True))
    return list(e.kmeanspp_seed(i["X"], i["cover"], i["u"], i["m"])), dev


PAIRS = [("quantize_norms", _pair_norms, "piece"), ("update_codebooks", _pair_update, "chain"), ("update_codebooks_struct", _pair_struct, "chain"),
         ("update_codebooks_spgl1", _pair_spgl1, "spg"), ("encode_viterbi", _pair_viterbi, "piece"), ("assign_codewords", _pair_assign, "piece"),
         ("update_centers_prev", _pair_centers(True), "piece"), ("update_centers_zero", _pair_centers(False), "piece"), ("kmeanspp_seed", _pair_seed, "piece")]


@pytest.mark.parametrize("pair,kind,m", _cases(PAIRS))
def test_a_host_form_equals_its_dev_twin_bit_for_bit(engines, pair, kind, m):
    inp, first = _inputs(kind, m), None
    for name, eng in engines.items():
        host, dev = pair(eng, inp)
        _same(host, dev, "host form vs _dev twin on the %s context" % name)
        if first is None:
            first = host
        _same(host, first, "the %s context vs the chunk64 one" % name)
