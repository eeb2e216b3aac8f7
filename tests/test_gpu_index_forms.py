"""The forms of a call on a resident index (lsq_index_search, lsq_index_search_ivf, lsq_index_rerank, lsq_index_knn) and on an encoder that no other
test reaches: query rows more than d elements apart through the C ABI (the packing copy of q_scan, the as-they-lie extent of q_exact and q_coarse), the
device form that reads its queries in place and writes straight into the caller's outputs, timed calls against untimed ones (results, counts, every
*_ms field), and the text of every refusal the four entry points share."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
H = 256
N, D, M, NQ, NN, SHORT, NLIST, NPROBE = 300, 5, 2, 7, 4, 10, 4, 2
PAD = 3


class _Problem:
    """integer-valued f32 rows throughout: every exact distance is an integer below 2^24, nothing rounds"""

    def __init__(self):
        rng = np.random.default_rng(20)
        self.K = rng.integers(-3, 4, (M * H, D)).astype(np.float32)
        self.codes = rng.integers(0, H, (N, M)).astype(np.uint8)
        recon = sum(self.K[j * H + self.codes[:, j].astype(np.int64)] for j in range(M))
        self.dbn = (recon.astype(np.float64) ** 2).sum(1).astype(np.float32)
        self.Xb = (recon + rng.integers(-1, 2, (N, D))).astype(np.float32)
        self.Xb8 = rng.integers(0, 256, (N, D)).astype(np.uint8)
        pick = rng.integers(0, N, NQ)
        # three different query sets: a call that reads one in another's place gives other results
        self.Qs = (recon[pick] + rng.integers(-1, 2, (NQ, D))).astype(np.float32)
        self.Qe = (self.Xb[pick] + rng.integers(-2, 3, (NQ, D))).astype(np.float32)
        self.Qc = (self.Xb[rng.integers(0, N, NQ)] + rng.integers(-1, 2, (NQ, D))).astype(np.float32)
        self.Q8 = rng.integers(0, 256, (NQ, D)).astype(np.uint8)
        self.cent = np.ascontiguousarray(self.Xb[:NLIST] + np.float32(0.5))
        self.lor = ((self.Xb[:, None, :] - self.cent[None]) ** 2).sum(2).argmin(1).astype(np.int32)
        self.cand = rng.integers(1, N + 1, (NQ, SHORT)).astype(np.int32)
        self.Xe = rng.integers(-3, 4, (70, D)).astype(np.float32)


@pytest.fixture(scope="module")
def prob():
    return _Problem()


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _index(eng, p, dev, base="f32", codes=True):
    Xb = {"f32": p.Xb, "u8": p.Xb8, None: None}[base]
    cs = (p.codes, p.K, p.dbn) if codes else (None, None, None)
    if dev:
        ix = eng.index_dev(_dev(cs[0]), _dev(cs[1]), _dev(cs[2]), M if codes else 0, base=_dev(Xb), d=D)
    else:
        ix = eng.index(cs[0], cs[1], cs[2], M if codes else 0, base=Xb, d=D)
    if codes:
        ix.set_lists(_dev(p.cent) if dev else p.cent, _dev(p.lor) if dev else p.lor)
    return ix


def _strided(Q, ldq, dev):
    """the rows of Q ldq elements apart in a buffer of exactly (nq - 1) ldq + d elements, NaN between the rows"""
    nq, d = Q.shape
    buf = np.full((nq - 1) * ldq + d, np.nan, dtype=np.float32)
    for r in range(nq):
        buf[r * ldq:r * ldq + d] = Q[r]
    return _dev(buf) if dev else buf


def _raw(ix, sym, nq, args_of):
    """one C-ABI call on the index's own road -> (dists, ids) as numpy; args_of(p(dists), p(ids)) gives the arguments after the handle"""
    side = ix._side
    dists, ids = side.topk(nq, NN, "cuda:0")
    ix._eng._call(side, sym, *args_of(side.ptr(dists), side.ptr(ids)), h=ix._h)
    if ix._dev:
        import torch
        torch.cuda.synchronize()
        return dists.cpu().numpy(), ids.cpu().numpy()
    return dists, ids


def _calls(p, ix, nq, ldq, shortlist):
    """name -> (dists, ids) of every call that takes f32 query rows, the first nq queries ldq elements apart"""
    dev, on = ix._dev, int(ix._dev)
    q = {k: _strided(v[:nq], ldq, dev) for k, v in (("s", p.Qs), ("e", p.Qe), ("c", p.Qc))}
    cand = _dev(p.cand[:nq]) if dev else np.ascontiguousarray(p.cand[:nq])
    a = ix._side.ptr
    out = {
        "search": _raw(ix, "lsq_index_search", nq, lambda dd, di: (dd, di, a(q["s"]), a(q["e"]), nq, ldq, shortlist, NN, on)),
        "ivf-own-coarse": _raw(ix, "lsq_index_search_ivf", nq,
                               lambda dd, di: (dd, di, a(q["s"]), a(q["c"]), a(q["e"]), nq, ldq, NPROBE, shortlist, NN, 0, on)),
        "ivf-null-coarse": _raw(ix, "lsq_index_search_ivf", nq,
                                lambda dd, di: (dd, di, a(q["s"]), None, a(q["e"]), nq, ldq, NPROBE, shortlist, NN, 0, on)),
        "rerank": _raw(ix, "lsq_index_rerank", nq, lambda dd, di: (dd, di, a(q["e"]), a(cand), nq, ldq, SHORT, NN, 1, on)),
    }
    return out


def _same(got, want, what):
    for name in want:
        for g, w in zip(got[name], want[name]):
            assert g.tobytes() == w.tobytes(), (what, name)


@pytest.mark.parametrize("shortlist", [0, SHORT])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_strided_queries_equal_packed_ones(engine, prob, dev, shortlist):
    with _index(engine, prob, dev) as ix:
        want = _calls(prob, ix, NQ, D, shortlist)
        assert not np.isnan(want["search"][0]).any() and not np.array_equal(want["ivf-own-coarse"][1], want["ivf-null-coarse"][1])
        _same(_calls(prob, ix, NQ, D + PAD, shortlist), want, (dev, shortlist))


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_one_strided_query(engine, prob, dev):
    """nq = 1, ldq = d + 3: the buffer holds d elements"""
    with _index(engine, prob, dev) as ix:
        for shortlist in (0, SHORT):
            _same(_calls(prob, ix, 1, D + PAD, shortlist), _calls(prob, ix, 1, D, shortlist), (dev, shortlist))


def test_device_form_writes_only_its_outputs(engine, prob):
    """ldq == d on a borrowed-device index: the query rows are read where they lie and the results go straight into the caller's tensors -- nothing past
    their nq nn entries is written and the queries are left as they were"""
    import torch
    p, tail = prob, 64
    with _index(engine, p, True) as ix, _index(engine, p, True, base="u8", codes=False) as ix8:
        qs, qe, qc, q8, cand = _dev(p.Qs), _dev(p.Qe), _dev(p.Qc), _dev(p.Q8), _dev(p.cand)
        a = lambda t: t.data_ptr()      # noqa: E731
        calls = {
            "search0": (ix, "lsq_index_search", lambda dd, di: (dd, di, a(qs), None, NQ, D, 0, NN, 1)),
            "search": (ix, "lsq_index_search", lambda dd, di: (dd, di, a(qs), a(qe), NQ, D, SHORT, NN, 1)),
            "ivf": (ix, "lsq_index_search_ivf", lambda dd, di: (dd, di, a(qs), a(qc), a(qe), NQ, D, NPROBE, SHORT, NN, 0, 1)),
            "rerank": (ix, "lsq_index_rerank", lambda dd, di: (dd, di, a(qe), a(cand), NQ, D, SHORT, NN, 1, 1)),
            "knn": (ix, "lsq_index_knn", lambda dd, di: (dd, di, a(qe), 0, NQ, D, NN, 0, 1)),
            "knn-u8": (ix8, "lsq_index_knn", lambda dd, di: (dd, di, a(q8), 1, NQ, D, NN, 0, 1)),
        }
        inputs = (qs, qe, qc, q8, cand)
        before = [t.clone() for t in inputs]
        for name, (index, sym, args_of) in calls.items():
            dd = torch.full((NQ * NN + tail,), -7.5, dtype=torch.float32, device="cuda")
            di = torch.full((NQ * NN + tail,), -77, dtype=torch.int32, device="cuda")
            index._eng._call(index._side, sym, *args_of(dd.data_ptr(), di.data_ptr()), h=index._h)
            torch.cuda.synchronize()
            assert bool((dd[NQ * NN:] == -7.5).all()) and bool((di[NQ * NN:] == -77).all()), name
            assert bool((di[:NQ * NN] != -77).all()), name
            for t, b in zip(inputs, before):
                assert torch.equal(t, b), name


# ---- timed equals untimed ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def timed_engine(lsq):
    eng = lsq.Engine(0, profile=True)
    yield eng
    eng.close()


def _split(info):
    return {k: v for k, v in info.items() if not k.endswith("_ms")}, {k: v for k, v in info.items() if k.endswith("_ms")}


def _ms_ok(ms, timed, what):
    for k, v in ms.items():
        assert (np.isfinite(v) and v >= 0) if timed else v == 0.0, (what, k, v, timed)


def _index_ops(p):
    """name -> (base of its index, f(ix) -> (results, the info that describes the call))"""
    return {
        "search": ("f32", lambda ix: (ix.search(p.Qs, NN, shortlist=SHORT, Q_exact=p.Qe), ix.stats())),
        "ivf-thresholded": ("f32", lambda ix: (ix.search_ivf(p.Qs, NN, NPROBE, shortlist=SHORT, Q_coarse=p.Qc, Q_exact=p.Qe), ix.ivf_info())),
        "ivf-every-record": ("f32", lambda ix: (ix.search_ivf(p.Qs, NN, NPROBE, shortlist=SHORT, Q_coarse=p.Qc, Q_exact=p.Qe, every_record=True),
                                                ix.ivf_info())),
        "rerank": ("f32", lambda ix: (ix.rerank(p.Qe, p.cand, NN), ix.stats())),
        "knn-int": ("u8", lambda ix: (ix.knn(p.Q8, NN), ix.knn_info())),
        "knn-f32": ("f32", lambda ix: (ix.knn(p.Qe, NN), ix.knn_info())),
    }


@pytest.mark.parametrize("name", ["search", "ivf-thresholded", "ivf-every-record", "rerank", "knn-int", "knn-f32"])
def test_timed_index_calls_equal_untimed_ones(engine, timed_engine, prob, name):
    base, op = _index_ops(prob)[name]
    got = {}
    for timed, eng in ((False, engine), (True, timed_engine)):
        with _index(eng, prob, False, base=base, codes=base == "f32") as ix:
            res, info = op(ix)
            got[timed] = (res, _split(info)[0], _split(ix.stats())[0])
            _ms_ok(_split(info)[1], timed, name)
            _ms_ok(_split(ix.stats())[1], timed, name)
            if name == "ivf-thresholded":
                assert info["threshold_queries"] + info["fallback_queries"] == NQ
            if name == "ivf-every-record":
                assert info["threshold_queries"] + info["fallback_queries"] == 0
            if name.startswith("knn"):
                assert info["int_road"] == (1 if name == "knn-int" else 0)
                assert (info["norms_ms"] > 0) if (timed and name == "knn-int") else info["norms_ms"] == 0.0
            # a second call: the index's stats accumulate, the ivf and knn infos describe the last call alone
            first, first_stats = info, ix.stats()
            res2, info2 = op(ix)
            for a, b in zip(res, res2):
                assert a.tobytes() == b.tobytes()
            st = ix.stats()
            assert st["queries"] == 2 * NQ and st["gather_ms"] >= first_stats["gather_ms"] and st["select_ms"] >= first_stats["select_ms"]
            assert st["scan_ms"] >= first_stats["scan_ms"]
            _ms_ok(_split(st)[1], timed, name)
            if name in ("search", "rerank"):
                assert st["batches"] == 2 * first_stats["batches"] == 2 and st["rows"] == 2 * first_stats["rows"]
            else:
                assert _split(info2)[0] == _split(first)[0] and info2["queries"] == NQ
                _ms_ok(_split(info2)[1], timed, name)
    (r0, i0, s0), (r1, i1, s1) = got[False], got[True]
    for a, b in zip(r0, r1):
        assert a.tobytes() == b.tobytes(), name
    assert i0 == i1 and s0 == s1, name


@pytest.mark.parametrize("L", [1, 3])
def test_timed_beam_equals_untimed(engine, timed_engine, prob, L):
    got = {}
    for timed, eng in ((False, engine), (True, timed_engine)):
        with eng.encoder(prob.K, M, chunk=32) as enc:                           # 70 vectors: three chunks
            codes, score = enc.beam(prob.Xe, L, want_score=True)
            info = enc.info()
            got[timed] = (codes, score, _split(info)[0])
            _ms_ok(_split(info)[1], timed, L)
            assert info["chunks"] == 3 and info["vectors"] == 70 and set(_split(info)[1]) == {"unaries_ms", "beam_ms"}
    assert got[False][0].tobytes() == got[True][0].tobytes() and got[False][1].tobytes() == got[True][1].tobytes() and got[False][2] == got[True][2]


# ---- the refusals the entry points share, word for word ---------------------------------------------------------------------------------------

def test_shared_refusals_keep_their_words(lsq, engine, prob):
    L, EINVAL, p = lsq._lib.load(), lsq._lib.LSQ_EINVAL, prob
    dd, di = np.full((NQ, NN), -7.5, np.float32), np.full((NQ, NN), -77, np.int32)
    qs, qe, cand = p.Qs.ctypes.data, p.Qe.ctypes.data, p.cand.ctypes.data

    def search(h, dists=dd.ctypes.data, ids=di.ctypes.data, q_scan=qs, q_exact=qe, nq=NQ, ldq=D, shortlist=0, nn=NN):
        return L.lsq_index_search(h, dists, ids, q_scan, q_exact, nq, ldq, shortlist, nn, 0)

    def ivf(h, dists=dd.ctypes.data, ids=di.ctypes.data, q_scan=qs, q_exact=qe, nq=NQ, ldq=D, shortlist=0, nn=NN):
        return L.lsq_index_search_ivf(h, dists, ids, q_scan, None, q_exact, nq, ldq, NPROBE, shortlist, nn, 0, 0)

    def rerank(h, dists=dd.ctypes.data, ids=di.ctypes.data, nq=NQ, ldq=D, nn=NN):
        return L.lsq_index_rerank(h, dists, ids, qe, cand, nq, ldq, SHORT, nn, 1, 0)

    def knn(h, dists=dd.ctypes.data, ids=di.ctypes.data, q=qe, nq=NQ, ldq=D, nn=NN):
        return L.lsq_index_knn(h, dists, ids, q, 0, nq, ldq, nn, 0, 0)

    shape = "needs nq >= 0, nn >= 1, ldq >= d (got nq=%d nn=%d ldq=%d d=5)"
    big = (1 << 28) + 1
    with _index(engine, p, False) as full, _index(engine, p, False, base=None) as scan_only, _index(engine, p, False, codes=False) as base_only:
        H_ = {"full": full._h, "scan_only": scan_only._h, "base_only": base_only._h, None: None}
        cases = []
        for fn, f in (("lsq_index_search", search), ("lsq_index_search_ivf", ivf), ("lsq_index_rerank", rerank)):
            cases += [
                (f, None, {}, fn + ": null index"),
                (f, "full", dict(nq=-1), fn + ": " + shape % (-1, NN, D)),
                (f, "full", dict(nn=0), fn + ": " + shape % (NQ, 0, D)),
                (f, "full", dict(ldq=D - 1), fn + ": " + shape % (NQ, NN, D - 1)),
                (f, "full", dict(dists=None), fn + ": null pointer"),
                (f, "full", dict(ids=None), fn + ": null pointer"),
            ]
        for fn, f in (("lsq_index_search", search), ("lsq_index_search_ivf", ivf)):
            cases += [
                (f, "base_only", {}, fn + ": the index holds no codes"),
                (f, "full", dict(shortlist=NN - 1), fn + ": needs shortlist == 0 or shortlist >= nn (got shortlist=%d nn=%d)" % (NN - 1, NN)),
                (f, "full", dict(shortlist=-1), fn + ": needs shortlist == 0 or shortlist >= nn (got shortlist=-1 nn=%d)" % NN),
                (f, "scan_only", dict(shortlist=SHORT), fn + ": a shortlist needs base rows, the index holds none"),
                (f, "full", dict(q_scan=None), fn + ": null pointer"),
                (f, "full", dict(shortlist=SHORT, q_exact=None), fn + ": null pointer"),
            ]
        cases += [
            (search, "full", dict(shortlist=N + 1), "lsq_index_search: shortlist=%d exceeds the database size %d" % (N + 1, N)),
            (search, "full", dict(nn=N + 1), "lsq_index_search: nn=%d exceeds the database size %d" % (N + 1, N)),
            (search, "full", dict(shortlist=big), "lsq_index_search: shortlist=%d exceeds the database size %d" % (big, N)),      # (n <= 2^28: this one first)
            (ivf, "full", dict(shortlist=big), "lsq_index_search_ivf: needs nn and shortlist <= 2^28 (got %d)" % big),
            (ivf, "full", dict(nn=big), "lsq_index_search_ivf: needs nn and shortlist <= 2^28 (got %d)" % big),
            (rerank, "scan_only", {}, "lsq_index_rerank: the index holds no base rows"),
            (knn, None, {}, "lsq_index_knn: null index"),
            (knn, "scan_only", {}, "lsq_index_knn: the index holds no base rows"),
            (knn, "full", dict(dists=None), "lsq_index_knn: null pointer"),
            (knn, "full", dict(ids=None), "lsq_index_knn: null pointer"),
            (knn, "full", dict(q=None), "lsq_index_knn: null pointer"),
            (knn, "full", dict(nq=0), "lsq_index_knn: needs nq >= 1 and ldq >= d (got nq=0 ldq=5 d=5)"),
            (knn, "full", dict(ldq=D - 1), "lsq_index_knn: needs nq >= 1 and ldq >= d (got nq=7 ldq=4 d=5)"),
            (knn, "full", dict(nn=0), "lsq_index_knn: needs 1 <= nn <= n (got nn=0 n=300)"),
        ]
        before = [ix.stats() for ix in (full, scan_only, base_only)]
        for f, which, kw, words in cases:
            assert f(H_[which], **kw) == EINVAL, words
            said = L.lsq_last_error().decode()
            assert said == words, (said, words)
            assert said.startswith(words.split(":")[0] + ": ")
            assert bool((dd == -7.5).all()) and bool((di == -77).all()), words
        assert [ix.stats() for ix in (full, scan_only, base_only)] == before and before[0]["queries"] == 0
        # ... and the calls these were the refusals of do run
        assert search(full._h) == 0 and search(full._h, shortlist=SHORT) == 0 and ivf(full._h, shortlist=SHORT) == 0 and rerank(full._h) == 0
        assert knn(full._h) == 0 and full.stats()["queries"] == 5 * NQ and not (di == -77).any()
