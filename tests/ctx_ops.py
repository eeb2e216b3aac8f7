"""The alphabet of the context walk (tests/test_gpu_ctx_state.py): one entry per device entry point reachable through Engine, host-buffer and _dev forms
apart, plus the moves that change nothing but the context's state (options, the bound stream, a rejected call, reset_timings) -- and the driver that
walks one long-lived Engine through a sequence of them, holding every step to the same entry on a fresh Engine.

Nothing here touches a GPU at import.  Each Op has
    variants            >= 3 seeded inputs that differ in n, d and m (small / large / odd), so that the shared work buffers grow and shrink between visits;
                        the encodes' large one is 70 001 x 32 (>= q16_min: the filtered walk, its verdict and its probe run on default options)
    run(engine, inp)    -> tuple of numpy arrays: the results, then the call's deltas of the path counters of timings() (COUNTERS; no millisecond field, no
                        table_reuses), then -- the scans -- the integer fields of linscan_stats()
    check(inp, out)     holds a result to the checker the entry point already has (oracle, f64ref, knn_check, kmeans_check, spgl1_check, init_oracle): the
                        baseline of the walk is never merely the code agreeing with itself.  No reference is written here.
"""
import ctypes as C
import importlib
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

H = 256
EINVAL = -1
COUNTERS = ("icm_launches", "icm_node_updates", "staged_blocks", "light_blocks", "filtered_blocks", "filter_refined", "filter_exact", "filter_f32",
            "filter_fallback_chunks")
SCAN_SUMS = ("queries", "candidates", "fallback_queries", "batches")                  # accumulated by every scan: the call's delta
SCAN_LAST = ("codes", "exhaustive", "threshold_rank", "list_capacity")                # describe the last scan: as they stand after the call
ERR = np.dtype([("lsq_error", np.int64)])                                              # a call that failed: its return code is the (deterministic) result

# ---- option profiles: an option move sets ONE of them (every other option back to its default first), so a later move restores it ------------------------
CHUNK_SMALL = 4096
OPTION_DEFAULTS = {"schedule": 6, "chunk": 256 * 3968, "q16_min": 65536, "light": -1, "filter_probe_div": 8, "filter_fallback_div": 64, "profile": 0}


def _forced():
    from conftest import ENCODE_VARIANTS
    return dict(next(v for v in ENCODE_VARIANTS if v.id == "s6_forced").values[0])


def profiles():
    return {"default": {}, "s4": {"schedule": 4}, "s3": {"schedule": 3}, "chunk_small": {"chunk": CHUNK_SMALL}, "s6_forced": _forced(),
            "profile1": {"profile": 1}}


PROFILE_NAMES = ("default", "s4", "s3", "chunk_small", "s6_forced", "profile1")


def apply_profile(eng, name):
    opts = dict(OPTION_DEFAULTS)
    opts.update(profiles()[name])
    for k, v in opts.items():
        eng.set_option(k, v)


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------------------------
def lsq_pkg():
    return importlib.import_module("local-search-quantization_amd")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rows(n, extra=24, seed=0):
    r = {0, n - 1, n // 2} | {i for i in (126, 127, 128, 129, 255, 256, 4095, 4096) if i < n}
    r |= set(np.random.default_rng(seed).choice(n, size=min(n, extra), replace=False).tolist())
    return np.array(sorted(r))


def _blocks(n):
    """the row ranges of a large encode that the oracle re-encodes at their global indices (results depend on (vector, global index) only)"""
    return [(0, n)] if n <= 20_000 else [(0, 256), (n // 2 - 128, n // 2 + 128), (n - 256, n)]


def is_error(out):
    return out[0].dtype == ERR


class Op:
    kind = "op"

    def __init__(self, name, symbols, shapes, make, call, check, dev=False, scan=False, auto=False, encode=False, fixed=False):
        if fixed:                                          # the mutant sequence: one shape, three seeds
            shapes = [FIXED] * 3
        else:
            assert len(shapes) >= 3 and len({s[0] for s in shapes}) >= 3 and len({s[1] for s in shapes}) >= 3 and len({s[2] for s in shapes}) >= 3, name
        self.name, self.symbols, self.shapes, self._make, self._call, self._check = name, tuple(symbols), list(shapes), make, call, check
        self.dev, self.scan, self.auto, self.encode = dev, scan, auto, encode

    def make(self, v):
        inp = self._make(*self.shapes[v], seed=1000 * (sum(map(ord, self.name)) % 997) + v)
        inp["shape"] = self.shapes[v]
        return inp

    def run(self, eng, inp):
        import torch
        LsqError = lsq_pkg()._lib.LsqError
        t0 = eng.timings()
        s0 = eng.linscan_stats() if self.scan else None
        try:
            out = tuple(np.asarray(o) for o in self._call(eng, inp))
        except LsqError as e:
            out = (np.array([(e.code,)], dtype=ERR),)
        torch.cuda.synchronize()
        t1 = eng.timings()
        out += (np.array([t1[k] - t0[k] for k in COUNTERS], dtype=np.int64),)
        if self.scan:
            s1 = eng.linscan_stats()
            out += (np.array([s1[k] - s0[k] for k in SCAN_SUMS] + [s1[k] for k in SCAN_LAST], dtype=np.int64),)
        return out

    def check(self, inp, out, profile="default"):
        if is_error(out):
            # the one legal failure of the walk: the worker keeps its vectors in ONE resident chunk
            assert self.name.startswith("encode_icm_fully") and profile == "chunk_small" and inp["shape"][0] > CHUNK_SMALL and out[0][0][0] == EINVAL, \
                "%s failed with %r under profile %s" % (self.name, out[0], profile)
            return
        self._check(inp, out)


class Move:
    """a step that changes nothing but the context's state"""
    kind = "move"

    def __init__(self, name, symbols):
        self.name, self.symbols = name, tuple(symbols)
        self.dev = self.scan = self.auto = self.encode = False


# ---- the encode family ----------------------------------------------------------------------------------------------------------------------------------------
ENC_SHAPES = [(300, 16, 4), (70_001, 32, 8), (1031, 33, 5)]
FIXED = (2085, 16, 4)                                       # the mutant sequence's one shape: a stale table always has the right size


def _enc_make(kseed=None, it=None):
    def make(n, d, m, seed):
        from conftest import make_problem
        X, K, B0 = make_problem(d, n, m, seed=seed % 100000, kind="gauss")
        if kseed is not None:                              # the mutant sequence: every host-buffer encode brings the SAME codebooks (the trainer's chain)
            K = make_problem(d, 8, m, seed=kseed, kind="gauss")[1]
        return {"X": X, "K": K, "B0": B0, "ils": [1, 2], "J": 3, "npert": 3, "seed": 40 + seed % 7, "it": it}
    return make


def _oracle():
    import oracle as O
    O.build()
    return O


def _check_objective(inp, codes0, obj_mean, what):
    import f64ref as R
    n, d, m = inp["shape"]
    c64, cb = R.veccost(inp["X"], inp["K"], codes0, m)
    R.check_values(obj_mean, c64.mean(), R.mean_bound(cb, c64), what)


def _enc_ref(inp):
    """the oracle's snapshots on the checked row blocks -> list of ((a, b), Bs (nr, b - a, m), objs or None)"""
    if "_ref" not in inp:
        O, (n, d, m) = _oracle(), inp["shape"]
        inp["_ref"] = [((a, b), O.encode_icm(inp["X"][a:b], inp["B0"][a:b], inp["K"], m, H, inp["ils"], inp["J"], inp["npert"], True, inp["seed"],
                                             global_offset=a)) for a, b in _blocks(n)]
    return inp["_ref"]


def _enc_check(one_based, per_vector):
    def check(inp, out):
        n, d, m = inp["shape"]
        Bs = out[0].astype(np.int64) + (0 if one_based else 1)
        objs = np.asarray(out[1], dtype=np.float64) / (1 if per_vector else n)
        for (a, b), (ref, robj) in _enc_ref(inp):
            assert np.array_equal(Bs[:, a:b], ref), "%d codes differ from the oracle in rows %d..%d" % ((Bs[:, a:b] != ref).sum(), a, b)
            if (a, b) == (0, n):
                assert np.allclose(objs, robj, rtol=1e-5, atol=0), (objs, robj)
        for r in range(len(inp["ils"])):
            _check_objective(inp, Bs[r] - 1, objs[r], "objective of snapshot %d" % r)
        _check_walked(inp, out)
    return check


def _check_walked(inp, out):
    """every ILS iteration recomputes node updates, and the call's statistics reach timings() -- also those an async call leaves on the device"""
    updates = int(out[-1][COUNTERS.index("icm_node_updates")])
    assert updates >= inp["shape"][0], "timings() counts %d node updates for an encode of %d vectors" % (updates, inp["shape"][0])


def _call_encode_icm(eng, inp):
    n, d, m = inp["shape"]
    return eng.encode_icm(inp["X"], inp["B0"], inp["K"], m, inp["ils"], inp["J"], inp["npert"], True, seed=inp["seed"])


def _call_encode_icm_dev(nonblocking):
    def call(eng, inp):
        import torch
        n, d, m = inp["shape"]
        dBs, sums, stats = eng.encode_icm_dev(dev(inp["X"]), dev((inp["B0"] - 1).astype(np.uint8)), dev(inp["K"]), m, inp["ils"], inp["J"], inp["npert"], True,
                                              seed=inp["seed"], nonblocking=nonblocking)
        torch.cuda.current_stream().synchronize()
        if nonblocking:
            sums, stats = sums.cpu().numpy(), stats.cpu().numpy()
        return dBs.cpu().numpy(), sums, stats
    return call


def _call_encoding_icm(eng, inp):
    n, d, m = inp["shape"]
    return (eng.encoding_icm(inp["X"], inp["B0"], inp["K"], m, inp["J"], True, inp["npert"], seed=inp["seed"], it=inp["it"]),)


def _the_it(inp):
    return inp["it"] if inp["it"] is not None else inp["auto_it"]          # auto: the driver's count of the successful LSQ_IT_AUTO calls so far


def _check_encoding_icm(inp, out):
    O, (n, d, m) = _oracle(), inp["shape"]
    for a, b in _blocks(n):
        ref = O.encoding_icm_faithful(inp["X"][a:b], inp["B0"][a:b], inp["K"], m, H, inp["J"], True, inp["npert"], inp["seed"], _the_it(inp), global_offset=a)
        assert np.array_equal(out[0][a:b], ref), "%d codes differ from the oracle's iteration %d in rows %d..%d" % ((out[0][a:b] != ref).sum(), _the_it(inp), a, b)
    _check_walked(inp, out)


def _call_fully(eng, inp):
    n, d, m = inp["shape"]
    B = inp["B0"].copy()
    eng.encode_icm_fully(B, inp["X"], inp["K"], m, inp["J"], True, inp["npert"], idx_first=1 + inp["seed"], seed=inp["seed"], it=inp["it"])
    return (B,)


def _check_fully(inp, out):
    O, (n, d, m) = _oracle(), inp["shape"]
    for a, b in _blocks(n):
        ref = O.encode_icm_fully(inp["X"][a:b], inp["B0"][a:b], inp["K"], m, H, inp["J"], True, inp["npert"], inp["seed"], _the_it(inp),
                                 global_offset=inp["seed"] + a)
        assert np.array_equal(out[0][a:b], ref), "%d codes differ from the oracle's worker in rows %d..%d" % ((out[0][a:b] != ref).sum(), a, b)


# ---- the encoder's pieces ----------------------------------------------------------------------------------------------------------------------------------
PIECE_SHAPES = [(129, 16, 2), (4097, 24, 8), (1031, 33, 5)]


def _piece_make(n, d, m, seed):
    rng = np.random.default_rng(seed)
    return {"X": rng.standard_normal((n, d)).astype(np.float32), "K": (rng.standard_normal((m * H, d)) / m).astype(np.float32),
            "B": rng.integers(1, H + 1, size=(n, m)).astype(np.int16), "seed": seed}


def _check_unaries(inp, out):
    import f64ref as R
    n, d, m = inp["shape"]
    rows = _rows(n)
    ref, bnd = R.unaries(inp["X"][rows], inp["K"], m)
    R.check_values(out[0][:, rows], ref, bnd, "unaries")


def _check_binaries(inp, out):
    import f64ref as R
    ref, bnd = R.pair_tables(inp["K"], inp["shape"][2])
    R.check_values(out[0], ref, bnd, "pair tables")


def _check_veccost(inp, out):
    import f64ref as R
    c64, cb = R.veccost(inp["X"], inp["K"], inp["B"].astype(np.int64) - 1, inp["shape"][2])
    R.check_values(out[0], c64, cb, "veccost")


def _check_qerror(inp, out):
    import f64ref as R
    c64, cb = R.veccost(inp["X"], inp["K"], inp["B"].astype(np.int64) - 1, inp["shape"][2])
    R.check_values(float(out[0][0]), c64.mean(), R.mean_bound(cb, c64), "qerror")


def _check_perturb(inp, out):
    O, (n, d, m) = _oracle(), inp["shape"]
    rows = _rows(n, extra=200)
    ref = np.stack([O.perturb(inp["seed"], 1000 + int(i), 3, (inp["B"][i] - 1).astype(np.uint8), H, min(m, 3)) for i in rows]).astype(np.int16) + 1
    assert np.array_equal(out[0][rows], ref)


# ---- the searches -------------------------------------------------------------------------------------------------------------------------------------------
SCAN_SHAPES = [(3000, 32, 4), (60_000, 24, 8), (1031, 33, 5)]                    # (n, d, m); nq and k below


def _scan_make(n, d, m, seed):
    import f64ref as R
    rng = np.random.default_rng(seed)
    K = (rng.standard_normal((m * H, d)) * 0.5).astype(np.float32)
    codes = rng.integers(0, H, size=(n, m), dtype=np.uint8)
    return {"codes": codes, "Q": rng.standard_normal((3 + m % 4, d)).astype(np.float32), "K": K,
            "dbn": (R.reconstruct(K, codes, m) ** 2).sum(1).astype(np.float32), "k": 10 if n != 1031 else n}


def _check_linscan(inp, out):
    import f64ref as R
    vals, bnd = R.lsq_adc(inp["Q"], inp["K"], inp["codes"], inp["dbn"], inp["shape"][2])
    R.check_topk(out[1].astype(np.int64) - 1, out[0], vals, bnd, "LSQ scan")


def _pq_make(n, d, m, seed):
    rng = np.random.default_rng(seed)
    sub = d // m
    return {"centers": rng.standard_normal((m, H, sub)).astype(np.float32), "Q": rng.standard_normal((3 + m % 4, m * sub + 3)).astype(np.float32),
            "codes": rng.integers(0, H, size=(n, m + 1), dtype=np.uint8), "k": 20, "sub": sub}


def _check_pq(inp, out):
    import f64ref as R
    m, sub = inp["shape"][2], inp["sub"]
    vals, bnd = R.pq_dist(inp["Q"][:, :m * sub], list(inp["centers"]), inp["codes"][:, :m])
    R.check_topk(out[1].astype(np.int64), out[0], vals, bnd, "PQ scan")


KNN_SHAPES = [(300, 16, 4), (20_000, 24, 8), (1031, 33, 5)]                      # m: only the number of queries here


def _knn_make(n, d, m, seed):
    rng = np.random.default_rng(seed)
    return {"Xb": rng.standard_normal((n, d)).astype(np.float32), "Xq": rng.standard_normal((m, d)).astype(np.float32), "k": 7}


def _check_knn(inp, out):
    import knn_check as kc
    dists, ids = kc.knn_np(inp["Xb"], inp["Xq"], inp["k"])
    assert np.array_equal(out[1].astype(np.int64), ids.astype(np.int64)) and kc.same_bits(out[0], dists)


# ---- norms ----------------------------------------------------------------------------------------------------------------------------------------------------
NORM_SHAPES = [(300, 16, 2), (3000, 30, 4), (1031, 64, 8)]


def _norm_make(n, d, m, seed):
    import f64ref as R
    rng = np.random.default_rng(seed)
    K = rng.standard_normal((m * H, d)).astype(np.float32)
    codes = rng.integers(0, H, size=(n, m), dtype=np.uint8)
    n64, _ = R.norms(K, codes, m)
    return {"K": K, "codes": codes, "cb": np.sort(rng.choice(n64, size=min(n, 256), replace=False)).astype(np.float32)}


def _check_norms(zero_based):
    def check(inp, out):
        import f64ref as R
        n64, nb = R.norms(inp["K"], inp["codes"], inp["shape"][2])
        idx = out[0].astype(np.int64) - (0 if zero_based else 1)
        R.check_values(out[2], n64, nb, "norms")
        vals, vb = R.norm_centroid_values(n64, nb, inp["cb"])
        R.check_argmin(idx, vals, vb, "norm centroid")
        assert np.array_equal(out[1], inp["cb"][idx])
    return check


# ---- the codebook updates -----------------------------------------------------------------------------------------------------------------------------------
LSQR_SHAPES = [(6000, 8, 2), (20_000, 16, 4), (9001, 7, 3)]


def _lsqr_make(n, d, m, seed):
    from test_f64ref import _lsqr_problem
    X, codes = _lsqr_problem(np.random.default_rng(seed), d, n, m)
    return {"X": X, "codes": codes}


def _check_lsqr(inp, out):
    from test_f64ref import check_lsqr
    n, d, m = inp["shape"]
    assert out[1][0] >= 1
    check_lsqr(out[0], inp["X"], inp["codes"], m, np.arange(d), "normal")


CHAIN_SHAPES = [(3000, 12, 4), (999, 7, 2), (5000, 33, 3)]


def _chain_make(n, d, m, seed):
    import chain_cases as cc
    X, codes, od = cc.chain_problem(d, n, m)
    return {"X": X, "codes": codes, "od": od, "cover": cc.cover_of(od, d, m)}


def _check_chain(inp, out):
    import chain_cases as cc
    n, d, m = inp["shape"]
    assert out[1][0] >= 1 and cc.zero_outside(out[0], inp["od"], d)
    cc.check_chain_lsqr(out[0], inp["X"], inp["codes"], inp["od"], cc.dims_to_check(d, inp["od"]), what="structured update")


SPG_SHAPES = [(300, 3, 2), (1200, 8, 4), (501, 5, 3)]
SPG_MAXIT = 400


def _spg_make(n, d, m, seed):
    from test_gpu_spgl1 import _data, _pq_l1
    X, codes = _data(seed, n, d, m)
    return {"X": X, "codes": codes, "tau": 0.7 * _pq_l1(X, codes, m)}


INFO_INT = ("status", "iterations", "line_search_trials", "nnz_before_threshold", "nnz")
INFO_F64 = ("f", "rel_gap", "l1", "tau")


def _info_arrays(info):
    return np.array([info[k] for k in INFO_INT], dtype=np.int64), np.array([info[k] for k in INFO_F64], dtype=np.float64)


def _check_spg(inp, out):
    import spgl1_check as chk
    from test_gpu_spgl1 import _certify
    info = dict(zip(INFO_INT, out[1].tolist()))
    info.update(zip(INFO_F64, out[2].tolist()))
    P = chk.Problem(inp["X"], inp["codes"], inp["shape"][2])
    if info["status"] == 0:
        _certify(P, out[0], inp["tau"], info)
    else:                                                  # stopped at the cap: still feasible, and a descent from K = 0 (tests/test_gpu_spgl1.py's rule)
        c = chk.certificate(P, out[0], inp["tau"])
        assert info["status"] == 1 and info["iterations"] == SPG_MAXIT, info
        assert c["l1"] <= inp["tau"] * (1 + 1e-6) and abs(info["f"] - c["f"]) <= 1e-6 * max(1.0, c["f"]) and c["f"] <= 0.5 * float(np.sum(P.X ** 2))


# ---- the initialisers ----------------------------------------------------------------------------------------------------------------------------------------
VIT_SHAPES = [(64, 24, 3), (129, 64, 8), (100, 32, 4)]


def _vit_make(n, d, m, seed):
    from test_f64ref import _chain_case
    X, K = _chain_case(seed, n, d, m)
    return {"X": X, "K": K}


def _check_vit(zero_based):
    def check(inp, out):
        import f64ref as R
        R.check_chain(inp["X"], inp["K"], out[0].astype(np.int64) - (0 if zero_based else 1), inp["shape"][2], what="Viterbi")
    return check


ASSIGN_SHAPES = [(300, 16, 4), (5000, 32, 8), (129, 30, 7)]


def _check_assign(zero_based):
    def check(inp, out):
        import oracle.init_oracle as ini
        wa, wmin = ini.assign_codewords_exact(inp["X"], inp["K"], inp["shape"][2], H)
        assert np.array_equal(out[0].astype(np.int64) - (0 if zero_based else 1), wa) and np.array_equal(out[1], wmin)
    return check


def _call_assign_own(eng, inp):
    """lsq_assign_codewords_dev on the context's OWN stream (the raw symbol: Engine's form rebinds the stream around every call)"""
    import torch
    n, d, m = inp["shape"]
    dX, dK = dev(inp["X"]), dev(inp["K"])
    dB, dmin = torch.empty((n, m), dtype=torch.uint8, device=dX.device), torch.empty((n, m), dtype=torch.float32, device=dX.device)
    torch.cuda.synchronize()
    eng._check(eng._L.lsq_assign_codewords_dev(eng._h, dX.data_ptr(), dK.data_ptr(), d, n, m, H, dB.data_ptr(), dmin.data_ptr()))
    eng.synchronize()
    return dB.cpu().numpy(), dmin.cpu().numpy()


CENTER_SHAPES = [(100, 16, 2), (5000, 30, 4), (4001, 33, 5)]


def _center_make(n, d, m, seed):
    import kmeans_check as kc
    rng = np.random.default_rng(seed)
    return {"X": (rng.standard_normal((n, d)) * 2 + 0.5).astype(np.float32), "codes": rng.integers(H, size=(n, m)).astype(np.uint8),
            "cover": kc.chain_cover(d, m) if m == 5 else kc.pq_cover(d, m), "K_prev": rng.standard_normal((m * H, d)).astype(np.float32)}


def _check_centers(inp, out):
    import kmeans_check as kc
    want, cnt = kc.centers_exact(inp["X"], inp["codes"], inp["cover"], H, inp["K_prev"])
    assert np.array_equal(out[1], cnt) and np.array_equal(_bits(out[0]), _bits(want))


SEED_SHAPES = [(3000, 16, 4), (20_000, 4, 1), (5003, 12, 3)]


def _seed_make(n, d, m, seed):
    import kmeans_check as kc
    return {"X": np.ascontiguousarray(kc.clustered(d, n, seed=2).T), "cover": kc.pq_cover(d, m), "u": np.random.default_rng(seed).random((m, H))}


def _check_seed(inp, out):
    import kmeans_check as kc
    v = kc.judge_seeding(inp["X"], inp["cover"], inp["u"], out[1])
    assert v["bad"] == [], v["bad"][:5]
    assert v["ambiguous"] <= 0.01 * v["steps"] and np.array_equal(_bits(out[2]), _bits(v["d2"]))
    for j in range(inp["shape"][2]):
        want = np.zeros((H, inp["shape"][1]), dtype=np.float32)
        cols = inp["cover"][:, j] == 1
        want[:, cols] = inp["X"][out[1][j]][:, cols]
        assert np.array_equal(_bits(out[0][j * H:(j + 1) * H]), _bits(want))


# ---- the generators -----------------------------------------------------------------------------------------------------------------------------------------
GEN_SHAPES = [(300, 16, 4), (70_001, 32, 8), (1031, 33, 5)]


def _gen_make(n, d, m, seed):
    return {"seed": seed, "goff": 1000 * m}


def _check_randinit(inp, out):
    n, d, m = inp["shape"]
    assert np.array_equal(out[0].astype(np.int16) + 1, _oracle().randinit(inp["seed"], n, m, H, global_offset=inp["goff"]))


def _check_synth_data(inp, out):
    n, d, m = inp["shape"]
    assert np.array_equal(_bits(out[0]), _bits(_oracle().synth_data_u8(inp["seed"], n, d, global_offset=inp["goff"])))


def _check_synth_codebooks(inp, out):
    """the header's rule: codeword (j, a) = a synthetic u8 data vector / m (no checker restates which one)"""
    n, d, m = inp["shape"]
    v = out[0].astype(np.float64) * m
    assert out[0].shape == (m * H, d) and np.all(np.abs(v - np.rint(v)) <= 1e-3) and v.min() >= -1e-3 and v.max() <= 255 + 1e-3 and np.unique(np.rint(v)).size > 16


def _h(t):
    return t.cpu().numpy()


def _b16(codes):
    return codes.astype(np.int16) + 1


def catalogue(fixed=False):
    """fixed=False: the whole alphabet's operations.  fixed=True: the mutant sequence's -- every variant has the ONE shape FIXED (they differ in their seeds),
    and every host-buffer encode brings the same codebooks."""
    ks = 4242 if fixed else None

    def op(*a, **k):
        return Op(*a, fixed=fixed, **k)

    m_of = lambda inp: inp["shape"][2]
    ops = [
        op("encode_icm", ["lsq_encode_icm"], ENC_SHAPES, _enc_make(ks), _call_encode_icm, _enc_check(True, True), encode=True),
        op("encode_icm_dev", ["lsq_encode_icm_dev"], ENC_SHAPES, _enc_make(), _call_encode_icm_dev(False), _enc_check(False, False), dev=True, encode=True),
        op("encode_icm_dev_nb", ["lsq_encode_icm_dev"], ENC_SHAPES, _enc_make(), _call_encode_icm_dev(True), _enc_check(False, False), dev=True, encode=True),
        op("encoding_icm_auto", ["lsq_encoding_icm"], ENC_SHAPES, _enc_make(ks), _call_encoding_icm, _check_encoding_icm, auto=True, encode=True),
        op("encoding_icm_it", ["lsq_encoding_icm"], ENC_SHAPES, _enc_make(ks, it=2), _call_encoding_icm, _check_encoding_icm, encode=True),
        op("encode_icm_fully", ["lsq_encode_icm_fully"], ENC_SHAPES, _enc_make(ks, it=1), _call_fully, _check_fully, encode=True),
        op("encode_icm_fully_auto", ["lsq_encode_icm_fully"], ENC_SHAPES, _enc_make(ks), _call_fully, _check_fully, auto=True, encode=True),
        op("get_unaries", ["lsq_get_unaries"], PIECE_SHAPES, _piece_make, lambda e, i: (e.get_unaries(i["X"], i["K"], m_of(i)),), _check_unaries),
        op("get_binaries", ["lsq_get_binaries"], PIECE_SHAPES, _piece_make, lambda e, i: (e.get_binaries(i["K"], m_of(i)),), _check_binaries),
        op("veccost", ["lsq_veccost"], PIECE_SHAPES, _piece_make, lambda e, i: (e.veccost(i["X"], i["B"], i["K"], m_of(i)),), _check_veccost),
        op("qerror", ["lsq_qerror"], PIECE_SHAPES, _piece_make, lambda e, i: (np.array([e.qerror(i["X"], i["B"], i["K"], m_of(i))]),), _check_qerror),
        op("perturb", ["lsq_perturb"], PIECE_SHAPES, _piece_make,
           lambda e, i: (e.perturb(i["B"], min(m_of(i), 3), seed=i["seed"], it=3, global_offset=1000),), _check_perturb),
        op("assign_codewords_dev_own", ["lsq_assign_codewords_dev", "lsq_synchronize"], ASSIGN_SHAPES, _piece_make, _call_assign_own, _check_assign(True)),
    ]
    if fixed:
        return [o for o in ops if o.name in MUTANT_NAMES]
    ops += [
        op("linscan", ["lsq_linscan"], SCAN_SHAPES, _scan_make, lambda e, i: e.linscan(i["codes"], i["Q"], i["K"], i["dbn"], m_of(i), i["k"]), _check_linscan,
           scan=True),
        op("linscan_dev", ["lsq_linscan_dev"], SCAN_SHAPES, _scan_make,
           lambda e, i: map(_h, e.linscan_dev(dev(i["codes"]), dev(i["Q"]), dev(i["K"]), dev(i["dbn"]), m_of(i), i["k"])), _check_linscan, scan=True, dev=True),
        op("linscan_pq", ["lsq_linscan_pq"], SCAN_SHAPES, _pq_make, lambda e, i: e.linscan_pq(i["codes"], i["Q"], i["centers"], m_of(i), i["k"], i["sub"]),
           _check_pq, scan=True),
        op("linscan_pq_dev", ["lsq_linscan_pq_dev"], SCAN_SHAPES, _pq_make,
           lambda e, i: map(_h, e.linscan_pq_dev(dev(i["codes"]), dev(i["Q"]), dev(i["centers"]), m_of(i), i["k"], i["sub"])), _check_pq, scan=True, dev=True),
        op("knn_exact", ["lsq_knn_exact"], KNN_SHAPES, _knn_make, lambda e, i: e.knn_exact(i["Xb"], i["Xq"], i["k"]), _check_knn, scan=True),
        op("knn_exact_dev", ["lsq_knn_exact_dev"], KNN_SHAPES, _knn_make, lambda e, i: map(_h, e.knn_exact_dev(dev(i["Xb"]), dev(i["Xq"]), i["k"])), _check_knn,
           scan=True, dev=True),
        op("quantize_norms", ["lsq_quantize_norms"], NORM_SHAPES, _norm_make, lambda e, i: e.quantize_norms(_b16(i["codes"]), i["K"], i["cb"], m_of(i)),
           _check_norms(False)),
        op("quantize_norms_dev", ["lsq_quantize_norms_dev"], NORM_SHAPES, _norm_make,
           lambda e, i: map(_h, e.quantize_norms_dev(dev(i["codes"]), dev(i["K"]), dev(i["cb"]), m_of(i))), _check_norms(True), dev=True),
        op("update_codebooks", ["lsq_update_codebooks_gpu"], LSQR_SHAPES, _lsqr_make,
           lambda e, i: (lambda K, it: (K, np.array([it])))(*e.update_codebooks(i["X"], _b16(i["codes"]), m_of(i))), _check_lsqr),
        op("update_codebooks_dev", ["lsq_update_codebooks_dev"], LSQR_SHAPES, _lsqr_make,
           lambda e, i: (lambda K, it: (_h(K), np.array([it])))(*e.update_codebooks_dev(dev(i["X"]), dev(i["codes"].astype(np.uint8)), m_of(i))), _check_lsqr,
           dev=True),
        op("update_codebooks_struct", ["lsq_update_codebooks_struct_gpu"], CHAIN_SHAPES, _chain_make,
           lambda e, i: (lambda K, it: (K, np.array([it])))(*e.update_codebooks_struct(i["X"], _b16(i["codes"]), i["cover"], m_of(i))), _check_chain),
        op("update_codebooks_struct_dev", ["lsq_update_codebooks_struct_dev"], CHAIN_SHAPES, _chain_make,
           lambda e, i: (lambda K, it: (_h(K), np.array([it])))(*e.update_codebooks_struct_dev(dev(i["X"]), dev(i["codes"].astype(np.uint8)), dev(i["cover"]),
                                                                                                m_of(i))), _check_chain, dev=True),
        op("update_codebooks_spgl1", ["lsq_update_codebooks_spgl1"], SPG_SHAPES, _spg_make,
           lambda e, i: (lambda K, info: (K,) + _info_arrays(info))(*e.update_codebooks_spgl1(i["X"], _b16(i["codes"]), m_of(i), i["tau"], max_iter=SPG_MAXIT)),
           _check_spg),
        op("update_codebooks_spgl1_dev", ["lsq_update_codebooks_spgl1_dev"], SPG_SHAPES, _spg_make,
           lambda e, i: (lambda K, info: (_h(K),) + _info_arrays(info))(*e.update_codebooks_spgl1_dev(dev(i["X"]), dev(i["codes"]), m_of(i), i["tau"],
                                                                                                        max_iter=SPG_MAXIT)), _check_spg, dev=True),
        op("encode_viterbi", ["lsq_encode_viterbi"], VIT_SHAPES, _vit_make, lambda e, i: (e.encode_viterbi(i["X"], i["K"], m_of(i)),), _check_vit(False)),
        op("encode_viterbi_dev", ["lsq_encode_viterbi_dev"], VIT_SHAPES, _vit_make, lambda e, i: (_h(e.encode_viterbi_dev(dev(i["X"]), dev(i["K"]), m_of(i))),),
           _check_vit(True), dev=True),
        op("assign_codewords", ["lsq_assign_codewords"], ASSIGN_SHAPES, _piece_make, lambda e, i: e.assign_codewords(i["X"], i["K"], m_of(i), want_min=True),
           _check_assign(False)),
        op("assign_codewords_dev", ["lsq_assign_codewords_dev"], ASSIGN_SHAPES, _piece_make,
           lambda e, i: map(_h, e.assign_codewords_dev(dev(i["X"]), dev(i["K"]), m_of(i), want_min=True)), _check_assign(True), dev=True),
        op("update_centers", ["lsq_update_centers"], CENTER_SHAPES, _center_make,
           lambda e, i: e.update_centers(i["X"], _b16(i["codes"]), i["cover"], m_of(i), K_prev=i["K_prev"]), _check_centers),
        op("update_centers_dev", ["lsq_update_centers_dev"], CENTER_SHAPES, _center_make,
           lambda e, i: map(_h, e.update_centers_dev(dev(i["X"]), dev(i["codes"]), i["cover"], m_of(i), K_prev=dev(i["K_prev"]))), _check_centers, dev=True),
        op("kmeanspp_seed", ["lsq_kmeanspp_seed"], SEED_SHAPES, _seed_make, lambda e, i: e.kmeanspp_seed(i["X"], i["cover"], i["u"], m_of(i)), _check_seed),
        op("kmeanspp_seed_dev", ["lsq_kmeanspp_seed_dev"], SEED_SHAPES, _seed_make,
           lambda e, i: map(_h, e.kmeanspp_seed_dev(dev(i["X"]), i["cover"], i["u"], m_of(i), want_d2=True)), _check_seed, dev=True),
        op("randinit_dev", ["lsq_randinit_dev"], GEN_SHAPES, _gen_make,
           lambda e, i: (_h(e.randinit_dev(i["seed"], i["shape"][0], m_of(i), global_offset=i["goff"])),), _check_randinit, dev=True),
        op("synth_data_u8_dev", ["lsq_synth_data_u8_dev"], GEN_SHAPES, _gen_make,
           lambda e, i: (_h(e.synth_data_u8_dev(i["seed"], i["shape"][0], i["shape"][1], global_offset=i["goff"])),), _check_synth_data, dev=True),
        op("synth_codebooks_dev", ["lsq_synth_codebooks_dev"], GEN_SHAPES, _gen_make,
           lambda e, i: (_h(e.synth_codebooks_dev(i["seed"], m_of(i), i["shape"][1])),), _check_synth_codebooks, dev=True),
    ]
    return ops


def moves():
    return [Move("opt:" + p, ["lsq_set_option"]) for p in PROFILE_NAMES] + [Move("stream:toggle", ["lsq_set_stream"]), Move("rejected", []),
                                                                            Move("reset_timings", ["lsq_reset_timings"])]


def alphabet():
    return catalogue() + moves()


# every context symbol is either walked (above) or listed here with the reason
EXCLUDED = {
    "lsq_create": "makes the context: every baseline and every walk starts with it",
    "lsq_destroy": "ends the context: nothing can follow it",
    "lsq_get_timings": "getter (the v400 prefix of lsq_get_timings_sized)",
    "lsq_get_timings_sized": "getter: read before and after every step of the walk",
    "lsq_get_walk_trace": "getter of host-side counters",
    "lsq_get_linscan_stats": "getter: read before and after every scan of the walk",
    "lsq_get_q16_snapshot": "getter: copies the resident levels and their parameters, computes nothing (tests/test_gpu_q16_bound.py reads it after encodes)",
}


def context_symbols():
    """the symbols whose first argument is a context, from the header"""
    with open(os.path.join(ROOT, "include", "lsq_mi355x.h")) as f:
        return sorted(set(re.findall(r"\b(lsq_\w+)\s*\(\s*lsq_ctx\s*\*", f.read())))


# ---- rejected calls: the raw symbol with every pointer null and m = 17 or h = 128 (or, where the symbol has neither, the null pointers alone) -----------------
ARG_NAMES = {
    "lsq_encode_icm": "X B K d n m h ils nr icmiter npert randord nsplits seed goff verbose Bs objs",
    "lsq_encode_icm_dev": "X B K d n m h ils nr icmiter npert randord seed goff Bs obj stats",
    "lsq_encoding_icm": "X B K d n m h niter randord npert seed it goff out",
    "lsq_encode_icm_fully": "B X K d n m h niter randord npert idx_first seed it",
    "lsq_get_unaries": "X K d n m h U", "lsq_get_binaries": "K d m h T", "lsq_veccost": "X B K d n m h out", "lsq_qerror": "X B K d n m h out",
    "lsq_perturb": "B n m h npert seed it goff",
    "lsq_linscan": "dists idx codes Q K dbn nq n m h d nn", "lsq_linscan_dev": "dists idx codes Q K dbn nq n m h d nn",
    "lsq_linscan_pq": "dists res codes centers Q n nq bits nn dc dq subdim", "lsq_linscan_pq_dev": "dists res codes centers Q n nq bits nn dc dq subdim",
    "lsq_knn_exact": "dists ids base Q n nq d ldb ldq nn", "lsq_knn_exact_dev": "dists ids base Q n nq d ldb ldq nn",
    "lsq_quantize_norms": "B K cb ncb d n m h idx dbn nrm", "lsq_quantize_norms_dev": "B K cb ncb d n m h idx dbn nrm",
    "lsq_update_codebooks_gpu": "X B d n m h K it", "lsq_update_codebooks_dev": "X B d n m h K it",
    "lsq_update_codebooks_struct_gpu": "X B cover d n m h K it", "lsq_update_codebooks_struct_dev": "X B cover d n m h K it",
    "lsq_update_codebooks_spgl1": "X B d n m h tau Kinit S params K info", "lsq_update_codebooks_spgl1_dev": "X B d n m h tau Kinit S params K info",
    "lsq_encode_viterbi": "X K d n m h B", "lsq_encode_viterbi_dev": "X K d n m h B",
    "lsq_assign_codewords": "X K d n m h B minval", "lsq_assign_codewords_dev": "X K d n m h B minval",
    "lsq_update_centers": "X B cover Kprev d n m h K counts", "lsq_update_centers_dev": "X B cover Kprev d n m h K counts",
    "lsq_kmeanspp_seed": "X cover u d n m h K idx d2", "lsq_kmeanspp_seed_dev": "X cover u d n m h K idx d2",
    "lsq_synth_data_u8_dev": "seed goff n d X", "lsq_randinit_dev": "seed goff n m h B", "lsq_synth_codebooks_dev": "seed m h d K",
}
_INTS = {"d": 8, "n": 4, "nq": 1, "nr": 1, "nn": 1, "ncb": 4, "ldb": 8, "ldq": 8, "dc": 17, "dq": 40, "subdim": 2, "idx_first": 1, "S": -1}


def rejected_calls():
    """-> list of (symbol, flavour, args after the context): every call must return LSQ_EINVAL before it touches a pointer"""
    from importlib import import_module
    sig = import_module("local-search-quantization_amd._lib").SIGNATURES
    out = []
    for sym, names in sorted(ARG_NAMES.items()):
        names, types = names.split(), sig[sym][1][1:]
        assert len(names) == len(types), sym
        has_m = "m" in names or "bits" in names
        flavours = [("m = 17", {"m": 17, "h": H, "bits": 8 * 17})] if has_m else [("null pointers", {})]
        if "h" in names:
            flavours.append(("h = 128", {"m": 8, "h": 128}))
        for what, mh in flavours:
            args = []
            for name, ty in zip(names, types):
                if ty is C.c_double:
                    args.append(1.0)
                elif ty in (C.c_int, C.c_int64, C.c_uint64, C.c_uint32):
                    args.append(mh.get(name, _INTS.get(name, 1)))
                else:
                    args.append(None)                      # every pointer: null
            out.append((sym, what, args))
    return out


# ---- sequences ------------------------------------------------------------------------------------------------------------------------------------------------
def eulerian_circuit(k, seed=0):
    """A seeded Eulerian circuit of the complete digraph on k nodes with self-loops (Hierholzer) -> k * k + 1 nodes, the first one repeated at the end:
    every ordered pair (a, b) is one consecutive pair of it, exactly once."""
    rng = np.random.default_rng(seed)
    out_edges = [list(rng.permutation(k)) for _ in range(k)]
    start = int(rng.integers(k))
    stack, circuit = [start], []
    while stack:
        v = stack[-1]
        if out_edges[v]:
            stack.append(int(out_edges[v].pop()))
        else:
            circuit.append(stack.pop())
    return circuit[::-1]


def plan(names_in_order, ops):
    """the (name, variant) of every visit: an entry's visits take its variants in rotation"""
    seen, out = {}, []
    for name in names_in_order:
        o = ops[name]
        v = None
        if o.kind == "op":
            v = seen.get(name, 0) % len(o.shapes)
            seen[name] = seen.get(name, 0) + 1
        out.append((name, v))
    return out


MUTANT_PRIME = "encoding_icm_it"
MUTANT_NAMES = ("encoding_icm_it", "encoding_icm_auto", "encode_icm_fully_auto", "encode_icm_dev", "encode_icm_dev_nb", "veccost", "assign_codewords_dev_own")
MUTANT_PHASES = ("default", "s6_forced")


def mutant_sequence():
    """The fixed-shape sequence the mutants are run on: under each of the two profiles, for every ordered pair (A, B) of the fixed catalogue the three steps
    prime, A, B -- the prime is a host-buffer encode with the shared codebooks, so that every pair starts from a valid host-table cache."""
    names = [o.name for o in catalogue(fixed=True)]
    seq = []
    for p in MUTANT_PHASES:
        seq.append("opt:" + p)
        for a in names:
            for b in names:
                seq += [MUTANT_PRIME, a, b]
    return seq + ["opt:default"]


# ---- the driver -----------------------------------------------------------------------------------------------------------------------------------------------
def first_difference(got, want):
    """-> None, or the first differing element of two result tuples in words (NaN equals NaN at the same position)"""
    if len(got) != len(want):
        return "%d outputs, the baseline has %d (%s)" % (len(got), len(want), "an error code" if is_error(got) or is_error(want) else "?")
    for q, (a, b) in enumerate(zip(got, want)):
        if a.dtype != b.dtype or a.shape != b.shape:
            return "output %d is %s%s, the baseline's %s%s: %r vs %r" % (q, a.dtype, a.shape, b.dtype, b.shape, a.reshape(-1)[:4], b.reshape(-1)[:4])
        if a.dtype.kind == "f":
            ne = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        else:
            ne = a != b
        if np.any(ne):
            at = tuple(int(i) for i in np.argwhere(np.atleast_1d(ne))[0])
            counters = a.shape == (len(COUNTERS),) and a.dtype == np.int64 and q >= len(got) - 2
            what = "counter deltas" if counters else "output %d" % q
            name = " (%s)" % COUNTERS[at[0]] if counters else ""
            return "%s differs at %r%s: got %r, the baseline has %r (%d of %d elements differ)" % (what, at, name, np.atleast_1d(a)[at], np.atleast_1d(b)[at],
                                                                                                   int(np.sum(ne)), a.size)
    return None


class Walk:
    """One long-lived Engine taken through a sequence of entries; every operation is held to the same entry and variant on a FRESH Engine that carries the
    option profile the driver believes is active (cached by entry, variant, profile -- and, for the LSQ_IT_AUTO entries, the count the driver believes in)."""

    def __init__(self, ops=None, seed=0):
        self.lsq = lsq_pkg()
        self.ops = {o.name: o for o in (ops if ops is not None else alphabet())}
        self.cache, self.inputs, self.demoted = {}, {}, {}
        self.rejects = None
        self.rng = np.random.default_rng(seed)
        self.eng = None
        self.fresh_runs = 0

    # -- the long-lived context and the driver's beliefs about it
    def open(self):
        self.close()
        self.eng = self.lsq.Engine(0)
        self.profile, self.side, self.auto, self.visits, self.prev, self.index = "default", False, 0, {}, None, 0
        self.after_reject = False
        return self

    def close(self):
        if self.eng is not None:
            self.eng.close()
            self.eng = None

    def inputs_for(self, name, v):
        if (name, v) not in self.inputs:
            self.inputs[(name, v)] = self.ops[name].make(v)
        return self.inputs[(name, v)]

    def _inp(self, name, v, auto):
        inp = self.inputs_for(name, v)
        if self.ops[name].auto:
            inp = dict(inp, auto_it=auto)
            inp.pop("_ref", None)
        return inp

    def fresh(self, name, v, profile="default", auto=0):
        import torch
        op = self.ops[name]
        self.fresh_runs += 1
        with self.lsq.Engine(0) as e:
            apply_profile(e, profile)
            if op.auto:
                e.set_option("ils_counter", auto)
            out = op.run(e, self._inp(name, v, auto))
            torch.cuda.synchronize()
        return out

    def baseline(self, name, v, profile="default", auto=0):
        key = (name, v, profile, auto if self.ops[name].auto else None)
        if key not in self.cache:
            out = self.fresh(name, v, profile, auto)
            self.ops[name].check(self._inp(name, v, auto), out, profile)
            self.cache[key] = out
        return self.cache[key]

    def determinism(self, name, v):
        """the entry on two fresh contexts -> None, or the first difference (the entry is then demoted: the walk holds it to its checker, not to equality)"""
        a = self.baseline(name, v)
        diff = first_difference(self.fresh(name, v), a)
        if diff is not None:
            self.demoted.setdefault(name, []).append("variant %d: %s" % (v, diff))
        return diff

    # -- one step
    def where(self, name, v):
        return "step %d: %s -> %s, variant %s %s, profile %s, %s stream" % (self.index, self.prev, name, v, self.ops[name].shapes[v] if v is not None else "",
                                                                           self.profile, "side" if self.side else "default")

    def step(self, name):
        """-> None, or the mismatch in words.  Moves never mismatch except a rejected call that is not rejected."""
        import torch
        op, v, bad = self.ops[name], None, None
        if name.startswith("opt:"):
            torch.cuda.synchronize()
            self.profile = name[4:]
            apply_profile(self.eng, self.profile)
        elif name == "stream:toggle":
            torch.cuda.synchronize()                        # the contract of lsq_set_stream: nothing un-awaited on the old stream
            self.side = not self.side
            if self.side and not hasattr(self, "side_stream"):
                self.side_stream = torch.cuda.Stream()
        elif name == "reset_timings":
            self.eng.reset_timings()
        elif name == "rejected":
            if self.rejects is None:
                self.rejects = rejected_calls()
            sym, what, args = self.rejects[int(self.rng.integers(len(self.rejects)))]
            rc = getattr(self.eng._L, sym)(self.eng._h, *args)
            if rc != EINVAL:
                bad = "%s: %s with %s returned %d, not LSQ_EINVAL" % (self.where(name, None), sym, what, rc)
        else:
            v = self.visits.get(name, 0) % len(op.shapes)
            self.visits[name] = self.visits.get(name, 0) + 1
            inp = self._inp(name, v, self.auto)
            try:
                want = self.baseline(name, v, self.profile, self.auto)
            except AssertionError as e:                     # the step still runs: the context must see the same sequence either way
                want, bad = None, "%s: the fresh context's result fails its checker: %s" % (self.where(name, v), str(e)[:300])
            if self.side and op.dev:
                with torch.cuda.stream(self.side_stream):
                    got = op.run(self.eng, inp)
            else:
                got = op.run(self.eng, inp)
            torch.cuda.synchronize()
            if op.auto and not is_error(got):
                self.auto += 1
            if name in self.demoted:
                try:
                    op.check(inp, got, self.profile)
                    diff = None
                except AssertionError as e:
                    diff = "checker: %s" % (e,)
            elif want is not None:
                diff = first_difference(got, want)
            else:
                diff = None
            if diff is not None and bad is None:
                bad = "%s: %s" % (self.where(name, v), diff)
        self.prev, self.index = name, self.index + 1
        return bad

    def run(self, names, stop_at_first=True):
        """-> list of (index, previous entry, entry, profile, message) of the steps that mismatch"""
        out = []
        for name in names:
            prev, profile = self.prev, self.profile
            bad = self.step(name)
            if bad is not None:
                out.append((self.index - 1, prev, name, profile if not name.startswith("opt:") else name[4:], bad))
                if stop_at_first:
                    break
        return out


def main(argv):
    """python tests/ctx_ops.py --mutant-sequence: the fixed-shape sequence on the library LSQ_LIB_PATH names -> one JSON line with every mismatching step"""
    import json
    if argv != ["--mutant-sequence"]:
        raise SystemExit(main.__doc__)
    w = Walk(catalogue(fixed=True) + moves()).open()
    try:
        bad = w.run(mutant_sequence(), stop_at_first=False)
    finally:
        w.close()
    print("CTX_MUTANT_RESULT " + json.dumps({"lib": lsq_pkg()._lib.LIB_PATH, "steps": w.index, "fresh_contexts": w.fresh_runs,
                                             "mismatches": [[i, p, c, prof, msg[:400]] for i, p, c, prof, msg in bad]}))


if __name__ == "__main__":
    main(sys.argv[1:])
