"""The seeded inputs that tests/test_gpu_select_model.py runs on the device and tests/test_select_model.py proves able to tell a wrong selection from a
right one (every entry of select_model.MUTANTS must predict other statistics than the model on at least one of them).  numpy only.

A case is (producer, inputs, nn, options): producer "lsq" (codes, Q, K, dbnorms, m), "pq" (codes, centers, Q, m, subdim), "exact" (Xb, Xq) or "u8"
(Xb, Xq uint8); `matrix(lib, case)` is its full distance matrix by the producer's host form."""
import functools

import numpy as np

import select_model as SM

H = 256
RANKS = (0, 1, 2, 255, 256, 257, 8192, 16383, 16384, 20000)      # option linscan_rank (0: the plan's own rank)
ID_BASE = {"lsq": 1, "pq": 0, "exact": 0, "u8": 0}
FLT_MAX = np.float32(3.4028234663852886e38)


class Case:
    def __init__(self, name, producer, inputs, nn, **options):
        self.name, self.producer, self.inputs, self.nn, self.options = name, producer, inputs, nn, options
        self.n = inputs[0].shape[0]
        self.nq = (inputs[1] if producer != "pq" else inputs[2]).shape[0]
        self.id_base = ID_BASE[producer]
        for a in inputs:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)

    def plan_args(self, rank=0):
        return dict(rank=rank, force_exhaustive=self.options.get("linscan_exhaustive", 0))


def matrix(lib, case):
    """the case's (nq, n) distance matrix by its producer's host form with nn = n (computed once per case object)"""
    if getattr(case, "_D", None) is None:
        f = {"lsq": SM.full_matrix_lsq, "pq": SM.full_matrix_pq, "exact": SM.full_matrix_exact, "u8": SM.full_matrix_exact_u8}[case.producer]
        case._D = f(lib, *case.inputs)
        case._D.setflags(write=False)
    return case._D


# ---- a. crafted key distributions through the LSQ scan: zero codebooks, so dist(i) == dbnorms[i] (-0.0 comes out as +0.0) ----------------------------
CRAFTED_N, CRAFTED_NQ, CRAFTED_NN, CRAFTED_D = 98_304, 5, 50, 4
CRAFTED_M = (8, 3)                                      # dword and byte code reads


def _keys_to_f32(keys):
    return SM.unkey(np.asarray(keys, dtype=np.uint32)).copy()


def _consecutive(count):
    """n keys drawn from `count` consecutive bit patterns, both ends of the range among the SAMPLED entries: the rank select sees hi - lo = count - 1"""
    def make(rng, n, stride):
        lo = int(np.float32(1.0).view(np.uint32)) | 0x80000000          # key(1.0)
        lo -= count // 2
        keys = lo + rng.integers(0, count, n)
        keys[0], keys[stride * 3] = lo, lo + count - 1
        return _keys_to_f32(keys)
    return make


def _all_equal(rng, n, stride):
    return np.full(n, 1.5, dtype=np.float32)


def _two_values(rng, n, stride):
    return rng.choice(np.array([-1.0, 1.0], dtype=np.float32), n)


def _log_uniform(rng, n, stride):
    mag = np.exp(rng.uniform(np.log(1e-38), np.log(1e38), n))
    return (mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def _tie_group(rng, n, stride):
    """500 equal entries; 12 of them are the sampled entries of rank 25 .. 36: the group straddles the plan's rank (31) in the sample"""
    v = rng.standard_normal(n).astype(np.float32)
    s = np.arange(SM.NS) * stride
    order = s[np.argsort(v[s], kind="stable")]
    val = v[order[24]]
    v[order[24:36]] = val
    free = np.setdiff1d(np.arange(n), s)
    v[rng.choice(free, 488, replace=False)] = val
    return v


def _list_filled_to(over):
    """ties with the plan's threshold among the UNSAMPLED entries until the list holds exactly cap + over pairs: the edge of `count > cap`"""
    def make(rng, n, stride):
        v = rng.standard_normal(n).astype(np.float32)
        P = SM.plan(n, CRAFTED_NN)
        s = np.arange(SM.NS) * stride
        tau = np.sort(v[s])[P["r"] - 1]
        free = np.setdiff1d(np.flatnonzero(v > tau), s)
        v[rng.choice(free, P["cap"] + over - int((v <= tau).sum()), replace=False)] = tau
        assert int((v <= tau).sum()) == P["cap"] + over
        return v
    return make


def _nan_share(share):
    def make(rng, n, stride):
        v = rng.standard_normal(n).astype(np.float32)
        v[rng.random(n) < share] = np.nan
        return v
    return make


def _inf_mix(rng, n, stride):
    v = rng.standard_normal(n).astype(np.float32)
    u = rng.random(n)
    v[u < 0.30] = np.inf
    v[(u >= 0.30) & (u < 0.3004)] = -np.inf
    v[(u >= 0.3004) & (u < 0.40)] = np.nan
    v[(u >= 0.40) & (u < 0.41)] = -0.0
    return v


DISTRIBUTIONS = [("all_equal", _all_equal), ("two_values", _two_values)]
DISTRIBUTIONS += [("consecutive_%d" % c, _consecutive(c)) for c in (255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24)]
DISTRIBUTIONS += [("log_uniform", _log_uniform), ("tie_group_at_rank", _tie_group), ("list_exactly_full", _list_filled_to(0)),
                  ("list_one_over_capacity", _list_filled_to(1)), ("nan_1_percent", _nan_share(0.01)),
                  ("nan_999_permille", _nan_share(0.999)), ("inf_and_nan_mix", _inf_mix)]
DISTRIBUTION_NAMES = [d[0] for d in DISTRIBUTIONS]


@functools.lru_cache(maxsize=None)
def crafted(name, m):
    k = DISTRIBUTION_NAMES.index(name)
    rng = np.random.default_rng(9000 + 16 * k + m)
    n = CRAFTED_N
    dbnorms = DISTRIBUTIONS[k][1](rng, n, n // SM.NS).astype(np.float32)
    codes = rng.integers(0, H, size=(n, m), dtype=np.uint8)
    Q = rng.standard_normal((CRAFTED_NQ, CRAFTED_D)).astype(np.float32)
    K = np.zeros((m * H, CRAFTED_D), dtype=np.float32)
    return Case("crafted_%s_m%d" % (name, m), "lsq", (codes, Q, K, dbnorms, m), CRAFTED_NN)


# ---- b. mixed fallbacks: a run of T identical entries, every third query pulled towards it (more than `cap` ties at its threshold), the rest pushed away
MIXED_N, MIXED_NQ, MIXED_NN, MIXED_AT = 70_001, 37, 10, 1000
MIXED_T = {"lsq": 1500, "pq": 1500, "exact": 1500, "u8": 1500}
MIXED_SEED = {"lsq": 0, "pq": 0, "exact": 0, "u8": 0}


def _pull(rng, nq, u):
    """queries 0.3 q + 3 u (every third) or 0.3 q - 3 u, u the unit vector of the run's entry"""
    q = rng.standard_normal((nq, u.size)).astype(np.float32)
    sign = np.where(np.arange(nq) % 3 == 0, 3.0, -3.0).astype(np.float32)
    return (np.float32(0.3) * q + sign[:, None] * u[None, :]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def mixed(producer):
    rng = np.random.default_rng(MIXED_SEED[producer])
    n, nq, T, at = MIXED_N, MIXED_NQ, MIXED_T[producer], MIXED_AT
    if producer == "lsq":
        d, m = 16, 7
        K = (rng.standard_normal((m * H, d)) * 0.5).astype(np.float32)
        codes = rng.integers(0, H, size=(n, m), dtype=np.uint8)
        codes[at:at + T] = codes[at]
        recon = sum(K[j * H + codes[:, j].astype(np.int64)] for j in range(m))
        dbnorms = (recon.astype(np.float64) ** 2).sum(1).astype(np.float32)
        Q = _pull(rng, nq, recon[at] / np.linalg.norm(recon[at]))
        inputs = (codes, Q, K, dbnorms, m)
    elif producer == "pq":
        m, subdim = 4, 4
        centers = rng.standard_normal((m, H, subdim)).astype(np.float32)
        codes = rng.integers(0, H, size=(n, m), dtype=np.uint8)
        codes[at:at + T] = codes[at]
        recon = np.concatenate([centers[k, codes[at, k]] for k in range(m)])
        Q = _pull(rng, nq, recon / np.linalg.norm(recon))
        inputs = (codes, centers, Q, m, subdim)
    elif producer == "exact":
        d = 16
        Xb = rng.standard_normal((n, d)).astype(np.float32)
        Xb[at:at + T] = Xb[at]
        inputs = (Xb, _pull(rng, nq, Xb[at] / np.linalg.norm(Xb[at])))
    else:
        d = 16
        Xb = rng.integers(0, 256, (n, d), dtype=np.uint8)
        Xb[at:at + T] = Xb[at]
        c = Xb[at].astype(np.float32) - np.float32(127.5)
        q = _pull(rng, nq, c / np.linalg.norm(c)) * np.float32(100.0) + np.float32(127.5)     # towards the run's row from the cube's centre, or away
        inputs = (Xb, np.clip(np.rint(q), 0, 255).astype(np.uint8))
    return Case("mixed_" + producer, producer, inputs, MIXED_NN)


# ---- c. more failed queries than one fallback batch holds ((2^28 // n) & ~15 = 4080 at n = 65 537) -----------------------------------------------------
MANY_N, MANY_NQ, MANY_NN = 65_537, 4100, 3


@functools.lru_cache(maxsize=None)
def many_failed():
    """entry 0 (sampled) is by far the nearest of every query: with linscan_rank = 1 the threshold is its distance and every list holds one pair"""
    rng = np.random.default_rng(4100)
    d, m = 8, 4
    K = (rng.standard_normal((m * H, d)) * 0.5).astype(np.float32)
    codes = rng.integers(0, H, size=(MANY_N, m), dtype=np.uint8)
    Q = rng.standard_normal((MANY_NQ, d)).astype(np.float32)
    recon = sum(K[j * H + codes[:, j].astype(np.int64)] for j in range(m))
    dbnorms = (recon.astype(np.float64) ** 2).sum(1).astype(np.float32)
    dbnorms[0] -= np.float32(1000.0)
    return Case("many_failed", "lsq", (codes, Q, K, dbnorms, m), MANY_NN, linscan_rank=1)


def many_failed_rows(case, q0, q1):
    """rows q0 .. q1 of its distance matrix by the numpy loop"""
    codes, Q, K, dbnorms, m = case.inputs
    return SM.lsq_dists_np(codes, Q[q0:q1], K, dbnorms, m)


MANY_TOP = 8


def many_failed_model(lib, case):
    """The model of this case without its 4100 x 65 537 matrix (a gigabyte, and minutes through numpy or through heaps of n entries): at rank 1 tau is
    the sample's minimum -- the host scan of the SAMPLED entries alone with nn = 1 -- and the pairs at or below it are among the MANY_TOP smallest of
    the whole scan (asserted: the last of them lies above tau, so the count is complete).  -> tau (f32), count, failed, (dists, ids 1-based) of nn"""
    codes, Q, K, dbnorms, m = case.inputs
    P = SM.plan(case.n, case.nn, rank=1)
    assert not P["exhaustive"] and P["r"] == 1
    s = np.arange(P["ns"]) * P["stride"]

    def scan(c, nrm, nn):
        c, nrm = np.ascontiguousarray(c), np.ascontiguousarray(nrm)
        dists, idx = np.zeros((case.nq, nn), np.float32), np.zeros((case.nq, nn), np.int32)
        rc = lib.lsq_linscan_aqd_query_extra_byte(dists.ctypes.data, idx.ctypes.data, c.ctypes.data, Q.ctypes.data, K.ctypes.data, nrm.ctypes.data,
                                                  case.nq, c.shape[0], m, H, Q.shape[1], nn, 0)
        assert rc == 0
        return dists, idx

    tau = scan(codes[s], dbnorms[s], 1)[0][:, 0]
    top_d, top_i = scan(codes, dbnorms, MANY_TOP)
    assert not np.isnan(top_d).any() and (top_d[:, -1] > tau).all()
    count = (top_d <= tau[:, None]).sum(axis=1).astype(np.int64)
    failed = (count > P["cap"]) | (count < case.nn)
    return P, tau, count, failed, (top_d[:, :case.nn].copy(), top_i[:, :case.nn].astype(np.int64))


# ---- d. non-finite distances --------------------------------------------------------------------------------------------------------------------------
def nonfinite_lsq(n, nq=5, seed=300):
    """NaN, +-Inf and -0.0 among the norms.  Small n: integer-valued codebooks and queries and four code values (massive ties).  Large n: Gaussian
    codebooks, and the non-finite norms rare enough that the lists of the thresholded road hold them (every NaN is appended) without overflowing"""
    rng = np.random.default_rng(seed + n)
    d, m = 6, 3
    small = n <= 1000
    if small:
        K = rng.integers(-2, 3, size=(m * H, d)).astype(np.float32)
        codes = rng.integers(0, 4, size=(n, m), dtype=np.uint8)
        Q = rng.integers(-2, 3, size=(nq, d)).astype(np.float32)
        dbnorms = rng.integers(0, 6, n).astype(np.float32)
    else:
        K = (rng.standard_normal((m * H, d)) * 0.5).astype(np.float32)
        codes = rng.integers(0, H, size=(n, m), dtype=np.uint8)
        Q = rng.standard_normal((nq, d)).astype(np.float32)
        dbnorms = (rng.standard_normal(n) ** 2).astype(np.float32)
    nan, pinf, ninf, nzero = (0.05, 0.05, 0.03, 0.12) if small else (0.0015, 0.05, 0.0001, 0.12)
    u = rng.random(n)
    dbnorms[u < nan] = np.nan
    dbnorms[(u >= nan) & (u < nan + pinf)] = np.inf
    dbnorms[(u >= nan + pinf) & (u < nan + pinf + ninf)] = -np.inf
    dbnorms[(u >= 0.5) & (u < 0.5 + nzero)] = -0.0
    return codes, Q, K, dbnorms, m


def nonfinite_pq(n, nq=5, seed=400):
    """+-Inf among the centres and the queries: (inf - inf)^2 is a NaN table entry, (inf - x)^2 a +Inf one.  Small n: integer values and eight code
    values (ties); large n: Gaussian values and every code value, so the queries with finite entries are served by their lists"""
    rng = np.random.default_rng(seed + n)
    m, subdim = 3, 2
    if n <= 1000:
        centers = rng.integers(-2, 3, size=(m, H, subdim)).astype(np.float32)
        codes = rng.integers(0, 8, size=(n, m), dtype=np.uint8)
        Q = rng.integers(-2, 3, size=(nq, m * subdim)).astype(np.float32)
    else:
        centers = rng.standard_normal((m, H, subdim)).astype(np.float32)
        codes = rng.integers(0, H, size=(n, m), dtype=np.uint8)
        Q = rng.standard_normal((nq, m * subdim)).astype(np.float32)
    centers[0, 1, 0] = np.inf
    centers[1, 2, 1] = -np.inf
    centers[2, 3, 0] = np.inf
    Q[1, 0] = np.inf            # query 1: NaN with code 1 in sub-space 0, +Inf with every other
    Q[2, 3] = np.inf            # query 2: +Inf everywhere (sub-space 1 holds -Inf and finite centres)
    Q[3, 4] = -np.inf           # query 3: +Inf everywhere
    return codes, centers, Q, m, subdim


NONFINITE_SMALL, NONFINITE_LARGE = 300, 70_001
NONFINITE_NN = {NONFINITE_SMALL: (1, 37, NONFINITE_SMALL), NONFINITE_LARGE: (37,)}


@functools.lru_cache(maxsize=None)
def nonfinite(producer, n, nn):
    inputs = nonfinite_lsq(n) if producer == "lsq" else nonfinite_pq(n)
    return Case("nonfinite_%s_n%d_nn%d" % (producer, n, nn), producer, inputs, nn)


# ---- e. the rounding boundaries of the records' id field ---------------------------------------------------------------------------------------------
IDBITS_N = (65_535, 65_536, 131_071, 131_072, 131_073)


@functools.lru_cache(maxsize=None)
def idbits(n, kind):
    """kind "lists": random data with the LAST entry the nearest of every query (its id n travels through the candidate lists where n is thresholded);
    kind "edge": zero codebooks and +Inf norms but for four small ones and FLT_MAX at the last entry -- the answer ends with (the largest finite key,
    the largest id), and the entry before it is among the answers too"""
    rng = np.random.default_rng(n)
    nq, nn, d, m = 3, 5, 8, 4
    codes = rng.integers(0, H, size=(n, m), dtype=np.uint8)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    if kind == "lists":
        K = (rng.standard_normal((m * H, d)) * 0.5).astype(np.float32)
        recon = sum(K[j * H + codes[:, j].astype(np.int64)] for j in range(m))
        dbnorms = (recon.astype(np.float64) ** 2).sum(1).astype(np.float32)
        dbnorms[n - 1] = np.float32(-1.0e4)
        dbnorms[n - 2] = FLT_MAX
    else:
        K = np.zeros((m * H, d), dtype=np.float32)
        dbnorms = np.full(n, np.inf, dtype=np.float32)
        dbnorms[[7, 100, 5000, n - 2]] = np.array([-3.0, 2.0, 2.0, 1.0e-3], dtype=np.float32)
        dbnorms[n - 1] = FLT_MAX
    return Case("idbits_%s_n%d" % (kind, n), "lsq", (codes, Q, K, dbnorms, m), nn)


def every_case():
    """(case, ranks) of everything the GPU file runs but `many_failed` (whose matrix comes in blocks of rows)"""
    out = [(crafted(name, m), RANKS) for name in DISTRIBUTION_NAMES for m in CRAFTED_M]
    out += [(mixed(p), (0,)) for p in ("lsq", "pq", "exact", "u8")]
    out += [(nonfinite(p, n, nn), (0,)) for p in ("lsq", "pq") for n, nns in NONFINITE_NN.items() for nn in nns]
    out += [(idbits(n, kind), (0,)) for n in IDBITS_N for kind in ("lists", "edge")]
    return out
