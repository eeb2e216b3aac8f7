"""numpy restatement of the search SELECTION of csrc/lsq_adc.hip: the model that tests/test_select_model.py and tests/test_gpu_select_model.py hold the
plan, the thresholds, the candidate counts and the answers of all four distance producers to.  It imports no GPU code.

    plan      make_plan: ns = 16384 sampled entries i = s * stride, stride = n // ns; the threshold rank r and the list capacity cap; exhaustive for
              n <= 65536, r >= 0.25 ns or cap >= 0.5 n; option linscan_rank replaces r (clamped to ns) on the thresholded road only
    tau       the r-th smallest order-preserving key among the query's ns sample distances (adc_rank_select_kernel)
    count     the entries with not (dist > unkey(tau)): a NaN on either side counts (MODE 0 of the scans)
    failed    count > cap or count < nn: the query is redone by the exhaustive road (adc_segments_kernel, lsq_adc_search)
    totals    fallback_queries = failed.sum(), candidates = count.sum() + n * failed.sum(), batches as lsq_adc_search cuts them
    answer    the nn smallest (key, id) records of a row, NaN last and as the one NaN 0x7fc00000 (`select`)

`predict` takes the full (nq, n) f32 distance matrix D of a call; the full_matrix_* helpers rebuild D for each producer from the host forms that the
reference pins (called with nn = n, scattered back by id) or, where that is too slow, from numpy loops in the contract's op order.

MUTANTS are one-slip copies of the model: the proof that the inputs of the GPU tests can tell a wrong selection from a right one."""
import math

import numpy as np

import knn_check as KC

NS = 16384                 # ADC_SAMPLE
SMALL_N = 65536            # ADC_SMALL_N
BATCH_ITEMS = 1 << 28      # records per key buffer of one batch
H = 256
NAN_KEY = np.uint32(0xFFFFFFFF)
NAN_BITS = np.uint32(0x7FC00000)


def unkey(keys):
    """f32 distances of order keys (KC.order_keys' inverse; the NaN key gives the one NaN 0x7fc00000)"""
    k = np.asarray(keys, dtype=np.uint32)
    b = np.where(k >> 31 == 1, k ^ np.uint32(0x80000000), ~k).astype(np.uint32)
    return np.where(k == NAN_KEY, NAN_BITS, b).astype(np.uint32).view(np.float32)


def plan(n, nn, force_exhaustive=0, rank=0, round_cap=True):
    """make_plan and the rank hook of lsq_adc_search -> dict(exhaustive, ns, stride, r, cap).  (round_cap=False: a mutant's plan.)"""
    p = dict(exhaustive=bool(force_exhaustive) or n <= SMALL_N, ns=NS, stride=n // NS, r=0, cap=n)
    if p["exhaustive"]:
        return p
    ks = float(nn) * NS / float(n)
    r = ks + 5.6 * math.sqrt(ks) + 6.0
    cap = (r + 8.0 * math.sqrt(r) + 32.0) * (float(n) / NS) + nn
    if r >= 0.25 * NS or cap >= 0.5 * n:
        p["exhaustive"] = True
        return p
    p["r"] = int(math.ceil(r))
    p["cap"] = (int(cap) + 63) & ~63 if round_cap else int(cap)
    if rank > 0:
        p["r"] = min(int(rank), NS)
    return p


def _batch(per_query, most=None):
    qb = max(1, BATCH_ITEMS // per_query)
    if most is not None:
        qb = min(qb, most)
    return qb & ~15 if qb > 16 else qb


def batches(P, n, nq, nfailed):
    """the batches of one call: queries per batch from the size of a key buffer (at most 16384 on the first pass), then the fallback's batches"""
    qb = _batch(n if P["exhaustive"] else max(P["cap"], P["ns"]), 16384)
    return -(-nq // qb) + (-(-nfailed // _batch(n)) if nfailed else 0)


def predict_rows(D, nn, P, dr=0, strict=False, nan_emits=True, sample_offset=0):
    """per query of D (rows, n): tau (u32 key), count, failed on the thresholded plan P.  The keyword arguments are the mutants' slips."""
    D = np.asarray(D, dtype=np.float32)
    n = D.shape[1]
    s = (np.arange(P["ns"], dtype=np.int64) * P["stride"] + sample_offset) % n
    keys = np.sort(KC.order_keys(D[:, s]), axis=1)
    r = min(max(P["r"] + dr, 1), P["ns"])
    tau = keys[:, r - 1]
    t = unkey(tau)[:, None]
    with np.errstate(invalid="ignore"):
        if strict:
            hit = ~(D >= t)
        elif nan_emits:
            hit = ~(D > t)
        else:
            hit = D <= t
    count = hit.sum(axis=1).astype(np.int64)
    failed = (count > P["cap"]) | (count < nn)
    return tau, count, failed


def totals(P, n, nq, count=None, failed=None):
    """the call's statistics as lsq_adc_search reports them, from the per-query counts (thresholded road) or from the plan alone (exhaustive)"""
    out = dict(exhaustive=int(P["exhaustive"]), threshold_rank=P["r"], list_capacity=P["cap"], queries=nq, codes=n)
    if P["exhaustive"]:
        out.update(fallback_queries=0, candidates=nq * n, batches=batches(P, n, nq, 0))
    else:
        nf = int(failed.sum())
        out.update(fallback_queries=nf, candidates=int(count.sum()) + n * nf, batches=batches(P, n, nq, nf))
    return out


def predict(D, nn, _slips=None, **plan_args):
    """-> dict(plan, tau, count, failed (None on the exhaustive road), stats): what one call on the distance matrix D (nq, n) must decide and report"""
    slips = dict(_slips or {})
    nq, n = D.shape
    P = plan(n, nn, round_cap=slips.pop("round_cap", True), **plan_args)
    if P["exhaustive"]:
        return dict(plan=P, tau=None, count=None, failed=None, stats=totals(P, n, nq))
    tau, count, failed = predict_rows(D, nn, P, **slips)
    return dict(plan=P, tau=tau, count=count, failed=failed, stats=totals(P, n, nq, count, failed))


def select(D, nn, id_base=0):
    """-> dists (nq, nn) f32, ids (nq, nn) int64 = row index + id_base: the nn smallest (key, id) records of each row of D, NaN last and as 0x7fc00000
    (KC.knn_select with the id base as a parameter)"""
    dists, ids = KC.knn_select(np.asarray(D, dtype=np.float32), nn)
    return dists, ids.astype(np.int64) + id_base


# (name, the slip): predict(D, nn, _slips=slip, ...) is the wrong model
MUTANTS = [
    ("rank_minus_one", dict(dr=-1)),                    # the (r - 1)-th smallest sample key
    ("rank_plus_one", dict(dr=+1)),                     # the (r + 1)-th
    ("strict_compare", dict(strict=True)),              # dist < tau appended, a tie with tau dropped
    ("nan_not_emitted", dict(nan_emits=False)),         # dist <= tau as written: false for a NaN on either side
    ("sample_off_by_one_row", dict(sample_offset=1)),   # the sample reads i = s * stride + 1
    ("cap_not_rounded", dict(round_cap=False)),         # the capacity without its round-up to 64
]


def mutant_stats(D, nn, slip, **plan_args):
    st = predict(D, nn, _slips=slip, **plan_args)["stats"]
    return st["fallback_queries"], st["candidates"]


# ---- the distance matrix of each producer ------------------------------------------------------------------------------------------------------------
def _scatter(dists, ids, id_base):
    """(nq, n) results of a host form called with nn = n -> D with D[q, id - id_base] = dist"""
    nq, n = dists.shape
    D = np.empty((nq, n), dtype=np.float32)
    cols = ids.astype(np.int64) - id_base
    assert all(np.array_equal(np.sort(c), np.arange(n)) for c in cols), "the host form did not return every id once"
    np.put_along_axis(D, cols, dists, axis=1)
    return D


def full_matrix_lsq(lib, codes, Q, K, dbnorms, m):
    """lsq_linscan_aqd_query_extra_byte with nn = n"""
    n, (nq, d) = codes.shape[0], Q.shape
    codes, Q, K, dbnorms = (np.ascontiguousarray(a) for a in (codes, Q, K, dbnorms))
    dists, idx = np.zeros((nq, n), np.float32), np.zeros((nq, n), np.int32)
    rc = lib.lsq_linscan_aqd_query_extra_byte(dists.ctypes.data, idx.ctypes.data, codes.ctypes.data, Q.ctypes.data, K.ctypes.data, dbnorms.ctypes.data,
                                              nq, n, m, H, d, n, 0)
    assert rc == 0
    return _scatter(dists, idx, 1)


def full_matrix_pq(lib, codes, centers, Q, m, subdim):
    """lsq_linscan_aqd_query with K = N"""
    n, nq = codes.shape[0], Q.shape[0]
    codes, centers, Q = (np.ascontiguousarray(a) for a in (codes, centers, Q))
    dists, res = np.zeros((nq, n), np.float32), np.zeros((nq, n), np.uint32)
    rc = lib.lsq_linscan_aqd_query(dists.ctypes.data, res.ctypes.data, codes.ctypes.data, centers.ctypes.data, Q.ctypes.data, n, nq, 8 * m, n,
                                   codes.shape[1], Q.shape[1], subdim)
    assert rc == 0
    return _scatter(dists, res, 0)


def full_matrix_exact(lib, Xb, Xq):
    """lsq_knn_exact_cpu with nn = n"""
    rc, dists, ids = KC.knn_cpu(lib, Xb, Xq, Xq.shape[1], Xb.shape[0])
    assert rc == 0
    return _scatter(dists, ids, 0)


def full_matrix_exact_u8(lib, Xb, Xq):
    """lsq_knn_exact_u8_cpu on uint8 rows and uint8 queries with nn = n"""
    Xb, Xq = np.ascontiguousarray(Xb, dtype=np.uint8), np.ascontiguousarray(Xq, dtype=np.uint8)
    (n, d), nq = Xb.shape, Xq.shape[0]
    dists, ids = np.zeros((nq, n), np.float32), np.zeros((nq, n), np.uint32)
    rc = lib.lsq_knn_exact_u8_cpu(dists.ctypes.data, ids.ctypes.data, Xb.ctypes.data, 1, Xq.ctypes.data, 1, n, nq, d, d, d, n, 0)
    assert rc == 0
    return _scatter(dists, ids, 0)


def lsq_dists_np(codes, Q, K, dbnorms, m):
    """the LSQ scan's distances by a numpy loop in the contract's op order (csrc/lsq_linscan.hip's header): where nn = n through the host form is too slow"""
    Q, K = np.asarray(Q, dtype=np.float32), np.asarray(K, dtype=np.float32)
    nq, d = Q.shape
    with np.errstate(invalid="ignore", over="ignore"):
        tab = np.zeros((nq, m * H), dtype=np.float32)
        for k in range(d):
            tab = tab - (np.float32(2) * Q[:, k, None]) * K[None, :, k]
        acc = np.zeros((nq, codes.shape[0]), dtype=np.float32)
        for j in range(m):
            acc = acc + tab[:, j * H + codes[:, j].astype(np.int64)]
        return acc + np.asarray(dbnorms, dtype=np.float32)[None, :]
