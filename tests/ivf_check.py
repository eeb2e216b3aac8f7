"""numpy restatement of the inverted-list search (lsq_ivf_search_cpu, lsq_index_search_ivf): the checker of tests/test_ivf.py and tests/test_gpu_ivf.py.

    probed lists  the nprobe smallest (coarse, list) pairs, coarse = knn_check.knn_dists' distance of the query's coarse row to the centroid
    table[e]      ((0 - (2 q_0) c_e0) - (2 q_1) c_e1) - ...        f32, k ascending, every op rounded
    dist(i)       (((0 + table[0 h + b_i0]) + table[1 h + b_i1]) + ...) + dbnorms[i]   [then + coarse(q, list of i) with add_coarse]
    result        the nn smallest (dist, id) pairs over the rows of the probed lists, ids 1-based original rows, NaN after every number, then (+inf, 0)"""
import numpy as np

from knn_check import knn_dists, order_keys

H = 256
ADD_COARSE, EVERY_RECORD, TEST_BATCH = 1, 2, 4


def adc_dists(codes, K, dbn, Qs):
    """(nq, n) f32 ADC distances by the scans' rule"""
    (n, m), (nq, d) = codes.shape, Qs.shape
    with np.errstate(invalid="ignore", over="ignore"):
        T = np.zeros((nq, K.shape[0]), dtype=np.float32)
        for k in range(d):
            T = T - (np.float32(2) * Qs[:, k, None]) * K[None, :, k]
        acc = np.zeros((nq, n), dtype=np.float32)
        for j in range(m):
            acc = acc + T[:, j * (K.shape[0] // m) + codes[:, j].astype(np.int64)]
        return acc + dbn[None, :]


def probes_np(cent, Qc, nprobe):
    """-> coarse (nq, nlist) f32, probes (nq, nprobe) list ids in rank order"""
    Dc = knn_dists(cent, Qc)
    keys = (order_keys(Dc).astype(np.uint64) << np.uint64(32)) | np.arange(cent.shape[0], dtype=np.uint64)[None, :]
    return Dc, (np.sort(keys, axis=1)[:, :nprobe] & np.uint64(0xFFFFFFFF)).astype(np.int64)


def ivf_np(codes, K, dbn, cent, lor, Qs, Qc, nprobe, nn, add_coarse=False):
    """-> dists (nq, nn) f32, ids (nq, nn) int32"""
    n, nq = codes.shape[0], Qs.shape[0]
    Dc, probes = probes_np(cent, Qc, nprobe)
    dist = adc_dists(codes, K, dbn, Qs)
    if add_coarse:
        with np.errstate(invalid="ignore", over="ignore"):
            dist = dist + Dc[:, lor]
    probed = np.zeros(Dc.shape, dtype=bool)
    probed[np.arange(nq)[:, None], probes] = True
    width = max(n, nn)                                                       # columns past n: the padding entries
    ok = np.zeros((nq, width), dtype=bool)
    ok[:, :n] = probed[:, lor]
    full = np.full((nq, width), np.float32(np.inf), dtype=np.float32)
    full[:, :n] = dist
    full = np.where(ok, full, np.float32(np.inf)).astype(np.float32)
    hi = order_keys(full).astype(np.uint64) | ((~ok).astype(np.uint64) << np.uint64(32))
    field = np.where(ok, np.arange(width)[None, :] + 1, 0)
    order = np.stack([np.lexsort((field[q], hi[q])) for q in range(nq)])[:, :nn]
    out_d = np.take_along_axis(full, order, axis=1)
    out_d[np.isnan(out_d)] = np.float32(np.nan)                              # the library hands out one NaN (0x7fc00000) whatever the payload
    return out_d, np.take_along_axis(field, order, axis=1).astype(np.int32)


def tail_hits_np(codes, K, dbn, cent, lor, Qs, Qc, nprobe, nn, add_coarse=False):
    """per query (rows of the head, rows of the tail, tail rows with !(dist > tau)): what the thresholded road appends, by the contract's definition
    of the head (the first probed lists, in rank order, that hold nn rows together) and of tau (the head's nn-th smallest distance)"""
    Dc, probes = probes_np(cent, Qc, nprobe)
    dist = adc_dists(codes, K, dbn, Qs)
    if add_coarse:
        dist = dist + Dc[:, lor]
    out = []
    for q in range(Qs.shape[0]):
        head, rows = [], 0
        for l in probes[q]:
            if rows >= nn:
                break
            head.append(l)
            rows += int((lor == l).sum())
        in_head = np.isin(lor, head)
        in_tail = np.isin(lor, probes[q][len(head):])
        if rows < nn:
            out.append((rows, 0, 0))
            continue
        head_d = dist[q, in_head]
        tau = head_d[np.argsort(order_keys(head_d), kind="stable")[nn - 1]]    # NaN sorts last: a NaN tau keeps every record
        with np.errstate(invalid="ignore"):
            out.append((rows, int(in_tail.sum()), int((~(dist[q, in_tail] > tau)).sum())))         # !(dist > tau): ties kept, a NaN on either side kept
    return out


def roads_np(hits, nn):
    """-> (tail_capacity, fall-back query numbers, records) of the thresholded road by the plan of DESIGN.md (inverted lists, "Plan"): a thresholded segment
    holds the longest head (at least nn records: a short head is padded) plus min(longest tail, 8 nn + 256) slots, never more than the longest query's rows; a
    query whose head and tail hits do not fit its segment is redone with every record.  records: what the segments held, the redone queries' second segments
    included.  hits: tail_hits_np's, with at least one non-empty tail"""
    max_rows = max(max(h[0] + h[1], nn) for h in hits)
    tail_cap = min(max(h[1] for h in hits), 8 * nn + 256)
    cap = min(max(max(h[0], nn) for h in hits) + tail_cap, max_rows)
    fallback = [q for q, h in enumerate(hits) if max(h[0], nn) + h[2] > cap]
    records = sum(min(max(h[0], nn) + h[2], cap) for h in hits) + sum(max(hits[q][0] + hits[q][1], nn) for q in fallback)
    return tail_cap, fallback, records


def ivf_cpu(lib, codes, K, dbn, cent, lor, Qs, Qc, nprobe, nn, flags=0, nthreads=0):
    """lsq_ivf_search_cpu on row arrays -> (rc, dists, ids)"""
    codes, K, dbn = np.ascontiguousarray(codes, dtype=np.uint8), np.ascontiguousarray(K, dtype=np.float32), np.ascontiguousarray(dbn, dtype=np.float32)
    cent, lor = np.ascontiguousarray(cent, dtype=np.float32), np.ascontiguousarray(lor, dtype=np.int32)
    Qs = np.ascontiguousarray(Qs, dtype=np.float32)
    Qc = None if Qc is None else np.ascontiguousarray(Qc, dtype=np.float32)
    (n, m), (nq, d) = codes.shape, Qs.shape
    dists, ids = np.zeros((nq, nn), dtype=np.float32), np.zeros((nq, nn), dtype=np.int32)
    rc = lib.lsq_ivf_search_cpu(dists.ctypes.data, ids.ctypes.data, codes.ctypes.data, K.ctypes.data, dbn.ctypes.data, cent.ctypes.data, lor.ctypes.data,
                                Qs.ctypes.data, None if Qc is None else Qc.ctypes.data, n, m, K.shape[0] // m, d, cent.shape[0], nq, d, nprobe, nn,
                                flags, nthreads)
    return rc, dists, ids


def skewed_lists(rng, n, nlist):
    """lists 1, 2 (and the last) empty, lists 3, 4 one row each, list 0 half of the rows (longer than one block pass), the others random"""
    if nlist < 7:
        return rng.integers(0, nlist, n).astype(np.int32) if nlist > 1 else np.zeros(n, dtype=np.int32)
    lor = rng.integers(5, nlist - 1, n).astype(np.int32)
    perm = rng.permutation(n)
    lor[perm[:n // 2]] = 0
    lor[perm[n // 2]], lor[perm[n // 2 + 1]] = 3, 4
    return lor


def problem(n, d, m, nlist, nq, seed, small_int=False, lists="skewed"):
    """codes, K, dbnorms, centroids, list_of_row, Q_scan, Q_coarse of a quantised base with a coarse partition laid over it"""
    rng = np.random.default_rng(seed)
    if small_int:                                                            # exact ties: every table entry and every norm is a small integer
        K = rng.integers(-2, 3, (m * H, d)).astype(np.float32)
        Qs = rng.integers(-2, 3, (nq, d)).astype(np.float32)
        cent = rng.integers(-2, 3, (nlist, d)).astype(np.float32)
    else:
        K = (rng.standard_normal((m * H, d)) / np.sqrt(m)).astype(np.float32)
        Qs = rng.standard_normal((nq, d)).astype(np.float32)
        cent = rng.standard_normal((nlist, d)).astype(np.float32)
    codes = rng.integers(0, H, (n, m)).astype(np.uint8)
    recon = sum(K[j * H + codes[:, j].astype(np.int64)] for j in range(m))
    dbn = (recon.astype(np.float64) ** 2).sum(1).astype(np.float32)
    lor = skewed_lists(rng, n, nlist) if lists == "skewed" else (np.arange(n) % nlist).astype(np.int32) if lists == "even" else \
        rng.integers(0, nlist, n).astype(np.int32)
    Qc = (Qs + np.float32(0.25) * rng.standard_normal((nq, d)).astype(np.float32)) if not small_int else Qs.copy()
    return codes, K, dbn, cent, lor, Qs, Qc


# (d, m, nlist, nprobe, nn, nq): every value of the issue's grid at least once; m = 8, 16 take the dword loader, 1 and 7 the byte loader; the last four:
# m = 4 and 12 (the one- and three-dword loaders; at m = 12 the tables come in 8-query tiles, which 37 queries cross), m = 2 and 15 (byte loader)
SHAPES = [(5, 1, 1, 1, 1, 1), (32, 7, 7, 3, 10, 37), (32, 8, 40, 3, 300, 37), (5, 16, 40, 40, 10, 37), (32, 8, 7, 7, 300, 1), (5, 7, 40, 1, 1, 37),
          (32, 16, 7, 1, 300, 37), (32, 8, 40, 40, 1, 37), (5, 8, 7, 3, 10, 1), (32, 1, 40, 3, 10, 37), (5, 16, 1, 1, 300, 37), (32, 7, 40, 40, 300, 1),
          (32, 4, 40, 3, 10, 37), (32, 12, 40, 3, 300, 37), (5, 2, 7, 3, 10, 37), (32, 15, 40, 40, 10, 37)]
N = 3000


# ---- named problems: each returns (the seven arrays of problem(), nprobe, nn).  tests/test_ivf.py holds lsq_ivf_search_cpu to ivf_np on each,
# tests/test_gpu_ivf.py the device to lsq_ivf_search_cpu and its road counts to tail_hits_np / roads_np ------------------------------------------------
SCAN_BLOCKS = 2048                                                           # the scan gives a query min(ceil(SCAN_BLOCKS / queries of the batch), nprobe) blocks


def scan_splits(nqb, nprobe):
    return min(-(-SCAN_BLOCKS // nqb), nprobe)


def stride_problem(which):
    """more (query, list) pairs than SCAN_BLOCKS: a block walks several lists with one staged table.  "m8": 300 queries, 40 of 40 skewed lists, 7 blocks
    per query (5 or 6 lists each); every query has a tail of up to 1333 hits, and none overflows: segments are sized by the longest head, and some
    query's head holds the 1500-row list.  "m12": 128 queries, 33 of 64 lists, 16 blocks per query (2 or 3 lists each); 59 queries overflow, 69 do not"""
    d, m, nlist, nprobe, nn, nq = {"m8": (32, 8, 40, 40, 10, 300), "m12": (32, 12, 64, 33, 10, 128)}[which]
    return problem(N, d, m, nlist, nq, 94 + m, lists="skewed"), nprobe, nn


def _even(d, m, nq, seed, small_int=False):
    """3000 rows, 40 lists of 75: row i is the (i // 40)-th row of list i % 40"""
    return problem(N, d, m, 40, nq, seed, small_int=small_int, lists="even")


def capacity_problem(t):
    """every probed row has the same code row; the first t rows of every list have norm 1, the others 2 + (position in the list).  nn = 1: the head is the
    nearest list, tau its norm-1 rows' distance, and exactly t rows of each of the 8 tail lists tie it (small integers: every sum exact).  8 t = 264 at
    t = 33 is the tail's capacity 8 nn + 256 to the record; t = 34 is 8 over"""
    codes, K, dbn, cent, lor, Qs, Qc = _even(5, 8, 37, 92, small_int=True)
    codes[:] = codes[0]
    at = np.arange(N) // 40
    dbn[:] = np.where(at < t, 1, 2 + at).astype(np.float32)
    return (codes, K, dbn, cent, lor, Qs, Qc), 9, 1


def _two_groups(seed):
    """the even layout with lists 0 .. 19 far from lists 20 .. 39; even queries probe the first group alone, odd queries the second"""
    codes, K, dbn, cent, lor, Qs, Qc = _even(32, 8, 37, seed)
    cent[:20] += np.float32(10)
    cent[20:] -= np.float32(10)
    rng = np.random.default_rng(seed + 1000)
    near = rng.integers(0, 20, 37) + 20 * (np.arange(37) % 2)
    Qc[:] = cent[near] + np.float32(0.25) * rng.standard_normal((37, 32)).astype(np.float32)
    return codes, K, dbn, cent, lor, Qs, Qc


def mixed_problem():
    """every row of lists 0 .. 19 is row 0 again: the 19 even queries' 7 x 75 tail rows all tie tau and overflow, the 18 odd queries see random rows and do
    not.  With TEST_BATCH the failed queries 0, 2, .. 36 are three fall-back batches (8, 8, 3) of a non-contiguous selection"""
    codes, K, dbn, cent, lor, Qs, Qc = _two_groups(93)
    first = lor < 20
    codes[first] = codes[0]
    dbn[first] = dbn[0]
    return (codes, K, dbn, cent, lor, Qs, Qc), 8, 1


def nan_tau_problem():
    """NaN norms in all of lists 0 .. 19: an even query's head has no number, its tau is NaN and every tail record is kept (and overflows); a sprinkling of
    +inf and -inf norms in lists 20 .. 39, where the odd queries search"""
    codes, K, dbn, cent, lor, Qs, Qc = _two_groups(95)
    dbn[lor < 20] = np.float32(np.nan)
    second = np.flatnonzero(lor >= 20)
    dbn[second[3::29]] = np.float32(np.inf)
    dbn[second[11::31]] = np.float32(-np.inf)
    return (codes, K, dbn, cent, lor, Qs, Qc), 8, 5


def short_list_problem():
    """one probed list of four rows against nn = 10, their distances a number, -inf, +inf and NaN: the real +inf row and the NaN row come before the
    (+inf, 0) padding records, which only the bit above the key tells from a real +inf"""
    codes, K, dbn, cent, lor, Qs, Qc = problem(N, 32, 8, 40, 5, 3)
    lor[:] = 0
    lor[:4] = 3
    dbn[1:4] = np.array([-np.inf, np.inf, np.nan], dtype=np.float32)
    cent[3] = 1000.0
    Qc[:] = 1000.0
    return (codes, K, dbn, cent, lor, Qs, Qc), 1, 10


def layout_problem(n, nlist):
    """lists 0, 1, 2 and the last three empty (list 0 empty: the first sorted position opens four lists at once; runs of three empty lists), nlist at a
    power of two and one above, n at a power of two (the id n needs the top bit of the record's id field) and one below.  The last row is made the strictly
    nearest row of query 0: the best probed row again, with a smaller norm"""
    codes, K, dbn, cent, lor, Qs, Qc = problem(n, 32, 8, nlist, 37, 96 + nlist, lists="random")
    lor[:] = 3 + lor % (nlist - 6)
    nprobe, nn = 12, 10
    best = int(ivf_np(codes, K, dbn, cent, lor, Qs[:1], Qc[:1], nprobe, 1)[1][0, 0]) - 1
    codes[n - 1], lor[n - 1], dbn[n - 1] = codes[best], lor[best], dbn[best] - np.float32(1)
    return (codes, K, dbn, cent, lor, Qs, Qc), nprobe, nn


# ---- many lists: nlist from 65 536 up, where the coarse search leaves the exhaustive road (tests/select_model.py, plan) and nlist >> n -----------------
MANY = 65537                                                                 # ADC_SMALL_N + 1: the first nlist whose coarse search samples and bets


def padding_ok(ids):
    """the condition of every many-lists case, on the CHECKER's ids: at most a quarter of the result slots are padding (id 0) and no query is all
    padding -- a case cannot pass by comparing infinities"""
    ids = np.asarray(ids)
    return bool((ids == 0).sum() * 4 <= ids.size and np.all((ids != 0).any(axis=1)))


def many_lists_problem():
    """262 148 rows on 65 537 random lists (about 4 each), 64 probed: heads of 10 .. 15 rows, tails of about 240, none overflowing"""
    return problem(262148, 8, 8, MANY, 37, seed=5, lists="random"), 64, 10


def near_lists(cent, Qc, n, nprobe, scatter=5, seed=0):
    """list_of_row for nlist >> n: row i lies in the ((i // nq) % nprobe)-th nearest list of query i % nq by the host exact search (lsq_knn_exact_cpu),
    so that the probed lists hold rows at all; every scatter-th row goes to a random list instead, one row is forced into list 0 and one into the last"""
    import importlib
    lsq = importlib.import_module("local-search-quantization_amd")
    nlist, nq = cent.shape[0], Qc.shape[0]
    ids = lsq.knn_exact(np.ascontiguousarray(cent.T), np.ascontiguousarray(Qc.T), nprobe)[1].T.astype(np.int64) - 1      # (nq, nprobe), 0-based
    i = np.arange(n)
    lor = ids[i % nq, (i // nq) % nprobe].astype(np.int32)
    lor[::scatter] = np.random.default_rng(seed).integers(0, nlist, lor[::scatter].shape[0])
    lor[1], lor[2] = 0, nlist - 1
    return lor


def coarse_stats(cent, Qc, nprobe, **plan_args):
    """what the coarse step of a search -- the exact search of Qc on the centroids for nprobe neighbours -- must decide, by the model of the selection
    (select_model.predict): exhaustive, threshold_rank, list_capacity, fallback_queries, candidates, batches"""
    import select_model as SM
    return SM.predict(knn_dists(cent, Qc), nprobe, **plan_args)["stats"]


def list_edge_problem(nlist, n=2048):
    """layout_problem's pattern at the values where the grouping sort's list bits change (8 -> 9 at 257, 16 -> 17 at 65 537): lists 0, 1, 2 and the last
    three empty, the last row (id n, a power of two) the nearest of query 0.  From 65 536 on the rows are placed by near_lists and the ends cleared"""
    if nlist <= 1024:
        return layout_problem(n, nlist)
    codes, K, dbn, cent, lor, Qs, Qc = problem(n, 32, 8, nlist, 37, 96 + nlist, lists="random")
    nprobe, nn = 12, 10
    lor = np.clip(near_lists(cent, Qc, n, nprobe), 3, nlist - 4).astype(np.int32)
    best = int(ivf_np(codes, K, dbn, cent, lor, Qs[:1], Qc[:1], nprobe, 1)[1][0, 0]) - 1
    codes[n - 1], lor[n - 1], dbn[n - 1] = codes[best], lor[best], dbn[best] - np.float32(1)
    return (codes, K, dbn, cent, lor, Qs, Qc), nprobe, nn


def many_probes_problem():
    """nprobe = 1024 of 65 537 lists, nn = 100, 5 queries: the coarse plan is r = 352, cap = 3200 (select_model.plan(65537, 1024))"""
    codes, K, dbn, cent, lor, Qs, Qc = problem(8192, 8, 8, MANY, 5, seed=13, lists="random")
    return (codes, K, dbn, cent, near_lists(cent, Qc, 8192, 1024), Qs, Qc), 1024, 100


def duplicated_centroids_problem():
    """40 000 centroids equal to 0.5 * Qc[0]: they tie at query 0's coarse threshold, its candidate list overflows and the coarse search redoes that
    query alone (a mixed coarse batch); the ties go to the smaller list id"""
    codes, K, dbn, cent, lor, Qs, Qc = problem(20000, 8, 8, MANY, 37, seed=12, lists="random")
    cent[5000:45000] = np.float32(0.5) * Qc[0]
    return (codes, K, dbn, cent, lor, Qs, Qc), 32, 10


BOUND = 1 << 24                                                              # the contract's largest nlist


def bound_problem(nlist=BOUND):
    """nlist >> n: 4096 rows on 2^24 lists, d = 2, placed by near_lists"""
    codes, K, dbn, cent, lor, Qs, Qc = problem(4096, 2, 8, nlist, 8, seed=11, lists="random")
    return (codes, K, dbn, cent, near_lists(cent, Qc, 4096, 16), Qs, Qc), 16, 10


PROBLEMS = {"stride-m8": lambda: stride_problem("m8"), "stride-m12": lambda: stride_problem("m12"), "capacity-33": lambda: capacity_problem(33),
            "capacity-34": lambda: capacity_problem(34), "mixed": mixed_problem, "nan-tau": nan_tau_problem, "short-list": short_list_problem,
            "layout-n2047-nlist64": lambda: layout_problem(2047, 64), "layout-n2048-nlist64": lambda: layout_problem(2048, 64),
            "layout-n2047-nlist65": lambda: layout_problem(2047, 65), "layout-n2048-nlist65": lambda: layout_problem(2048, 65)}
