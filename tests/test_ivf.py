"""The inverted-list search without a GPU: the host checker lsq_ivf_search_cpu against the numpy statement of the contract (tests/ivf_check.py) and against
the exhaustive host scan, the boundary (header, binding, version), and every argument the library refuses before it needs a device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivf_check as ic  # noqa: E402
from knn_check import same_bits  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 256


def test_boundary_declares_exports_and_binds_the_four_symbols(lsq):
    hdr = open(os.path.join(ROOT, "include", "lsq_mi355x.h")).read()
    assert int(re.search(r"#define LSQ_VERSION (\d+)", hdr).group(1)) >= 1700
    L, tun = lsq._lib.load(), lsq._lib.load(tuning=True)
    assert L.lsq_version() >= 1700
    for s in ("lsq_index_set_lists", "lsq_index_search_ivf", "lsq_index_get_ivf_info", "lsq_ivf_search_cpu"):
        assert re.search(r"LSQ_API int %s\(" % s, hdr), s
        assert s in lsq._lib.SIGNATURES and hasattr(L, s) and hasattr(tun, s)
    assert re.search(r"LSQ_IVF_ADD_COARSE = 1, LSQ_IVF_EVERY_RECORD = 2", hdr)
    assert (lsq._lib.IVF_ADD_COARSE, lsq._lib.IVF_EVERY_RECORD) == (ic.ADD_COARSE, ic.EVERY_RECORD) == (1, 2)
    # the info struct of the binding has the header's fields, in order
    body = re.search(r"typedef struct lsq_ivf_info \{(.*?)\} lsq_ivf_info;", hdr, flags=re.S).group(1)
    fields = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in lsq._lib.IvfInfo._fields_]
    for name in ("ivf_assign", "train_coarse", "ivf_residual_norms"):
        assert callable(getattr(lsq, name))
    assert all(hasattr(lsq.Index, f) for f in ("set_lists", "search_ivf", "ivf_info"))


@pytest.mark.parametrize("shape", ic.SHAPES, ids=lambda s: "d%d-m%d-nlist%d-nprobe%d-nn%d-nq%d" % s)
@pytest.mark.parametrize("add", [False, True], ids=["plain", "add_coarse"])
def test_host_checker_returns_the_numpy_contract(lsq, shape, add):
    d, m, nlist, nprobe, nn, nq = shape
    p = ic.problem(ic.N, d, m, nlist, nq, 7 + sum(shape))
    p[2][5::97] = np.float32(np.nan)                                         # NaN norms: after every number, before the padding
    rc, dd, di = ic.ivf_cpu(lsq._lib.load(), *p, nprobe, nn, flags=ic.ADD_COARSE if add else 0)
    assert rc == 0, lsq._lib.load().lsq_last_error()
    rd, ri = ic.ivf_np(*p, nprobe, nn, add_coarse=add)
    assert same_bits(dd, rd) and np.array_equal(di, ri)
    # one thread and all of them: the same result
    rc1, d1, i1 = ic.ivf_cpu(lsq._lib.load(), *p, nprobe, nn, flags=ic.ADD_COARSE if add else 0, nthreads=1)
    assert rc1 == 0 and same_bits(d1, dd) and np.array_equal(i1, di)


@pytest.mark.parametrize("name", list(ic.PROBLEMS))
def test_host_checker_returns_the_numpy_contract_on_the_named_problems(lsq, name):
    """the chain tests/test_gpu_ivf.py rests on: the device is held to lsq_ivf_search_cpu, which is held to ivf_np here, with and without the coarse add"""
    p, nprobe, nn = ic.PROBLEMS[name]()
    for add in (False, True):
        rc, dd, di = ic.ivf_cpu(lsq._lib.load(), *p, nprobe, nn, flags=ic.ADD_COARSE if add else 0)
        assert rc == 0, lsq._lib.load().lsq_last_error()
        rd, ri = ic.ivf_np(*p, nprobe, nn, add_coarse=add)
        assert same_bits(dd, rd) and np.array_equal(di, ri), (name, add)


def test_named_problems_are_what_their_names_say():
    """what the device tests take for granted of the builders, from the numpy checker alone: which queries overflow their tails, by how much, and why"""
    for name, splits in (("stride-m8", 7), ("stride-m12", 16)):
        p, nprobe, nn = ic.PROBLEMS[name]()
        hits = ic.tail_hits_np(*p, nprobe, nn)
        assert p[5].shape[0] * nprobe > ic.SCAN_BLOCKS and ic.scan_splits(p[5].shape[0], nprobe) == splits < nprobe and all(h[1] > 0 for h in hits)
    assert 0 < len(ic.roads_np(hits, nn)[1]) < p[5].shape[0]                 # stride-m12: some queries overflow, some do not
    for t, over in ((33, 0), (34, 37)):
        p, nprobe, nn = ic.capacity_problem(t)
        hits = ic.tail_hits_np(*p, nprobe, nn)
        cap, fallback, records = ic.roads_np(hits, nn)
        assert cap == 264 and all(h == (75, 600, 8 * t) for h in hits) and len(fallback) == over
        assert over or records == 37 * (75 + 264)
    p, nprobe, nn = ic.mixed_problem()
    hits = ic.tail_hits_np(*p, nprobe, nn)
    assert ic.roads_np(hits, nn)[:2] == (264, list(range(0, 37, 2))) and all(h[2] == 525 for h in hits[0::2]) and max(h[2] for h in hits[1::2]) <= 264
    p, nprobe, nn = ic.nan_tau_problem()
    rd, ri = ic.ivf_np(*p, nprobe, nn)
    for add in (False, True):
        hits = ic.tail_hits_np(*p, nprobe, nn, add_coarse=add)
        assert ic.roads_np(hits, nn)[:2] == (296, list(range(0, 37, 2))) and all(h[2] == h[1] == 525 for h in hits[0::2])
    assert np.all(np.isnan(rd[0::2])) and np.all(ri[0::2] > 0) and np.all(np.isneginf(rd[1::2, 0])) and not np.any(np.isnan(rd[1::2]))
    assert np.any(np.isposinf(p[2][p[4] >= 20])) and np.any(np.isneginf(p[2][p[4] >= 20]))
    p, nprobe, nn = ic.short_list_problem()
    rd, ri = ic.ivf_np(*p, nprobe, nn)
    assert np.array_equal(ri, np.tile([2, 1, 3, 4, 0, 0, 0, 0, 0, 0], (5, 1)))
    assert np.all(np.isneginf(rd[:, 0]) & np.isfinite(rd[:, 1]) & np.isposinf(rd[:, 2]) & np.isnan(rd[:, 3])) and np.all(np.isposinf(rd[:, 4:]))
    for n in (2047, 2048):
        for nlist in (64, 65):
            p, nprobe, nn = ic.layout_problem(n, nlist)
            counts = np.bincount(p[4], minlength=nlist)
            assert not counts[:3].any() and not counts[-3:].any() and counts[3:-3].all() and p[0].shape[0] == n and p[3].shape[0] == nlist
            assert ic.ivf_np(*p, nprobe, nn)[1][0, 0] == n and n in ic.ivf_np(*p, nprobe, nn, add_coarse=True)[1][0]


# ---- many lists: the problems of tests/test_gpu_many_lists.py, from the checkers alone ---------------------------------------------------------------
def _checked(lsq, p, nprobe, nn, numpy=True):
    """lsq_ivf_search_cpu on the problem, with and without the coarse add: the padding condition, and (numpy) ivf_np's bits"""
    for add in (False, True):
        rc, dd, di = ic.ivf_cpu(lsq._lib.load(), *p, nprobe, nn, flags=ic.ADD_COARSE if add else 0)
        assert rc == 0 and ic.padding_ok(di), (add, int((di == 0).sum()))
        if numpy:
            rd, ri = ic.ivf_np(*p, nprobe, nn, add_coarse=add)
            assert same_bits(dd, rd) and np.array_equal(di, ri), add
    return di


def test_padding_condition_refuses_results_that_compare_infinities():
    assert ic.padding_ok(np.array([[1, 2, 3, 0], [4, 5, 6, 7]])) and not ic.padding_ok(np.array([[1, 2, 0, 0], [4, 5, 6, 0]]))
    assert not ic.padding_ok(np.array([[0], [1], [2], [3], [4]]))                 # under a quarter, but one query is all padding


def test_many_lists_problem_is_what_its_name_says(lsq):
    """65 537 lists of about four rows, 64 probed: the three numbers of roads_np are pinned, so that the problem cannot drift into one that tests nothing"""
    p, nprobe, nn = ic.many_lists_problem()
    assert p[0].shape == (262148, 8) and p[3].shape == (ic.MANY, 8) and (nprobe, nn) == (64, 10)
    di = _checked(lsq, p, nprobe, nn)
    assert not np.any(di == 0)                                               # no slot is padding
    hits = ic.tail_hits_np(*p, nprobe, nn)
    assert min(h[0] for h in hits) == 10 and max(h[0] for h in hits) == 15 and 200 < min(h[1] for h in hits) and max(h[1] for h in hits) == 276
    assert ic.roads_np(hits, nn) == (276, [], 7809)
    # the coarse step by the model of the selection: the sampled road, rank 45, lists of 640; the options send it down the other two roads
    st = ic.coarse_stats(p[3], p[6], nprobe)
    assert (st["exhaustive"], st["threshold_rank"], st["list_capacity"]) == (0, 45, 640) and 0 <= st["fallback_queries"] < 37
    assert ic.coarse_stats(p[3], p[6], nprobe, rank=1)["fallback_queries"] == 37 and ic.coarse_stats(p[3], p[6], nprobe, force_exhaustive=1)["exhaustive"] == 1


@pytest.mark.parametrize("nlist", [256, 257, 65536, 65537])
def test_list_edge_problems_keep_the_layout_pattern(lsq, nlist):
    p, nprobe, nn = ic.list_edge_problem(nlist)
    counts = np.bincount(p[4], minlength=nlist)
    assert p[3].shape[0] == nlist and p[0].shape[0] == 2048 and not counts[:3].any() and not counts[-3:].any()
    assert nlist < 65536 or (counts == 0).sum() > 64000                      # nlist >> n: runs of thousands of empty lists
    _checked(lsq, p, nprobe, nn)
    assert ic.ivf_np(*p, nprobe, nn)[1][0, 0] == 2048                        # the last row, id n, is query 0's nearest
    assert ic.coarse_stats(p[3], p[6], nprobe)["exhaustive"] == (nlist <= 65536)      # the coarse search changes roads between the last two


def test_many_probes_and_duplicated_centroid_problems(lsq):
    p, nprobe, nn = ic.many_probes_problem()
    _checked(lsq, p, nprobe, nn)
    st = ic.coarse_stats(p[3], p[6], nprobe)
    assert (st["exhaustive"], st["threshold_rank"], st["list_capacity"]) == (0, 352, 3200)
    p, nprobe, nn = ic.duplicated_centroids_problem()
    di = _checked(lsq, p, nprobe, nn)
    assert (di == 0).sum() == 45                                             # of 370 slots
    st = ic.coarse_stats(p[3], p[6], nprobe)                                 # a mixed coarse batch: query 0 overflows on the 40 000 ties, others are served
    assert 1 <= st["fallback_queries"] < 37 and ic.coarse_stats(p[3], p[6][:1], nprobe)["fallback_queries"] == 1
    probes = ic.probes_np(p[3], p[6][:1], nprobe)[1][0]
    tied = probes[(probes >= 5000) & (probes < 45000)]                       # the ties go to the smaller list ids, after the few nearer centroids
    assert 8 <= tied.shape[0] < nprobe and np.array_equal(tied, np.arange(5000, 5000 + tied.shape[0])) and np.array_equal(tied, probes[-tied.shape[0]:])


def test_near_lists_put_rows_into_probed_lists_at_the_bound(lsq):
    """nlist = 2^24, 4096 rows: no padding at nprobe = 16 or 1, although all but 950 lists are empty"""
    p, nprobe, nn = ic.bound_problem()
    counts = np.bincount(p[4], minlength=ic.BOUND)
    assert p[3].shape == (ic.BOUND, 2) and counts[0] == 1 and counts[-1] == 1 and ((counts > 0).sum(), counts.max()) == (950, 26)
    for k in (nprobe, 1):
        assert not np.any(_checked(lsq, p, k, nn, numpy=False) == 0)


def test_padding_entries_follow_nan_when_the_probed_lists_are_short(lsq):
    codes, K, dbn, cent, lor, Qs, Qc = ic.problem(ic.N, 32, 8, 40, 5, 3)
    lor[:] = 0
    lor[:4] = 3                                                              # list 3 holds rows 1 .. 4 (1-based), one of them with a NaN norm
    dbn[1] = np.float32(np.nan)
    cent[3] = 1000.0
    Qc[:] = 1000.0                                                           # every query probes list 3 first
    rc, dd, di = ic.ivf_cpu(lsq._lib.load(), codes, K, dbn, cent, lor, Qs, Qc, 1, 10)
    assert rc == 0
    assert np.array_equal(np.sort(di[:, :3], axis=1), np.tile([1, 3, 4], (5, 1))) and np.all(di[:, 3] == 2) and np.all(np.isnan(dd[:, 3]))
    assert np.all(di[:, 4:] == 0) and np.all(np.isposinf(dd[:, 4:]))
    rd, ri = ic.ivf_np(codes, K, dbn, cent, lor, Qs, Qc, 1, 10)
    assert same_bits(dd, rd) and np.array_equal(di, ri)


@pytest.mark.parametrize("small_int", [False, True], ids=["gauss", "ties"])
def test_every_list_probed_is_the_exhaustive_host_scan(lsq, small_int):
    """nprobe = nlist, no flag: the distances, ids and tie order of lsq_linscan_aqd_query_extra_byte"""
    L = lsq._lib.load()
    n, d, m, nlist, nq, nn = 2500, 32, 8, 7, 9, 300
    codes, K, dbn, cent, lor, Qs, Qc = ic.problem(n, d, m, nlist, nq, 21, small_int=small_int)
    if small_int:
        codes[n // 2:] = codes[:n - n // 2]                                  # duplicated code rows, in other lists
        dbn[n // 2:] = dbn[:n - n // 2]
    rc, dd, di = ic.ivf_cpu(L, codes, K, dbn, cent, lor, Qs, Qc, nlist, nn)
    assert rc == 0
    sd, si = np.zeros((nq, nn), np.float32), np.zeros((nq, nn), np.int32)
    assert L.lsq_linscan_aqd_query_extra_byte(sd.ctypes.data, si.ctypes.data, codes.ctypes.data, Qs.ctypes.data, K.ctypes.data, dbn.ctypes.data, nq, n, m,
                                              H, d, nn, 0) == 0
    assert same_bits(dd, sd) and np.array_equal(di, si)
    if small_int:
        assert any(len(np.unique(row)) < nn for row in dd)                   # the ties are there


def test_equidistant_centroids_go_to_the_smaller_list(lsq):
    codes, K, dbn, cent, lor, Qs, Qc = ic.problem(2000, 5, 7, 7, 6, 33, small_int=True, lists="random")
    cent[4] = cent[2]                                                        # lists 2 and 4 tie for every query
    Qc[:] = cent[2]
    _, probes = ic.probes_np(cent, Qc, 1)
    assert np.all(probes == 2)
    rc, dd, di = ic.ivf_cpu(lsq._lib.load(), codes, K, dbn, cent, lor, Qs, Qc, 1, 10)
    assert rc == 0 and np.all(lor[di - 1] == 2)
    rd, ri = ic.ivf_np(codes, K, dbn, cent, lor, Qs, Qc, 1, 10)
    assert same_bits(dd, rd) and np.array_equal(di, ri)


def test_helpers_assign_train_and_residual_norms(lsq):
    rng = np.random.default_rng(5)
    centres = rng.standard_normal((6, 8)).astype(np.float32) * 8
    X = (centres[rng.integers(0, 6, 600)] + rng.standard_normal((600, 8))).astype(np.float32)
    cent, assign = lsq.train_coarse(X, 6, niter=5, seed=1)
    assert cent.shape == (6, 8) and cent.dtype == np.float32 and assign.shape == (600,) and assign.dtype == np.int32
    assert np.array_equal(assign, lsq.ivf_assign(X, cent)) and np.array_equal(lsq.train_coarse(X, 6, niter=5, seed=1)[0], cent)
    d2 = ((X[:, None, :].astype(np.float64) - cent[None].astype(np.float64)) ** 2).sum(2)
    assert np.mean(assign == d2.argmin(1)) > 0.99                            # (f32 against f64: a near-tie may differ)
    # an empty cluster keeps its centroid: two identical rows of X cannot both win
    Xd = np.repeat(X[:3], 4, axis=0)
    c2, a2 = lsq.train_coarse(Xd, 3, niter=2, seed=0)
    assert c2.shape == (3, 8) and np.all(np.isfinite(c2))
    # the residual form: the scan's sum plus the coarse distance is |q - c - r^|^2
    m = 2
    K = rng.standard_normal((m * H, 8)).astype(np.float32)
    codes = rng.integers(0, H, (600, m)).astype(np.uint8)
    dbn = lsq.ivf_residual_norms(codes, K, cent, assign)
    recon = sum(K[j * H + codes[:, j].astype(np.int64)] for j in range(m)).astype(np.float64)
    q = rng.standard_normal(8)
    want = ((q[None] - cent[assign] - recon) ** 2).sum(1)
    got = -2 * (recon @ q) + dbn + ((q[None] - cent[assign]) ** 2).sum(1)
    assert np.allclose(got, want, rtol=1e-5, atol=1e-4)


def _cpu_args(p, nprobe=3, nn=5, flags=0):
    codes, K, dbn, cent, lor, Qs, Qc = p
    (n, m), (nq, d) = codes.shape, Qs.shape
    dd, di = np.zeros((nq, nn), np.float32), np.zeros((nq, nn), np.int32)
    keep = (dd, di, codes, K, dbn, cent, lor, Qs, Qc)
    return keep, [a.ctypes.data for a in keep] + [n, m, H, d, cent.shape[0], nq, d, nprobe, nn, flags, 0]


def test_host_checker_refuses_bad_arguments(lsq):
    L, EINVAL = lsq._lib.load(), lsq._lib.LSQ_EINVAL
    p = ic.problem(300, 5, 2, 7, 3, 1)
    keep, good = _cpu_args(p)
    assert L.lsq_ivf_search_cpu(*good) == 0
    for k in range(8):                                                       # a null pointer, one at a time (q_coarse may be null: it is q_scan then)
        bad = list(good)
        bad[k] = None
        assert L.lsq_ivf_search_cpu(*bad) == EINVAL and b"null" in L.lsq_last_error()
    nocoarse = list(good)
    nocoarse[8] = None
    assert L.lsq_ivf_search_cpu(*nocoarse) == 0
    names = ["n", "m", "h", "d", "nlist", "nq", "ldq", "nprobe", "nn", "flags"]
    for name, value in (("nprobe", 0), ("nprobe", 8), ("nlist", 0), ("nlist", (1 << 24) + 1), ("nn", 0), ("flags", 8), ("flags", -1), ("ldq", 4),
                        ("n", 0), ("m", 0), ("h", 257), ("d", 0), ("nq", -1)):
        bad = list(good)
        bad[9 + names.index(name)] = value
        assert L.lsq_ivf_search_cpu(*bad) == EINVAL, (name, value)
    for entry in (-1, 7):                                                    # a list_of_row entry outside [0, nlist)
        p[4][11] = entry
        assert L.lsq_ivf_search_cpu(*good) == EINVAL and b"list_of_row" in L.lsq_last_error()
    p[4][11] = 0
    assert L.lsq_ivf_search_cpu(*good) == 0 and keep is not None


def test_index_symbols_refuse_a_null_handle(lsq):
    L, EINVAL = lsq._lib.load(), lsq._lib.LSQ_EINVAL
    desc, info = lsq._lib.IvfDesc(), lsq._lib.IvfInfo()
    buf = np.zeros(64, np.float32)
    assert L.lsq_index_set_lists(None, C.byref(desc)) == EINVAL
    assert L.lsq_index_search_ivf(None, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None, None, 1, 5, 1, 0, 1, 0, 0) == EINVAL
    assert L.lsq_index_get_ivf_info(None, C.byref(info)) == EINVAL
