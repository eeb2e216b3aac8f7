"""The encoder BETWEEN the corners the rest of the suite holds it at (README: "All schedules and option values give bit-identical codes").

A. the light / staged switch of both walk kernels (`nact <= direct_max`, csrc/lsq_icmq.hip and csrc/lsq_icm.hip) with the threshold moved through every
   block's activity range, so that a block alternates between the two routines inside one launch -- they share the records, the validity words and, for
   m <= 8, the LDS validity mirror; every instantiation family; two passes per block with the mirror reloaded in between (option `chunk` above its default);
B. node sequences longer than one launch holds (icmiter * m > 64 = LSQ_WALK_MAX_NODES): the three launchers' one splitter cuts them (lsq_wave.h), the
   per-position trace wraps modulo 64 (lsq_internal.h), option `per_node` cuts them into single node updates, the filter probe into two parts;
C. every PAIR of option values (tests/option_space.py), one encode per row of a covering array.

The reference is always the CPU oracle (oracle.encode_icm: it executes every node update and knows nothing about roads): codes equal, objectives within
rtol 1e-5, accept counters equal to its `want_stats`.  The counter identities asserted on top follow from the kernels' bookkeeping (one thread per block adds
nact to [0], one to light / staged / filtered per (block, node update) with nact > 0, nact to trace[position mod 64]) -- they are not measurements.
"""
import functools

import numpy as np
import pytest

import option_space as S
from conftest import make_problem, open_engine
from test_gpu_depth import _check_rows, _rows_small

pytestmark = pytest.mark.gpu

H = 256
PER = 280                      # vectors per block: 256 blocks x 280, ONE pass per block in both walks for every m (PP >= 3328: lsq_wave.h, lsq_q16.h)
N = 256 * PER                  # 71 680 > q16_min = 65 536
BIG = 2 ** 31 - 1
SEED = 42
RULES = [(1, 1), (0, 1), (1, 0)]      # (skip, fallback)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")          # (a copy: the problems' arrays are read-only)


class Problem:
    """inputs on the host and on the device + the oracle's answer, computed once and never changed"""

    def __init__(self, oracle, X, K, B0, m, ils, J, npert, u8=False):
        self.X, self.K, self.B0, self.m, self.ils, self.J, self.npert = X, K, B0, m, list(ils), J, npert
        self.n, self.d = X.shape
        self.ref, self.objs, st = oracle.encode_icm(X, B0, K, m, H, self.ils, J, npert, True, SEED, want_stats=True)
        self.stats = st.astype(np.int64)
        self.X8 = None
        if u8:
            assert X.min() >= 0 and X.max() <= 255 and np.array_equal(X, np.floor(X)), "the rows must also serve the 8-bit entry points"
            self.X8 = X.astype(np.uint8)
        for a in (self.X, self.K, self.B0, self.ref, self.objs, self.stats):
            a.setflags(write=False)
        self._dev = None

    def dev(self):
        if self._dev is None:
            self._dev = {"X": _dev(self.X), "K": _dev(self.K), "B0": _dev((self.B0 - 1).astype(np.uint8)), "ref": _dev((self.ref - 1).astype(np.uint8)),
                         "X8": None if self.X8 is None else _dev(self.X8)}
        return self._dev

    def cut(self, nsnap):
        """the same problem seen through its first `nsnap` snapshots (an encode to ils[:nsnap] runs the same iterations up to there)"""
        return self.ref[:nsnap], self.objs[:nsnap], self.stats[:self.ils[nsnap - 1]]


def trapped(d, n, m, seed, u8=False):
    """make_problem's SIFT-like integer rows with the traps of test_filter_light_blocks: one codebook with duplicated codewords (exact ties at one node) and
    ~1 % of the rows scaled x 6 in 128-row panels the level-range sample does not visit (it reads every (n / 16384)-th panel, starting with panel 0): the GEMM
    epilogue flags them and they take the f32 routine inside the filtered walk.  u8: everything is first divided by 6 (rows rounded down: still integers), so
    that the scaled rows stay within 0 .. 255 and the same rows serve the 8-bit entry points."""
    X, K, B0 = make_problem(d, n, m, seed=seed, kind="sift")
    if u8:
        X, K = np.floor(X / np.float32(6.0)), K / np.float32(6.0)
    K = K.reshape(m, H, d).copy()
    K[min(3, m - 1), 1::2] = K[min(3, m - 1), 0::2]
    K = np.ascontiguousarray(K.reshape(m * H, d))
    rts = max(n // 16384, 1)
    hot = np.array([i for i in range(0, n, 79) if rts > 1 and (i // 128) % rts != 0], dtype=np.int64)
    X = X.copy()
    if hot.size:
        X[hot] *= np.float32(6.0)
    return np.ascontiguousarray(X, dtype=np.float32), K, B0


@pytest.fixture(scope="module")
def std(oracle):
    """the standard problem: d = 32, m = 8, n = 71 680; ILS snapshots [1, 3], 4 sweeps, npert 4, random order"""
    X, K, B0 = trapped(32, N, 8, seed=77, u8=True)
    return Problem(oracle, X, K, B0, 8, [1, 3], 4, 4, u8=True)


def run_dev(eng, P, ils=None, u8=False, nonblocking=False):
    """one device-resident encode -> (codes tensor (nr, n, m) u8, sums f64 (nr,), stats i64 (I, 2), counters dict, trace i64 (64,))"""
    import torch
    D = P.dev()
    eng.reset_timings()
    dBs, sums, stats = eng.encode_icm_dev(D["X8"] if u8 else D["X"], D["B0"], D["K"], P.m, P.ils if ils is None else ils, P.J, P.npert, True, seed=SEED,
                                          nonblocking=nonblocking)
    torch.cuda.synchronize()
    if nonblocking:
        sums, stats = sums.cpu().numpy(), stats.cpu().numpy()
    t = eng.timings()                    # (folds what an async call left on the device)
    return dBs, np.asarray(sums), np.asarray(stats), t, eng.walk_trace()


def run_host(eng, P, ils=None, u8=False):
    """one host-buffer encode (the entry point returns no accept counters) -> (codes, objs f32, None, counters, trace)"""
    eng.reset_timings()
    Bs, objs = eng.encode_icm(P.X8 if u8 else P.X, P.B0, P.K, P.m, P.ils if ils is None else ils, P.J, P.npert, True, seed=SEED)
    return Bs, objs, None, eng.timings(), eng.walk_trace()


def check(P, got, tag, nsnap=None):
    """the full oracle check: codes equal, objectives rtol 1e-5, accept counters equal"""
    import torch
    codes, sums, stats = got[:3]
    ref, objs, st = P.cut(len(P.ils) if nsnap is None else nsnap)
    if isinstance(codes, torch.Tensor):
        dref = P.dev()["ref"][:ref.shape[0]]
        assert codes.shape == dref.shape, tag
        if not torch.equal(codes, dref):
            bad = (codes != dref).any(dim=2)
            raise AssertionError("%s: %d of %d rows differ from the oracle (first: snapshot, row %s)" % (tag, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist()))
        assert np.allclose(sums / P.n, objs, rtol=1e-5, atol=0), (tag, sums / P.n, objs)
        assert np.array_equal(stats, st), (tag, stats.tolist(), st.tolist())
    else:
        assert np.array_equal(codes, ref), "%s: %d of %d rows differ from the oracle" % (tag, int((codes != ref).any(axis=2).sum()), ref.shape[0] * ref.shape[1])
        assert np.allclose(sums, objs, rtol=1e-5, atol=0), (tag, sums, objs)


def blocks(t):
    return t["light_blocks"], t["filtered_blocks"], t["staged_blocks"]


# ======================================================================================================================================================
# A. the threshold sweep
# ======================================================================================================================================================
THRESHOLDS = [-1, 0, 1, 16, 63, 64, 65, 128, 159, 160, 161, 200, 255, 256, 257, 279, 280, 281, BIG]
ROADS = {"s6": dict(schedule=6, q16_min=0, filter_probe_div=0, filter_fallback_div=0, wave_max=0),      # the 16-bit filtered walk, kept to its end
         "s4": dict(schedule=4, wave_max=0)}                                                          # the f32 walk (never the wave kernel)
DEFAULT_LIGHT = {"s6": 160, "s4": 256}                                                                # what light = -1 stands for in each launcher

_NODE_UPDATES = {}       # (skip, fallback) -> icm_node_updates of the standard problem, from an oracle-checked run of part A; part C holds its rows to it


def threshold_sweep(lsq, P, road, thresholds, per, remember=None):
    L = P.ils[-1] * P.J * P.m                                    # node updates per vector
    for skip, fb in RULES:
        seen = {}
        with open_engine(lsq, dict(ROADS[road], skip=skip, fallback=fb)) as eng:
            for thr in thresholds:
                eng.set_option("light", thr)
                got = run_dev(eng, P)
                tag = "%s skip=%d fallback=%d light=%d" % (road, skip, fb, thr)
                check(P, got, tag)
                t = got[3]
                seen[thr] = (t["icm_node_updates"],) + blocks(t)
                print(tag, "node updates %d light %d filtered %d staged %d" % seen[thr], "f32 %d refined %d" % (t["filter_f32"], t["filter_refined"]))
                assert got[4].sum() == t["icm_node_updates"], tag
                # the routine that is not this road's never runs
                assert (t["staged_blocks"] if road == "s6" else t["filtered_blocks"]) == 0, (tag, t)
        eff = lambda thr: DEFAULT_LIGHT[road] if thr < 0 else thr
        order = sorted(thresholds, key=eff)
        upd = {seen[thr][0] for thr in thresholds}
        assert len(upd) == 1, "%s skip=%d fallback=%d: icm_node_updates depends on the threshold: %r" % (road, skip, fb, {k: v[0] for k, v in seen.items()})
        if skip == 0:
            assert upd == {P.n * L}, (upd, P.n * L)
        total = {sum(seen[thr][1:]) for thr in thresholds}       # the (block, node update) pairs with nact > 0
        assert len(total) == 1, "%s skip=%d fallback=%d: light + filtered + staged depends on the threshold: %r" % (road, skip, fb, seen)
        if skip == 0:
            assert total == {256 * L}, (total, 256 * L)          # every block is active at every node update
        lights = [seen[thr][1] for thr in order]
        assert lights == sorted(lights), "%s skip=%d fallback=%d: light_blocks falls as the threshold rises: %r" % (road, skip, fb, list(zip(order, lights)))
        for thr in thresholds:
            nu, light, filt, staged = seen[thr]
            if thr == 0:
                assert light == 0, (road, skip, fb, seen[thr])
            if eff(thr) >= per:
                assert filt == 0 and staged == 0, (road, skip, fb, thr, seen[thr])
            if skip == 1 and 16 <= eff(thr) <= 256:
                assert light > 0 and filt + staged > 0, "%s fallback=%d light=%d: one routine only: %r" % (road, fb, thr, seen[thr])
            if skip == 0 and eff(thr) < per:
                assert light == 0, (road, fb, thr, seen[thr])    # every block holds `per` active vectors throughout
        if -1 in seen and DEFAULT_LIGHT[road] in seen:
            assert seen[-1] == seen[DEFAULT_LIGHT[road]], (road, skip, fb, seen[-1], seen[DEFAULT_LIGHT[road]])
        if remember is not None:
            val = next(iter(upd))
            assert remember.setdefault((skip, fb), val) == val, "the two walks disagree on the node updates they recompute"


@pytest.mark.parametrize("road", ["s6", "s4"])
def test_threshold_sweep_standard_problem(lsq, std, road):
    """Both routines of a walk inside one launch, block by block, with the crossover at 19 places between "never light" and "always light": per-block activity
    falls from ~274 to ~17 over the four sweeps of an iteration, so every threshold in between cuts every block's sequence somewhere else."""
    threshold_sweep(lsq, std, road, THRESHOLDS, PER, remember=_NODE_UPDATES)
    if road == "s6":                                             # the traps are live: flagged rows took the f32 routine, ties the exact refinement
        with open_engine(lsq, dict(ROADS["s6"], light=0)) as eng:
            t = run_dev(eng, std)[3]
        assert t["filter_f32"] > 0 and t["filter_refined"] > 0, t


@functools.lru_cache(maxsize=None)
def family_problem(m):
    import oracle as O
    X, K, B0 = trapped(16, N, m, seed=200 + m)
    return Problem(O, X, K, B0, m, [2], 4, min(4, m))


@pytest.mark.parametrize("road", ["s6", "s4"])
@pytest.mark.parametrize("m", [3, 9, 13, 16])
def test_threshold_sweep_every_family(lsq, oracle, m, road):
    """m = 3 / 9 / 13 / 16: both LSQ_LIGHT_LB values, 8- and 16-byte records, with and without the validity mirror, the three instantiation families of the
    f32 walk and both slice widths of the filtered one."""
    threshold_sweep(lsq, family_problem(m), road, [0, 64, 160, PER, BIG], PER)


def test_two_passes_per_block_reload_the_mirror(lsq, oracle):
    """m = 8 with option `chunk` raised to n = 1 060 000 > 256 x 3968: every block of the filtered walk makes TWO passes of 2071 vectors and reloads its LDS
    validity mirror in between (unreachable at the default chunk).  Sampled rows -- both sides of block-pass edges, of the seam between the blocks' first and
    second passes, the ends, a seeded scatter -- against the oracle; the three thresholds must also agree on every row."""
    import torch
    n, d, m, ils, J, npert = 1_060_000, 16, 8, [2], 4, 4
    per, npass = 2071, 512                                       # launch_walkq_t: rounds = ceil(n / (256 PP)) = 2 at PP = 3968, per = ceil(n / 512)
    assert 256 * 3968 < n <= 512 * 3968 and -(-n // 512) == per and -(-n // per) == npass
    edges = [(per - 8, per + 8), (255 * per - 8, 255 * per + 8), (256 * per - 24, 256 * per + 24), (257 * per - 8, 257 * per + 8), (511 * per - 8, 511 * per + 8)]
    rows = _rows_small(n, extra=edges)
    codes = {}
    with lsq.Engine(0, chunk=n) as eng:
        for k, v in ROADS["s6"].items():
            eng.set_option(k, v)
        dX = eng.synth_data_u8_dev(1234, n, d)
        dB0 = eng.randinit_dev(7, n, m)
        dK = eng.synth_codebooks_dev(4321, m, d)
        for thr in (0, 1500, BIG):
            eng.set_option("light", thr)
            eng.reset_timings()
            dBs, sums, stats = eng.encode_icm_dev(dX, dB0, dK, m, ils, J, npert, True, seed=SEED)
            torch.cuda.synchronize()
            t = eng.timings()
            print("light=%d" % thr, {k: t[k] for k in ("icm_node_updates", "light_blocks", "filtered_blocks", "staged_blocks", "filter_f32")})
            bad, cnt = _check_rows(oracle, dX, dB0, dBs[0], dK, rows, m, ils, J, npert, SEED)
            assert cnt >= 200 and bad == 0, "light=%d: %d of %d checked rows differ from the oracle" % (thr, bad, cnt)
            assert np.isfinite(sums[0]) and sums[0] > 0 and stats.shape == (2, 2)
            assert eng.walk_trace().sum() == t["icm_node_updates"] and t["staged_blocks"] == 0
            assert (t["light_blocks"] == 0) if thr == 0 else (t["filtered_blocks"] == 0) if thr == BIG else (t["light_blocks"] > 0 and t["filtered_blocks"] > 0), t
            codes[thr] = (dBs, t["icm_node_updates"], t["light_blocks"] + t["filtered_blocks"], stats.copy(), sums.copy())
        # the geometry itself: without the skip rule every pass is active at every node update -- 512 passes, two per block
        eng.set_option("skip", 0)
        eng.reset_timings()
        dBs, _, _ = eng.encode_icm_dev(dX, dB0, dK, m, [1], 1, npert, True, seed=SEED)
        torch.cuda.synchronize()
        t = eng.timings()
        assert t["light_blocks"] == npass * m and t["icm_node_updates"] == n * m, t
    for thr in (1500, BIG):
        assert torch.equal(codes[thr][0], codes[0][0]), "light=%d: %d rows differ from light=0" % (thr, int((codes[thr][0] != codes[0][0]).any(dim=2).sum()))
        assert codes[thr][1:3] == codes[0][1:3] and np.array_equal(codes[thr][3], codes[0][3]) and np.array_equal(codes[thr][4], codes[0][4])


# ======================================================================================================================================================
# B. node sequences longer than one launch
# ======================================================================================================================================================
PAIRS = [(8, 8), (16, 4), (13, 5), (8, 9), (16, 5), (13, 10), (1, 70)]      # (m, icmiter): 64, 64, 65, 72, 80, 130, 70 node updates per ILS iteration
FORCED = dict(schedule=6, q16_min=0, light=0, filter_probe_div=0, filter_fallback_div=0)
NWAVE, NFULLY = 2048, 20_480


@functools.lru_cache(maxsize=None)
def long_problem(m, J):
    """d = 16, n = 71 680, ILS snapshots [1, 2] (one oracle run serves the calls of one and of two iterations), SIFT-like integer rows (they also serve the
    8-bit call), one codebook with duplicated codewords"""
    import oracle as O
    X, K, B0 = make_problem(16, N, m, seed=300 + m, kind="sift")
    K = K.reshape(m, H, 16).copy()
    K[m // 2, 1::2] = K[m // 2, 0::2]
    return Problem(O, X, np.ascontiguousarray(K.reshape(m * H, 16)), B0, m, [1, 2], J, min(4, m), u8=True)


@functools.lru_cache(maxsize=None)
def wave_problem(m, J):
    """the first 2048 rows of long_problem: 8 vectors per block, the wave kernel's size (its own oracle run: the accept counters are per call)"""
    import oracle as O
    P = long_problem(m, J)
    return Problem(O, P.X[:NWAVE].copy(), P.K.copy(), P.B0[:NWAVE].copy(), m, [1, 2], J, P.npert)


def expected_trace(n, iterations, L):
    e = np.zeros(64, dtype=np.int64)
    for q in range(L):
        e[q % 64] += n * iterations                              # position q of every iteration lands in word q mod 64 (LSQ_WALK_TRACE)
    return e


def long_road(lsq, P, tag, options, nsnap, u8=False, nonblocking=False, light0=True, expect=None):
    """One road on one problem, all rows against the oracle: without the skip rule (every node update of every vector runs: counter and trace are known in
    closed form), with it (the trace still sums to the counter), and -- unless the road already has light = 0 -- with it at light = 0, which must recompute
    the same node updates at the same positions.  -> what the skip = 1 run returned."""
    ils = P.ils[:nsnap]
    L = P.J * P.m
    out = {}
    for skip in (0, 1):
        with open_engine(lsq, dict(options, skip=skip)) as eng:
            got = run_dev(eng, P, ils=ils, u8=u8, nonblocking=nonblocking)
        check(P, got, "%s skip=%d" % (tag, skip), nsnap)
        t, tr = got[3], got[4]
        print("%s skip=%d: node updates %d light %d filtered %d staged %d launches %d fallback chunks %d" % (
            tag, skip, t["icm_node_updates"], t["light_blocks"], t["filtered_blocks"], t["staged_blocks"], t["icm_launches"], t["filter_fallback_chunks"]))
        assert tr.sum() == t["icm_node_updates"], (tag, skip, tr.sum(), t["icm_node_updates"])
        if skip == 0:
            assert t["icm_node_updates"] == P.n * ils[-1] * L, (tag, t["icm_node_updates"], P.n * ils[-1] * L)
            assert np.array_equal(tr, expected_trace(P.n, ils[-1], L)), (tag, tr.tolist())
        else:
            assert t["icm_node_updates"] < P.n * ils[-1] * L, tag                      # the memoisation rules did skip something
        if expect is not None:
            assert expect(t), (tag, skip, t)
        out[skip] = got
    if light0:
        with open_engine(lsq, dict(options, skip=1, light=0)) as eng:
            got0 = run_dev(eng, P, ils=ils, u8=u8, nonblocking=nonblocking)
        check(P, got0, "%s skip=1 light=0" % tag, nsnap)
        assert got0[3]["icm_node_updates"] == out[1][3]["icm_node_updates"] and np.array_equal(got0[4], out[1][4]), (tag, got0[4].tolist(), out[1][4].tolist())
    return out[1]


@pytest.mark.parametrize("m,J", PAIRS, ids=["m%d_x%d" % p for p in PAIRS])
def test_long_node_sequences_walk_roads(lsq, oracle, m, J):
    """The four ways run_sweeps issues a sequence (csrc/lsq_api.hip): the filtered walk in launches of 64 (and of ONE: `per_node`), the f32 walk's launcher
    splitting a whole iteration, schedule 3's launch per node update, the wave kernel's launcher."""
    P = long_problem(m, J)
    nl = -(-J * m // 64)                                         # launches of 64 per iteration

    a = long_road(lsq, P, "s6 forced", FORCED, 1, light0=False,
                  expect=lambda t: t["filtered_blocks"] > 0 and t["staged_blocks"] == 0 and t["light_blocks"] == 0)
    # icm_launches in closed form (run_sweeps, csrc/lsq_api.hip): with schedule >= 4 one run_sweeps call issues its nsweeps * m node updates in launches of at
    # most 64 -- ceil(nsweeps * m / 64) of them on the filtered walk, the f32 walk and the wave kernel alike -- and without the probe encode_chunk calls it
    # once per ILS iteration with nsweeps = J: nl launches per iteration, whichever road the chunk's verdict names
    long_road(lsq, P, "s6 default light", dict(schedule=6, q16_min=0, filter_probe_div=0, filter_fallback_div=0), 2,
              expect=lambda t: t["icm_launches"] == 2 * nl)
    long_road(lsq, P, "s4 light=0", dict(schedule=4, light=0), 2, light0=False,
              expect=lambda t: t["staged_blocks"] > 0 and t["light_blocks"] == 0 and t["filtered_blocks"] == 0 and t["icm_launches"] == 2 * nl)
    long_road(lsq, P, "s3", dict(schedule=3), 1, expect=lambda t: t["icm_launches"] == J * m)
    long_road(lsq, wave_problem(m, J), "wave kernel", {}, 2, light0=False,
              expect=lambda t: t["light_blocks"] > 0 and t["staged_blocks"] == 0 and t["filtered_blocks"] == 0 and t["icm_launches"] == 2 * nl)
    # (2048 rows < q16_min: no filtered walk, so no probe; 8 vectors per block <= wave_max: the wave kernel's launcher, nl launches in each of two iterations)
    # per_node = 1: one launch per node update -- the same codes, accept counters, walk counters and trace as the launches of 64
    b = long_road(lsq, P, "s6 forced per_node", dict(FORCED, per_node=1), 1, light0=False,
                  expect=lambda t: t["icm_launches"] == J * m)
    import torch
    assert torch.equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[4], b[4])
    keys = ("icm_node_updates", "light_blocks", "filtered_blocks", "staged_blocks", "filter_refined", "filter_exact", "filter_f32")
    assert [a[3][k] for k in keys] == [b[3][k] for k in keys], (a[3], b[3])
    assert a[3]["icm_launches"] == nl


@pytest.mark.parametrize("m,J", PAIRS, ids=["m%d_x%d" % p for p in PAIRS])
def test_long_node_sequences_entry_points(lsq, oracle, m, J):
    """The same sequences through the other entry points, on the roads their defaults take at this size: the async device call (the chunk's road is a device
    word: both walks are enqueued), the 8-bit device call, the filter probe left on -- in a call of one iteration it splits the iteration's sweeps in two, in a
    call of two it reads the first iteration's counters --, and the two CPU-shaped calls (niter * m > 64)."""
    P = long_problem(m, J)
    # icm_launches in closed form, from run_sweeps and encode_chunk (csrc/lsq_api.hip).  One run_sweeps call of nsweeps sweeps makes ceil(nsweeps * m / 64)
    # launches on whichever walk it takes (schedule >= 4, per_node = 0), and none when nsweeps = 0.
    nl = -(-J * m // 64)                                         # ... of a whole iteration
    # The probe (filter_probe_div > 0, a chunk the verdict gave to the filtered walk) cuts the FIRST iteration into probe_sweeps and the rest, two run_sweeps
    # calls.  A call of two iterations: probe_sweeps = J, the rest is empty -- nl + 0, then nl for the second iteration, probed or not.  A call of one
    # iteration: probe_sweeps = 2 (J >= 3 in every pair), so ceil(2 m / 64) + ceil((J - 2) m / 64); the second part takes the road the probe chose, at the
    # same count (280 vectors per block > wave_max: never the wave kernel).
    assert J >= 3
    split = -(-2 * m // 64) + -(-(J - 2) * m // 64)
    # option "async": the verdict and the probe are device words, so every run_sweeps call enqueues the filtered launches AND the f32 launches behind them:
    # iteration one nl + nl (+ an empty rest), iteration two nl + nl
    long_road(lsq, P, "async", {}, 2, nonblocking=True, expect=lambda t: t["icm_launches"] == 4 * nl)
    long_road(lsq, P, "u8 device call", {}, 1, u8=True, expect=lambda t: t["icm_launches"] == split)      # the defaults probe: one iteration, cut in two
    for nsnap in (1, 2):
        long_road(lsq, P, "probe on, %d iteration(s)" % nsnap, dict(schedule=6, q16_min=0, filter_probe_div=8), nsnap,
                  expect=lambda t: t["icm_launches"] == (split if nsnap == 1 else 2 * nl))
    # lsq_encoding_icm: one ILS iteration with the accept rule = the call's first snapshot (it = 0)
    with lsq.Engine(0) as eng:
        eng.reset_timings()
        B1 = eng.encoding_icm(P.X, P.B0, P.K, m, J, True, P.npert, seed=SEED, it=0)
        t, tr = eng.timings(), eng.walk_trace()
    assert np.array_equal(B1, P.ref[0]), "encoding_icm: %d rows differ from the oracle" % int((B1 != P.ref[0]).any(axis=1).sum())
    assert tr.sum() == t["icm_node_updates"] > 0
    assert t["icm_launches"] == split, (t["icm_launches"], split)      # one iteration under the default probe: cut in two, as above
    # lsq_encode_icm_fully: perturbation + sweeps without the accept step (the oracle's worker), on the first 20 480 rows, filtered walk forced and defaults
    Xs, Bs = P.X[:NFULLY], P.B0[:NFULLY]
    want = oracle.encode_icm_fully(Xs, Bs, P.K, m, H, J, True, P.npert, seed=SEED, it=0)
    for options in (FORCED, {}):
        with open_engine(lsq, options) as eng:
            got = eng.encode_icm_fully(Bs.copy(), Xs, P.K, m, J, True, P.npert, seed=SEED, it=0)
        assert np.array_equal(got, want), "encode_icm_fully %r: %d rows differ from the oracle" % (options, int((got != want).any(axis=1).sum()))


# ======================================================================================================================================================
# C. every pair of option values
# ======================================================================================================================================================
ARRAY = S.covering_array()


def node_updates_of_part_a(lsq, P, skip, fb):
    """what part A measured for this (skip, fallback) on an oracle-checked run; on its own (part A deselected) the same run is made here"""
    if skip == 0:
        return P.n * P.ils[-1] * P.J * P.m                       # part A holds skip = 0 to this number, whatever `fallback` is (no rule reads the reference then)
    if (skip, fb) not in _NODE_UPDATES:
        with open_engine(lsq, dict(ROADS["s4"], skip=skip, fallback=fb, light=0)) as eng:
            got = run_dev(eng, P)
        check(P, got, "s4 light=0 skip=%d fallback=%d" % (skip, fb))
        _NODE_UPDATES[(skip, fb)] = got[3]["icm_node_updates"]
    return _NODE_UPDATES[(skip, fb)]


@pytest.mark.parametrize("row", ARRAY, ids=[S.row_id(r) for r in ARRAY])
def test_every_pair_of_option_values(lsq, std, row):
    opts, entry = S.resolve(row, std.n)
    want_updates = node_updates_of_part_a(lsq, std, opts["skip"], opts["fallback"])
    with open_engine(lsq, opts) as eng:
        if entry.startswith("host"):
            got = run_host(eng, std, u8=entry == "host_u8")
        else:
            got = run_dev(eng, std, u8=entry == "dev_u8", nonblocking=entry == "dev_async")
    check(std, got, S.row_id(row))
    t, tr = got[3], got[4]
    print(S.row_id(row), {k: t[k] for k in ("icm_node_updates", "light_blocks", "filtered_blocks", "staged_blocks", "filter_fallback_chunks", "icm_launches")})
    per_block = -(-min(opts["chunk"], std.n) // 256)
    wave = S.takes_wave_kernel(row, std.n, per_block)
    if opts["schedule"] in (3, 4) or not S.takes_filtered_walk(row, std.n):
        assert t["filtered_blocks"] == 0, t
    if opts["light"] == 0 and not wave:
        assert t["light_blocks"] == 0, t
    if wave:
        assert t["light_blocks"] > 0 and t["staged_blocks"] == 0 and t["filtered_blocks"] == 0, t
    assert t["icm_node_updates"] == want_updates, (t["icm_node_updates"], want_updates)
    assert tr.sum() == t["icm_node_updates"]
