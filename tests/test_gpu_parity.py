"""GPU parity: the HIP path (through the C-ABI) vs the CPU oracle on the same seeded inputs.

Bar (north_star): integer codes BIT-EXACT; float tables bit-exact too (the kernels are built to
reproduce the oracle's canonical fp32 operation order); objective within 1e-5 relative.
"""
import numpy as np
import pytest

from conftest import ENCODE_VARIANTS, make_problem, open_engine

pytestmark = pytest.mark.gpu

H = 256


def _same_f32(a, b):
    """bitwise equality up to the sign of zero (np.array_equal: -0 == +0, NaN != NaN)."""
    return a.shape == b.shape and np.array_equal(a, b)


# ---- tables -----------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m,kind", [(16, 4, "gauss"), (128, 8, "sift"), (100, 3, "gauss"), (33, 2, "gauss")])
def test_binaries_bit_exact(engine, oracle, d, m, kind):
    _, K, _ = make_problem(d, 4, m, seed=d + m, kind=kind)
    T = engine.get_binaries(K, m)
    Tref = oracle.tables(K, m, H)
    assert _same_f32(T, Tref), "max abs diff %g" % np.abs(T - Tref).max()


@pytest.mark.parametrize("d,n,m,kind", [(16, 64, 4, "gauss"), (128, 300, 8, "sift"), (128, 129, 7, "gauss"),
                                        (960, 40, 8, "gauss"), (100, 77, 3, "gauss"), (128, 64, 16, "sift"), (5, 10, 1, "gauss")])
def test_unaries_bit_exact(engine, oracle, d, n, m, kind):
    X, K, _ = make_problem(d, n, m, seed=n, kind=kind)
    U = engine.get_unaries(X, K, m)
    Uref = oracle.unaries(X, K, m, H)
    assert _same_f32(U, Uref), "max abs diff %g" % np.abs(U - Uref).max()


@pytest.mark.parametrize("d,n,m,kind", [(16, 64, 4, "gauss"), (128, 1000, 8, "sift"), (960, 33, 8, "gauss"),
                                        (100, 77, 3, "gauss"), (128, 64, 16, "sift"), (7, 5, 2, "gauss"),
                                        (2, 70, 4, "gauss"), (30, 200, 8, "sift"), (130, 300, 8, "gauss"), (258, 40, 16, "gauss"),
                                        (129, 150, 9, "sift")])
def test_veccost_bit_exact(engine, oracle, d, n, m, kind):
    X, K, B0 = make_problem(d, n, m, seed=d, kind=kind)
    c = engine.veccost(X, B0, K, m)
    cref = oracle.veccost(X, K, (B0 - 1).astype(np.uint8), H)
    assert _same_f32(c, cref)
    q = engine.qerror(X, B0, K, m)
    assert abs(q - oracle.qerror(X, B0, K, m, H)) <= 1e-6 * abs(q)


@pytest.mark.parametrize("m,npert", [(8, 4), (7, 4), (16, 4), (4, 2), (3, 3), (5, 0), (2, 9)])
def test_perturb_exact(engine, oracle, m, npert):
    n = 500
    B0 = oracle.randinit(11, n, m, H)
    out = engine.perturb(B0, npert, seed=77, it=3, global_offset=1000)
    ref = np.stack([oracle.perturb(77, 1000 + i, 3, (B0[i] - 1).astype(np.uint8), H, npert) for i in range(n)]).astype(np.int16) + 1
    assert np.array_equal(out, ref)


# ---- the whole call ---------------------------------------------------------------------------
CONFIGS = [
    # d, n, m, ilsiters, J, npert, randord, seed, kind
    (16, 64, 4, [1, 2], 4, 2, True, 1, "gauss"),
    (128, 64, 7, [2], 4, 4, True, 2, "sift"),
    (128, 256, 8, [1, 2, 4], 4, 4, True, 3, "sift"),
    (128, 48, 16, [2], 4, 4, True, 4, "sift"),
    (960, 16, 8, [1], 4, 4, False, 5, "gauss"),
    (128, 1, 8, [3], 2, 4, True, 6, "gauss"),        # single vector
    (32, 300, 2, [2], 3, 1, True, 7, "gauss"),
    (64, 100, 5, [1, 3], 1, 5, False, 8, "gauss"),
    (128, 200, 8, [2], 4, 0, True, 9, "sift"),        # no perturbation
    (24, 90, 1, [2], 2, 1, True, 10, "gauss"),        # one codebook: argmin of the unary
    (32, 150, 8, [2], 9, 3, True, 11, "gauss"),       # 72 node updates per ILS iteration: more than one launch's node list (64)
    (32, 70, 16, [1], 5, 4, True, 12, "gauss"),       # 80 node updates, 16-byte code records
    (130, 120, 8, [1, 2], 4, 4, True, 13, "gauss"),   # d % 4 == 2: the cost pass's 4-byte loads
    (33, 90, 5, [2], 3, 2, True, 14, "sift"),         # odd d
]


@pytest.mark.parametrize("variant", ENCODE_VARIANTS)
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "d%d_n%d_m%d" % (c[0], c[1], c[2]))
def test_encode_icm_matches_oracle(lsq, oracle, cfg, variant):
    d, n, m, ils, J, npert, randord, seed, kind = cfg
    X, K, B0 = make_problem(d, n, m, seed=seed, kind=kind)
    Bs_ref, objs_ref, st_ref = oracle.encode_icm(X, B0, K, m, H, ils, J, npert, randord, seed, want_stats=True)
    with open_engine(lsq, variant, profile=True) as eng:
        Bs, objs = eng.encode_icm(X, B0, K, m, ils, J, npert, randord, seed=seed)
        t = eng.timings()
    assert np.array_equal(Bs, Bs_ref), "%d of %d codes differ" % ((Bs != Bs_ref).sum(), Bs.size)
    assert np.allclose(objs, objs_ref, rtol=1e-5, atol=0)
    if variant.get("q16_min") == 0 and variant.get("light") == 0:       # the shipped default kernel produced every code
        assert t["filtered_blocks"] > 0 and t["staged_blocks"] == 0 and t["light_blocks"] == 0, t


def test_skip_unchanged_is_exact(lsq, oracle):
    """Schedules 3/4 memoise node updates whose conditioning codes did not change.  It must be a pure
    optimisation: identical codes/objective with skip on and off (and equal to the oracle), while
    strictly fewer node updates are recomputed.  n spans several passes per block and ragged tails."""
    d, n, m, ils, J, npert, seed = 64, 9001, 8, [1, 3], 4, 4, 77
    X, K, B0 = make_problem(d, n, m, seed=seed)
    Bs_ref, objs_ref, st_ref = oracle.encode_icm(X, B0, K, m, H, ils, J, npert, True, seed, want_stats=True)
    for schedule in (6, 4, 3):
        counts = {}
        for skip in (1, 0):
            with lsq.Engine(0, schedule=schedule, skip=skip, profile=True) as eng:
                eng.set_option("q16_min", 0)
                Bs, objs = eng.encode_icm(X, B0, K, m, ils, J, npert, True, seed=seed)
                counts[skip] = eng.timings()["icm_node_updates"]
            assert np.array_equal(Bs, Bs_ref), "schedule %d skip=%d: %d codes differ" % (schedule, skip, (Bs != Bs_ref).sum())
            assert np.allclose(objs, objs_ref, rtol=1e-5, atol=0)
        assert counts[0] == n * 3 * J * m
        assert 0 < counts[1] < counts[0]


def test_fallback_to_current_state_is_exact(lsq, oracle):
    """Option "fallback": a candidate whose codes become equal to the vector's current codes inherits that state's
    validity bits.  Pure optimisation: codes, objective and the equal / better counters identical with it on and off
    (and equal to the oracle), strictly fewer node updates recomputed.  Several ILS iterations so that vectors do fall back."""
    import torch
    d, n, m, ils, J, npert, seed = 32, 20_000, 8, [6], 4, 4, 314
    X, K, B0 = make_problem(d, n, m, seed=seed)
    Bs_ref, objs_ref, st_ref = oracle.encode_icm(X, B0, K, m, H, ils, J, npert, True, seed, want_stats=True)
    dX, dK = torch.from_numpy(X).cuda(), torch.from_numpy(K).cuda()
    dB = torch.from_numpy((B0 - 1).astype(np.uint8)).cuda()
    counts = {}
    for fb in (1, 0):
        for light in (-1, 0):                                  # both node-update paths
            with lsq.Engine(0, profile=True) as eng:
                eng.set_option("fallback", fb)
                eng.set_option("light", light)
                dBs, sums, stats = eng.encode_icm_dev(dX, dB, dK, m, ils, J, npert, True, seed=seed)
                counts[(fb, light)] = eng.timings()["icm_node_updates"]
                assert np.array_equal(dBs.cpu().numpy().astype(np.int16) + 1, Bs_ref), "fallback=%d light=%d" % (fb, light)
                assert np.allclose(sums / n, objs_ref, rtol=1e-5, atol=0)
                assert np.array_equal(stats, st_ref.astype(np.int64))
    assert counts[(1, -1)] == counts[(1, 0)] and counts[(0, -1)] == counts[(0, 0)]
    assert counts[(1, -1)] < counts[(0, -1)]


def test_device_api_chunking_and_offsets(lsq, oracle):
    """Results must not depend on the resident chunk size nor on how the caller shards (P8):
    encode [0,n) in one call == two calls on halves with global_offset."""
    import torch
    d, n, m, ils, J, npert, seed = 128, 1000, 8, [1, 3], 4, 4, 21
    X, K, B0 = make_problem(d, n, m, seed=seed)
    Bs_ref, objs_ref, st_ref = oracle.encode_icm(X, B0, K, m, H, ils, J, npert, True, seed, want_stats=True)
    dX, dK = torch.from_numpy(X).cuda(), torch.from_numpy(K).cuda()
    dB = torch.from_numpy((B0 - 1).astype(np.uint8)).cuda()
    with lsq.Engine(0, chunk=192) as eng:           # 6 chunks, ragged tail
        dBs, sums, stats = eng.encode_icm_dev(dX, dB, dK, m, ils, J, npert, True, seed=seed)
        got = dBs.cpu().numpy().astype(np.int16) + 1
        assert np.array_equal(got, Bs_ref)
        assert np.allclose(sums / n, objs_ref, rtol=1e-5, atol=0)
        assert np.array_equal(stats, st_ref.astype(np.int64))
        # two shards with offsets
        h1 = 437
        a, sa, _ = eng.encode_icm_dev(dX[:h1].contiguous(), dB[:h1].contiguous(), dK, m, ils, J, npert, True, seed=seed, global_offset=0)
        b, sb, _ = eng.encode_icm_dev(dX[h1:].contiguous(), dB[h1:].contiguous(), dK, m, ils, J, npert, True, seed=seed, global_offset=h1)
        both = torch.cat([a, b], dim=1).cpu().numpy().astype(np.int16) + 1
        assert np.array_equal(both, Bs_ref)
        assert np.allclose((sa + sb) / n, objs_ref, rtol=1e-5, atol=0)


def test_host_api_chunking(lsq, oracle):
    """Host-buffer entry point with several resident chunks: chunk c+1's X is uploaded on a second stream under the
    compute of chunk c (double-buffered staging) -- results must equal the one-chunk call and the oracle, for
    1, 2, 3 (odd: both staging buffers end up last) and many ragged chunks, and on repeated calls of one context."""
    d, n, m, ils, J, npert, seed = 64, 1531, 8, [2, 3], 3, 4, 5
    X, K, B0 = make_problem(d, n, m, seed=seed)
    Bs_ref, objs_ref = oracle.encode_icm(X, B0, K, m, H, ils, J, npert, True, seed)
    for chunk in (4096, 800, 600, 127):
        with lsq.Engine(0, chunk=chunk) as eng:
            for _ in range(2):
                Bs, objs = eng.encode_icm(X, B0, K, m, ils, J, npert, True, seed=seed)
                assert np.array_equal(Bs, Bs_ref), "chunk %d: %d codes differ" % (chunk, (Bs != Bs_ref).sum())
                assert np.allclose(objs, objs_ref, rtol=1e-5, atol=0)


def test_reference_shaped_api(lsq, oracle):
    """The Julia-shaped mirror: encode_icm_cuda / encoding_icm / encode_icm_fully / helpers."""
    d, n, m, seed = 128, 200, 8, 33
    X, K, B0 = make_problem(d, n, m, seed=seed)
    C = [np.ascontiguousarray(K[j * H:(j + 1) * H].T) for j in range(m)]      # list of (d, h)
    RX, B = np.asfortranarray(X.T), np.asfortranarray(B0.T)                    # Julia shapes
    Bs, objs = lsq.encode_icm_cuda(RX, B, C, [2, 4], 4, 4, True, 2, False, seed=seed)
    Bs_ref, objs_ref = oracle.encode_icm(X, B0, K, m, H, [2, 4], 4, 4, True, seed)
    assert len(Bs) == 2 and Bs[0].shape == (m, n) and Bs[0].dtype == np.int16
    assert np.array_equal(Bs[1].T, Bs_ref[1]) and np.array_equal(Bs[0].T, Bs_ref[0])
    assert np.allclose(objs, objs_ref, rtol=1e-5, atol=0)
    # encoding_icm chained == the reference demo loop `for i=1:ilsiter B = encoding_icm(...)` (demo_lsq.jl:48-51)
    Bc = B.copy()
    for it in range(4):
        Bc = lsq.encoding_icm(RX, Bc, C, 4, True, 4, False, seed=seed, it=it)
    assert np.array_equal(Bc.T, Bs_ref[1])
    # the worker without the accept test
    Bw = np.array(B, dtype=np.int16, order="F")
    lsq.encode_icm_fully(Bw, RX, C, None, None, 4, True, 4, (1, n), False, seed=seed, it=0)
    ref_w = oracle.encoding_icm_faithful(X, B0, K, m, H, 4, True, 4, seed, 0)    # accept applied on top
    cost_w = lsq.veccost(RX, Bw, C)
    cost_0 = lsq.veccost(RX, B, C)
    expect = np.where((cost_w < cost_0)[:, None], Bw.T, B0)
    assert np.array_equal(expect, ref_w)
    # helpers
    un = lsq.get_unaries(RX, C)
    assert len(un) == m and un[0].shape == (H, n)
    assert np.array_equal(np.stack([u.T for u in un]), oracle.unaries(X, K, m, H))
    bins, cbi = lsq.get_binaries(C)
    assert len(bins) == m * (m - 1) // 2 and cbi.shape == (2, len(bins))
    T = oracle.tables(K, m, H)
    assert np.array_equal(bins[0], T[0, 1].T) and tuple(cbi[:, 0]) == (1, 2)
    assert abs(lsq.qerror(RX, Bs[1], C) - objs_ref[1]) <= 1e-5 * objs_ref[1]


def test_chained_default_calls_equal_the_whole_call(lsq, oracle):
    """The reference demo loop `for i = 1:ilsiter; B = encoding_icm(X, B, C, niter, randord, npert, V); end` (demos/demo_lsq.jl:48-51)
    through the reference's own argument list -- no iteration index: the context counts (LSQ_IT_AUTO).  8 chained default-argument calls
    == encode_icm_cuda(..., [8], ...) == the oracle.  A fixed index on every call would re-draw the same perturbation:
    shown here to give different codes."""
    d, n, m, seed, I = 64, 700, 8, 77, 8
    X, K, B0 = make_problem(d, n, m, seed=seed)
    C = [np.ascontiguousarray(K[j * H:(j + 1) * H].T) for j in range(m)]
    RX, B = np.asfortranarray(X.T), np.asfortranarray(B0.T)
    Bs_ref, _ = oracle.encode_icm(X, B0, K, m, H, [I], 4, 4, True, seed)
    with lsq.Engine(0) as eng:
        Bc = B.copy()
        for _ in range(I):
            Bc = lsq.encoding_icm(RX, Bc, C, 4, True, 4, False, seed=seed, engine=eng)          # the reference's positional arguments only
        assert np.array_equal(Bc.T, Bs_ref[0])
        Bs, _ = lsq.encode_icm_cuda(RX, B, C, [I], 4, 4, True, 2, False, seed=seed, engine=eng)
        assert np.array_equal(Bs[0], Bc)
        # the counter went on: the same chained loop now continues the sequence (iterations 8..15) ...
        Bd = B.copy()
        for _ in range(I):
            Bd = lsq.encoding_icm(RX, Bd, C, 4, True, 4, False, seed=seed, engine=eng)
        assert not np.array_equal(Bd, Bc)
        # ... and "ils_counter" rewinds it
        eng.set_option("ils_counter", 0)
        Be = B.copy()
        for _ in range(I):
            Be = lsq.encoding_icm(RX, Be, C, 4, True, 4, False, seed=seed, engine=eng)
        assert np.array_equal(Be, Bc)
        # the trap this removes: the same explicit index on every call
        Bf = B.copy()
        for _ in range(I):
            Bf = lsq.encoding_icm(RX, Bf, C, 4, True, 4, False, seed=seed, it=0, engine=eng)
        assert not np.array_equal(Bf, Bc)
        # the worker shares the counter: perturbation of iteration 0 after a rewind == explicit it = 0
        eng.set_option("ils_counter", 0)
        Bw0 = np.array(B, dtype=np.int16, order="F")
        lsq.encode_icm_fully(Bw0, RX, C, None, None, 4, True, 4, (1, n), False, seed=seed, engine=eng)
        Bw1 = np.array(B, dtype=np.int16, order="F")
        lsq.encode_icm_fully(Bw1, RX, C, None, None, 4, True, 4, (1, n), False, seed=seed, it=0, engine=eng)
        assert np.array_equal(Bw0, Bw1)


def test_ties_pick_lowest_index(lsq, oracle):
    """Duplicate codewords create exact ties; the node update must return the LOWEST index (P3),
    which the reference CUDA tree reduction does not guarantee."""
    d, n, m, seed = 32, 128, 4, 55
    X, K, B0 = make_problem(d, n, m, seed=seed, kind="gauss")
    K = K.reshape(m, H, d).copy()
    K[:, 1::2] = K[:, 0::2]            # every codeword appears twice (indices 2a and 2a+1)
    K[1, 200:] = K[1, 3]               # and a long run of copies
    K = K.reshape(m * H, d)
    Bs_ref, _ = oracle.encode_icm(X, B0, K, m, H, [2], 4, 2, True, seed)
    with lsq.Engine(0) as eng:
        Bs, _ = eng.encode_icm(X, B0, K, m, [2], 4, 2, True, seed=seed)
    assert np.array_equal(Bs, Bs_ref)
    changed = Bs[0] != B0
    assert ((Bs[0][changed] - 1) % 2 == 0).all(), "a tie was resolved to the higher duplicate"


@pytest.mark.parametrize("n", [300, 80_000])     # 300: every block is "light" (L2-gather path); 80 000: 313 vectors per block, LDS-staged path
def test_nonfinite_inputs_follow_the_reference_scan(lsq, oracle, n):
    """NaN / Inf in the data: the reference's argmin is a strict-'<' scan (encode_icm.jl:105-119), so a NaN candidate never
    wins unless it sits at index 0, -0 == +0, and a NaN cost is never accepted (`<` is false).  Both node-update paths of the
    walk kernel (packed LDS atomic keys / wave DPP argmin) and the cost kernel must reproduce the oracle bit for bit."""
    d, m, seed = 16, 8, 91
    X, K, B0 = make_problem(d, n, m, seed=seed, kind="gauss")
    rng = np.random.default_rng(4)
    bad = rng.choice(n, size=40, replace=False)
    X[bad[:10], 0] = np.nan                              # whole unary rows NaN
    X[bad[10:20], 3] = np.inf                            # +-Inf / NaN mix in the unaries
    X[bad[20:30], 5] = -np.inf
    X[bad[30:], :] = 0.0                                 # zero vectors: exact zeros and signed zeros in the sums
    K = K.copy()
    K[7] = 0.0
    K[300] = -0.0
    import torch
    Bs_ref, objs_ref, st_ref = oracle.encode_icm(X, B0, K, m, H, [1, 2, 4], 3, 4, True, seed, want_stats=True)
    for options in ({}, {"schedule": 6, "q16_min": 0}, {"schedule": 4}, {"schedule": 3}):      # {}: the shipped defaults
        with open_engine(lsq, options) as eng:
            Bs, objs = eng.encode_icm(X, B0, K, m, [1, 2, 4], 3, 4, True, seed=seed)
            assert np.array_equal(Bs, Bs_ref), "%r: %d codes differ" % (options, (Bs != Bs_ref).sum())
            assert np.array_equal(np.isnan(objs), np.isnan(objs_ref))
            # the "% equal / % better" counters too: a vector whose codes come back unchanged is "equal" without a cost
            # evaluation -- unless its cost is NaN, which the reference's `==` never counts
            dBs, _, stats = eng.encode_icm_dev(torch.from_numpy(X).cuda(), torch.from_numpy((B0 - 1).astype(np.uint8)).cuda(),
                                               torch.from_numpy(K).cuda(), m, [4], 3, 4, True, seed=seed)
            assert np.array_equal(stats, st_ref.astype(np.int64))


def test_staged_path_full_oracle_parity(lsq, oracle):
    """A shape where every block holds more vectors than the light-block threshold (so the LDS-staged walk runs) and
    several passes per block at a small chunk -- compared with the oracle on ALL vectors, not a sample."""
    d, n, m, ils, J, npert, seed = 16, 150_000, 8, [2], 3, 4, 23
    X, K, B0 = make_problem(d, n, m, seed=seed, kind="gauss")
    Bs_ref, objs_ref = oracle.encode_icm(X, B0, K, m, H, ils, J, npert, True, seed)
    with lsq.Engine(0) as eng:
        Bs, objs = eng.encode_icm(X, B0, K, m, ils, J, npert, True, seed=seed)
    assert np.array_equal(Bs, Bs_ref), "%d codes differ" % (Bs != Bs_ref).sum()
    assert np.allclose(objs, objs_ref, rtol=1e-5, atol=0)


def test_generators_match_oracle(engine, oracle):
    X = engine.synth_data_u8_dev(1234, 300, 128, global_offset=17).cpu().numpy()
    assert np.array_equal(X, oracle.synth_data_u8(1234, 300, 128, global_offset=17))
    X2 = engine.synth_data_u8_dev(5, 10, 1030).cpu().numpy()
    assert np.array_equal(X2, oracle.synth_data_u8(5, 10, 1030))
    B = engine.randinit_dev(9, 1000, 7, global_offset=5).cpu().numpy()
    assert np.array_equal(B.astype(np.int16) + 1, oracle.randinit(9, 1000, 7, H, global_offset=5))


def test_errors_are_loud(lsq, engine):
    X = np.zeros((4, 8), np.float32)
    K = np.zeros((2 * 256, 8), np.float32)
    B = np.ones((4, 2), np.int16)
    with pytest.raises(lsq._lib.LsqError):
        engine.encode_icm(X, B * 300, K, 2, [1], 1, 1, True)          # code out of range
    with pytest.raises(lsq._lib.LsqError):
        engine.encode_icm(X, B, K, 2, [0], 1, 1, True)                # ilsiters < 1
    with pytest.raises(lsq._lib.LsqError):
        engine.get_unaries(X, np.zeros((2 * 128, 8), np.float32), 2, h=128)   # h != 256
    # empty input is fine
    Bs, objs = engine.encode_icm(np.zeros((0, 8), np.float32), np.zeros((0, 2), np.int16), K, 2, [1], 1, 1, True)
    assert Bs.shape == (1, 0, 2)


def test_full_size_properties(lsq):
    """BASELINE config sizes (10^6 x 128, m = 8) are beyond what the oracle finishes in seconds, so parity at
    full size is checked through size-independent properties that follow from the reference semantics
    (SURVEY P2/P6/P8/P10): monotone per-vector cost, strict-accept rule, objective = mean cost, determinism,
    and invariance to sharding / chunking / schedule."""
    import torch
    n, d, m, ils, J, npert, seed = 1_000_000, 128, 8, [1, 3], 4, 4, 42
    with lsq.Engine(0) as eng, lsq.Engine(0, chunk=300_000, schedule=3) as eng2, lsq.Engine(0, schedule=4) as eng4:
        dX = eng.synth_data_u8_dev(1234, n, d)
        dB0 = eng.randinit_dev(7, n, m)
        dK = eng.synth_codebooks_dev(4321, m, d)
        dBs, sums, stats = eng.encode_icm_dev(dX, dB0, dK, m, ils, J, npert, True, seed=seed)
        torch.cuda.synchronize()
        X, K = dX.cpu().numpy(), dK.cpu().numpy()
        B0 = dB0.cpu().numpy().astype(np.int16) + 1
        B1 = dBs[0].cpu().numpy().astype(np.int16) + 1
        B3 = dBs[1].cpu().numpy().astype(np.int16) + 1
        c0, c1, c3 = (eng.veccost(X, B, K, m) for B in (B0, B1, B3))
        assert np.all(c1 <= c0) and np.all(c3 <= c1)                           # P2/P6: cost never increases
        assert np.array_equal(B1[c1 == c0], B0[c1 == c0])                      # not strictly better -> input kept bit for bit
        assert np.array_equal(B3[c3 == c1], B1[c3 == c1])
        assert abs(sums[0] / n - c1.astype(np.float64).mean()) <= 1e-6 * sums[0] / n      # P10: objective = mean cost
        assert abs(sums[1] / n - c3.astype(np.float64).mean()) <= 1e-6 * sums[1] / n
        assert stats[0, 1] == int((c1 < c0).sum())                             # "% better" counter of iteration 1
        assert sums[1] < sums[0] < c0.astype(np.float64).sum()
        assert B3.min() >= 1 and B3.max() <= 256
        # determinism + invariance: other schedule, 4 ragged chunks, and two shards with global offsets
        dBs2, sums2, _ = eng2.encode_icm_dev(dX, dB0, dK, m, ils, J, npert, True, seed=seed)
        assert torch.equal(dBs2, dBs)
        assert np.allclose(sums2, sums, rtol=1e-9)
        # the default is the 16-bit filtered walk: the f32 walk must give the same codes, sums, counters and memoisation counts
        tq = eng.timings()
        dBs4, sums4, stats4 = eng4.encode_icm_dev(dX, dB0, dK, m, ils, J, npert, True, seed=seed)
        t4 = eng4.timings()
        assert torch.equal(dBs4, dBs) and np.array_equal(sums4, sums) and np.array_equal(stats4, stats)
        assert tq["filtered_blocks"] > 0 and t4["filtered_blocks"] == 0 and t4["staged_blocks"] > 0
        assert tq["icm_node_updates"] == t4["icm_node_updates"]
        h1 = 400_001
        a, sa, _ = eng.encode_icm_dev(dX[:h1].contiguous(), dB0[:h1].contiguous(), dK, m, ils, J, npert, True, seed=seed, global_offset=0)
        b, sb, _ = eng.encode_icm_dev(dX[h1:].contiguous(), dB0[h1:].contiguous(), dK, m, ils, J, npert, True, seed=seed, global_offset=h1)
        assert torch.equal(torch.cat([a, b], dim=1), dBs)                      # P8
        assert np.allclose(sa + sb, sums, rtol=1e-9)
        # the two node-update paths of the walk kernel at full size: every block staged (light = 0) vs every block gathering
        # from L2 (light = 4096, on a quarter of the data to keep the run short), with and without the exact skip
        q = n // 4
        ref_q, sums_q, _ = eng.encode_icm_dev(dX[:q].contiguous(), dB0[:q].contiguous(), dK, m, ils, J, npert, True, seed=seed)
        for light, skip in ((0, 1), (4096, 1), (4096, 0)):
            with lsq.Engine(0, skip=skip) as e3:
                e3.set_option("light", light)
                got_q, s_q, _ = e3.encode_icm_dev(dX[:q].contiguous(), dB0[:q].contiguous(), dK, m, ils, J, npert, True, seed=seed)
                assert torch.equal(got_q, ref_q), "light=%d skip=%d" % (light, skip)
                assert np.allclose(s_q, sums_q, rtol=1e-9)


@pytest.mark.parametrize("d,m", [(960, 8), (128, 16)])
def test_small_chunk_road_at_the_large_shapes_sample_vs_oracle(lsq, oracle, d, m):
    """The SMALL-CHUNK road (n = 60 000 < q16_min: f32 walk, every block light) at the dimensions of cfg3 (m = 16) and cfg4 (d = 960): what a
    trainer-sized call of those shapes runs.  (The filtered walk at these shapes is covered at their real sizes by tests/test_gpu_staged.py:
    test_cfg3_m16_staged_sample_and_full_size_properties, test_cfg4_per_gpu_share_runs_the_filtered_walk -- VERDICT r3, weak #8.)  A random
    sample of vectors against the oracle run on exactly those vectors (results depend only on the global index, P8); the counters assert the road."""
    import torch
    n, ils, J, npert, seed = 60_000, [2], 4, 4, 11
    with lsq.Engine(0) as eng:
        dX = eng.synth_data_u8_dev(77, n, d)
        dB0 = eng.randinit_dev(8, n, m)
        dK = eng.synth_codebooks_dev(99, m, d)
        dBs, sums, _ = eng.encode_icm_dev(dX, dB0, dK, m, ils, J, npert, True, seed=seed)
        torch.cuda.synchronize()
        t = eng.timings()
        assert t["filtered_blocks"] == 0 and t["staged_blocks"] + t["light_blocks"] > 0, t
        X, K = dX.cpu().numpy(), dK.cpu().numpy()
        B0 = dB0.cpu().numpy().astype(np.int16) + 1
        got = dBs[0].cpu().numpy().astype(np.int16) + 1
    rng = np.random.default_rng(0)
    for i in np.sort(rng.choice(n, size=24, replace=False)):
        ref, _ = oracle.encode_icm(X[i:i + 1], B0[i:i + 1], K, m, H, ils, J, npert, True, seed, global_offset=int(i))
        assert np.array_equal(ref[0, 0], got[i]), "vector %d differs" % i


def _run_c_consumer(tmp_path, X, B0, K, m, ils, J, npert, randord, seed):
    """Builds tests/c_abi_consumer.c with plain gcc and runs it in a fresh process (no Python / torch inside)."""
    import os
    import struct
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "c_abi_consumer")
    libdir = os.path.join(root, "local-search-quantization_amd")
    subprocess.check_call(["gcc", "-O2", os.path.join(root, "tests", "c_abi_consumer.c"), "-I", os.path.join(root, "include"),
                           "-L", libdir, "-llsq_mi355x", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    n, d = X.shape
    ils = np.asarray(ils, dtype=np.int64)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<8i", d, n, m, H, len(ils), J, npert, int(randord)))
        f.write(struct.pack("<Q", seed))
        f.write(ils.tobytes())
        f.write(np.ascontiguousarray(X, np.float32).tobytes())
        f.write(np.ascontiguousarray(B0, np.int16).tobytes())
        f.write(np.ascontiguousarray(K, np.float32).tobytes())
    out = subprocess.check_output([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], env=dict(os.environ)).decode()
    raw = open(tmp_path / "out.bin", "rb").read()
    nb = len(ils) * n * m
    Bs = np.frombuffer(raw[:2 * nb], dtype=np.int16).reshape(len(ils), n, m)
    objs = np.frombuffer(raw[2 * nb:2 * nb + 4 * len(ils)], dtype=np.float32)
    secs = struct.unpack("<d", raw[2 * nb + 4 * len(ils):])[0]
    return Bs, objs, secs, out


def test_plain_c_consumer_matches_oracle(oracle, tmp_path):
    """Drop-in proof: a C program that only includes include/lsq_mi355x.h and links liblsq_mi355x.so (what a Julia
    ccall binding does) gets the oracle's codes bit for bit."""
    d, n, m, ils, J, npert, seed = 128, 3000, 8, [1, 3], 4, 4, 5
    X, K, B0 = make_problem(d, n, m, seed=seed)
    Bs, objs, secs, out = _run_c_consumer(tmp_path, X, B0, K, m, ils, J, npert, True, seed)
    Bs_ref, objs_ref = oracle.encode_icm(X, B0, K, m, H, ils, J, npert, True, seed)
    assert np.array_equal(Bs, Bs_ref)
    assert np.allclose(objs, objs_ref, rtol=1e-5, atol=0)


def test_single_process_multi_gpu_handle(lsq, oracle):
    """lsq_multi_*: one context + host thread per listed device, `splitarray` shards with global offsets.  With the device
    list [0, 0, 0] three shards time-share the one GPU of the test box; the result must equal the one-device call and the
    oracle bit for bit (P8), through the reference-shaped entry point as well; errors of a shard must surface."""
    d, n, m, ils, J, npert, seed = 32, 1003, 8, [1, 3], 3, 4, 17
    X, K, B0 = make_problem(d, n, m, seed=seed)
    Bs_ref, objs_ref = oracle.encode_icm(X, B0, K, m, H, ils, J, npert, True, seed)
    for devices in ([0], [0, 0, 0]):
        with lsq.MultiEngine(devices) as mg:
            Bs, objs = mg.encode_icm(X, B0, K, m, ils, J, npert, True, seed=seed)
            assert np.array_equal(Bs, Bs_ref), "%r: %d codes differ" % (devices, (Bs != Bs_ref).sum())
            assert np.allclose(objs, objs_ref, rtol=1e-5, atol=0)
            C = [np.ascontiguousarray(K[j * H:(j + 1) * H].T) for j in range(m)]
            Bj, oj = lsq.encode_icm_cuda(np.asfortranarray(X.T), np.asfortranarray(B0.T), C, ils, J, npert, True, 2, False, seed=seed, engine=mg)
            assert np.array_equal(np.stack([b.T for b in Bj]), Bs_ref)
            bad = B0.copy()
            bad[n - 1, 0] = 300                                         # lands in the last shard
            with pytest.raises(lsq._lib.LsqError, match="shard 2|codes must lie" if len(devices) == 3 else "codes must lie"):
                mg.encode_icm(X, bad, K, m, ils, J, npert, True, seed=seed)
    with pytest.raises(lsq._lib.LsqError):
        lsq.MultiEngine([99])
    # fewer vectors than devices: empty shards are fine
    with lsq.MultiEngine([0, 0, 0, 0]) as mg:
        Bs, objs = mg.encode_icm(X[:2], B0[:2], K, m, [1], J, npert, True, seed=seed)
        ref, _ = oracle.encode_icm(X[:2], B0[:2], K, m, H, [1], J, npert, True, seed)
        assert np.array_equal(Bs, ref)


def test_async_call_matches_the_blocking_call_and_can_be_captured(lsq):
    """Option "async" (VERDICT r3, weak #9): lsq_encode_icm_dev with NO host synchronisation -- the chunk's verdict and probe are taken on the device,
    both walks are enqueued, sums and counters land in device tensors in stream order.  (a) Same codes, sums and counters as the blocking call on a
    well-conditioned chunk (filtered walk) AND on a scale-mixture chunk that the probe hands to the f32 walk; (b) the statistics reach lsq_get_timings
    at its next call; (c) the call can be captured into a graph on torch's stream and replayed."""
    import torch
    d, n, m, ils, J, npert, seed = 32, 70_000, 8, [1, 3], 3, 4, 21
    with lsq.Engine(0) as eng:
        dX = eng.synth_data_u8_dev(5, n, d)
        dB0 = eng.randinit_dev(6, n, m)
        dK = eng.synth_codebooks_dev(7, m, d)
        g = torch.Generator(device=dX.device)
        g.manual_seed(3)
        dXc = (dX * torch.empty((n, 1), dtype=torch.float32, device=dX.device).cauchy_(generator=g)).contiguous()
        for X, expect_fallback in ((dX, 0), (dXc, 1)):
            ref, sums, stats = eng.encode_icm_dev(X, dB0, dK, m, ils, J, npert, True, seed=seed)
            t_ref = eng.timings()
            eng.reset_timings()
            got, sums_t, stats_t = eng.encode_icm_dev(X, dB0, dK, m, ils, J, npert, True, seed=seed, nonblocking=True)
            torch.cuda.synchronize()
            assert torch.equal(got, ref)
            # (the objective is a sum of f64 partial sums added in arrival order: equal up to the last bits)
            assert np.allclose(sums_t.cpu().numpy(), sums, rtol=1e-12, atol=0) and np.array_equal(stats_t.cpu().numpy(), stats)
            t = eng.timings()
            assert t["icm_node_updates"] == t_ref["icm_node_updates"] and t["filter_fallback_chunks"] == expect_fallback == t_ref["filter_fallback_chunks"], (t, t_ref)
            eng.reset_timings()
        # (c) graph capture on a side stream: the warm-up above sized every work buffer for this shape
        side = torch.cuda.Stream()
        out = torch.zeros((len(ils), n, m), dtype=torch.uint8, device=dX.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            eng.encode_icm_dev(dX, dB0, dK, m, ils, J, npert, True, seed=seed, out=out, nonblocking=True)      # warm-up on the capture stream
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                _, gs, gst = eng.encode_icm_dev(dX, dB0, dK, m, ils, J, npert, True, seed=seed, out=out, nonblocking=True)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        ref, sums, stats = eng.encode_icm_dev(dX, dB0, dK, m, ils, J, npert, True, seed=seed)
        assert torch.equal(out, ref) and np.allclose(gs.cpu().numpy(), sums, rtol=1e-12, atol=0) and np.array_equal(gst.cpu().numpy(), stats)
