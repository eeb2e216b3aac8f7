"""The float64 replay (tests/icm_replay.py) judging the shipped library's encoder on the device: every node decision and every accept of every
ILS iteration, returned one by one (encode_icm_dev with ilsiters = 1..I, or encoding_icm with an explicit `it`), on every route the encoder
takes -- the small-chunk wave kernel, the 16-bit filtered walk with light and with staged blocks, the f32 walk, the probe's hand-over --
with each route asserted through the context's counters.  The perturbed states come from the product (Engine.perturb).

Exact regime (small integers, tests/icm_replay.exact_problem): every f32 step is exact, so every vector-iteration must be verified and the
codes equal the replay's bit for bit.  Bounded regimes: no wrong decision and at least 90 % of the vector-iterations verified."""
import numpy as np
import pytest

import icm_replay as IR
from conftest import ENCODE_VARIANTS, make_problem, open_engine

pytestmark = pytest.mark.gpu
H = 256


def dev(a, offset=0):
    """a host array as a contiguous cuda tensor; offset > 0: a view starting `offset` elements into its allocation"""
    import torch
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + offset, dtype=torch.from_numpy(a[:0].reshape(-1)).dtype, device="cuda:0")
    t = buf[offset:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    return t


def problem(kind, n, d, m, seed):
    """exact | gauss | sift | offset (every vector and codeword moved along one direction by ~20x the data's scale) | dup (duplicated codewords and a run of copies) |
    cauchy (Cauchy-scaled rows)"""
    if kind == "exact":
        return IR.exact_problem(n, d, m, seed)
    X, K, B0 = make_problem(d, n, m, seed=seed, kind="sift" if kind == "sift" else "gauss")
    if kind == "offset":
        u = np.random.default_rng(seed).standard_normal(d).astype(np.float32)
        u /= np.linalg.norm(u)
        X, K = X + np.float32(20.0) * u, K + np.float32(20.0 / m) * u
    elif kind == "dup":
        K = K.reshape(m, H, d).copy()
        K[:, 1::2] = K[:, 0::2]
        K[0, 200:] = K[0, 3]
        K = K.reshape(m * H, d)
    elif kind == "cauchy":
        X = X * np.random.default_rng(seed).standard_cauchy((n, 1)).astype(np.float32)
    return np.ascontiguousarray(X, np.float32), np.ascontiguousarray(K, np.float32), B0


def encode_and_replay(lsq, eng, X, K, B0, m, I, J, npert, seed, randord=True, offset=0, rows=None):
    """encode_icm_dev with ilsiters = 1..I (X and K as views `offset` floats into their allocations), then the replay of `rows` (default all)
    -> (Report, timings, codes (I, n, m) 0-based)"""
    import torch
    n = X.shape[0]
    eng.reset_timings()
    dBs, _, stats = eng.encode_icm_dev(dev(X, offset), dev((B0 - 1).astype(np.uint8)), dev(K, offset), m, list(range(1, I + 1)), J, npert, randord, seed=seed)
    torch.cuda.synchronize()
    t = eng.timings()
    outs = dBs.cpu().numpy().astype(np.int64)
    rows = np.arange(n) if rows is None else np.asarray(rows)

    def perturb(codes, it):
        B = np.ones((n, m), np.int16)
        B[rows] = codes + 1
        return eng.perturb(B, npert, seed=seed, it=it)[rows].astype(np.int64) - 1

    orders = [lsq.node_order(seed, it, m, randord) for it in range(I)]
    rep = IR.replay(IR.Case(X[rows], K, m), B0[rows].astype(np.int64) - 1, [o[rows] for o in outs], perturb, orders, J, npert,
                    stats if rows.size == n else None)
    return rep, t, outs


def judge(rep, kind, what):
    rep.assert_no_wrong(what)
    f = rep.fraction_verified()
    print("%s: %s, verified %.4f" % (what, rep.counts(), f))
    if kind == "exact":
        assert rep.counts()["verified"] == rep.verdict.size, "%s: %s" % (what, rep.message())
    else:
        assert f >= 0.9, "%s: %s" % (what, rep.message())


def route(t, which):
    if which == "light":            # the wave kernel, or the light blocks of either walk
        ok = t["light_blocks"] > 0 and t["staged_blocks"] == 0 and t["filtered_blocks"] == 0
    elif which == "filtered":       # the 16-bit filtered walk, every block staged
        ok = t["filtered_blocks"] > 0 and t["staged_blocks"] == 0 and t["light_blocks"] == 0
    elif which == "filtered_natural":
        ok = t["filtered_blocks"] > 0 and t["staged_blocks"] == 0 and t["filter_fallback_chunks"] == 0
    elif which == "f32_staged":
        ok = t["staged_blocks"] > 0 and t["filtered_blocks"] == 0
    elif which == "probe":          # the first iteration filtered, the rest handed to the f32 walk
        ok = t["filter_fallback_chunks"] == 1 and t["filtered_blocks"] > 0 and t["staged_blocks"] > 0
    else:
        raise ValueError(which)
    assert ok, (which, t)


def sample_rows(n, per, extra, seed):
    """block / chunk boundaries (multiples of `per`, both sides) and a seeded random sample"""
    b = np.arange(per, n, per)
    r = set(np.concatenate([b - 1, b, [0, n - 1]]).tolist())
    r |= set(np.random.default_rng(seed).choice(n, size=extra, replace=False).tolist())
    return np.array(sorted(r))


# ---- the it convention, and the replay driven through encoding_icm ----------------------------------------------------------------------

def test_encoding_icm_it_matches_encode_icm_dev_iterations(lsq):
    d, n, m, I, J, npert, seed = 32, 1500, 8, 3, 4, 4, 21
    X, K, B0 = problem("exact", n, d, m, seed)
    with lsq.Engine(0) as eng:
        _, _, outs = encode_and_replay(lsq, eng, X, K, B0, m, I, J, npert, seed)
        assert np.array_equal(eng.perturb(B0, npert, seed=seed, it=1) - 1, IR.perturb(B0 - 1, npert, seed, 1))      # the product's perturbation = the replay's RNG
        B, chain = B0, []
        for it in range(I):
            B = eng.encoding_icm(X, B, K, m, J, True, npert, seed=seed, it=it)
            chain.append(B.astype(np.int64) - 1)
        assert all(np.array_equal(chain[it], outs[it]) for it in range(I)), "encoding_icm(it=k) is not iteration k of encode_icm_dev"
        orders = [lsq.node_order(seed, it, m, True) for it in range(I)]
        rep = IR.replay(IR.Case(X, K, m), B0.astype(np.int64) - 1, chain, lambda c, it: eng.perturb(c + 1, npert, seed=seed, it=it) - 1, orders, J, npert)
    judge(rep, "exact", "encoding_icm chain")


# ---- every variant of conftest, exact and bounded -----------------------------------------------------------------------------------------

VARIANT_ROUTE = {"default": "light", "s6_forced": "filtered", "s6_light": "light", "s4": "light", "s3": "light"}


@pytest.mark.parametrize("kind", ["exact", "gauss"])
@pytest.mark.parametrize("vid,variant", [(v.id, v.values[0]) for v in ENCODE_VARIANTS], ids=[v.id for v in ENCODE_VARIANTS])
def test_every_variant(lsq, vid, variant, kind):
    d, n, m, I, J, npert, seed = 32, 2000, 8, 3, 4, 4, 5
    X, K, B0 = problem(kind, n, d, m, seed)
    with open_engine(lsq, variant) as eng:
        rep, t, _ = encode_and_replay(lsq, eng, X, K, B0, m, I, J, npert, seed)
    route(t, VARIANT_ROUTE[vid])
    judge(rep, kind, "variant %s, %s" % (vid, kind))


# ---- m = 1 .. 16 through the forced filtered walk ---------------------------------------------------------------------------------------

S6_FORCED = [v for v in ENCODE_VARIANTS if v.id == "s6_forced"][0].values[0]


@pytest.mark.parametrize("m", list(range(1, 17)))
def test_every_m_through_the_filtered_walk(lsq, m):
    d, n, I = 24, 800, 2
    J, npert = (4, 4) if m % 2 == 0 else (1, 0 if m % 4 == 1 else m)
    X, K, B0 = problem("exact", n, d, m, 100 + m)
    with open_engine(lsq, S6_FORCED) as eng:
        rep, t, _ = encode_and_replay(lsq, eng, X, K, B0, m, I, J, npert, 100 + m)
    route(t, "filtered")
    judge(rep, "exact", "m=%d" % m)


# ---- d and alignment: the 16-byte and the 4-byte cost / accept paths ---------------------------------------------------------------------

@pytest.mark.parametrize("variant", [v for v in ENCODE_VARIANTS if v.id in ("default", "s6_forced")])
@pytest.mark.parametrize("d,offset,kind", [(1, 0, "exact"), (3, 1, "exact"), (30, 2, "exact"), (32, 0, "exact"), (33, 1, "gauss"),
                                           (128, 0, "sift"), (128, 2, "sift"), (960, 1, "gauss")])
def test_shapes_and_offset_views(lsq, variant, d, offset, kind):
    m, I, npert, seed = 8, 2, 4, d + offset
    n, J = (600, 1) if d == 960 else (1500, 2)          # d = 960, one sweep: the accepted vectors' decisions all visible (two: 81 % verified)
    X, K, B0 = problem(kind, n, d, m, seed)
    if d == 960:
        X = X * np.float32(0.1)
    with open_engine(lsq, variant) as eng:
        rep, t, _ = encode_and_replay(lsq, eng, X, K, B0, m, I, J, npert, seed, offset=offset)
    route(t, "filtered" if variant.get("light") == 0 else "light")
    judge(rep, kind, "d=%d offset=%d %s" % (d, offset, kind))


# ---- the data ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [v for v in ENCODE_VARIANTS if v.id in ("default", "s6_forced")])
@pytest.mark.parametrize("kind,npert", [("sift", 4), ("offset", 4), ("dup", 4), ("exact", 0), ("gauss", 0)])
def test_data(lsq, variant, kind, npert):
    d, n, m, I, J, seed = 32, 2000, 8, 3, 4, 61
    X, K, B0 = problem(kind, n, d, m, seed)
    with open_engine(lsq, variant) as eng:
        rep, t, _ = encode_and_replay(lsq, eng, X, K, B0, m, I, J, npert, seed)
    route(t, "filtered" if variant.get("light") == 0 else "light")
    judge(rep, kind, "%s npert=%d" % (kind, npert))


# ---- the routes at size: a sample of ~2000 rows with the block and chunk boundaries --------------------------------------------------------

def test_filtered_walk_staged_blocks_across_chunks(lsq):
    """Default options, two resident chunks of 75 000 (> q16_min): the filtered walk with its staged blocks (293 vectors each)."""
    d, n, m, I, J, npert, seed, chunk = 32, 150_000, 8, 2, 3, 4, 71, 75_000
    X, K, B0 = problem("exact", n, d, m, seed)
    rows = np.unique(np.concatenate([sample_rows(chunk, -(-chunk // 256), 900, 1), chunk + sample_rows(chunk, -(-chunk // 256), 900, 2)]))
    with lsq.Engine(0, chunk=chunk) as eng:
        eng.set_option("filter_probe_div", 0)            # exact ties everywhere: keep the filtered walk on every iteration
        eng.set_option("filter_fallback_div", 0)
        rep, t, _ = encode_and_replay(lsq, eng, X, K, B0, m, I, J, npert, seed, rows=rows)
    route(t, "filtered_natural")
    judge(rep, "exact", "filtered walk, staged blocks, %d rows" % rows.size)


def test_filtered_walk_light_blocks(lsq):
    """schedule 6 on a chunk below q16_min with the wave kernel off: every block of the filtered walk is light (157 vectors)."""
    d, n, m, I, J, npert, seed = 24, 40_000, 8, 2, 3, 4, 72
    X, K, B0 = problem("dup", n, d, m, seed)
    with lsq.Engine(0, schedule=6) as eng:
        for k, v in (("q16_min", 0), ("wave_max", 0), ("filter_probe_div", 0), ("filter_fallback_div", 0)):
            eng.set_option(k, v)
        rep, t, _ = encode_and_replay(lsq, eng, X, K, B0, m, I, J, npert, seed, rows=sample_rows(n, -(-n // 256), 1500, 3))
    route(t, "light")
    judge(rep, "dup", "filtered walk, light blocks")


def test_f32_walk_staged_blocks(lsq):
    d, n, m, I, J, npert, seed = 32, 20_000, 8, 2, 3, 4, 73
    X, K, B0 = problem("sift", n, d, m, seed)
    with lsq.Engine(0, schedule=4) as eng:
        eng.set_option("light", 0)
        rep, t, _ = encode_and_replay(lsq, eng, X, K, B0, m, I, J, npert, seed, rows=sample_rows(n, -(-n // 256), 1500, 4))
    route(t, "f32_staged")
    judge(rep, "sift", "f32 walk, staged blocks")


def test_probe_hands_cauchy_rows_to_the_f32_walk(lsq):
    d, n, m, I, J, npert, seed = 16, 40_000, 8, 3, 3, 4, 79
    X, K, B0 = problem("cauchy", n, d, m, seed)
    with lsq.Engine(0, schedule=6) as eng:
        for k, v in (("q16_min", 0), ("light", 0), ("filter_fallback_div", 0)):
            eng.set_option(k, v)
        rep, t, _ = encode_and_replay(lsq, eng, X, K, B0, m, I, J, npert, seed, rows=sample_rows(n, -(-n // 256), 1500, 5))
    route(t, "probe")
    judge(rep, "cauchy", "probe hand-over")
