"""The 8-bit encode on the device: lsq_encode_icm_u8 / lsq_encode_icm_u8_dev / lsq_multi_encode_icm_u8 against the two references they have.

uint8 -> float32 is exact, so for random uint8 data X8 three results must agree on the codes of every snapshot:
    (a) the new call on X8,
    (b) the shipped f32 call on X8.astype(float32), same seed, on a FRESH engine,
    (c) the CPU oracle on the widened data;
(a) and (b) also on objs / obj_sums as identical BITS and on the stats counters exactly; (a) and (c) on the objective within the project's 1e-5.
Every case runs both the host-buffer and the device-resident entry point (the latter returns the counters).  The oracle's result does not depend on the
engine's options, so one oracle run serves all option sets of a shape."""
import numpy as np
import pytest

from conftest import ENCODE_VARIANTS, open_engine
from ctx_ops import COUNTERS
from q16_cases import FILTER, FORCED

pytestmark = pytest.mark.gpu

H = 256
OPTIONS = {v.id: dict(v.values[0]) for v in ENCODE_VARIANTS}      # default, s6_forced, s6_light (q16_min = 0 alone), s4, s3
assert OPTIONS["s6_forced"] == FORCED and OPTIONS["s6_light"] == {"schedule": 6, "q16_min": 0}
OPTIONS["filter"] = dict(FILTER)                                    # forced, with the product's cap on flagged pairs in force (the fall-back road)
MAIN = [k for k in OPTIONS if k != "filter"]
ILS, J, NPERT, SEED = [1, 2], 3, 3, 11


def make_u8(d, n, m, seed):
    """random uint8 rows; codebooks = random byte vectors / m (the scale of a sum of m codewords is the data's); random initial codes"""
    import oracle as O
    rng = np.random.default_rng(seed)
    X8 = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
    K = np.ascontiguousarray(rng.integers(0, 256, size=(m * H, d)).astype(np.float32) / np.float32(m))
    return X8, K, O.randinit(3000 + seed, n, m, H)


def _blocks(n):
    """row ranges the oracle re-encodes at their global indices (a result depends on (vector, global index) only)"""
    return [(0, n)] if n <= 20_000 else [(0, 256), (n // 2 - 128, n // 2 + 128), (n - 256, n)]


_REF = {}


def oracle_ref(oracle, key, X8, K, B0, m, ils=ILS, goff=0):
    if key not in _REF:
        Xf = X8.astype(np.float32)
        _REF[key] = [((a, b), oracle.encode_icm(Xf[a:b], B0[a:b], K, m, H, ils, J, NPERT, True, SEED, global_offset=goff + a, want_stats=True))
                     for a, b in _blocks(X8.shape[0])]
    return _REF[key]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def dev_view(X8, off):
    """X8 on the device as a view that starts `off` bytes into a larger (256-byte-aligned) allocation"""
    import torch
    n, d = X8.shape
    buf = torch.zeros(n * d + 16, dtype=torch.uint8, device="cuda:0")
    v = buf[off:off + n * d].view(n, d)
    v.copy_(torch.from_numpy(X8))
    assert v.is_contiguous() and v.data_ptr() % 4 == off % 4
    return v


def host_view(X8, off):
    n, d = X8.shape
    buf = np.zeros(n * d + 64, dtype=np.uint8)
    base = (-buf.ctypes.data) % 16                        # a 16-byte boundary inside the buffer, then `off` bytes past it
    v = buf[base + off:base + off + n * d].reshape(n, d)
    v[...] = X8
    assert v.flags["C_CONTIGUOUS"] and v.ctypes.data % 16 == off
    return v


def run_both(eng, X, K, B0, m, ils=ILS, goff=0, dX=None, nonblocking=False):
    """host-buffer and device-resident call on one engine -> (Bs int16 1-based, objs f32, dBs 1-based, sums f64, stats, counter deltas)"""
    import torch
    t0 = eng.timings()
    Bs, objs = eng.encode_icm(X, B0, K, m, ils, J, NPERT, True, seed=SEED, global_offset=goff)
    dBs, sums, stats = eng.encode_icm_dev(dev(X) if dX is None else dX, dev((B0 - 1).astype(np.uint8)), dev(K), m, ils, J, NPERT, True, seed=SEED,
                                          global_offset=goff, nonblocking=nonblocking)
    torch.cuda.synchronize()
    if nonblocking:
        assert sums.is_cuda and stats.is_cuda, "async results must stay on the device"
        sums, stats = sums.cpu().numpy(), stats.cpu().numpy()
    t1 = eng.timings()
    return Bs, objs, dBs.cpu().numpy().astype(np.int16) + 1, np.asarray(sums), np.asarray(stats), np.array([t1[k] - t0[k] for k in COUNTERS])


def check_triple(lsq, oracle, key, X8, K, B0, m, options, ils=ILS, goff=0, X8_host=None, X8_dev=None, nonblocking=False, same_counters=False):
    n = X8.shape[0]
    with open_engine(lsq, options) as e8:
        a = run_both(e8, X8 if X8_host is None else X8_host, K, B0, m, ils, goff, dX=X8_dev, nonblocking=nonblocking)
    with open_engine(lsq, options) as ef:
        b = run_both(ef, X8.astype(np.float32), K, B0, m, ils, goff, nonblocking=nonblocking)
    print("%s: objs u8 %r f32 %r; sums u8 %r f32 %r; stats u8 %r" % (key, a[1].tolist(), b[1].tolist(), a[3].tolist(), b[3].tolist(), a[4].tolist()))
    # (a) == (b): codes, objective bits, accept counters
    assert np.array_equal(a[0], b[0]), "host call: %d codes differ from the f32 call" % int((a[0] != b[0]).sum())
    assert np.array_equal(a[2], b[2]), "device call: %d codes differ from the f32 call" % int((a[2] != b[2]).sum())
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), (a[1], b[1])
    assert np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64)), (a[3], b[3])
    assert np.array_equal(a[4], b[4]), (a[4], b[4])
    assert np.array_equal(a[0], a[2]), "host and device entry points disagree"
    if same_counters:        # aligned rows: sigma, the sampled ranges and so every level are the f32 call's numbers -> the same roads, block by block
        assert np.array_equal(a[5], b[5]), dict(zip(COUNTERS, zip(a[5].tolist(), b[5].tolist())))
    # (a) == (c): codes of the checked rows, objective within 1e-5, the counters
    for (r0, r1), (ref, robj, rstats) in oracle_ref(oracle, key, X8, K, B0, m, ils, goff):
        assert np.array_equal(a[0][:, r0:r1], ref), "%d codes differ from the oracle in rows %d..%d" % (int((a[0][:, r0:r1] != ref).sum()), r0, r1)
        if (r0, r1) == (0, n):
            assert np.allclose(a[1], robj, rtol=1e-5, atol=0), (a[1], robj)
            assert np.allclose(a[3] / max(n, 1), robj, rtol=1e-5, atol=0), (a[3] / max(n, 1), robj)
            assert np.array_equal(a[4], rstats.astype(np.int64)), (a[4], rstats)
    return a


# ---- d: every loader road, under every option set -----------------------------------------------------------------------------------------------------
# 128: dword loads, one 128-byte line per row | 32 | 30: byte loads, rows 2-byte aligned | 33: odd | 260: past the short shift kernel's 256 |
# 960 at n = 301: LONGV, the GEMM's last K tile (960 = 60 x 16) at its boundary
D_CASES = [(128, 1000), (32, 1000), (30, 1000), (33, 1000), (260, 1000), (960, 301)]


@pytest.mark.parametrize("opt", MAIN)
@pytest.mark.parametrize("d, n", D_CASES)
def test_every_d_road_under_every_option_set(lsq, oracle, d, n, opt):
    X8, K, B0 = make_u8(d, n, 8, seed=d)
    check_triple(lsq, oracle, ("d", d, n), X8, K, B0, 8, OPTIONS[opt])


# ---- n (row-tile tails) x m, on the dword road and on the byte road ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, opt", [(128, "default"), (30, "s6_forced")])
@pytest.mark.parametrize("m", [1, 4, 8, 16])
@pytest.mark.parametrize("n", [1, 127, 129])
def test_row_tile_tails_and_every_m(lsq, oracle, n, m, d, opt):
    X8, K, B0 = make_u8(d, n, m, seed=7 * n + m)
    check_triple(lsq, oracle, ("nm", d, n, m), X8, K, B0, m, OPTIONS[opt])


@pytest.mark.parametrize("opt", MAIN)
@pytest.mark.parametrize("m", [1, 4, 16])
def test_every_m_under_every_option_set(lsq, oracle, m, opt):
    X8, K, B0 = make_u8(32, 1000, m, seed=50 + m)
    check_triple(lsq, oracle, ("m", m), X8, K, B0, m, OPTIONS[opt])


# ---- alignment: d % 4 == 0 with the base 1, 2 and 3 bytes past a 16-byte boundary (host) / a 256-byte one (device) ------------------------------------------
@pytest.mark.parametrize("opt", ["default", "s6_forced"])
@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("d", [32, 128])
def test_base_pointer_at_any_byte_offset(lsq, oracle, d, off, opt):
    X8, K, B0 = make_u8(d, 1000, 8, seed=d)                # the data of the d cases: the same oracle run
    check_triple(lsq, oracle, ("d", d, 1000), X8, K, B0, 8, OPTIONS[opt], X8_host=host_view(X8, off), X8_dev=dev_view(X8, off))


# ---- default options above q16_min: the size tests/ctx_ops.py uses -- verdict and probe on 8-bit rows -------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    return make_u8(32, 70_001, 8, seed=70)


def test_default_options_above_q16_min(lsq, oracle, big):
    X8, K, B0 = big
    check_triple(lsq, oracle, ("big",), X8, K, B0, 8, {}, same_counters=True)


def test_host_pipeline_sample_road_on_8bit_rows(lsq, oracle, big):
    """the first chunk goes up panel by panel (five 512 KB panels of 8-bit rows), the level parameters come from the host-side row sample"""
    X8, K, B0 = big
    a = check_triple(lsq, oracle, ("big",), X8, K, B0, 8, {"upload_pipeline_min_bytes": 1, "upload_panel_bytes": 1 << 19}, same_counters=True)
    assert a[5][COUNTERS.index("filtered_blocks")] > 0, "the filtered walk did not run: %r" % (dict(zip(COUNTERS, a[5].tolist())),)


# ---- chunk boundary: 1 300 vectors over resident chunks of 512, global_offset != 0 ----------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["default", "s6_forced", "filter"])
def test_call_spanning_several_resident_chunks(lsq, oracle, opt):
    X8, K, B0 = make_u8(32, 1300, 4, seed=13)
    check_triple(lsq, oracle, ("chunk",), X8, K, B0, 4, dict(OPTIONS[opt], chunk=512), goff=777)


# ---- data edges ---------------------------------------------------------------------------------------------------------------------------------------------
def edge_data(d=32, n=1000, m=4, seed=5):
    X8, K, B0 = make_u8(d, n, m, seed)
    q = n // 4
    X8[:q] = 0                                             # all-zero rows
    X8[q:2 * q] = 255                                      # all-255 rows
    X8[2 * q:3 * q] = X8[2 * q]                            # identical rows
    base = np.clip(X8[3 * q], 0, 254)
    X8[3 * q:] = base                                      # rows that differ from one another in ONE component by 1
    for i in range(3 * q, n):
        X8[i, (i - 3 * q) % d] += (i - 3 * q) // d % 2
    return X8, K, B0


@pytest.mark.parametrize("opt", ["default", "s6_forced", "filter", "s4"])
def test_data_edges(lsq, oracle, opt):
    X8, K, B0 = edge_data()
    assert X8[:250].max() == 0 and X8[250:500].min() == 255 and np.abs(X8[750:].astype(int) - X8[750].astype(int)).max() == 1
    check_triple(lsq, oracle, ("edges",), X8, K, B0, 4, OPTIONS[opt])


# ---- several snapshots; option "async" with device-resident sums and counters ------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["default", "s6_forced"])
def test_several_snapshots_and_async(lsq, oracle, opt):
    X8, K, B0 = make_u8(128, 1000, 8, seed=21)
    check_triple(lsq, oracle, ("snaps",), X8, K, B0, 8, OPTIONS[opt], ils=[1, 3, 4], nonblocking=True)


def test_async_above_q16_min(lsq, oracle, big):
    """the road words (verdict, probe) decided on the device, on 8-bit rows"""
    X8, K, B0 = big
    check_triple(lsq, oracle, ("big",), X8, K, B0, 8, {}, nonblocking=True)


# ---- the multi-device call: a repeated ordinal equals the one-context call ----------------------------------------------------------------------------------
def test_multi_device_call_with_a_repeated_ordinal(lsq, oracle):
    X8, K, B0 = make_u8(32, 1001, 4, seed=31)
    with lsq.Engine(0) as e:
        Bs1, objs1 = e.encode_icm(X8, B0, K, 4, ILS, J, NPERT, True, seed=SEED)
    mg = lsq.MultiEngine([0, 0])
    try:
        Bs2, objs2 = mg.encode_icm(X8, B0, K, 4, ILS, J, NPERT, True, seed=SEED)
        Bf, objf = mg.encode_icm(X8.astype(np.float32), B0, K, 4, ILS, J, NPERT, True, seed=SEED)
    finally:
        mg.close()
    assert np.array_equal(Bs2, Bs1) and np.array_equal(Bf, Bs1)
    assert np.array_equal(objs2.view(np.uint32), objf.view(np.uint32)), (objs2, objf)      # same shards, same sums: the same bits
    assert np.allclose(objs2, objs1, rtol=1e-6, atol=0), (objs2, objs1)                  # (two shard sums added on the host vs one sum)
    (_, (ref, robj, _)), = oracle_ref(oracle, ("multi",), X8, K, B0, 4)
    assert np.array_equal(Bs2, ref) and np.allclose(objs2, robj, rtol=1e-5, atol=0)


# ---- mixing on one context: 8-bit, f32 of OTHER data of the same shape, 8-bit again ----------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["default", "s6_forced"])
def test_mixing_8bit_and_f32_calls_on_one_context(lsq, oracle, opt):
    d, n, m = 32, 1000, 8
    X8, K, B0 = make_u8(d, n, m, seed=d)
    Xo = np.random.default_rng(99).standard_normal((n, d)).astype(np.float32) * 40 + 100      # other data, same shape, same codebooks (the table cache is hit)
    fresh = []
    for X in (X8, Xo):
        with open_engine(lsq, OPTIONS[opt]) as e:
            fresh.append(run_both(e, X, K, B0, m))
    with open_engine(lsq, OPTIONS[opt]) as e:
        seq = [run_both(e, X, K, B0, m) for X in (X8, Xo, X8)]
    for step, (got, want) in enumerate(zip(seq, (fresh[0], fresh[1], fresh[0]))):
        for q in range(5):
            assert np.array_equal(got[q], want[q]), "step %d, output %d differs from its fresh-context result" % (step, q)
    for (r0, r1), (ref, robj, rstats) in oracle_ref(oracle, ("d", d, n), X8, K, B0, m):
        assert np.array_equal(seq[2][0], ref)


# ---- errors follow the existing conventions ------------------------------------------------------------------------------------------------------------------
def test_errors(lsq, engine):
    L, EINVAL = engine._L, lsq._lib.LSQ_EINVAL
    X8, K, B0 = make_u8(8, 4, 2, seed=1)
    ils = np.array([1], dtype=np.int64)
    Bs, objs = np.zeros((1, 4, 2), np.int16), np.zeros(1, np.float32)
    ok = (X8.ctypes.data, B0.ctypes.data, K.ctypes.data, 8, 4, 2, H, ils.ctypes.data, 1, 1, 1, 1, 1, 0, 0, 0, Bs.ctypes.data, objs.ctypes.data)
    for i in (0, 1, 2, 16, 17):                            # each pointer null in turn
        args = list(ok)
        args[i] = None
        assert L.lsq_encode_icm_u8(engine._h, *args) == EINVAL and b"null pointer" in L.lsq_last_error()
    args = list(ok)
    args[6] = 128                                          # the h = 256 rule
    assert L.lsq_encode_icm_u8(engine._h, *args) == EINVAL
    args = list(ok)
    args[5] = 17
    assert L.lsq_encode_icm_u8(engine._h, *args) == EINVAL
    assert L.lsq_encode_icm_u8_dev(engine._h, None, None, None, 8, 4, 2, H, ils.ctypes.data, 1, 1, 1, 1, 0, 0, None, None, None) == EINVAL
    assert L.lsq_encode_icm_u8_dev(engine._h, None, None, None, 8, 4, 2, 128, ils.ctypes.data, 1, 1, 1, 1, 0, 0, None, None, None) == EINVAL
    with pytest.raises(TypeError, match="int8"):
        engine.encode_icm(X8.view(np.int8), B0, K, 2, [1], 1, 1, True)
    import torch
    with pytest.raises(TypeError, match="int8"):
        engine.encode_icm_dev(dev(X8).view(torch.int8), dev((B0 - 1).astype(np.uint8)), dev(K), 2, [1], 1, 1, True)
    # and the engine is still good for a call
    assert np.array_equal(engine.encode_icm(X8, B0, K, 2, [1], 1, 1, True)[0], engine.encode_icm(X8.astype(np.float32), B0, K, 2, [1], 1, 1, True)[0])
