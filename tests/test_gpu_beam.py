"""The beam-search encoder on the device (csrc/lsq_beam.hip behind lsq_encoder_*) against its numpy checker (tests/beam_check.py): codes AND score bits,
host form and device form, at the smallest shapes at which its pieces can go wrong -- L = 1 (the greedy kernel), odd L, L at its cap, m = 1, 2 and 16,
n = 1 and n ragged against the greedy kernel's four vectors per block, duplicated codewords and small-integer data (exact ties at the selection
boundary, within and across parents), and the routes a shape threshold selects: codebooks 8 .. 15 of the greedy kernel in both visiting orders, a wave's
second vector (n above the grids' 4096 blocks in one launch), widths strictly inside an instantiation's range (2, 9 .. 15, 17 .. 31), every candidate
tying, the score against a float64 reconstruction error within a derived bound -- and the handle's contract: order, chunks, 8-bit rows, independence from the context and from other encoders,
its codes as the start of an ILS encode, rejections, lifetime."""
import functools

import numpy as np
import pytest

from beam_check import beam_exact, cost_and_score_bound

pytestmark = pytest.mark.gpu
H = 256

CASES = [(16, 100, 2, 1, "gauss"), (32, 257, 4, 3, "gauss"), (128, 300, 8, 16, "gauss"), (64, 65, 7, 32, "gauss"), (128, 33, 16, 32, "gauss"),
         (24, 40, 12, 5, "gauss"), (32, 130, 5, 4, "dup"), (48, 31, 9, 7, "dup"), (20, 64, 3, 5, "int"), (20, 64, 6, 8, "int"), (24, 77, 1, 1, "gauss"),
         (128, 1, 8, 16, "gauss")]


@functools.lru_cache(maxsize=None)
def _case(d, n, m, kind):
    """X (n, d), K (m h, d), generated as tests/test_gpu_initializers.py does"""
    rng = np.random.default_rng(100 + d + n + m)
    X = rng.standard_normal((d, n)).astype(np.float32)
    if kind == "int":                                                          # small integers: every sum exact, many exact ties
        X = rng.integers(-3, 4, size=(d, n)).astype(np.float32)
        C = [rng.integers(-2, 3, size=(d, H)).astype(np.float32) for _ in range(m)]
    else:
        C = [rng.standard_normal((d, H)).astype(np.float32) for _ in range(m)]
        if kind == "dup":                                                      # every other codeword duplicated
            for c in C:
                c[:, 1::2] = c[:, 0::2]
    return np.ascontiguousarray(X.T), np.ascontiguousarray(np.concatenate([c.T for c in C], axis=0))


@functools.lru_cache(maxsize=None)
def _want(d, n, m, L, kind, order=None):
    X, K = _case(d, n, m, kind)
    return beam_exact(X, K, m, L, order)


def _same(codes0, score, want):
    wc, ws = want
    assert np.array_equal(codes0, wc), "%d of %d vectors differ" % (int((codes0 != wc).any(axis=1).sum()), wc.shape[0])
    assert score.dtype == np.float32 and score.tobytes() == ws.tobytes(), "%d scores differ in their bits" % int((score.view(np.uint32) != ws.view(np.uint32)).sum())


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host_beam(enc, X, L, order=None):
    B, s = enc.beam(X, L, order=order, want_score=True)
    assert B.dtype == np.int16 and B.shape == (X.shape[0], enc.m)
    return B.astype(np.int64) - 1, s


def _dev_beam(enc, X, L, order=None):
    import torch
    dB, ds = enc.beam(_dev(X), L, order=order, want_score=True)
    torch.cuda.synchronize()
    assert dB.dtype == torch.uint8 and tuple(dB.shape) == (X.shape[0], enc.m)
    return dB.cpu().numpy().astype(np.int64), ds.cpu().numpy()


@pytest.mark.parametrize("d,n,m,L,kind", CASES)
def test_codes_and_score_bits_vs_checker(engine, d, n, m, L, kind):
    X, K = _case(d, n, m, kind)
    want = _want(d, n, m, L, kind)
    with engine.encoder(K, m) as enc:
        _same(*_host_beam(enc, X, L), want)
        assert enc.info()["vectors"] == n and enc.info()["beam"] == L and enc.info()["chunks"] == 1
        assert np.array_equal(enc.beam(X, L).astype(np.int64) - 1, want[0])          # without the score
    with engine.encoder_dev(_dev(K), m) as enc:
        _same(*_dev_beam(enc, X, L), want)


def _both_forms(engine, d, n, m, L, kind, order=None):
    """codes and score bits of the host form and of the device form against the checker -> the host form's info()"""
    X, K = _case(d, n, m, kind)
    want = _want(d, n, m, L, kind, order)
    with engine.encoder(K, m) as enc:
        _same(*_host_beam(enc, X, L, order=None if order is None else list(order)), want)
        info = enc.info()
    with engine.encoder_dev(_dev(K), m) as enc:
        _same(*_dev_beam(enc, X, L, order=None if order is None else np.array(order, dtype=np.int64)), want)
    assert info["vectors"] == n and info["beam"] == L
    return info


def _high_first(m):
    """a visiting order that starts with the highest codebook and alternates high and low ones: m = 11 -> 10 0 9 1 8 2 7 3 6 4 5"""
    lo, hi = list(range(m // 2)), list(range(m - 1, m // 2 - 1, -1))
    return tuple(x for pair in zip(hi, lo + [None]) for x in pair if x is not None)


@pytest.mark.parametrize("order", ["ascending", "high-first"])
@pytest.mark.parametrize("d,n,m,kind", [(16, 130, 16, "gauss"), (16, 131, 9, "gauss"), (16, 67, 13, "gauss"), (20, 64, 11, "int")])
def test_greedy_codebooks_8_to_15(engine, d, n, m, kind, order):
    """L = 1 with m > 8: the greedy kernel keeps the codes of codebooks 8 .. 15 in a second word.  Ascending fills the first word before the second; the
    other order writes and reads the second word first and switches words at every stage.  Small integers: exact ties inside the wave's first minimum"""
    o = None if order == "ascending" else _high_first(m)
    assert m > 8 and (o is None or (sorted(o) == list(range(m)) and o[0] >= 8 and o[1] < 8))
    _both_forms(engine, d, n, m, 1, kind, o)


@pytest.mark.parametrize("n,m", [(1, 3), (2, 3), (3, 3), (5, 3), (1, 16)])
def test_greedy_ragged_last_block(engine, n, m):
    """L = 1 serves four vectors per block: a last block with one, two and three of them, a whole block and one more"""
    assert n % 4 != 0
    _both_forms(engine, 16, n, m, 1, "gauss")


@pytest.mark.parametrize("d,n,m,L,kind", [(8, 16500, 2, 1, "gauss"), (8, 4200, 3, 2, "gauss"), (8, 4200, 3, 5, "gauss"), (8, 4200, 3, 5, "int")])
def test_a_wave_encodes_a_second_vector(engine, d, n, m, L, kind):
    """the grids stop at 4096 blocks -- four vectors a block at L = 1, one otherwise -- so in ONE launch of more vectors than that some wave goes round its
    vector loop again: the stride, the beam state and the candidate keys left in LDS by the vector before (small integers: ties that stale keys would win)"""
    assert n > 4096 * (4 if L == 1 else 1)
    assert _both_forms(engine, d, n, m, L, kind)["chunks"] == 1               # the whole n was one launch


@pytest.mark.parametrize("d,n,m,L,kind", [(16, 70, 4, 2, "gauss"), (16, 70, 4, 2, "dup"), (16, 70, 6, 9, "gauss"), (16, 70, 6, 12, "dup"), (16, 70, 6, 15, "gauss"),
                                          (16, 70, 5, 17, "gauss"), (16, 70, 5, 24, "dup"), (16, 70, 5, 31, "gauss"), (16, 70, 13, 17, "dup"),
                                          (16, 70, 13, 24, "gauss"), (16, 70, 13, 31, "gauss")])
def test_widths_below_their_instantiation(engine, d, n, m, L, kind):
    """beam_kernel<LMAX> serves every L <= LMAX in {2, 4, 8, 16, 32}, its register slots past L clamped to the last parent: L = 2 (LMAX = 2 itself), L strictly
    inside (8, 16) and (16, 32).  In the last range 4 L lies strictly between 64 and 128: some lanes read a second slot of the re-scanned column, some do not"""
    assert L == 2 or 8 < L < 16 or (16 < L < 32 and 64 < 4 * L < 128)
    assert m > 2                                                             # a stage with L parents and a stage after it
    _both_forms(engine, d, n, m, L, kind)


@pytest.mark.parametrize("L", [4, 32])
def test_every_candidate_ties(engine, L):
    """one codeword 256 m times and rows of zeros: all 256 L_t candidates of every stage share a key, position alone decides, and the answer is code 0
    everywhere (the checker says so too) with the score of four equal codewords"""
    d, n, m = 16, 9, 4
    c = np.random.default_rng(7).integers(-2, 3, size=d).astype(np.float32)
    X, K = np.zeros((n, d), np.float32), np.ascontiguousarray(np.tile(c, (m * H, 1)))
    want = beam_exact(X, K, m, L)
    assert not want[0].any() and np.all(want[1] == np.float32(m * m * (c * c).sum()))
    with engine.encoder(K, m) as enc:
        _same(*_host_beam(enc, X, L), want)
    with engine.encoder_dev(_dev(K), m) as enc:
        _same(*_dev_beam(enc, X, L), want)


def test_score_plus_norm_is_the_float64_reconstruction_error(engine):
    """||x||^2 + score against the reconstruction error of the returned codes in float64 numpy -- no device cost kernel on either side -- within the bound
    beam_check.cost_and_score_bound derives from the contract's operation count (c = d + 2 + m + m (m - 1) / 2 = 166 rounded operations on any leaf:
    gamma_c 2^-24 times the leaves' magnitudes).  On the MI355X the largest ratio to the bound was 0.00595 at L = 1 and 0.00547 at L = 16 (the bound itself: 4.5e-5 of the cost)"""
    d, n, m = 128, 300, 8
    X, K = _case(d, n, m, "gauss")
    K = np.ascontiguousarray(K / np.float32(m))
    with engine.encoder(K, m) as enc:
        for L in (1, 16):
            codes, s = _host_beam(enc, X, L)
            cost, bound = cost_and_score_bound(X, K, m, codes)
            err = np.abs((X.astype(np.float64) ** 2).sum(1) + s.astype(np.float64) - cost)
            print("L=%d: max |error| / bound %.3g (max bound / cost %.3g)" % (L, (err / bound).max(), (bound / cost).max()))
            assert np.all(err <= bound)


def test_visiting_order(lsq, engine):
    d, n, m, L = 32, 257, 4, 3
    X, K = _case(d, n, m, "gauss")
    with engine.encoder(K, m) as enc, engine.encoder_dev(_dev(K), m) as denc:
        for order in ((2, 0, 3, 1), (3, 2, 1, 0)):
            want = _want(d, n, m, L, "gauss", order)
            _same(*_host_beam(enc, X, L, order=list(order)), want)
            _same(*_dev_beam(denc, X, L, order=np.array(order, dtype=np.int64)), want)
        _same(*_host_beam(enc, X, L, order=range(m)), _want(d, n, m, L, "gauss"))      # None is range(m)
        for bad in ((0, 1, 2, 2), (0, 1, 2, 4), (-1, 0, 1, 2)):
            for e in (enc, denc):
                with pytest.raises(lsq._lib.LsqError) as err:
                    e.beam(X if e is enc else _dev(X), L, order=list(bad))
                assert err.value.code == lsq._lib.LSQ_EINVAL
        _same(*_host_beam(enc, X, L), _want(d, n, m, L, "gauss"))                       # and the encoder is as it was


def test_chunks_do_not_matter(engine):
    d, n, m, L = 24, 333, 3, 6
    X, K = _case(d, n, m, "gauss")
    want = _want(d, n, m, L, "gauss")
    with engine.encoder(K, m, chunk=100) as enc:
        _same(*_host_beam(enc, X, L), want)
        assert enc.info()["chunks"] == 4
        _same(*_host_beam(enc, X, 1), _want(d, n, m, 1, "gauss"))
    with engine.encoder_dev(_dev(K), m, chunk=100) as enc:
        _same(*_dev_beam(enc, X, L), want)
    with engine.encoder(K, m) as enc:
        _same(*_host_beam(enc, X, L), want)


def test_uint8_rows_give_the_bits_of_the_f32_call(engine, oracle):
    d, n, m, L = 32, 150, 4, 8
    Xf = oracle.synth_data_u8(77, n, d)                                        # SIFT-like: integer-valued float32
    X8 = Xf.astype(np.uint8)
    assert np.array_equal(X8.astype(np.float32), Xf)
    K = np.ascontiguousarray(oracle.synth_data_u8(78, m * H, d) / np.float32(m))
    want = beam_exact(Xf, K, m, L)
    with engine.encoder(K, m, chunk=64) as enc:
        _same(*_host_beam(enc, X8, L), want)
        _same(*_host_beam(enc, Xf, L), want)
    with engine.encoder_dev(_dev(K), m) as enc:
        _same(*_dev_beam(enc, X8, L), want)
        _same(*_dev_beam(enc, X8, 1), beam_exact(Xf, K, m, 1))


def test_one_codebook_is_assign_codewords(engine):
    X, K = _case(24, 77, 1, "gauss")
    B, mv = engine.assign_codewords(X, K, 1, want_min=True)
    with engine.encoder(K, 1) as enc:
        for L in (1, 5):
            Bb, s = enc.beam(X, L, want_score=True)
            assert np.array_equal(Bb, B) and s.tobytes() == mv[:, 0].tobytes()


def test_score_plus_norm_is_veccost(engine):
    d, n, m = 128, 300, 8
    X, K = _case(d, n, m, "gauss")
    K = np.ascontiguousarray(K / np.float32(m))
    with engine.encoder(K, m) as enc:
        for L in (1, 16):
            B, s = enc.beam(X, L, want_score=True)
            cost = engine.veccost(X, B, K, m).astype(np.float64)
            rel = np.abs((X.astype(np.float64) ** 2).sum(1) + s - cost) / cost
            print("L=%d: max relative difference %.3g" % (L, rel.max()))
            assert rel.max() <= 1e-5


def test_encoders_and_context_do_not_disturb_each_other(engine, oracle):
    from conftest import make_problem
    Xc, Kc, B0 = make_problem(32, 400, 4, seed=3)
    args = (4, [1, 2], 2, 2, True)
    Bs0, objs0 = engine.encode_icm(Xc, B0, Kc, *args, seed=9)
    Bk0 = engine.encoding_icm(Xc, B0, Kc, 4, 2, True, 2, seed=9, it=0)         # the host-table cache is warm from here on
    (X1, K1), (X2, K2) = _case(64, 65, 7, "gauss"), _case(20, 64, 3, "int")
    w1, w2 = _want(64, 65, 7, 32, "gauss"), _want(20, 64, 3, 5, "int")
    with engine.encoder(K1, 7) as e1, engine.encoder_dev(_dev(K2), 3) as e2:
        _same(*_host_beam(e1, X1, 32), w1)
        Bk1 = engine.encoding_icm(Xc, B0, Kc, 4, 2, True, 2, seed=9, it=0)     # same codebooks: the cached tables must still be the context's own
        _same(*_dev_beam(e2, X2, 5), w2)
        Bs1, objs1 = engine.encode_icm(Xc, B0, Kc, *args, seed=9)
        _same(*_host_beam(e1, X1, 32), w1)
        _same(*_dev_beam(e2, X2, 5), w2)
        Bs2, objs2 = engine.encode_icm(Xc, B0, Kc, *args, seed=9)
    assert np.array_equal(Bk0, Bk1)
    assert np.array_equal(Bs0, Bs1) and np.array_equal(Bs0, Bs2) and objs0.tobytes() == objs1.tobytes() == objs2.tobytes()


def test_device_codes_start_an_ils_encode(engine):
    """the device form's codes ARE encode_icm_dev's B0; an ILS iteration accepts a vector's new codes only when they cost strictly less, so the objective
    returned is not above the beam codes' own.  Both sums are float64 sums of the per-vector f32 costs; 1e-6 relative covers a cost rounded differently by
    the two kernels that compute it (2^-24 per operation), three orders below the 1e-3 an ILS iteration moves the objective by."""
    import torch
    d, n, m, L = 128, 300, 8, 16
    X, K = _case(d, n, m, "gauss")
    K = np.ascontiguousarray(K / np.float32(m))
    dX, dK = _dev(X), _dev(K)
    with engine.encoder_dev(dK, m) as enc:
        dB0 = enc.beam(dX, L)
        dBs, sums, _ = engine.encode_icm_dev(dX, dB0, dK, m, [2], 4, 4, True, seed=5)
        torch.cuda.synchronize()
    B0 = dB0.cpu().numpy()
    assert np.array_equal(B0.astype(np.int64), beam_exact(X, K, m, L)[0])
    own = float(engine.veccost(X, B0.astype(np.int16) + 1, K, m).astype(np.float64).sum())
    print("beam codes %.6f, after 2 ILS iterations %.6f" % (own / n, float(sums[0]) / n))
    assert float(sums[0]) <= own * (1 + 1e-6)
    after = dBs[0].cpu().numpy()
    assert after.shape == (n, m) and float(engine.veccost(X, after.astype(np.int16) + 1, K, m).astype(np.float64).sum()) <= own * (1 + 1e-6)


def test_rejections(lsq, engine):
    import ctypes as C
    EINVAL, L = lsq._lib.LSQ_EINVAL, engine._L
    rng = np.random.default_rng(1)
    X = rng.standard_normal((10, 8)).astype(np.float32)
    K = rng.standard_normal((2 * H, 8)).astype(np.float32)
    for make in (lambda: engine.encoder(rng.standard_normal((2 * 128, 8)).astype(np.float32), 2, h=128),          # h != 256
                 lambda: engine.encoder(rng.standard_normal((17 * H, 8)).astype(np.float32), 17),                  # m > 16
                 lambda: engine.encoder(K, 2, chunk=-1)):
        with pytest.raises(lsq._lib.LsqError) as err:
            make()
        assert err.value.code == EINVAL
    desc = lsq._lib.EncoderDesc()
    desc.d, desc.m, desc.h, desc.codebooks = 8, 2, H, None
    h = C.c_void_p()
    assert L.lsq_encoder_create(C.byref(h), engine._h, C.byref(desc)) == EINVAL and not h.value       # null codebooks
    desc.d, desc.codebooks = 0, K.ctypes.data
    assert L.lsq_encoder_create(C.byref(h), engine._h, C.byref(desc)) == EINVAL                       # d < 1
    assert L.lsq_encoder_create(C.byref(h), engine._h, None) == EINVAL                                # null description
    with engine.encoder(K, 2) as enc:
        for beam in (0, 33, -1):
            with pytest.raises(lsq._lib.LsqError) as err:
                enc.beam(X, beam)
            assert err.value.code == EINVAL
        out = np.zeros((10, 2), np.int16)
        assert L.lsq_encoder_beam(enc._h, None, 0, 10, 4, None, out.ctypes.data, None, 0) == EINVAL           # null X
        assert L.lsq_encoder_beam(enc._h, X.ctypes.data, 0, 10, 4, None, None, None, 0) == EINVAL             # null codes
        assert L.lsq_encoder_beam(enc._h, X.ctypes.data, 0, -1, 4, None, out.ctypes.data, None, 0) == EINVAL  # n < 0
        assert not out.any()
        assert L.lsq_encoder_beam(enc._h, None, 0, 0, 4, None, None, None, 0) == lsq._lib.LSQ_OK              # n = 0
        assert enc.beam(np.zeros((0, 8), np.float32), 4).shape == (0, 2)
        assert enc.beam(X, 4).min() >= 1                                                                      # and it still encodes


def test_a_closed_engine_closes_its_encoders(lsq):
    X, K = _case(16, 100, 2, "gauss")
    eng = lsq.Engine(0)
    enc = eng.encoder(K, 2)
    assert np.array_equal(enc.beam(X, 1).astype(np.int64) - 1, _want(16, 100, 2, 1, "gauss")[0])
    eng.close()
    assert enc._h is None
    enc.close()                                                                # a no-op now
    with lsq.Engine(0) as eng2:
        with eng2.encoder(K, 2) as enc2:
            assert np.array_equal(enc2.beam(X, 1).astype(np.int64) - 1, _want(16, 100, 2, 1, "gauss")[0])
