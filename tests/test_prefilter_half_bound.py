"""The window of the pre-filter's 16-bit tile (lsq_knn_prefilter_half_bound), apart from any kernel: numpy forms the bf16 pieces by the pinned
integer rule (round to nearest even on the upper 16 bits), sums the tile's product pairs in float64 and in f32 in either order, and holds
a = (Nx + Nq) - 2 SUM_pairs to kappa^h (Nx + Nq) + eta^h of the contract's direct chain (tests/knn_check.py) on the widened rows; and the split's two
exactness claims."""
import numpy as np
import pytest

import knn_check as KC

EPS_HW = 2.0 ** -19


def _bf16(x):
    """x float32 -> the float32 value of its bf16 rounding (nearest even; finite input)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def _narrow(x, fmt):
    return x.astype(np.float16).astype(np.float32) if fmt == "f16" else _bf16(x)


def _seq(terms, dtype):
    acc = np.zeros(terms.shape[:-1], dtype=dtype)
    for s in range(terms.shape[-1]):
        acc = acc + terms[..., s].astype(dtype)
    return acc


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
@pytest.mark.parametrize("d", [1, 128, 960, 16_384])
def test_constants(lsq, d, fmt):
    kappa, eta = lsq.knn_prefilter_half_bound(d, fmt)
    want = ((4 * d + 32) * 2.0 ** -24 + 2.0 ** (-15 if fmt == "f16" else -16) + (3 * ((d + 15) // 16) + 3) * EPS_HW) * 1.01
    up = np.float32(want) if float(np.float32(want)) >= want else np.nextafter(np.float32(want), np.float32(np.inf))
    assert kappa.dtype == np.float32 and kappa == up and float(kappa) >= want
    assert float(eta) == (8 * d + 64) * 2.0 ** -120
    assert float(kappa) > float(lsq.knn_prefilter_bound(d)[0])
    for bad_d, bad_fmt in ((0, fmt), (16_385, fmt), (d, 0), (d, 1)):
        with pytest.raises(lsq._lib.LsqError):
            lsq.knn_prefilter_half_bound(bad_d, bad_fmt)


def test_every_f16_value_splits_exactly():
    x = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)
    x = x[np.isfinite(x)]
    hi = _bf16(x)
    lo = x - hi
    assert (hi.astype(np.float64) + lo.astype(np.float64) == x.astype(np.float64)).all()
    assert (_bf16(lo) == lo).all() and (lo.view(np.uint32) & 0xFFFF == 0).all()              # x_lo is a bf16 value: its upper 16 bits are all of it
    assert (np.abs(lo) <= 2.0 ** -8 * np.abs(x)).all()


@pytest.mark.parametrize("data", ["gauss", "offset", "tiny", "wide"])
@pytest.mark.parametrize("d", [3, 128, 960])
@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_product_pairs_stay_inside_the_window(lsq, fmt, d, data):
    rng = np.random.default_rng(d)
    Xb, Xq = rng.standard_normal((200, d)).astype(np.float32), rng.standard_normal((16, d)).astype(np.float32)
    if data == "offset":
        Xb, Xq = Xb + np.float32(1000), Xq + np.float32(1000)
    if data == "tiny":                                        # f16 rows hold nothing that small: 1e-3 there
        s = np.float32(1e-3 if fmt == "f16" else 1e-20)
        Xb, Xq = Xb * s, Xq * np.float32(1e-20)
    if data == "wide":                                        # 2^-40 .. 2^20 (f16 rows: what the format holds, 2^-20 .. 2^10)
        lo, hi = (-20, 10) if fmt == "f16" else (-40, 20)
        Xb, Xq = np.ldexp(Xb, rng.integers(lo, hi, Xb.shape)).astype(np.float32), np.ldexp(Xq, rng.integers(-40, 20, Xq.shape)).astype(np.float32)
    Xb = _narrow(Xb, fmt)                                     # the rows as stored, widened
    q1 = _bf16(Xq)
    q2 = _bf16(Xq - q1)
    miss = np.abs(Xq.astype(np.float64) - q1 - q2.astype(np.float64))
    assert (miss <= 2.0 ** -17 * np.abs(Xq) + 2.0 ** -134).all()      # the representation term's share of a query
    if fmt == "bf16":
        pairs = [(Xb, q1), (Xb, q2)]
    else:
        xh = _bf16(Xb)
        pairs = [(xh, q1), (xh, q2), (Xb - xh, q1)]
    kappa, eta = lsq.knn_prefilter_half_bound(d, fmt)
    chain = KC.knn_dists(Xb, Xq).astype(np.float64)
    for order in (slice(None), slice(None, None, -1)):
        nsum = (_seq((Xb * Xb)[:, order], np.float32)[None, :] + _seq((Xq * Xq)[:, order], np.float32)[:, None]).astype(np.float32)
        window = float(kappa) * nsum.astype(np.float64) + float(eta)
        for dtype in (np.float64, np.float32):
            terms = np.concatenate([(b[:, None, :] * a[None, :, :])[..., order] for a, b in pairs], axis=-1)      # products of bf16 values: exact in f32
            dot = _seq(terms, dtype)
            a_val = nsum.astype(np.float64) - 2.0 * dot.astype(np.float64) if dtype is np.float64 else (nsum - np.float32(2) * dot).astype(np.float64)
            assert (np.abs(a_val - chain) <= window).all()
