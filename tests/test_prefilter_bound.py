"""The window of exact k-NN's MFMA pre-filter (lsq_knn_prefilter_bound), as a formula and apart from any kernel: the stated constants, and
|a - dist| <= kappa_d (Nx + Nq) + eta_d between a float32 expanded form a = (Nx + Nq) - 2 <x, q> -- sequential f32 sums, in either order -- and the
direct chain of the contract (tests/knn_check.py)."""
import numpy as np
import pytest

import knn_check as KC


@pytest.mark.parametrize("d", [1, 128, 960, 16_384])
def test_constants(lsq, d):
    kappa, eta = lsq.knn_prefilter_bound(d)
    want = (4 * d + 32) * 2.0 ** -24 * 1.01
    up = np.float32(want) if float(np.float32(want)) >= want else np.nextafter(np.float32(want), np.float32(np.inf))      # rounded UP to float
    assert kappa.dtype == np.float32 and kappa == up and float(kappa) >= want
    assert eta == np.float32((4 * d + 32) * 2.0 ** -120) and float(eta) == (4 * d + 32) * 2.0 ** -120
    for bad in (0, 16_385):
        with pytest.raises(lsq._lib.LsqError):
            lsq.knn_prefilter_bound(bad)


def _seq(terms):
    """f32 sum of terms[..., s] over s ascending from +0, every add rounded"""
    acc = np.zeros(terms.shape[:-1], dtype=np.float32)
    for s in range(terms.shape[-1]):
        acc = acc + terms[..., s]
    return acc


@pytest.mark.parametrize("data", ["gauss", "offset", "tiny"])
@pytest.mark.parametrize("d", [3, 128, 960])
def test_expanded_form_stays_inside_the_window(lsq, d, data):
    rng = np.random.default_rng(d)
    Xb, Xq = rng.standard_normal((300, d)).astype(np.float32), rng.standard_normal((20, d)).astype(np.float32)
    if data == "offset":
        Xb, Xq = Xb + np.float32(1000), Xq + np.float32(1000)
    if data == "tiny":
        Xb, Xq = Xb * np.float32(1e-20), Xq * np.float32(1e-20)
    kappa, eta = lsq.knn_prefilter_bound(d)
    chain = KC.knn_dists(Xb, Xq).astype(np.float64)
    for order in (slice(None), slice(None, None, -1)):
        xb, xq = Xb[:, order], Xq[:, order]
        nsum = (_seq(xb * xb)[None, :] + _seq(xq * xq)[:, None]).astype(np.float32)
        a = nsum - np.float32(2) * _seq(xq[:, None, :] * xb[None, :, :])
        window = float(kappa) * nsum.astype(np.float64) + float(eta)
        assert (np.abs(a.astype(np.float64) - chain) <= window).all()
