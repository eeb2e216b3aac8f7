"""The structured (ChainQ) codebook update on the host: lsq_update_codebooks_struct (update_codebooks_generic / update_codebooks_chain,
src/codebook_update.jl:104-158) against the float64 optimum, against the unstructured solver where the two must coincide, and its argument rules.
No GPU needed.  The device solver is held to the same criteria in tests/test_gpu_chain_update.py."""
import numpy as np
import pytest

import chain_cases as CC
from test_f64ref import _lsqr_problem

H = CC.H


@pytest.mark.parametrize("d,n,m", CC.SHAPES)
def test_host_chain_update_reaches_the_float64_optimum(lsq, d, n, m):
    """Per dimension, over the two codebooks that cover it: residual, reconstruction and LSQR's stopping rule in float64 (chain_cases).  The
    existing host LSQR run on each sub-system gave at worst 1.8e-5 / 1.1e-4 / 1.6e-4 over these shapes (limits 1e-4 / 2e-4 / 3.45e-4)."""
    X, codes, od = CC.chain_problem(d, n, m)
    K = CC.struct_host(lsq, X, codes, CC.cover_of(od, d, m), prefill=np.nan)
    assert CC.zero_outside(K, od, d)
    CC.check_chain_lsqr(K, X, codes, od, CC.dims_to_check(d, od), what="host (%d, %d, %d)" % (d, n, m))


def test_host_chain_update_skewed_histogram(lsq):
    """90 % of codebook 1's codes are one value: residual and stopping rule only, as check_lsqr(skewed=True)"""
    d, n, m = 16, 60_000, 4
    X, codes = _lsqr_problem(np.random.default_rng(d + n + m), d, n, m, skew=True)
    od = CC.chain_dims(d, m)
    K = CC.struct_host(lsq, X, codes, CC.cover_of(od, d, m))
    CC.check_chain_lsqr(K, X, codes, od, list(range(d)), skewed=True, what="host skewed")


def test_zeroing_a_codebook_fails_the_criteria(lsq):
    """the criteria are not vacuous: one codebook's update dropped and they fail"""
    d, n, m = 12, 3000, 4
    X, codes, od = CC.chain_problem(d, n, m)
    K = CC.struct_host(lsq, X, codes, CC.cover_of(od, d, m))
    CC.check_chain_lsqr(K, X, codes, od, list(range(d)))
    for i in range(m):
        Kb = K.copy()
        Kb[i * H:(i + 1) * H] = 0
        with pytest.raises(AssertionError):
            CC.check_chain_lsqr(Kb, X, codes, od, list(range(d)))


@pytest.mark.parametrize("d,n,m", [(12, 3000, 4), (33, 5000, 3)])
def test_full_cover_is_the_unstructured_solver(lsq, d, n, m):
    """dim2C = NULL and an all-ones map return lsq_update_codebooks' bits"""
    X, codes = _lsqr_problem(np.random.default_rng(d + n + m), d, n, m)
    want = CC.unstruct_host(lsq, X, codes)
    assert CC.same_bits(CC.struct_host(lsq, X, codes, None, prefill=np.nan), want)
    assert CC.same_bits(CC.struct_host(lsq, X, codes, np.ones((d, m), dtype=np.uint8), prefill=np.nan), want)


def test_chain_of_two_codebooks_is_the_unstructured_solver(lsq):
    """m = 2: both codebooks cover every dimension"""
    d, n, m = 7, 999, 2
    X, codes, od = CC.chain_problem(d, n, m)
    dim2C = CC.cover_of(od, d, m)
    assert np.all(dim2C == 1)
    assert CC.same_bits(CC.struct_host(lsq, X, codes, dim2C), CC.unstruct_host(lsq, X, codes))


@pytest.mark.parametrize("d,n,m", [(12, 3000, 4), (33, 5000, 3), (15, 600, 16)])
def test_structured_call_equals_the_unstructured_solver_on_each_group(lsq, d, n, m):
    """bit for bit: lsq_update_codebooks on X restricted to the dimensions of one cover set and B to its codebooks"""
    X, codes, od = CC.chain_problem(d, n, m)
    K = CC.struct_host(lsq, X, codes, CC.cover_of(od, d, m), prefill=np.nan)
    groups = {}
    for t in range(d):
        groups.setdefault(tuple(CC.covering(od, t)), []).append(t)
    assert len(groups) == (m - 1 if m > 2 else 1)
    want = np.zeros_like(K)
    for cbs, ts in groups.items():
        Ks = CC.unstruct_host(lsq, X[:, ts], codes[:, list(cbs)])
        for q, i in enumerate(cbs):
            want[i * H:(i + 1) * H, ts] = Ks[q * H:(q + 1) * H]
    assert CC.same_bits(K, want), "%d words differ" % (K.view(np.uint32) != want.view(np.uint32)).sum()


def test_zeros_outside_the_cover_and_uncovered_dimensions(lsq):
    d, n, m = 12, 3000, 4
    X, codes, od = CC.chain_problem(d, n, m)
    dim2C = CC.cover_of(od, d, m)
    K = CC.struct_host(lsq, X, codes, dim2C, prefill=np.nan)
    assert np.isfinite(K).all() and CC.zero_outside(K, od, d)
    assert all(np.any(K[i * H:(i + 1) * H, od[i]] != 0) for i in range(m))
    # a general (non-chain) map with a dimension that nothing covers and one covered by three codebooks
    dim2C[5, :] = 0
    dim2C[2, :] = [1, 0, 1, 1]
    K2 = CC.struct_host(lsq, X, codes, dim2C, prefill=np.nan)
    assert np.all(K2[:, 5] == 0) and np.isfinite(K2).all()
    assert np.all(K2[H:2 * H, 2] == 0) and np.any(K2[:H, 2] != 0) and np.any(K2[3 * H:, 2] != 0)
    Ks = CC.unstruct_host(lsq, X[:, [2]], codes[:, [0, 2, 3]])
    assert CC.same_bits(np.concatenate([K2[:H, 2], K2[2 * H:, 2]]), Ks[:, 0])
    untouched = [t for t in range(d) if t not in (2, 5)]
    assert CC.same_bits(K2[:, untouched], K[:, untouched])


def test_bad_arguments(lsq):
    E = lsq._lib
    d, n, m = 12, 300, 4
    X, codes, od = CC.chain_problem(d, n, m)
    dim2C = CC.cover_of(od, d, m)
    bad = dim2C.copy()
    bad[3, 1] = 2
    with pytest.raises(E.LsqError) as e:
        CC.struct_host(lsq, X, codes, bad)
    assert e.value.code == E.LSQ_EINVAL and "dim2C" in str(e.value)
    for off in (0, H + 1):
        B = (codes + 1).astype(np.int16)
        B[7, 2] = off
        with pytest.raises(E.LsqError) as e:
            CC.struct_host(lsq, X, codes, dim2C, B16=B)
        assert e.value.code == E.LSQ_ECODE
    # the chain's map needs m >= 2 and d >= m - 1
    for dd, mm in ((12, 1), (2, 4)):
        with pytest.raises(E.LsqError) as e:
            lsq.get_cbdims_chain(dd, mm)
        assert e.value.code == E.LSQ_EINVAL and "chain" in str(e.value)
        with pytest.raises(E.LsqError) as e:
            lsq.update_codebooks_chain(np.zeros((dd, 50), np.float32), np.ones((mm, 50), np.int16), H, solver="host")
        assert e.value.code == E.LSQ_EINVAL
    with pytest.raises(ValueError):
        lsq.update_codebooks_chain(X.T, (codes.T + 1).astype(np.int16), H, solver="nope")
    with pytest.raises(ValueError):
        lsq.train_chainq(X.T, m, H, np.eye(d, dtype=np.float32), (codes.T + 1).astype(np.int16), None, 1, device_update=True)


def test_update_codebooks_chain_host_solver_against_the_default_path(lsq):
    """Julia shapes; the f32 host solver and scipy's float64 LSQR both stop at sqrt(eps_f32): reconstructions agree to 1e-3 relative"""
    d, n, m = 12, 3000, 4
    X, codes, od = CC.chain_problem(d, n, m)
    Xj, Bj = np.ascontiguousarray(X.T), (codes.T + 1).astype(np.int16)
    C_ref = lsq.update_codebooks_chain(Xj, Bj, H)
    C_host = lsq.update_codebooks_chain(Xj, Bj, H, solver="host", nthreads=4)
    C_gen = lsq.update_codebooks_generic(Xj, Bj, H, lsq.get_cbdims_chain, solver="host", nthreads=2)
    assert all(c.shape == (d, H) and c.dtype == np.float32 for c in C_host)
    assert all(CC.same_bits(a, b) for a, b in zip(C_host, C_gen))
    K_host = np.concatenate([c.T for c in C_host], axis=0)
    assert CC.same_bits(K_host, CC.struct_host(lsq, X, codes, CC.cover_of(od, d, m)))
    rec = lambda C: sum(C[j][:, codes[:, j]] for j in range(m)).astype(np.float64)
    err = np.linalg.norm(rec(C_host) - rec(C_ref)) / np.linalg.norm(rec(C_ref))
    print("host solver vs scipy path, reconstruction: %.3e" % err)
    assert err <= 1e-3, err
