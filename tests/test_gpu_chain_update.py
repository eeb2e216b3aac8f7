"""The structured (ChainQ) codebook update on the device: lsq_update_codebooks_struct_gpu / _dev (csrc/lsq_lsqr.hip with a cover map) against the
host solver, against float64 directly, against the unstructured device solver where the two must coincide, and inside train_chainq /
train_chainq_dev.  Problems and criteria: tests/chain_cases.py (shared with the host tests in tests/test_chain_update.py)."""
import numpy as np
import pytest

import chain_cases as CC
import f64ref as R
from test_f64ref import _lsqr_problem

pytestmark = pytest.mark.gpu
H = CC.H


def _dev_tensors(X, codes):
    import torch
    return torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(codes.astype(np.uint8))).cuda()


def _device_pair(engine, X, codes, dim2C):
    """-> (K of the _gpu entry, its iterations, K of the _dev entry with out= pre-filled with NaN, its iterations)"""
    import torch
    m = codes.shape[1]
    Kg, itg = engine.update_codebooks_struct(X, (codes + 1).astype(np.int16), dim2C, m)
    dX, dB = _dev_tensors(X, codes)
    out = torch.full((m * H, X.shape[1]), float("nan"), dtype=torch.float32, device=dX.device)
    dK, itd = engine.update_codebooks_struct_dev(dX, dB, None if dim2C is None else torch.from_numpy(np.asarray(dim2C)).cuda(), m, out=out)
    torch.cuda.synchronize()
    assert dK.data_ptr() == out.data_ptr()
    return Kg, itg, dK.cpu().numpy(), itd


@pytest.mark.parametrize("d,n,m", CC.SHAPES + [(128, 100_000, 8), (3, 13, 2)])
def test_device_chain_update_agrees_with_the_host_solver(lsq, engine, d, n, m):
    """The agreement the project requires of the unstructured pair (reconstruction 1e-5, K 1e-4, relative), and -- as for that pair -- the same
    words: the device adds S v and S'u in the host's order and its norms in a grouping that has rounded to the host's f32 on every tested problem."""
    X, codes, od = CC.chain_problem(d, n, m)
    dim2C = CC.cover_of(od, d, m)
    Kh = CC.struct_host(lsq, X, codes, dim2C)
    Kg, itg, Kd, itd = _device_pair(engine, X, codes, dim2C)
    print("device (%d, %d, %d): %d iterations" % (d, n, m, itg))
    assert CC.same_bits(Kg, Kd) and itg == itd, "the _gpu and _dev entry points differ"
    assert 1 <= itg <= max(n, 2 * H), itg
    assert CC.zero_outside(Kd, od, d)
    rec = lambda K: sum(K[j * H + codes[:, j]].astype(np.float64) for j in range(m))
    rh, rd = rec(Kh), rec(Kd)
    assert np.linalg.norm(rd - rh) <= 1e-5 * np.linalg.norm(rh), np.linalg.norm(rd - rh) / np.linalg.norm(rh)
    assert np.linalg.norm(Kd - Kh) <= 1e-4 * np.linalg.norm(Kh), np.linalg.norm(Kd - Kh) / np.linalg.norm(Kh)
    diff = int((Kd.view(np.uint32) != Kh.view(np.uint32)).sum())
    assert diff == 0, "device and host structured LSQR differ in %d of %d words" % (diff, Kd.size)


@pytest.mark.parametrize("d,n,m", CC.SHAPES)
def test_device_chain_update_reaches_the_float64_optimum(engine, d, n, m):
    X, codes, od = CC.chain_problem(d, n, m)
    K, _ = engine.update_codebooks_struct(X, (codes + 1).astype(np.int16), CC.cover_of(od, d, m), m)
    assert CC.zero_outside(K, od, d)
    CC.check_chain_lsqr(K, X, codes, od, CC.dims_to_check(d, od), what="device (%d, %d, %d)" % (d, n, m))
    Kb = K.copy()
    Kb[H:2 * H] = 0                                                          # one codebook's update dropped
    with pytest.raises(AssertionError):
        CC.check_chain_lsqr(Kb, X, codes, od, CC.dims_to_check(d, od))


def test_device_chain_update_skewed_histogram(engine):
    d, n, m = 16, 60_000, 4
    X, codes = _lsqr_problem(np.random.default_rng(d + n + m), d, n, m, skew=True)
    od = CC.chain_dims(d, m)
    K, _ = engine.update_codebooks_struct(X, (codes + 1).astype(np.int16), CC.cover_of(od, d, m), m)
    CC.check_chain_lsqr(K, X, codes, od, list(range(d)), skewed=True, what="device skewed")


@pytest.mark.parametrize("d,n,m", [(128, 20_000, 8), (33, 120_000, 8)])
def test_full_cover_on_the_device_is_the_unstructured_solver(engine, d, n, m):
    """a null map takes the unstructured path; an all-ones map walks the lists and still returns its bits"""
    import torch
    X, codes = _lsqr_problem(np.random.default_rng(d + n), d, n, m)
    dX, dB = _dev_tensors(X, codes)
    dK0, it0 = engine.update_codebooks_dev(dX, dB, m)
    want = dK0.cpu().numpy()
    for dim2C in (None, np.ones((d, m), dtype=np.uint8)):
        Kg, itg, Kd, itd = _device_pair(engine, X, codes, dim2C)
        assert CC.same_bits(Kg, want) and CC.same_bits(Kd, want) and itg == itd == it0, (dim2C is None, itg, itd, it0)
    dK1, it1 = engine.update_codebooks_dev(dX, dB, m)                        # the unstructured path after structured calls on the same context
    torch.cuda.synchronize()
    assert CC.same_bits(dK1.cpu().numpy(), want) and it1 == it0


def test_device_zeros_outside_the_cover_and_repeatability(lsq, engine):
    import torch
    d, n, m = 128, 20_000, 8
    X, codes, od = CC.chain_problem(d, n, m)
    dim2C = CC.cover_of(od, d, m)
    _, it1, K1, _ = _device_pair(engine, X, codes, dim2C)
    _, it2, K2, _ = _device_pair(engine, X, codes, dim2C)
    assert np.isfinite(K1).all() and CC.zero_outside(K1, od, d)
    assert CC.same_bits(K1, K2) and it1 == it2
    # a general map: one dimension that nothing covers, one covered by three codebooks -- against the host solver
    dim2C[5, :] = 0
    dim2C[70, :] = 0
    dim2C[70, [0, 3, 7]] = 1
    Kh = CC.struct_host(lsq, X, codes, dim2C)
    _, _, Kd, _ = _device_pair(engine, X, codes, dim2C)
    assert np.all(Kd[:, 5] == 0) and np.isfinite(Kd).all()
    assert np.array_equal(Kd == 0, Kh == 0)
    assert np.linalg.norm(Kd - Kh) <= 1e-4 * np.linalg.norm(Kh)
    # argument rules on the device entries
    bad = dim2C.copy()
    bad[1, 1] = 2
    with pytest.raises(lsq._lib.LsqError) as e:
        engine.update_codebooks_struct(X, (codes + 1).astype(np.int16), bad, m)
    assert e.value.code == lsq._lib.LSQ_EINVAL
    dX, dB = _dev_tensors(X, codes)
    with pytest.raises(lsq._lib.LsqError) as e:
        engine.update_codebooks_struct_dev(dX, dB, torch.from_numpy(bad).cuda(), m)
    assert e.value.code == lsq._lib.LSQ_EINVAL


@pytest.mark.parametrize("n,d,m", [(3000, 16, 4), (20_000, 64, 8)])
def test_train_chainq_on_the_device_follows_the_default_trainer(lsq, engine, n, d, m):
    """device_update=True and train_chainq_dev against train_chainq's default (scipy float64) path, two iterations: the objective within the 5e-3
    a trainer trajectory with another solver's arithmetic is granted (tests/test_pipeline_gpu.py); codebooks zero outside the chain; the codes
    are the chain optimum for the returned codebooks and rotation (first 256 vectors); R orthogonal to 1e-5."""
    import torch
    rng = np.random.default_rng(n + d + m)
    X = rng.standard_normal((d, n)).astype(np.float32) * np.linspace(3, 0.3, d, dtype=np.float32)[:, None]
    _, B0, R0, _ = lsq.train_opq(X, m, H, 1, "natural", engine=engine)
    C0, B_ref, R_ref, obj_ref = lsq.train_chainq(X, m, H, R0, B0, None, 2, engine=engine)
    od = lsq.get_cbdims_chain(d, m)

    def judge(K, codes, Rot, obj, what):
        print("%s obj %s vs default %s" % (what, obj.tolist(), obj_ref.tolist()))
        assert obj.shape == obj_ref.shape
        assert np.all(np.abs(obj - obj_ref) <= 5e-3 * np.abs(obj_ref)), (what, obj, obj_ref)
        assert CC.zero_outside(K, od, d), what
        Rd = Rot.astype(np.float64)
        assert np.abs(Rd.T @ Rd - np.eye(d)).max() <= 1e-5, what
        RXr = np.ascontiguousarray((Rot.T @ X).T[:256])
        R.check_chain(RXr, K, codes[:256], m, what=what)

    C1, B1, R1, obj1 = lsq.train_chainq(X, m, H, R0, B0, None, 2, engine=engine, device_update=True)
    judge(np.ascontiguousarray(np.concatenate(C1, axis=1).T), B1.T.astype(np.int64) - 1, R1, obj1, "train_chainq(device_update=True)")
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    dB0 = torch.from_numpy(np.ascontiguousarray((B0.T - 1).astype(np.uint8))).cuda()
    dK, dB, R2, obj2 = lsq.train_chainq_dev(dX, m, H, R0, dB0, 2, engine=engine)
    torch.cuda.synchronize()
    assert dK.is_cuda and dB.is_cuda and dB.dtype == torch.uint8 and tuple(dK.shape) == (m * H, d) and tuple(dB.shape) == (n, m)
    judge(dK.cpu().numpy(), dB.cpu().numpy().astype(np.int64), R2, obj2, "train_chainq_dev")
