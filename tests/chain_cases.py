"""Shared by tests/test_chain_update.py (host solver) and tests/test_gpu_chain_update.py (device solver): the problems of the structured
(ChainQ) codebook update, the C-ABI calls in row-major shapes, and the float64 criteria.

Shapes here are row-major: X (n, d) f32, codes (n, m) 0-based, K (m h, d), dim2C (d, m) 0 / 1 (the reference's map, codebook_update.jl:134-136).
The criteria are those of tests/test_f64ref.py::check_lsqr, applied per dimension over the codebooks that cover it (as
tests/test_gpu_f64.py::test_train_chainq_codebooks_are_the_block_least_squares does for the scipy path):
  residual        ||x_t - S k||        <= (1 + 1e-4) x the float64 optimum's
  reconstruction  ||S k - S k_opt||    <= 2e-4 ||S k_opt||                       (not for a skewed code histogram, see check_lsqr)
  stopping rule   ||S'r|| / (||S||_F ||r||) <= sqrt(eps_f32), LSQR's own rule at the reference's tolerance, evaluated in float64
The optimum is f64ref.lsq_codebooks(method="normal"): the normal equations of the 2 h = 512 covered columns, solved by least squares."""
import importlib

import numpy as np

import f64ref as R

H = 256
SQRT_EPS = float(np.sqrt(np.finfo(np.float32).eps))
# (d, n, m) of the chain-consistent problems
SHAPES = [(12, 3000, 4), (7, 999, 2), (33, 5000, 3), (128, 20_000, 8), (64, 50_000, 16), (15, 600, 16)]


def ini():
    return importlib.import_module("local-search-quantization_amd.initializers")


def chain_dims(d, m):
    return ini().get_cbdims_chain(d, m)


def cover_of(od, d, m):
    dim2C = np.zeros((d, m), dtype=np.uint8)
    for i in range(m):
        dim2C[od[i], i] = 1
    return dim2C


def chain_problem(d, n, m, noise=0.05):
    """Chain-consistent data: random codes, true codebooks that are non-zero only inside the chain's dimensions, X = S Ktrue + noise N(0, 1)."""
    rng = np.random.default_rng(d + n + m)
    codes = rng.integers(0, H, size=(n, m))
    od = chain_dims(d, m)
    Ktrue = np.zeros((m * H, d), dtype=np.float32)
    for i in range(m):
        Ktrue[i * H:(i + 1) * H, od[i]] = rng.standard_normal((H, od[i].stop - od[i].start)).astype(np.float32)
    X = (sum(Ktrue[j * H + codes[:, j]] for j in range(m)) + noise * rng.standard_normal((n, d))).astype(np.float32)
    return X, codes, od


def dims_to_check(d, od):
    """every dimension for d <= 33, else 0, the first and last dimension of codebook 2's range, d / 2 and d - 1"""
    return list(range(d)) if d <= 33 else sorted({0, od[1].start, od[1].stop - 1, d // 2, d - 1})


def covering(od, t):
    return [i for i in range(len(od)) if od[i].start <= t < od[i].stop]


def chain_figures(K, X, codes, od, dims):
    """Per checked dimension (residual / optimum's - 1, reconstruction distance / ||optimum's||, stopping rule) in float64."""
    out = []
    for t in dims:
        cbs = covering(od, t)
        Kb = np.concatenate([K[i * H:(i + 1) * H] for i in cbs], axis=0)
        sub = codes[:, cbs]
        crit = float(R.lsqr_stopping_rule(X, sub, len(cbs), Kb, [t])[0])
        _, rec_ref = R.lsq_codebooks(X, sub, len(cbs), cols=[t], method="normal")
        rec = R.reconstruct(Kb[:, [t]], sub, len(cbs))
        xt = X[:, [t]].astype(np.float64)
        r, r0 = np.linalg.norm(xt - rec), np.linalg.norm(xt - rec_ref)
        out.append((t, r / r0 - 1.0, np.linalg.norm(rec - rec_ref) / np.linalg.norm(rec_ref), crit))
    return out


def check_chain_lsqr(K, X, codes, od, dims, skewed=False, what=""):
    figs = chain_figures(K, X, codes, od, dims)
    print("%s worst of %d dimensions: residual excess %.3e  reconstruction %.3e  stopping rule %.3e (limit %.3e)"
          % (what, len(figs), max(f[1] for f in figs), max(f[2] for f in figs), max(f[3] for f in figs), SQRT_EPS))
    for t, res, rec, crit in figs:
        assert res <= 1e-4, (what, t, "residual", res)
        if not skewed:
            assert rec <= 2e-4, (what, t, "reconstruction", rec)
        assert crit <= SQRT_EPS, (what, t, "stopping rule", crit)
    return figs


# ---- the C-ABI host calls in row-major shapes ----------------------------------------------------------------------------------------------
def struct_host(lsq, X, codes, dim2C, nthreads=8, prefill=None, B16=None):
    """lsq_update_codebooks_struct -> K (m h, d).  dim2C (d, m) or None (NULL).  Raises LsqError on a non-zero return."""
    L = lsq._lib.load()
    X = np.ascontiguousarray(X, dtype=np.float32)
    n, d = X.shape
    B = np.ascontiguousarray(codes + 1, dtype=np.int16) if B16 is None else np.ascontiguousarray(B16, dtype=np.int16)
    m = B.shape[1]
    K = np.full((m * H, d), np.float32(0 if prefill is None else prefill), dtype=np.float32)
    cover = None if dim2C is None else np.ascontiguousarray(np.asarray(dim2C).T.astype(np.uint8))
    assert cover is None or cover.shape == (m, d)
    lsq._lib.check(L.lsq_update_codebooks_struct(X.ctypes.data, B.ctypes.data, None if cover is None else cover.ctypes.data, d, n, m, H, nthreads, K.ctypes.data))
    return K


def unstruct_host(lsq, X, codes, nthreads=8):
    """lsq_update_codebooks -> K (m h, d)"""
    L = lsq._lib.load()
    X = np.ascontiguousarray(X, dtype=np.float32)
    n, d = X.shape
    B = np.ascontiguousarray(codes + 1, dtype=np.int16)
    m = B.shape[1]
    K = np.zeros((m * H, d), dtype=np.float32)
    lsq._lib.check(L.lsq_update_codebooks(X.ctypes.data, B.ctypes.data, d, n, m, H, nthreads, K.ctypes.data))
    return K


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def zero_outside(K, od, d):
    for i in range(len(od)):
        outside = np.ones(d, dtype=bool)
        outside[od[i]] = False
        if not np.all(K[i * H:(i + 1) * H][:, outside] == 0):
            return False
    return True
