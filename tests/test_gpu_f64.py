"""Every device kernel of the shipped library against the float64 references of tests/f64ref.py, at the shapes and alignments where kernels go
wrong: the unary and pair tables, the encoder's costs and objective, both ADC scans, the norm quantiser, the device LSQR, the Viterbi and
assignment kernels and the trainers' host glue around them.  The other GPU tests hold the kernels to this project's f32 restatements bit for bit;
these hold them to the quantity itself, within a rigorous bound on its f32 evaluation, so a slip shared by a kernel and its restatement shows.

Unaligned cases pass contiguous views with a storage offset of one float (codes: one byte), as any caller may."""
import importlib

import numpy as np
import pytest

import f64ref as R
from conftest import ENCODE_VARIANTS, make_problem, open_engine
from test_f64ref import _chain_case, _lsqr_problem, check_lsqr

pytestmark = pytest.mark.gpu
H = 256


def dev(a, offset=0):
    """a host array as a contiguous cuda tensor; offset > 0: a view starting `offset` elements into its allocation"""
    import torch
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + offset, dtype=torch.from_numpy(a[:0].reshape(-1)).dtype, device="cuda:0")
    t = buf[offset:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and t.storage_offset() == offset
    return t


def _rows(n, extra=24, seed=0):
    """the rows the float64 reference is evaluated on: the ends, the 128-row tile edges, and a seeded sample"""
    r = {0, n - 1, n // 2} | {i for i in (126, 127, 128, 129, 255, 256, 4095, 4096) if i < n}
    r |= set(np.random.default_rng(seed).choice(n, size=min(n, extra), replace=False).tolist())
    return np.array(sorted(r))


# ---- the encoder's tables --------------------------------------------------------------------------------------------------------------------

TABLE_CASES = [(1, 1, 1), (127, 3, 2), (128, 5, 7), (129, 16, 16), (4097, 100, 2), (128, 129, 7), (1, 960, 16), (129, 1030, 1), (4097, 1030, 16),
               (127, 16, 1), (129, 3, 16)]


@pytest.mark.parametrize("n,d,m", TABLE_CASES)
def test_unaries_and_pair_tables(lsq, engine, n, d, m):
    rng = np.random.default_rng(n + d + m)
    X = rng.standard_normal((n, d)).astype(np.float32)
    K = (rng.standard_normal((m * H, d)) / m).astype(np.float32)
    U = engine.get_unaries(X, K, m)
    rows = _rows(n)
    ref, bnd = R.unaries(X[rows], K, m)
    R.check_values(U[:, rows], ref, bnd, "unaries n=%d d=%d m=%d" % (n, d, m))
    T = engine.get_binaries(K, m)
    ref, bnd = R.pair_tables(K, m)
    R.check_values(T, ref, bnd, "pair tables d=%d m=%d" % (d, m))


def test_rejected_shapes_raise(lsq, engine):
    X = np.zeros((4, 1), np.float32)
    assert engine.get_unaries(X, np.ones((H, 1), np.float32), 1).shape == (1, 4, H)          # d = 1 is a shape the engine computes
    with pytest.raises(lsq._lib.LsqError):
        engine.get_unaries(np.zeros((4, 8), np.float32), np.zeros((17 * H, 8), np.float32), 17)
    with pytest.raises(lsq._lib.LsqError):
        engine.get_binaries(np.zeros((17 * H, 8), np.float32), 17)


# ---- cost and the encoder ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [v for v in ENCODE_VARIANTS if v.id in ("default", "s6_forced")])
@pytest.mark.parametrize("d,n,m", [(128, 3000, 8), (33, 1031, 4)])
def test_encoder_objective_and_no_vector_gets_worse(lsq, variant, d, n, m):
    X, K, B0 = make_problem(d, n, m, seed=d)
    with open_engine(lsq, variant) as eng:
        Bs, objs = eng.encode_icm(X, B0, K, m, [1, 3], 4, 4, True, seed=11)
        cost = eng.veccost(X, Bs[-1], K, m)
        q = eng.qerror(X, Bs[-1], K, m)
    codes = Bs[-1].astype(np.int64) - 1
    c64, cb = R.veccost(X, K, codes, m)
    R.check_values(cost, c64, cb, "veccost")
    R.check_values(q, c64.mean(), R.mean_bound(cb, c64), "qerror")
    R.check_values(objs[-1], c64.mean(), R.mean_bound(cb, c64), "returned objective")
    c0, b0 = R.veccost(X, K, B0.astype(np.int64) - 1, m)
    worse = c64 > c0 + cb + b0
    assert not worse.any(), "%d vectors cost more than their initial codes, e.g. %r > %r" % (worse.sum(), c64[worse][:3], c0[worse][:3])
    assert c64.mean() < c0.mean()


@pytest.mark.parametrize("variant", [v for v in ENCODE_VARIANTS if v.id in ("default", "s6_forced")])
def test_encoder_on_views_with_an_offset(lsq, variant):
    """d = 32: the aligned call takes the 16-byte paths (cost4, the vec4 GEMM, sqnorms' and the 16-bit walk's vector loads), the views offset by
    one float (4-byte aligned) and by two (8-byte aligned) the narrower loads; all must return the same codes and sums"""
    import torch
    d, n, m = 32, 700, 4
    X, K, B0 = make_problem(d, n, m, seed=5)
    B0u = (B0 - 1).astype(np.uint8)
    with open_engine(lsq, variant) as eng:
        a, sa, _ = eng.encode_icm_dev(dev(X), dev(B0u), dev(K), m, [2], 4, 4, True, seed=3)
        for offset in (1, 2):
            b, sb, _ = eng.encode_icm_dev(dev(X, offset), dev(B0u), dev(K, offset), m, [2], 4, 4, True, seed=3)
            torch.cuda.synchronize()
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()) and np.array_equal(sa, sb), "offset %d" % offset
            c64, cb = R.veccost(X, K, b.cpu().numpy()[0].astype(np.int64), m)
            R.check_values(sb[0] / n, c64.mean(), R.mean_bound(cb, c64), "objective on views offset by %d" % offset)


# ---- the LSQ ADC scan ----------------------------------------------------------------------------------------------------------------------

def _lsq_scan_case(seed, n, nq, d, m):
    rng = np.random.default_rng(seed)
    K = (rng.standard_normal((m * H, d)) * 0.5).astype(np.float32)
    codes = rng.integers(0, H, size=(n, m), dtype=np.uint8)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    dbn = (R.reconstruct(K, codes, m) ** 2).sum(1).astype(np.float32)
    return codes, Q, K, dbn


@pytest.mark.parametrize("n,nq,d,m,k,offset,road", [(3000, 5, 1030, 4, 1, 0, "exhaustive"), (3000, 4, 1030, 3, 3000, 0, "exhaustive"),
                                                      (5000, 6, 32, 8, 50, 1, "exhaustive"), (4000, 3, 32, 4, 4000, 1, "exhaustive"),
                                                      (200_000, 6, 24, 8, 1, 0, "thresholded"), (200_000, 6, 32, 8, 100, 1, "thresholded")])
def test_lsq_scan(lsq, n, nq, d, m, k, offset, road):
    codes, Q, K, dbn = _lsq_scan_case(n + d + k, n, nq, d, m)
    with lsq.Engine(0) as eng:                                              # a context of its own: the stats describe this call alone
        dists, ids = eng.linscan_dev(dev(codes, offset), dev(Q, offset), dev(K, offset), dev(dbn, offset), m, k)
        st = eng.linscan_stats()
    dists, ids = dists.cpu().numpy(), ids.cpu().numpy()
    assert st["exhaustive"] == (1 if road == "exhaustive" else 0), st
    vals, bnd = R.lsq_adc(Q, K, codes, dbn, m)
    R.check_topk(ids - 1, dists, vals, bnd, "LSQ scan n=%d d=%d k=%d offset=%d" % (n, d, k, offset))


# ---- the PQ / OPQ scan -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,nq,m,subdim,k,dc,offset", [(3000, 5, 1, 1030, 20, 1, 0), (3000, 4, 1, 1031, 20, 1, 0), (3000, 4, 1, 1032, 20, 1, 0), (4000, 6, 5, 7, 30, 5, 0),
                                                        (2500, 3, 4, 8, 2500, 4, 0), (3000, 5, 4, 8, 40, 4, 1), (3000, 5, 3, 12, 40, 7, 1),
                                                        (200_000, 4, 8, 4, 50, 11, 1)])
def test_pq_scan(lsq, engine, n, nq, m, subdim, k, dc, offset):
    rng = np.random.default_rng(n + m + subdim)
    centers = rng.standard_normal((m, H, subdim)).astype(np.float32)
    Q = rng.standard_normal((nq, m * subdim + 3)).astype(np.float32)
    codes = rng.integers(0, H, size=(n, dc), dtype=np.uint8)                 # dc > m: strided code rows, the bytes beyond m unused
    d, i = engine.linscan_pq_dev(dev(codes), dev(Q, offset), dev(centers, offset), m, k, subdim)
    d, i = d.cpu().numpy(), i.cpu().numpy()
    vals, bnd = R.pq_dist(Q[:, :m * subdim], list(centers), codes[:, :m])
    R.check_topk(i, d, vals, bnd, "PQ scan m=%d subdim=%d k=%d offset=%d" % (m, subdim, k, offset))


# ---- norms ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,n,m,offset", [(30, 3000, 4, 0), (64, 2000, 8, 1), (960, 300, 16, 1)])
def test_quantize_norms(lsq, engine, d, n, m, offset):
    rng = np.random.default_rng(d + n)
    K = rng.standard_normal((m * H, d)).astype(np.float32)
    codes = rng.integers(0, H, size=(n, m), dtype=np.uint8)
    n64, nb = R.norms(K, codes, m)
    cb = np.sort(rng.choice(n64, size=min(n, 256), replace=False)).astype(np.float32)
    idx, dbn, nrm = engine.quantize_norms_dev(dev(codes), dev(K, offset), dev(cb), m)
    idx, dbn, nrm = idx.cpu().numpy().astype(np.int64), dbn.cpu().numpy(), nrm.cpu().numpy()
    R.check_values(nrm, n64, nb, "norms d=%d m=%d" % (d, m))
    vals, vb = R.norm_centroid_values(n64, nb, cb)
    R.check_argmin(idx, vals, vb, "norm centroid d=%d m=%d" % (d, m))
    assert np.array_equal(dbn, cb[idx])


# ---- the codebook update (LSQR) --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,n,m,skew,method,cols", [(8, 20_000, 1, False, "normal", None), (100, 20_000, 16, False, "lsqr", [0, 37, 63, 64, 99]),
                                                    (960, 20_000, 8, False, "lsqr", [0, 63, 64, 500, 959]), (8, 1_000_000, 4, False, "normal", None),
                                                    (16, 200_000, 4, True, "normal", None)])
def test_update_codebooks(lsq, engine, d, n, m, skew, method, cols):
    rng = np.random.default_rng(d + n + m)
    X, codes = _lsqr_problem(rng, d, n, m, skew=skew)
    dK, iters = engine.update_codebooks_dev(dev(X), dev(codes.astype(np.uint8)), m)
    K = dK.cpu().numpy()
    assert 1 <= iters
    check_lsqr(K, X, codes, m, np.arange(d) if cols is None else np.array(cols), method, skew)


# ---- the initialisers' kernels ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,d,m", [(64, 24, 3), (100, 32, 4), (129, 64, 8), (40, 32, 16)])
def test_viterbi_is_the_chain_optimum(lsq, engine, n, d, m):
    X, K = _chain_case(7 * n + m, n, d, m)
    B = engine.encode_viterbi(X, K, m).astype(np.int64) - 1
    R.check_chain(X, K, B, m, what="Viterbi (host buffers) m=%d" % m)
    dB = engine.encode_viterbi_dev(dev(X, 1), dev(K), m)                    # X offset by one float
    Bd = dB.cpu().numpy().astype(np.int64)
    R.check_chain(X, K, Bd, m, what="Viterbi (device, offset X) m=%d" % m)
    if m == 3:
        e, _ = R.chain_energy(X[:4], K, Bd[:4], m)
        for i in range(4):
            opt, _ = R.chain_exhaustive_m3(X[i], K)
            _, eb = R.chain_energy(X[i:i + 1], K, Bd[i:i + 1], m)
            assert e[i] <= opt + 2 * eb[0], (i, e[i], opt)


@pytest.mark.parametrize("n,d,m,offset", [(300, 16, 4, 0), (300, 32, 4, 1), (129, 30, 7, 1), (64, 1030, 2, 1)])
def test_assign_codewords(lsq, engine, n, d, m, offset):
    rng = np.random.default_rng(n + d + m)
    X = rng.standard_normal((n, d)).astype(np.float32)
    sd = R.splitarray(d, m)
    K = np.zeros((m * H, d), dtype=np.float32)
    for j in range(m):
        K[j * H:(j + 1) * H, sd[j]] = rng.standard_normal((H, sd[j].stop - sd[j].start))
    Bh, mh = engine.assign_codewords(X, K, m, want_min=True)
    dB, dmin = engine.assign_codewords_dev(dev(X, offset), dev(K, offset), m, want_min=True)
    Bd, md = dB.cpu().numpy().astype(np.int64), dmin.cpu().numpy()
    vals, bnd = R.assign_values(X, K, m, sd)
    for codes, mins, what in ((Bh.astype(np.int64) - 1, mh, "host buffers"), (Bd, md, "device, offset %d" % offset)):
        for j in range(m):
            xs = (X[:, sd[j]].astype(np.float64) ** 2).sum(1)
            R.check_argmin(codes[:, j], vals[j], bnd[j], "assignment (%s), sub-space %d" % (what, j))
            sel = np.arange(n), codes[:, j]
            R.check_values(mins[:, j] + xs, vals[j][sel], bnd[j][sel], "assignment minima (%s), sub-space %d" % (what, j))


# ---- the trainers' host glue ---------------------------------------------------------------------------------------------------------------

def test_kmeans_centres_are_the_means_of_their_members(lsq):
    init = importlib.import_module("local-search-quantization_amd.initializers")
    rng = np.random.default_rng(2)
    r, n = 6, 4096
    centres = rng.standard_normal((r, H)) * 10
    X = (centres[:, rng.integers(0, H, n)] + 0.1 * rng.standard_normal((r, n))).astype(np.float32)
    C, a, _ = init.kmeans(X, H, niter=100, seed=1)
    X64 = X.astype(np.float64)
    cnt = np.bincount(a, minlength=H)
    assert cnt.min() >= 1
    for k in range(H):
        mem = X64[:, a == k]
        # an f32 mean: cnt - 1 adds of the members and one division: gamma_{cnt+1} * mean |x|
        R.check_values(C[:, k], mem.mean(1), R.gamma(cnt[k] + 1) * np.abs(mem).mean(1), "k-means centre %d" % k)
    # converged: every member is (within the bound) nearest to its own centre
    vals, bnd = R.assign_values(X.T, C.T, 1)
    R.check_argmin(a, vals[0], bnd[0], "k-means assignment")


def test_train_opq_rotation_is_orthogonal_and_optimal(lsq, monkeypatch):
    init = importlib.import_module("local-search-quantization_amd.initializers")
    calls = []
    orig = init._procrustes
    monkeypatch.setattr(init, "_procrustes", lambda X, CB: calls.append((X.copy(), CB.copy(), orig(X, CB))) or calls[-1][2])
    rng = np.random.default_rng(4)
    d, n, m = 16, 3000, 4
    X = rng.standard_normal((d, n)).astype(np.float32) * np.linspace(3, 0.3, d, dtype=np.float32)[:, None]
    C, B, Rot, obj = lsq.train_opq(X, m, H, 3, "natural")
    assert calls and np.array_equal(calls[-1][2], Rot)
    Rd = Rot.astype(np.float64)
    assert np.abs(Rd.T @ Rd - np.eye(d)).max() <= 1e-5
    for Xc, CB, Rc in calls:
        M = Xc.astype(np.float64) @ CB.astype(np.float64).T
        best = np.linalg.svd(M, compute_uv=False).sum()                     # max over orthogonal R of trace(R' M): the nuclear norm of M
        got = float((Rc.astype(np.float64) * M).sum())
        # R rounded to f32 (u |R_ij| each) and orthogonal only to that rounding: u * sum |R_ij M_ij| twice, plus the float64 SVD's own error
        assert got >= best - 2 * R.U32 * float((np.abs(Rc) * np.abs(M)).sum()) - 1e-12 * best, (got, best)


def test_train_chainq_codebooks_are_the_block_least_squares(lsq, monkeypatch):
    init = importlib.import_module("local-search-quantization_amd.initializers")
    calls = []
    orig = init.update_codebooks_chain
    monkeypatch.setattr(init, "update_codebooks_chain", lambda X, B, h, V=False: calls.append((X.copy(), np.array(B), orig(X, B, h, V))) or calls[-1][2])
    rng = np.random.default_rng(6)
    d, n, m = 12, 3000, 4
    X = rng.standard_normal((d, n)).astype(np.float32)
    _, B0, R0, _ = lsq.train_opq(X, m, H, 1, "natural")
    C, B, Rot, obj = lsq.train_chainq(X, m, H, R0, B0, None, 2)
    assert calls and all(np.array_equal(a, b) for a, b in zip(calls[-1][2], C))
    od = lsq.get_cbdims_chain(d, m)
    for i in range(m):
        outside = np.ones(d, dtype=bool)
        outside[od[i]] = False
        assert np.all(C[i][outside] == 0), "codebook %d is not zero outside its dimensions" % i
    RX, Bc, _ = calls[-1]
    codes = Bc.T.astype(np.int64) - 1
    Xr = np.ascontiguousarray(RX.T)
    for t in range(d):
        cbs = [i for i in range(m) if od[i].start <= t < od[i].stop]
        Kb = np.concatenate([C[i].T for i in cbs], axis=0)                  # (len(cbs) h, d): the codebooks that cover t
        # scipy LSQR in float64 with atol = btol = sqrt(eps_f32): its stopping rule holds, and the residual is within (1 + 1e-4) of the optimum's
        crit = R.lsqr_stopping_rule(Xr, codes[:, cbs], len(cbs), Kb, [t])
        assert crit[0] <= np.sqrt(np.finfo(np.float32).eps) * (1 + 1e-6), (t, crit)
        _, rec_ref = R.lsq_codebooks(Xr, codes[:, cbs], len(cbs), cols=[t])
        rec = R.reconstruct(Kb[:, [t]], codes[:, cbs], len(cbs))
        r, r0 = np.linalg.norm(Xr[:, [t]] - rec), np.linalg.norm(Xr[:, [t]] - rec_ref)
        assert r <= r0 * (1 + 1e-4), (t, r, r0)
