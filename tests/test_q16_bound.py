"""The checker of the 16-bit filter's bound (tests/q16_bound.py) without a GPU: a synthetic snapshot whose levels are taken by rint against a known
step and slack passes, and each planted violation -- a displaced table level, a slack below the constructed worst case, an unflagged unary level above
hiq, a wrong layout decode, a window that does not follow from the slack -- is reported.  Also: every mutant of tests/q16_mutants.py is one unambiguous
arithmetic-only replacement."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q16_bound as QB  # noqa: E402
import q16_mutants  # noqa: E402

H = 256
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "local-search-quantization_amd", "csrc")


def encode_planes(V, sl):
    """[m][rows][256] -> slice-major [m][256/sl][rows][sl]"""
    m, rows, _ = V.shape
    return np.ascontiguousarray(V.reshape(m, rows, H // sl, sl).transpose(0, 2, 1, 3))


def encode_tables(qT, m, slq, row_of=QB.table_row):
    """[m][m-1][256 b][256 a] -> [m][256/slq][(m-1)*256][slq] with (kk, b) at row row_of(m, slq, kk, b)"""
    out = np.zeros((m, H // slq, (m - 1) * H, slq), dtype=np.uint16)
    for kk in range(m - 1):
        rows = row_of(m, slq, kk, np.arange(H))
        out[:, :, rows, :] = qT[:, kk].reshape(m, H, H // slq, slq).transpose(0, 2, 1, 3)
    return out


def synthetic(m, rows, seed, worst=True, tie=False):
    """A snapshot that obeys the bound by construction: U level = rint((u - min U_j) / D), table level = rint((t - row minimum) / D), D = range sum / 65500,
    slack = m D / 2 + the f32 chain's rounding (m adds of values below smax, 2^-24 each, x2) + the float64 noise of the construction.  worst: row 0's held
    codes are given table entries whose levels err by +0.49 D at candidate 5 and -0.49 D at candidate 9 on node 0 (a spread of >= 0.98 (m - 1) D).
    tie (m = 4): on node 1, row 1's held tuple sees candidate 20 at 100.4 + 3 x 50.4 levels and candidate 21 at 99.6 + 3 x 50.6, far below every other
    candidate: 21 is the f32 argmin by 0.2 D and its level sum is 3 above the smallest."""
    rng = np.random.default_rng(seed)
    slq, slf = QB.slice_widths(m)
    U = (rng.standard_normal((m, rows, H)) * 30.0).astype(np.float32)
    T = (rng.standard_normal((m, m, H, H)) * 5.0).astype(np.float32)
    held = rng.integers(0, H, size=(rows, m))
    loU = U.min(axis=(1, 2)).astype(np.float64)
    lo = T.min(axis=3).astype(np.float64)                                               # [j][k][b]
    rsum = (U.max(axis=(1, 2)) - loU) + np.array([sum((T[j, k].max(axis=1) - T[j, k].min(axis=1)).max() for k in range(m) if k != j) for j in range(m)])
    D = (rsum / 65500.0).astype(np.float32).astype(np.float64)
    if worst and m > 1:
        for k in range(1, m):
            b = held[0, k]
            for a, err in ((5, 0.49), (9, -0.49)):                                      # level q, value lo + (q - err) D: D q - (t - lo) = err D
                q = np.rint((float(T[0, k, b, a]) - lo[0, k, b]) / D[0])
                T[0, k, b, a] = np.float32(lo[0, k, b] + (q - err) * D[0])
        assert np.array_equal(T.min(axis=3).astype(np.float64), lo)
    if tie:
        assert m == 4
        for a, ul, tl in ((20, 100.4, 50.4), (21, 99.6, 50.6)):
            U[1, 1, a] = np.float32(loU[1] + ul * D[1])
            for k in (0, 2, 3):
                T[1, k, held[1, k], a] = np.float32(lo[1, k, held[1, k]] + tl * D[1])
    qU = np.rint((U.astype(np.float64) - loU[:, None, None]) / D[:, None, None])
    qT = np.zeros((m, max(m - 1, 0), H, H))
    for j in range(m):
        for kk in range(m - 1):
            k = QB.k_of(j, kk)
            qT[j, kk] = np.rint((T[j, k].astype(np.float64) - lo[j, k][:, None]) / D[j])
    assert all(qU[j].max() + (qT[j].max(axis=1).sum(axis=0).max() if m > 1 else 0) <= 65535 for j in range(m))
    smax = np.abs(U).max(axis=(1, 2)).astype(np.float64) + np.array([sum(np.abs(T[j, k]).max() for k in range(m) if k != j) for j in range(m)])
    slack = 0.5 * m * D + 2.0 * (m + 1) * smax * 2.0 ** -24
    params = {"ok": 1, "D": D.astype(np.float32), "hiq": np.floor((U.max(axis=(1, 2)) - loU) / D).astype(np.float32) + 2, "slack": slack,
              "window": np.floor(2.0 * slack / D).astype(np.int64) + 1}
    parts = {"m": m, "params": params, "Uq": encode_planes(qU.astype(np.uint16), slq), "Tq": encode_tables(qT.astype(np.uint16), m, slq),
             "qflag": np.zeros(rows, dtype=np.uint16), "U": encode_planes(U, slf), "T": T}
    return parts, held


def snap_of(parts):
    return QB.Snapshot(**parts)


def carry(parts):
    return QB.check_carry(parts["m"], parts["params"], parts["Uq"], parts["Tq"], parts["qflag"])


@pytest.mark.parametrize("m,rows", [(1, 40), (2, 40), (4, 64), (6, 24), (8, 16), (10, 12), (16, 6)])
def test_synthetic_snapshot_passes_and_the_adversary_beats_random_tuples(m, rows):
    parts, held = synthetic(m, rows, seed=m)
    rep = QB.check_rows(snap_of(parts), held, seed=1)
    rep.assert_ok("synthetic m=%d" % m)
    crep, nflag = carry(parts)
    crep.assert_ok("carry")
    assert nflag == 0 and rep.pairs_checked == m * rows and rep.tuples_checked >= 5 * m * rows
    assert np.all(rep.tight_random > 0.0) and np.all(rep.tight_random <= 1.0) and np.all(rep.tight_adversarial <= 1.0)
    if m > 1:
        # rint levels err uniformly in +-D/2: random tuples sit near sqrt(m) D of spread, the adversary must come close to the m D the slack allows
        assert np.all(rep.tight_adversarial > rep.tight_random), (rep.tight_adversarial, rep.tight_random)
        assert rep.tight_adversarial.min() > 0.8, rep.tight_adversarial
        assert rep.tight_adversarial[0] >= 0.98 * (m - 1) / m                           # the planted worst case is found (it is row 0's held tuple as well)


def test_layouts_follow_the_header():
    """the restated row rule against the header's words, and decode(encode) round trips at every m"""
    with open(os.path.join(os.path.dirname(CSRC), "..", "include", "lsq_mi355x.h")) as f:
        hdr = f.read()
    assert "R = b * n0 + kk  (kk < S),  R = n0 * h + b * (m - 1 - n0) + (kk - S)  (kk >= S)" in hdr
    for m in range(2, 17):
        slq = 32 if m <= 8 else 16
        S = 4 if slq == 32 else 8
        n0 = min(m - 1, S)
        rows = [int(QB.table_row(m, slq, kk, b)) for kk in range(m - 1) for b in range(H)]
        want = [b * n0 + kk if kk < S else n0 * H + b * (m - 1 - n0) + (kk - S) for kk in range(m - 1) for b in range(H)]
        assert rows == want and sorted(rows) == list(range((m - 1) * H))                # a permutation of the slice's rows
    rng = np.random.default_rng(0)
    for m in (2, 5, 8, 9, 16):
        slq, slf = QB.slice_widths(m)
        qT = rng.integers(0, 65536, size=(m, m - 1, H, H)).astype(np.uint16)
        assert np.array_equal(QB.decode_tables(encode_tables(qT, m, slq), m, slq), qT)
        V = rng.integers(0, 65536, size=(m, 7, H)).astype(np.uint16)
        assert np.array_equal(QB.decode_planes(encode_planes(V, slq), slq), V)
        # candidate a of (node j, row i) sits where the header says
        P = encode_planes(V, slq).reshape(-1)
        for j, i, a in ((0, 0, 0), (m - 1, 6, 255), (m // 2, 3, slq), (0, 5, slq - 1)):
            assert P[((j * (H // slq) + a // slq) * 7 + i) * slq + a % slq] == V[j, i, a]


@pytest.mark.parametrize("m", [4, 6, 10])
def test_a_table_level_displaced_by_two_is_reported(m):
    parts, held = synthetic(m, 16, seed=20 + m, worst=False)
    slq = QB.slice_widths(m)[0]
    qT = QB.decode_tables(parts["Tq"], m, slq).copy()
    j, kk, b, a = 1, m - 2, int(held[3, QB.k_of(1, m - 2)]), 77                         # a level row 3's held tuple reads (the last table: group 1 at m = 6, 10)
    qT[j, kk, b, a] += 2
    parts["Tq"] = encode_tables(qT, m, slq)
    rep = QB.check_rows(snap_of(parts), held, seed=1)
    assert rep.reported("A") and all(v[1] == j for v in rep.reported("A")), rep.violations
    # (two levels on one term hide inside 2 slack = m D at the held and the random tuples: it takes the adversary, from any row, to expose them)
    adv = [v for v in rep.reported("A") if v[3]["tuple"].startswith("adv")]
    assert adv and all(v[3]["codes"][QB.k_of(j, kk)] == b for v in adv)                 # every reported tuple reads the displaced level


def test_a_slack_below_the_constructed_worst_case_is_reported():
    m = 8
    parts, held = synthetic(m, 16, seed=3)
    rep = QB.check_rows(snap_of(parts), held, seed=1)
    rep.assert_ok()
    p = dict(parts["params"])
    p["slack"] = parts["params"]["slack"].copy()
    p["slack"][0] = 0.45 * (m - 1) * float(p["D"][0])                                   # the planted tuple spreads >= 0.98 (m - 1) D
    p["window"] = np.floor(2.0 * p["slack"] / p["D"].astype(np.float64)).astype(np.int64) + 1
    rep = QB.check_rows(snap_of(dict(parts, params=p)), held, seed=1)
    assert rep.reported("A") and all(v[1] == 0 for v in rep.violations), rep.violations
    assert any(v[2].startswith("held: row 0 ") for v in rep.reported("A"))
    assert not rep.reported("D")                                                        # the window follows from the (wrong) slack: only A can tell


def test_an_unflagged_unary_level_above_hiq_is_reported_and_a_flagged_one_is_not():
    m = 4
    parts, held = synthetic(m, 32, seed=4)
    slq = QB.slice_widths(m)[0]
    qU = QB.decode_planes(parts["Uq"], slq).copy()
    qU[2, 17, 200] = int(parts["params"]["hiq"][2]) + 1
    parts["Uq"] = encode_planes(qU, slq)
    crep, nflag = carry(parts)
    assert len(crep.reported("C")) == 1 and crep.reported("C")[0][1] == 2 and "row 17 candidate 200" in crep.reported("C")[0][2], crep.violations
    parts["qflag"][17] = 1 << 2
    crep, nflag = carry(parts)
    assert nflag == 1 and not crep.violations
    rep = QB.check_rows(snap_of(parts), held, seed=1)                                   # A and B leave the flagged pair alone
    assert rep.pairs_checked == m * 32 - 1 and not rep.violations
    # a level sum that would carry out of 16 bits, hiq permitting
    parts["qflag"][17] = 0
    p = dict(parts["params"], hiq=np.full(m, 65535.0, dtype=np.float32))
    qU[2, 17, 200] = 65000
    crep, _ = QB.check_carry(m, p, encode_planes(qU, slq), parts["Tq"], parts["qflag"])
    assert len(crep.reported("C")) == 1 and "row 17 candidate 200" in crep.reported("C")[0][2]


@pytest.mark.parametrize("m", [6, 10])
def test_a_wrong_layout_decode_is_reported(m):
    parts, held = synthetic(m, 8, seed=5, worst=False)
    slq = QB.slice_widths(m)[0]
    qT = QB.decode_tables(parts["Tq"], m, slq)
    parts["Tq"] = encode_tables(qT, m, slq, row_of=lambda m_, s_, kk, b: kk * H + b)      # table-major rows: not what the library writes
    rep = QB.check_rows(snap_of(parts), held, seed=1)
    assert len(rep.reported("A")) >= m
    parts2, held2 = synthetic(m, 8, seed=5, worst=False)
    with pytest.raises(AssertionError):
        QB.Snapshot(**dict(parts2, slq=32 if slq == 16 else 16))                        # the other slice width does not even fit the planes
    # the f32 unaries decoded with the levels' slice width: every sum is scrambled
    bad = dict(parts2)
    bad["U"] = encode_planes(QB.decode_planes(parts2["U"], QB.slice_widths(m)[1]), slq).reshape(parts2["U"].shape)
    assert len(QB.check_rows(snap_of(bad), held2, seed=1).reported("A")) >= m


def test_window_rule_and_argmin_window():
    m = 4
    parts, held = synthetic(m, 16, seed=6)
    p = dict(parts["params"], window=parts["params"]["window"].copy())
    p["window"][1] = (p["window"][1] - 1) // 2 + 1                                      # half the window
    rep = QB.check_rows(snap_of(dict(parts, params=p)), held, seed=1)
    assert rep.reported("D") and rep.reported("D")[0][1] == 1
    assert not QB.check_params(parts["params"], m).violations
    assert QB.check_params(dict(parts["params"], ok=0), m).reported("D")
    # B: a planted near tie whose f32 argmin has a level sum 3 above the smallest: inside the true window, outside a window of 2
    parts, held = synthetic(m, 16, seed=6, tie=True)
    QB.check_rows(snap_of(parts), held, seed=1).assert_ok("near tie")
    p2 = dict(parts["params"], window=np.full(m, 2, dtype=np.int64))
    rep = QB.check_rows(snap_of(dict(parts, params=p2)), held, seed=1)
    assert [v for v in rep.reported("B") if v[1] == 1 and "held: row 1 " in v[2] and "argmin 21 " in v[2]], rep.violations


def test_every_mutant_is_one_unambiguous_arithmetic_slip():
    assert 4 <= len(q16_mutants.MUTANTS) <= 5 and len(set(q16_mutants.NAMES)) == len(q16_mutants.NAMES)
    assert sum(1 for mu in q16_mutants.MUTANTS if mu[4]) >= 4
    assert set(q16_mutants.FILES) <= {"lsq_icmq.hip", "lsq_gemm.hip"}
    for name, fname, old, new, required in q16_mutants.MUTANTS:
        with open(os.path.join(CSRC, fname)) as f:
            src = f.read()
        assert src.count(old) == 1, name
        out = q16_mutants.mutate(src, name)
        assert out != src and out.count("\n") == src.count("\n")
        # arithmetic only: what changes is a literal, an operator or a variable of the expression -- the copy names no pointer, size, index, loop, branch or
        # launch that the shipped line does not (it may read one parameter less)
        drop = re.sub(r"\s+", " ", old)
        keep = re.sub(r"\s+", " ", new)
        for word in ("[", "]", "*)", "for", "while", "if", "<<<", "hipLaunch", "sizeof", "Idx", "return", "->"):
            assert keep.count(word) <= drop.count(word), (name, word)
        assert old.count("\n") == new.count("\n") and old.count(";") == new.count(";")
