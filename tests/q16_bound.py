"""The inequality the 16-bit filtered walk's window rests on (csrc/lsq_icmq.hip, BOUND), checked directly on a snapshot of the context
(lsq_get_q16_snapshot / Engine.q16_snapshot).  Plain numpy, no GPU.

For every vector i, node j and candidate a the library claims
    |C_i + D_j Q[a] - s_f32[a]| <= slack_j,    Q[a] = qU[a] + SUM_k qT_k[b_k][a]  (the stored 16-bit levels),
    s_f32[a] = ((U_j[a] + T_jk1[b_k1][a]) + T_jk2[b_k2][a]) + ...  (f32 adds, ascending k, k != j),  C_i the same for all 256 candidates,
and takes window_j = floor(2 slack_j / D_j) + 1 from it.  C_i is not observable, but it cancels in the SPREAD of e_a = D Q[a] - s_f32[a]:

    A  max_a e_a - min_a e_a <= 2 slack                                   (exact, no margin: both sides in float64, D Q exact there)
    B  the first f32 argmin and every exact tie of it have Q <= Qmin + window
    C  every unflagged (i, j): qU[a] <= hiq and qU[a] + SUM_k max_b qT_k[b][a] <= 65535 for every a  (levels are unsigned: >= 0 by type) -- all rows
    D  window == floor(2 slack / D) + 1 (or 65535) on the published parameters

A and B are evaluated at code tuples b: the codes the encoder held, seeded random tuples, and ADVERSARIAL tuples built from the snapshot's own levels.
With E_k[b][a] = D qT_k[b][a] - T_k[b][a], the part of E_k that is the same for every b (the column shift the library moved to the unary, its own
business) is removed by centring over b; what is left is the level's rounding error.  For a pair (a1, a2) the tuple that pushes e_a1 - e_a2 furthest takes,
for every k, the row b_k = argmax_b (E_k[b][a1] - E_k[b][a2]) -- 256 choices per term.  Three ways to pick the pair: the arg-max / arg-min of the unary's
own error; starting from the table row of largest error spread; and a search over (a1 in a seeded subset) x (all a2) of the unary difference plus the
sum of the per-table maxima.  Every tuple is a real configuration and is judged through the same f32 chain: no tolerance.

The layouts are restated here (not imported): Uq [m][256/SLQ][rows][SLQ], Tq [m][256/SLQ][R(kk, b)][SLQ], U [m][256/SLF][rows][SLF], T [m][m][256][256].
"""
import numpy as np

H = 256


def slice_widths(m):
    """-> (SLQ, SLF): candidates per 16-bit slice / per f32 slice"""
    return (32, 16) if m <= 8 else (16, 8)


def table_row(m, slq, kk, code):
    """row of (conditioning table kk, code) inside a slice of Tq: [group][code][slot], 4 slots per line for slices of 32, 8 for slices of 16"""
    spl = 4 if slq == 32 else 8
    nt0 = min(m - 1, spl)
    kk, code = np.asarray(kk), np.asarray(code)
    return np.where(kk >= spl, nt0 * H + code * (m - 1 - nt0) + (kk - spl), code * nt0 + kk)


def decode_planes(P, sl):
    """slice-major planes [m][256/sl][rows][sl] -> [m][rows][256]"""
    m, ns, rows, w = P.shape
    assert w == sl and ns * sl == H, (P.shape, sl)
    return np.ascontiguousarray(P.transpose(0, 2, 1, 3)).reshape(m, rows, H)


def decode_tables(Tq, m, slq):
    """Tq [m][256/slq][(m-1)*256][slq] -> [m][m-1 (kk)][256 (code b)][256 (candidate a)]"""
    assert Tq.shape == (m, H // slq, (m - 1) * H, slq), (Tq.shape, m, slq)
    if m == 1:
        return np.zeros((1, 0, H, H), dtype=Tq.dtype)
    idx = table_row(m, slq, np.arange(m - 1)[:, None], np.arange(H)[None, :])          # [kk][b]
    lv = Tq[:, :, idx, :]                                                               # [m][ns][kk][b][slq]
    return np.ascontiguousarray(lv.transpose(0, 2, 3, 1, 4)).reshape(m, m - 1, H, H)


def k_of(j, kk):
    return kk + (1 if kk >= j else 0)


class Snapshot:
    """The numpy side of a snapshot, restricted to `rows` of the chunk (Uq, U and qflag hold those rows only; rows = their indices in the chunk).
    params: dict with D, hiq (f32 [m]), window (int [m]), slack (f64 [m]), ok."""

    def __init__(self, m, params, Uq, Tq, qflag, U, T, rows=None, slq=None, slf=None):
        self.m = int(m)
        d_slq, d_slf = slice_widths(self.m)
        self.slq, self.slf = int(slq or d_slq), int(slf or d_slf)
        self.params = params
        self.qU = decode_planes(np.asarray(Uq).view(np.uint16), self.slq)              # [m][R][256]
        self.qT = decode_tables(np.asarray(Tq).view(np.uint16), self.m, self.slq)      # [m][m-1][256][256]
        self.U = decode_planes(np.asarray(U, dtype=np.float32), self.slf)              # [m][R][256]
        self.T = np.asarray(T, dtype=np.float32).reshape(self.m, self.m, H, H)
        self.qflag = np.asarray(qflag).view(np.uint16).astype(np.int64)
        self.nrows = self.qU.shape[1]
        self.rows = np.arange(self.nrows) if rows is None else np.asarray(rows)
        assert self.U.shape == self.qU.shape and self.qflag.shape == (self.nrows,) and self.rows.shape == (self.nrows,)

    def flagged(self, j):
        return ((self.qflag >> j) & 1).astype(bool)

    def evaluate(self, j, sel, codes):
        """rows `sel` (indices into the snapshot's rows), codes [len(sel)][m] 0-based -> Q int64 [.][256], s float32 [.][256]"""
        Q = self.qU[j][sel].astype(np.int64)
        s = self.U[j][sel].copy()
        for kk in range(self.m - 1):                                                    # ascending k, skipping j: the canonical order
            k = k_of(j, kk)
            Q += self.qT[j, kk][codes[:, k]]
            s = s + self.T[j, k][codes[:, k]]                                           # one f32 rounding per add
        return Q, s


class Report:
    def __init__(self, m):
        self.violations = []                                  # (assertion, node, text, {tuple, row, codes} where they apply)
        self.tight_random = np.zeros(m)
        self.tight_adversarial = np.zeros(m)
        self.pairs_checked = 0
        self.tuples_checked = 0

    def add(self, which, j, text, **info):
        if len(self.violations) < 200:
            self.violations.append((which, j, text, info))

    def reported(self, which=None):
        return [v for v in self.violations if which is None or v[0] == which]

    def merge(self, other):
        self.violations += other.violations
        return self

    def assert_ok(self, what=""):
        assert not self.violations, "%s: %d violations of the filter's bound, the first: %s" % (what, len(self.violations), self.violations[:5])


def check_params(params, m, rep=None):
    """D: the published window against the published slack and step.  D is published as the f32 rounding of the double the window was taken with, so the
    quotient is only known to a relative 2^-24: a window is accepted when it matches the rule for SOME step within that rounding (never more than one
    level of freedom, and only when the quotient sits within 2^-24 of an integer)."""
    rep = rep or Report(m)
    if int(params["ok"]) != 1:
        rep.add("D", -1, "params.ok = %r" % (params["ok"],))
    for j in range(m):
        D, slack, win = float(params["D"][j]), float(params["slack"][j]), int(params["window"][j])
        if not (D > 0 and slack > 0 and np.isfinite(D) and np.isfinite(slack)):
            rep.add("D", j, "D = %r, slack = %r" % (D, slack))
            continue
        want = set()
        for f in (1.0 - 2.0 ** -24, 1.0, 1.0 + 2.0 ** -24):
            w = 2.0 * slack / (D * f)
            want.add(int(np.floor(w)) + 1 if w < 30000.0 else 65535)
        if win not in want:
            rep.add("D", j, "window = %d, floor(2 slack / D) + 1 = %s (slack %.9g, D %.9g)" % (win, sorted(want), slack, D))
    return rep


def check_carry(m, params, Uq, Tq, qflag, slq=None, rep=None):
    """C on EVERY row of a chunk: Uq [m][256/slq][cn][slq] u16, qflag [cn] u16, Tq as in the snapshot.  -> (Report, flagged pairs)"""
    rep = rep or Report(m)
    slq = int(slq or slice_widths(m)[0])
    Uq, qflag = np.asarray(Uq).view(np.uint16), np.asarray(qflag).view(np.uint16)
    qT = decode_tables(np.asarray(Tq).view(np.uint16), m, slq)
    nflag = 0
    for j in range(m):
        flagged = ((qflag >> j) & 1).astype(bool)
        nflag += int(flagged.sum())
        tmax = qT[j].max(axis=1).astype(np.int64).sum(axis=0)                           # SUM_kk max_b qT[a]
        hiq = float(params["hiq"][j])
        room = np.minimum(np.floor(hiq), 65535 - tmax)                                  # the largest unary level candidate a may hold
        lv = Uq[j]                                                                      # [ns][cn][slq]
        if room.min() < 0:
            bad = np.ones(lv.shape[1], dtype=bool)
        else:
            bad = (lv > room.astype(np.uint16).reshape(-1, 1, slq)).any(axis=(0, 2))
        bad &= ~flagged
        for i in np.flatnonzero(bad)[:3]:
            q = lv[:, i, :].reshape(-1).astype(np.int64)
            a = int(np.argmax(q - room))
            rep.add("C", j, "row %d candidate %d: unary level %d, hiq %g, table maxima %d (sum %d), unflagged -- %d such rows"
                    % (i, a, q[a], hiq, tmax[a], q[a] + tmax[a], int(bad.sum())))
    return rep, nflag


def _adversarial_tuples(snap, j, sel, held, rng, pair_subset):
    """-> list of (name, codes [len(sel)][m]) built from the levels' own rounding errors (module docstring)"""
    m = snap.m
    if m == 1:
        return []
    D = float(snap.params["D"][j])
    ks = [k_of(j, kk) for kk in range(m - 1)]
    E = np.stack([D * snap.qT[j, kk].astype(np.float64) - snap.T[j, k].astype(np.float64) for kk, k in enumerate(ks)])      # [kk][b][a]
    colpart = E.mean(axis=1)                                                            # what every b shares: belongs to the unary
    E -= colpart[:, None, :]
    eU = D * snap.qU[j][sel].astype(np.float64) - snap.U[j][sel].astype(np.float64) + colpart.sum(axis=0)[None, :]            # [R][a]
    R = len(sel)

    def best_rows(a1, a2, fixed=None):
        codes = held.copy()
        for kk, k in enumerate(ks):
            codes[:, k] = np.argmax(E[kk][:, a1] - E[kk][:, a2], axis=0)               # [b][R] -> the row that pushes e_a1 - e_a2 furthest
        if fixed is not None:
            codes[:, ks[fixed[0]]] = fixed[1]
        return codes

    out = []
    # 1: the pair = the extremes of the unary's own error
    out.append(("adv_unary", best_rows(np.argmax(eU, axis=1), np.argmin(eU, axis=1))))
    # 2: start from the table row of largest error spread
    spread = E.max(axis=2) - E.min(axis=2)                                              # [kk][b]
    kk0, b0 = np.unravel_index(int(np.argmax(spread)), spread.shape)
    v = eU + E[kk0, b0][None, :]
    out.append(("adv_row", best_rows(np.argmax(v, axis=1), np.argmin(v, axis=1), fixed=(kk0, b0))))
    # 3: search the pair: a1 in a seeded subset, every a2
    if pair_subset > 0:
        S = np.sort(rng.choice(H, size=min(pair_subset, H), replace=False))
        E32 = E.astype(np.float32)
        G = np.zeros((len(S), H), dtype=np.float32)
        for kk in range(m - 1):
            G += (E32[kk][:, S, None] - E32[kk][:, None, :]).max(axis=0)                # max_b (E[b][a1] - E[b][a2])
        score = eU[:, S, None].astype(np.float32) - eU[:, None, :].astype(np.float32) + G[None]      # [R][S][a2]
        flat = score.reshape(R, -1).argmax(axis=1)
        out.append(("adv_pair", best_rows(S[flat // H], flat % H)))
    return out


def check_rows(snap, held, seed=0, nrandom=4, pair_subset=16, rep=None):
    """A and B on every unflagged (row, node) of the snapshot's rows, at the held codes (`held` [rows][m], 0-based), `nrandom` seeded random tuples and
    the adversarial tuples; D on the parameters.  -> Report (tightness = max spread / (2 slack) per node, random and adversarial)"""
    m = snap.m
    rep = rep or Report(m)
    check_params(snap.params, m, rep)
    held = np.asarray(held).astype(np.int64)
    assert held.shape == (snap.nrows, m) and held.min() >= 0 and held.max() < H
    rng = np.random.default_rng(seed)
    for j in range(m):
        sel = np.flatnonzero(~snap.flagged(j))
        if sel.size == 0:
            continue
        D, slack, window = float(snap.params["D"][j]), float(snap.params["slack"][j]), int(snap.params["window"][j])
        tuples = [("held", held[sel])] + [("random%d" % t, rng.integers(0, H, size=(sel.size, m))) for t in range(nrandom)]
        tuples += _adversarial_tuples(snap, j, sel, held[sel], rng, pair_subset)
        rep.pairs_checked += sel.size
        for name, codes in tuples:
            Q, s = snap.evaluate(j, sel, codes)
            rep.tuples_checked += sel.size
            e = D * Q.astype(np.float64) - s.astype(np.float64)
            spread = e.max(axis=1) - e.min(axis=1)
            if not np.all(np.isfinite(spread)):
                rep.add("A", j, "%s: non-finite conditioned sums at row %d" % (name, snap.rows[sel[int(np.argmax(~np.isfinite(spread)))]]))
                continue
            t = float(spread.max()) / (2.0 * slack) if slack > 0 else np.inf
            if name.startswith("adv"):
                rep.tight_adversarial[j] = max(rep.tight_adversarial[j], t)
            else:
                rep.tight_random[j] = max(rep.tight_random[j], t)
            badA = np.flatnonzero(spread > 2.0 * slack)                                 # A: exact, no margin
            for r in badA[:2]:
                rep.add("A", j, "%s: row %d codes %s: spread %.9g > 2 slack %.9g (D %.9g; %d such rows)"
                        % (name, snap.rows[sel[r]], codes[r].tolist(), spread[r], 2.0 * slack, D, badA.size),
                        tuple=name, row=int(snap.rows[sel[r]]), codes=codes[r].tolist())
            smin = s.min(axis=1, keepdims=True)
            Qmin = Q.min(axis=1, keepdims=True)
            badB = np.flatnonzero(((s == smin) & (Q > Qmin + window)).any(axis=1))      # B: the argmin (first or tied) outside the window
            for r in badB[:2]:
                a = int(np.argmin(s[r]))
                rep.add("B", j, "%s: row %d codes %s: the f32 argmin %d has level sum %d, the smallest is %d, window %d (%d such rows)"
                        % (name, snap.rows[sel[r]], codes[r].tolist(), a, Q[r, a], Qmin[r, 0], window, badB.size),
                        tuple=name, row=int(snap.rows[sel[r]]), codes=codes[r].tolist())
    return rep
