"""Float64 replay of the ILS / ICM encoder that judges every node decision and every accept of an encode call.

Written from the method (the reference's encode_icm.jl:55-125 -- perturbation, ICM sweeps, argmin -- and :131-189 / encode_icm_cuda.jl:111-205
-- one node order per ILS iteration, strict-improvement accept), not from oracle/ or the product.  What it shares with them is the build's
RNG (Philox4x32-10 keyed by the seed, counter = global vector index, ILS iteration, domain; restated below from the published algorithm) and
nothing else: the values a node update minimises are computed here in float64 from X and K with this file's own indexing.

For node j of a vector x whose other codebooks hold codewords c_k (k != j), candidate a of codebook j is worth

    E_j(a) = ||c_ja||^2 - 2 <x, c_ja> + sum_{k != j} 2 <c_ja, c_k>            (= ||x - sum_k c_k||^2 minus a constant in a)

evaluated here as ||c_ja||^2 - 2 <x, c_ja> + 2 <r, c_ja>, r = sum_{k != j} c_k (one float64 GEMM per node over all replayed rows).

Bound on the kernel's f32 value of E_j(a) (Higham 3.1, every evaluation order; tests/f64ref.py derives the first two terms):
    the unary          gamma_{2d+2} (||c_ja||^2 + 2 <|x|, |c_ja|>)
  + the pair entries   gamma_d sum_k 2 <|c_k|, |c_ja|>
  + their m - 1 f32 additions   gamma_m (|U| + bound_U + (1 + gamma_d) sum_k 2 <|c_k|, |c_ja|>)
When X and K hold integers and the sum of the magnitudes of every product in the value is at most 2^24, every partial sum any evaluation
forms is an integer of at most that size: every f32 operation is exact and the bound is 0 (the same for a vector's cost with
sum_t (|x_t| + sum_k |c_kt|)^2).  That is the exact regime, where the replay must equal the engine bit for bit.

The decisions.  A candidate can be the kernel's argmin iff its value minus its bound is at most the smallest value plus bound (the
candidate set).  Codewords that are bit-identical get bit-identical f32 values in any deterministic evaluation, so of such twins only the
lowest index can win.  A decision is FORCED when the candidate set holds one canonical codeword, or when every member's bound is 0 (equal
exact values: the lowest index wins).  A decision is VISIBLE when the engine's output shows it: the last sweep's decisions of a vector
whose ILS iteration was accepted (its output differs from the state before).  The accept is forced to reject when the new codes are the
old ones up to twins (bit-identical costs, strict <) or when new cost - bound >= old cost + bound, forced to accept when
new cost + bound < old cost - bound, and visible in every iteration whose output is returned.

Verdict per vector and ILS iteration: VERIFIED (every decision and the accept forced or visible, all agreeing), AMBIGUOUS (a hidden
decision or a hidden accept was a near-tie: counted, not judged), WRONG (the engine's output contradicts a forced or visible decision;
reported with vector, iteration, sweep, node, the candidates, their float64 values and bounds), UNJUDGED (the state before the iteration
or its output is not known).
"""
import numpy as np

import f64ref as R

H = 256
EXACT = 2.0 ** 24
VERIFIED, AMBIGUOUS, WRONG, UNJUDGED = 0, 1, 2, 3
DOM_PERTURB = 1


# ---- the build's RNG: Philox4x32-10 (Salmon et al., SC'11), and the perturbation drawn from it ------------------------------------------

def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised over uint64 arrays holding 32-bit words -> the four output words."""
    M = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & M, np.uint64(k1) & M
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return c0, c1, c2, c3


def rng_word(seed, idx, it, domain, w):
    """32-bit word w of the stream (seed; vector indices idx (array), ILS iteration it, domain) -> uint64 array"""
    idx = np.asarray(idx, dtype=np.uint64)
    out = philox4x32_10(idx & np.uint64(0xFFFFFFFF), idx >> np.uint64(32), np.full(idx.shape, it, np.uint64),
                        np.full(idx.shape, (domain << 16) | (w >> 2), np.uint64), seed & 0xFFFFFFFF, seed >> 32)
    return out[w & 3]


def perturb(codes, npert, seed, it, global_offset=0, h=H):
    """encode_icm.jl:55-70: min(npert, m) distinct positions per vector get a uniform new code.  Positions by the selection-sampling scan of
    the reference's cudautils.cu (take position p with probability need / (m - p)), in integer form on the words p (select) and 16 + p
    (value): take p iff mulhi(word_p, m - p) < need, value mulhi(word_{16+p}, h).  codes (n, m) 0-based -> perturbed copy."""
    codes = np.array(codes, dtype=np.int64)
    n, m = codes.shape
    gidx = np.uint64(global_offset) + np.arange(n, dtype=np.uint64)
    need = np.full(n, min(npert, m), dtype=np.int64)
    for p in range(m):
        take = ((rng_word(seed, gidx, it, DOM_PERTURB, p) * np.uint64(m - p)) >> np.uint64(32)).astype(np.int64) < need
        val = ((rng_word(seed, gidx, it, DOM_PERTURB, 16 + p) * np.uint64(h)) >> np.uint64(32)).astype(np.int64)
        codes[take, p] = val[take]
        need -= take
    return codes


# ---- the float64 quantities of one problem -----------------------------------------------------------------------------------------

class Case:
    """X (n, d), K (m h, d) as the engine sees them (f32), in float64, with what every node update of every replayed row needs."""

    def __init__(self, X, K, m, h=H):
        X32, K32 = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(K, np.float32)
        self.n, self.d = X32.shape
        self.m, self.h = m, h
        self.X = X32.astype(np.float64)
        self.C = K32.astype(np.float64).reshape(m, h, self.d)           # C[j, a] = codeword a of codebook j
        self.aC = np.abs(self.C)
        self.nrm = (self.C * self.C).sum(2)                              # (m, h)
        aX = np.abs(self.X)
        self.U = [self.nrm[j][None, :] - 2.0 * (self.X @ self.C[j].T) for j in range(m)]        # (n, h) per codebook
        self.magU = [self.nrm[j][None, :] + 2.0 * (aX @ self.aC[j].T) for j in range(m)]
        self.integer = bool(np.all(self.X == np.round(self.X)) and np.all(self.C == np.round(self.C)))
        d = self.d
        self.g_u, self.g_t, self.g_s = float(R.gamma(2 * d + 2)), float(R.gamma(d)), float(R.gamma(m))
        # twins: canon[j, a] = the lowest index holding the same f32 codeword (bit for bit) as a
        self.canon = np.empty((m, h), dtype=np.int64)
        for j in range(m):
            _, first, inv = np.unique(K32.reshape(m, h, self.d)[j].view(np.uint32), axis=0, return_index=True, return_inverse=True)
            self.canon[j] = first[inv.reshape(-1)]
        self.is_canon = self.canon == np.arange(h)[None, :]

    def gather(self, codes):
        """codes (r, m) -> sum_k c_k and sum_k |c_k| (r, d)"""
        S = np.zeros((codes.shape[0], self.d))
        A = np.zeros_like(S)
        for k in range(self.m):
            S += self.C[k][codes[:, k]]
            A += self.aC[k][codes[:, k]]
        return S, A

    def node(self, rows, S, A, cj, j):
        """E_j(a) and its bound for the given rows (S, A: their sum_k c_k and sum_k |c_k| over ALL codebooks; cj: their code at j) -> (r, h) x 2"""
        r = S - self.C[j][cj]
        ar = A - self.aC[j][cj]
        U, magU = self.U[j][rows], self.magU[j][rows]
        E = U + 2.0 * (r @ self.C[j].T)
        P = 2.0 * (ar @ self.aC[j].T)
        bU = self.g_u * magU
        b = bU + self.g_t * P + self.g_s * (np.abs(U) + bU + (1.0 + self.g_t) * P)
        if self.integer:
            b = np.where(magU + P <= EXACT, 0.0, b)
        return E, b

    def direct(self, rows, codes, j):
        """||x - sum_k c_k||^2 with codebook j holding each candidate a in turn, straight from the definition -> (r, h)"""
        c = np.asarray(codes)[rows]
        S, _ = self.gather(c)
        res = self.X[rows] - (S - self.C[j][c[:, j]])                    # x - sum_{k != j} c_k
        return ((res[:, None, :] - self.C[j][None, :, :]) ** 2).sum(2)

    def cost(self, rows, codes):
        """f64ref.veccost of the given rows -> (value, bound); bound 0 where every f32 step is exact"""
        K = self.C.reshape(self.m * self.h, self.d).astype(np.float32)
        v, b = R.veccost(self.X[rows].astype(np.float32), K, codes, self.m, self.h)
        if self.integer:
            _, A = self.gather(codes)
            b = np.where(((np.abs(self.X[rows]) + A) ** 2).sum(1) <= EXACT, 0.0, b)
        return v, b

    def same_reconstruction(self, a, b):
        """codes (r, m) x 2: equal up to twins (bit-identical reconstructions, hence bit-identical f32 costs)"""
        j = np.arange(self.m)[None, :]
        return (self.canon[j, a] == self.canon[j, b]).all(1)


# ---- the replay ------------------------------------------------------------------------------------------------------------------------

class Report:
    def __init__(self, I, n):
        self.verdict = np.full((I, n), UNJUDGED, dtype=np.int8)
        self.wrong = []                      # one dict per wrong vector-iteration (its first wrong decision)
        self.equal = [None] * I              # predicted number of equal costs (stats[:, 0]) where every row's is known exactly
        self.accepted = [None] * I           # number of visible accepts (stats[:, 1]) where every row's previous state is known
        self.counters = []                   # disagreements of the engine's ==/< counters with the above

    def counts(self):
        return {k: int((self.verdict == v).sum()) for k, v in (("verified", VERIFIED), ("ambiguous", AMBIGUOUS), ("wrong", WRONG), ("unjudged", UNJUDGED))}

    def fraction_verified(self):
        c = self.counts()
        return c["verified"] / max(1, c["verified"] + c["ambiguous"] + c["wrong"])

    def message(self, limit=3):
        c = self.counts()
        head = "%(wrong)d wrong, %(verified)d verified, %(ambiguous)d ambiguous vector-iterations" % c
        return "\n".join([head] + [_fmt(w) for w in self.wrong[:limit]] + self.counters[:limit])

    def assert_no_wrong(self, what=""):
        if self.wrong or self.counters:
            raise AssertionError("%s: %s" % (what, self.message()))


def _fmt(w):
    return ("vector %(row)d, ILS iteration %(it)d, %(where)s: engine %(engine)s, replay %(expected)s; candidates %(cands)s, float64 values "
            "%(values)s, bounds %(bounds)s" % w)


def replay(case, B0, outs, perturb_fn, orders, icmiter, npert, stats=None):
    """Replay ILS iterations 0..I-1 of an encode call on the rows of `case`.
    B0 (n, m) 0-based initial codes; outs: I entries, the engine's codes (n, m) 0-based after each iteration, or None where the call did
    not return them; perturb_fn(codes, it) -> the perturbed state (the product's perturbation); orders[it]: the node order of iteration it;
    stats (I, 2), when given: the engine's per-iteration (#equal costs, #accepted), checked where the replay determines them.  -> Report"""
    n, m = case.n, case.m
    I = len(outs)
    rep = Report(I, n)
    cur = np.array(B0, dtype=np.int64)
    known = np.ones(n, dtype=bool)
    for it in range(I):
        pert = np.array(perturb_fn(cur, it), dtype=np.int64)
        moved = (pert != cur).sum(1)
        assert (moved <= min(npert, m)).all(), "P5: ILS iteration %d perturbed %d > %d positions of vector %d" % (
            it, moved.max(), npert, int(np.argmax(moved)))
        out = None if outs[it] is None else np.asarray(outs[it], dtype=np.int64)
        cur, known = _iteration(case, rep, it, cur, pert, out, np.asarray(orders[it]), icmiter, known)
        if stats is not None and out is not None:
            if rep.equal[it] is not None and int(stats[it][0]) != rep.equal[it]:
                rep.counters.append("ILS iteration %d: the engine counts %d equal costs, the exact replay %d" % (it, int(stats[it][0]), rep.equal[it]))
            if rep.accepted[it] is not None and int(stats[it][1]) != rep.accepted[it]:
                rep.counters.append("ILS iteration %d: the engine counts %d accepts, its output shows %d" % (it, int(stats[it][1]), rep.accepted[it]))
    return rep


def _iteration(case, rep, it, cur, pert, out, order, icmiter, known):
    n = case.n
    status = np.where(known, VERIFIED, UNJUDGED).astype(np.int8)
    acc = None if out is None else (out != cur).any(1)
    st = pert.copy()
    S, A = case.gather(st)

    for sw in range(icmiter):
        last = sw == icmiter - 1
        for j in order:
            rows = np.nonzero(status == VERIFIED)[0]
            if rows.size == 0:
                break
            E, b = case.node(rows, S[rows], A[rows], st[rows, j], j)
            cand = (E - b <= (E + b).min(1, keepdims=True)) & case.is_canon[j][None, :]
            first = cand.argmax(1)                                       # the lowest index in the candidate set
            forced = (cand.sum(1) == 1) | ~(cand & (b > 0)).any(1)
            vis = acc[rows] & last if acc is not None else np.zeros(rows.size, dtype=bool)
            new = st[rows, j].copy()
            # hidden decisions: follow the forced ones; a near-tie ends the vector's replay
            new[~vis & forced] = first[~vis & forced]
            status[rows[~vis & ~forced]] = AMBIGUOUS
            # visible decisions: the engine's code must be the forced one, or a member of the candidate set
            q = np.nonzero(vis)[0]
            if q.size:
                v = out[rows[q], j]
                ok = np.where(forced[q], v == first[q], cand[q, v])
                for t in q[~ok]:
                    cs = np.nonzero(cand[t])[0][:6].tolist()
                    shown = sorted(set(cs) | {int(out[rows[t], j])})
                    status[rows[t]] = WRONG
                    rep.wrong.append(dict(row=int(rows[t]), it=it, where="sweep %d, node %d" % (sw, j), engine=int(out[rows[t], j]),
                                          expected="%d (forced)" % first[t] if forced[t] else "one of %s" % cs, cands=shown,
                                          values=[float(E[t, c]) for c in shown], bounds=[float(b[t, c]) for c in shown]))
                new[q] = v
            ch = np.nonzero(new != st[rows, j])[0]
            if ch.size:
                r = rows[ch]
                S[r] += case.C[j][new[ch]] - case.C[j][st[r, j]]
                A[r] += case.aC[j][new[ch]] - case.aC[j][st[r, j]]
                st[r, j] = new[ch]

    # the accept: strict < of the f32 costs
    live = np.nonzero(status == VERIFIED)[0]
    nxt = cur.copy() if out is None else out.copy()
    if live.size:
        c1, b1 = case.cost(live, st[live])
        c0, b0 = case.cost(live, cur[live])
        same = case.same_reconstruction(st[live], cur[live])
        must_rej = same | (c1 - b1 >= c0 + b0)
        must_acc = ~same & (c1 + b1 < c0 - b0)
        if out is not None:
            a = acc[live]
            bad = (a & ((st[live] != out[live]).any(1) | must_rej)) | (~a & must_acc)
            for t in np.nonzero(bad)[0]:
                i = live[t]
                status[i] = WRONG
                rep.wrong.append(dict(row=int(i), it=it, where="accept", engine="accepted %s" % out[i].tolist() if a[t] else "rejected",
                                      expected="%s %s" % ("reject" if must_rej[t] else "accept" if must_acc[t] else "either of", st[i].tolist()),
                                      cands=["new", "old"], values=[float(c1[t]), float(c0[t])], bounds=[float(b1[t]), float(b0[t])]))
            if live.size == n and not (b1.any() or b0.any()):
                rep.equal[it] = int((c1 == c0).sum())
        else:
            status[live[~(must_rej | must_acc)]] = AMBIGUOUS
            nxt[live[must_acc]] = st[live[must_acc]]
    if out is None:
        # nothing of this iteration is visible: the vectors whose every decision was forced carry a known state into the next one
        nknown = status == VERIFIED
        status[:] = UNJUDGED
    else:
        nknown = np.ones(n, dtype=bool)
        rep.accepted[it] = int(acc.sum()) if known.all() else None
    rep.verdict[it] = status
    return nxt, nknown


def check_decomposition(case, codes, rows, rtol=1e-12):
    """For every node j of the given rows: the direct ||x - sum_k c_k||^2 minus E_j(a) is the same for every candidate a."""
    codes = np.asarray(codes, dtype=np.int64)
    S, A = case.gather(codes[rows])
    for j in range(case.m):
        E, _ = case.node(rows, S, A, codes[rows, j], j)
        D = case.direct(rows, codes, j)
        diff = D - E
        scale = np.abs(D).max(1, keepdims=True) + np.abs(E).max(1, keepdims=True)
        err = np.abs(diff - diff[:, :1])
        assert (err <= rtol * scale).all(), "node %d: direct - decomposed varies by %g over the candidates" % (j, float(err.max()))


# ---- data for the exact regime -------------------------------------------------------------------------------------------------------

def exact_problem(n, d, m, seed, h=H):
    """X in [0, 7], codebook entries in [-3, 3] (integers), random 1-based initial codes: for d <= 64 and m <= 16 every f32 step of the
    path is exact, and the data are full of exact ties."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 8, size=(n, d)).astype(np.float32)
    K = rng.integers(-3, 4, size=(m * h, d)).astype(np.float32)
    B0 = (rng.integers(0, h, size=(n, m)) + 1).astype(np.int16)
    return X, K, B0
