"""The beam-search encoder's contract (include/lsq_mi355x.h, "beam-search encoder") restated in numpy on the oracle's unaries and pair tables: what
csrc/lsq_beam.hip is held to bit for bit (tests/test_beam_check.py checks this file, tests/test_gpu_beam.py the kernel against it)."""
import numpy as np

import oracle as O


def beam_exact(X, K, m, L, order=None, h=256):
    """X (n, d) float32 or uint8, K (m h, d), beam width L >= 1, order: visiting order (None: ascending)
    -> codes (n, m) int64 0-based and score (n,) float32 of the rank-0 beam after the last stage."""
    X, K = np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(K, dtype=np.float32)
    n = X.shape[0]
    order = list(range(m)) if order is None else [int(o) for o in order]
    assert sorted(order) == list(range(m)), "order must be a permutation of range(m)"
    U, T = O.unaries(X, K, m, h), O.tables(K, m, h)              # U[j][i][a];  T[j][k][b][a] = 2 <c_kb, c_ja>
    codes, S = np.zeros((n, 1, m), dtype=np.int64), None
    for t, j in enumerate(order):
        if t == 0:
            v = U[j][:, None, :]                                 # stage 0: the unaries, no add
        else:
            s = np.broadcast_to(U[j][:, None, :], (n, codes.shape[1], h))
            for r in range(t):                                   # plain f32 adds in stage order
                s = s + T[j, order[r]][codes[:, :, order[r]]]
            v = S[:, :, None] + s                                # one rounded add
        flat = v.reshape(n, -1)                                  # (p major, a minor): a stable sort IS the (v, p, a) rule
        idx = np.argsort(flat, axis=1, kind="stable")[:, :min(L, flat.shape[1])]
        S = np.take_along_axis(flat, idx, axis=1)
        codes = np.take_along_axis(codes, (idx // h)[:, :, None], axis=1)
        codes[:, :, j] = idx % h
    return codes[:, 0, :].copy(), S[:, 0].astype(np.float32)


def cost_and_score_bound(X, K, m, codes, h=256):
    """float64 reconstruction error ||x - sum_j c_j||^2 of 0-based codes (n, m), and the bound on |(||x||^2 + score) - that| for an f32 score of the contract.

    In real arithmetic ||x||^2 + score IS the reconstruction error: score = sum_j (||c_j||^2 - 2 <x, c_j>) + sum_{j > k} 2 <c_k, c_j>.  The f32 score is that
    sum evaluated with rounding, whatever the order: every leaf (a product x_s c_js, c_js^2 or c_ks c_js; the factors 2 are exact) passes through at most
        d      rounded operations of its own dot product (the product, d - 1 accumulations; an FMA takes one away),
        2      to join the codeword's norm and the unary,
        N - 1  additions among the N = m + m (m - 1) / 2 unaries and table entries (a stage's adds and the S + s of every later stage)
    so the computed score is sum_leaves leaf * prod (1 + delta_i) over at most c = d + 2 + N factors, |delta_i| <= u = 2^-24, and (Higham, Accuracy and
    Stability of Numerical Algorithms, lemma 3.1) |error| <= gamma_c * M with gamma_c = c u / (1 - c u) and M the sum of the leaves' magnitudes:
        M = sum_j sum_s (c_js^2 + 2 |x_s c_js|) + sum_{j > k} sum_s 2 |c_ks c_js|.
    The float64 side (this function and the caller's ||x||^2 + score) follows the same count with u = 2^-53 over leaves of magnitude <= ||x||^2 + M."""
    X64, K64 = np.asarray(X, dtype=np.float64), np.asarray(K, dtype=np.float64)
    d = X64.shape[1]
    C = [K64[j * h + np.asarray(codes)[:, j]] for j in range(m)]               # the chosen codewords, (n, d) each
    cost = ((X64 - sum(C)) ** 2).sum(1)
    M = sum((c * c).sum(1) + 2 * np.abs(X64 * c).sum(1) for c in C)
    for j in range(m):
        for k in range(j):
            M = M + 2 * np.abs(C[k] * C[j]).sum(1)
    c = d + 2 + m + m * (m - 1) // 2
    gamma = lambda u: c * u / (1 - c * u)                                    # noqa: E731
    return cost, gamma(2.0 ** -24) * M + gamma(2.0 ** -53) * ((X64 * X64).sum(1) + M)
