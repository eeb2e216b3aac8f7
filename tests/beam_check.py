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
