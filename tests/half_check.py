"""The contract of the half-precision base rows, stated in numpy -- what tests/test_half_base.py and tests/test_gpu_half_base.py hold the
library to.

  Identity N   narrow(x) is round-to-nearest-even.  f16: the bits of x.astype(np.float16) (overflow to +-inf from 65520 on, subnormals kept, NaN to a NaN).
               bf16: for a non-NaN x with bits u, (u + 0x7fff + ((u >> 16) & 1)) >> 16; NaN to a NaN, payload not pinned.
  Identity W   widening is exact, so an index over the halves H answers as the index over the float32 matrix widen(H): every comparison is bit for bit, NaN
               for NaN.

bf16 rows travel as uint16 arrays holding the bits (numpy has no bfloat16)."""
import numpy as np

F16, BF16 = 2, 3                                    # LSQ_BASE_F16, LSQ_BASE_BF16
FORMATS = {"f16": F16, "bf16": BF16}
HOST_DTYPE = {"f16": np.float16, "bf16": np.uint16}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


def narrow_f16(x):
    """-> float16 array: numpy's own convert, which is IEEE round-to-nearest-even"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(x, dtype=np.float32).astype(np.float16)


def narrow_bf16(x):
    """-> uint16 array of bfloat16 bits: the integer rule; a NaN becomes a quiet NaN of the same sign"""
    u = bits(x).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r[nan] = ((u[nan] >> 16) | 0x0040).astype(np.uint16)
    return r


def narrow(x, fmt):
    return narrow_f16(x) if fmt == "f16" else narrow_bf16(x)


def widen(h, fmt):
    """halves (float16 array, or uint16 bits for bf16) -> float32, exact"""
    if fmt == "f16":
        return np.ascontiguousarray(h).view(np.float16).astype(np.float32)
    return from_bits(np.ascontiguousarray(h).view(np.uint16).astype(np.uint32) << 16)


def half_bits(h):
    return np.ascontiguousarray(h).view(np.uint16)


def same_bits(a, b):
    """float32 arrays equal bit for bit, with NaN where NaN (any payload)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def same_halves(got, want, fmt):
    """narrowed arrays equal bit for bit, NaN for NaN"""
    g, w = half_bits(got), half_bits(want)
    if g.shape != w.shape:
        return False
    gn, wn = np.isnan(widen(g, fmt)), np.isnan(widen(w, fmt))
    return bool(np.array_equal(gn, wn) and np.array_equal(g[~gn], w[~wn]))


def counts(x, fmt):
    """what lsq_index_narrow_base counts: (finite values that became +-inf, non-zero values that became +-0, NaNs)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = widen(narrow(x, fmt), fmt)
    return (int(np.count_nonzero(np.isfinite(x) & np.isinf(w))), int(np.count_nonzero((x != 0) & ~np.isnan(x) & (w == 0))), int(np.count_nonzero(np.isnan(x))))


def edge_values():
    """float32 values at which a narrowing can go wrong, both signs of each"""
    u = [
        0x00000000,                                                           # 0
        0x33000000, 0x33000001, 0x337FFFFF, 0x33800000, 0x33C00000,           # 2^-25 (half of the smallest f16 subnormal: ties to 0), just above, 2^-24, 1.5 2^-24
        0x387FC000, 0x387FE000, 0x38800000,                                   # the largest f16 subnormal, the tie above it, the smallest f16 normal 2^-14
        0x3F800000, 0x3F801000, 0x3F802000, 0x3F803000, 0x3F800FFF, 0x3F801001, 0x3F802FFF, 0x3F803001,      # f16 ties at an even and an odd mantissa, and beside them
        0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,                              # the same for bf16 (16 dropped bits)
        0x477FE000, 0x477FEFFF, 0x477FF000, 0x477FF001, 0x47800000,           # 65504, 65519.99.., 65520 (the first to overflow f16), above, 65536
        0x3F7FFFFF, 0x3F7F7FFF, 0x3F7F8000,                                   # the bf16 carry into the exponent; below the tie; the tie (odd mantissa: up)
        0x7F7FFFFF, 0x7F7F7FFF, 0x7F7F8000,                                   # f32 max (bf16 inf), the largest that stays finite in bf16, the tie that overflows
        0x00000001, 0x007FFFFF, 0x00800000, 0x00008000, 0x00018000, 0x00010000, 0x0000FFFF,      # f32 subnormals (bf16 subnormals and their ties), the smallest normal
        0x00400000, 0x007F8000,                                               # bf16's largest subnormal region, and a subnormal tie that rounds into the normals
        0x7F800000,                                                           # inf
        0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0x7F80FFFF,                       # NaNs: quiet, signalling with a low payload (bits lost by a truncation), all ones
    ]
    u = np.array(u, dtype=np.uint32)
    return from_bits(np.concatenate([u, u | np.uint32(0x80000000)]))


def random_floats(rng, count):
    """float32 values across the whole exponent range: random bit patterns (NaNs and infs among them are kept)"""
    return from_bits(rng.integers(0, 2 ** 32, count, dtype=np.uint64).astype(np.uint32))


def matrix(rng, n, d, scale=1.0, edges=True):
    """(n, d) float32 rows: normal values, the edge values scattered over them, and whole rows of NaN, +-inf and subnormals"""
    X = (rng.standard_normal((n, d)) * scale).astype(np.float32)
    if edges:
        e = edge_values()
        e = e[~np.isnan(e) & np.isfinite(e)]
        at = rng.integers(0, n * d, min(len(e), max(1, n * d // 4)))
        X.reshape(-1)[at] = e[: len(at)]
    return X


def special_rows(X, rng):
    """rows of NaN, +inf, -inf and f16 / bf16 subnormals written into X (n >= 8); -> their indexes"""
    n, d = X.shape
    rows = rng.choice(n, 5, replace=False)
    X[rows[0]] = np.nan
    X[rows[1]] = np.inf
    X[rows[2]] = -np.inf
    X[rows[3]] = from_bits(np.full(d, 0x33800000, np.uint32))                 # 2^-24: an f16 subnormal
    X[rows[4]] = from_bits(np.full(d, 0x00400000, np.uint32))                 # an f32 (and bf16) subnormal
    return rows
