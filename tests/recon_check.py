"""The decode's contract, said once (tests/test_reconstruct.py, tests/test_gpu_reconstruct.py, tools/reconstruct_bench.py):

    decode(codes, K, m)[i, t] = (((+0.0f + K[(0 h + b_0), t]) + K[(1 h + b_1), t]) + ...) + K[((m - 1) h + b_(m-1)), t]      b = codes[i, :m]

in float32, every add rounded, codebooks ascending, starting from +0.0 -- the bits of reference_api.reconstruct (its zeros / +=) -- and the comparison every
test uses: bit identity, except that where the contract's value is a NaN (inf + -inf gives NaNs of different sign on x86 and on the GPU) any NaN will do.
"""
import numpy as np

H = 256
NAN_BITS = 0x7FC00000


def decode(codes, K, m, h=H):
    """codes (n, >=m) uint8 0-based (further columns -- a packed row's norm byte -- are ignored), K (m*h, d) float32 -> (n, d) float32"""
    codes, K = np.asarray(codes), np.asarray(K, dtype=np.float32)
    out = np.zeros((codes.shape[0], K.shape[1]), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(m):
            out += K[j * h + codes[:, j].astype(np.int64)]
    return out


def add_coarse(x, cent, lor):
    """one more rounded add: the centroid of every row's list"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(x, dtype=np.float32) + np.asarray(cent, dtype=np.float32)[np.asarray(lor, dtype=np.int64)]).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    """the same shape and, element by element, the same bits -- or a NaN where the contract's value is a NaN"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != np.float32 or want.dtype != np.float32:
        return False
    nan = np.isnan(want)
    return bool(np.all(np.where(nan, np.isnan(got), bits(got) == bits(want))))


def decode_ids(codes, K, m, ids, id_base=0, pad_nan=False, cent=None, lor=None):
    """the id form: row r = decode(codes[ids[r] - id_base]) (+ the centroid of its list); with pad_nan an id outside gives a row of NAN_BITS"""
    ids = np.asarray(ids, dtype=np.int64) - id_base
    n = codes.shape[0]
    ok = (ids >= 0) & (ids < n)
    assert pad_nan or ok.all()
    safe = np.where(ok, ids, 0)
    out = decode(codes[safe], K, m)
    if cent is not None:
        out = add_coarse(out, cent, np.asarray(lor)[safe])
    out.view(np.uint32)[~ok] = NAN_BITS
    return out


def special_codebooks(rng, m, d, h=H):
    """codebooks with the values a careless decode gets wrong: column 0 holds -0.0 in EVERY codeword (the contract gives +0.0: the sum starts from +0.0;
    starting from the first codeword would give -0.0); where d allows, column 1 holds +inf in codebook 0 and -inf in the last one (inf - inf: a NaN),
    column 2 a NaN in some codewords, column 3 denormals"""
    K = (rng.standard_normal((m * h, d)) / np.sqrt(m)).astype(np.float32)
    K[:, 0] = -0.0
    if d > 1 and m > 1:
        K[:h, 1] = np.inf
        K[(m - 1) * h:, 1] = -np.inf
    if d > 2:
        K[::7, 2] = np.nan
    if d > 3:
        K[:, 3] = (rng.integers(1, 1 << 20, m * h).astype(np.uint32)).view(np.float32)      # denormals: exponent field 0
    return K


def order_sensitive(n, m, d, seed):
    """(codes, K) on which the contract's sum differs in bits, somewhere, both from the descending-codebook-order sum and from the float64 sum rounded
    once; asserts it.  A decode that reassociates or widens fails on it"""
    rng = np.random.default_rng(seed)
    K = (rng.standard_normal((m * H, d)) * np.exp(rng.uniform(-6, 6, (m * H, 1)))).astype(np.float32)
    codes = rng.integers(0, H, (n, m)).astype(np.uint8)
    want = decode(codes, K, m)
    desc = np.zeros_like(want)
    for j in reversed(range(m)):
        desc += K[j * H + codes[:, j].astype(np.int64)]
    wide = sum(K[j * H + codes[:, j].astype(np.int64)].astype(np.float64) for j in range(m)).astype(np.float32)
    assert (bits(want) != bits(desc)).any(), "the order-sensitivity case does not tell the ascending order from the descending"
    assert (bits(want) != bits(wide)).any(), "the order-sensitivity case does not tell the f32 chain from a float64 sum"
    return codes, K


def reconstruct_cpu(lib, codes, K, m, ids=None, id_base=0, ldo=None, cent=None, lor=None, flags=0, nthreads=0, h=H, sentinel=None):
    """lsq_reconstruct_cpu as it is -> (rc, out (count, ldo) float32 -- the whole pitch, so that the gaps show)"""
    codes = np.asarray(codes, dtype=np.uint8)
    n, d = codes.shape[0], K.shape[1]
    ldc = codes.strides[0] if n > 1 else codes.shape[1]
    count = n if ids is None else len(ids)
    ldo = d if ldo is None else ldo
    out = np.zeros((count, ldo), dtype=np.float32)
    if sentinel is not None:
        out.view(np.uint32)[...] = sentinel
    ids32 = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
    cent32 = None if cent is None else np.ascontiguousarray(cent, dtype=np.float32)
    lor32 = None if lor is None else np.ascontiguousarray(lor, dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data      # noqa: E731
    rc = lib.lsq_reconstruct_cpu(out.ctypes.data, ldo, codes.ctypes.data, ldc, K.ctypes.data, ptr(ids32), count, id_base, n, m, h, d, ptr(cent32), ptr(lor32),
                                 flags, nthreads)
    return rc, out
