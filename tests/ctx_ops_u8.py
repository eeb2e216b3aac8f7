"""The 8-bit encode entry points as entries of the context walk, in the pattern of tests/ctx_ops.py (whose catalogue is closed): lsq_encode_icm_u8 and
lsq_encode_icm_u8_dev (blocking and option "async") next to their f32 counterparts and the option moves that change how a chunk is walked.  The driver,
the checkers and the comparison are ctx_ops's own: one long-lived Engine, every step held to the same entry and variant on a FRESH Engine, the fresh
result held to the oracle and the float64 objective.  What the pairs are after: the context's chunk buffers (sX / sX2, the sample), the table cache and the
level buffers are shared by the two element types -- an 8-bit chunk must never be read as an f32 one or the other way round.

Nothing here touches a GPU at import."""
import numpy as np

import ctx_ops as ops

H = ops.H
U8_SYMBOLS = ("lsq_encode_icm_u8", "lsq_encode_icm_u8_dev")
PROFILES = ("default", "chunk_small", "s6_forced")


def _make(n, d, m, seed):
    """random uint8 rows (kept as "X8"; "X" is the widened matrix the checkers read), codebooks = random byte vectors / m"""
    import oracle as O
    rng = np.random.default_rng(seed)
    X8 = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
    K = np.ascontiguousarray(rng.integers(0, 256, size=(m * H, d)).astype(np.float32) / np.float32(m))
    return {"X8": X8, "X": X8.astype(np.float32), "K": K, "B0": O.randinit(3000 + seed % 100000, n, m, H), "ils": [1, 2], "J": 3, "npert": 3,
            "seed": 40 + seed % 7, "it": None}


def _call_host(eng, inp):
    n, d, m = inp["shape"]
    assert inp["X8"].dtype == np.uint8
    return eng.encode_icm(inp["X8"], inp["B0"], inp["K"], m, inp["ils"], inp["J"], inp["npert"], True, seed=inp["seed"])


def _call_dev(nonblocking):
    def call(eng, inp):
        import torch
        n, d, m = inp["shape"]
        dBs, sums, stats = eng.encode_icm_dev(ops.dev(inp["X8"]), ops.dev((inp["B0"] - 1).astype(np.uint8)), ops.dev(inp["K"]), m, inp["ils"], inp["J"],
                                              inp["npert"], True, seed=inp["seed"], nonblocking=nonblocking)
        torch.cuda.current_stream().synchronize()
        if nonblocking:
            sums, stats = sums.cpu().numpy(), stats.cpu().numpy()
        return dBs.cpu().numpy(), sums, stats
    return call


def u8_ops():
    return [
        ops.Op("encode_icm_u8", ["lsq_encode_icm_u8"], ops.ENC_SHAPES, _make, _call_host, ops._enc_check(True, True), encode=True),
        ops.Op("encode_icm_u8_dev", ["lsq_encode_icm_u8_dev"], ops.ENC_SHAPES, _make, _call_dev(False), ops._enc_check(False, False), dev=True, encode=True),
        ops.Op("encode_icm_u8_dev_nb", ["lsq_encode_icm_u8_dev"], ops.ENC_SHAPES, _make, _call_dev(True), ops._enc_check(False, False), dev=True, encode=True),
    ]


def alphabet():
    """the 8-bit entries, the f32 encodes they share a context with, and the option moves"""
    f32 = [o for o in ops.catalogue() if o.name in ("encode_icm", "encode_icm_dev")]
    assert len(f32) == 2
    return u8_ops() + f32 + [ops.Move("opt:" + p, ["lsq_set_option"]) for p in PROFILES]
