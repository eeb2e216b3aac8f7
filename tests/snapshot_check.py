"""The numpy statement of the snapshot format (include/lsq_mi355x.h (3p), csrc/lsq_snapshot_check.h): the digest, a writer and a reader of the file, and
builders of corrupted files -- which recompute digests where a test needs a corrupt payload under a valid table.  Helpers of tests/test_snapshot.py and
tests/test_gpu_snapshot.py.

THE DIGEST of a byte range whose first byte is byte 0 of word `first_word` of its section, over its little-endian 32-bit words w_i (the last zero-padded):

    SUM_i (uint64) fmix32(w_i ^ (uint32)(i * 0x9E3779B1)) * (uint64)(uint32)(2 i + 1)  +  bytes * 0x9E3779B97F4A7C15        (mod 2^64)
    fmix32(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16

An index's state travels as a dict with the keys of Index.export(): codebooks, codes, dbnorms | norm_codes + cbnorms, base (float32 / uint8 / float16 /
uint16 bfloat16 bits: then base_format="bf16"), centroids + list_of_row, filter_bits (+ filter_force)."""
import struct

import numpy as np

MAGIC = b"LSQSNAP\0"
FORMAT, ENDIAN, HEADER_BYTES, ENTRY_BYTES, ALIGN = 1, 0x01020304, 128, 32, 64
GOLD32, GOLD64 = 0x9E3779B1, 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
KINDS = {"codebooks": 1, "codes": 2, "dbnorms": 3, "norm_codes": 4, "cbnorms": 5, "base": 6, "centroids": 7, "list_of_row": 8, "filter_bits": 9}
NAMES = {v: k for k, v in KINDS.items()}
SECTION_NAMES = {1: "CODEBOOKS", 2: "CODES", 3: "DBNORMS", 4: "NORM_CODES", 5: "CBNORMS", 6: "BASE", 7: "CENTROIDS", 8: "LIST_OF_ROW", 9: "FILTER_BITS"}
DTYPES = {"codebooks": np.float32, "codes": np.uint8, "dbnorms": np.float32, "norm_codes": np.uint8, "cbnorms": np.float32, "centroids": np.float32,
          "list_of_row": np.int32, "filter_bits": np.uint32}
BASE_FORMATS = {"float32": 0, "uint8": 1, "float16": 2, "uint16": 3}
BASE_DTYPES = {0: np.float32, 1: np.uint8, 2: np.float16, 3: np.uint16}
FORCE_DENSE, FORCE_COMPACT = 2, 4
EINVAL, EIO, EFORMAT = -1, -6, -7


def fmix32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def digest(data, first_word=0):
    """the digest of bytes (bytes / any numpy array) as words first_word, first_word + 1, ... of a section -> int"""
    raw = data if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data).tobytes()
    nbytes = len(raw)
    words = np.frombuffer(raw + b"\0" * (-nbytes % 4), dtype="<u4")
    i = np.arange(first_word, first_word + len(words), dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = (i.astype(np.uint32) * np.uint32(GOLD32)).astype(np.uint32)
        pos = (np.uint32(2) * i.astype(np.uint32) + np.uint32(1)).astype(np.uint64)
        total = int(np.sum(fmix32(words ^ key).astype(np.uint64) * pos, dtype=np.uint64)) if len(words) else 0
    return (total + nbytes * GOLD64) & M64


def canonical(state):
    """a state dict -> (scalars, [(kind, element bytes, bytes of the section)]) in file order; filter bits at or past n dropped, allowed recounted"""
    has_codes, has_base = state.get("codes") is not None, state.get("base") is not None
    sc = dict(n=0, d=0, m=0, h=0, packed=0, ncb=0, base_format=0, nlist=0, has_codes=int(has_codes), has_base=int(has_base), filter_active=0, filter_force=0,
              allowed=0)
    arr = {}
    if has_codes:
        arr["codes"] = np.ascontiguousarray(state["codes"], dtype=np.uint8)
        arr["codebooks"] = np.ascontiguousarray(state["codebooks"], dtype=np.float32)
        sc["n"], sc["m"], sc["h"], sc["d"] = arr["codes"].shape[0], arr["codes"].shape[1], 256, arr["codebooks"].shape[1]
        if state.get("norm_codes") is not None:
            arr["norm_codes"], arr["cbnorms"] = np.ascontiguousarray(state["norm_codes"], dtype=np.uint8), np.ascontiguousarray(state["cbnorms"], dtype=np.float32)
            sc["packed"], sc["ncb"] = 1, arr["cbnorms"].shape[0]
        else:
            arr["dbnorms"] = np.ascontiguousarray(state["dbnorms"], dtype=np.float32)
    if has_base:
        arr["base"] = np.ascontiguousarray(state["base"])
        sc["base_format"] = BASE_FORMATS[arr["base"].dtype.name]
        sc["n"], sc["d"] = arr["base"].shape
    if state.get("centroids") is not None:
        arr["centroids"], arr["list_of_row"] = np.ascontiguousarray(state["centroids"], dtype=np.float32), np.ascontiguousarray(state["list_of_row"], dtype=np.int32)
        sc["nlist"] = arr["centroids"].shape[0]
    if state.get("filter_bits") is not None:
        bits = np.array(state["filter_bits"], dtype=np.uint32).reshape(-1)[:(sc["n"] + 31) // 32].copy()
        if sc["n"] % 32:
            bits[-1] &= np.uint32((1 << (sc["n"] % 32)) - 1)
        arr["filter_bits"] = bits
        sc["filter_active"], sc["filter_force"] = 1, int(state.get("filter_force", 0))
        sc["allowed"] = int(sum(bin(int(w)).count("1") for w in bits))
    sections = [(KINDS[k], arr[k].dtype.itemsize, arr[k].tobytes()) for k in sorted(arr, key=KINDS.get)]
    return sc, sections


def align(x):
    return (x + ALIGN - 1) // ALIGN * ALIGN


def table_end(ns):
    return HEADER_BYTES + ENTRY_BYTES * ns + 8


def encode_header(sc, table, file_bytes):
    """table: [(kind, elem, offset, bytes, digest)] -> header + table + header digest"""
    flags = sc["has_codes"] | (sc["has_base"] << 1) | (sc["filter_active"] << 2)
    head = MAGIC + struct.pack("<IIIIqiiiiiiiiiiqq", FORMAT, ENDIAN, HEADER_BYTES, len(table), sc["n"], sc["d"], sc["m"], sc["h"], sc["packed"], sc["ncb"],
                               sc["base_format"], sc["nlist"], flags, sc["filter_force"], 0, sc["allowed"], file_bytes)
    head += b"\0" * (HEADER_BYTES - len(head))
    for kind, elem, off, nbytes, dig in table:
        head += struct.pack("<IIQQQ", kind, elem, off, nbytes, dig)
    return head + struct.pack("<Q", digest(head))


def file_bytes_of(state):
    """the bytes of the snapshot file of a state"""
    sc, sections = canonical(state)
    end, table = table_end(len(sections)), []
    for kind, elem, raw in sections:
        off = align(end)
        table.append((kind, elem, off, len(raw), digest(raw)))
        end = off + len(raw)
    out = bytearray(encode_header(sc, table, end))
    for (kind, elem, off, nbytes, dig), (_, _, raw) in zip(table, sections):
        out += b"\0" * (off - len(out)) + raw
    assert len(out) == end
    return bytes(out)


def write(path, state):
    with open(path, "wb") as f:
        f.write(file_bytes_of(state))


def parse(raw):
    """the reader: file bytes -> (scalars, table [(kind, elem, offset, bytes, digest)], state dict).  Asserts what the format promises"""
    assert raw[:8] == MAGIC
    version, endian, hb, ns, n, d, m, h, packed, ncb, fmt, nlist, flags, force, zero, allowed, fbytes = struct.unpack_from("<IIIIqiiiiiiiiiiqq", raw, 8)
    assert (version, endian, hb, zero) == (FORMAT, ENDIAN, HEADER_BYTES, 0) and fbytes == len(raw) and raw[88:HEADER_BYTES] == b"\0" * (HEADER_BYTES - 88)
    sc = dict(n=n, d=d, m=m, h=h, packed=packed, ncb=ncb, base_format=fmt, nlist=nlist, has_codes=flags & 1, has_base=(flags >> 1) & 1,
              filter_active=(flags >> 2) & 1, filter_force=force, allowed=allowed)
    te = table_end(ns)
    assert struct.unpack_from("<Q", raw, te - 8)[0] == digest(raw[:te - 8])
    table, state, end = [], {}, te
    shapes = {"codebooks": (m * 256, d), "codes": (n, m), "dbnorms": (n,), "norm_codes": (n,), "cbnorms": (ncb,), "base": (n, d), "centroids": (nlist, d),
              "list_of_row": (n,), "filter_bits": ((n + 31) // 32,)}
    for k in range(ns):
        kind, elem, off, nbytes, dig = struct.unpack_from("<IIQQQ", raw, HEADER_BYTES + ENTRY_BYTES * k)
        assert off == align(end) and raw[end:off] == b"\0" * (off - end) and digest(raw[off:off + nbytes]) == dig
        name = NAMES[kind]
        dt = BASE_DTYPES[fmt] if name == "base" else DTYPES[name]
        state[name] = np.frombuffer(raw[off:off + nbytes], dtype=dt).reshape(shapes[name]).copy()
        table.append((kind, elem, off, nbytes, dig))
        end = off + nbytes
    assert end == len(raw)
    if sc["filter_active"]:
        state["filter_force"] = force
    return sc, table, state


def same_state(a, b):
    """two state dicts hold the same keys and the same BYTES (NaN payloads included)"""
    keys = lambda s: {k for k, v in s.items() if v is not None}      # noqa: E731
    if keys(a) != keys(b):
        return False
    for k in keys(a):
        if k == "filter_force":
            if int(a[k]) != int(b[k]):
                return False
        elif np.ascontiguousarray(a[k]).tobytes() != np.ascontiguousarray(b[k]).tobytes() or np.asarray(a[k]).shape != np.asarray(b[k]).shape:
            return False
    return True


# ---- corrupted files ----------------------------------------------------------------------------------------------------------------------------------
def reseal(raw):
    """the header's digest recomputed over a (changed) header and table"""
    raw = bytearray(raw)
    te = table_end(struct.unpack_from("<I", raw, 20)[0])
    struct.pack_into("<Q", raw, te - 8, digest(bytes(raw[:te - 8])))
    return bytes(raw)


def patch_header(raw, offset, fmt, value, seal=True):
    """one header field overwritten (struct format `fmt` at byte `offset`); seal: with the header's digest recomputed, so that only the field is wrong"""
    raw = bytearray(raw)
    struct.pack_into(fmt, raw, offset, value)
    return reseal(raw) if seal else bytes(raw)


def patch_entry(raw, k, field, value, seal=True):
    """field "kind" / "elem" / "offset" / "bytes" / "digest" of table entry k overwritten"""
    off, fmt = {"kind": (0, "<I"), "elem": (4, "<I"), "offset": (8, "<Q"), "bytes": (16, "<Q"), "digest": (24, "<Q")}[field]
    return patch_header(raw, HEADER_BYTES + ENTRY_BYTES * k + off, fmt, value, seal)


def flip_payload_bit(raw, k, byte=0, bit=0):
    """one bit of section k's payload flipped; the table keeps the digest of the original bytes"""
    raw = bytearray(raw)
    off = struct.unpack_from("<Q", raw, HEADER_BYTES + ENTRY_BYTES * k + 8)[0]
    raw[off + byte] ^= 1 << bit
    return bytes(raw)


def corrupt_payload_valid_table(raw, name, mutate):
    """section `name` replaced by mutate(its array) with its digest and the header's RECOMPUTED: a file whose every digest is right and whose payload is bad"""
    sc, table, state = parse(raw)
    state[name] = mutate(state[name].copy())
    out = bytearray(raw)
    for k, (kind, elem, off, nbytes, dig) in enumerate(table):
        if NAMES[kind] == name:
            new = np.ascontiguousarray(state[name]).tobytes()
            assert len(new) == nbytes
            out[off:off + nbytes] = new
            struct.pack_into("<Q", out, HEADER_BYTES + ENTRY_BYTES * k + 24, digest(new))
    return reseal(out)


def nonzero_padding(raw, k):
    """a non-zero byte in the padding before section k (None when that section needs no padding)"""
    prev_end = table_end(struct.unpack_from("<I", raw, 20)[0]) if k == 0 else sum(struct.unpack_from("<QQ", raw, HEADER_BYTES + ENTRY_BYTES * (k - 1) + 8))
    off = struct.unpack_from("<Q", raw, HEADER_BYTES + ENTRY_BYTES * k + 8)[0]
    if off == prev_end:
        return None
    raw = bytearray(raw)
    raw[off - 1] = 1
    return bytes(raw)


# ---- states for the tests -----------------------------------------------------------------------------------------------------------------------------
def make_state(rng, n, m, d, kind="plain", base=None, nlist=0, filt=False, force=0):
    """kind: "plain", "packed", "base-only", "scan-only" (= plain without base rows); base: None / "f32" / "u8" / "f16" / "bf16" """
    s = {}
    if kind != "base-only":
        s["codebooks"] = rng.standard_normal((m * 256, d)).astype(np.float32)
        s["codes"] = rng.integers(0, 256, (n, m), dtype=np.uint8)
        if kind == "packed":
            s["cbnorms"] = np.sort(rng.standard_normal(5).astype(np.float32))
            s["norm_codes"] = rng.integers(0, 5, n, dtype=np.uint8)
        else:
            s["dbnorms"] = rng.standard_normal(n).astype(np.float32)
            s["dbnorms"][0] = np.frombuffer(struct.pack("<I", 0x7FC12345), dtype=np.float32)[0]      # a NaN with a payload: bytes travel verbatim
    if kind == "base-only" and base is None:
        base = "f32"
    if kind == "scan-only":
        base = None
    if base == "f32":
        s["base"] = rng.standard_normal((n, d)).astype(np.float32)
    elif base == "u8":
        s["base"] = rng.integers(0, 256, (n, d), dtype=np.uint8)
    elif base == "f16":
        s["base"] = rng.standard_normal((n, d)).astype(np.float16)
    elif base == "bf16":
        s["base"] = (rng.standard_normal((n, d)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    if nlist and "codes" in s:
        s["centroids"] = rng.standard_normal((nlist, d)).astype(np.float32)
        s["list_of_row"] = rng.integers(0, nlist, n).astype(np.int32)
    if filt:
        bits = rng.integers(0, 1 << 32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32)
        if n % 32:
            bits[-1] &= np.uint32((1 << (n % 32)) - 1)
        s["filter_bits"], s["filter_force"] = bits, force
    return s


def write_args(state):
    """a state dict as the keyword arguments of the package's snapshot_write"""
    kw = {k: v for k, v in state.items() if v is not None}
    if "base" in kw and np.asarray(kw["base"]).dtype == np.uint16:
        kw["base_format"] = "bf16"
    return kw
