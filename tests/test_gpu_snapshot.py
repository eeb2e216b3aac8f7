"""Snapshots on the device (-m gpu): the two kernels of csrc/lsq_snapshot.hip against the numpy statement of tests/snapshot_check.py, and the two identities
of include/lsq_mi355x.h (3p) --

  Identity S  load(save(ix)) answers every call bit for bit like ix, deterministic statistics included, and like an index freshly built from ix.export();
  Identity F  the bytes of save(ix) are those of snapshot_write over ix.export() and those of the numpy writer over the test's own model of the state;
              digest() is the file's table.

The kernels are reached through the public calls: snap_digest_kernel through Index.digest() of a base-only uint8 index with d = 1 borrowed at any byte
address (its BASE section is then the tensor's bytes, read where they lie), snap_unpack_kernel through the export, the digest and the save of a packed
index.  Option "snapshot_chunk" makes sections straddle staging chunks at these sizes."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_add_check as IA  # noqa: E402
import index_compact_check as ICC  # noqa: E402
import snapshot_check as SC  # noqa: E402

pytestmark = pytest.mark.gpu
N = 4097
LENGTHS = (1, 3, 4, 5, 255, 256, 257, 65535, 65537, (1 << 20) + 3)


@pytest.fixture
def chunked(engine):
    """set the staging chunk for one test; the default comes back afterwards"""
    def set_chunk(value):
        engine.set_option("snapshot_chunk", value)
    yield set_chunk
    engine.set_option("snapshot_chunk", 0)


def _table(info):
    return [(s["kind"], s["elem_bytes"], s["offset"], s["bytes"], s["digest"]) for s in info["sections"]]


def _read(path):
    with open(path, "rb") as f:
        return f.read()


# ---- the kernels against numpy --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 4096])
def test_digest_kernel_equals_numpy_at_every_length_and_alignment(engine, chunked, chunk):
    import torch
    chunked(chunk)
    rng = np.random.default_rng(1)
    raw = rng.integers(0, 256, LENGTHS[-1] + 64, dtype=np.uint8)
    dev = torch.from_numpy(raw).cuda()
    for length in LENGTHS:
        for start in (0, 1, 2, 3, 13):
            view = dev[start:start + length].view(length, 1)                # rows of one byte at any address: the BASE section is these bytes
            with engine.index_dev(None, None, None, 0, base=view, d=1) as ix:
                info = ix.digest()
            want = SC.digest(raw[start:start + length])
            assert (info["n"], info["nsections"]) == (length, 1) and info["sections"][0]["bytes"] == length
            assert info["sections"][0]["digest"] == want, (length, start, chunk)
    # the whole table of such an index is the numpy writer's
    state = {"base": raw[13:13 + 257].reshape(257, 1)}
    with engine.index_dev(None, None, None, 0, base=dev[13:13 + 257].view(257, 1), d=1) as ix:
        sc, table, _ = SC.parse(SC.file_bytes_of(state))
        info = ix.digest()
        assert _table(info) == table and all(info[k] == sc[k] for k in sc)


@pytest.mark.parametrize("n", [1, 63, 64, 65, N])
def test_unpack_kernel_equals_numpy_at_every_row_width(engine, chunked, n, tmp_path):
    rng = np.random.default_rng(n)
    path = str(tmp_path / "p.snap")
    for m in range(1, 17):
        codes = rng.integers(0, 256, (n, m), dtype=np.uint8)
        nc = rng.integers(0, 200, n, dtype=np.uint8)
        cb = rng.standard_normal(200).astype(np.float32)
        K = rng.standard_normal((m * 256, 2)).astype(np.float32)
        state = {"codebooks": K, "codes": codes, "norm_codes": nc, "cbnorms": cb}
        with engine.index_packed(codes, K, nc, cb, m) as ix:
            for dev in (False, True):                                        # the whole streams at once, into host and device arrays
                ex = ix.export(dev=dev)
                assert np.array_equal(IA.to_np(ex["codes"]), codes) and np.array_equal(IA.to_np(ex["norm_codes"]), nc), (n, m, dev)
            want = SC.file_bytes_of(state)
            for chunk in (64, 4096, 0):                                      # sub-ranges of the streams: every chunk start is a multiple of 64
                chunked(chunk)
                assert _table(ix.digest()) == SC.parse(want)[1], (n, m, chunk)
            chunked(64 if m % 2 else 4096)
            ix.save(path)
            assert _read(path) == want, (n, m)


# ---- Identities S and F ----------------------------------------------------------------------------------------------------------------------------------
def _half(a, fmt):
    """(host array in the stored format, torch dtype name) of float32 rows narrowed to fmt"""
    if fmt == "f16":
        return a.astype(np.float16)
    return ((a.view(np.uint32) + np.uint32(0x7FFF) + ((a.view(np.uint32) >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def _build(engine, P, kind, base, dev, pitched):
    """an index over problem P -> (index, the base rows as stored (host array) or None).  dev: borrowed device tensors; pitched: the base is a row view with
    a pitch above d at a byte offset into its allocation"""
    import torch
    n, d = P["n"], P["d"]
    stored, fmt = None, None
    if base is not None:
        rows = np.random.default_rng(P["n"] + 3).standard_normal((n, d)).astype(np.float32)
        if base == "u8":
            stored = (np.abs(rows) * 60).astype(np.uint8)
        elif base == "f32":
            stored = rows
        else:
            stored, fmt = _half(rows, base), base
    b = None
    if stored is not None:
        if dev:
            tdt = {"f32": torch.float32, "u8": torch.uint8, "f16": torch.float16, "bf16": torch.bfloat16}[base]
            t = torch.from_numpy(stored.view(np.int16) if base == "bf16" else stored).cuda()
            t = t.view(torch.bfloat16) if base == "bf16" else t
            if pitched:
                big = torch.zeros((n, d + 5), dtype=tdt, device="cuda")
                big[:, 3:3 + d] = t
                b = big[:, 3:3 + d]                                          # pitch d + 5, start 3 elements into the allocation
            else:
                b = t
        else:
            b = stored
    conv = IA.t if dev else np.ascontiguousarray
    if kind == "base-only":
        ix = (engine.index_dev if dev else engine.index)(None, None, None, 0, base=b, d=d, base_format=None if dev else fmt)
    elif kind == "packed":
        ix = (engine.index_packed_dev if dev else engine.index_packed)(conv(P["codes"]), conv(P["K"]), conv(P["nc"]), conv(P["cb"]), P["m"], base=b,
                                                                       base_format=None if dev else fmt)
    else:
        ix = (engine.index_dev if dev else engine.index)(conv(P["codes"]), conv(P["K"]), conv(P["dbn"]), P["m"], base=b, base_format=None if dev else fmt)
    if "cent" in P and kind != "base-only":
        ix.set_lists(conv(P["cent"]), conv(P["lor"]))
    return ix, stored


def _model(P, kind, stored, bits=None, force=0):
    """the test's own model of the logical state"""
    s = {}
    if kind != "base-only":
        s["codebooks"], s["codes"] = P["K"], P["codes"]
        if kind == "packed":
            s["norm_codes"], s["cbnorms"] = P["nc"], P["cb"]
        else:
            s["dbnorms"] = P["dbn"]
        if "cent" in P:
            s["centroids"], s["list_of_row"] = P["cent"], P["lor"]
    if stored is not None:
        s["base"] = stored
    if bits is not None:
        s["filter_bits"], s["filter_force"] = bits, force
    return s


def _everything(ix, P):
    """every call of the comparison: index_add_check's answers, the decode, the stored rows, a range search -- with the deterministic statistics"""
    lists = bool(getattr(ix, "nlist", 0))
    out = IA.answers(ix, P, nns=(10,), nprobes=(min(3, ix.nlist),) if lists else (), shortlist=40 if ix._has_base else 0, knn=ix._has_base)
    conv = IA.t if ix._dev else (lambda a: a)
    if ix._has_codes:
        ids = np.array([0, ix.n - 1, ix.n // 2, 5 % ix.n], np.int32)
        out["reconstruct"] = ((IA.to_np(ix.reconstruct(ids=conv(ids))),), None)
        if lists:
            out["reconstruct-coarse"] = ((IA.to_np(ix.reconstruct(start=ix.n - 3, add_coarse=True)),), None)
        d0, _ = IA.call(ix, "search", P["Q"][:4], 3)
        radius = np.ascontiguousarray(np.where(np.isfinite(d0[:, 2]), d0[:, 2], 0).astype(np.float32))
        res = ix.range_search(conv(P["Q"][:4]), conv(radius), nprobe=min(2, ix.nlist) if lists else 0, Q_coarse=conv(P["Qc"][:4]) if lists else None)
        out["range"] = (tuple(IA.to_np(a) for a in res), IA.pick(ix.range_info(), ("rows_walked", "results", "max_per_query")))
    if ix._has_base:
        out["base_rows"] = ((IA.to_np(ix.base_rows(start=max(ix.n - 7, 0))),), None)
    return out


def _to_host(key, v):
    """an entry of export(dev=True) as the host form holds it: bfloat16 rows as uint16 bits, the filter's int32 words as uint32"""
    import torch
    if not hasattr(v, "cpu"):
        return v
    if v.dtype == torch.bfloat16:
        return v.view(torch.int16).cpu().numpy().view(np.uint16)
    a = v.cpu().numpy()
    return a.view(np.uint32) if key == "filter_bits" else a


def _fresh_from(engine, ex):
    """the index a caller builds from an export: create, set_lists, set_filter over host arrays"""
    base = ex.get("base")
    fmt = "bf16" if base is not None and base.dtype == np.uint16 else "f16" if base is not None and base.dtype == np.float16 else None
    if "codes" not in ex:
        ix = engine.index(None, None, None, 0, base=base, base_format=fmt)
    elif "norm_codes" in ex:
        ix = engine.index_packed(ex["codes"], ex["codebooks"], ex["norm_codes"], ex["cbnorms"], ex["codes"].shape[1], base=base, base_format=fmt)
    else:
        ix = engine.index(ex["codes"], ex["codebooks"], ex["dbnorms"], ex["codes"].shape[1], base=base, base_format=fmt)
    if "centroids" in ex:
        ix.set_lists(ex["centroids"], ex["list_of_row"])
    if "filter_bits" in ex:
        ix.set_filter(bits=ex["filter_bits"], road={0: None, SC.FORCE_DENSE: "dense", SC.FORCE_COMPACT: "compact"}[ex["filter_force"]])
    return ix


def _check_identities(engine, ix, P, model, path, tmp_path):
    """Identity F on ix against the model, then Identity S: the loaded index and the index built from the export against ix"""
    ix.save(path)
    raw = _read(path)
    assert raw == SC.file_bytes_of(model), "save() differs from the numpy writer over the model"
    sc, table, _ = SC.parse(raw)
    info = ix.digest()
    assert _table(info) == table and info["file_bytes"] == len(raw) and all(info[k] == sc[k] for k in sc)
    assert info["header_digest"] == struct.unpack_from("<Q", raw, SC.table_end(len(table)) - 8)[0]
    lsq = sys.modules["local-search-quantization_amd"]
    assert _table(lsq.snapshot_info(path, verify=True)) == table
    ex = ix.export()
    assert SC.same_state(ex, model), "export() differs from the model"
    assert SC.same_state({k: _to_host(k, v) for k, v in ix.export(dev=True).items()}, model), "export(dev=True) differs from the model"
    other = str(tmp_path / "w.snap")
    lsq.snapshot_write(other, **SC.write_args(ex))
    assert _read(other) == raw, "save() differs from snapshot_write over export()"
    io = ix.snapshot_info()
    assert io["op"] == 1 and io["bytes"] == len(raw) and io["sections"] == len(table) and io["host_staging_bytes"] == 2 * io["chunk_bytes"]
    want = _everything(ix, P)
    with engine.load_index(path, dev=ix._dev) as lx:
        assert (lx.n, lx.d, lx._has_codes, lx._has_base, lx._packed) == (ix.n, ix.d, ix._has_codes, ix._has_base, ix._packed)
        assert lx.snapshot_info()["op"] == 2 and lx.snapshot_info()["bytes"] == len(raw)
        assert IA.equal_answers(_everything(lx, P), want) == []
        if lx._has_base:
            assert lx.base_info()["owned"] == 1 and lx.base_info()["ldb"] == lx.d
        lx.save(other)
        assert _read(other) == raw                                           # saving what was loaded gives the file back
        assert _table(lx.digest()) == table
    with _fresh_from(engine, ex) as fx:
        assert IA.equal_answers(_everything(fx, P), want) == []


CASES = [
    # name, kind, m, base, nlist, filter road, borrowed device tensors, pitched base, staging chunk
    ("plain-m8-f32-host", "plain", 8, "f32", 7, None, False, False, 0),
    ("plain-m8-f16-dev-pitched", "plain", 8, "f16", 300, "dense", True, True, 4096),
    ("plain-m8-f32-dev-pitched", "plain", 8, "f32", 1, "compact", True, True, 4096),
    ("packed-m7-u8-dev-pitched", "packed", 7, "u8", 7, "compact", True, True, 4096),
    ("packed-m8-bf16-host", "packed", 8, "bf16", 300, "none", False, False, 0),
    ("packed-m7-bf16-dev-pitched", "packed", 7, "bf16", 0, "dense", True, True, 4096),
    ("base-only-f16-dev-pitched", "base-only", 0, "f16", 0, "none", True, True, 4096),
    ("base-only-u8-host", "base-only", 0, "u8", 0, None, False, False, 0),
    ("scan-only-m8-host", "scan-only", 8, None, 300, "none", False, False, 4096),
]


@pytest.mark.parametrize("name,kind,m,base,nlist,road,dev,pitched,chunk", CASES, ids=[c[0] for c in CASES])
def test_identities_S_and_F(engine, chunked, tmp_path, name, kind, m, base, nlist, road, dev, pitched, chunk):
    chunked(chunk)
    d = 24
    P = IA.problem(N, max(m, 1), d, 9, seed=len(name), nlist=nlist, packed=kind == "packed", lists="skewed")
    ix, stored = _build(engine, P, kind, base, dev, pitched)
    with ix:
        bits = None
        if road is not None:
            rng = np.random.default_rng(7)
            mask = rng.random(N) < (0.3 if road != "dense" else 0.7)
            ix.set_filter(mask=IA.t(mask.view(np.uint8)) if dev else mask, road=None if road == "none" else road)
            bits = np.packbits(np.concatenate([mask, np.zeros(-N % 32, bool)]).reshape(-1, 32)[:, ::-1], axis=1).view(">u4").astype(np.uint32).reshape(-1)
        force = {"dense": SC.FORCE_DENSE, "compact": SC.FORCE_COMPACT}.get(road, 0)
        model = _model(P, kind, stored, bits, force)
        if dev:
            before = ix.growth_info()
        _check_identities(engine, ix, P, model, str(tmp_path / "a.snap"), tmp_path)
        if dev:                                                              # a borrowing index was saved from the caller's arrays: nothing was adopted
            after = ix.growth_info()
            assert after["adopted"] == 0 and after["reallocations"] == before["reallocations"]
            if ix._has_base:
                assert ix.base_info()["owned"] == 0 and ix.base_info()["ldb"] == d + (5 if pitched else 0)


def test_identities_across_the_65536_thresholds(engine, tmp_path):
    n = 70000
    P = IA.problem(n, 8, 16, 9, seed=70, nlist=7, lists="skewed")
    with IA.fresh(engine, P, n) as ix:
        mask = np.random.default_rng(70).random(n) < 0.95                    # allowed rows above 65536 too
        ix.set_filter(mask=mask)
        bits = np.packbits(np.concatenate([mask, np.zeros(-n % 32, bool)]).reshape(-1, 32)[:, ::-1], axis=1).view(">u4").astype(np.uint32).reshape(-1)
        _check_identities(engine, ix, P, _model(P, "plain", None, bits, 0), str(tmp_path / "big.snap"), tmp_path)


# ---- a life cycle -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
def test_life_cycle(engine, chunked, tmp_path, packed):
    """create -> add -> remove -> compact -> add -> save -> load -> add -> compact: the export is the model after each mutation, the save is byte-equal to a
    fresh index's, and the loaded index stays equal to the original at every later step"""
    chunked(4096)
    total, n0 = 3000, 1500
    P = IA.problem(total, 7 if packed else 8, 16, 9, seed=33, nlist=7, packed=packed, base="f32", lists="skewed")
    kind = "packed" if packed else "plain"
    rows = np.arange(n0)                                                     # the model: the problem's rows the index holds, in order

    def model():
        Ps = ICC.sub(P, rows)
        return Ps, _model(Ps, kind, Ps["base"])

    path, other = str(tmp_path / "life.snap"), str(tmp_path / "fresh.snap")
    with IA.fresh(engine, P, n0) as ix:
        IA.grow(ix, P, n0, 2000)
        rows = np.arange(2000)
        assert SC.same_state(ix.export(), model()[1])
        gone = np.arange(0, 2000, 3, dtype=np.int32)
        ix.remove(gone)
        keep = np.ones(2000, bool)
        keep[gone] = False
        ex = ix.export()                                                     # tombstoned: the rows are still there, the filter says which are allowed
        bits = np.packbits(np.concatenate([keep, np.zeros(-2000 % 32, bool)]).reshape(-1, 32)[:, ::-1], axis=1).view(">u4").astype(np.uint32).reshape(-1)
        assert SC.same_state(ex, dict(model()[1], filter_bits=bits, filter_force=0))
        ix.compact()
        rows = rows[keep]
        assert SC.same_state(ix.export(), model()[1])
        # the next add takes rows 2000 .. 2499 of the problem
        kw = IA.add_args(P, 2000, 2500, ix)
        ix.add(**kw)
        rows = np.concatenate([rows, np.arange(2000, 2500)])
        Ps, mdl = model()
        assert SC.same_state(ix.export(), mdl)
        ix.save(path)
        with IA.fresh(engine, Ps, Ps["n"]) as fx:                            # the save of the grown, compacted, grown index = the save of a fresh one
            fx.save(other)
        assert _read(path) == _read(other) == SC.file_bytes_of(mdl)
        with engine.load_index(path) as lx:
            assert IA.equal_answers(_everything(lx, Ps), _everything(ix, Ps)) == []
            for x in (ix, lx):
                x.add(**IA.add_args(P, 2500, 3000, x))
            rows = np.concatenate([rows, np.arange(2500, 3000)])
            Ps, mdl = model()
            assert lx.n == ix.n == Ps["n"] and SC.same_state(lx.export(), mdl) and SC.same_state(ix.export(), mdl)
            assert IA.equal_answers(_everything(lx, Ps), _everything(ix, Ps)) == []
            gone = np.arange(1, lx.n, 5, dtype=np.int32)
            keep = np.ones(lx.n, bool)
            keep[gone] = False
            for x in (ix, lx):
                x.remove(gone)
            assert IA.equal_answers(_everything(lx, Ps), _everything(ix, Ps)) == []
            for x in (ix, lx):
                x.compact()
            rows = rows[keep]
            Ps, mdl = model()
            assert SC.same_state(lx.export(), mdl) and IA.equal_answers(_everything(lx, Ps), _everything(ix, Ps)) == []
            assert ICC.held_C(lx, Ps, nns=(10,), nprobes=(3,), knn=True) == []
            # new lists on both
            lor2 = np.ascontiguousarray((Ps["lor"] + 1) % 7).astype(np.int32)
            for x in (ix, lx):
                x.set_lists(Ps["cent"], lor2)
            assert IA.equal_answers(_everything(lx, Ps), _everything(ix, Ps)) == []
            lx.save(other)
            ix.save(path)
            assert _read(path) == _read(other) == SC.file_bytes_of(dict(mdl, list_of_row=lor2))


# ---- export's refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_export_refuses_an_absent_array_before_writing_anything(engine, lsq):
    import ctypes as C
    P = IA.problem(300, 8, 16, 3, seed=1)
    L = lsq._lib.load()
    with IA.fresh(engine, P, 300) as ix:
        a = lsq._lib.SnapshotArrays()
        codes = np.full((300, 8), 0xAB, np.uint8)
        base = np.full((300, 16), 7, np.float32)
        a.codes, a.base = codes.ctypes.data, base.ctypes.data                # the index keeps no base rows
        a.n = -5
        assert L.lsq_index_export(ix._h, C.byref(a), 0) == SC.EINVAL and b"BASE" in L.lsq_last_error()
        assert np.all(codes == 0xAB) and np.all(base == 7) and a.n == -5     # the outputs are untouched
        for absent in ("norm_codes", "cbnorms", "centroids", "list_of_row", "filter_bits"):
            b = lsq._lib.SnapshotArrays()
            setattr(b, absent, base.ctypes.data)
            assert L.lsq_index_export(ix._h, C.byref(b), 0) == SC.EINVAL, absent
        assert np.all(base == 7)
        a.base = None
        assert L.lsq_index_export(ix._h, C.byref(a), 0) == 0 and np.array_equal(codes, P["codes"][:300]) and (a.n, a.m, a.d, a.h) == (300, 8, 16, 256)


# ---- refusals on load -------------------------------------------------------------------------------------------------------------------------------------
def test_load_refusals_leave_the_context_serving(engine, lsq, tmp_path, chunked):
    chunked(4096)
    P = IA.problem(N, 7, 16, 9, seed=44, nlist=7, packed=True, lists="skewed")
    P["cb"], P["nc"] = np.ascontiguousarray(P["cb"][:100]), np.ascontiguousarray(P["nc"] % 100)      # a norm table of 100 entries: byte 100 is out of range
    P["dbn"] = P["cb"][P["nc"]]
    state = _model(P, "packed", (np.arange(N * 16).reshape(N, 16) % 251).astype(np.uint8))
    raw = SC.file_bytes_of(state)
    sc, table, _ = SC.parse(raw)
    names = [SC.NAMES[t[0]] for t in table]
    E = SC.EFORMAT
    huge = SC.patch_header(SC.patch_header(SC.patch_header(raw, 24, "<q", (1 << 31) - 2, seal=False), 52, "<i", 0, seal=False), 32, "<i", (1 << 31) - 1)      # f32 rows
    cases = [
        ("magic", b"XSQSNAP\0" + raw[8:], E, "magic"),
        ("newer version", SC.patch_header(raw, 8, "<I", 2), E, "newer"),
        ("big-endian", SC.patch_header(raw, 12, ">I", SC.ENDIAN), E, "big-endian"),
        ("unaligned", SC.patch_entry(raw, 1, "offset", table[1][2] + 4), E, "CODES"),
        ("overlapping", SC.patch_entry(raw, 2, "offset", table[1][2]), E, "overlaps"),
        ("past the end", SC.patch_entry(raw, len(table) - 1, "offset", SC.align(len(raw)) + 64), E, "past the end"),
        ("inconsistent", SC.patch_entry(raw, 1, "bytes", table[1][3] + 7), E, "inconsistent"),
        ("overflow", huge, E, "overflow"),
        ("padding", SC.nonzero_padding(raw, names.index("norm_codes")), E, "non-zero padding"),
        ("short", raw[:-1], E, "truncated"),
        ("flipped bit", SC.flip_payload_bit(raw, names.index("base"), byte=5000, bit=3), E, "BASE"),
        ("flipped bit in the last chunk", SC.flip_payload_bit(raw, names.index("codes"), byte=table[names.index("codes")][3] - 1, bit=7), E, "CODES"),
        # every digest right, the payload wrong: refused by the kernels that refuse such input from any caller
        ("list id = nlist", SC.corrupt_payload_valid_table(raw, "list_of_row", lambda a: np.where(np.arange(len(a)) == 77, 7, a).astype(np.int32)), SC.EINVAL, "list_of_row"),
        ("norm byte = ncb", SC.corrupt_payload_valid_table(raw, "norm_codes", lambda a: np.where(np.arange(len(a)) == 4000, len(P["cb"]), a).astype(np.uint8)), SC.EINVAL, "norm"),
    ]
    import ctypes as C
    L = lsq._lib.load()
    path = str(tmp_path / "bad.snap")
    with IA.fresh(engine, P, N) as beside:                                   # an untouched index on the same context
        want = IA.answers(beside, P, nns=(10,), nprobes=(3,))
        for what, bad, code, word in cases:
            assert bad is not None, what
            with open(path, "wb") as f:
                f.write(bad)
            handle = C.c_void_p(1)
            rc = L.lsq_index_load(C.byref(handle), engine._h, path.encode(), 0)
            msg = L.lsq_last_error().decode()
            assert rc == code and handle.value is None and word in msg, (what, rc, msg)
            assert IA.equal_answers(IA.answers(beside, P, nns=(10,), nprobes=(3,)), want) == [], what
        with pytest.raises(lsq._lib.LsqError) as e:
            engine.load_index(str(tmp_path / "nothing.snap"))
        assert e.value.code == SC.EIO
        with open(path, "wb") as f:                                          # and the good file loads
            f.write(raw)
        with engine.load_index(path) as lx:
            assert SC.same_state(lx.export(), state)
            assert IA.equal_answers(IA.answers(lx, P, nns=(10,), nprobes=(3,)), want) == []


# ---- save failures ----------------------------------------------------------------------------------------------------------------------------------------
def test_failed_saves_leave_the_old_file_intact(engine, lsq, tmp_path):
    P = IA.problem(500, 8, 16, 3, seed=2)
    Pb = IA.problem(400, 8, 16, 3, seed=3)
    with IA.fresh(engine, P, 500) as ix, IA.fresh(engine, Pb, 400) as other:
        with pytest.raises(lsq._lib.LsqError) as e:
            ix.save(str(tmp_path / "missing" / "a.snap"))
        assert e.value.code == SC.EIO and not os.path.exists(str(tmp_path / "missing"))
        path = str(tmp_path / "a.snap")
        ix.save(path)
        old = _read(path)
        assert os.listdir(tmp_path) == ["a.snap"]                            # the temporary is gone
        # the write of the temporary fails: a directory stands where the temporary would be (this holds for any user, a privileged one included)
        os.mkdir(path + ".tmp-snapshot")
        with pytest.raises(lsq._lib.LsqError) as e:
            other.save(path)
        assert e.value.code == SC.EIO and _read(path) == old
        os.rmdir(path + ".tmp-snapshot")
        if os.geteuid() != 0:                                                # a read-only directory: meaningful only where permissions bind
            os.chmod(tmp_path, 0o555)
            try:
                with pytest.raises(lsq._lib.LsqError) as e:
                    other.save(path)
                assert e.value.code == SC.EIO
            finally:
                os.chmod(tmp_path, 0o755)
            assert _read(path) == old and os.listdir(tmp_path) == ["a.snap"]
        other.save(path)                                                     # and a save that succeeds replaces it
        assert _read(path) != old and lsq.snapshot_info(path, verify=True)["n"] == 400
        assert sorted(os.listdir(tmp_path)) == ["a.snap"]
