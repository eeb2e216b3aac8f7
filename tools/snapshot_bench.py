"""Snapshots of a resident index, measured.  Nothing here is promised in advance.  One JSON line per measurement, APPENDED to
profiles/snapshot.jsonl and printed.

    python tools/snapshot_bench.py [--n 1000000] [--dir /dev/shm] [--big 50000000]

The indexes hold random rows (a snapshot moves bytes: their values do not matter): n x 128, m = 8 plain and m = 7 packed, an f16 base, nlist = 1024, a
filter that allows 60 % of the rows.  Every timing is the median of 5 with its spread, the candidates ALTERNATED with their yardstick in one process
after one warm-up round.  Files go to --dir; the record says which file system that is (tmpfs: the write is a copy into the page cache).
  digest        Index.digest() of a base-only uint8 index (ONE section read where it lies: the digest kernel, its sum kernel and the read-back of the
                accumulators) against a float4 device copy of the same bytes (torch), at a launch-bound size (n x 8 bytes) and at 512 MB
  unpack        lsq_index_export of codes + norm bytes of a packed index of --big rows into device arrays (two launches of the unpack kernel) against a
                device copy of the bytes it writes
  save          Index.save() with option "profile": the phases derive / digest / device-to-host / write, against a pinned device-to-host copy of the same
                bytes, at the staging chunk sizes 2, 4, 8, 16, 32 MiB
  load          Engine.load_index() against the rebuild it replaces: create + set_lists + set_filter from host arrays already in memory
  peak_host     the resident set of the process sampled every millisecond during a save and a load, over its value before the call: the two-chunk claim"""
import argparse, ctypes as C, importlib, json, os, statistics, sys, tempfile, threading, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lsq = importlib.import_module("local-search-quantization_amd")
REPS, D, NLIST = 5, 128, 1024
MIB = 1 << 20


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternated(fns, after=None):
    for k, f in fns.items():
        f()
    ms, extra = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(REPS):
        for k, f in fns.items():
            ms[k].append(wall(f)[0])
            if after:
                extra[k].append(after(k))
    return ms, extra


def stat(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def med(v):
    return statistics.median(v)


def rss_bytes():
    with open("/proc/self/statm") as f:
        return int(f.read().split()[1]) * os.sysconf("SC_PAGE_SIZE")


def peak_during(f):
    """(result, peak of the resident set during f() minus its value before) -- sampled from another thread: the library call releases the interpreter"""
    before, peak, stop = rss_bytes(), [0], threading.Event()

    def sample():
        while not stop.is_set():
            peak[0] = max(peak[0], rss_bytes())
            time.sleep(0.001)

    th = threading.Thread(target=sample)
    th.start()
    try:
        out = f()
    finally:
        stop.set()
        th.join()
    return out, max(peak[0] - before, 0)


def fs_of(path):
    best = ("", "?")
    with open("/proc/mounts") as f:
        for line in f:
            _, mount, kind = line.split()[:3]
            if os.path.realpath(path).startswith(mount) and len(mount) > len(best[0]):
                best = (mount, kind)
    return best[1]


def build(eng, dev, g, n, packed):
    m = 7 if packed else 8
    codes = torch.randint(0, 256, (n, m), device=dev, generator=g, dtype=torch.uint8)
    K = torch.randn((m * 256, D), device=dev, generator=g)
    base = torch.randn((n, D), device=dev, generator=g).to(torch.float16)
    if packed:
        ix = eng.index_packed_dev(codes, K, torch.randint(0, 256, (n,), device=dev, generator=g, dtype=torch.uint8), torch.randn(256, device=dev, generator=g), m, base=base)
    else:
        ix = eng.index_dev(codes, K, torch.randn(n, device=dev, generator=g), m, base=base)
    ix.set_lists(torch.randn((NLIST, D), device=dev, generator=g), torch.randint(0, NLIST, (n,), device=dev, generator=g, dtype=torch.int32))
    ix.set_filter(mask=(torch.rand(n, device=dev, generator=g) < 0.6).to(torch.uint8))
    return ix


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--big", type=int, default=50_000_000)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot.jsonl"))
    a = ap.parse_args()
    if not os.access(a.dir, os.W_OK):
        a.dir = tempfile.gettempdir()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(2600)
    sink = open(a.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    path = os.path.join(a.dir, "lsq_snapshot_bench.snap")
    with lsq.Engine(0) as eng:
        common = dict(bench="snapshot", n=a.n, d=D, reps=REPS, device=torch.cuda.get_device_name(0))
        # ---- the digest kernel against a float4 device copy
        for label, rows, width in (("launch-bound", a.n, 8), ("512 MB", 1 << 20, 512)):
            x = torch.randint(0, 256, (rows, width), device=dev, generator=g, dtype=torch.uint8)
            y = torch.empty_like(x)
            with eng.index_dev(None, None, None, 0, base=x, d=width) as ix:
                ms, _ = alternated({"digest": ix.digest, "copy": lambda: y.copy_(x)})
            nbytes = rows * width
            emit(dict(common, what="digest", size=label, bytes=nbytes, digest_ms=stat(ms["digest"]), copy_ms=stat(ms["copy"]),
                      digest_GBps=round(nbytes / med(ms["digest"]) / 1e6, 1), copy_read_GBps=round(nbytes / med(ms["copy"]) / 1e6, 1),
                      digest_vs_copy=round(med(ms["digest"]) / med(ms["copy"]), 3)))
            del x, y
        # ---- the unpack kernel at --big rows against a device copy of its output
        nb, m = a.big, 7
        codes = torch.randint(0, 256, (nb, m), device=dev, generator=g, dtype=torch.uint8)
        nc = torch.randint(0, 256, (nb,), device=dev, generator=g, dtype=torch.uint8)
        K = torch.randn((m * 256, 8), device=dev, generator=g)
        with eng.index_packed_dev(codes, K, nc, torch.randn(256, device=dev, generator=g), m) as ix:
            oc, on = torch.empty_like(codes), torch.empty_like(nc)
            arr = lsq._lib.SnapshotArrays()
            arr.codes, arr.norm_codes = oc.data_ptr(), on.data_ptr()
            L = lsq._lib.load()

            def unpack():
                lsq._lib.check(L.lsq_index_export(ix._h, C.byref(arr), 1))

            def copy():
                oc.copy_(codes)
                on.copy_(nc)

            ms, _ = alternated({"unpack": unpack, "copy": copy})
            assert torch.equal(oc, codes) and torch.equal(on, nc)
            nbytes = nb * (m + 1)
            emit(dict(common, what="unpack", rows=nb, m=m, bytes_out=nbytes, unpack_ms=stat(ms["unpack"]), copy_ms=stat(ms["copy"]),
                      unpack_out_GBps=round(nbytes / med(ms["unpack"]) / 1e6, 1), unpack_vs_copy=round(med(ms["unpack"]) / med(ms["copy"]), 3)))
        del codes, nc, oc, on
        torch.cuda.empty_cache()
        # ---- save, load, peak host memory
        for packed in (False, True):                                         # (a small save and load first: the first call of a process loads code objects)
            with build(eng, dev, g, 4096, packed) as warm:
                warm.save(path)
                eng.load_index(path).close()
            ix = build(eng, dev, g, a.n, packed)
            kind = "packed m=7" if packed else "plain m=8"
            (_, peak_save) = peak_during(lambda: ix.save(path))
            nbytes = os.path.getsize(path)
            (lx, peak_load) = peak_during(lambda: eng.load_index(path, dev=True))
            lx.close()
            emit(dict(common, what="peak_host", index=kind, file_bytes=nbytes, save_peak_bytes=peak_save, load_peak_bytes=peak_load,
                      two_chunks_bytes=ix.snapshot_info()["host_staging_bytes"]))
            pinned = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
            blob = torch.randint(0, 256, (nbytes,), device=dev, generator=g, dtype=torch.uint8)
            eng.set_option("profile", 1)
            for chunk in (2, 4, 8, 16, 32):
                eng.set_option("snapshot_chunk", chunk * MIB)
                phases = {k: [] for k in ("derive_ms", "digest_ms", "copy_ms", "file_ms", "total_ms")}

                def note(k):
                    if k == "save":
                        info = ix.snapshot_info()
                        for p in phases:
                            phases[p].append(info[p])

                ms, _ = alternated({"save": lambda: ix.save(path), "d2h": lambda: pinned.copy_(blob)}, after=note)
                emit(dict(common, what="save", index=kind, chunk_MiB=chunk, file_bytes=nbytes, fs=fs_of(a.dir), save_ms=stat(ms["save"]), pinned_d2h_ms=stat(ms["d2h"]),
                          save_vs_d2h=round(med(ms["save"]) / med(ms["d2h"]), 3), save_GBps=round(nbytes / med(ms["save"]) / 1e6, 2),
                          **{p: round(med(v), 3) for p, v in phases.items()}))
            eng.set_option("snapshot_chunk", 0)
            eng.set_option("profile", 0)
            del pinned, blob
            # ---- load against the rebuild from host arrays already in memory
            ex = ix.export()
            fmt = "f16"

            def rebuild():
                if packed:
                    fx = eng.index_packed(ex["codes"], ex["codebooks"], ex["norm_codes"], ex["cbnorms"], ex["codes"].shape[1], base=ex["base"], base_format=fmt)
                else:
                    fx = eng.index(ex["codes"], ex["codebooks"], ex["dbnorms"], ex["codes"].shape[1], base=ex["base"], base_format=fmt)
                fx.set_lists(ex["centroids"], ex["list_of_row"])
                fx.set_filter(bits=ex["filter_bits"])
                fx.close()

            ms, _ = alternated({"load": lambda: eng.load_index(path).close(), "rebuild": rebuild})
            emit(dict(common, what="load", index=kind, file_bytes=nbytes, fs=fs_of(a.dir), load_ms=stat(ms["load"]), rebuild_ms=stat(ms["rebuild"]),
                      load_vs_rebuild=round(med(ms["load"]) / med(ms["rebuild"]), 3), load_GBps=round(nbytes / med(ms["load"]) / 1e6, 2)))
            ix.close()
            del ex
    if os.path.exists(path):
        os.remove(path)
    sink.close()


if __name__ == "__main__":
    main()
