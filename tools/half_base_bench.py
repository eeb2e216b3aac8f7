"""Half-precision base rows on the resident index, measured.  Nothing here is promised: the re-rank is a gather kernel and halving the row bytes
is the one lever it has that changes no arithmetic; exact k-NN is VALU-bound and should gain memory, not time.  One JSON line per
measurement, APPENDED to profiles/half_base.jsonl and printed.

    python tools/half_base_bench.py [--n 1000000] [--dims 128,960]

Data, codebooks and codes as the other index benches build them (a Gaussian mixture, train_lsq_dev on 20 000 rows with m = 8, one encode of the n rows).  The
f32, f16, bf16 and uint8 indexes hold the SAME rows as far as the format allows (the halves are narrow(X); the bytes are X scaled into 0..255: rows for the
timing, not for recall) and are ALTERNATED in one process: every format once as a warm-up, then 5 rounds in which each runs once, in turn; device events
around every call; medians of 5 with the spread (min, max) beside them.
  rerank        10^4 queries, their ADC shortlists of L = 1000 (from the f32 index's scan) re-ranked to 100; call_ms = events around the call, gather_ms =
                the re-rank kernel alone (lsq_index_stats.gather_ms with option "profile")
  search        search(shortlist = 1000) to 100: the scan and the re-rank
  knn           10^3 queries, k = 100 (d = 128)
  narrow_base   lsq_index_narrow_base's kernel (lsq_index_base_info.narrow_ms) against a device copy of the same f32 bytes (torch, 16 bytes per lane)
  base_rows     lsq_index_get_base on device arrays against a device copy of its output
  recall        recall@R of the re-ranked list against the exact f32 ground truth (Index.knn on the f32 rows), 10^3 queries: what the format costs"""
import argparse, importlib, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lsq = importlib.import_module("local-search-quantization_amd")
REPS, H, M = 5, 256, 8
FORMATS = ("f32", "f16", "bf16", "u8")
RANKS = (1, 2, 5, 10, 20, 50, 100)


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def alternated(fns, after=None):
    """every function once as a warm-up, then REPS rounds in which each runs once, in turn -> {name: [ms]} (and {name: [after(name)]} when given)"""
    for k, f in fns.items():
        f()
        if after:
            after(k)
    torch.cuda.synchronize()
    ms, extra = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(REPS):
        for k, f in fns.items():
            ms[k].append(timed(f)[0])
            if after:
                extra[k].append(after(k))
    return ms, extra


def stat(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def mixture(g, dev, n, d):
    centres = 3.0 * torch.randn((2048, d), device=dev, generator=g)
    pick = torch.randint(0, centres.shape[0], (n,), device=dev, generator=g)
    return (centres[pick] + torch.randn((n, d), device=dev, generator=g)).contiguous()


def point(eng, dev, g, n, d, emit, with_knn):
    X = mixture(g, dev, n, d)
    ntrain = min(n, 20_000)
    dK, _, _, _, _ = lsq.train_lsq_dev(X[:ntrain].contiguous(), M, H, eng.randinit_dev(3, ntrain, M), 3, 2, 2, True, 4, seed=5, engine=eng, norm_codebook=False)
    dBs, _, _ = eng.encode_icm_dev(X, eng.randinit_dev(4, n, M), dK, M, [2], 2, 4, True, seed=6)
    codes = dBs[-1].contiguous()
    _, _, norms = eng.quantize_norms_dev(codes, dK, torch.zeros(1, dtype=torch.float32, device=dev), M)
    lo, hi = X.min(), X.max()
    rows = {"f32": X, "f16": X.to(torch.float16), "bf16": X.to(torch.bfloat16), "u8": ((X - lo) * (255.0 / (hi - lo))).round().clamp(0, 255).to(torch.uint8)}
    nq, L, k = 10_000, 1000, 100
    pick = torch.randint(0, n, (nq,), device=dev, generator=g)
    Q = (X[pick] + 0.5 * torch.randn((nq, d), device=dev, generator=g)).contiguous()
    Q8 = ((Q - lo) * (255.0 / (hi - lo))).contiguous()                       # the queries in the frame of the uint8 rows
    ixs = {f: eng.index_dev(codes, dK, norms, M, base=rows[f]) for f in FORMATS}
    common = dict(bench="half_base", n=n, d=d, m=M, reps=REPS)
    try:
        for f in FORMATS:
            info = ixs[f].base_info()
            emit(dict(common, what="resident", format=f, elem_bytes=info["elem_bytes"], base_bytes=info["resident_bytes"], code_bytes=n * M + 4 * n))
        _, cand = ixs["f32"].search(Q, L)                                     # the ADC shortlists, 1-based: the same candidates for every format
        qf = lambda f: Q8 if f == "u8" else Q                                # noqa: E731
        # ---- the re-rank alone
        eng.set_option("profile", 1)
        last = {f: ixs[f].stats()["gather_ms"] for f in FORMATS}

        def gather(f):
            now = ixs[f].stats()["gather_ms"]
            d_ms, last[f] = now - last[f], now
            return d_ms

        ms, kern = alternated({f: (lambda f=f: ixs[f].rerank(qf(f), cand, k, id_base=1)) for f in FORMATS}, after=gather)
        eng.set_option("profile", 0)
        for f in FORMATS:
            row_bytes = d * ixs[f].base_info()["elem_bytes"]
            g_ms = statistics.median(kern[f])
            emit(dict(common, what="rerank", format=f, nq=nq, L=L, k=k, call_ms=stat(ms[f]), gather_ms=stat(kern[f]), row_bytes=row_bytes,
                      gathered_GBps=round(nq * L * row_bytes / g_ms / 1e6, 1), gather_vs_f32=round(g_ms / statistics.median(kern["f32"]), 3),
                      call_vs_f32=round(statistics.median(ms[f]) / statistics.median(ms["f32"]), 3)))
        # ---- the two stages together
        ms, _ = alternated({f: (lambda f=f: ixs[f].search(Q, k, shortlist=L, Q_exact=qf(f))) for f in FORMATS})
        for f in FORMATS:
            emit(dict(common, what="search", format=f, nq=nq, shortlist=L, k=k, call_ms=stat(ms[f]), call_vs_f32=round(statistics.median(ms[f]) / statistics.median(ms["f32"]), 3)))
        # ---- recall of the re-ranked list against the exact f32 ground truth
        nr = 1000
        _, gt = ixs["f32"].knn(Q[:nr], 1, id_base=1)
        for f in ("f32", "f16", "bf16"):
            _, ids = ixs[f].rerank(Q[:nr], cand[:nr].contiguous(), k, id_base=1)
            emit(dict(common, what="recall", format=f, nq=nr, L=L, against="exact f32 k-NN",
                      recall_at={str(r): round(float((ids[:, :r] == gt[:, :1]).any(dim=1).float().mean()), 4) for r in RANKS}))
        _, adc = ixs["f32"].search(Q[:nr], k)
        emit(dict(common, what="recall", format="adc only (no re-rank)", nq=nr, L=0, against="exact f32 k-NN",
                  recall_at={str(r): round(float((adc[:, :r] == gt[:, :1]).any(dim=1).float().mean()), 4) for r in RANKS}))
        # ---- exact k-NN
        if with_knn:
            nk = 1000
            ms, _ = alternated({f: (lambda f=f: ixs[f].knn(qf(f)[:nk], k)) for f in FORMATS})
            for f in FORMATS:
                emit(dict(common, what="knn", format=f, nq=nk, k=k, call_ms=stat(ms[f]), call_vs_f32=round(statistics.median(ms[f]) / statistics.median(ms["f32"]), 3)))
        # ---- base_rows against a copy of its output
        out, dst = torch.empty((n, d), device=dev), torch.empty((n, d), device=dev)
        fns = {f: (lambda f=f: ixs[f].base_rows(out=out)) for f in ("f16", "bf16", "u8")}
        fns["copy"] = lambda: dst.copy_(out)
        ms, _ = alternated(fns)
        for f in ("f16", "bf16", "u8"):
            emit(dict(common, what="base_rows", format=f, call_ms=stat(ms[f]), copy_ms=stat(ms["copy"]), out_bytes=n * d * 4,
                      call_over_copy=round(statistics.median(ms[f]) / statistics.median(ms["copy"]), 3)))
        del out, dst
    finally:
        for ix in ixs.values():
            ix.close()
    # ---- narrow_base against a device copy of the same f32 bytes (a fresh borrowed index per call: a narrowing happens once)
    eng.set_option("profile", 1)
    src, dst = X, torch.empty_like(X)
    kern = {"f16": [], "bf16": []}
    info = {}

    def narrow(f):
        with eng.index_dev(None, None, None, 0, base=X) as ix:
            before = ix.base_info()["resident_bytes"]
            ix.narrow_base(f)
            info[f] = dict(ix.base_info(), before_bytes=before)
            kern[f].append(info[f]["narrow_ms"])

    ms, _ = alternated({"f16": lambda: narrow("f16"), "bf16": lambda: narrow("bf16"), "copy": lambda: dst.copy_(src)})
    eng.set_option("profile", 0)
    for f in ("f16", "bf16"):
        k_ms = statistics.median(kern[f][1:])
        emit(dict(common, what="narrow_base", format=f, kernel_ms=stat(kern[f][1:]), call_ms=stat(ms[f]), copy_ms=stat(ms["copy"]), read_bytes=n * d * 4, written_bytes=n * d * 2,
                  moved_GBps=round(n * d * 6 / k_ms / 1e6, 1), copy_GBps_both_ways=round(n * d * 8 / statistics.median(ms["copy"]) / 1e6, 1),
                  kernel_over_copy=round(k_ms / statistics.median(ms["copy"]), 3), bytes_before=info[f]["before_bytes"], bytes_after=info[f]["resident_bytes"],
                  to_inf=info[f]["to_inf"], to_zero=info[f]["to_zero"], nans=info[f]["nans"]))


def main(n, dims):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(2500)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    f = open(os.path.join(ROOT, "profiles", "half_base.jsonl"), "a")

    def emit(line):
        line["device"] = torch.cuda.get_device_name(0)
        s = json.dumps(line)
        print(s, flush=True)
        f.write(s + "\n")
        f.flush()

    with lsq.Engine(0) as eng:
        for i, d in enumerate(dims):
            point(eng, dev, g, n, d, emit, with_knn=(i == 0))
            torch.cuda.empty_cache()
    f.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dims", default="128,960")
    a = ap.parse_args()
    main(a.n, [int(x) for x in a.dims.split(",")])
