"""tools/index_add_bench.py [n] -- appending rows to a resident index (lsq_index_add, csrc/lsq_grow.hip) next to WHAT A CALLER DOES WITHOUT IT: a new index
over the concatenation, set_lists over all rows again, set_filter again.  One JSON line per grid point, written to profiles/index_add.jsonl and printed.
Without arguments: n = 10^6 rows x 128, plain m = 8 and packed m = 7, nlist = 1024.

Data, codebooks, centroids and lists as tools/ivf_bench.py builds them (Gaussian mixture, train_lsq_dev on 20 000 rows, one encode of n + n/10 rows,
train_coarse on 100 000 rows, ivf_assign of every row).  The packed index takes the first 7 code bytes and the norms of their reconstruction quantised to
256 levels: the rows are what the timing needs, not their recall.

Grid: adds of n/1000, n/100 and n/10 rows; an index without lists or filter ("flat") and one with both ("lists+filter": nlist = 1024, a mask of 3/4 of the
rows).  Per point, REPS rounds in ONE process, in each round ALTERNATED:
    add_reserved   a fresh index of n rows (created, lists, filter, reserve(n + count) -- untimed), then Index.add of `count` device rows      -- timed
    add_growing    the same without reserve: the add adopts / re-allocates (geometric, 3/2)                                                    -- timed
    rebuild        the arrays concatenated (torch.cat), index_dev over the n + count rows, set_lists and set_filter over all of them            -- timed
device events around the timed part, option "profile" off, medians; nothing else runs in the process during the timed rounds.  A pass of its own with "profile" on reads growth_info's phase times; merge_ms covers
the sort of the new keys, their offsets, the three shift streams and the placement.  merge_GBps = bytes moved by the shift (old layout read + new layout
written) / merge_ms, beside copy_GBps: a device-to-device torch copy (16 bytes per lane) of the same number of bytes, timed in the same run.
resident_*: device memory in use (hipMemGetInfo) before and after the add, and resident_peak_sampled_over_before_*: the largest excess over `before` that a
second thread read while the add ran (it polls hipMemGetInfo as fast as it can: a sample, so a lower bound of the true peak; the largest of REPS rounds).
These come from ROUNDS OF THEIR OWN, after the timed ones: no poller runs while an add is timed.

The last data line is a RATE POINT at a size where bandwidth decides: n = 5 * 10^7 random rows (plain m = 8, 1024 random lists, no filter), an add of n/1000
rows into reserved capacity with "profile" on: merge_ms there is the three shift streams plus about 0.1 ms of sort and launches, beside a device copy of
the same bytes.  (tools/index_add_bench.py N 0 skips it.)

--probe: the set-up, then one warm-up and five reserved adds of n/100 rows on the plain index with lists and a filter, and nothing else: the run that
`rocprofv3 --kernel-trace --stats` is given to read grow_shift_kernel's own time (profiles/index_add_kernel_stats.csv)."""
import importlib, json, os, statistics, sys, threading
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lsq = importlib.import_module("local-search-quantization_amd")
REPS = 5
D, NLIST = 128, 1024
med = statistics.median


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def mixture(g, dev, centres, n):
    pick = torch.randint(0, centres.shape[0], (n,), device=dev, generator=g)
    return (centres[pick] + torch.randn((n, D), device=dev, generator=g)).contiguous()


def in_use():
    free, total = torch.cuda.mem_get_info()
    return total - free


def rate_point(eng, dev, g, K, dcent, nbig, emit):
    """the merge at a bandwidth-bound size: random rows, random lists"""
    count = nbig // 1000
    codes = torch.randint(0, 256, (nbig + count, 8), device=dev, generator=g, dtype=torch.uint8)
    norms = torch.rand(nbig + count, device=dev, generator=g)
    assign = torch.randint(0, NLIST, (nbig + count,), device=dev, generator=g, dtype=torch.int32)
    eng.set_option("profile", 1)
    ph, totals = [], []
    for _ in range(REPS + 1):                                                   # the first round is the warm-up
        with eng.index_dev(codes[:nbig], K, norms[:nbig], 8) as ix:
            ix.set_lists(dcent, assign[:nbig])
            ix.reserve(nbig + count)
            torch.cuda.synchronize()
            ms, _ = timed(lambda: ix.add(codes=codes[nbig:], dbnorms=norms[nbig:], assign=assign[nbig:]))
            gi = ix.growth_info()
            ph.append(gi["merge_ms"])
            totals.append(ms)
    eng.set_option("profile", 0)
    stream = nbig * 16
    src, dst = torch.empty(stream, dtype=torch.uint8, device=dev), torch.empty(stream, dtype=torch.uint8, device=dev)
    dst.copy_(src)
    cp = med(timed(lambda: dst.copy_(src))[0] for _ in range(REPS))
    mm = med(ph[1:])
    emit(dict(bench="index_add", rate_point=True, format="plain-m8", config="lists", n=nbig, count=count, nlist=NLIST, reps=REPS, add_reserved_profiled_ms=round(med(totals[1:]), 3),
              merge_ms=round(mm, 4), merge_bytes_moved=2 * stream, merge_GBps=round(2 * stream / mm / 1e6, 1), copy_ms=round(cp, 4),
              copy_GBps=round(2 * stream / cp / 1e6, 1), merge_share_of_copy_rate=round(cp / mm, 3)))


def main(n, nbig=50_000_000, probe=False):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    centres = 3.0 * torch.randn((2 * NLIST, D), device=dev, generator=g)
    ntot = n + n // 10
    X = mixture(g, dev, centres, ntot)
    out = open(os.devnull if probe else os.path.join(ROOT, "profiles", "index_add.jsonl"), "w")

    def emit(line):
        s = json.dumps(line)
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    with lsq.Engine(0) as eng:
        ntrain = min(n, 20_000)
        dK8, _, _, _, _ = lsq.train_lsq_dev(X[:ntrain].contiguous(), 8, 256, eng.randinit_dev(3, ntrain, 8), 3, 2, 2, True, 4, seed=5, engine=eng, norm_codebook=False)
        dBs, _, _ = eng.encode_icm_dev(X, eng.randinit_dev(4, ntot, 8), dK8, 8, [2], 2, 4, True, seed=6)
        codes8 = dBs[-1].contiguous()
        zero = torch.zeros(1, dtype=torch.float32, device=dev)
        _, _, norms8 = eng.quantize_norms_dev(codes8, dK8, zero, 8)
        codes7, dK7 = codes8[:, :7].contiguous(), dK8[:7 * 256].contiguous()
        _, _, norms7 = eng.quantize_norms_dev(codes7, dK7, zero, 7)
        cb = torch.quantile(norms7[:100_000].float(), torch.linspace(0, 1, 256, device=dev)).contiguous()
        nc7, _, _ = eng.quantize_norms_dev(codes7, dK7, cb, 7)
        Xh = X.cpu().numpy()
        cent, _ = lsq.train_coarse(Xh[:min(n, 100_000)], NLIST, niter=5, seed=2, engine=eng)
        assign = torch.from_numpy(lsq.ivf_assign(Xh, cent, engine=eng)).to(dev)
        dcent = torch.from_numpy(cent).to(dev)
        del Xh, X
        mask = torch.rand(ntot, device=dev, generator=g) < 0.75
        formats = {"plain-m8": dict(m=8, rowb=8, norm_bytes=4, codes=codes8, K=dK8, norms=norms8.contiguous()),
                   "packed-m7": dict(m=7, rowb=8, norm_bytes=0, codes=codes7, K=dK7, nc=nc7.contiguous(), cb=cb)}
        verdict = {}
        for fname, F in formats.items():
            m = F["m"]

            def make_from(codes, nrm):
                if "nc" in F:
                    return eng.index_packed_dev(codes, F["K"], nrm, F["cb"], m)
                return eng.index_dev(codes, F["K"], nrm, m)

            def make(rows):
                return make_from(F["codes"][:rows], F["nc" if "nc" in F else "norms"][:rows])

            def new_rows(lo, hi, lists):
                kw = dict(codes=F["codes"][lo:hi])
                kw.update(norm_codes=F["nc"][lo:hi]) if "nc" in F else kw.update(dbnorms=F["norms"][lo:hi])
                if lists:
                    kw["assign"] = assign[lo:hi]
                return kw

            for config in ("flat", "lists+filter"):
                lists = config != "flat"

                def dress(ix, rows):
                    if lists:
                        ix.set_lists(dcent, assign[:rows])
                        ix.set_filter(mask=mask[:rows])
                    return ix

                for div in (1000, 100, 10):
                    count = n // div
                    kw = new_rows(n, n + count, lists)
                    times = {"add_reserved": [], "add_growing": [], "rebuild": []}
                    mem = {}

                    def run_add(reserve, watch=False):
                        with dress(make(n), n) as ix:
                            if reserve:
                                ix.reserve(n + count)
                            torch.cuda.synchronize()
                            before = in_use()
                            peak, stop = [before], threading.Event()

                            def poll():
                                while not stop.is_set():
                                    peak[0] = max(peak[0], in_use())
                            th = threading.Thread(target=poll)
                            if watch:
                                th.start()
                            ms, _ = timed(lambda: ix.add(**kw))
                            stop.set()
                            if watch:
                                th.join()
                            return ms, before, in_use(), ix.growth_info(), peak[0]

                    def run_rebuild():
                        def f():                                               # the concatenation has to exist: the caller holds the old arrays and the new rows
                            nk = "nc" if "nc" in F else "norms"
                            cat = [torch.cat([F[k][:n], F[k][n:n + count]]) for k in ("codes", nk)]
                            ix = make_from(*cat)
                            if lists:
                                ix.set_lists(dcent, torch.cat([assign[:n], assign[n:n + count]]))
                                ix.set_filter(mask=torch.cat([mask[:n], mask[n:n + count]]))
                            return ix
                        ms, ix = timed(f)
                        ix.close()
                        return ms

                    if probe:
                        if lists and div == 100 and fname == "plain-m8":
                            for _ in range(REPS + 1):
                                run_add(True)
                        continue
                    run_add(True), run_add(False), run_rebuild()                # warm-up: code objects, scratch of the sorts
                    for _ in range(REPS):                                       # the timed rounds: no poller
                        for key, reserve in (("reserved", True), ("growing", False)):
                            times["add_" + key].append(run_add(reserve)[0])
                        times["rebuild"].append(run_rebuild())
                    for _ in range(REPS):                                       # the memory rounds: a second thread reads the memory in use while the add runs
                        for key, reserve in (("reserved", True), ("growing", False)):
                            _, b, a, gi, pk = run_add(reserve, watch=True)
                            mem[key] = (b, a, gi, max(pk - b, mem[key][3] if key in mem else 0))
                    line = dict(bench="index_add", format=fname, config=config, n=n, count=count, d=D, m=m, nlist=NLIST if lists else 0, reps=REPS)
                    for k, v in times.items():
                        line[k + "_ms"] = round(med(v), 3)
                        line[k + "_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]
                    line["rebuild_over_add_reserved"] = round(line["rebuild_ms"] / line["add_reserved_ms"], 2)
                    line["rebuild_over_add_growing"] = round(line["rebuild_ms"] / line["add_growing_ms"], 2)
                    # memory: measured before / after, and the largest excess over `before` that the polling thread saw during the add
                    for k, (b, a, gi, excess) in mem.items():
                        line["resident_before_%s" % k], line["resident_after_%s" % k] = int(b), int(a)
                        line["resident_peak_sampled_over_before_%s" % k] = int(excess)
                        line["reallocations_%s" % k], line["capacity_rows_%s" % k] = gi["reallocations"], gi["capacity_rows"]
                    line["row_bytes_all_arrays"] = F["rowb"] + F["norm_bytes"]
                    # the phases, from a pass with "profile" on; the merge's rate beside a device copy of the same bytes
                    if lists:
                        eng.set_option("profile", 1)
                        ph = []
                        for _ in range(REPS):
                            _, _, _, gi, _ = run_add(True)
                            ph.append((gi["append_ms"], gi["merge_ms"], gi["filter_ms"]))
                        eng.set_option("profile", 0)
                        line["append_ms"], line["merge_ms"], line["filter_ms"] = (round(med(p[i] for p in ph), 4) for i in range(3))
                        stream = n * (F["rowb"] + 4 + F["norm_bytes"])             # bytes of the old layout: read once, written once
                        src, dst = torch.empty(stream, dtype=torch.uint8, device=dev), torch.empty(stream, dtype=torch.uint8, device=dev)
                        dst.copy_(src)
                        cp = med(timed(lambda: dst.copy_(src))[0] for _ in range(REPS))
                        del src, dst
                        line["merge_bytes_moved"] = 2 * stream
                        line["merge_GBps"] = round(2 * stream / line["merge_ms"] / 1e6, 1)
                        line["copy_ms"], line["copy_GBps"] = round(cp, 4), round(2 * stream / cp / 1e6, 1)
                        line["merge_share_of_copy_rate"] = round(line["merge_GBps"] / line["copy_GBps"], 3)
                    emit(line)
                    if div == 100 and lists:
                        verdict["%s %s" % (fname, config)] = line["rebuild_over_add_reserved"]
        if probe:
            out.close()
            return
        if nbig:
            rate_point(eng, dev, g, dK8, dcent, nbig, emit)
        emit(dict(bench="index_add", summary="acceptance", question="is an add of n/100 rows into reserved capacity faster than the rebuild it replaces (index with lists and a filter)?",
                  rebuild_over_add_reserved=verdict, faster=all(v > 1 for v in verdict.values()), n=n))
    out.close()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--probe"]
    main(int(args[0]) if args else 1_000_000, int(args[1]) if len(args) > 1 else 50_000_000, probe="--probe" in sys.argv)
