"""tools/index_compact_bench.py [n] [nbig] -- removing rows from a resident index (lsq_index_remove / lsq_index_compact, csrc/lsq_compact.hip) next to WHAT A
CALLER DOES WITHOUT IT: index_select of its own arrays by old_of_new, a new index over them, set_lists again.  One JSON line per grid point, written to
profiles/index_compact.jsonl and printed.  Without arguments: n = 10^6 rows x 128, nlist = 1024, plain m = 8 and packed m = 7, with and without f32 base
rows; nbig = 5 * 10^7 (0 skips the rate point).

The rows are random (codes, norms, lists, centroids, base): the timings need rows, not their recall.  Removals: n/100, n/10 and n/2 random rows and one
contiguous range of n/10.  Per point, REPS rounds in ONE process, in each round ALTERNATED (device events around the timed part, option "profile" off,
medians; a warm-up round first):
    compact   a fresh index of n rows (created, lists, the rows removed -- untimed), then Index.compact()                                       -- timed
    rebuild   index_select of codes / norms / base / lists by old_of_new, index_dev over them, set_lists                                        -- timed
(a) rebuild_over_compact, with the rebuild's own min .. max as the margin.
(b) a pass of its own with "profile" on reads compact_info's phase times; gather_GBps = 2 x the flat destination bytes / gather_ms beside copy_GBps: a
    device-to-device torch copy (16 bytes per lane) of the same number of bytes, timed in the same run.  The last data line repeats it at a size where
    bandwidth decides: nbig random rows (plain m = 8, lists, no base), n/10 random rows removed.
(c) search (100 queries, 10 neighbours) and search_ivf (16 of 1024 lists) before the removal, under the tombstones and after the compact (indexes without
    base rows: the scans do not read them).
(d) on an index with n/10 rows removed already: Index.remove of 1, 10^3 and 10^5 more ids beside the set_filter of the whole deny list a caller would keep.
(e) device memory in use (hipMemGetInfo) before and after the compact and the largest excess over `before` that a second thread read while it ran (a
    sample: a lower bound of the true peak), with and without shrink, in rounds of their own: no poller runs while a compact is timed."""
import importlib, json, os, statistics, sys, threading
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lsq = importlib.import_module("local-search-quantization_amd")
REPS = 5
D, NLIST, NQ, NN, NPROBE = 128, 1024, 100, 10, 16
med = statistics.median


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def in_use():
    free, total = torch.cuda.mem_get_info()
    return total - free


def watched(f):
    """f() with a second thread polling the memory in use -> (before, after, largest excess over before)"""
    torch.cuda.synchronize()
    before = in_use()
    peak, stop = [before], threading.Event()

    def poll():
        while not stop.is_set():
            peak[0] = max(peak[0], in_use())
    th = threading.Thread(target=poll)
    th.start()
    f()
    torch.cuda.synchronize()
    stop.set()
    th.join()
    return before, in_use(), peak[0] - before


def copy_ms(nbytes, dev):
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst.copy_(src)
    return med(timed(lambda: dst.copy_(src))[0] for _ in range(REPS))


def main(n, nbig):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    out = open(os.path.join(ROOT, "profiles", "index_compact.jsonl"), "w")

    def emit(line):
        s = json.dumps(line)
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    def rows(count, m):
        return (torch.randint(0, 256, (count, m), device=dev, generator=g, dtype=torch.uint8), torch.rand(count, device=dev, generator=g),
                torch.randint(0, NLIST, (count,), device=dev, generator=g, dtype=torch.int32))

    with lsq.Engine(0) as eng:
        K8 = torch.randn((8 * 256, D), device=dev, generator=g) / 8 ** 0.5
        cent = torch.randn((NLIST, D), device=dev, generator=g)
        Q = torch.randn((NQ, D), device=dev, generator=g)
        codes8, norms, assign = rows(n, 8)
        base = torch.randn((n, D), device=dev, generator=g)
        cb = torch.sort(torch.rand(256, device=dev, generator=g))[0].contiguous()
        nc = torch.randint(0, 256, (n,), device=dev, generator=g, dtype=torch.uint8)
        formats = {"plain-m8": dict(m=8, codes=codes8, K=K8, norms=norms, rowb=8, norm_bytes=4),
                   "packed-m7": dict(m=7, codes=codes8[:, :7].contiguous(), K=K8[:7 * 256].contiguous(), nc=nc, cb=cb, rowb=8, norm_bytes=0)}
        perm = torch.randperm(n, device=dev, generator=g).int()
        removals = {"random n/100": perm[: n // 100].contiguous(), "random n/10": perm[: n // 10].contiguous(), "random n/2": perm[: n // 2].contiguous(),
                    "range n/10": torch.arange(n // 3, n // 3 + n // 10, device=dev, dtype=torch.int32)}

        def make(F, codes, nrm, b, lor):
            ix = eng.index_packed_dev(codes, F["K"], nrm, F["cb"], F["m"], base=b) if "nc" in F else eng.index_dev(codes, F["K"], nrm, F["m"], base=b)
            ix.set_lists(cent, lor)
            return ix

        for fname, F in formats.items():
            nrm = F["nc"] if "nc" in F else F["norms"]
            for with_base in (False, True):
                b = base if with_base else None
                for rname, ids in removals.items():
                    def tombstoned():
                        ix = make(F, F["codes"], nrm, b, assign)
                        ix.remove(ids)
                        torch.cuda.synchronize()
                        return ix

                    def run_compact(shrink=False):
                        with tombstoned() as ix:
                            ms, o = timed(lambda: ix.compact(shrink=shrink))
                            return ms, o, ix.compact_info()

                    def run_rebuild(o):
                        def f():
                            sel = o.long()
                            return make(F, F["codes"].index_select(0, sel), nrm.index_select(0, sel), None if b is None else b.index_select(0, sel),
                                        assign.index_select(0, sel))
                        ms, ix = timed(f)
                        ix.close()
                        return ms

                    _, o, _ = run_compact()                                    # warm-up: code objects, scratch
                    run_rebuild(o)
                    t_c, t_r = [], []
                    for _ in range(REPS):
                        t_c.append(run_compact()[0])
                        t_r.append(run_rebuild(o))
                    line = dict(bench="index_compact", format=fname, base="f32" if with_base else None, removal=rname, n=n, removed=int(ids.shape[0]), d=D, m=F["m"],
                                nlist=NLIST, reps=REPS, compact_ms=round(med(t_c), 3), compact_ms_min_max=[round(min(t_c), 3), round(max(t_c), 3)],
                                rebuild_ms=round(med(t_r), 3), rebuild_ms_min_max=[round(min(t_r), 3), round(max(t_r), 3)])
                    line["rebuild_over_compact"] = round(line["rebuild_ms"] / line["compact_ms"], 2)
                    line["compact_wins_beyond_rebuild_spread"] = bool(max(t_c) < min(t_r))
                    # (b) the phases and the gather's rate
                    eng.set_option("profile", 1)
                    ph = [run_compact()[2] for _ in range(REPS)]
                    eng.set_option("profile", 0)
                    n2 = n - int(ids.shape[0])
                    flat = n2 * (F["rowb"] + F["norm_bytes"] + (4 * D if with_base else 0))
                    line["gather_ms"], line["layout_ms"] = round(med(p["gather_ms"] for p in ph), 4), round(med(p["layout_ms"] for p in ph), 4)
                    line["moved_bytes"], line["gather_bytes"] = ph[0]["moved_bytes"], flat
                    cp = copy_ms(flat, dev)
                    line["gather_GBps"], line["copy_ms"], line["copy_GBps"] = round(2 * flat / line["gather_ms"] / 1e6, 1), round(cp, 4), round(2 * flat / cp / 1e6, 1)
                    line["gather_share_of_copy_rate"] = round(cp / line["gather_ms"], 3)
                    # (e) memory, in rounds of their own
                    for key, shrink in (("keep", False), ("shrink", True)):
                        with tombstoned() as ix:
                            bf, af, ex = watched(lambda: ix.compact(shrink=shrink, want_map=False))
                            line["resident_before_%s" % key], line["resident_after_%s" % key], line["resident_peak_sampled_over_before_%s" % key] = int(bf), int(af), int(ex)
                            line["capacity_rows_%s" % key] = ix.growth_info()["capacity_rows"]
                    # (c) the searches before, under the tombstones, after
                    if not with_base:
                        def searches(ix):
                            ix.search(Q, NN), ix.search_ivf(Q, NN, NPROBE)
                            return (round(med(timed(lambda: ix.search(Q, NN))[0] for _ in range(REPS)), 3),
                                    round(med(timed(lambda: ix.search_ivf(Q, NN, NPROBE))[0] for _ in range(REPS)), 3))
                        with make(F, F["codes"], nrm, None, assign) as ix:
                            line["search_ms_before"], line["search_ivf_ms_before"] = searches(ix)
                            ix.remove(ids)
                            line["search_ms_tombstoned"], line["search_ivf_ms_tombstoned"] = searches(ix)
                            line["filter_road_tombstoned"] = ix.filter_info()["road"]
                            ix.compact(want_map=False)
                            line["search_ms_compacted"], line["search_ivf_ms_compacted"] = searches(ix)
                    emit(line)
            # (d) remove beside the set_filter of the whole deny list
            held = removals["random n/10"]
            for more in (1, 1000, 100_000):
                extra = perm[n // 2: n // 2 + more].contiguous()
                deny = torch.cat([held, extra]).contiguous()
                t_rm, t_sf = [], []
                for r in range(REPS + 1):
                    with make(F, F["codes"], nrm, None, assign) as ix:
                        ix.remove(held)
                        torch.cuda.synchronize()
                        t_rm.append(timed(lambda: ix.remove(extra))[0])
                    with make(F, F["codes"], nrm, None, assign) as ix:
                        ix.set_filter(ids=held, deny=True)
                        torch.cuda.synchronize()
                        t_sf.append(timed(lambda: ix.set_filter(ids=deny, deny=True))[0])
                emit(dict(bench="index_compact", part="remove_vs_set_filter", format=fname, n=n, nlist=NLIST, removed_before=int(held.shape[0]), ids=more, reps=REPS,
                          remove_ms=round(med(t_rm[1:]), 4), set_filter_ms=round(med(t_sf[1:]), 4), set_filter_over_remove=round(med(t_sf[1:]) / med(t_rm[1:]), 2)))
        if nbig:                                                               # the rate point: bandwidth decides
            del base, codes8, norms, assign
            codes, nrm, lor = rows(nbig, 8)
            ids = torch.randperm(nbig, device=dev, generator=g)[: nbig // 10].int().contiguous()
            eng.set_option("profile", 1)
            ph, tot = [], []
            for _ in range(3):                                                 # the first round is the warm-up
                with eng.index_dev(codes, K8, nrm, 8) as ix:
                    ix.set_lists(cent, lor)
                    ix.remove(ids)
                    torch.cuda.synchronize()
                    tot.append(timed(lambda: ix.compact(want_map=False))[0])
                    ph.append(ix.compact_info())
            eng.set_option("profile", 0)
            flat = (nbig - nbig // 10) * 12
            gm, lm, cp = med(p["gather_ms"] for p in ph[1:]), med(p["layout_ms"] for p in ph[1:]), copy_ms(flat, dev)
            emit(dict(bench="index_compact", rate_point=True, format="plain-m8", base=None, removal="random n/10", n=nbig, nlist=NLIST, reps=2, compact_profiled_ms=round(med(tot[1:]), 3),
                      gather_ms=round(gm, 4), layout_ms=round(lm, 4), gather_bytes=flat, moved_bytes=ph[1]["moved_bytes"], gather_GBps=round(2 * flat / gm / 1e6, 1),
                      copy_ms=round(cp, 4), copy_GBps=round(2 * flat / cp / 1e6, 1), gather_share_of_copy_rate=round(cp / gm, 3),
                      layout_GBps=round(2 * (ph[1]["moved_bytes"] - flat) / lm / 1e6, 1)))
    out.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000, int(sys.argv[2]) if len(sys.argv) > 2 else 50_000_000)
