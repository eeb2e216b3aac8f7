"""tools/filter_bench.py [n nq] -- row filters on the resident index (lsq_index_set_filter): the unfiltered call, the DENSE road (every row read, the
filter's bit beside it) and the COMPACT road (the list of allowed rows walked) at allowed fractions 1, 1/2, 1/4, 1/16, 1/64, 1/256, 1/4096, one JSON line
per grid point, written to profiles/filter.jsonl and printed.  Without arguments: 10^4 queries x 10^6 codes x d = 128, m = 8, nn = 100.

Data and codebooks as tools/packed_bench.py builds them (synth_data_u8 rows, codebooks from train_lsq_dev on the first 100 000 rows, one encode of the whole
set).  Filters: seeded random masks (torch.rand(n) < fraction, seed 11), so the allowed rows are spread over the whole base.

Three calls: lsq_index_search (nq queries), lsq_index_knn on the f32 base rows (nq / 10 queries), lsq_index_search_ivf at nlist = 1024, nprobe = 16 and
fractions 1, 1/2, 1/16 (its threshold_queries / fallback_queries beside the times).  One process; a warm-up of every variant at full size; then the variants
of a grid point ALTERNATED, device events around each call, option "profile" off, REPS repeats, medians.  The dense and compact results are asserted equal
bit for bit at every point.  The last line is the crossover: the largest measured fraction at which the compact road is no slower than the dense one."""
import importlib, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lsq = importlib.import_module("local-search-quantization_amd")
REPS = 5
D, M, NN, NLIST, NPROBE = 128, 8, 100, 1024, 16
FRACTIONS = (1, 2, 4, 16, 64, 256, 4096)
IVF_FRACTIONS = (1, 2, 16)


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def same(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def main(n, nq):
    dev = torch.device("cuda:0")
    out = open(os.path.join(ROOT, "profiles", "filter.jsonl"), "w")

    def emit(line):
        s = json.dumps(line)
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    with lsq.Engine(0) as eng:
        X = eng.synth_data_u8_dev(1234, n, D)
        Q = eng.synth_data_u8_dev(777, nq, D)
        Qk = Q[:max(nq // 10, 1)].contiguous()
        Xh = X.cpu().numpy()
        cent, _ = lsq.train_coarse(Xh[:min(n, 100_000)], NLIST, niter=5, seed=2, engine=eng)
        assign = torch.from_numpy(lsq.ivf_assign(Xh, cent, engine=eng)).to(dev)
        dcent = torch.from_numpy(cent).to(dev)
        del Xh
        ns = min(n, 100_000)
        dK, _, _, _, _ = lsq.train_lsq_dev(X[:ns].contiguous(), M, 256, eng.randinit_dev(7, ns, M), 8, 4, 4, True, 4, seed=42, engine=eng, norm_codebook=False)
        dBs, _, _ = eng.encode_icm_dev(X, eng.randinit_dev(7, n, M), dK, M, [4], 4, 4, True, seed=42)
        codes = dBs[-1].contiguous()
        _, _, norms = eng.quantize_norms_dev(codes, dK, torch.zeros(1, dtype=torch.float32, device=dev), M)
        gen = torch.Generator(device=dev)
        gen.manual_seed(11)
        draw = torch.rand(n, device=dev, generator=gen)
        with eng.index_dev(codes, dK, norms.contiguous(), M, base=X) as ix:
            ix.set_lists(dcent, assign)
            calls = {"search": (lambda: ix.search(Q, NN), nq, FRACTIONS), "knn": (lambda: ix.knn(Qk, NN), Qk.shape[0], FRACTIONS),
                     "search_ivf": (lambda: ix.search_ivf(Q, NN, NPROBE), nq, IVF_FRACTIONS)}
            crossover = {}
            for name, (call, queries, fractions) in calls.items():
                ix.clear_filter()
                call()                                                         # warm-up at full size: code objects, work buffers
                for frac in fractions:
                    mask = draw < 1.0 / frac if frac > 1 else torch.ones(n, dtype=torch.bool, device=dev)
                    roads = ("dense",) if name == "search_ivf" else ("dense", "compact")      # the inverted layout has no compact form
                    for road in roads:
                        ix.set_filter(mask=mask, road=road)
                        call()
                    ix.clear_filter()
                    torch.cuda.synchronize()
                    line = dict(bench="filter", call=name, n=n, d=D, m=M, nq=queries, nn=NN, reps=REPS, fraction="1/%d" % frac)
                    results = {}
                    # alternated: unfiltered, dense, compact in every round
                    times = {k: [] for k in ("unfiltered",) + roads}
                    for _ in range(REPS):
                        for k in times:
                            if k == "unfiltered":
                                ix.clear_filter()
                            else:
                                ix.set_filter(mask=mask, road=k)
                            ms, results[k] = timed(call)
                            times[k].append(ms)
                            if k != "unfiltered" and name == "search_ivf":
                                info = ix.ivf_info()
                                line.update(threshold_queries=info["threshold_queries"], fallback_queries=info["fallback_queries"])
                    line["allowed"] = ix.filter_info()["allowed"]
                    for k, v in times.items():
                        line[k + "_ms"] = round(statistics.median(v), 3)
                        line[k + "_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]
                    line["dense_over_unfiltered"] = round(line["dense_ms"] / line["unfiltered_ms"], 4)
                    if "compact" in roads:
                        assert same(results["dense"], results["compact"]), (name, frac)
                        line["compact_over_unfiltered"] = round(line["compact_ms"] / line["unfiltered_ms"], 4)
                        line["fraction_times_unfiltered_ms"] = round(line["unfiltered_ms"] / frac, 3)
                        if line["compact_ms"] <= line["dense_ms"]:
                            crossover.setdefault(name, "1/%d" % frac)
                    if frac == 1:
                        assert same(results["dense"], results["unfiltered"]), name
                    if name == "search_ivf":
                        line.update(nlist=NLIST, nprobe=NPROBE)
                    emit(line)
            ix.clear_filter()
            emit(dict(bench="filter", summary="crossover", largest_fraction_where_compact_is_no_slower=crossover,
                      crossover_rows_of_this_build=ix.filter_info()["crossover_rows"], n=n))
    out.close()


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:3]] + [1_000_000, 10_000][len(sys.argv) - 1:]
    main(*a)
