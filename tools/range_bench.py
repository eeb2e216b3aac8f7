"""tools/range_bench.py [n nq] -- range search (lsq_index_range_search + lsq_index_range_fetch, csrc/lsq_range.hip) next to the k-NN search of the SAME
resident index in the same process (lsq_index_search / lsq_index_search_ivf with nn = the mean result count), one JSON line per grid point, written to
profiles/range.jsonl and printed.  Without arguments: 10^6 codes x d = 128, 10^4 and 100 queries.

Data and codebooks as tools/packed_bench.py builds them: synth_data_u8 rows (seed 1234), codebooks from train_lsq_dev on the first 100 000 rows, one encode
of the whole set.  Two indexes: plain m = 8 (8-byte rows and a float norm) and packed m = 7 (8-byte rows with the norm byte; the table: 256 evenly ranked
norms).  Lists: train_coarse on 100 000 rows, nlist = 1024, nprobe = 16.

Radii: per query the distance of its R-th neighbour by a search of the same index on the same road, R in {10, 100, 1000} -- so the mean result is R rows
(ties can add a few).  The yardstick is that search at nn = R: the parent's own scan, not the code under test.  One process; a warm-up of every call at full
size; then range and k-NN ALTERNATED, device events around each call, option "profile" off, REPS repeats, medians.  The phase times (coarse / lut / count /
fill / sort) come from a pass of its own with "profile" on, which waits on events inside the call.  Memory: held_bytes is the library's figure; the scratch
of the fill is computed from the shapes (two record buffers of 8 bytes per record of the largest batch, and the tables of the resident queries)."""
import importlib, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lsq = importlib.import_module("local-search-quantization_amd")
REPS = 5
D, NLIST, NPROBE = 128, 1024, 16
PHASES = ("coarse_ms", "lut_ms", "count_ms", "fill_ms", "sort_ms")


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def alternate(calls):
    """calls: name -> thunk; REPS rounds of every call in turn -> name -> (median ms, [min, max]), and the last results"""
    times, last = {k: [] for k in calls}, {}
    for _ in range(REPS):
        for k, f in calls.items():
            t, last[k] = timed(f)
            times[k].append(t)
    return {k: (round(statistics.median(v), 3), [round(min(v), 3), round(max(v), 3)]) for k, v in times.items()}, last


def main(n, nq_large):
    dev = torch.device("cuda:0")
    out = open(os.path.join(ROOT, "profiles", "range.jsonl"), "w")

    def emit(line):
        s = json.dumps(line)
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    with lsq.Engine(0) as eng:
        X = eng.synth_data_u8_dev(1234, n, D)
        Qall = eng.synth_data_u8_dev(777, nq_large, D)
        Xh = X.cpu().numpy()
        cent, _ = lsq.train_coarse(Xh[:min(n, 100_000)], NLIST, niter=5, seed=2, engine=eng)
        assign = torch.from_numpy(lsq.ivf_assign(Xh, cent, engine=eng)).to(dev)
        dcent = torch.from_numpy(cent).to(dev)
        del Xh
        for m, packed in ((8, False), (7, True)):
            ns = min(n, 100_000)
            dK, _, _, _, _ = lsq.train_lsq_dev(X[:ns].contiguous(), m, 256, eng.randinit_dev(7, ns, m), 4, 2, 4, True, 4, seed=42, engine=eng,
                                               norm_codebook=False)
            dBs, _, _ = eng.encode_icm_dev(X, eng.randinit_dev(7, n, m), dK, m, [4], 4, 4, True, seed=42)
            codes = dBs[-1].contiguous()
            _, _, norms = eng.quantize_norms_dev(codes, dK, torch.zeros(1, dtype=torch.float32, device=dev), m)
            if packed:
                cb = torch.sort(norms)[0][torch.linspace(0, n - 1, 256, device=dev).round().long()].contiguous()
                nc, _, _ = eng.quantize_norms_dev(codes, dK, cb, m)
                ix = eng.index_packed_dev(codes, dK, nc, cb, m)
            else:
                ix = eng.index_dev(codes, dK, norms.contiguous(), m)
            with ix:
                ix.set_lists(dcent, assign)
                for nq in sorted({nq_large, min(100, nq_large)}, reverse=True):
                    Q = Qall[:nq].contiguous()
                    for R in (10, 100, 1000):
                        if R > n:
                            continue
                        for kind in ("scan", "ivf"):
                            if kind == "scan":
                                knn = lambda: ix.search(Q, R)                                           # noqa: E731
                                rad = knn()[0][:, R - 1].contiguous()
                                rng = lambda: ix.range_search(Q, rad)                                   # noqa: E731
                            else:
                                knn = lambda: ix.search_ivf(Q, R, NPROBE)                               # noqa: E731
                                rad = knn()[0][:, R - 1].contiguous()
                                rng = lambda: ix.range_search(Q, rad, nprobe=NPROBE)                    # noqa: E731
                            calls = {"range": rng, "knn": knn}
                            for f in calls.values():                             # warm-up at full size: code objects, work buffers
                                f()
                            torch.cuda.synchronize()
                            ms, last = alternate(calls)
                            lims, rd, ri = last["range"]
                            kd, ki = last["knn"]
                            counts = (lims[1:] - lims[:-1])
                            # the k-NN answer is the head of every range result: the same bits
                            first = lims[:-1].unsqueeze(1) + torch.arange(R, device=dev).unsqueeze(0)
                            assert bool((counts >= R).all()) and torch.equal(ri[first], ki) and torch.equal(rd[first].view(torch.int32), kd.view(torch.int32))
                            eng.set_option("profile", 1)
                            rng()
                            info = ix.range_info()
                            knn()
                            kst = ix.scan_stats() if kind == "scan" else ix.ivf_info()
                            eng.set_option("profile", 0)
                            phases = {p: round(info[p], 3) for p in PHASES}
                            kphases = {p: round(kst[p], 3) for p in kst if p.endswith("_ms")}
                            walks = phases["count_ms"] + phases["fill_ms"]
                            line = dict(bench="range", kind=kind, index="packed" if packed else "plain", n=n, d=D, m=m, nq=nq, mean_results_asked=R,
                                        mean_results=round(float(counts.float().mean()), 2), max_per_query=info["max_per_query"], reps=REPS,
                                        range_ms=ms["range"][0], range_ms_min_max=ms["range"][1], knn_ms=ms["knn"][0], knn_ms_min_max=ms["knn"][1],
                                        range_over_knn=round(ms["range"][0] / ms["knn"][0], 4), phases_ms=phases, knn_phases_ms=kphases,
                                        dominant_phase=max(PHASES, key=lambda p: phases[p]),
                                        fill_share_of_call=round(phases["fill_ms"] / max(sum(phases.values()), 1e-9), 4),
                                        walks_over_knn_scan=round(walks / max(kst["scan_ms"], 1e-9), 3),
                                        rows_walked_per_query=round(info["rows_walked"] / nq, 1), batches=info["batches"], held_bytes=info["held_bytes"],
                                        fill_scratch_bytes=16 * info["results"], tables_bytes=nq * m * 1024)
                            if kind == "ivf":
                                line.update(nlist=NLIST, nprobe=NPROBE)
                            emit(line)
            del codes, dBs, norms
    out.close()


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:3]] + [1_000_000, 10_000][len(sys.argv) - 1:]
    main(*a)
