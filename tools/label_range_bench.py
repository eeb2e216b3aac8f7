"""tools/label_range_bench.py [n nq [grid]] -- labelled range search (lsq_index_range_search_labelled, csrc/lsq_labelrange.hip) next to three yardsticks on
the SAME resident index in the same process, one JSON line per grid point, written to profiles/label_range.jsonl and printed.  Without arguments: 10^6 codes
x d = 128, 10^4 queries with 10^4 predicates; grid = "full" (every point) or "short" (plain rows, R = 100 only).

Data, codebooks, the two indexes (plain m = 8, packed m = 7) and the lists (nlist = 1024, nprobe = 16) as tools/range_bench.py builds them.  Labels: a
tenant word per row, uniform over T tenants, T = 1 / (allowed fraction) in {1, 8, 1024}; query q asks for tenant q mod T (mask = all ones).  Radius: the
distance of the query's R-th ALLOWED neighbour by search(where=, nn=R) on the same road (a tenant of fewer than R rows: +inf, every allowed row), R in
{10, 100, 1000}.

Yardsticks: (1) the per-query road -- set_filter(the query's tenant) and a one-query range_search --, timed on SAMPLE queries and scaled to nq; (2) the
unlabelled range_search with the same radii (it answers another question: every tenant's rows); (3) search(where=, nn=R).  One process; a warm-up of every
call at full size; then the calls ALTERNATED, device events around each, option "profile" off, REPS repeats, medians.  The phase times come from a pass of
its own with "profile" on."""
import importlib, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lsq = importlib.import_module("local-search-quantization_amd")
REPS, SAMPLE = 5, 8
CELLS = (1024, 2048, 4096, 8192)
D, NLIST, NPROBE = 128, 1024, 16


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


def cells_sweep(eng, ix, call, what):
    """the every-row call at each cell length in turn (LSQ_LABELRANGE_CELL, read at every call by the tuning library) -> one line"""
    times, phases = {c: [] for c in CELLS}, {}
    for rep in range(REPS + 1):                      # (the first round warms up)
        for c in CELLS:
            os.environ["LSQ_LABELRANGE_CELL"] = str(c)
            t = timed(call)[0]
            if rep:
                times[c].append(t)
    eng.set_option("profile", 1)
    for c in CELLS:
        os.environ["LSQ_LABELRANGE_CELL"] = str(c)
        call()
        li = ix.label_range_info()
        assert li["rows_per_cell"] == c
        phases[c] = dict(count_ms=round(li["count_ms"], 3), plan_ms=round(li["plan_ms"], 3), fill_ms=round(li["fill_ms"], 3), sort_ms=round(li["sort_ms"], 3),
                         skipped_share=round(li["fill_blocks_skipped"] / max(li["fill_blocks_launched"], 1), 4))
    eng.set_option("profile", 0)
    del os.environ["LSQ_LABELRANGE_CELL"]
    return dict(bench="label_range_cells", reps=REPS, call_ms={c: round(statistics.median(v), 3) for c, v in times.items()}, phases=phases, **what)


def main(n, nq, grid):
    dev = torch.device("cuda:0")
    out = open(os.path.join(ROOT, "profiles", "label_range_cells.jsonl" if grid == "cells" else "label_range.jsonl"), "w")

    def emit(line):
        s = json.dumps(line)
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    with lsq.Engine(0, tuning=(grid == "cells")) as eng:
        X = eng.synth_data_u8_dev(1234, n, D)
        Q = eng.synth_data_u8_dev(777, nq, D)
        Xh = X.cpu().numpy()
        cent, _ = lsq.train_coarse(Xh[:min(n, 100_000)], NLIST, niter=5, seed=2, engine=eng)
        assign = torch.from_numpy(lsq.ivf_assign(Xh, cent, engine=eng)).to(dev)
        dcent = torch.from_numpy(cent).to(dev)
        del Xh
        ones = torch.full((nq,), -1, dtype=torch.int32, device=dev)
        for m, packed in ((8, False), (7, True))[:2 if grid == "full" else 1]:
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
                for T in (1, 8, 1024):
                    labels = torch.from_numpy(np.random.default_rng(T).integers(0, T, n).astype(np.int32)).to(dev)
                    want = (torch.arange(nq, device=dev, dtype=torch.int32) % T).contiguous()
                    ix.set_labels(labels)
                    for R in ((10, 100, 1000) if grid == "full" else (100,)):
                        for kind, kw in (("scan", {}), ("ivf", dict(nprobe=NPROBE))):
                            if kind == "scan":
                                knn = lambda: ix.search(Q, R, where=(ones, want))                         # noqa: E731
                            else:
                                knn = lambda: ix.search_ivf(Q, R, NPROBE, where=(ones, want))             # noqa: E731
                            rad = knn()[0][:, R - 1].contiguous()
                            if grid == "cells":                                  # the cell length, alternated by the tuning library's knob
                                if kind == "scan":
                                    emit(cells_sweep(eng, ix, lambda: ix.range_search(Q, rad, where=(ones, want)), dict(n=n, m=m, nq=nq, allowed_fraction="1/%d" % T, results_asked=R)))
                                continue
                            calls = {"labelled": lambda: ix.range_search(Q, rad, where=(ones, want), **kw),
                                     "unlabelled": lambda: ix.range_search(Q, rad, **kw), "knn": knn}
                            for f in calls.values():                             # warm-up at full size: code objects, work buffers
                                f()
                            torch.cuda.synchronize()
                            ms, last = alternate(calls)
                            lims = last["labelled"][0]
                            eng.set_option("profile", 1)
                            calls["labelled"]()
                            li = ix.label_range_info()
                            calls["unlabelled"]()
                            ui = ix.range_info()
                            eng.set_option("profile", 0)

                            def one(q):                                          # the per-query road
                                ix.set_filter(mask=(labels == want[q]))
                                return ix.range_search(Q[q:q + 1], rad[q:q + 1], **kw)
                            one(0)
                            per = []
                            for _ in range(REPS):
                                per.append(sum(timed(lambda: one(q))[0] for q in range(min(SAMPLE, nq))) / min(SAMPLE, nq) * nq)
                            got = one(0)
                            ix.clear_filter()
                            assert torch.equal(got[1].view(torch.int32), last["labelled"][1][:lims[1]].view(torch.int32)) and torch.equal(got[2], last["labelled"][2][:lims[1]])
                            phases = {p: round(li[p], 3) for p in li if p.endswith("_ms")}
                            line = dict(bench="label_range", kind=kind, index="packed" if packed else "plain", n=n, d=D, m=m, nq=nq, allowed_fraction="1/%d" % T,
                                        results_asked=R, mean_results=round(float((lims[1:] - lims[:-1]).float().mean()), 2), reps=REPS,
                                        labelled_ms=ms["labelled"][0], labelled_ms_min_max=ms["labelled"][1], unlabelled_ms=ms["unlabelled"][0],
                                        unlabelled_ms_min_max=ms["unlabelled"][1], knn_where_ms=ms["knn"][0], knn_where_ms_min_max=ms["knn"][1],
                                        per_query_road_ms=round(statistics.median(per), 1), per_query_sample=min(SAMPLE, nq),
                                        per_query_over_labelled=round(statistics.median(per) / ms["labelled"][0], 1),
                                        labelled_over_unlabelled=round(ms["labelled"][0] / ms["unlabelled"][0], 3),
                                        labelled_over_knn_where=round(ms["labelled"][0] / ms["knn"][0], 3), phases_ms=phases,
                                        fill_over_count=round(li["fill_ms"] / max(li["count_ms"], 1e-9), 3),
                                        unlabelled_fill_over_count=round(ui["fill_ms"] / max(ui["count_ms"], 1e-9), 3),
                                        fill_blocks_launched=li["fill_blocks_launched"], fill_blocks_skipped=li["fill_blocks_skipped"],
                                        skipped_share=round(li["fill_blocks_skipped"] / max(li["fill_blocks_launched"], 1), 4),
                                        cells_per_query=li["cells_per_query"], rows_per_cell=li["rows_per_cell"], cells_nonempty=li["cells_nonempty"],
                                        cells=li["cells"], queries_per_block=li["queries_per_block"], allowed_pairs=li["allowed_pairs"], batches=li["batches"])
                            if kind == "ivf":
                                line.update(nlist=NLIST, nprobe=NPROBE)
                            emit(line)
            del codes, dBs, norms
    out.close()


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:3]] + [1_000_000, 10_000][len(sys.argv[1:3]):]
    main(*a, sys.argv[3] if len(sys.argv) > 3 else "full")
