"""tools/ivf_bench.py [n nlist] -- the inverted-list search (lsq_index_search_ivf, csrc/lsq_ivf.hip) next to the exhaustive scan of the SAME resident index
(lsq_index_search), one JSON line per grid point, written to profiles/ivf.jsonl and printed.  Without arguments: 10^6 x 128, m = 8, nlist = 1024.

Data: a Gaussian mixture generated here (2 nlist centres of scale 3, unit noise) -- uniform bytes have no coarse structure, every list would be as far as
every other.  Codebooks: train_lsq_dev on a prefix of 20 000 rows, then one encode of the whole set; dbnorms are the exact norms of the reconstructions.
Centroids: train_coarse on a prefix of 100 000 rows, every row assigned by ivf_assign.  Plain (non-residual) codes: q_coarse = q_scan.

Grid: nprobe in {1, 4, 16, 64}, nn in {100, 1000}, nq in {100, 10^4}.  One process; a warm-up of every call at full size; then the thresholded road, the
every-record road and the exhaustive scan ALTERNATED, device events around each call, option "profile" off, REPS repeats, medians.  The phase times
(coarse / lut / scan / select) and the records written come from a pass of its own with "profile" on, which waits on events inside the call.
recall_of_exhaustive: the share of the exhaustive scan's top-nn ids that the IVF result contains, averaged over the queries."""
import importlib, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lsq = importlib.import_module("local-search-quantization_amd")
REPS = 5
D, M = 128, 8


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


def main(n, nlist):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    centres = 3.0 * torch.randn((2 * nlist, D), device=dev, generator=g)
    X, Qall = mixture(g, dev, centres, n), mixture(g, dev, centres, 10_000)
    out = open(os.path.join(ROOT, "profiles", "ivf.jsonl"), "w")
    med = statistics.median
    with lsq.Engine(0) as eng:
        ntrain = min(n, 20_000)
        B0 = eng.randinit_dev(3, ntrain, M)
        dK, _, _, _, obj = lsq.train_lsq_dev(X[:ntrain].contiguous(), M, 256, B0, 3, 2, 2, True, 4, seed=5, engine=eng, norm_codebook=False)
        dBs, _, _ = eng.encode_icm_dev(X, eng.randinit_dev(4, n, M), dK, M, [2], 2, 4, True, seed=6)
        codes = dBs[-1].contiguous()
        _, _, norms = eng.quantize_norms_dev(codes, dK, torch.zeros(1, dtype=torch.float32, device=dev), M)
        Xh = X.cpu().numpy()
        cent, _ = lsq.train_coarse(Xh[:min(n, 100_000)], nlist, niter=5, seed=2, engine=eng)
        assign = lsq.ivf_assign(Xh, cent, engine=eng)
        sizes = np.bincount(assign, minlength=nlist)
        with eng.index_dev(codes, dK, norms.contiguous(), M) as ix:
            ix.set_lists(torch.from_numpy(cent).to(dev), torch.from_numpy(assign).to(dev))
            for nq in (100, 10_000):
                Q = Qall[:nq].contiguous()
                for nn in (100, 1000):
                    ed, ei = ix.search(Q, nn)                                   # warm-up of the exhaustive scan, and the recall's ground
                    truth = ei.cpu().numpy()
                    for nprobe in (1, 4, 16, 64):
                        if nprobe > nlist:
                            continue
                        for every in (False, True):
                            ix.search_ivf(Q, nn, nprobe, every_record=every)    # warm-up at full size: code objects, work buffers
                        torch.cuda.synchronize()
                        t_thr, t_all, t_exh = [], [], []
                        for _ in range(REPS):
                            t, (_, ids) = timed(lambda: ix.search_ivf(Q, nn, nprobe))
                            t_thr.append(t)
                            t, (_, ids_all) = timed(lambda: ix.search_ivf(Q, nn, nprobe, every_record=True))
                            t_all.append(t)
                            t, _ = timed(lambda: ix.search(Q, nn))
                            t_exh.append(t)
                        assert torch.equal(ids, ids_all)                        # the two roads agree
                        got = ids.cpu().numpy()
                        recall = float(np.mean([len(np.intersect1d(got[q], truth[q])) / nn for q in range(nq)]))
                        eng.set_option("profile", 1)
                        phases = {}
                        for every in (False, True):
                            ix.search_ivf(Q, nn, nprobe, every_record=every)
                            phases["every" if every else "thresholded"] = ix.ivf_info()
                        eng.set_option("profile", 0)
                        thr, al = phases["thresholded"], phases["every"]
                        line = dict(bench="ivf", n=n, d=D, m=M, nlist=nlist, nprobe=nprobe, nn=nn, nq=nq, reps=REPS,
                                    list_rows_min_median_max=[int(sizes.min()), int(np.median(sizes)), int(sizes.max())],
                                    ivf_ms=round(med(t_thr), 3), ivf_ms_min_max=[round(min(t_thr), 3), round(max(t_thr), 3)],
                                    ivf_every_record_ms=round(med(t_all), 3), exhaustive_ms=round(med(t_exh), 3),
                                    exhaustive_ms_min_max=[round(min(t_exh), 3), round(max(t_exh), 3)],
                                    speedup_over_exhaustive=round(med(t_exh) / med(t_thr), 3), recall_of_exhaustive=round(recall, 4),
                                    probed_rows_per_query=round(thr["probed_rows"] / nq, 1), records_per_query=round(thr["records"] / nq, 1),
                                    records_per_query_every_record=round(al["records"] / nq, 1), threshold_queries=thr["threshold_queries"],
                                    fallback_queries=thr["fallback_queries"], batches=thr["batches"], tail_capacity=thr["tail_capacity"],
                                    phases_ms={k: round(thr[k], 3) for k in ("coarse_ms", "lut_ms", "scan_ms", "select_ms")},
                                    phases_every_record_ms={k: round(al[k], 3) for k in ("coarse_ms", "lut_ms", "scan_ms", "select_ms")},
                                    # the list scan's LDS gathers: probed rows x m table reads of 4 bytes, over scan_ms
                                    scan_gather_Gps=round(thr["probed_rows"] * M / max(thr["scan_ms"], 1e-6) / 1e6, 1))
                        s = json.dumps(line)
                        print(s, flush=True)
                        out.write(s + "\n")
                        out.flush()
    out.close()


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:3]] + [1_000_000, 1024][len(sys.argv) - 1:]
    main(*a)
