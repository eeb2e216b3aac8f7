"""tools/label_bench.py [n nlist] -- labelled search (lsq_index_search_labelled / _search_ivf_labelled, csrc/lsq_label.hip) next to what the same resident index
offers today, one JSON line per grid point, written to profiles/label_search.jsonl and printed.  Without arguments: 10^6 x 128, m = 8, nlist = 1024, nprobe = 16.

Data, codebooks, centroids: tools/ivf_bench.py's (a Gaussian mixture, train_lsq_dev on a prefix, one encode, train_coarse).  Labels: 32 independent random
bits per row; a predicate fixes k randomly chosen bits to random values, so it admits 2^-k of the rows: k = 0, 1, 3, 7, 10 stand for the fractions 1, 1/2,
~1/10, ~1/100, ~1/1000, and every query draws its own bits (at k = 1 there are only 64 different predicates).

Roads, ALTERNATED in one process, device events around each call, REPS repeats, medians and min / max:
  labelled   search(Q, nn, where=...) -- every query its own predicate
  (a)        the unfiltered search (lists: with option "ivf_select")
  (b)        set_filter of ONE set of the same fraction (not timed) + search: the best today's code does when all queries agree
  (c)        today's only per-query road: for each of 100 queries set_filter(its rows) + a one-query search; the masks are made beforehand, not timed.
             Reported per query, and times the number of queries as the figure the labelled call is held against (the gate).
Rows: m = 8 plain and m = 7 packed (the norm byte in the row).

Then, on the TUNING library (Engine(0, tuning=True)), WHAT QB BUYS: the exhaustive labelled call at 10^4 queries with the queries per block capped at 1, 2
and 4 by the knob LSQ_LABEL_QB (read at every call: the three geometries are alternated in one process), its time, its scan phase, and the bytes of rows
(code, norm, label) the call reads: query groups x n x bytes per row.  Lines with bench = "label_qb".  nn = 257 on packed rows is the rule's 4 -> 2 edge."""
import importlib, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
lsq = importlib.import_module("local-search-quantization_amd")
from ivf_bench import mixture, timed, D  # noqa: E402
REPS, LOOP_Q, NPROBE = 5, 100, 16


def spread(ts):
    return dict(ms=round(statistics.median(ts), 3), min_max=[round(min(ts), 3), round(max(ts), 3)])


def main(n, nlist):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    centres = 3.0 * torch.randn((2 * nlist, D), device=dev, generator=g)
    X, Qall = mixture(g, dev, centres, n), mixture(g, dev, centres, 10_000)
    rng = np.random.default_rng(7)
    labels = torch.from_numpy(rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.int32)).to(dev)
    out = open(os.path.join(ROOT, "profiles", "label_search.jsonl"), "w")

    def make_index(eng, m, packed):
        ntrain = min(n, 20_000)
        dK, _, _, _, _ = lsq.train_lsq_dev(X[:ntrain].contiguous(), m, 256, eng.randinit_dev(3, ntrain, m), 3, 2, 2, True, 4, seed=5, engine=eng, norm_codebook=False)
        dBs, _, _ = eng.encode_icm_dev(X, eng.randinit_dev(4, n, m), dK, m, [2], 2, 4, True, seed=6)
        codes = dBs[-1].contiguous()
        _, _, norms = eng.quantize_norms_dev(codes, dK, torch.zeros(1, dtype=torch.float32, device=dev), m)
        if not packed:
            return eng.index_dev(codes, dK, norms.contiguous(), m)
        cb = torch.sort(norms)[0][torch.linspace(0, n - 1, 256, device=dev).round().long()].contiguous()
        nc, _, _ = eng.quantize_norms_dev(codes, dK, cb, m)
        return eng.index_packed_dev(codes, dK, nc, cb, m)

    def predicates(k):
        bits = np.stack([rng.permutation(32)[:k] for _ in range(10_000)]).reshape(10_000, k)
        mask = (np.uint32(1) << bits.astype(np.uint32)).sum(1).astype(np.uint32) if k else np.zeros(10_000, np.uint32)
        want = mask & rng.integers(0, 2 ** 32, 10_000, dtype=np.uint64).astype(np.uint32)
        return mask, want

    eng = lsq.Engine(0)
    Xh = X.cpu().numpy()
    cent, _ = lsq.train_coarse(Xh[:min(n, 100_000)], nlist, niter=5, seed=2, engine=eng)
    assign = lsq.ivf_assign(Xh, cent, engine=eng)
    del Xh
    for M, packed in ((8, False), (7, True)):
        with make_index(eng, M, packed) as ix:
            ix.set_lists(torch.from_numpy(cent).to(dev), torch.from_numpy(assign).to(dev))
            ix.set_labels(labels)
            for road in ("exhaustive", "ivf"):
                eng.set_option("ivf_select", 1 if road == "ivf" else 0)
                plain = (lambda Q, nn, **kw: ix.search(Q, nn, **kw)) if road == "exhaustive" else (lambda Q, nn, **kw: ix.search_ivf(Q, nn, NPROBE, **kw))
                for nn in (100, 1000):
                    for k in (0, 1, 3, 7, 10):
                        mask, want = predicates(k)
                        dmask, dwant = (torch.from_numpy(a.view(np.int32)).to(dev) for a in (mask, want))
                        sets = [((labels & int(mask[q].view(np.int32))) == int(want[q].view(np.int32))).to(torch.uint8) for q in range(LOOP_Q)]
                        for nq in (10_000, 100):
                            Q, where = Qall[:nq].contiguous(), (dmask[:nq].contiguous(), dwant[:nq].contiguous())

                            def loop():
                                for q in range(LOOP_Q):
                                    ix.set_filter(mask=sets[q])
                                    plain(Q[q:q + 1], nn)
                                ix.clear_filter()
                            plain(Q, nn, where=where), plain(Q, nn), loop()          # warm-up at full size
                            torch.cuda.synchronize()
                            t = dict(labelled=[], a=[], b=[], c=[])
                            for _ in range(REPS):
                                t["labelled"].append(timed(lambda: plain(Q, nn, where=where))[0])
                                t["a"].append(timed(lambda: plain(Q, nn))[0])
                                ix.set_filter(mask=sets[0])
                                t["b"].append(timed(lambda: plain(Q, nn))[0])
                                ix.clear_filter()
                                if nq == 10_000:
                                    t["c"].append(timed(loop)[0] / LOOP_Q)
                            eng.set_option("profile", 1)
                            plain(Q, nn, where=where)
                            info = ix.label_info()
                            eng.set_option("profile", 0)
                            line = dict(bench="label_search", road=road, n=n, d=D, m=M, packed=int(packed), nn=nn, nq=nq, fixed_bits=k, reps=REPS,
                                        allowed_fraction=round(info["allowed_pairs"] / (nq * n), 6) if road == "exhaustive" else None,
                                        labelled=spread(t["labelled"]), a_unfiltered=spread(t["a"]), b_one_shared_filter=spread(t["b"]),
                                        queries_per_block=info["queries_per_block"], blocks_per_query=info["blocks_per_query"], compactions=info["compactions"],
                                        offered=info["offered"], allowed_pairs=info["allowed_pairs"],
                                        phases_ms={p: round(info[p], 3) for p in ("coarse_ms", "lut_ms", "scan_ms", "merge_ms")},
                                        # the scan's LDS gathers: (row, query) pairs that passed x m table reads of 4 bytes, over scan_ms
                                        scan_gather_Gps=round(info["allowed_pairs"] * M / max(info["scan_ms"], 1e-6) / 1e6, 1))
                            if t["c"]:
                                c = spread(t["c"])
                                line.update(c_per_query_loop=c, c_times_nq_ms=round(c["ms"] * nq, 1),
                                            gate_labelled_beats_c=bool(max(t["labelled"]) < min(t["c"]) * nq))
                            s = json.dumps(line)
                            print(s, flush=True)
                            out.write(s + "\n")
                            out.flush()
    eng.close()
    # ---- what QB buys: the tuning library, the knob alternated -------------------------------------------------------------------------------------------
    with lsq.Engine(0, tuning=True) as eng:
        Q = Qall.contiguous()
        for M, packed in ((8, False), (7, True)):
            row_bytes = (M + 1 if packed else M + 4) + 4                     # code (and norm byte) or code and f32 norm; the label
            with make_index(eng, M, packed) as ix:
                ix.set_labels(labels)
                for nn in (100, 257, 1000):
                    for k in (0, 3, 10):
                        mask, want = predicates(k)
                        where = tuple(torch.from_numpy(a.view(np.int32)).to(dev) for a in (mask, want))
                        t, info = {1: [], 2: [], 4: []}, {}
                        for cap in t:                                          # warm-up at full size
                            os.environ["LSQ_LABEL_QB"] = str(cap)
                            ix.search(Q, nn, where=where)
                        torch.cuda.synchronize()
                        for _ in range(REPS):
                            for cap in t:
                                os.environ["LSQ_LABEL_QB"] = str(cap)
                                t[cap].append(timed(lambda: ix.search(Q, nn, where=where))[0])
                        eng.set_option("profile", 1)
                        for cap in t:
                            os.environ["LSQ_LABEL_QB"] = str(cap)
                            ix.search(Q, nn, where=where)
                            info[cap] = ix.label_info()
                        eng.set_option("profile", 0)
                        del os.environ["LSQ_LABEL_QB"]
                        line = dict(bench="label_qb", n=n, d=D, m=M, packed=int(packed), nn=nn, nq=10_000, fixed_bits=k, reps=REPS,
                                    by_cap={str(cap): dict(queries_per_block=info[cap]["queries_per_block"], **spread(t[cap]), scan_ms=round(info[cap]["scan_ms"], 3),
                                                           row_GB_read=round(-(-10_000 // info[cap]["queries_per_block"]) * n * row_bytes / 1e9, 2))
                                            for cap in t})
                        s = json.dumps(line)
                        print(s, flush=True)
                        out.write(s + "\n")
                        out.flush()
    out.close()


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    main(a[0] if a else 1_000_000, a[1] if len(a) > 1 else 1024)
