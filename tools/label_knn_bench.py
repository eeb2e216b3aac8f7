"""tools/label_knn_bench.py [n] -- labelled exact k-NN (lsq_index_knn_labelled, csrc/lsq_labelknn.hip) next to what the same resident index offers without it,
one JSON line per grid point, written to profiles/label_knn.jsonl and printed.  Without arguments: 10^6 x 128.

Data: tools/ivf_bench.py's Gaussian mixture, as f32 rows with f32 queries and as uint8 rows (8 x + 128, clamped) with uint8 queries.  Labels and predicates:
tools/label_bench.py's -- 32 independent random bits per row, a predicate fixes k randomly chosen bits, so it admits 2^-k of the rows: k = 0, 3, 7, 10 stand
for the fractions 1, 1/8, 1/128, 1/1024, and every query draws its own bits.

Roads, ALTERNATED in one process, device events around each call, REPS repeats, medians and min / max:
  labelled   knn(Q, nn, where=...) -- every query its own predicate
  unlabelled knn(Q, nn) of the same index (no predicate: another answer, the cost of the road the labelled one is modelled on)
  (c)        the only per-query road without this call: for each of 100 queries set_filter(its rows) + a one-query knn; the masks are made beforehand, not
             timed.  Reported per query, and times the number of queries as the figure the labelled call is held against (the gate, at 10^4 queries).
Each line carries the call's account (queries per block, blocks per query, compactions, skipped wave steps, scan and merge times) and the bytes of rows the
scan reads: query groups x n x (row bytes + 4 of label).

Then WHAT THE GROUND TRUTH IS FOR (bench = "label_recall"): recall@1 / 10 / 100 of search(where=) and search_ivf(where=) on an m = 8 LSQ index of the f32
rows (tools/label_bench.py's training) against the labelled knn of the same predicates, 10^3 queries, per fraction."""
import importlib, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
lsq = importlib.import_module("local-search-quantization_amd")
from ivf_bench import mixture, timed, D  # noqa: E402
REPS, LOOP_Q, NLIST, NPROBE, M = 5, 100, 1024, 16, 8


def spread(ts):
    return dict(ms=round(statistics.median(ts), 3), min_max=[round(min(ts), 3), round(max(ts), 3)])


def main(n):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    centres = 3.0 * torch.randn((2 * NLIST, D), device=dev, generator=g)
    X, Qall = mixture(g, dev, centres, n), mixture(g, dev, centres, 10_000)
    rng = np.random.default_rng(7)
    labels = torch.from_numpy(rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.int32)).to(dev)
    out = open(os.path.join(ROOT, "profiles", "label_knn.jsonl"), "w")

    def emit(line):
        s = json.dumps(line)
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    def predicates(k):
        bits = np.stack([rng.permutation(32)[:k] for _ in range(10_000)]).reshape(10_000, k)
        mask = (np.uint32(1) << bits.astype(np.uint32)).sum(1).astype(np.uint32) if k else np.zeros(10_000, np.uint32)
        want = mask & rng.integers(0, 2 ** 32, 10_000, dtype=np.uint64).astype(np.uint32)
        return tuple(torch.from_numpy(a.view(np.int32)).to(dev) for a in (mask, want))

    def to_u8(A):
        return (A * 8 + 128).round().clamp(0, 255).to(torch.uint8).contiguous()

    with lsq.Engine(0) as eng:
        for rows, base, Qfmt in (("f32", X, Qall), ("uint8", to_u8(X), to_u8(Qall))):
            with eng.index_dev(None, None, None, 0, base=base) as ix:
                ix.set_labels(labels)
                for nn in (100, 1000):
                    for k in (0, 3, 7, 10):
                        mask, want = predicates(k)
                        sets = [((labels & int(mask[q])) == int(want[q])).to(torch.uint8) for q in range(LOOP_Q)]
                        for nq in (10_000, 1000):
                            Q, where = Qfmt[:nq].contiguous(), (mask[:nq].contiguous(), want[:nq].contiguous())

                            def loop():
                                for q in range(LOOP_Q):
                                    ix.set_filter(mask=sets[q])
                                    ix.knn(Q[q:q + 1], nn)
                                ix.clear_filter()
                            ix.knn(Q, nn, where=where), ix.knn(Q, nn), loop()           # warm-up at full size
                            torch.cuda.synchronize()
                            t = dict(labelled=[], plain=[], c=[])
                            for _ in range(REPS):
                                t["labelled"].append(timed(lambda: ix.knn(Q, nn, where=where))[0])
                                t["plain"].append(timed(lambda: ix.knn(Q, nn))[0])
                                t["c"].append(timed(loop)[0] / LOOP_Q)
                            eng.set_option("profile", 1)
                            ix.knn(Q, nn, where=where)
                            info = ix.label_knn_info()
                            eng.set_option("profile", 0)
                            lab, c, groups = spread(t["labelled"]), spread(t["c"]), -(-nq // info["queries_per_block"])
                            emit(dict(bench="label_knn", rows=rows, n=n, d=D, nn=nn, nq=nq, fixed_bits=k, reps=REPS,
                                      allowed_fraction=round(info["allowed_pairs"] / (nq * n), 6), labelled=lab, unlabelled=spread(t["plain"]),
                                      ratio_to_unlabelled=round(lab["ms"] / statistics.median(t["plain"]), 2), c_per_query_loop=c, c_times_nq_ms=round(c["ms"] * nq, 1),
                                      gate_labelled_beats_c=bool(max(t["labelled"]) < min(t["c"]) * nq),
                                      queries_per_block=info["queries_per_block"], blocks_per_query=info["blocks_per_query"], lds_bytes=info["lds_bytes"],
                                      compactions=info["compactions"], offered=info["offered"], allowed_pairs=info["allowed_pairs"],
                                      skipped_wave_steps=info["skipped_wave_steps"], phases_ms=dict(scan_ms=round(info["scan_ms"], 3), merge_ms=round(info["merge_ms"], 3)),
                                      row_GB_read=round(groups * n * (D * base.element_size() + 4) / 1e9, 1),
                                      # (row, query, dimension) triples per second of the scan: 1.5 VALU lane-instructions each at QB >= 2
                                      scan_Gtriples_per_s=round(nq * n * D / max(info["scan_ms"], 1e-6) / 1e6, 1)))
        # ---- recall of the labelled searches against the new ground truth ------------------------------------------------------------------------------
        ntrain = min(n, 20_000)
        dK, _, _, _, _ = lsq.train_lsq_dev(X[:ntrain].contiguous(), M, 256, eng.randinit_dev(3, ntrain, M), 3, 2, 2, True, 4, seed=5, engine=eng, norm_codebook=False)
        dBs, _, _ = eng.encode_icm_dev(X, eng.randinit_dev(4, n, M), dK, M, [2], 2, 4, True, seed=6)
        codes = dBs[-1].contiguous()
        _, _, norms = eng.quantize_norms_dev(codes, dK, torch.zeros(1, dtype=torch.float32, device=dev), M)
        Xh = X.cpu().numpy()
        cent, _ = lsq.train_coarse(Xh[:min(n, 100_000)], NLIST, niter=5, seed=2, engine=eng)
        assign = lsq.ivf_assign(Xh, cent, engine=eng)
        with eng.index_dev(codes, dK, norms.contiguous(), M, base=X) as ix:
            ix.set_lists(torch.from_numpy(cent).to(dev), torch.from_numpy(assign).to(dev))
            ix.set_labels(labels)
            Q = Qall[:1000].contiguous()
            for k in (0, 3, 7, 10):
                mask, want = predicates(k)
                where = (mask[:1000].contiguous(), want[:1000].contiguous())
                gt = ix.knn(Q, 100, id_base=1, where=where)[1]
                line = dict(bench="label_recall", n=n, d=D, m=M, nq=1000, fixed_bits=k, nlist=NLIST, nprobe=NPROBE)
                for name, ids in (("search", ix.search(Q, 100, where=where)[1]), ("search_ivf", ix.search_ivf(Q, 100, NPROBE, where=where)[1])):
                    for r in (1, 10, 100):                              # recall@r: the share of the r true neighbours found among the first r answers
                        hit = (ids[:, :r, None] == gt[:, None, :r]) & (gt[:, None, :r] > 0)
                        line["%s_recall@%d" % (name, r)] = round(float(hit.any(1).sum() / max(int((gt[:, :r] > 0).sum()), 1)), 4)
                emit(line)
    out.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000)
