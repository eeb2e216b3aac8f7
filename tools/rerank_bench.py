"""tools/rerank_bench.py [n nq d m L nn] -- the two-stage search on a resident index (lsq_index_*, csrc/lsq_rerank.hip): the ADC scan for a shortlist of L
(lsq_linscan_dev) against the exact re-rank of that shortlist to nn (gather + select), f32 and uint8 base rows, one JSON line each.
Without arguments: 10^4 queries x 10^6 synthetic rows, d = 128, m = 8, L = 1000, nn = 100.

The scan and the re-rank are timed in the same process, alternated, with device events around each call and the option "profile" off (warm-up first,
REPS repeats, the median).  The re-rank's split into gather_ms (the distance kernel) and select_ms (segmented sort + hand-out) comes from the index's own
events in a second pass with "profile" on, which waits on events inside the call and is therefore kept out of the comparison.
Byte model of the gather: nq L rows, each rounded up to whole 128-byte lines, over gather_ms; GATHER_TBS is the rate the microarchitecture guide measures
for random rows of 1 152 - 2 304 bytes gathered into registers (5.5 - 5.8 TB/s) -- rows of 512 and 128 bytes are not measured there, so the fraction is a
finding, not a target.  The one condition: the re-rank call (rerank_ms) takes no longer than the scan call that feeds it (scan_ms), both timed the same way."""
import importlib, json, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
lsq = importlib.import_module("local-search-quantization_amd")
GATHER_TBS = 5.5
REPS = 7


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def run(n, nq, d, m, L, nn, u8):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    base8 = torch.randint(0, 256, (n, d), dtype=torch.uint8, device=dev, generator=g)
    base = base8 if u8 else base8.float()
    Q = torch.randint(0, 256, (nq, d), device=dev, generator=g).float()
    codes = torch.randint(0, 256, (n, m), dtype=torch.uint8, device=dev, generator=g)
    K = torch.randn((m * 256, d), device=dev, generator=g)
    norms = torch.rand(n, device=dev, generator=g) * 1e4
    with lsq.Engine(0) as eng, eng.index_dev(codes, K, norms, m, base=base) as ix:
        for _ in range(2):                                                      # warm-up at full size: code objects, work buffers
            _, short = eng.linscan_dev(codes, Q, K, norms, m, L)
            ix.rerank(Q, short, nn)
            ix.search(Q, nn, shortlist=L)
        torch.cuda.synchronize()
        scan, rer, gather, select, both = [], [], [], [], []
        for _ in range(REPS):                                                   # alternated, "profile" off: no event waits inside either call
            t, (_, short) = timed(lambda: eng.linscan_dev(codes, Q, K, norms, m, L))
            scan.append(t)
            t, (dd, di) = timed(lambda: ix.rerank(Q, short, nn))
            rer.append(t)
            t, (sd, si) = timed(lambda: ix.search(Q, nn, shortlist=L))
            both.append(t)
        assert torch.equal(di, si) and torch.equal(dd.view(torch.int32), sd.view(torch.int32))      # the two roads give the same bits
        eng.set_option("profile", 1)                                            # a pass of its own for the split of the re-rank
        ix.rerank(Q, short, nn)
        for _ in range(REPS):
            s0 = ix.stats()
            ix.rerank(Q, short, nn)
            s1 = ix.stats()
            gather.append(s1["gather_ms"] - s0["gather_ms"])
            select.append(s1["select_ms"] - s0["select_ms"])
        batches = s1["batches"] - s0["batches"]
        st = ix.stats()
    med = statistics.median
    row_bytes = d * (1 if u8 else 4)
    lines = (row_bytes + 127) // 128 * 128
    gbytes = float(nq) * L * lines
    g_ms, s_ms = med(gather), med(select)
    rate = gbytes / (g_ms * 1e-3) / 1e12
    print(json.dumps(dict(bench="rerank", base="uint8" if u8 else "f32", n=n, nq=nq, d=d, m=m, L=L, nn=nn, reps=REPS,
                          scan_ms=round(med(scan), 3), scan_ms_min_max=[round(min(scan), 3), round(max(scan), 3)],
                          rerank_ms=round(med(rer), 3), rerank_ms_min_max=[round(min(rer), 3), round(max(rer), 3)],
                          gather_ms=round(g_ms, 3), select_ms=round(s_ms, 3), search_two_stage_ms=round(med(both), 3),
                          gathered_bytes=gbytes, row_bytes=row_bytes, gather_TBps=round(rate, 3), fraction_of_guide_gather_rate=round(rate / GATHER_TBS, 3),
                          rerank_no_longer_than_scan=bool(med(rer) <= med(scan)), invalid=st["invalid"], batches_per_call=batches)),
          flush=True)
    return med(rer) <= med(scan)


if __name__ == "__main__":
    shape = [int(x) for x in sys.argv[1:7]] + [1_000_000, 10_000, 128, 8, 1000, 100][len(sys.argv) - 1:]
    ok = [run(*shape, u8=u8) for u8 in (False, True)]
    sys.exit(0 if all(ok) else 1)
