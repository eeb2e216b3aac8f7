"""tools/linscan_pq_bench.py [n nq d m knn] -- the device PQ / OPQ scan (lsq_linscan_pq_dev, csrc/lsq_adc.hip) on synthetic codes: queries/s,
table lookups/s, the breakdown (tables / sample + thresholds / scan / selection) and, on a few queries, the host drop-in lsq_linscan_aqd_query
as the CPU figure and checker.  Without arguments: the three shapes of DESIGN 4.6 (10^4 queries x 10^6 codes x 1000 neighbours at d = 128 with
m = 8 and m = 16, and at d = 960 with m = 8), one JSON line each."""
import importlib, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
lsq = importlib.import_module("local-search-quantization_amd")
H = 256


def run(n, nq, d, m, knn):
    subdim = d // m
    rng = np.random.default_rng(1)
    centers = rng.standard_normal((m, H, subdim)).astype(np.float32)
    codes = rng.integers(0, H, size=(n, m), dtype=np.uint8)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    dev = torch.device("cuda:0")
    dC, dQ, dK = torch.from_numpy(codes).to(dev), torch.from_numpy(Q).to(dev), torch.from_numpy(centers).to(dev)
    with lsq.Engine(0, profile=True) as eng:
        eng.linscan_pq_dev(dC, dQ, dK, m, knn, subdim)             # warm-up at full size (allocates the scan's work buffers)
        torch.cuda.synchronize()
        eng.reset_timings()
        reps = 3
        t0 = time.perf_counter()
        for _ in range(reps):
            dd, di = eng.linscan_pq_dev(dC, dQ, dK, m, knn, subdim)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        st = eng.linscan_stats()
    # host drop-in on a few queries: checker + CPU figure
    nh = min(nq, 16)
    hd = np.zeros((nh, knn), np.float32)
    hi = np.zeros((nh, knn), np.uint32)
    L = lsq._lib.load()
    t1 = time.perf_counter()
    lsq._lib.check(L.lsq_linscan_aqd_query(hd.ctypes.data, hi.ctypes.data, codes.ctypes.data, centers.ctypes.data, Q.ctypes.data, n, nh, 8 * m, knn,
                                           m, d, subdim))
    th = time.perf_counter() - t1
    same = bool(np.array_equal(hi, di[:nh].cpu().numpy().view(np.uint32)) and np.array_equal(hd.view(np.uint32), dd[:nh].cpu().numpy().view(np.uint32)))
    lookups = float(n) * nq * m
    print(json.dumps(dict(scan="pq", n=n, nq=nq, d=d, m=m, knn=knn, ms=round(dt * 1e3, 3), queries_per_s=round(nq / dt, 1), lookups_per_s=lookups / dt,
                          breakdown_ms={k: round(st[k] / reps, 3) for k in ("lut_ms", "sample_ms", "scan_ms", "select_ms")},
                          candidates_per_query=round(st["candidates"] / max(st["queries"], 1), 1), fallback_queries=st["fallback_queries"],
                          threshold_rank=st["threshold_rank"], list_capacity=st["list_capacity"], batches=st["batches"] // reps,
                          exhaustive=st["exhaustive"],
                          host_scan=dict(queries=nh, s=round(th, 3), queries_per_s=round(nh / th, 1), threads=min(nh, os.cpu_count()), same_results=same))),
          flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        run(*(int(x) for x in (sys.argv[1:6] + ["1000000", "10000", "128", "8", "1000"][len(sys.argv) - 1:])))
    else:
        for d, m in ((128, 8), (128, 16), (960, 8)):
            run(1_000_000, 10_000, d, m, 1000)
