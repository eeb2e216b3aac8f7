"""tools/knn_exact_bench.py [n nq d k] -- exact k-NN on the device (lsq_knn_exact_dev, csrc/lsq_knn.hip) on Gaussian data: queries/s, the breakdown
(sample + thresholds / scan / selection), the scan's share of its VALU bound and, on a few queries, the host drop-in lsq_knn_exact_cpu as the CPU
figure and checker.  Without arguments: 10^4 queries x 10^6 base vectors at d = 128 and d = 960 with k in {1, 100, 1000}, one JSON line each.

VALU bound: three f32 element-ops (subtract, multiply, add) per (query, row, dimension), at 32 element-ops/clk/SIMD (packed f32), 4 SIMDs x 256 CUs,
2.4 GHz: 7.86e13 element-ops/s."""
import importlib, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
lsq = importlib.import_module("local-search-quantization_amd")
VALU_OPS_PER_S = 32 * 4 * 256 * 2.4e9


def run(n, nq, d, k, host_queries=16, host_threads=16):
    rng = np.random.default_rng(1)
    Xb = rng.standard_normal((n, d), dtype=np.float32)
    Xq = rng.standard_normal((nq, d), dtype=np.float32)
    dev = torch.device("cuda:0")
    dXb, dXq = torch.from_numpy(Xb).to(dev), torch.from_numpy(Xq).to(dev)
    with lsq.Engine(0, profile=True) as eng:
        eng.knn_exact_dev(dXb, dXq, k)                              # warm-up at full size (allocates the selection's work buffers)
        torch.cuda.synchronize()
        eng.reset_timings()
        reps = 3
        t0 = time.perf_counter()
        for _ in range(reps):
            dd, di = eng.knn_exact_dev(dXb, dXq, k)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        st = eng.linscan_stats()
    # host drop-in on a few queries: checker + CPU figure
    nh = min(nq, host_queries)
    hd = np.zeros((nh, k), np.float32)
    hi = np.zeros((nh, k), np.uint32)
    L = lsq._lib.load()
    t1 = time.perf_counter()
    lsq._lib.check(L.lsq_knn_exact_cpu(hd.ctypes.data, hi.ctypes.data, Xb.ctypes.data, Xq.ctypes.data, n, nh, d, d, d, k, host_threads))
    th = time.perf_counter() - t1
    same = bool(np.array_equal(hi, di[:nh].cpu().numpy().view(np.uint32)) and np.array_equal(hd.view(np.uint32), dd[:nh].cpu().numpy().view(np.uint32)))
    ops = 3.0 * n * nq * d
    bound_ms = ops / VALU_OPS_PER_S * 1e3
    bd = {key: round(st[key] / reps, 3) for key in ("lut_ms", "sample_ms", "scan_ms", "select_ms")}
    print(json.dumps(dict(search="knn_exact", n=n, nq=nq, d=d, k=k, ms=round(dt * 1e3, 3), queries_per_s=round(nq / dt, 1),
                          valu_bound_ms=round(bound_ms, 2), scan_fraction_of_bound=round(bound_ms / bd["scan_ms"], 3) if bd["scan_ms"] > 0 else None,
                          call_fraction_of_bound=round(bound_ms / (dt * 1e3), 3), breakdown_ms=bd,
                          candidates_per_query=round(st["candidates"] / max(st["queries"], 1), 1), fallback_queries=st["fallback_queries"],
                          threshold_rank=st["threshold_rank"], list_capacity=st["list_capacity"], batches=st["batches"] // reps,
                          exhaustive=st["exhaustive"],
                          host=dict(queries=nh, threads=host_threads, s=round(th, 3), queries_per_s=round(nh / th, 2), same_results=same),
                          device_over_host_per_query=round((th / nh) / (dt / nq), 1))),
          flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        run(*(int(x) for x in (sys.argv[1:5] + ["1000000", "10000", "128", "100"][len(sys.argv) - 1:])))
    else:
        for d in (128, 960):
            for k in (1, 100, 1000):
                run(1_000_000, 10_000, d, k)
