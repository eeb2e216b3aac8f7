"""tools/knn_exact_bench.py [n nq d k] -- exact k-NN on the device (lsq_knn_exact_dev, csrc/lsq_knn.hip) on Gaussian data: queries/s, the breakdown
(sample + thresholds / scan / selection), the scan's share of its VALU bound and, on a few queries, the host drop-in lsq_knn_exact_cpu as the CPU
figure and checker.  Without arguments: 10^4 queries x 10^6 base vectors at d = 128 and d = 960 with k in {1, 100, 1000}, one JSON line each.

--u8 [n nq d] [--dot4-lane-ops-per-s R]: an 8-bit base and 8-bit queries, three legs alternated in one process and timed with device events (one warm-up
each, medians of 5 repeats), k in {1, 100, 1000}:
    (a) knn_exact_dev on the base widened to f32 (the f32 road);  (b) Index.knn on the resident uint8 base with option knn_u8_int = 0 (the same kernel,
    bytes widened in registers);  (c) Index.knn on the integer road (v_dot4_u32_u8).
Every leg's result is compared with (a)'s, bits and ids.  Exit status 1 when (c) is slower than (a), or (b) slower than (a) by more than the spread of
(a)'s own repeats.  R: the dot4 lane-op rate tools/ubench_dot4.hip printed ("dot4_lane_ops_per_s"); with it (c)'s scan is given as a fraction of the bound
nq n d / 4 / R.

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


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def run_u8(n, nq, d, dot4_rate=None, reps=5):
    rng = np.random.default_rng(1)
    dev = torch.device("cuda:0")
    d8 = torch.from_numpy(rng.integers(0, 256, (n, d), dtype=np.uint8)).to(dev)
    q8 = torch.from_numpy(rng.integers(0, 256, (nq, d), dtype=np.uint8)).to(dev)
    df, qf = d8.float(), q8.float()
    ok = True
    with lsq.Engine(0, profile=True) as eng, eng.index_dev(None, None, None, 0, base=d8) as ix:
        def widened(k):
            eng.set_option("knn_u8_int", 0)
            try:
                return ix.knn(q8, k)
            finally:
                eng.set_option("knn_u8_int", 1)
        for k in (1, 100, 1000):
            legs = {"a": lambda: eng.knn_exact_dev(df, qf, k), "b": lambda: widened(k), "c": lambda: ix.knn(q8, k)}
            ms = {name: [] for name in legs}
            info = {}
            ref = None
            for rep in range(reps + 1):                             # repeat 0 is the warm-up
                for name, fn in legs.items():
                    t, (dd, di) = _timed(fn)
                    if rep == 0:
                        ref = (dd, di) if name == "a" else ref
                        same = torch.equal(dd.view(torch.int32), ref[0].view(torch.int32)) and torch.equal(di, ref[1])
                        info[name + "_same_as_a"] = bool(same)
                        ok = ok and same
                    else:
                        ms[name].append(t)
                    if name == "c":
                        ci = ix.knn_info()
            med = {name: float(np.median(v)) for name, v in ms.items()}
            spread_a = max(ms["a"]) - min(ms["a"])
            c_ok, b_ok = med["c"] <= med["a"], med["b"] <= med["a"] + spread_a
            ok = ok and c_ok and b_ok and ci["int_road"] == 1
            bound_ms = (nq * n * d / 4.0) / dot4_rate * 1e3 if dot4_rate else None
            print(json.dumps(dict(search="knn_exact_u8", n=n, nq=nq, d=d, k=k, reps=reps, a_f32_ms=round(med["a"], 3), b_widened_ms=round(med["b"], 3),
                                  c_integer_ms=round(med["c"], 3), a_spread_ms=round(spread_a, 3), a_over_c=round(med["a"] / med["c"], 3),
                                  a_over_b=round(med["a"] / med["b"], 3), c_not_slower_than_a=c_ok, b_within_a_spread=b_ok,
                                  norms_ms=round(ci["norms_ms"], 3), c_scan_ms=round(ci["scan_ms"], 3), c_select_ms=round(ci["select_ms"], 3),
                                  fallback_queries=ci["fallback_queries"], int_road=ci["int_road"],
                                  resident_bytes=dict(a=n * d * 4, b=n * d, c=n * d + 4 * n),
                                  dot4_bound_ms=round(bound_ms, 3) if bound_ms else None,
                                  c_scan_fraction_of_dot4_bound=round(bound_ms / ci["scan_ms"], 3) if bound_ms and ci["scan_ms"] > 0 else None, **info)),
                  flush=True)
    return ok


if __name__ == "__main__":
    if "--u8" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--u8"]
        rate = None
        if "--dot4-lane-ops-per-s" in args:
            i = args.index("--dot4-lane-ops-per-s")
            rate = float(args[i + 1])
            del args[i:i + 2]
        sys.exit(0 if run_u8(*(int(x) for x in (args[:3] + ["1000000", "10000", "128"][len(args):])), dot4_rate=rate) else 1)
    if len(sys.argv) > 1:
        run(*(int(x) for x in (sys.argv[1:5] + ["1000000", "10000", "128", "100"][len(sys.argv) - 1:])))
    else:
        for d in (128, 960):
            for k in (1, 100, 1000):
                run(1_000_000, 10_000, d, k)
