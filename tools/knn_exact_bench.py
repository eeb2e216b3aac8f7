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

--prefilter [n nq] [--out PATH]: the MFMA pre-filter (option "knn_prefilter", csrc/lsq_knnm.hip) against the direct call, alternated in one process on one
resident base (Index.knn), device events, one warm-up, medians of 5: Gaussian rows at d = 128 and d = 960 as f32 and as f16, k in {1, 100, 1000}, and one
offset set (x + 1000, d = 128, f32, k = 100) whose norms dwarf its distances, to show what a switched-off call costs.  One JSON line per case, appended to
PATH (default profiles/knn_prefilter.jsonl): the ratio direct / pre-filtered, the MFMA pass as a fraction of its bound 2 nq n d / 157 TF, pending / kept, and
whether bits and ids equal the direct leg's.  Exit status 1 when they differ anywhere, or when on a Gaussian set the pre-filtered call is not faster than
the direct one by more than the spread of the direct leg's five repeats.

--prefilter --half [n nq] [--mfma-per-s R] [--out PATH]: the pre-filter's 16-bit tile (option "knn_prefilter_half", csrc/lsq_knnh.hip) on bf16 and f16 rows:
the direct call, the f32-tile pre-filter and the 16-bit tile alternated in one process on one resident base, medians of 5 with each leg's spread; d = 128 and
960, k in {1, 100, 1000}.  One JSON line per case appended to PATH (default profiles/knn_prefilter_half.jsonl): call times, split / norms / MFMA pass / recheck,
pending / kept of both tiles, the pass as a fraction of R = "chip_mfma_per_s" of tools/ubench_mfma_bf16.hip, bits and ids.  Exit status 1 when bits or ids
differ anywhere or the 16-bit tile was not served.

--u8 --mfma [n nq d] [--mfma-per-s R] [--dot4-lane-ops-per-s R] [--out PATH]: the third arm of --u8 -- the i8 matrix-core road (option "knn_u8_mfma",
csrc/lsq_knnu.hip) against the dot4 road on ONE resident uint8 index (Index.knn), calls alternated in one process, device events, option "profile" off, one
warm-up, medians of 5, k in {1, 100, 1000}; bits and ids compared on every case.  A separate pass with "profile" on records the phases (norms, sample +
scan, selection) of either road.  R: what tools/ubench_mfma_i8.hip printed as "chip_mfma_per_s" (the matrix-core pass is then given as a fraction of its
bound nq n ceil(d / 32) / 1024 / R) and tools/ubench_dot4.hip as "dot4_lane_ops_per_s".  One JSON line per k, appended to PATH (default
profiles/knn_u8_mfma.jsonl).  Exit status 1 when bits or ids differ anywhere; the ratio is reported, not judged.

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


def run_u8_mfma(n, nq, d, out_path, mfma_rate=None, dot4_rate=None, reps=5):
    rng = np.random.default_rng(1)
    dev = torch.device("cuda:0")
    d8 = torch.from_numpy(rng.integers(0, 256, (n, d), dtype=np.uint8)).to(dev)
    q8 = torch.from_numpy(rng.integers(0, 256, (nq, d), dtype=np.uint8)).to(dev)
    ok, lines = True, []
    with lsq.Engine(0) as eng, eng.index_dev(None, None, None, 0, base=d8) as ix:
        def leg(on, k):
            eng.set_option("knn_u8_mfma", on)
            return ix.knn(q8, k)
        for k in (1, 100, 1000):
            eng.set_option("profile", 0)
            ms, same = {0: [], 1: []}, True
            for r in range(reps + 1):                               # repeat 0 is the warm-up
                res = {}
                for on in (0, 1):
                    t, res[on] = _timed(lambda: leg(on, k))
                    if r > 0:
                        ms[on].append(t)
                same = same and torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32)) and torch.equal(res[0][1], res[1][1])
            eng.set_option("profile", 1)                            # the phases, apart from the timed calls
            ph = {}
            for on in (0, 1):
                leg(on, k)
                ph[on] = (ix.knn_info(), ix.knn_mfma_info())
            med = {on: float(np.median(v)) for on, v in ms.items()}
            spread = {on: max(v) - min(v) for on, v in ms.items()}
            mf = ph[1][1]
            ok = ok and same and mf["served"] == 1 and ph[1][0]["fallback_queries"] == ph[0][0]["fallback_queries"]
            mfma_bound = nq * n * ((d + 31) // 32) / 1024.0 / mfma_rate * 1e3 if mfma_rate else None
            dot4_bound = (nq * n * d / 4.0) / dot4_rate * 1e3 if dot4_rate else None
            lines.append(json.dumps(dict(
                search="knn_u8_mfma", n=n, nq=nq, d=d, k=k, reps=reps, dot4_ms=round(med[0], 3), mfma_ms=round(med[1], 3), dot4_spread_ms=round(spread[0], 3),
                mfma_spread_ms=round(spread[1], 3), dot4_over_mfma=round(med[0] / med[1], 3), faster_beyond_spread=bool(med[0] - med[1] > max(spread.values())),
                same_bits_and_ids=bool(same), served=mf["served"], pairs=mf["pairs"], kept=mf["kept"], fallback_queries=ph[1][0]["fallback_queries"],
                dot4_phases_ms=dict(norms=round(ph[0][0]["norms_ms"], 3), sample_and_scan=round(ph[0][0]["scan_ms"], 3), select=round(ph[0][0]["select_ms"], 3)),
                mfma_phases_ms=dict(norms=round(ph[1][0]["norms_ms"], 3), shifted_norms=round(mf["norms_ms"], 3), sample_and_scan=round(ph[1][0]["scan_ms"], 3),
                                    mfma_pass=round(mf["scan_ms"], 3), select=round(ph[1][0]["select_ms"], 3)),
                mfma_bound_ms=round(mfma_bound, 3) if mfma_bound else None,
                mfma_pass_fraction_of_ubench_rate=round(mfma_bound / mf["scan_ms"], 3) if mfma_bound and mf["scan_ms"] > 0 else None,
                dot4_bound_ms=round(dot4_bound, 3) if dot4_bound else None,
                dot4_scan_fraction_of_ubench_rate=round(dot4_bound / ph[0][0]["scan_ms"], 3) if dot4_bound and ph[0][0]["scan_ms"] > 0 else None)))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
    return ok


MFMA_FLOPS = 157e12                          # f32 matrix-core peak


def run_prefilter(n, nq, out_path, reps=5):
    dev = torch.device("cuda:0")
    ok = True
    lines = []
    for d, fmt, offset, ks in [(128, "f32", 0, (1, 100, 1000)), (128, "f16", 0, (1, 100, 1000)), (960, "f32", 0, (1, 100, 1000)),
                               (960, "f16", 0, (1, 100, 1000)), (128, "f32", 1000, (100,))]:
        g = torch.Generator(device=dev).manual_seed(2700 + d)
        rows = torch.randn((n, d), generator=g, device=dev) + offset
        Q = torch.randn((nq, d), generator=g, device=dev) + offset
        if fmt == "f16":
            rows = rows.half()
        with lsq.Engine(0, profile=True) as eng, eng.index_dev(None, None, None, 0, base=rows) as ix:
            def leg(pre, k):
                eng.set_option("knn_prefilter", pre)
                return ix.knn(Q, k)
            for k in ks:
                ms, acct = {0: [], 1: []}, {}
                same = True
                for r in range(reps + 1):                           # repeat 0 is the warm-up
                    res = {}
                    for pre in (0, 1):
                        t, res[pre] = _timed(lambda: leg(pre, k))
                        if r > 0:
                            ms[pre].append(t)
                        acct[pre] = (ix.knn_info(), ix.knn_prefilter_info())
                    same = same and torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32)) and torch.equal(res[0][1], res[1][1])
                med = {pre: float(np.median(v)) for pre, v in ms.items()}
                spread = max(ms[0]) - min(ms[0])
                faster = med[0] - med[1] > spread
                ok = ok and same and (faster or offset != 0)
                pf = acct[1][1]
                bound_ms = 2.0 * nq * n * d / MFMA_FLOPS * 1e3
                lines.append(json.dumps(dict(
                    search="knn_prefilter", n=n, nq=nq, d=d, k=k, rows=fmt, offset=offset, reps=reps, direct_ms=round(med[0], 3), prefilter_ms=round(med[1], 3),
                    direct_spread_ms=round(spread, 3), direct_over_prefilter=round(med[0] / med[1], 3), faster_beyond_spread=faster, same_bits_and_ids=same,
                    direct_scan_ms=round(acct[0][0]["scan_ms"], 3), prefilter_scan_ms=round(acct[1][0]["scan_ms"], 3), norms_ms=round(pf["norms_ms"], 3),
                    mfma_ms=round(pf["mfma_ms"], 3), recheck_ms=round(pf["recheck_ms"], 3), mfma_bound_ms=round(bound_ms, 3),
                    mfma_fraction_of_bound=round(bound_ms / pf["mfma_ms"], 3) if pf["mfma_ms"] > 0 else None, pairs=pf["pairs"], pending=pf["pending"],
                    kept=pf["kept"], pending_over_kept=round(pf["pending"] / pf["kept"], 4) if pf["kept"] else None, overflow_queries=pf["overflow_queries"],
                    switched_off=pf["switched_off"], served=pf["served"], kappa=pf["kappa"], fallback_queries=acct[1][0]["fallback_queries"])))
                print(lines[-1], flush=True)
        del rows, Q
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
    return ok


def run_prefilter_half(n, nq, out_path, mfma_per_s, reps=5):
    """--prefilter --half: on f16 and bf16 rows, the direct call, the f32-tile pre-filter (4.29) and the 16-bit tile (4.31) alternated on one index"""
    dev = torch.device("cuda:0")
    ok, lines = True, []
    legs = {"direct": (0, 0), "f32_tile": (1, 0), "half_tile": (1, 1)}
    for d in (128, 960):
        for fmt in ("bf16", "f16"):
            g = torch.Generator(device=dev).manual_seed(2900 + d)
            rows = torch.randn((n, d), generator=g, device=dev).to(torch.float16 if fmt == "f16" else torch.bfloat16)
            Q = torch.randn((nq, d), generator=g, device=dev)
            with lsq.Engine(0, profile=True) as eng, eng.index_dev(None, None, None, 0, base=rows) as ix:
                def leg(name, k):
                    eng.set_option("knn_prefilter", legs[name][0])
                    eng.set_option("knn_prefilter_half", legs[name][1])
                    return ix.knn(Q, k)
                for k in (1, 100, 1000):
                    ms, acct, same = {name: [] for name in legs}, {}, True
                    for r in range(reps + 1):                       # repeat 0 is the warm-up
                        res = {}
                        for name in legs:
                            t, res[name] = _timed(lambda: leg(name, k))
                            if r > 0:
                                ms[name].append(t)
                            acct[name] = (ix.knn_info(), ix.knn_prefilter_info(), ix.knn_prefilter_half_info())
                        for name in ("f32_tile", "half_tile"):
                            same = same and torch.equal(res["direct"][0].view(torch.int32), res[name][0].view(torch.int32)) and torch.equal(res["direct"][1], res[name][1])
                    med = {name: float(np.median(v)) for name, v in ms.items()}
                    spread = {name: max(v) - min(v) for name, v in ms.items()}
                    hi, pf = acct["half_tile"][2], acct["f32_tile"][1]
                    mfmas = hi["pieces"] * nq * n * ((d + 15) // 16) / 1024.0       # 32 x 32 x 16 instructions of the pass
                    bound_ms = mfmas / mfma_per_s * 1e3 if mfma_per_s else None
                    ok = ok and same and hi["served"] == 1
                    lines.append(json.dumps(dict(
                        search="knn_prefilter_half", n=n, nq=nq, d=d, k=k, rows=fmt, reps=reps, direct_ms=round(med["direct"], 3),
                        f32_tile_ms=round(med["f32_tile"], 3), half_tile_ms=round(med["half_tile"], 3), spread_ms={a: round(b, 3) for a, b in spread.items()},
                        f32_tile_over_half_tile=round(med["f32_tile"] / med["half_tile"], 3),
                        faster_beyond_spread=bool(med["f32_tile"] - med["half_tile"] > max(spread["f32_tile"], spread["half_tile"])), same_bits_and_ids=same,
                        norms_ms=round(acct["half_tile"][1]["norms_ms"], 3), split_ms=round(hi["split_ms"], 3), scan_ms=round(hi["scan_ms"], 3),
                        recheck_ms=round(hi["recheck_ms"], 3), f32_tile_mfma_ms=round(pf["mfma_ms"], 3), f32_tile_recheck_ms=round(pf["recheck_ms"], 3),
                        scan_bound_ms=round(bound_ms, 3) if bound_ms else None,
                        scan_fraction_of_measured_mfma_rate=round(bound_ms / hi["scan_ms"], 3) if bound_ms and hi["scan_ms"] > 0 else None,
                        pieces=hi["pieces"], pairs=hi["pairs"], pending=hi["pending"], kept=hi["kept"],
                        pending_over_kept=round(hi["pending"] / hi["kept"], 4) if hi["kept"] else None,
                        f32_tile_pending_over_kept=round(pf["pending"] / pf["kept"], 4) if pf["kept"] else None, overflow_queries=hi["overflow_queries"],
                        switched_off=hi["switched_off"], served=hi["served"], kappa=hi["kappa"], eta=hi["eta"])))
                    print(lines[-1], flush=True)
            del rows, Q
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
    return ok


if __name__ == "__main__":
    if "--prefilter" in sys.argv[1:] and "--half" in sys.argv[1:]:
        # --prefilter --half [n nq] [--mfma-per-s R] [--out PATH]: R = chip_mfma_per_s of tools/ubench_mfma_bf16.hip (the pass's share of that rate is reported)
        args = [a for a in sys.argv[1:] if a not in ("--prefilter", "--half")]
        opts = {"--out": os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "knn_prefilter_half.jsonl"), "--mfma-per-s": "0"}
        for flag in list(opts):
            if flag in args:
                i = args.index(flag)
                opts[flag] = args[i + 1]
                del args[i:i + 2]
        sys.exit(0 if run_prefilter_half(*(int(x) for x in (args[:2] + ["1000000", "10000"][len(args):])), out_path=opts["--out"],
                                         mfma_per_s=float(opts["--mfma-per-s"])) else 1)
    if "--prefilter" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--prefilter"]
        out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "knn_prefilter.jsonl")
        if "--out" in args:
            i = args.index("--out")
            out = args[i + 1]
            del args[i:i + 2]
        sys.exit(0 if run_prefilter(*(int(x) for x in (args[:2] + ["1000000", "10000"][len(args):])), out_path=out) else 1)
    if "--u8" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--u8"]
        rate, opts = None, {}
        for flag in ("--dot4-lane-ops-per-s", "--mfma-per-s", "--out"):
            if flag in args:
                i = args.index(flag)
                opts[flag] = args[i + 1]
                del args[i:i + 2]
        rate = float(opts["--dot4-lane-ops-per-s"]) if "--dot4-lane-ops-per-s" in opts else None
        if "--mfma" in args:
            args.remove("--mfma")
            out = opts.get("--out", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "knn_u8_mfma.jsonl"))
            mrate = float(opts["--mfma-per-s"]) if "--mfma-per-s" in opts else None
            sys.exit(0 if run_u8_mfma(*(int(x) for x in (args[:3] + ["1000000", "10000", "128"][len(args):])), out_path=out, mfma_rate=mrate, dot4_rate=rate) else 1)
        sys.exit(0 if run_u8(*(int(x) for x in (args[:3] + ["1000000", "10000", "128"][len(args):])), dot4_rate=rate) else 1)
    if len(sys.argv) > 1:
        run(*(int(x) for x in (sys.argv[1:5] + ["1000000", "10000", "128", "100"][len(sys.argv) - 1:])))
    else:
        for d in (128, 960):
            for k in (1, 100, 1000):
                run(1_000_000, 10_000, d, k)
