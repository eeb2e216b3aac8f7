"""What 8-bit rows buy the encode: lsq_encode_icm_u8 / _u8_dev against lsq_encode_icm / _dev on the same 8-bit-valued data, in ONE process, the two element
types alternated call by call, warm-up excluded.

    python tools/u8_bench.py [--vectors 1000000] [--dim 128] [--reps 5] [--out profiles/encode_u8.jsonl] [--no-first-call]

Workload: n x d random bytes, m = 8 codebooks of sampled rows / m, 16 ILS iterations x 4 sweeps, npert = 4 (the benchmark's cfg2 shape by default).
Per element type one JSON line:
    host_steady_vps      vectors/s through host buffers (Engine.encode_icm: upload + encode + codes back), median of --reps calls on a warm context
    host_first_vps       the same for the FIRST call of a fresh process (a child process per element type: context creation excluded, everything else in)
    resident_vps         vectors/s of encode_icm_dev on device-resident X (median of --reps)
    profile_ms           the library's own event timings of one resident call with option "profile": unaries_ms = the unary GEMM (both outputs),
                         tables_ms = pair tables + level parameters (this is where the shift kernel and the sampled range pass are booked), cost_ms = the
                         cost / accept passes, icm_ms = the walks.  Per-kernel times want `rocprofv3 --kernel-trace --stats -- python tools/u8_bench.py --resident-only`.
    x_bytes_per_1e6      bytes of X resident per 10^6 vectors (from the shape: d x itemsize x 10^6) -- also what a host-buffer call uploads
Codes of the two element types are compared on every timed call: a faster call that encodes differently is not a result.
Host times: perf_counter around calls that end in a device synchronise (the host call returns the codes; the resident call is followed by torch.cuda.synchronize)."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lsq = importlib.import_module("local-search-quantization_amd")

M, H, ILS, J, NPERT, SEED = 8, 256, [16], 4, 4, 42


def problem(n, d):
    rng = np.random.default_rng(2026)
    X8 = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
    K = np.ascontiguousarray(X8[rng.choice(n, size=M * H, replace=n < M * H)].astype(np.float32) / np.float32(M))
    return X8, K, lsq.randinit_rows(n, M, H, seed=7)


def host_call(eng, X, K, B0):
    t = time.perf_counter()
    Bs, objs = eng.encode_icm(X, B0, K, M, ILS, J, NPERT, True, seed=SEED)
    return time.perf_counter() - t, Bs, objs


def first_call(elem, n, d):
    """child process: one host-buffer call on a fresh context"""
    X8, K, B0 = problem(n, d)
    X = X8 if elem == "u8" else X8.astype(np.float32)
    with lsq.Engine(0) as eng:
        dt, Bs, objs = host_call(eng, X, K, B0)
    print("U8_BENCH_FIRST " + json.dumps({"elem": elem, "seconds": dt, "obj": float(objs[-1]), "code_sum": int(Bs.astype(np.int64).sum())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-first-call", action="store_true")
    ap.add_argument("--resident-only", action="store_true", help="warm-up + --reps resident calls per element type and nothing else (for a kernel trace)")
    ap.add_argument("--first-call", choices=["f32", "u8"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    n, d = a.vectors, a.dim
    if a.first_call:
        return first_call(a.first_call, n, d)
    import torch
    assert torch.cuda.is_available(), "u8_bench needs a GPU: nothing here is a CPU number"
    X8, K, B0 = problem(n, d)
    Xs = {"f32": X8.astype(np.float32), "u8": X8}
    res = {e: {"elem": e, "n": n, "d": d, "m": M, "ils": ILS[0], "icmiter": J, "x_bytes_per_1e6": int(d * Xs[e].itemsize * 10**6)} for e in Xs}
    codes = {}
    with lsq.Engine(0) as eng:
        dK, dB0 = torch.from_numpy(K).cuda(), torch.from_numpy((B0 - 1).astype(np.uint8)).cuda()
        dX = {e: torch.from_numpy(Xs[e]).cuda() for e in Xs}

        def resident(e):
            torch.cuda.synchronize()
            t = time.perf_counter()
            dBs, sums, stats = eng.encode_icm_dev(dX[e], dB0, dK, M, ILS, J, NPERT, True, seed=SEED)
            torch.cuda.synchronize()
            return time.perf_counter() - t, dBs, sums

        for e in Xs:                                        # warm-up: code objects, work buffers of the shape
            codes[e] = resident(e)[1].cpu().numpy()
        assert np.array_equal(codes["f32"], codes["u8"]), "the two element types encode differently"
        times = {e: [] for e in Xs}
        for _ in range(a.reps):
            for e in Xs:
                dt, dBs, sums = resident(e)
                times[e].append(dt)
        for e in Xs:
            res[e]["resident_vps"] = n / statistics.median(times[e])
            res[e]["resident_s"] = sorted(times[e])
        if not a.resident_only:
            for e in Xs:
                dt, Bs, objs = host_call(eng, Xs[e], K, B0)      # warm-up: staging buffers, pinned staging of the runtime
                assert np.array_equal(Bs[-1].astype(np.int64) - 1, codes["f32"][-1]), "host call (%s) encodes differently" % e
            times = {e: [] for e in Xs}
            for _ in range(a.reps):
                for e in Xs:
                    times[e].append(host_call(eng, Xs[e], K, B0)[0])
            for e in Xs:
                res[e]["host_steady_vps"] = n / statistics.median(times[e])
                res[e]["host_steady_s"] = sorted(times[e])
    if not a.resident_only:
        with lsq.Engine(0, profile=True) as eng:                # the library's event timings, a run of their own
            for e in Xs:
                eng.encode_icm_dev(dX[e], dB0, dK, M, ILS, J, NPERT, True, seed=SEED)
            for e in Xs:
                torch.cuda.synchronize()
                eng.reset_timings()
                eng.encode_icm_dev(dX[e], dB0, dK, M, ILS, J, NPERT, True, seed=SEED)
                torch.cuda.synchronize()
                t = eng.timings()
                res[e]["profile_ms"] = {k: round(t[k], 4) for k in ("unaries_ms", "tables_ms", "cost_ms", "icm_ms", "other_ms")}
        if not a.no_first_call:
            for e in Xs:                                    # fresh processes, one after the other (the parent holds no context any more)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--first-call", e, "--vectors", str(n), "--dim", str(d)],
                                   capture_output=True, text=True, timeout=600)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("U8_BENCH_FIRST ")]
                if p.returncode != 0 or not line:
                    raise SystemExit("first-call child (%s) failed: %s" % (e, p.stderr[-800:]))
                f = json.loads(line[-1][len("U8_BENCH_FIRST "):])
                res[e]["host_first_vps"] = n / f["seconds"]
                res[e]["first_call_code_sum"] = f["code_sum"]
            assert res["f32"]["first_call_code_sum"] == res["u8"]["first_call_code_sum"]
    for e in Xs:
        line = json.dumps(res[e])
        print(line)
        if a.out:
            with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
