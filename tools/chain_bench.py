"""Times the structured (ChainQ) codebook update and the ChainQ trainer on the device; one JSON line per measurement.

    python tools/chain_bench.py update  [--shapes demo,1e5,d960] [--repeat 5] [--out profiles/chain_update.jsonl]
    python tools/chain_bench.py train   [--shapes demo,1e5] [--niter 10] [--out ...]
    python tools/chain_bench.py calls   [--shapes 1e5]                      # a few structured + unstructured calls, to be run under rocprofv3
    python tools/chain_bench.py passes  --stats <kernel_stats.csv> [--shapes 1e5] [--out ...]      # bytes from shapes over the traced kernel times

update: per shape one process, a warm-up of every variant, then the structured (lsq_update_codebooks_struct_dev) and the unstructured
(lsq_update_codebooks_dev) device update ALTERNATED `repeat` times (host clock around a synchronise); the scipy path of update_codebooks_chain
(what train_chainq runs by default) and solver="host" on 16 threads once each.  Data: chain-consistent (random codes, true codebooks inside the
chain's dimensions, noise 0.05), seeded.  The two device solvers stop after different counts, so they are compared PER ITERATION; the margin is the
spread of the unstructured figure over the repeats.
train: train_chainq (default path) against train_chainq_dev on SIFT-like data with OPQ's codes (one OPQ iteration): wall time and the share
of it inside the codebook update.
Bytes of one iteration, from shapes (P = covered (codebook, dimension) pairs, 2 d for a chain, m d unstructured):
    row pass     8 n d (U read and written) + 4 n P (V gathers) + n m (codes)
    column pass  4 n P (U through the sorted rows) + 8 n m ceil(longest list / 64) (the keys, once per wave of a column)"""
import argparse
import csv
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lsq = importlib.import_module("local-search-quantization_amd")
ini = importlib.import_module("local-search-quantization_amd.initializers")

H = 256
SHAPES = {"demo": (10_000, 128, 7), "1e5": (100_000, 128, 8), "d960": (100_000, 960, 8), "tiny": (2_000, 16, 4)}
HBM_PEAK = 8e12


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def chain_problem(n, d, m, seed=1):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, H, size=(n, m)).astype(np.uint8)
    od = ini.get_cbdims_chain(d, m)
    K = np.zeros((m * H, d), dtype=np.float32)
    for i in range(m):
        K[i * H:(i + 1) * H, od[i]] = rng.standard_normal((H, od[i].stop - od[i].start)).astype(np.float32)
    X = np.zeros((n, d), dtype=np.float32)
    for j in range(m):
        X += K[j * H + codes[:, j].astype(np.int64)]
    X += (0.05 * rng.standard_normal((n, d))).astype(np.float32)
    return X, codes, ini._cover_map(od, d, m)


def pass_bytes(n, d, m, dim2C):
    """(row pass, column pass) bytes of one iteration; dim2C None = unstructured"""
    P = m * d if dim2C is None else int(dim2C.sum())
    longest = d if dim2C is None else int(dim2C.sum(0).max())
    return 8 * n * d + 4 * n * P + n * m, 4 * n * P + 8 * n * m * -(-longest // 64)


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def mode_update(a):
    import torch
    eng = lsq.Engine(0)
    for name in a.shapes.split(","):
        n, d, m = SHAPES[name]
        X, codes, dim2C = chain_problem(n, d, m)
        dX, dB, dC = torch.from_numpy(X).cuda(), torch.from_numpy(codes).cuda(), torch.from_numpy(dim2C).cuda()
        out = torch.empty((m * H, d), dtype=torch.float32, device=dX.device)
        struct = lambda: eng.update_codebooks_struct_dev(dX, dB, dC, m, out=out)[1]
        plain = lambda: eng.update_codebooks_dev(dX, dB, m, out=out)[1]
        struct(), plain()                                                    # warm-up: buffers, code objects
        ts, tp = [], []
        for _ in range(a.repeat):
            ms, its = timed(struct)
            ts.append(ms)
            ms, itp = timed(plain)
            tp.append(ms)
        per_s, per_p = [t / its for t in ts], [t / itp for t in tp]
        rec = dict(kind="update", shape=name, n=n, d=d, m=m, repeat=a.repeat,
                   struct_dev_ms=round(float(np.median(ts)), 3), struct_iterations=its, struct_ms_per_iteration=round(float(np.median(per_s)), 4),
                   struct_ms_per_iteration_min_max=[round(min(per_s), 4), round(max(per_s), 4)],
                   unstruct_dev_ms=round(float(np.median(tp)), 3), unstruct_iterations=itp, unstruct_ms_per_iteration=round(float(np.median(per_p)), 4),
                   unstruct_ms_per_iteration_min_max=[round(min(per_p), 4), round(max(per_p), 4)])
        rec["struct_bytes_per_iteration_row_col"] = list(pass_bytes(n, d, m, dim2C))
        rec["unstruct_bytes_per_iteration_row_col"] = list(pass_bytes(n, d, m, None))
        Xj, Bj = np.ascontiguousarray(X.T), (codes.T.astype(np.int16) + 1)
        if not a.no_host:
            t0 = time.perf_counter()
            Ch = ini.update_codebooks_chain(Xj, Bj, H, solver="host", nthreads=16)
            rec["host_16_threads_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            Kh = np.concatenate([c.T for c in Ch], axis=0)
            rec["device_equals_host_bits"] = bool(np.array_equal(Kh.view(np.uint32), eng.update_codebooks_struct_dev(dX, dB, dC, m)[0].cpu().numpy().view(np.uint32)))
        if not a.no_scipy:
            t0 = time.perf_counter()
            ini.update_codebooks_chain(Xj, Bj, H)
            rec["scipy_default_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        emit(rec, a.out)
        del dX, dB, dC, out
    eng.close()


def mode_train(a):
    import torch
    eng = lsq.Engine(0)
    for name in a.shapes.split(","):
        n, d, m = SHAPES[name]
        X = np.ascontiguousarray(eng.synth_data_u8_dev(1, n, d).cpu().numpy().T)          # d x n, SIFT-like
        _, B0, R0, _ = ini.train_opq(X, m, H, 1, "natural", engine=eng)
        dX = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
        dB0 = torch.from_numpy(np.ascontiguousarray((B0.T - 1).astype(np.uint8))).cuda()
        spent = {"host": 0.0, "dev": 0.0}
        iters = []
        orig_chain, orig_dev = ini.update_codebooks_chain, eng.update_codebooks_struct_dev

        def chain_timed(*args, **kw):
            t0 = time.perf_counter()
            r = orig_chain(*args, **kw)
            spent["host"] += time.perf_counter() - t0
            return r

        def dev_timed(*args, **kw):
            ms, r = timed(lambda: orig_dev(*args, **kw))
            spent["dev"] += ms * 1e-3
            iters.append(r[1])
            return r

        ini.train_chainq_dev(dX, m, H, R0, dB0, 1, engine=eng)                # warm-up
        eng.update_codebooks_struct_dev = dev_timed
        ms_dev, res_dev = timed(lambda: ini.train_chainq_dev(dX, m, H, R0, dB0, a.niter, engine=eng))
        eng.update_codebooks_struct_dev = orig_dev
        ini.update_codebooks_chain = chain_timed
        t0 = time.perf_counter()
        res_host = ini.train_chainq(X, m, H, R0, B0, None, a.niter, engine=eng)
        ms_host = (time.perf_counter() - t0) * 1e3
        ini.update_codebooks_chain = orig_chain
        emit(dict(kind="train", shape=name, n=n, d=d, m=m, niter=a.niter,
                  train_chainq_default_ms=round(ms_host, 1), default_update_share=round(spent["host"] * 1e3 / ms_host, 4),
                  train_chainq_dev_ms=round(ms_dev, 1), dev_update_share=round(spent["dev"] * 1e3 / ms_dev, 4),
                  dev_update_iterations=iters, obj_default=[float(x) for x in res_host[3]], obj_dev=[float(x) for x in res_dev[3]]), a.out)
        del dX, dB0
    eng.close()


def mode_calls(a):
    import torch
    eng = lsq.Engine(0)
    for name in a.shapes.split(","):
        n, d, m = SHAPES[name]
        X, codes, dim2C = chain_problem(n, d, m)
        dX, dB, dC = torch.from_numpy(X).cuda(), torch.from_numpy(codes).cuda(), torch.from_numpy(dim2C).cuda()
        for _ in range(3):
            _, its = eng.update_codebooks_struct_dev(dX, dB, dC, m)
            _, itp = eng.update_codebooks_dev(dX, dB, m)
        torch.cuda.synchronize()
        print(json.dumps(dict(kind="calls", shape=name, struct_iterations=its, unstruct_iterations=itp)))
    eng.close()


def mode_passes(a):
    """kernel times of a `calls` run under rocprofv3 --kernel-trace --stats -> achieved bytes/s of the two passes (one shape per trace)"""
    name = a.shapes.split(",")[0]
    n, d, m = SHAPES[name]
    _, _, dim2C = chain_problem(min(n, 512), d, m)
    rows = list(csv.DictReader(open(a.stats)))
    avg = {}
    for r in rows:
        nm = r.get("Name") or r.get("KernelName") or ""
        for key in ("lsqr_u_update<true>", "lsqr_u_update<false>", "lsqr_v_update<true>", "lsqr_v_update<false>"):
            tag = key.replace("<true>", "ILb1E").replace("<false>", "ILb0E")
            if key in nm or tag in nm:
                avg[key] = float(r["AverageNs"])
                avg[key + " calls"] = int(r["Calls"])
    rec = dict(kind="passes", shape=name, n=n, d=d, m=m, source="rocprofv3 --kernel-trace --stats, average over all launches (the first pass of a call included)")
    for label, cover in (("struct", dim2C), ("unstruct", None)):
        rb, cb = pass_bytes(n, d, m, cover)
        t = "<true>" if cover is not None else "<false>"
        for pname, b, k in (("row", rb, "lsqr_u_update" + t), ("column", cb, "lsqr_v_update" + t)):
            if k in avg:
                rec["%s_%s_pass" % (label, pname)] = dict(bytes=b, avg_us=round(avg[k] / 1e3, 2), launches=avg[k + " calls"], TBps=round(b / avg[k] / 1e3, 3),
                                                         share_of_8TBps=round(b / (avg[k] * 1e-9) / HBM_PEAK, 4))
            else:
                rec["%s_%s_pass" % (label, pname)] = "not measured"
    emit(rec, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["update", "train", "calls", "passes"])
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    if a.shapes is None:
        a.shapes = {"update": "demo,1e5,d960", "train": "demo,1e5", "calls": "1e5", "passes": "1e5"}[a.mode]
    {"update": mode_update, "train": mode_train, "calls": mode_calls, "passes": mode_passes}[a.mode](a)


if __name__ == "__main__":
    main()
