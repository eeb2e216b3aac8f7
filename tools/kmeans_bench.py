"""Times the device cluster means, the device k-means++ seeding and the resident PQ / OPQ trainers; one JSON line per measurement.

    python tools/kmeans_bench.py kernels [--shapes 1e5_128_8,...] [--repeat 5] [--out profiles/kmeans_dev.jsonl]
    python tools/kmeans_bench.py train   [--repeat 3] [--niter 10] [--out ...]
    python tools/kmeans_bench.py host    [--out ...]                     # the host steps the resident trainers replace, on this machine's CPUs
    python tools/kmeans_bench.py calls   [--shapes 1e5_128_8]            # a few means calls and one seeding, to be run under rocprofv3 --kernel-trace --stats
    python tools/kmeans_bench.py stats   --stats <kernel_stats.csv> [--trace <kernel_trace.csv>] [--shapes 1e5_128_8] [--out ...]

kernels: per shape one warm-up, then `repeat` timed calls between device events (lsq_update_centers_dev; lsq_kmeanspp_seed_dev as a whole, 255 steps).
         SIFT-like data and uniform codes made on the device.  The streaming bound of one seeding step is (4 n d + 8 n m) bytes -- X once, d2 read and
         written -- over the measured HBM copy rate of the MI355X (6.29 TB/s).
train:   train_pq_dev against train_pq and train_opq_dev against train_opq at 10^5 x 128, m = 8, in one process, alternated, after a warm-up of both;
         host clock around a device synchronise; every repeat listed.
stats:   kernel times of a `calls` run: the means call split into its sort (keys, radix sort, segments) and its walk; the seeding's two kernels; with
         --trace also the gaps between consecutive kernels of the seeding."""
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
HBM_MEASURED = 6.29e12
DEFAULT_SHAPES = "1e5_128_8,1e5_128_16,1e5_960_8,1e5_960_16,1e6_128_8,1e6_128_16,1e6_960_8,1e6_960_16"


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def shape_of(name):
    n, d, m = name.split("_")
    return int(float(n)), int(d), int(m)


def pq_cover(d, m):
    return ini._cover_map(ini._subdims(d, m), d, m)


def event_ms(fn, repeat):
    import torch
    out = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def mode_kernels(a):
    import torch
    eng = lsq.Engine(0)
    for name in a.shapes.split(","):
        n, d, m = shape_of(name)
        dX = eng.synth_data_u8_dev(1, n, d)
        dB = eng.randinit_dev(2, n, m)
        cover = pq_cover(d, m)
        u = np.random.default_rng(3).random((m, H))
        out = torch.empty((m * H, d), dtype=torch.float32, device=dX.device)
        cnt = torch.empty(m * H, dtype=torch.int32, device=dX.device)
        means = lambda: eng.update_centers_dev(dX, dB, cover, m, out=out, counts=cnt)
        seed = lambda: eng.kmeanspp_seed_dev(dX, cover, u, m, want_idx=False, out=out)
        means(), seed()
        torch.cuda.synchronize()
        tm, ts = event_ms(means, a.repeat), event_ms(seed, a.repeat)
        step_bytes = 4 * n * d + 8 * n * m
        step_ms = float(np.median(ts)) / (H - 1)
        emit(dict(kind="kernels", shape=name, n=n, d=d, m=m, repeat=a.repeat,
                  means_ms=round(float(np.median(tm)), 4), means_ms_min_max=[round(min(tm), 4), round(max(tm), 4)],
                  means_bytes_of_X=4 * n * d, means_TBps_of_X=round(4 * n * d / (float(np.median(tm)) * 1e-3) / 1e12, 3),
                  seeding_ms=round(float(np.median(ts)), 3), seeding_ms_min_max=[round(min(ts), 3), round(max(ts), 3)],
                  seeding_step_ms=round(step_ms, 5), seeding_step_bytes=step_bytes, seeding_step_bound_ms=round(step_bytes / HBM_MEASURED * 1e3, 5),
                  seeding_step_share_of_bound=round(step_bytes / HBM_MEASURED * 1e3 / step_ms, 4)), a.out)
        del dX, dB, out, cnt
        torch.cuda.empty_cache()
    eng.close()


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def mode_train(a):
    import torch
    n, d, m = shape_of(a.shapes.split(",")[0]) if a.shapes else (100_000, 128, 8)
    eng = lsq.Engine(0)
    dX = eng.synth_data_u8_dev(1, n, d)
    X = np.ascontiguousarray(dX.cpu().numpy().T)                       # d x n for the host trainers
    pq_dev = lambda: ini.train_pq_dev(dX, m, H, seed=0, engine=eng)
    pq_host = lambda: ini.train_pq(X, m, H, seed=0, engine=eng)
    opq_dev = lambda: ini.train_opq_dev(dX, m, H, a.niter, "natural", seed=0, engine=eng)
    opq_host = lambda: ini.train_opq(X, m, H, a.niter, "natural", seed=0, engine=eng)
    ini.train_opq_dev(dX, m, H, 1, "natural", seed=0, engine=eng)       # warm-up: code objects, buffers, BLAS
    ini.train_opq(X[:, :4096], m, H, 1, "natural", seed=0, engine=eng)
    ini.train_pq_dev(dX[:4096].contiguous(), m, H, seed=0, engine=eng)
    for label, dev, host in (("train_pq", pq_dev, pq_host), ("train_opq", opq_dev, opq_host)):
        td, th = [], []
        for _ in range(a.repeat):
            ms, rd = wall_ms(dev)
            td.append(round(ms, 1))
            ms, rh = wall_ms(host)
            th.append(round(ms, 1))
        rec = dict(kind="train", trainer=label, n=n, d=d, m=m, repeat=a.repeat, dev_ms=td, host_ms=th, dev_ms_median=float(np.median(td)),
                   host_ms_median=float(np.median(th)), host_over_dev=round(float(np.median(th) / np.median(td)), 1))
        if label == "train_opq":
            rec.update(niter=a.niter, obj_dev=[float(x) for x in rd[3]], obj_host=[float(x) for x in rh[3]])
        else:
            rec.update(err_dev=float(rd[2]), err_host=float(rh[2]))
        emit(rec, a.out)
    eng.close()


def mode_host(a):
    """the host steps of train_pq / train_opq at 10^5 x 128, m = 8, h = 256 on the CPUs of the machine this runs on"""
    n, d, m = 100_000, 128, 8
    rng = np.random.default_rng(0)
    X = rng.integers(0, 256, size=(d, n)).astype(np.float32)
    B = rng.integers(0, H, size=(m, n))
    sd = ini._subdims(d, m)
    C = [X[sd[i]][:, :H].copy() for i in range(m)]

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return round(time.perf_counter() - t0, 3)

    def seeding():
        Xs = X[sd[0]]
        c = Xs[:, :1]
        d2 = ((Xs - c) ** 2).sum(axis=0)
        for k in range(1, H):
            idx = int(np.searchsorted(np.cumsum(d2), 0.5 * float(d2.sum())))
            d2 = np.minimum(d2, ((Xs - Xs[:, idx:idx + 1]) ** 2).sum(axis=0))

    CB = np.zeros_like(X)
    for i in range(m):
        CB[sd[i]] = C[i][:, B[i]]
    R = np.eye(d, dtype=np.float32)
    emit(dict(kind="host", n=n, d=d, m=m, cpus=os.cpu_count(), threads_env=os.environ.get("OMP_NUM_THREADS"),
              cluster_means_all_subspaces_s=clock(lambda: [ini._centers(X[sd[i]], B[i], H, rng, old=C[i]) for i in range(m)]),
              procrustes_and_rotation_s=clock(lambda: ini._procrustes(X, CB).T @ X),
              objective_s=clock(lambda: float(((R @ CB - X) ** 2).sum())),
              kmeanspp_seeding_one_subspace_s=clock(seeding)), a.out)


def mode_calls(a):
    import torch
    eng = lsq.Engine(0)
    n, d, m = shape_of(a.shapes.split(",")[0])
    dX, dB = eng.synth_data_u8_dev(1, n, d), eng.randinit_dev(2, n, m)
    cover = pq_cover(d, m)
    u = np.random.default_rng(3).random((m, H))
    for _ in range(5):
        eng.update_centers_dev(dX, dB, cover, m)
    for _ in range(2):
        eng.kmeanspp_seed_dev(dX, cover, u, m, want_idx=False)
    torch.cuda.synchronize()
    print(json.dumps(dict(kind="calls", n=n, d=d, m=m, means_calls=5, seeding_calls=2)))
    eng.close()


def mode_stats(a):
    n, d, m = shape_of(a.shapes.split(",")[0])
    groups = {"means_walk": ("kmeans_centers_walk",), "means_sort": ("lsqr_make_keys", "lsqr_segments", "rocprim", "hipcub"),
              "seeding_dist": ("kpp_dist",), "seeding_locate": ("kpp_locate",)}
    tot, calls = {k: 0.0 for k in groups}, {k: 0 for k in groups}
    for r in csv.DictReader(open(a.stats)):
        nm = r.get("Name") or r.get("KernelName") or ""
        for g, keys in groups.items():
            if any(k in nm for k in keys):
                tot[g] += float(r["TotalDurationNs"])
                calls[g] += int(r["Calls"])
                break
    rec = dict(kind="kernel_stats", n=n, d=d, m=m, source="rocprofv3 --kernel-trace --stats of `kmeans_bench.py calls` (5 means calls, 2 seedings)")
    rec["means_walk_us_per_call"] = round(tot["means_walk"] / 5 / 1e3, 2) if calls["means_walk"] else "not measured"
    rec["means_sort_us_per_call"] = round(tot["means_sort"] / 5 / 1e3, 2) if calls["means_sort"] else "not measured"
    for g in ("seeding_dist", "seeding_locate"):
        rec[g + "_us_avg"] = round(tot[g] / calls[g] / 1e3, 2) if calls[g] else "not measured"
        rec[g + "_launches"] = calls[g]
    if calls["seeding_dist"]:
        b = 4 * n * d + 8 * n * m
        rec["seeding_dist_TBps"] = round(b / (tot["seeding_dist"] / calls["seeding_dist"]) / 1e3, 3)
        rec["seeding_dist_share_of_6.29TBps"] = round(b / (tot["seeding_dist"] / calls["seeding_dist"] * 1e-9) / HBM_MEASURED, 4)
    if a.trace:
        ev = []
        for r in csv.DictReader(open(a.trace)):
            nm = r.get("Kernel_Name") or r.get("Name") or ""
            if "kpp_" in nm:
                ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
        ev.sort()
        gaps = [b0 - a1 for (a0, a1), (b0, b1) in zip(ev, ev[1:]) if 0 <= b0 - a1 < 1_000_000]
        if gaps:
            rec["seeding_gap_us_median"] = round(float(np.median(gaps)) / 1e3, 2)
            rec["seeding_gap_us_total_per_seeding"] = round(float(np.sum(gaps)) / 2 / 1e3, 1)
    emit(rec, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "train", "host", "calls", "stats"])
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--repeat", type=int, default=None)
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--trace", default=None)
    a = ap.parse_args()
    if a.shapes is None:
        a.shapes = {"kernels": DEFAULT_SHAPES, "train": "1e5_128_8", "host": "", "calls": "1e5_128_8", "stats": "1e5_128_8"}[a.mode]
    if a.repeat is None:
        a.repeat = 3 if a.mode == "train" else 5
    {"kernels": mode_kernels, "train": mode_train, "host": mode_host, "calls": mode_calls, "stats": mode_stats}[a.mode](a)


if __name__ == "__main__":
    main()
