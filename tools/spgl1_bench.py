"""Times the SPGL1 codebook update on the device (lsq_update_codebooks_spgl1_dev) and prints one JSON line per shape: iterations, line-search
trials, ms per call and per iteration, algorithmic bytes per iteration and the rate they imply.

    python tools/spgl1_bench.py [--out profiles/spgl1.jsonl] [--max-iter K] [--shapes demo,1e5,1e6,d960]

Data: SIFT-like seeded integers and uniform codes made on the device; tau = 0.7 ||K_pq||_1 (the demo's SLSQ1 setting, K_pq = sub-space means of
the codes' rows), S = d h.  Algorithmic bytes of one iteration with one line-search trial: residual pass (X 4 nd, r 8 nd, codes n m), gradient
(r 8 n m d through the sorted rows, keys 8 n m), projection (vkeys 32 N, sort 2 x 8 passes x 16 N, tiles and scan 24 N, apply 40 N) and the BB
pass 32 N, N = m h d."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lsq = importlib.import_module("local-search-quantization_amd")

SHAPES = {"demo": (10_000, 128, 7), "1e5": (100_000, 128, 8), "1e6": (1_000_000, 128, 8), "d960": (100_000, 960, 8)}


def pq_l1(X, codes, m, h=256):
    import torch
    n, d = X.shape
    bounds = np.linspace(0, d, m + 1).astype(int)
    tot = 0.0
    for j in range(m):
        lo, hi = bounds[j], bounds[j + 1]
        idx = codes[:, j].long()
        cnt = torch.zeros(h, dtype=torch.float64, device=X.device).index_add_(0, idx, torch.ones(n, dtype=torch.float64, device=X.device))
        s = torch.zeros((h, hi - lo), dtype=torch.float64, device=X.device).index_add_(0, idx, X[:, lo:hi].double())
        used = cnt > 0
        tot += float((s[used] / cnt[used, None]).abs().sum())
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--max-iter", type=int, default=2000)
    ap.add_argument("--shapes", default="demo,1e5,1e6,d960")
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args()
    import torch
    eng = lsq.Engine(0)
    for name in a.shapes.split(","):
        n, d, m = SHAPES[name]
        h = 256
        dX = eng.synth_data_u8_dev(1, n, d)
        dc = eng.randinit_dev(2, n, m)
        torch.cuda.synchronize()
        tau, S = 0.7 * pq_l1(dX, dc, m), d * h
        eng.update_codebooks_spgl1_dev(dX, dc, m, tau, S=S, max_iter=2)          # warm-up: buffers, code objects
        torch.cuda.synchronize()
        best = None
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            dK, info = eng.update_codebooks_spgl1_dev(dX, dc, m, tau, S=S, max_iter=a.max_iter)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            best = ms if best is None else min(best, ms)
        N, nd = m * h * d, n * d
        bytes_iter = (4 * nd + 8 * nd + n * m) + (8 * nd * m + 8 * n * m) + (32 * N + 2 * 8 * 16 * N + 24 * N + 40 * N) + 32 * N
        it = max(1, info["iterations"])
        rec = dict(shape=name, n=n, d=d, m=m, tau=tau, S=S, status=info["status"], iterations=info["iterations"],
                   line_search_trials=info["line_search_trials"], rel_gap=info["rel_gap"], nnz_before=info["nnz_before_threshold"], nnz=info["nnz"],
                   ms_per_call=round(best, 3), ms_per_iteration=round(best / it, 4), bytes_per_iteration=int(bytes_iter),
                   achieved_GBps=round(bytes_iter / (best / it * 1e-3) / 1e9, 1))
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del dX, dc, dK
    eng.close()


if __name__ == "__main__":
    main()
